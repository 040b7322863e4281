"""-m gpu: the real-time synthesis (rt.cpp; k_rt_hop2, k_rt_hop, k_rt_front, k_rt_back, k_rt_rings, k_rt_excite, k_rt_mix,
k_rt_template, rt_stage_rows) held to the float64 oracle's restatement of llsmrt.c SAMPLE BY SAMPLE, on the synthetic cases
of tests/rt_reference.py: more than 256 harmonics (the second trip of rt_stage_rows), more than 1024 PSD points, more
harmonics than the transform has points (the clamp of rt.cpp / llsmrt.c:280), eight bands with eight envelope harmonics,
synthesis below the analysed rate (bands at and across the synthesis Nyquist), one band without envelope harmonics, frames
on either side of the -100 dB gate, voiced frames without harmonics, a stream that starts voiced -- each in the form
(RT_HOP_CHIP / RT_HOP_ONE / RT_HOP_TWO) that rt_reference.CASES writes beside it (the library has no public way to read the
launch counts of a real-time buffer, which lives on the library's own context: the form is derived from rt_hop_form's
conditions in tests/test_rt_reference_host.py, not read back here).

Bounds (rt_reference.rt_violations; tests/test_rt_reference_host.py shows every fault of rt_reference.FAULTS flagged under them):
  ysin_local <= max(60, the float32 oracle's value on the case)   60: gpu_common.SYN_CEILING, the same device function synth_frame;
                                                                  the float32 oracle: KAPPA_F32 = 1, where K or the window
                                                                  exceed what the 60 was calibrated on
  ysin_nonzero_uncovered == 0
  ynoise_local <= 6e-5                                            gpu_common.SYN_CEILING: the same noise_filter_pair
The pulse-by-pulse path (use_l1 = 1) needs a scale built from pulses and is not covered here (LAB.md)."""
import numpy as np
import pytest

import libllsm2_amd as llsm
import rt_reference as R
from gpu_common import report
from test_gpu_rt import _group_run, chunk_from_oracle, rt_run, synced

pytestmark = pytest.mark.gpu


def case_chunk(L, name):
    """the case's rows as a product chunk; only make_soptions(fs) knows the synthesis rate"""
    fs, pr, seed = R.rt_case(name)
    c = R.CASES[name]
    kw = dict(f0_refine=0, thop=pr.thop, npsd=pr.npsd, maxnhar=pr.maxnhar, maxnhar_e=pr.maxnhar_e, nchannel=pr.nchannel)
    if pr.nchannel > 1:
        kw["chanfreq"] = list(pr.chanfreq)
    else:
        kw["chanfreq"] = []
    ao = llsm.make_aoptions(**kw)
    return chunk_from_oracle(L, ao, pr, c["fs_ana"]), llsm.make_soptions(fs), pr, seed


def judge(name, tag, o64, o32, yp, yap, lat, seed_offset=0):
    fs, pr, _seed = R.rt_case(name)
    sched, S, m32 = R.case_yardsticks(o64, synced(o32), name)
    ypo, yapo, lato = R.oracle_streams(o64, name, seed_offset)
    assert lat == lato == sched["latency"] and len(yp) == len(yap) == len(ypo) == sched["n"], (name, tag, lat, lato, len(yp), len(ypo))
    m = R.rt_metrics(pr, sched, yp, ypo, yap, yapo, S)
    m["ysin_local_f32_oracle"] = m32["ysin_local"]; m["latency"] = lat; m["n"] = len(yp); m["form"] = R.CASES[name]["form"]
    report("rt_samples_%s%s" % (name, tag), m)
    bad = R.rt_violations(m, m32["ysin_local"])
    assert not bad, (name, tag, bad)
    return m


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_rt_case_sample_by_sample(o64, o32, name):
    """one buffer, the default launch mode, drained after every feed"""
    L = llsm.load()
    ch, so, pr, seed = case_chunk(L, name)
    try:
        L.llsm_gpu_set_default_seed(seed)
        yp, yap, lat = rt_run(L, so, ch, pr.nfrm)
    finally:
        L.llsm_delete_chunk(ch)
    assert np.sqrt(np.mean(yp ** 2)) > 1e-3 and np.sqrt(np.mean(yap ** 2)) > 0
    judge(name, "", o64, o32, yp, yap, lat)


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_rt_case_launch_modes(o64, o32, name):
    """the same stream under llsm_gpu_rt_fused 0, 1, 2 and 3: the harmonic part bit-identical in all four, the noise part
    bit-identical in 1, 2 and 3, and mode 0 (five launches: another float32 rounding of the noise part) held to the oracle
    by the same ynoise_local bound"""
    L = llsm.load()
    ch, so, pr, seed = case_chunk(L, name)
    prev_f, prev_d = L.llsm_gpu_rt_fused(-1), L.llsm_gpu_rt_direct(-1)
    runs = {}
    try:
        for mode in (0, 1, 2, 3):
            L.llsm_gpu_rt_fused(mode)
            L.llsm_gpu_set_default_seed(seed)
            runs[mode] = rt_run(L, so, ch, pr.nfrm)
    finally:
        L.llsm_gpu_rt_fused(prev_f); L.llsm_gpu_rt_direct(prev_d)
        L.llsm_delete_chunk(ch)
    for mode in (0, 2, 3):
        assert runs[mode][2] == runs[1][2] and len(runs[mode][0]) == len(runs[1][0])
        assert np.array_equal(runs[mode][0], runs[1][0]), (name, mode)
        if mode:
            assert np.array_equal(runs[mode][1], runs[1][1]), (name, mode)
    judge(name, "_mode0", o64, o32, *runs[0])
    judge(name, "_mode1", o64, o32, *runs[1])


@pytest.mark.parametrize("name,S", [("bench", 3), ("k400", 2)])
def test_rt_group_against_oracle(o64, o32, name, S):
    """S streams of a case fed in lock-step and pulled 256 samples at a time; stream s against the oracle run of seed + s
    (the pair partner in the complex transform changes a stream's noise rounding: the oracle is the arbiter, not the
    single-stream run).  Three streams leave the last transform pair half empty; two streams of k400 put more than 256
    harmonics into both halves of one workgroup."""
    L = llsm.load()
    ch, so, pr, seed = case_chunk(L, name)
    try:
        outp, outap = _group_run(L, so, [ch] * S, pr.nfrm, seed)
    finally:
        L.llsm_delete_chunk(ch)
    lat = R.oracle_streams(o64, name)[2]
    for s in range(S):
        judge(name, "_group%d_of_%d" % (s, S), o64, o32, outp[s], outap[s], lat, seed_offset=s)
        assert np.array_equal(outp[s], outp[0])                # the same rows: the same harmonic part
