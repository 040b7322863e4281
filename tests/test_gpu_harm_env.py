"""-m gpu: k_harm_env on ITS OWN input plane against float64, value by value.

The whole-chain parity bounds on the band energies and the envelope harmonics (tests/gpu_common.py: edc 1e-4 relative,
lifted by two yardsticks up to 1e-3; envelope harmonics 1e-4 of the utterance's largest amplitude and 1e-3 rad) are
bounds on  x -> harmonic analysis -> residual -> Chebyshev filtfilt -> square -> k_harm_env,  whose filter is
ill-conditioned for low band edges.  The kernel after the plane is not: given the plane it reads (plane 2 of
llsm_gpu_batch_debug_plane, the pointer launch_harm_env is given), EDC, NHAR_E, EENV_AMPL and EENV_PHSE are determined to
float32 rounding.  So every value of those rows is held to harm_env_ref(float64) of the DOWNLOADED plane under
harm_env_check (tests/harm_env_reference.py, whose docstring carries the metric, the bounds 4 Y + 4 EPS / 4 Y + 2 EPS
and the derivation of the additive terms; proven against the oracle by tests/test_harm_env_host.py).  Plane 2 is an
input here and is never judged (tests/test_gpu_filtfilt_samples.py does that).

The configurations are the smallest that reach every instantiation and branch of the kernel: <4,4>, <4,8> and <8,8>
(the lane-0 reduction), one live channel of four register rows, maxnhar_e = 0, K < maxnhar_e (the live cut), windows of
a single trip and of 23, the mean riding along the main loop and in its own pass (rel_winsize 2 and 1.5: the first time a
kernel of the tree sees that option off its default), HMPP (edc and nhar_e only: the envelope rows are peak-picked by
another kernel).  The utterances: harm_env_reference.harm_env_inputs.  Every batch is first analysed on another signal
of ten times the level, and the utterances shorter than their windows sit between neighbours of ten times their level:
a sample read across an utterance boundary, or a row left unwritten, lands far outside the bound.

The additive terms are what the float32 yardstick Y does not contain.  A harmonic: the store of an amplitude a (half an
ulp: EPS a) and of an angle of magnitude up to pi (half an ulp: pi EPS / 2 radians, which moves the complex value by that
times a), together below 2.1 EPS a <= 2.1 EPS A0; the rest of the 4 EPS is sqrtf and atan2f.  The mean: one division and
one store, 2 EPS.  No bound is calibrated on the kernel, and none may exceed 2e-5 (harmonics) / 1e-5 (mean): an input whose
yardstick lifts it higher fails as "cap_z" / "cap_d" and is to be replaced.

What the kernel measures against these bounds: the table in DESIGN.md section 8."""
import numpy as np
import pytest

import libllsm2_amd as llsm
from gpu_common import report
from harm_env_reference import (CONFIGS, HMPP, I_CLIPPED, I_LOW, I_SPEECH, I_ZERO, NAMES, REL_CONFIGS, config_options, frame_index,
                                harm_env_check, harm_env_inputs, loud_inputs, offsets, plan_values)

pytestmark = pytest.mark.gpu


def run_batch(ctx, cid, xs, f0s, stale_first=True):
    """one batch: analysed on the loud signal, then on xs with profiling on; the rows and plane 2 downloaded"""
    fs, thop, opt = config_options(cid)
    ao = llsm.make_aoptions(f0_refine=0, thop=thop, **opt)
    b = llsm.Batch(ctx, ao, fs, [len(x) for x in xs], [len(f) for f in f0s])
    try:
        b.upload(llsm.A_F0, np.concatenate(f0s))
        if stale_first:
            b.upload(llsm.A_X, np.concatenate(loud_inputs(xs)))
            b.analyze()
        b.upload(llsm.A_X, np.concatenate(xs))
        ctx.set_profiling(True); ctx.reset_profile()
        try:
            b.analyze(); ctx.sync()
            prof = ctx.profile()
        finally:
            ctx.set_profiling(False)
        F, nch, me = sum(len(f) for f in f0s), opt["nchannel"], opt["maxnhar_e"]
        ce = b.debug_plane(2).reshape(nch, -1)
        assert ce.shape[1] == b.layout.total_samples == sum(len(x) for x in xs)
        assert np.array_equal(b.x_off, offsets(xs)) and np.array_equal(b.frm_off, offsets(f0s))
        assert np.array_equal(b.download(llsm.A_F0), np.concatenate(f0s))                    # (f0_refine = 0: F0 is an input)
        return dict(prof=prof, ce=ce, nx_off=offsets(xs), frm_off=offsets(f0s), f0=np.concatenate(f0s), fs=fs, thop=thop, opt=opt,
                    edc=b.download(llsm.A_EDC).reshape(F, nch), nhar_e=b.download(llsm.A_NHAR_E),
                    ampl=b.download(llsm.A_EENV_AMPL).reshape(F, nch, max(me, 1)),
                    phse=b.download(llsm.A_EENV_PHSE).reshape(F, nch, max(me, 1)))
    finally:
        b.close()


@pytest.fixture(scope="module")
def ctx():
    c = llsm.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def runs(ctx):
    """one batch per configuration, analysed once and shared"""
    cache = {}

    def get(cid):
        if cid not in cache:
            xs, f0s = harm_env_inputs(cid)
            cache[cid] = run_batch(ctx, cid, xs, f0s)
        return cache[cid]
    return get


def _judge(cid, r):
    opt = r["opt"]
    me, rel = opt["maxnhar_e"], opt["rel_winsize"]
    assert r["prof"].get("k_harm_env", (0, 0))[1] >= 1, (cid, sorted(r["prof"]))
    assert np.all(np.isfinite(r["ce"]))                          # (an input: only that the reference can be formed)
    judge_env = opt["hm_method"] != HMPP and me > 0
    got = (r["nhar_e"], r["ampl"][:, :, :me] if me > 0 else None, r["phse"][:, :, :me] if me > 0 else None, r["edc"])
    bad, st = harm_env_check(got, r["ce"], r["nx_off"], r["frm_off"], r["f0"], r["thop"], r["fs"], rel, me, judge_env=judge_env)
    for rec in st["utterances"]:
        rec["name"] = NAMES[rec["utt"]]
        print("harm_env %-12s %-9s Y_Z %.3g Y_D %.3g  eZ %.3g (%.2f of its bound) at %s  eD %.3g (%.2f) at %s" % (
            cid, rec["name"], rec["Y_Z"], rec["Y_D"], rec["eZ"], rec["ratio_z"], rec["eZ_at"], rec["eD"], rec["ratio_d"], rec["eD_at"]))
    report("harm_env_stage_" + cid, st)
    # the branches the configuration is there for, from the frames it holds
    utt, idx = frame_index(r["frm_off"])
    c0, n, K, ndc = plan_values(r["f0"], idx, r["thop"], r["fs"], rel, me)
    v = r["f0"] > 0
    assert {int(a) % 2 for a in ndc[v]} == {0, 1}
    assert {int(o) % 4 for o in r["nx_off"][:-1]} == {0, 1, 2, 3}
    # the all-zero utterance: every row exactly 0 and finite (HMPP's residual of silence is not silence: not there)
    z = slice(int(r["frm_off"][I_ZERO]), int(r["frm_off"][I_ZERO + 1]))
    if opt["hm_method"] != HMPP:
        assert not r["ce"][:, int(r["nx_off"][I_ZERO]):int(r["nx_off"][I_ZERO + 1])].any()
        assert not r["edc"][z].any() and not r["ampl"][z, :, :me].any() and not r["phse"][z, :, :me].any()
        assert np.array_equal(r["nhar_e"][z], K[z])
    assert not bad, (cid, bad[:8], {k: st[k] for k in st if k != "utterances"})
    return st


@pytest.mark.parametrize("cid", [c for c in CONFIGS if c not in REL_CONFIGS])
def test_harm_env_on_its_own_plane(runs, cid):
    """EDC, NHAR_E, EENV_AMPL, EENV_PHSE of every frame against float64 of the downloaded plane: nothing excluded, no
    share allowed to miss."""
    _judge(cid, runs(cid))


@pytest.mark.parametrize("cid", REL_CONFIGS)
def test_harm_env_rel_winsize_off_default(runs, cid):
    """rel_winsize 2 (n and ndc differ by rounding: the mean's window is inside the analysis window for some F0 and one
    sample outside for others) and 1.5 (never inside): the voiced frames' mean in its own pass."""
    r = runs(cid)
    utt, idx = frame_index(r["frm_off"])
    c0, n, K, ndc = plan_values(r["f0"], idx, r["thop"], r["fs"], r["opt"]["rel_winsize"], r["opt"]["maxnhar_e"])
    v = r["f0"] > 0
    inside = v & (c0 - ndc // 2 >= c0 - n // 2) & (c0 - ndc // 2 + ndc <= c0 - n // 2 + n)
    assert np.any(v & ~inside)
    if cid == "44k_rel2":
        assert np.any(inside)
    _judge(cid, r)


def test_bits_do_not_depend_on_neighbours(ctx, runs):
    """No tolerance.  The utterance order reversed, and the 30 Hz utterance, the clipped one and a make_speechlike one each
    alone: the bits of edc, nhar_e, eenv_ampl and eenv_phse of an utterance are the same in all three arrangements (which
    block of the grid a frame is, the alignment of its samples and what lies beyond its utterance's ends all change)."""
    cid = "44k_default"
    r = runs(cid)
    xs, f0s = harm_env_inputs(cid)
    nu = len(xs)

    def rows(res, k):
        f = slice(int(res["frm_off"][k]), int(res["frm_off"][k + 1]))
        s = slice(int(res["nx_off"][k]), int(res["nx_off"][k + 1]))
        return dict(plane2=res["ce"][:, s].view(np.int32), edc=res["edc"][f].view(np.int32), nhar_e=res["nhar_e"][f],
                    eenv_ampl=res["ampl"][f].view(np.int32), eenv_phse=res["phse"][f].view(np.int32))

    def same(a, b_, how):
        if not np.array_equal(a["plane2"], b_["plane2"]):
            pytest.fail("%s: plane 2 (the kernel's INPUT) differs in %d samples: the finding belongs to the band filter "
                        "(k_filtfilt), not to k_harm_env" % (how, int(np.count_nonzero(a["plane2"] != b_["plane2"]))))
        for name in ("edc", "nhar_e", "eenv_ampl", "eenv_phse"):
            assert np.array_equal(a[name], b_[name]), (how, name, int(np.count_nonzero(a[name] != b_[name])))
    rev = run_batch(ctx, cid, xs[::-1], f0s[::-1])
    for k in range(nu):
        same(rows(r, k), rows(rev, nu - 1 - k), "reversed, utterance %d (%s)" % (k, NAMES[k]))
    for k in (I_LOW, I_CLIPPED, I_SPEECH):
        solo = run_batch(ctx, cid, [xs[k]], [f0s[k]], stale_first=False)
        same(rows(r, k), rows(solo, 0), "alone, utterance %d (%s)" % (k, NAMES[k]))
