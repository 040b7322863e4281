"""CPU-side preconditions of tests/test_gpu_invariance.py.

The fallback spectrogram cases there are only worth something while each pinned configuration really contains a frame
whose float64 DC or Nyquist spectrogram bin lies >= 110 dB under the bin of the frame's F0, and while the launcher's
size rule really sends it to the LDS kernel k_spgm_env rather than to the register-resident k_spgm_env_wf.  Both are
checked here, on the float64 oracle and on the product's own plan queries, so that an edit of a pinned constant cannot
quietly take the teeth out of the GPU test.  The time-segment rule of the zero-phase filter (llsm_gpu_plan_index case
13) is checked to be a function of the signal alone."""
import ctypes as C
import math

import numpy as np
import pytest

import libllsm2_amd as llsm
from conftest import make_speechlike

EDGE_DB = 110.0                 # the depth kernels.hip SPGM_EDGE_THRESH (12.7 nepers) stands for

# id: (fs, thop, analysis options, frame, which edge bin cancels).  Found by a float64 scan over make_speechlike seeds
# (96 kHz: 360 seeds of 0.4 s; the two deepest cancellations, one of each bin) and, for the short hop, seed 123208 of the
# fuzz matrix (tests/test_gpu_regressions.py) at a quarter of its hop with every F0 value repeated four times: frame
# 4 * 43 = 172 sits on sample 5504 with the F0 and window of the original frame 43.
FALLBACK_CASES = {
    "96k_nyquist": dict(fs=96000.0, thop=0.005, kw=dict(maxnhar=200), seed=269, nx=38400, frame=67, edge="nyquist"),
    "96k_dc": dict(fs=96000.0, thop=0.005, kw=dict(maxnhar=200), seed=358, nx=38400, frame=29, edge="dc"),
    "32k_hop1ms_fold8": dict(fuzz_seed=123208, hop_div=4, frame=172, edge="dc"),
}
# the register-resident path on the configuration its list-and-redo launch was made for: the yardstick of the envelope
# bound in test_gpu_invariance (fold 1, 1024 points)
WF_REFERENCE_CASE = dict(fuzz_seed=123208, hop_div=1, frame=43, edge="dc")


def case_signal(case):
    """(fs, thop, options, x, f0) of a pinned case"""
    if "fuzz_seed" in case:
        from test_gpu_regressions import _case
        fs, thop, kw, x, f0 = _case(case["fuzz_seed"])
        d = case["hop_div"]
        return fs, thop / d, kw, x, np.repeat(f0, d).astype(np.float32)
    x, f0 = make_speechlike(case["seed"], nx=case["nx"], fs=case["fs"], thop=case["thop"])
    return case["fs"], case["thop"], case["kw"], x, f0.astype(np.float32)


# (log2 N, log2 fold) of the register-resident spectrogram kernel's instantiations (kernels.hip launch_spgm_env)
WF_SHAPES = {(9, 0), (9, 1), (10, 0), (10, 1), (10, 2), (11, 0), (11, 1), (11, 2)}


def nextpow2(v):
    return int(2 ** math.ceil(math.log2(v)))


def spgm_sizes(fs, thop):
    """(nfft_spgm, nfft_psd) as engine.cpp llsm_gpu_create_batch derives them, through the product's own plan query"""
    L = llsm.load()
    nwin_psd = L.llsm_gpu_plan_index(4, 0, 0, 0.0, thop, fs, 0.0)
    return nextpow2(0.03 * fs), nextpow2(nwin_psd)


def takes_fallback(fs, thop):
    """kernels.hip launch_spgm_env: k_spgm_env_wf serves (logN, logF) = (9, 0 .. 1) and (10 .. 11, 0 .. 2), logF the log2 of
    the fold N / nfft_psd; every other shape takes k_spgm_env"""
    N, npsd = spgm_sizes(fs, thop)
    logN = int(round(math.log2(N)))
    if npsd > N:
        return True
    logF = int(round(math.log2(N // npsd)))
    return (logN, logF) not in WF_SHAPES


def oracle_stages(o, fs, thop, kw, x, f0, stages=(1, 2)):
    """run the oracle's analysis and return the arrays its stage hook passes for `stages` (oracle/llsm_oracle.c STAGE:
    1 the normalised spectrogram magnitudes [nfrm][nfft_spgm / 2 + 1], 2 the resampled log envelope [nfrm][nfft_psd / 2 + 1])"""
    from gpu_common import aopt_kwargs
    ao = llsm.make_aoptions(f0_refine=0, thop=thop, **kw)
    okw = aopt_kwargs(ao)
    if "chanfreq" in kw:
        okw["chanfreq"] = kw["chanfreq"]
    fpt = C.c_double if o.dtype == np.float64 else C.c_float
    HT = C.CFUNCTYPE(None, C.c_int, C.c_int, C.POINTER(fpt), C.c_long)
    got = {}

    def hook(stage, index, data, n):
        if stage in stages and index == 0:
            got[stage] = np.ctypeslib.as_array(data, shape=(n,)).astype(np.float64).reshape(len(f0), -1)
    cb = HT(hook)
    o.lib.o_set_stage_hook(cb)
    try:
        pr = o.analyze(o.aoptions(**okw), x, fs, f0)
    finally:
        o.lib.o_set_stage_hook(C.cast(None, HT))
    return got, pr


def edge_depth_db(spec_row, f0, fs, N):
    """(DC, Nyquist) bin of one spectrogram frame in dB against the bin of the frame's F0 (200 Hz when unvoiced), the
    yardstick of the product's detector"""
    k0 = min(63, max(1, int((f0 if f0 > 0 else 200.0) / fs * N + 0.5)))
    top = spec_row[k0]
    return 20 * np.log10(spec_row[0] / top + 1e-300), 20 * np.log10(spec_row[N // 2] / top + 1e-300)


@pytest.mark.parametrize("cid", sorted(FALLBACK_CASES))
def test_pinned_fallback_case_takes_the_lds_kernel(cid):
    fs, thop, kw, x, f0 = case_signal(FALLBACK_CASES[cid])
    assert takes_fallback(fs, thop), (cid, spgm_sizes(fs, thop))


def test_the_reference_case_takes_the_register_kernel():
    fs, thop, kw, x, f0 = case_signal(WF_REFERENCE_CASE)
    assert not takes_fallback(fs, thop), spgm_sizes(fs, thop)


def test_the_size_rule_itself():
    # 96 kHz: 4096-point spectrogram; 1 ms hop at 32 kHz: fold 8; 44.1 kHz with a 12 ms hop: PSD transform longer than it;
    # 16 kHz with a 2 ms hop: 512 points with a fold of 4 (no such instantiation); 8 kHz: 256 points
    assert spgm_sizes(16000.0, 0.002) == (512, 128)
    assert takes_fallback(96000.0, 0.005) and takes_fallback(88200.0, 0.005)
    assert takes_fallback(32000.0, 0.001) and takes_fallback(44100.0, 0.012)
    assert takes_fallback(16000.0, 0.002) and takes_fallback(8000.0, 0.005)
    assert not takes_fallback(44100.0, 0.005) and not takes_fallback(32000.0, 0.004) and not takes_fallback(16000.0, 0.005)


@pytest.mark.parametrize("cid", sorted(FALLBACK_CASES) + ["wf_reference"])
def test_pinned_case_cancels_in_float64(o64, cid):
    case = WF_REFERENCE_CASE if cid == "wf_reference" else FALLBACK_CASES[cid]
    fs, thop, kw, x, f0 = case_signal(case)
    got, _ = oracle_stages(o64, fs, thop, kw, x, f0, stages=(1,))
    N, _ = spgm_sizes(fs, thop)
    spec = got[1]
    assert spec.shape == (len(f0), N // 2 + 1)
    g = case["frame"]
    assert f0[g] > 0, "the pinned frame is voiced"
    dc, ny = edge_depth_db(spec[g], float(f0[g]), fs, N)
    depth = dc if case["edge"] == "dc" else ny
    assert depth <= -EDGE_DB, (cid, g, dc, ny)


def test_filter_segments_depend_on_the_signal_alone():
    """llsm_gpu_plan_index(13, n, H): how many time segments the zero-phase filter cuts a signal of n samples into when
    its slowest pole reaches H samples.  Nothing about the batch enters: the bench shape (1 s at 44.1 kHz, and every
    synthesis template of at most 20 128 samples) stays whole, a 150 000-sample drop-in signal is cut."""
    L = llsm.load()

    def segs(n, H):
        return L.llsm_gpu_plan_index(13, n, H, 0.0, 0.005, 44100.0, 0.0)

    for H in (0, 96, 416, 1088, 3200):
        assert segs(44100, H) == 1 and segs(20128, H) == 1
    assert segs(150000, 0) == 1                      # (no pole reach: not a job that is cut)
    for H in (96, 416, 1088):
        s = segs(150000, H)
        assert s == min(150000 // max(2048, 6 * H), 64) and s > 1, (H, s)
    # the other plan arguments do not enter
    assert L.llsm_gpu_plan_index(13, 150000, 416, 0.0, 0.001, 96000.0, 0.3) == segs(150000, 416)
    # at most 64 segments, never fewer than 2048 or 6 H samples each
    for n in (65536, 100000, 1 << 20, 1 << 24):
        for H in (96, 2000):
            s = segs(n, H)
            assert 1 <= s <= 64 and (s == 1 or n // s >= max(2048, 6 * H)), (n, H, s)
