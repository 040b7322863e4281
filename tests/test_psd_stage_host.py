"""CPU: the numpy restatement of tests/psd_stage_reference.py IS the float64 oracle's noise-PSD tail, its float32 form is
a tight yardstick, and the checker built on both notices errors the whole-chain parity bounds let through.

tests/test_gpu_psd_stages.py judges k_psd_frames* and k_kalman with psd_frames_ref / kalman_ref / kalman_check; this
module is what entitles it to.  The oracle's intermediate arrays come through o_set_stage_hook (oracle/llsm_oracle.c:
stage 0 residual, 2 resampled envelope [nfrm][nspec], 3 log periodogram [nspec][nfrm])."""
import ctypes as C

import numpy as np
import pytest

from conftest import make_speechlike
from psd_stage_reference import FAULTS, PSD_FRAMES_BOUND, kalman_check, kalman_ref, psd_frames_full, psd_frames_metric, psd_frames_ref

INPUTS = {"44k_5ms": (44100.0, 0.005, 31), "16k_5ms": (16000.0, 0.005, 32), "8k_10ms": (8000.0, 0.010, 33)}
NPSD = 256                              # the default of llsm_create_aoptions: points between bins
CONV = [(0, 0), (1, 0), (0, 1), (1, 1)]                 # (kalman_init, interp1u_exclusive)


def _analyze_captured(o, fs, thop, x, f0):
    cap = {}
    HT = C.CFUNCTYPE(None, C.c_int, C.c_int, C.POINTER(o.fpt), C.c_long)

    def hook(stage, index, data, n):
        if stage in (0, 2, 3):
            cap[stage] = np.ctypeslib.as_array(data, shape=(n,)).astype(np.float64).copy()
    cb = HT(hook)
    o.lib.o_set_stage_hook(cb)
    try:
        pr = o.analyze(o.aoptions(thop=thop, npsd=NPSD, f0_refine=0, nchannel=1), x, fs, f0)
    finally:
        o.lib.o_set_stage_hook(C.cast(None, HT))
    return pr, cap


@pytest.fixture(scope="module")
def cases(o64):
    """per input and convention pair: the oracle's rows and its captured planes ([nfrm][nspec] both)"""
    out = {}
    try:
        for cid, (fs, thop, seed) in INPUTS.items():
            x, f0 = make_speechlike(seed, fs=fs, thop=thop)
            for ki, ex in CONV:
                o64.set_convention("kalman_init", ki); o64.set_convention("interp1u_exclusive", ex)
                pr, cap = _analyze_captured(o64, fs, thop, x, f0)
                n = len(f0)
                out[cid, ki, ex] = dict(fs=fs, thop=thop, n=n, nx=len(x), psd=pr.psd.copy(), psdres=pr.psdres.copy(),
                                        xres=cap[0], env=cap[2].reshape(n, -1), z=cap[3].reshape(-1, n).T.copy())
    finally:
        o64.set_convention("kalman_init", 0); o64.set_convention("interp1u_exclusive", 0)
    return out


@pytest.mark.parametrize("ki,ex", CONV)
@pytest.mark.parametrize("cid", sorted(INPUTS))
def test_kalman_ref_is_the_oracle(cases, cid, ki, ex):
    c = cases[cid, ki, ex]
    psd, res = kalman_ref(c["env"], c["z"], [0, c["n"]], NPSD, c["fs"], ki, ex, np.float64)
    assert psd.shape == c["psd"].shape
    assert np.max(np.abs(psd - c["psd"])) <= 1e-9, np.max(np.abs(psd - c["psd"]))
    assert np.max(np.abs(res - c["psdres"])) <= 1e-9, np.max(np.abs(res - c["psdres"]))


def test_conventions_change_the_reference(cases):
    """(so the four cases above are four statements)"""
    a = cases["44k_5ms", 0, 0]
    for ki, ex in CONV[1:]:
        assert np.max(np.abs(cases["44k_5ms", ki, ex]["psd"] - a["psd"])) > 1e-3, (ki, ex)


@pytest.mark.parametrize("cid", sorted(INPUTS))
def test_psd_frames_ref_is_the_oracle(cases, cid):
    c = cases[cid, 0, 0]
    logp = psd_frames_ref(c["xres"], [0, c["nx"]], [0, c["n"]], c["thop"], c["fs"])
    assert logp.shape == c["z"].shape
    assert np.max(np.abs(logp - c["z"])) <= 1e-10, np.max(np.abs(logp - c["z"]))


@pytest.mark.parametrize("cid", sorted(INPUTS))
def test_stage_a_metric_passes_rounding_and_flags_errors(cases, cid):
    """The Stage A metric under its bound: the float64 log periodogram merely rounded to float32 passes (half an ulp of a
    logarithm of magnitude <= 23.03 is 9.6e-7); every frame one sample late, the periodic Blackman window, or the window
    power of the other window (a shift of 1 / nwin) does not."""
    c = cases[cid, 0, 0]
    args = (c["xres"].astype(np.float32), [0, c["nx"]], [0, c["n"]], c["thop"], c["fs"])
    logp, mag = psd_frames_full(*args)
    assert psd_frames_metric(logp.astype(np.float32), logp, mag).max() <= 9.6e-7
    for fault in ("centre", "periodic", "wpow"):
        wrong = psd_frames_full(*args, fault=fault)[0].astype(np.float32)
        assert psd_frames_metric(wrong, logp, mag).max() > PSD_FRAMES_BOUND, fault


def _f32_planes(c):
    return c["env"].astype(np.float32), c["z"].astype(np.float32)


def _yardstick(cases, npsd):
    worst = [0.0, 0.0]
    for cid in INPUTS:
        c = cases[cid, 0, 0]
        env, z = _f32_planes(c)
        p64, r64 = kalman_ref(env, z, [0, c["n"]], npsd, c["fs"], dtype=np.float64)
        p32, r32 = kalman_ref(env, z, [0, c["n"]], npsd, c["fs"], dtype=np.float32)
        assert p32.dtype == np.float32 and r32.dtype == np.float32
        worst[0] = max(worst[0], float(np.max(np.abs(p32 - p64)))); worst[1] = max(worst[1], float(np.max(np.abs(r32 - r64))))
    print("float32 yardstick, npsd %d: PSD %.3g dB, PSDRES %.3g dB" % (npsd, worst[0], worst[1]))
    return worst


def test_float32_yardstick_is_small(cases):
    """The float32 restatement on float32-rounded planes against float64, largest value over the three inputs.  If it
    ever grows, the bound 4 Y + 5e-5 dB of the GPU test stops meaning anything.  Two parts:
    * the recursions and the output formulas alone, seen where every PSD point falls on a bin (npsd = 129 on 513, 257,
      129 bins): 2.2e-5 dB (PSD), 1.6e-5 dB (PSDRES) when this was written; held under the additive term 5e-5 dB;
    * with points between bins (npsd = 256) the float32 POSITION, off by up to 2 ulp of a number near 500 (6e-5 bins),
      times the bin-to-bin step of the plane being interpolated -- a few dB for the smoothed level, the periodogram's own
      +-5.6 dB scatter for the residual: 3.3e-4 dB (PSD) and 8.2e-4 dB (PSDRES), both on the 513 bins of the 44.1 kHz
      input (16 kHz: 1.2e-4 / 3.1e-4; 8 kHz: 1.3e-4 / 5.1e-4; over seeds 0 ... 2 of the same inputs the 44.1 kHz values
      reach 4.1e-4 / 9.95e-4).  Held under 5e-4 / 1e-3 dB."""
    exact = _yardstick(cases, 129)
    assert exact[0] <= 5e-5 and exact[1] <= 5e-5, exact
    worst = _yardstick(cases, NPSD)
    assert worst[0] <= 5e-4 and worst[1] <= 1e-3, worst


@pytest.mark.parametrize("cid", sorted(INPUTS))
def test_checker_passes_the_float32_restatement(cases, cid):
    c = cases[cid, 0, 0]
    env, z = _f32_planes(c)
    p32, r32 = kalman_ref(env, z, [0, c["n"]], NPSD, c["fs"], dtype=np.float32)
    bad, st = kalman_check(p32, r32, env, z, [0, c["n"]], NPSD, c["fs"])
    assert not bad, bad
    assert st["ratio_psd"] <= 0.25 + 1e-12 and st["ratio_psdres"] <= 0.25 + 1e-12       # Y / (4 Y + add)


@pytest.mark.parametrize("fault", FAULTS)
@pytest.mark.parametrize("cid", sorted(INPUTS))
def test_checker_flags_subtle_errors(cases, cid, fault):
    """EULERGAMMA typed 0.58 (0.012 dB everywhere); the last point from bin nspec - 2; Q[i] for Q[i + 1] in the smoother
    at the last frame of every chunk of 8; the frame two back as the earliest envelope frame at the first frame of
    every chunk: each in the float32 restatement, each must be flagged."""
    c = cases[cid, 0, 0]
    env, z = _f32_planes(c)
    pf, rf = kalman_ref(env, z, [0, c["n"]], NPSD, c["fs"], dtype=np.float32, fault=fault)
    bad, st = kalman_check(pf, rf, env, z, [0, c["n"]], NPSD, c["fs"])
    assert bad, (fault, st)
    rows = {b[1] for b in bad}
    if fault == "gamma":
        assert rows == {"psd"}, bad                       # (the residual does not see the bias term)
    if fault == "lastbin":
        assert all(b[3] == NPSD - 1 for b in bad) and rows == {"psd", "psdres"}, bad


def test_checker_flags_nonfinite_rows(cases):
    c = cases["8k_10ms", 0, 0]
    env, z = _f32_planes(c)
    p32, r32 = kalman_ref(env, z, [0, c["n"]], NPSD, c["fs"], dtype=np.float32)
    p32[3, 5] = np.nan
    bad, _ = kalman_check(p32, r32, env, z, [0, c["n"]], NPSD, c["fs"])
    assert [b[:4] for b in bad] == [(0, "psd", 3, 5)], bad
