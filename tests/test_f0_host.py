"""Host side of llsm_gpu_batch_estimate_f0 (no GPU): the default options, the sizes of llsm_gpu_f0_plan, the refusals
that need no batch, and the numpy restatement of the rules (tests/f0_reference.py, float64, FFT route) against the
committed golden tracks, which tests/golden/make_f0_track.py made with its direct sums."""
import ctypes as C
import os

import numpy as np
import pytest

import libllsm2_amd as llsm
import f0_reference as ref


def test_default_options():
    o = llsm.F0Options()
    llsm.load().llsm_gpu_f0_default_options(C.byref(o))
    assert (o.fmin, o.fmax, o.window_extra, o.smooth, o.keep_cmndf) == (50.0, 500.0, 200, 1, 0)
    assert o.threshold == float(np.float32(0.15)) and o.silence_rel == float(np.float32(0.05))
    d = ref.options()
    assert all(getattr(o, k) == d[k] for k in d)


# (fs, fmin, fmax) -> (lmin, lmax, W, nfft): the four transform sizes the GPU tests run
PLANS = [((44100.0, 50.0, 500.0), (88, 882, 1082, 2048)),
         ((8000.0, 100.0, 500.0), (16, 80, 280, 512)),
         ((16000.0, 50.0, 500.0), (32, 320, 520, 1024)),
         ((44100.0, 40.0, 800.0), (55, 1102, 1302, 4096))]


@pytest.mark.parametrize("cfg,want", PLANS)
def test_plan_sizes(cfg, want):
    fs, fmin, fmax = cfg
    p = llsm.f0_plan(fs, fmin=fmin, fmax=fmax)
    assert (p["lmin"], p["lmax"], p["W"], p["nfft"]) == want
    assert ref.plan(fs, ref.options(fmin=fmin, fmax=fmax)) == want


def test_plan_defaults_from_null_and_null_outputs():
    L = llsm.load()
    v = [C.c_int() for _ in range(4)]
    assert L.llsm_gpu_f0_plan(None, 44100.0, *[C.byref(x) for x in v]) == 0
    assert [x.value for x in v] == [88, 882, 1082, 2048]
    assert L.llsm_gpu_f0_plan(None, 44100.0, None, None, None, None) == 0
    # the smallest transform is 256 points; 4096 is still taken, one sample more is not
    assert llsm.f0_plan(8000.0, fmin=400.0, fmax=2000.0, window_extra=1)["nfft"] == 256
    assert llsm.f0_plan(44100.0, fmin=40.0, fmax=800.0, window_extra=4096 - 2 * 1102)["nfft"] == 4096


nan = float("nan")
REFUSED = [dict(fmin=nan), dict(fmax=nan), dict(threshold=nan), dict(silence_rel=nan),
           dict(fmin=0.0), dict(fmin=-50.0), dict(fmin=500.0), dict(fmin=600.0),
           dict(fmax=30000.0),                                  # lmin = 1
           dict(fmin=497.0, fmax=500.0),                        # lmin 88, lmax 88
           dict(fmin=495.0, fmax=500.0),                        # lmin 88, lmax 89 = lmin + 1
           dict(threshold=0.0), dict(threshold=-0.1), dict(threshold=1.5),
           dict(silence_rel=-0.01), dict(window_extra=0), dict(window_extra=-5),
           dict(smooth=2), dict(smooth=-1), dict(keep_cmndf=2), dict(keep_cmndf=-1),
           dict(fmin=40.0, fmax=800.0, window_extra=4096 - 2 * 1102 + 1),   # W + lmax = 4097
           dict(fmin=10.0)]                                     # lmax = 4410 alone is beyond the transform


@pytest.mark.parametrize("kw", REFUSED, ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()))
def test_plan_refusals(kw):
    L = llsm.load()
    o = llsm.make_f0_options(**kw)
    v = [C.c_int(-7) for _ in range(4)]
    rc = L.llsm_gpu_f0_plan(C.byref(o), 44100.0, *[C.byref(x) for x in v])
    assert rc == -1
    assert L.llsm_gpu_last_error().decode().startswith("llsm_gpu_batch_estimate_f0:")
    assert [x.value for x in v] == [-7] * 4                     # nothing written
    with pytest.raises(llsm.LlsmError):
        llsm.f0_plan(44100.0, **kw)


def test_plan_edges_and_bad_rate():
    assert llsm.f0_plan(44100.0, threshold=1.0)["nfft"] == 2048          # (0, 1]: 1 is inside
    p = llsm.f0_plan(44100.0, fmin=490.0)                                # the narrowest range taken: lmax = lmin + 2
    assert (p["lmin"], p["lmax"]) == (88, 90)
    assert llsm.f0_plan(44100.0, silence_rel=0.0)["nfft"] == 2048
    for fs in (0.0, -1.0, nan):
        with pytest.raises(llsm.LlsmError, match="llsm_gpu_batch_estimate_f0:"):
            llsm.f0_plan(fs)


def test_estimate_refuses_null_batch():
    L = llsm.load()
    assert L.llsm_gpu_batch_estimate_f0(None, None) == -1
    assert L.llsm_gpu_last_error().decode().startswith("llsm_gpu_batch_estimate_f0:")


@pytest.mark.parametrize("name", ["arctic_a0001", "are-you-ready"])
def test_restatement_reproduces_golden_track(name):
    x, fs = ref.read_wav(name)
    want = np.load(os.path.join(ref.GOLDEN, name + "_f0_hop128.npy"))
    assert fs == 44100.0 and want.dtype == np.float32 and len(want) == len(x) // 128
    got, raw, cm, gated = ref.estimate(x, fs, len(want), np.float32(128.0 / 44100.0))
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert np.all(cm[gated] == 1.0) and np.all(raw[gated] == 0)


def test_smooth5_rule():
    z = np.float32
    raw = np.array([100, 0, 101, 103, 0, 0, 0, 107, 0, 0, 110, 111, 112, 113, 114, 0, 0], z)
    got = ref.smooth5(raw)
    want = raw.copy()                           # i = 2: (100, 0, 101, 103, 0) and i = 10, 14: three non-zero, kept
    want[3] = 0                                 # (0, 101, 103, 0, 0): two non-zero
    want[7] = 0                                 # isolated
    want[11] = z(0.5) * (z(111) + z(112))       # (0, 110, 111, 112, 113): four -> the mean of the middle two
    want[12] = 112                              # five -> the median
    want[13] = z(0.5) * (z(112) + z(113))       # (111, 112, 113, 114, 0): four
    assert np.array_equal(got, want), (got, want)
