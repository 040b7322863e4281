"""The rules of llsm_gpu_batch_estimate_f0 (llsm_gpu.h) restated in numpy, float64, with the cross-correlation by FFT:
the reference of tests/test_f0_host.py and tests/test_gpu_f0.py.  Rules 2 - 8 are yin_track of
tests/golden/make_f0_track.py on the batch's frame grid, plus the all-zero gate of rule 3."""
import os
import wave

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEFAULTS = dict(fmin=50.0, fmax=500.0, threshold=0.15, silence_rel=0.05, window_extra=200, smooth=1, keep_cmndf=0)


def read_wav(name):
    w = wave.open(os.path.join(GOLDEN, name + ".wav"))
    assert w.getnchannels() == 1 and w.getsampwidth() == 2
    x = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").astype(np.float64) / 32768.0
    return x.astype(np.float32), float(w.getframerate())      # (int16 / 32768 is exact in float32)


def options(**kw):
    """the options as the library holds them: the float members rounded to float32"""
    o = dict(DEFAULTS)
    o.update(kw)
    for k in ("fmin", "fmax", "threshold", "silence_rel"):
        o[k] = float(np.float32(o[k]))
    return o


def plan(fs, o):
    """rule 1"""
    fs = float(np.float32(fs))
    lmin, lmax = int(fs / o["fmax"]), int(fs / o["fmin"])
    W = lmax + o["window_extra"]
    nfft = 256
    while nfft < W + lmax:
        nfft *= 2
    return lmin, lmax, W, nfft


def centers(nfrm, thop, fs):
    """plan.h center(): round(i * thop * fs), float32 products, halves away from zero"""
    v = (np.arange(nfrm).astype(np.float32) * np.float32(thop)) * np.float32(fs)
    return np.floor(v.astype(np.float64) + 0.5).astype(np.int64)


def smooth5(raw):
    """rule 8, in the dtype of `raw`"""
    out = raw.copy()
    for i in range(2, len(raw) - 2):
        w = raw[i - 2: i + 3]
        nz = np.count_nonzero(w)
        if raw[i] != 0 and nz >= 4:
            out[i] = np.median(w[w != 0])
        elif raw[i] != 0 and nz <= 2:
            out[i] = 0
    return out


def estimate(x, fs, nfrm, thop, **kw):
    """rules 1 - 9 for one utterance: (f0 float32 [nfrm], raw float64 [nfrm], cm float64 [nfrm][lmax + 1], gated bool [nfrm])"""
    o = options(**kw)
    lmin, lmax, W, nfft = plan(fs, o)
    x = np.asarray(x, np.float64)
    nx = len(x)
    fs = float(np.float32(fs))
    L = W + lmax
    raw = np.zeros(nfrm)
    cm = np.ones((nfrm, lmax + 1))
    gated = np.ones(nfrm, bool)
    if nfrm == 0:
        return raw.astype(np.float32), raw, cm, gated
    idx = (centers(nfrm, thop, fs) - W // 2)[:, None] + np.arange(L)[None, :]
    ok = (idx >= 0) & (idx < nx)
    s = np.where(ok, x[np.clip(idx, 0, max(nx - 1, 0))] if nx else 0.0, 0.0)          # rule 2
    sq = s * s
    e0 = sq[:, :W].sum(axis=1)
    floor = o["silence_rel"] ** 2 * float(np.sum(x * x)) / nx if nx else 0.0
    gated = (e0 == 0) | (e0 / W < floor)                                                 # rule 3
    A = np.fft.rfft(s[:, :W], nfft, axis=1)
    S = np.fft.rfft(s, nfft, axis=1)
    r = np.fft.irfft(np.conj(A) * S, nfft, axis=1)[:, : lmax + 1]
    csq = np.concatenate([np.zeros((nfrm, 1)), np.cumsum(sq, axis=1)], axis=1)
    tau = np.arange(lmax + 1)
    E = csq[:, tau + W] - csq[:, tau]
    d = e0[:, None] + E - 2.0 * r                                                        # rule 4
    cs = np.cumsum(d[:, 1:], axis=1)
    cm[:, 1:] = d[:, 1:] * tau[1:] / np.maximum(cs, 1e-12)                               # rule 5
    cm[gated] = 1.0
    for i in np.where(~gated)[0]:
        c = cm[i]
        cand = np.where(c[lmin:lmax] < o["threshold"])[0]                                # rule 6
        if len(cand) == 0:
            continue
        l = int(cand[0]) + lmin
        while l + 1 < lmax and c[l + 1] < c[l]:
            l += 1
        y0, y1, y2 = c[l - 1], c[l], c[l + 1]                                            # rule 7
        den = y0 - 2 * y1 + y2
        off = 0.5 * (y0 - y2) / den if abs(den) > 1e-12 else 0.0
        raw[i] = fs / (l + off)
    out = smooth5(raw) if o["smooth"] else raw
    return out.astype(np.float32), raw, cm, gated
