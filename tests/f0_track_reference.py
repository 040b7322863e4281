"""Rules T1 - T5 of llsm_gpu_batch_track_f0 (llsm_gpu.h) restated in numpy: the reference of tests/test_f0_track_host.py
and tests/test_gpu_f0_track.py.  candidates() works from a float32 CMNDF plane (the device's own, or the float64 plane of
f0_reference.estimate rounded to float32), viterbi() in float32, operation by operation, from the candidate arrays;
track() chains f0_reference.estimate into both.  trap() is the signal whose odd harmonics fade: the CMNDF of such a frame
dips below the estimator's threshold at half the period."""
import numpy as np

import f0_reference as ref

K = 7                                                       # candidate slots; state 7 is "unvoiced"
TRACK_DEFAULTS = dict(cand_threshold=0.5, unvoiced_cost=0.2, switch_cost=0.05, jump_cost=0.5, octave_cost=0.02)


def track_options(**kw):
    """the track options as the library holds them: float32"""
    o = dict(TRACK_DEFAULTS)
    o.update(kw)
    return {k: np.float32(v) for k, v in o.items()}


def candidates(cm, gated, fs, lmin, lmax, cand_threshold=TRACK_DEFAULTS["cand_threshold"]):
    """rule T1 over a float32 plane cm[F][lmax + 1]: (f0, cost, l2) float32 [F][8] each, slot for slot as plane 5 holds
    them (l2[:, 7] = L, unused slots zero), and the number of candidates n[F]"""
    cm = np.asarray(cm, np.float32)
    F = cm.shape[0]
    fs = float(np.float32(fs))
    f0 = np.zeros((F, 8), np.float32); cost = np.zeros((F, 8), np.float32); l2 = np.zeros((F, 8), np.float32)
    n = np.zeros(F, np.int64)
    l2[:, 7] = np.float32(np.log2(fs / lmin))
    if F == 0:
        return f0, cost, l2, n
    c = cm[:, lmin:lmax]
    is_c = (c < cm[:, lmin - 1:lmax - 1]) & (c <= cm[:, lmin + 1:lmax + 1]) & (c < np.float32(cand_threshold))
    is_c &= ~np.asarray(gated, bool)[:, None]
    key = np.where(is_c, c, np.float32(np.inf))
    order = np.argsort(key, axis=1, kind="stable")[:, :K]                # lowest cm first, ties to the smaller lag
    k = order.shape[1]
    valid = np.take_along_axis(is_c, order, axis=1)
    tau = order + lmin
    rows = np.arange(F)[:, None]
    y0, y1, y2 = (cm[rows, tau + d].astype(np.float64) for d in (-1, 0, 1))
    den = y0 - 2.0 * y1 + y2
    with np.errstate(divide="ignore", invalid="ignore"):
        off = np.where(np.abs(den) > 1e-12, 0.5 * (y0 - y2) / den, 0.0)  # rule 7 of estimate_f0
        f = (fs / (tau + off)).astype(np.float32)
        lg = np.log2(f.astype(np.float64)).astype(np.float32)
    f0[:, :k] = np.where(valid, f, 0); cost[:, :k] = np.where(valid, cm[rows, tau], 0); l2[:, :k] = np.where(valid, lg, 0)
    n[:] = valid.sum(axis=1)
    return f0, cost, l2, n


def viterbi(f0, cost, l2, n, L, **kw):
    """rules T2 - T5 for one utterance, float32 with one rounding per operation: the F0 row"""
    o = track_options(**kw)
    uc, sc, jc, oc = o["unvoiced_cost"], o["switch_cost"], o["jump_cost"], o["octave_cost"]
    f0 = np.asarray(f0, np.float32); cost = np.asarray(cost, np.float32); l2 = np.asarray(l2, np.float32)
    L = np.float32(L)
    F = len(n)
    out = np.zeros(F, np.float32)
    if F == 0:
        return out
    inf = np.float32(np.inf)

    def local(i):                                                         # T2
        loc = np.full(8, inf, np.float32)
        m = int(n[i])
        loc[:m] = cost[i, :m] + oc * (L - l2[i, :m])
        loc[7] = uc if m > 0 else np.float32(0)
        return loc

    bp = np.zeros((F, 8), np.int64)
    acc = local(0)
    with np.errstate(invalid="ignore"):
        for i in range(1, F):
            tr = np.zeros((8, 8), np.float32)                             # T3, [a][j]
            tr[:7, :7] = jc * np.abs(l2[i, None, :7] - l2[i - 1, :7, None])
            tr[7, :7] = sc; tr[:7, 7] = sc
            tot = acc[:, None] + tr                                       # T4; +inf where state a does not exist
            bp[i] = np.argmin(tot, axis=0)                                # the first, that is smallest, a of the minimum
            acc = tot.min(axis=0) + local(i)
            acc = acc - acc.min()
    s = int(np.argmin(acc))
    for i in range(F - 1, -1, -1):                                        # T5
        out[i] = f0[i, s] if s < 7 else 0
        s = int(bp[i, s])
    return out


def track(x, fs, nfrm, thop, **kw):
    """rules 1 - 5 of estimate_f0 in float64 (f0_reference.estimate), the CMNDF rounded to float32, then T1 - T5:
    (f0 float32 [nfrm], (f0, cost, l2, n) of candidates(), cm float32, gated)"""
    topt = {k: kw.pop(k) for k in list(kw) if k in TRACK_DEFAULTS}
    o = ref.options(**kw)
    lmin, lmax, _, _ = ref.plan(fs, o)
    _, _, cm, gated = ref.estimate(x, fs, nfrm, thop, **kw)
    cm = cm.astype(np.float32)
    t = track_options(**topt)
    cand = candidates(cm, gated, fs, lmin, lmax, t["cand_threshold"])
    row = viterbi(*cand, cand[2][0, 7] if nfrm else 0, **topt)
    return row, cand, cm, gated


def gross_errors(got, true, rel=0.2):
    """frames voiced on both sides whose F0 is more than `rel` from the true one"""
    got = np.asarray(got, np.float64); true = np.asarray(true, np.float64)
    both = (got > 0) & (true > 0)
    return int(np.count_nonzero(np.abs(got[both] - true[both]) > rel * true[both]))


def trap(u, fs=44100.0, thop=0.005):
    """0.6 s whose odd harmonics fade in and out (a formant on 2 F0): (x float32, true f0 float32 [120])"""
    rng = np.random.default_rng(4242 + u)
    nx = int(0.6 * fs)
    nfrm = int(nx / fs / thop)
    t = np.arange(nfrm) * thop
    contour = 110.0 + 25.0 * np.sin(2 * np.pi * 0.9 * t + u) + 6.0 * np.sin(2 * np.pi * 3.3 * t)
    voiced = np.ones(nfrm, bool)
    voiced[:8] = False
    voiced[-8:] = False
    f0 = np.where(voiced, contour, 0.0)
    ts = np.arange(nx) / fs
    f0s = np.interp(ts, t, contour)                         # the phase runs on under the unvoiced frames
    vs = np.interp(ts, t, voiced.astype(float))
    phase = 2 * np.pi * np.cumsum(f0s) / fs
    odd = 0.04 + 0.96 * np.clip(2.0 * np.abs(np.sin(2 * np.pi * 1.5 * ts + 0.4 * u)) - 0.8, 0.0, 1.0)
    x = np.zeros(nx)
    for k in range(1, 30):
        x += 0.25 * k ** -1.1 * (odd if k % 2 else 1.0) * np.cos(k * phase + 0.37 * k * k)
    x *= vs
    x += (0.003 + 0.03 * (1 - vs)) * rng.standard_normal(nx)
    return x.astype(np.float32), f0.astype(np.float32)
