"""Plain numpy restatement of the two last stages of the noise-PSD analysis, and the checkers built on it.

    residual -> [log periodogram per frame]  -> plane 1 of llsm_gpu_batch_debug_plane      (k_psd_frames*)
    planes 0 (envelope) and 1                -> [Kalman filter, RTS smoother, PSD grid]    (k_kalman) -> PSD, PSDRES

No GPU, no libllsm2_amd, no oracle: tests/test_psd_stage_host.py proves these functions against the float64 oracle
(oracle/llsm_oracle.c analyze_noise_psd, oracle/dsp_core.c o_kalmanf1d / o_kalmans1d) before tests/test_gpu_psd_stages.py
judges a kernel with them.  Offsets (nx_off, frm_off) are cumulative, one entry more than there are utterances."""
import numpy as np

EULERGAMMA = 0.57721566
LN10_REF = 2.3025851                  # the reference's LOG2IN(x) = x / 2.3025851 * 10
KAL_ADD_DB = 5e-5                     # the additive term of the Stage B bound (kalman_check)
PSD_FRAMES_CAP = 4e-5                 # the Stage A constant may never exceed this (psd_frames_metric)
# Stage A bound: 4 x the worst value of psd_frames_metric over the nine batches of tests/test_gpu_psd_stages.py on one
# MI355X, 3.72e-6 (96 kHz, 25 ms hop, 16384 points, frame 11 bin 8163; the other eight: 1.4e-6 ... 2.3e-6).  The factor:
# rounding noise differs from input to input and nine batches are a small sample.
PSD_FRAMES_BOUND = 4 * 3.72e-6
assert PSD_FRAMES_BOUND <= PSD_FRAMES_CAP


def _iround(v):
    v = np.asarray(v, np.float64)
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)          # C round(): half away from zero


def psd_geometry(nfrm, thop, fs):
    """(centres[nfrm], nwin, nfft) of the PSD frames: centre round(i thop fs), nwin = round(thop 4 fs), both products
    in float32 left to right (gpu_common.sin_geometry does the same for the harmonic overlap-add)."""
    t32, f32 = np.float32(thop), np.float32(fs)
    nwin = int(_iround(np.float32(t32 * np.float32(4.0)) * f32))
    c = _iround((np.arange(nfrm, dtype=np.float32) * t32).astype(np.float32) * f32)
    nfft = 1
    while nfft < nwin:
        nfft *= 2
    return c, nwin, nfft


def blackman(n, periodic=False):
    if n == 1:
        return np.ones(1)
    t = 2.0 * np.pi * np.arange(n) / (n if periodic else n - 1)
    return 0.42 - 0.5 * np.cos(t) + 0.08 * np.cos(2.0 * t)


def psd_frames_full(xres, nx_off, frm_off, thop, fs, fault=None):
    """(log periodogram, |X|) of every frame, each [total_frames][nfft / 2 + 1] float64; |X| is the magnitude of the
    windowed frame's transform before the division by the window power.  fault (host test only: the metric must notice
    each): "centre" every frame one sample late; "periodic" the periodic Blackman window; "wpow" the window power
    taken from the periodic window while the symmetric one is applied (a level shift of about 1 / nwin)."""
    xres = np.asarray(xres, np.float64)
    total = int(frm_off[-1])
    _, nwin, nfft = psd_geometry(0, thop, fs)
    w = blackman(nwin, periodic=fault == "periodic")
    wp = blackman(nwin, periodic=True) if fault == "wpow" else w
    wpow = float(np.sum(wp * wp))
    logp = np.zeros((total, nfft // 2 + 1)); mag = np.zeros((total, nfft // 2 + 1))
    for u in range(len(frm_off) - 1):
        n = int(frm_off[u + 1] - frm_off[u])
        x = xres[int(nx_off[u]):int(nx_off[u + 1])]
        c, _, _ = psd_geometry(n, thop, fs)
        for i in range(n):
            base = int(c[i]) - nwin // 2 + (1 if fault == "centre" else 0)
            a, b = max(base, 0), min(base + nwin, len(x))
            fr = np.zeros(nwin)
            if a < b:
                fr[a - base:b - base] = x[a:b]
            X = np.fft.rfft(fr * w, nfft)
            g = int(frm_off[u]) + i
            mag[g] = np.abs(X)
            logp[g] = np.log(np.maximum(1e-10, (X.real ** 2 + X.imag ** 2) / wpow))
    return logp, mag


def psd_frames_ref(xres, nx_off, frm_off, thop, fs):
    """[total_frames][nfft / 2 + 1] float64: log(max(1e-10, |rfft(w x)|^2 / sum(w^2))), symmetric Blackman window of
    round(thop 4 fs) samples centred at round(i thop fs), samples outside the utterance zero."""
    return psd_frames_full(xres, nx_off, frm_off, thop, fs)[0]


def psd_frames_metric(plane1, logp_ref, mag_ref):
    """Stage A metric at every value: |plane1 - ref| min(1, |X_ref| / S_g).  Two frames share one complex transform (a
    lone frame sits beside its own copy), so a quiet frame carries the float32 error of its louder partner; which
    frames are partners is not visible here, so S_g is the largest RMS (over bins) of |X_ref| among flat frames
    g - 1, g, g + 1, which bounds either choice.  Weight 1 where S_g = 0."""
    plane1 = np.asarray(plane1, np.float64).reshape(logp_ref.shape)
    rms = np.sqrt(np.mean(mag_ref ** 2, axis=1)) if len(mag_ref) else np.zeros(0)
    pad = np.concatenate([[0.0], rms, [0.0]])
    S = np.maximum(np.maximum(pad[:-2], pad[1:-1]), pad[2:])
    with np.errstate(divide="ignore", invalid="ignore"):
        wgt = np.where(S[:, None] > 0, np.minimum(1.0, mag_ref / S[:, None]), 1.0)
    return np.abs(plane1 - logp_ref) * wgt


# ---- Kalman filter + RTS smoother + PSD grid ----
# fault (host test only: the checker must notice each): "gamma" EULERGAMMA typed 0.58; "lastbin" the last output point
# from bin nspec - 2; "q_chunk" Q[i + 1] replaced by Q[i] in the smoother at frames i % 8 == 7; "eprev_chunk" the frame
# two back as the earliest of the three envelope frames at frames i % 8 == 0.
FAULTS = ("gamma", "lastbin", "q_chunk", "eprev_chunk")


def _process_variance(e, dtype, fault):
    """e: [n][nspec] -> Q [n][nspec]: the 3-frame moving variance with clamped ends, floor 1e-8.  float64: the oracle's
    m2 / 3 - m1^2 / 9.  float32: the mean squared deviation from the 3-frame mean (the form k_kalman documents; the
    difference of squares cancels in float32 and would make the yardstick several times more lenient)."""
    n = len(e)
    i = np.arange(n)
    ip, inx = np.maximum(i - 1, 0), np.minimum(i + 1, n - 1)
    if fault == "eprev_chunk":
        ip = np.where(i % 8 == 0, np.maximum(i - 2, 0), ip)
    a, b, c = e[ip], e, e[inx]
    if dtype == np.float64:
        m1 = (a + b) + c
        m2 = (a * a + b * b) + c * c
        return np.maximum(1e-8, m2 / 3 - m1 * m1 / 9)
    third = dtype(1.0) / dtype(3.0)
    mean = ((a + b) + c) * third
    da, db, dc = a - mean, b - mean, c - mean
    return np.maximum(dtype(1e-8), ((da * da + db * db) + dc * dc) * third)


def _grid(nspec, npsd, fs, excl, dtype):
    """(k0, k1, r) per output point: interp1u of nspec uniform bins onto linspace(0, fs / 2, npsd); excl: the bins are
    taken to span [0, fs / 2) (position scaled by nspec instead of nspec - 1).  Beyond the last bin pair: the last bin."""
    fnyq = dtype(fs / 2.0)
    j = np.arange(npsd).astype(dtype)
    xq = fnyq * j / dtype(npsd - 1) if npsd > 1 else np.zeros(npsd, dtype)
    pos = xq / fnyq * dtype(nspec - 1 + int(bool(excl)))
    k = np.floor(pos).astype(np.int64)
    last = k >= nspec - 1
    k0 = np.where(last, nspec - 1, np.maximum(k, 0))
    k1 = np.where(last, nspec - 1, k0 + 1)
    r = np.where(last | (k < 0), dtype(0), pos - k0.astype(dtype)).astype(dtype)
    return k0, k1, r


def kalman_ref(env, z, frm_off, npsd, fs, kalman_init=0, interp1u_excl=0, dtype=np.float64, fault=None):
    """(psd, psdres), each [total_frames][npsd] of `dtype`, from the envelope plane and the log-periodogram plane
    ([total_frames][nspec] each): Q from env, R = pi^2 / 6, scalar random-walk Kalman filter (first observation = first
    state; kalman_init = 1: its covariance takes the update of frame 0 as well), RTS smoother, residual z - s,
    s + 0.57721566, both interpolated onto the PSD grid, psdres = res / 2.3025851 x 10,
    psd = 10 log10(exp(.) 44100 / fs + 1e-12).  dtype float64: the reference.  dtype float32: the yardstick -- the same
    rules with every intermediate in float32 and IEEE division."""
    dtype = np.dtype(dtype).type
    env = np.asarray(env).astype(dtype); z = np.asarray(z).astype(dtype)
    total, nspec = z.shape
    R = dtype(np.pi * np.pi / 6.0)
    one = dtype(1.0)
    k0, k1, r = _grid(nspec, npsd, fs, interp1u_excl, dtype)
    if fault == "lastbin":
        k1 = k1.copy(); k0 = k0.copy()
        k0[-1] = k1[-1] = nspec - 2
    gamma = dtype(0.58 if fault == "gamma" else EULERGAMMA)
    psd = np.zeros((total, npsd), dtype); res = np.zeros((total, npsd), dtype)
    for u in range(len(frm_off) - 1):
        lo, n = int(frm_off[u]), int(frm_off[u + 1] - frm_off[u])
        if n == 0:
            continue
        zu = z[lo:lo + n]
        Q = _process_variance(env[lo:lo + n], dtype, fault)
        y = np.zeros((n, nspec), dtype); P = np.zeros((n, nspec), dtype)
        x = zu[0].copy(); p = np.full(nspec, R, dtype)
        if kalman_init == 1:
            pp = p + Q[0]
            p = (one - pp / (pp + R)) * pp
        y[0], P[0] = x, p
        for i in range(1, n):
            pp = p + Q[i]
            k = pp / (pp + R)
            x = x + k * (zu[i] - x)
            p = (one - k) * pp
            y[i], P[i] = x, p
        s = np.zeros((n, nspec), dtype)
        s[n - 1] = y[n - 1]
        for i in range(n - 2, -1, -1):
            qn = Q[i] if (fault == "q_chunk" and i % 8 == 7) else Q[i + 1]
            c = P[i] / (P[i] + qn)
            s[i] = y[i] + c * (s[i + 1] - y[i])
        m = s + gamma
        rs = zu - s
        a = m[:, k0] + (m[:, k1] - m[:, k0]) * r
        b = rs[:, k0] + (rs[:, k1] - rs[:, k0]) * r
        res[lo:lo + n] = b / dtype(LN10_REF) * dtype(10.0)
        e = np.exp(a)
        psd[lo:lo + n] = dtype(10.0) * np.log10(e * dtype(44100.0) / dtype(fs) + dtype(1e-12))
    assert psd.dtype == dtype and res.dtype == dtype
    return psd, res


def kalman_check(psd_dev, res_dev, env, z, frm_off, npsd, fs, kalman_init=0, interp1u_excl=0, add=KAL_ADD_DB):
    """Stage B: rows computed from the planes (env, z) against kalman_ref(float64) of the same planes.  At EVERY
    (frame, point) of utterance u:   |rows - ref| <= 4 Y_u + add,   Y_u the largest distance between
    kalman_ref(float32) and kalman_ref(float64) on that utterance's planes (PSD and PSDRES each with their own Y).
    Returns (violations, stats): violations a list of (utterance, row, frame, point, error, bound)."""
    p64, r64 = kalman_ref(env, z, frm_off, npsd, fs, kalman_init, interp1u_excl, np.float64)
    p32, r32 = kalman_ref(env, z, frm_off, npsd, fs, kalman_init, interp1u_excl, np.float32)
    total = int(frm_off[-1])
    bad = []
    stats = dict(ratio_psd=0.0, ratio_psdres=0.0, y_psd=0.0, y_psdres=0.0, err_psd=0.0, err_psdres=0.0, values=0)
    for name, dev, ref, yard in (("psd", psd_dev, p64, p32), ("psdres", res_dev, r64, r32)):
        dev = np.asarray(dev, np.float64).reshape(total, npsd)
        for u in range(len(frm_off) - 1):
            sl = slice(int(frm_off[u]), int(frm_off[u + 1]))
            if sl.start == sl.stop:
                continue
            Y = float(np.max(np.abs(yard[sl].astype(np.float64) - ref[sl])))
            bound = 4.0 * Y + add
            err = np.abs(dev[sl] - ref[sl])
            err = np.where(np.isfinite(err), err, np.inf)
            w = np.unravel_index(int(np.argmax(err)), err.shape)
            stats["ratio_" + name] = max(stats["ratio_" + name], float(err[w]) / bound)
            stats["err_" + name] = max(stats["err_" + name], float(err[w]))
            stats["y_" + name] = max(stats["y_" + name], Y)
            if name == "psd":
                stats["values"] += err.size
            if not err[w] <= bound:
                bad.append((u, name, int(w[0]), int(w[1]), float(err[w]), bound, int(np.count_nonzero(err > bound))))
    return bad, stats
