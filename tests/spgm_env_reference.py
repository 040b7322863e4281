"""Plain numpy restatement of the spectral-envelope stage, the pointwise bound formed from it, the checker, and the inputs
both of its test modules use.

    A_X, A_F0  ->  Hann-windowed frame of three periods, zero-phase, N-point transform
               ->  L = log(|X| norm_base / ws + 1e-10)  ->  cepstrum  ->  lifter sinc(q f0 / fs)  ->  transform
               ->  plane 0 of llsm_gpu_batch_debug_plane: 2 env[(j N) // nfft_psd], j <= nfft_psd / 2
                   (k_spgm_env_wf<LOGN, LOGF, FIX> and its LDS fallback k_spgm_env; layer0.c:324-345)

No GPU and no oracle in this file: tests/test_spgm_env_host.py proves spgm_env_ref(float64) against the float64 oracle
before tests/test_gpu_spgm_env.py judges the kernels with spgm_env_check.  The kernel's inputs are uploaded by the caller,
so the reference needs no downloaded intermediate.

The bound (spgm_env_bound) is first-order sensitivity of the float64 reference, per frame, EPS = 2^-24:

    r[m] = EPS_X rms(|X|) nrm / (|X[m]| nrm + 1e-10),  t = -log1p(-min(r, 0.5)),  nrm = norm_base / ws
    B[k] = 2 (|h| (*) t)[idx(k)] + A,                    h = real(ifft(lifter)), (*) circular over the N bins

t is how far log(|X| nrm + 1e-10) moves when the bin moves by EPS_X of the RMS spectrum; the envelope is h (*) L.

EPS_X = EPS_FFT + EPS_WIN.
  * EPS_FFT = 4e-6: the pointwise allowance the project holds for a float32 transform against its RMS spectrum
    (tests/test_gpu_fft.py).
  * EPS_WIN = 1.8e-6: the float32 Hann window by phasor recurrence.  A seed (c, s) rounded from float64: 1.5 EPS per
    component.  One rotation step: two products and a sum of values below 1, half an ulp each (3 x EPS / 2), and the
    rotator's own rounding (|d| <= sqrt(2) EPS / 2 = 0.71 EPS), which is the same at every step and so adds linearly:
    2.21 EPS per step, worst case.  The longest recurrence of the tree walks half of 2048 points in strides of 64: 15
    steps, PH = 1.5 + 15 x 2.21 = 34.7 EPS on the phasor, (PH / 2 + 1) EPS = 18.3 EPS = 1.1e-6 on w = 0.5 - 0.5 c.  By
    Parseval rms(dX) / rms(X) = rms(x dw) / rms(x w) <= max |dw| sqrt(sum x^2 / sum (x w)^2) = max |dw| sqrt(8 / 3) for a
    stationary frame under a Hann window: 1.8e-6.  (A coherent dw moves a strong bin by dw / w of ITSELF, a few EPS of
    L: inside the first term of A.)

A, per frame, covers what t does not contain.  With S = rms(L), Lmax = max |L| (at most 23.03 = -log 1e-10),
H1 = sum |h|, c = real(ifft(L)), x_q = qq f0n, l_q = sinc(x_q):

    A = 2 [ H1 (4 EPS Lmax + 6 EPS) + 2 EPS_FFT S + sum_{q != 0} |c_q| (6 EPS |l_q| + EPS |cos(pi x_q) - l_q| + PH EPS / (pi x_q)) ]

  * the logarithm.  The hardware log2 is within one ulp of its result (2 EPS |L| at worst), the product with ln 2 adds
    EPS |L|: 3 EPS Lmax.  Its argument: the unpacking sum, the squares' sum, the square root (one ulp), the product with
    nrm and the sum with 1e-10, 6 EPS relative, which the logarithm turns into 6 EPS absolute.  Both pass through the
    lifter: x H1.  The store of 2 env (|env| <= H1 Lmax) is the fourth EPS Lmax.
  * two float32 transforms of L.  EPS_FFT of the RMS of what each transforms.  The first one's error passes the lifter
    (|l| <= 1) and an exact transform, which keep its RMS (Parseval): EPS_FFT S.  The second one's is EPS_FFT rms(env) <=
    EPS_FFT S.  Rounding errors of a transform are spread over its points, so the pointwise allowance serves pointwise.
  * the lifter.  l_q is formed as (1 / (N pi f0n)) sin(pi x_q) rcp(qq): the reciprocal is within one ulp (2 EPS), the
    scale's division and product 2 EPS, two products 2 EPS: 6 EPS |l_q|.  f0n = f0 / fs is a float32 on the device (EPS
    relative), which moves l_q by EPS |x l'(x)| = EPS |cos(pi x) - l|.  The sine comes from the same recurrence as the
    window: PH EPS absolute, divided by pi x_q.  Each moves the envelope by at most |c_q| times itself.  (l_0 = 1 / N is
    exact.)
The factor 2 is the plane's "* 2".  Nothing here is calibrated on a kernel.

spgm_env_check judges (a) |got - ref| <= B at every (frame, point), nothing excluded, no share allowed to miss; and
(b) per frame rms_j(got - ref) <= KAPPA rms_j(B), which catches a small systematic error that the worst-case form (a)
lets through.  KAPPA is four times the largest such ratio the float32 restatement reaches against the float64 one over
all inputs below (measured by tests/test_spgm_env_host.py, written beside the constant), and may not exceed 1.

The float32 restatement holds every array and transform to float32 (scipy.fft keeps complex64); window and lifter are
evaluated in float64 and rounded.  It does not know how any kernel forms them.

Conditions on the inputs (asserted by the host test): at most 20 % of a configuration's points with B > 1e-3 nepers, at
most 0.1 % with B > 1e-2.  An input that breaks either is replaced, not excused."""
import math

import numpy as np
import scipy.fft as sfft

EPS = 2.0 ** -24
EPS_FFT = 4e-6
PH_STEPS = 15
PH = 1.5 + PH_STEPS * (1.5 + math.sqrt(2.0) / 2.0)            # 34.7 (EPS): a recurrence phasor's component, worst case
EPS_WIN = math.sqrt(8.0 / 3.0) * (PH / 2.0 + 1.0) * EPS       # 1.8e-6
EPS_X = EPS_FFT + EPS_WIN                                     # 5.8e-6
# (b): 4 x the float32 restatement's largest per-frame ratio rms(err) / rms(B) over CONFIGS (test_spgm_env_host.py
# test_float32_restatement_is_inside_the_bound measures it: KAPPA_MEASURED, reached on the configuration named there)
KAPPA_MEASURED = 0.01898                                      # wf_10_1, frame 11; the median over frames is 0.003
KAPPA = 0.08                                                  # 4 x 0.01898 = 0.0759, rounded up: numpy's float32 log and
#                                                               sine differ in the last place between CPUs
CAP_1E3, CAP_1E2 = 0.20, 0.001
LOG_FLOOR = 1e-10


def _iround(v):
    v = np.asarray(v, np.float64)
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)          # C round(): half away from zero


def nextpow2(v):
    return int(2 ** math.ceil(math.log2(v)))


def norm_base_product():
    """engine.cpp:545-547: 1024 / (0.5 sum of the float32-rounded symmetric Hann(1024)), rounded to float32"""
    w = (0.5 - 0.5 * np.cos(2.0 * 3.14159265358979323846 * np.arange(1024) / 1023.0)).astype(np.float32)
    s = 0.0
    for v in w:
        s += float(v)
    return float(np.float32(1024.0 / (0.5 * s)))


def norm_base_oracle():
    """oracle/llsm_oracle.c o_compute_spectrogram in float64: the same sum, nothing rounded to float32"""
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(1024) / 1023.0)
    s = 0.0
    for v in w:
        s += float(v)
    return 1024.0 / (0.5 * s)


def sizes(fs, thop):
    """(nwin_psd, N, nfft_psd): csrc/plan.h nwin_psd, engine.cpp:463-465"""
    s32, t32 = np.float32(fs), np.float32(thop)
    nwin = int(_iround(np.float32(np.float32(t32 * np.float32(4.0)) * s32)))
    return nwin, nextpow2(0.03 * float(s32)), nextpow2(nwin)


def plan_values(f0, index, fs, thop):
    """(ws, centre) per frame: lp::spgmwin (float32 quotient and product, truncated) and lp::center"""
    f0 = np.asarray(f0, np.float32)
    s32, t32 = np.float32(fs), np.float32(thop)
    nwin = sizes(fs, thop)[0]
    v = f0 > 0
    per = (s32 / np.where(v, f0, np.float32(1.0)).astype(np.float32)).astype(np.float32)
    ws = np.where(v, (per * np.float32(3.0)).astype(np.float32).astype(np.int64), nwin)
    i32 = np.asarray(index).astype(np.float32)
    c = _iround(((i32 * t32).astype(np.float32) * s32).astype(np.float32))
    return ws.astype(np.int64), c


def frame_index(frm_off):
    frm_off = np.asarray(frm_off, np.int64)
    cnt = np.diff(frm_off)
    utt = np.repeat(np.arange(len(cnt)), cnt)
    return utt, np.arange(int(frm_off[-1])) - frm_off[utt]


def offsets(arrs):
    return np.concatenate([[0], np.cumsum([len(a) for a in arrs])]).astype(np.int64)


def hann(ws, periodic=False):
    if ws <= 1:
        return np.ones(max(ws, 0))
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(ws) / (ws if periodic else ws - 1))


def _core(xs, f0s, fs, thop, dtype, norm_base=None, bound=None, fault=None):
    """out [F][nfft_psd / 2 + 1] of `dtype`; bound = dict(eps, eps_fft, eps_x, ph): also B (float64 only)"""
    dtype = np.dtype(dtype).type
    nwin, N, npsd = sizes(fs, thop)
    nspec = npsd // 2 + 1
    nb = norm_base_product() if norm_base is None else norm_base
    frm_off = offsets(f0s)
    F = int(frm_off[-1])
    f0 = np.concatenate(f0s).astype(np.float32) if F else np.zeros(0, np.float32)
    utt, idx = frame_index(frm_off)
    ws_all, c_all = plan_values(f0, idx, fs, thop)
    f0n = np.where(f0 > 0, f0, np.float32(200.0)).astype(np.float64) / float(np.float32(fs))
    pick = (np.arange(nspec, dtype=np.int64) * N) // npsd
    q = np.arange(N)
    qq = np.minimum(q, N - q).astype(np.float64)
    out = np.zeros((F, nspec), dtype)
    B = np.zeros((F, nspec)) if bound else None
    for ws in np.unique(ws_all):
        ws = int(ws)
        fr = np.flatnonzero(ws_all == ws)
        half = ws // 2
        frames = np.zeros((len(fr), ws), dtype)
        for r, g in enumerate(fr):
            x = xs[int(utt[g])]
            base = int(c_all[g]) - half
            a, b = max(base, 0), min(base + ws, len(x))
            if a < b:
                frames[r, a - base:b - base] = x[a:b]
        fw = frames * hann(ws, periodic=fault == "periodic").astype(dtype)[None, :]
        pos = (np.arange(ws) - half) % N
        buf = np.zeros((len(fr), N), dtype)
        for s in range(0, ws, N):                                             # a window longer than N is time-aliased
            buf[:, pos[s:s + N]] += fw[:, s:s + N]
        X = sfft.fft(buf, axis=1)
        mag = np.abs(X)
        nrm = dtype(dtype(nb) / dtype(ws))
        L = np.log(mag * nrm + dtype(LOG_FLOOR))
        cep = sfft.ifft(L, axis=1).real
        xq = qq[None, :] * f0n[fr][:, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            lift64 = np.where(xq > 0, np.sin(np.pi * xq) / (np.pi * xq), 1.0)
            if fault == "lifter_bin":
                lift64 = np.where(xq > 0, np.sin(np.pi * xq) / (np.pi * (qq[None, :] + 1.0) * f0n[fr][:, None]), 1.0)
        env = sfft.fft(cep * lift64.astype(dtype), axis=1).real
        assert X.dtype == (np.complex128 if dtype == np.float64 else np.complex64) and L.dtype == dtype and env.dtype == dtype
        out[fr] = dtype(2.0) * env[:, (pick + 1) % N if fault == "pick" else pick]
        if bound:
            e, e_fft, e_x, ph = bound["eps"], bound["eps_fft"], bound["eps_x"], bound["ph"]
            rms_x = np.sqrt(np.mean(mag * mag, axis=1, keepdims=True))
            r = e_x * rms_x * nrm / (mag * nrm + LOG_FLOOR)
            t = -np.log1p(-np.minimum(r, 0.5))
            h = np.fft.ifft(lift64, axis=1).real
            conv = np.fft.ifft(np.fft.fft(np.abs(h), axis=1) * np.fft.fft(t, axis=1), axis=1).real
            H1 = np.abs(h).sum(axis=1)
            S = np.sqrt(np.mean(L * L, axis=1))
            Lmax = np.abs(L).max(axis=1)
            with np.errstate(invalid="ignore", divide="ignore"):
                per_q = np.where(xq > 0, 6.0 * e * np.abs(lift64) + e * np.abs(np.cos(np.pi * xq) - lift64) + ph * e / (np.pi * xq), 0.0)
            lift_term = (np.abs(cep) * per_q).sum(axis=1)
            A = 2.0 * (H1 * (4.0 * e * Lmax + 6.0 * e) + 2.0 * e_fft * S + lift_term)
            B[fr] = 2.0 * np.maximum(conv[:, pick], 0.0) + A[:, None]
    return (out, B) if bound else out


# Wrong variants of the restatement (host test only: the checker must notice each):
#   lifter_bin  the lifter's reciprocal taken one quefrency bin late: sin(pi qq f0n) / (pi (qq + 1) f0n)
#   periodic    Hann window with denominator ws instead of ws - 1
#   pick        the decimation one envelope bin late
FAULTS = ("lifter_bin", "periodic", "pick")


def spgm_env_ref(xs, f0s, fs, thop, dtype=np.float64, norm_base=None, fault=None):
    """plane 0, [total frames][nfft_psd / 2 + 1] of `dtype`, of the utterances xs (float32 samples) with the F0 tracks f0s.
    Per frame, vectorised over the frames of equal window length, with the kernel's integer plan: ws = nwin_psd when
    unvoiced, else int(float32(fs) / f0 * 3) in float32; centre lp::center; N = nextpow2(0.03 fs), nfft_psd =
    nextpow2(round(4 thop fs)); Hann 0.5 - 0.5 cos(2 pi j / (ws - 1)) (ws == 1: 1); samples outside [0, nx) of the frame's
    own utterance zero; zero-phase placement at (j - ws / 2) mod N, a longer window time-aliased; N-point FFT;
    L = log(|X| norm_base / ws + 1e-10); cep = real(ifft(L)); lifter sinc(qq f0n), qq = min(q, N - q), f0n = f0 / fs or
    200 / fs when unvoiced; forward FFT; out[j] = 2 env[(j N) // nfft_psd].  norm_base: the product's (engine.cpp:547)
    unless given.  dtype float64: the reference; float32: the yardstick restatement (module docstring)."""
    return _core(xs, f0s, fs, thop, dtype, norm_base, fault=fault)


def spgm_env_bound(xs, f0s, fs, thop, norm_base=None, eps=EPS, eps_fft=EPS_FFT, eps_x=EPS_X, ph=PH):
    """(ref, B): the float64 reference and the pointwise bound of the module docstring, formed from the reference alone.
    The defaults are float32's; tests/test_spgm_env_host.py passes float64's to bound the oracle's own rounding."""
    return _core(xs, f0s, fs, thop, np.float64, norm_base, bound=dict(eps=eps, eps_fft=eps_fft, eps_x=eps_x, ph=ph))


def spgm_env_check(got, ref, B, kappa=None):
    """(bad, stats) of rows `got` against the float64 reference under the bound B, all [F][nspec].
    bad: ("nonfinite", frame, point, value, 0), every one; ("point", frame, point, |error|, bound): the worst point of a
    frame that misses (a), with the count of its misses as a sixth entry; ("frame", frame, -1, rms error, kappa rms B): a
    frame that misses (b).  stats: frames, points, the worst pointwise ratio and where, the worst per-frame ratio and
    where, its median, the shares of points with B > 1e-3 and B > 1e-2, the largest B and the largest error."""
    kappa = KAPPA if kappa is None else kappa
    got = np.asarray(got, np.float64).reshape(ref.shape)
    fin = np.isfinite(got)
    err = np.abs(np.where(fin, got, 0.0) - ref)
    bad = [("nonfinite", int(g), int(j), float(got[g, j]), 0.0) for g, j in np.argwhere(~fin)]
    ratio = err / B
    rms_e = np.sqrt(np.mean(err * err, axis=1)); rms_b = np.sqrt(np.mean(B * B, axis=1))
    fratio = rms_e / rms_b
    for g in np.flatnonzero((ratio > 1.0).any(axis=1)):
        j = int(np.argmax(ratio[g]))
        bad.append(("point", int(g), j, float(err[g, j]), float(B[g, j]), int(np.count_nonzero(ratio[g] > 1.0))))
    for g in np.flatnonzero(~(fratio <= kappa)):
        bad.append(("frame", int(g), -1, float(rms_e[g]), float(kappa * rms_b[g])))
    st = dict(frames=int(ref.shape[0]), points=int(ref.size), kappa=float(kappa))
    if ref.size:
        w = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        gw = int(np.argmax(fratio))
        st.update(ratio_point=float(ratio[w]), ratio_point_at=(int(w[0]), int(w[1])), err_at_it=float(err[w]), bound_at_it=float(B[w]),
                  ratio_frame=float(fratio[gw]), ratio_frame_at=gw, ratio_frame_median=float(np.median(fratio)),
                  share_1e3=float(np.mean(B > 1e-3)), share_1e2=float(np.mean(B > 1e-2)), bound_max=float(B.max()),
                  bound_median=float(np.median(B)), err_max=float(err.max()))
    return bad, st


# =====================================================================
# The inputs of tests/test_gpu_spgm_env.py (built here so that tests/test_spgm_env_host.py sees the same ones)
# =====================================================================
# id: (fs, hop, the kernel the launcher takes, (logN, logF) or None for the LDS kernel)
CONFIGS = {
    "wf_9_0": (16000.0, 0.005, "k_spgm_env_wf", (9, 0)),
    "wf_9_1": (16000.0, 0.004, "k_spgm_env_wf", (9, 1)),
    "wf_10_0": (32000.0, 0.005, "k_spgm_env_wf", (10, 0)),
    "wf_10_1": (32000.0, 0.004, "k_spgm_env_wf", (10, 1)),
    "wf_10_2": (32000.0, 0.002, "k_spgm_env_wf", (10, 2)),
    "wf_11_0": (44100.0, 0.010, "k_spgm_env_wf", (11, 0)),
    "wf_11_1": (44100.0, 0.005, "k_spgm_env_wf", (11, 1)),
    "wf_11_2": (44100.0, 0.0025, "k_spgm_env_wf", (11, 2)),
    "lds_256": (8000.0, 0.005, "k_spgm_env", None),            # 256 points
    "lds_512_fold4": (16000.0, 0.002, "k_spgm_env", None),     # fold 4 at 512 points: no such instantiation
    "lds_fold8": (32000.0, 0.001, "k_spgm_env", None),         # fold 8
    "lds_psd_longer": (44100.0, 0.012, "k_spgm_env", None),    # PSD transform longer than N
    "lds_4096": (96000.0, 0.005, "k_spgm_env", None),          # 4096 points
}
K8 = dict(nchannel=2, chanfreq=[1500.0], maxnhar=60)            # band plans that fit under the Nyquist frequency
K16 = dict(nchannel=3, chanfreq=[1000.0, 3000.0])


def config_options(cid):
    """(fs, thop, analysis options besides f0_refine = 0 and the hop)"""
    fs, thop = CONFIGS[cid][:2]
    return fs, thop, dict(K8 if fs == 8000.0 else K16 if fs == 16000.0 else {})


NAMES = ("speech_a", "flat", "v200_unv", "low_f0", "short", "speech_b", "zero", "single", "speech_c", "flat2", "low_mix")
I_SPEECH, I_FLAT, I_V200, I_LOW, I_SHORT, I_SPEECH_B, I_ZERO, I_SINGLE, I_SPEECH_C, I_FLAT2, I_LOWMIX = range(11)
NFRM = (49, 8, 9, 6, 3, 24, 9, 1, 33, 2, 5)                     # 149 frames; odd and even counts
# the neighbours of `short` (an utterance shorter than one window) carry ten times its level
LEVEL = (1.0, 1.0, 1.0, 10.0, 1.0, 10.0, 0.0, 1.0, 1.0, 1.0, 1.0)
FLAT_F0 = 123.0
LOW_F0 = 50.0                                                   # below 3 fs / N (64.6 ... 93.75 Hz) at every rate
V200 = np.array([200.0, 0.0, 0.0, 200.0, 200.0, 200.0, 0.0, 0.0, 200.0], np.float32)
NOISE = 0.08                                                    # white floor under every signal (see spgm_env_inputs)


def _signal(seed, nfrm, fs, thop):
    """a make_speechlike signal of nfrm frames, ending half a hop after its last frame's centre, with a white floor"""
    from conftest import make_speechlike
    hop = float(np.float32(thop) * np.float32(fs))
    nx = int(_iround((nfrm - 0.5) * hop)) if nfrm > 1 else int(_iround(1.5 * hop))
    x, f0 = make_speechlike(seed, nx=max(nx, int(_iround(60 * hop))), fs=fs, thop=thop)
    rng = np.random.default_rng(9100 + seed)
    x = x + np.float32(NOISE) * rng.standard_normal(len(x)).astype(np.float32)
    return np.ascontiguousarray(x[:nx], np.float32), f0


def spgm_env_inputs(cid):
    """(xs, f0s) of configuration cid, float32 each; F0 is an input of the analysis (f0_refine = 0), so the tracks are chosen:
      speech_a, _b, _c  conftest.make_speechlike: voiced and unvoiced runs, an F0 that changes every frame (the seed cache
                        always misses); speech_a starts at the track's frame 6 so that its first frame is voiced
      flat, flat2       a constant F0: the cache hits for frame a and for frame b
      v200_unv          voiced frames of exactly 200.0 Hz beside unvoiced ones, in both orders within a pair and across
                        pairs: the same f0n bits, different window lengths
      low_f0, low_mix   50 Hz: the window is longer than the transform (time-aliased); low_mix pairs one with a short window
      short             100 samples, voiced - unvoiced - voiced, between neighbours of ten times its level
      zero              all-zero samples, voiced and unvoiced frames
      single            one frame: a pair with a missing second frame
    Every signal ends half a hop after its last frame's centre, so the last windows hang over the end as the first hang over
    the start.  The white floor of 0.08 (a third of the first harmonic) is a condition of the bound, not of the kernel.
    The lifter term of A weighs the cepstrum by 1 / (pi qq f0n), and make_speechlike's spectrum falls 40 dB from its 39th
    harmonic to its own floor of 0.004, a step whose cepstrum is large at low quefrency: with a floor of 0.02 the share
    of points with B > 1e-3 was 0.24 (wf_11_0, wf_11_1), 0.20 (lds_psd_longer) and 0.47 (lds_4096), over the cap of
    0.20, so that input was replaced; with 0.06 the largest share was 0.16, with 0.08 it is 0.016 (lds_4096)."""
    fs, thop = CONFIGS[cid][:2]
    xs, f0s = [], []
    for u, n in enumerate(NFRM):
        x, f0 = _signal(700 + u, max(n, 40) + 6, fs, thop)
        hop = float(np.float32(thop) * np.float32(fs))
        nx = int(_iround((n - 0.5) * hop)) if n > 1 else int(_iround(1.5 * hop))
        if u == I_SPEECH:
            f = f0[6:6 + n].copy(); x = x[int(_iround(6 * hop)):][:nx]
        elif u in (I_SPEECH_B, I_SPEECH_C):
            f = f0[:n].copy(); x = x[:nx]
        elif u in (I_FLAT, I_FLAT2):
            f = np.full(n, FLAT_F0, np.float32); x = x[:nx]
        elif u == I_V200:
            f = V200.copy(); x = x[:nx]
        elif u == I_LOW:
            f = np.full(n, LOW_F0, np.float32); x = x[:nx]
        elif u == I_LOWMIX:
            f = np.array([LOW_F0, 180.0, 0.0, LOW_F0, LOW_F0], np.float32); x = x[:nx]
        elif u == I_SHORT:
            f = np.array([150.0, 0.0, 150.0], np.float32); x = x[1000:1100]
        elif u == I_ZERO:
            f = np.array([120.0, 120.0, 0.0, 0.0, 120.0, 0.0, 120.0, 120.0, 120.0], np.float32); x = np.zeros(nx, np.float32)
        else:
            f = np.array([160.0], np.float32); x = x[:nx]
        assert len(f) == n
        xs.append(np.ascontiguousarray(x * np.float32(LEVEL[u]), np.float32)); f0s.append(np.asarray(f, np.float32))
    return xs, f0s


def loud_inputs(xs):
    """another signal per utterance at ten times the level: what a batch is analysed on first, so that a row the second
    analysis leaves unwritten holds a value far outside any bound"""
    out = []
    for u, x in enumerate(xs):
        rng = np.random.default_rng(8900 + u)
        out.append((3.0 + 3.0 * rng.standard_normal(len(x))).astype(np.float32))
    return out


def cache_pair(cid):
    """the utterances of test_bits_do_not_depend_on_neighbours_or_cache: (target, same, other).  `same` ends on an odd frame
    count -- its last pair holds one frame, whose seeds stay in the cache -- with the F0 bits and window length of the
    target's first frame; `other` ends on another F0."""
    fs, thop = CONFIGS[cid][:2]
    xt, _ = _signal(760, 12, fs, thop)
    ft = np.full(12, FLAT_F0, np.float32); ft[5:] = 171.0
    xa, _ = _signal(761, 7, fs, thop)
    fa = np.full(7, 97.0, np.float32); fa[-1] = FLAT_F0
    fb = np.full(7, 97.0, np.float32)
    return (xt, ft), (xa, fa), (xa.copy(), fb)
