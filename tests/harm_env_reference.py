"""Plain numpy restatement of the envelope analysis of the squared band signals, the checker built on it, and the inputs
both of its test modules use.

    plane 2 of llsm_gpu_batch_debug_plane (ce, [nchannel][total_samples]) + F0
        -> [short-time mean, harmonics 1 .. K of the Blackman-windowed frame]   (k_harm_env)
        -> EDC, NHAR_E, EENV_AMPL, EENV_PHSE

harm_env_ref restates layer0.c:425-458 with dsputils.c:117-124 (the mean), 145-169 (the harmonics) and 190 (the window
length).  No GPU, no libllsm2_amd, no oracle in this file: tests/test_harm_env_host.py proves harm_env_ref(float64)
against the float64 oracle before tests/test_gpu_harm_env.py judges the kernel with harm_env_check.  Offsets (nx_off,
frm_off) are cumulative, one entry more than there are utterances.

The metric.  Per (frame, channel), in float64:
    A0 = 2 sum_j w_j |x_j| / sum_j w_j     the level-free scale of a harmonic: every float32 error of the windowed sum is
                                           absolute against it (ce >= 0, so it is twice the windowed mean);
    M  = sum |x| over the mean's window / ndc.
Every harmonic k < K is ONE complex number:  eZ = |a_g e^{i phi_g} - a_64 e^{i phi_64}| / A0;  eD = |edc_g - edc_64| / M.

The bounds.  eZ <= 4 Y_Z(u) + 4 EPS,  eD <= 4 Y_D(u) + 2 EPS,  EPS = 2^-24.  Y_.(u): the largest value of the same metric
for the float32 yardstick (below) against float64 over utterance u -- all frames, channels, harmonics.  The margin 4 is
the project's (psd_stage_reference.kalman_check).  The additive terms are what the yardstick does not contain:
  * Z.  Storing an amplitude a costs half an ulp relative: at most EPS a.  Storing an angle of magnitude up to pi costs
    half an ulp relative, at most pi EPS / 2 in radians, which moves Z by at most (pi EPS / 2) a.  Together below
    2.1 EPS a <= 2.1 EPS A0 (a <= A0: |sum w x e^{..}| <= sum w |x|).  tests/test_harm_env_host.py holds the float64 rows
    rounded to float32 to exactly this.  The rest, 1.9 EPS A0, is sqrtf and atan2f on the device, each within about an
    ulp of its result.
  * D.  One division and one store, EPS each, of a value that is at most M (the host test: float64 rounded is within EPS).
The yardstick contains one rounding of each store already; the additive terms count them again, on the kernel's side.

The cap is a condition, not a measurement: no utterance's bound may exceed 2e-5 (eZ) or 1e-5 (eD), a fifth and a tenth
of the whole-chain contract (tests/gpu_common.py CONTRACT: 1e-4).  An input whose yardstick lifts a bound above that is
reported as a failure: the input is to be replaced, not the cap.

The float32 yardstick is the PLAIN form and nothing cleverer: window and phasors evaluated in float64 (phase reduced mod
one turn first) and rounded to float32, float32 products, float32 accumulation sequential in sample order (a cumulative
sum, not numpy's pairwise np.sum), the result scaled in float32.  It does not know how any kernel splits the sum: the
next kernel is judged by the same one."""
import numpy as np

EPS = 2.0 ** -24
MARGIN = 4.0
ADD_Z = 4.0 * EPS
ADD_D = 2.0 * EPS
CAP_Z = 2e-5
CAP_D = 1e-5

# Wrong variants of the restatement (host test only: the checker must notice each where it changes anything):
#   centre      every frame one sample late (analysis window and mean)
#   periodic    Blackman window with denominator n instead of n - 1
#   halfsample  phase referred to (n - 1) / 2, the put-back rotation left out
#   seed        the fundamental's phasor 1e-5 rad ahead at every sample: harmonic k is k 1e-5 rad off
#   live        row K - 1 zeroed where K < me (an off-by-one in the cut)
#   clip        a window that starts before sample 0 reads the first 8 in-range samples as zero
#   dcdiv       the mean divided by the number of in-range samples instead of ndc (differs at clipped ends only)
#   dcwin       a voiced frame's mean taken over the unvoiced window length
#   dcpair      odd ndc, voiced: the one sample of the mean's window without a mirror image about the analysis window's
#               centre (c0 + ndc / 2) taken from the other side (c0 - ndc / 2 - 1)
FAULTS = ("centre", "periodic", "halfsample", "seed", "live", "clip", "dcdiv", "dcwin", "dcpair")


def _iround(v):
    v = np.asarray(v, np.float64)
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)          # C round(): half away from zero


def plan_values(f0, nfrm_index, thop, fs, rel_winsize, me):
    """(c0, n, K, ndc) per frame from the float32 / float64 expressions of csrc/plan.h (center, hwin, nhar, dcwin).
    f0: float32 per frame, nfrm_index: the frame's index within its utterance.  n and K are 0 for unvoiced frames."""
    f0 = np.asarray(f0, np.float32)
    i32 = np.asarray(nfrm_index).astype(np.float32)
    t32, s32, r32 = np.float32(thop), np.float32(fs), np.float32(rel_winsize)
    c0 = _iround(((i32 * t32).astype(np.float32) * s32).astype(np.float32))
    v = f0 > 0
    fsafe = np.where(v, f0, np.float32(1.0)).astype(np.float32)
    per = (s32 / fsafe).astype(np.float32)
    n = np.where(v, _iround(((per * r32).astype(np.float32) / np.float32(2.0)).astype(np.float32)) * 2, 0)
    K = np.where(v, np.minimum(np.floor((per / np.float32(2.0)).astype(np.float32).astype(np.float64)).astype(np.int64), int(me)), 0)
    nd_u = _iround(np.float64(np.float32(t32 * np.float32(2.0))) * np.float64(s32))
    fz = np.where(f0 == 0, np.float32(1.0), f0).astype(np.float64)
    ndc = np.where(f0 == 0, nd_u, _iround((2.0 / fz) * np.float64(s32)))
    return c0, n.astype(np.int64), K.astype(np.int64), ndc.astype(np.int64)


def frame_index(frm_off):
    """(utterance, index within it) of every flat frame"""
    frm_off = np.asarray(frm_off, np.int64)
    cnt = np.diff(frm_off)
    utt = np.repeat(np.arange(len(cnt)), cnt)
    return utt, np.arange(int(frm_off[-1])) - frm_off[utt]


def blackman(n, periodic=False):
    if n <= 1:
        return np.ones(max(n, 0))
    t = 2.0 * np.pi * np.arange(n) / (n if periodic else n - 1)
    return 0.42 - 0.5 * np.cos(t) + 0.08 * np.cos(2.0 * t)


def _fetch(x, base, n, clip8=False):
    """x[..., base : base + n] with zeros outside [0, nx); clip8: if base < 0 the first 8 in-range samples read as 0"""
    nx = x.shape[-1]
    out = np.zeros(x.shape[:-1] + (max(n, 0),), x.dtype)
    a, b = max(base, 0), min(base + n, nx)
    if a < b:
        out[..., a - base:b - base] = x[..., a:b]
        if clip8 and base < 0:
            out[..., a - base:min(a - base + 8, b - base)] = 0
    return out


def _core(ce, nx_off, frm_off, f0, thop, fs, rel_winsize, me, dtype, fault=None, scales=False):
    dtype = np.dtype(dtype).type
    f64 = dtype == np.float64
    ce = np.asarray(ce)
    assert ce.ndim == 2
    nch = ce.shape[0]
    f0 = np.asarray(f0, np.float32)
    F = int(frm_off[-1])
    utt, idx = frame_index(frm_off)
    c0s, ns, Ks, ndcs = plan_values(f0, idx, thop, fs, rel_winsize, me)
    nd_unv = int(plan_values(np.zeros(1, np.float32), [0], thop, fs, rel_winsize, me)[3][0])
    mw = max(int(me), 0)
    nhar = np.zeros(F, np.int32)
    ampl = np.zeros((F, nch, mw), dtype); phse = np.zeros((F, nch, mw), dtype); edc = np.zeros((F, nch), dtype)
    A0 = np.zeros((F, nch)); Mm = np.zeros((F, nch))
    late = 1 if fault == "centre" else 0
    turn1s = f0.astype(np.float64) / np.float64(np.float32(fs))
    for g in range(F):
        u = int(utt[g])
        x = ce[:, int(nx_off[u]):int(nx_off[u + 1])]
        xw = x.astype(dtype)
        c0, n, K, ndc = int(c0s[g]) + late, int(ns[g]), int(Ks[g]), int(ndcs[g])
        voiced = f0[g] > 0
        # ---- the mean
        nd = nd_unv if (fault == "dcwin" and voiced) else ndc
        bdc = c0 - nd // 2 - (1 if (fault == "dcpair" and voiced and nd % 2 == 1) else 0)
        fr = _fetch(xw, bdc, nd, clip8=fault == "clip")
        div = nd
        if fault == "dcdiv":
            div = max(min(bdc + nd, x.shape[1]) - max(bdc, 0), 1)
        if nd > 0:
            s = fr.sum(axis=1) if f64 else np.cumsum(fr, axis=1, dtype=np.float32)[:, -1]
            edc[g] = s / dtype(div)
        if scales and ndc > 0:
            Mm[g] = np.abs(_fetch(x.astype(np.float64), int(c0s[g]) - ndc // 2, ndc)).sum(axis=1) / ndc
        if not voiced:
            continue
        nhar[g] = K
        base = c0 - n // 2
        w = blackman(n, periodic=fault == "periodic")
        if scales:
            w0 = blackman(n)
            A0[g] = 2.0 * (np.abs(_fetch(x.astype(np.float64), int(c0s[g]) - n // 2, n)) * w0).sum(axis=1) / w0.sum()
        if K <= 0 or n <= 0:
            continue
        fr = _fetch(xw, base, n, clip8=fault == "clip")                       # [nch][n]
        ref = (n - 1) / 2.0 if fault == "halfsample" else float(n // 2)
        tau = np.arange(n, dtype=np.float64) - ref
        k = np.arange(1, K + 1, dtype=np.float64)
        ph = (turn1s[g] * k)[:, None] * tau[None, :]                          # turns, [K][n]
        ph -= np.rint(ph)
        ang = 2.0 * np.pi * ph
        if fault == "seed":
            ang = ang + k[:, None] * 1e-5
        cr, sr = np.cos(ang), -np.sin(ang)                                    # e^{-i ang}
        if f64:
            wx = fr * w[None, :]
            re = wx @ cr.T; im = wx @ sr.T                                    # [nch][K]
            a = np.sqrt(re * re + im * im) * 2.0 / w.sum()
        else:
            w32 = w.astype(np.float32)
            wx = fr * w32[None, :]
            pr = wx[:, None, :] * cr.astype(np.float32)[None, :, :]
            pi = wx[:, None, :] * sr.astype(np.float32)[None, :, :]
            re = np.cumsum(pr, axis=2, dtype=np.float32)[:, :, -1]
            im = np.cumsum(pi, axis=2, dtype=np.float32)[:, :, -1]
            wsum = np.cumsum(w32, dtype=np.float32)[-1]
            a = np.sqrt(re * re + im * im) * (np.float32(2.0) / wsum)
        p = np.arctan2(im, re)
        if fault == "live" and K < me:
            a[:, K - 1] = 0; p[:, K - 1] = 0
        ampl[g, :, :K] = a; phse[g, :, :K] = p
    assert ampl.dtype == dtype and phse.dtype == dtype and edc.dtype == dtype
    if scales:
        return nhar, ampl, phse, edc, A0, Mm, Ks
    return nhar, ampl, phse, edc


def harm_env_ref(ce, nx_off, frm_off, f0, thop, fs, rel_winsize, me, dtype=np.float64, fault=None):
    """(nhar_e [F] int32, ampl [F][nch][me], phse [F][nch][me], edc [F][nch]) of `dtype` for all utterances.
    Frame centre round(i thop fs), n = round(fs / f0 rel / 2) 2, K = min(floor(fs / f0 / 2), me),
    ndc = round((f0 == 0 ? 2 thop : 2 / f0) fs) (plan_values); frame ce[c0 - n/2 + j], zero outside [0, nx); symmetric
    Blackman window; X_k = sum_j w_j x_j e^{-i 2 pi (f0 / fs) k (j - n/2)}, k = 1 .. K; ampl = |X_k| 2 / sum w,
    phse = atan2(Im, Re); rows beyond K and every row of an unvoiced frame exactly 0; edc = (sum of the ndc samples from
    c0 - ndc/2 on, zeros outside) / ndc.  dtype float64: the reference; float32: the yardstick (module docstring)."""
    return _core(ce, nx_off, frm_off, f0, thop, fs, rel_winsize, me, dtype, fault)


def harm_env_metric(got, ref64, A0, M, Ks):
    """(eZ [F][nch][me], eD [F][nch]) of rows `got` = (nhar_e, ampl, phse, edc) against the float64 rows; NaN where the
    scale is 0 or the harmonic is not live (k >= K)"""
    _, ag, pg, dg = got
    _, a64, p64, d64 = ref64
    ag = np.asarray(ag, np.float64).reshape(a64.shape); pg = np.asarray(pg, np.float64).reshape(a64.shape)
    dg = np.asarray(dg, np.float64).reshape(d64.shape)
    live = np.arange(a64.shape[2])[None, None, :] < np.asarray(Ks)[:, None, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        eZ = np.abs(ag * np.exp(1j * pg) - a64 * np.exp(1j * p64)) / A0[:, :, None]
        eZ = np.where(live & (A0[:, :, None] > 0), eZ, np.nan)
        eD = np.where(M > 0, np.abs(dg - d64) / M, np.nan)
    return eZ, eD


def harm_env_check(got, ce, nx_off, frm_off, f0, thop, fs, rel_winsize, me, judge_env=True):
    """Rows `got` = (nhar_e, ampl, phse, edc) computed from the plane `ce` against harm_env_ref(float64) of the same
    plane, under the metric and the bounds of the module docstring.  judge_env = False (HMPP, whose envelope rows come
    from another kernel): only edc and nhar_e.  Nothing is excluded; no share of values may miss.
    Returns (bad, stats).  bad: a list of (utterance, row, flat frame, channel, k, value, bound) -- row "eZ" / "eD": the
    worst value of an utterance over its bound (value = the error, plus the count as an eighth entry); "ampl" / "phse" /
    "edc": a non-finite value (every one listed); "nhar_e": a mismatch; "zero_ampl" / "zero_phse": a row that must be +0.0
    bits (k >= K, unvoiced, A0 == 0 or M == 0) and is not; "cap_z" / "cap_d": the utterance's bound is over its cap.
    stats: per utterance Y_Z, Y_D, bounds, the worst eZ / eD with their (frame, channel, k) and the ratios to the bound;
    overall the largest of each."""
    nh_g, a_g, p_g, d_g = got
    me = int(me)
    r64 = _core(ce, nx_off, frm_off, f0, thop, fs, rel_winsize, me, np.float64, scales=True)
    ref64, A0, M, Ks = r64[:4], r64[4], r64[5], r64[6]
    r32 = harm_env_ref(ce, nx_off, frm_off, f0, thop, fs, rel_winsize, me, np.float32)
    F, nch = ref64[3].shape
    nh_g = np.asarray(nh_g).reshape(F)
    d_g = np.asarray(d_g, np.float32).reshape(F, nch)
    if judge_env and me > 0:
        a_g = np.asarray(a_g, np.float32).reshape(F, nch, me); p_g = np.asarray(p_g, np.float32).reshape(F, nch, me)
    else:
        judge_env = False
        a_g, p_g = ref64[1].astype(np.float32), ref64[2].astype(np.float32)
    yZ, yD = harm_env_metric(r32, ref64, A0, M, Ks)
    with np.errstate(invalid="ignore"):
        eZ, eD = harm_env_metric((nh_g, np.where(np.isfinite(a_g), a_g, 0), np.where(np.isfinite(p_g), p_g, 0),
                                  np.where(np.isfinite(d_g), d_g, 0)), ref64, A0, M, Ks)
    live = np.arange(max(me, 0))[None, None, :] < Ks[:, None, None]
    bad, per = [], []
    tot = dict(ratio_z=0.0, ratio_d=0.0, err_z=0.0, err_d=0.0, y_z=0.0, y_d=0.0, values_z=0, values_d=0)
    for u in range(len(frm_off) - 1):
        lo, hi = int(frm_off[u]), int(frm_off[u + 1])
        if lo == hi:
            continue
        sl = slice(lo, hi)
        rec = dict(utt=u, frames=hi - lo)

        def nmax(a):
            return float(np.nanmax(a)) if a.size and np.any(~np.isnan(a)) else 0.0
        YZ, YD = (nmax(yZ[sl]) if judge_env else 0.0), nmax(yD[sl])
        bZ, bD = MARGIN * YZ + ADD_Z, MARGIN * YD + ADD_D
        rec.update(Y_Z=YZ, Y_D=YD, bound_z=bZ, bound_d=bD)
        if bZ > CAP_Z:
            bad.append((u, "cap_z", -1, -1, -1, bZ, CAP_Z))
        if bD > CAP_D:
            bad.append((u, "cap_d", -1, -1, -1, bD, CAP_D))
        # ---- counts
        for g in np.flatnonzero(nh_g[sl] != ref64[0][sl]):
            bad.append((u, "nhar_e", lo + int(g), -1, -1, int(nh_g[lo + g]), int(ref64[0][lo + g])))
        # ---- non-finite values, every one
        for name, arr in (("ampl", a_g), ("phse", p_g)) if judge_env else ():
            for w in np.argwhere(~np.isfinite(arr[sl])):
                bad.append((u, name, lo + int(w[0]), int(w[1]), int(w[2]), float(arr[lo + w[0], w[1], w[2]]), 0.0))
        for w in np.argwhere(~np.isfinite(d_g[sl])):
            bad.append((u, "edc", lo + int(w[0]), int(w[1]), -1, float(d_g[lo + w[0], w[1]]), 0.0))
        # ---- rows that must be +0.0: beyond K, unvoiced, and where the scale is zero
        if judge_env:
            must0 = ~live[sl] | (A0[sl] == 0)[:, :, None]
            for name, arr in (("zero_ampl", a_g), ("zero_phse", p_g)):
                bits = arr[sl].view(np.int32)
                strict = ~live[sl]                                    # not live: +0.0 BITS; live with A0 == 0: the value 0.0
                wrong = (strict & (bits != 0)) | (must0 & ~strict & ~(arr[sl] == 0))
                for w in np.argwhere(wrong):
                    bad.append((u, name, lo + int(w[0]), int(w[1]), int(w[2]), float(arr[lo + w[0], w[1], w[2]]), 0.0))
        for w in np.argwhere((M[sl] == 0) & ~(d_g[sl] == 0)):
            bad.append((u, "zero_edc", lo + int(w[0]), int(w[1]), -1, float(d_g[lo + w[0], w[1]]), 0.0))
        # ---- the metric
        for name, e, bound, fin in (("eZ", eZ[sl], bZ, np.isfinite(a_g[sl]) & np.isfinite(p_g[sl])), ("eD", eD[sl], bD, np.isfinite(d_g[sl]))):
            if name == "eZ" and not judge_env:
                rec.update(eZ=0.0, eZ_at=None, ratio_z=0.0)
                continue
            e = np.where(fin, e, np.nan)                              # (non-finite values are listed above)
            key = "z" if name == "eZ" else "d"
            if not np.any(~np.isnan(e)):
                rec.update({name: 0.0, name + "_at": None, "ratio_" + key: 0.0})
                continue
            w = np.unravel_index(int(np.nanargmax(e)), e.shape)
            at = (lo + int(w[0]), int(w[1]), int(w[2]) if len(w) > 2 else -1)
            worst = float(e[w])
            rec.update({name: worst, name + "_at": at, "ratio_" + key: worst / bound})
            tot["ratio_" + key] = max(tot["ratio_" + key], worst / bound); tot["err_" + key] = max(tot["err_" + key], worst)
            tot["values_" + key] += int(np.count_nonzero(~np.isnan(e)))
            if not worst <= bound:
                bad.append((u, name) + at + (worst, bound, int(np.count_nonzero(e > bound))))
        tot["y_z"] = max(tot["y_z"], YZ); tot["y_d"] = max(tot["y_d"], YD)
        per.append(rec)
    tot["utterances"] = per
    return bad, tot


# =====================================================================
# The inputs of tests/test_gpu_harm_env.py (built here so that tests/test_harm_env_host.py sees the same ones)
# =====================================================================
HMPP, HMCZT = 0, 1
# id: (fs, analysis options, the constant F0 of low_f0, of mid_f0, of high_f0)
CONFIGS = {
    "44k_default": (44100.0, dict(), 30.0, 80.0, 3000.0),                                           # <4,4>, LOWBIT 2, riding-along mean
    "44k_2ch_me8": (44100.0, dict(nchannel=2, chanfreq=[3000.0], maxnhar_e=8), 30.0, 80.0, 3000.0),  # <4,8>, LOWBIT 1, K = 7 < 8
    "44k_6ch_me5": (44100.0, dict(nchannel=6, chanfreq=[1000.0, 2000.0, 4000.0, 6000.0, 10000.0], maxnhar_e=5), 30.0, 80.0, 3000.0),
    "44k_1ch_me3": (44100.0, dict(nchannel=1, chanfreq=[], maxnhar_e=3), 30.0, 80.0, 3000.0),         # one live channel of four rows
    "44k_me0": (44100.0, dict(maxnhar_e=0), 30.0, 80.0, 3000.0),                                     # edc only
    "8k_2ch": (8000.0, dict(nchannel=2, chanfreq=[1500.0]), 30.0, 80.0, 1300.0),                     # single-trip windows, K = 3 < 4
    "96k": (96000.0, dict(), 60.0, 150.0, 3000.0),                                                    # long windows at speech F0
    "44k_hmpp": (44100.0, dict(hm_method=HMPP), 30.0, 80.0, 3000.0),                                 # edc and nhar_e only
    "44k_rel2": (44100.0, dict(rel_winsize=2.0), 30.0, 80.0, 3000.0),                                # n against ndc: the knife edge
    "44k_rel1p5": (44100.0, dict(rel_winsize=1.5), 30.0, 80.0, 3000.0),                              # the mean's window not inside
}
REL_CONFIGS = ("44k_rel2", "44k_rel1p5")
THOP = 0.005
DEFAULT_CF = [2000.0, 4000.0, 8000.0]
# the utterances of every configuration, in batch order; I_* index them
NAMES = ("speech_a", "low_f0", "mid_f0", "clipped", "high_f0", "short", "speech_b", "zero")
I_SPEECH, I_LOW, I_MID, I_CLIPPED, I_HIGH, I_SHORT, I_SPEECH_B, I_ZERO = range(8)
# the neighbours of the utterances shorter than their windows (low_f0, clipped, short): ten times their level
LEVEL = (10.0, 1.0, 10.0, 1.0, 10.0, 1.0, 10.0, 0.0)
# seeds of conftest.make_speechlike / make_utterance (speech_a: F0 90 ... 110 Hz, speech_b: 150 ... 205 Hz)
SEED = {I_SPEECH: 520, I_SPEECH_B: 523, I_LOW: 41, I_MID: 142, I_CLIPPED: 43, I_HIGH: 44}
NX_LOW = 1800                                            # samples of low_f0, at every rate (see harm_env_inputs)


def config_options(cid):
    """(fs, thop, analysis options with every default spelled out)"""
    fs, kw = CONFIGS[cid][:2]
    o = dict(nchannel=4, chanfreq=list(DEFAULT_CF), maxnhar_e=4, rel_winsize=4.0, hm_method=HMCZT)
    o.update(kw)
    return fs, THOP, o


def harm_env_inputs(cid):
    """(xs, f0s) of configuration cid, float32 each.  F0 is an input of the analysis, so the tracks are chosen:
      speech_a, speech_b  conftest.make_speechlike: voiced and unvoiced runs, moving F0 (both forms of the mean, odd and
                          even ndc)
      low_f0              constant 30 Hz (60 Hz at 96 kHz) in 1800 samples: at 44.1 kHz windows of 5880 samples, 23 trips of 64 x 4 pairs and
                          46 rotation steps to the pairs at the window's centre -- which are the ones inside the signal
      mid_f0              constant 80 Hz (150 Hz at 96 kHz), 0.15 s: the longest windows that lie inside their signal
      clipped             1500 samples at 44.1 kHz, 60 Hz: shorter than its analysis window, both ends clipped at once
      high_f0             constant 3000 Hz (1300 Hz at 8 kHz): windows of one trip, K below the default 4 / the 8 of me8
      short               100 samples, 3 frames, voiced - unvoiced - voiced
      zero                all-zero samples under a voiced track
    Lengths ragged so that the sample offsets take every residue mod 4.

    Why low_f0 is short.  The mean of a voiced frame runs over two periods -- 2940 samples at 30 Hz and 44.1 kHz -- and
    the sequential float32 sum of n positive terms sits 0.24 sqrt(n) EPS rms from float64 (measured on a 0.25 s
    utterance at 30 Hz: 14 EPS rms, 46 ... 53 EPS at the worst of its 200 values, a bound 4 Y + 2 EPS of 1.1e-5 ... 1.3e-5
    against the cap of 1e-5).  The cap is a condition, so that input was replaced: in 1800 samples no window holds more
    than 1800 non-zero terms (a zero adds exactly), the yardstick stays near 30 EPS, and the kernel still walks all 23
    trips of the 5880-sample window.  mid_f0 and the 96 kHz rows are chosen by the same rule: ndc <= 1300 samples."""
    from conftest import make_speechlike, make_utterance
    fs, _, f_lo, f_mid, f_hi = CONFIGS[cid]
    thop = THOP
    want = [int(0.3 * fs), NX_LOW, int(0.15 * fs), int(round(1500 * fs / 44100.0)), int(0.2 * fs), 100, int(0.22 * fs),
            int(round(10 * thop * fs))]
    nudge = {I_SPEECH: 1, I_MID: 2, I_HIGH: 3}           # the offset after these, mod 4 (the others keep their length)
    xs, f0s, off = [], [], 0
    for u, nx in enumerate(want):
        if u in nudge:
            nx += (nudge[u] - (off + nx)) % 4
        if u in (I_SPEECH, I_SPEECH_B):
            x, f0 = make_speechlike(SEED[u], nx=nx, fs=fs, thop=thop)
        elif u in (I_LOW, I_MID, I_HIGH, I_CLIPPED):
            f = {I_LOW: f_lo, I_MID: f_mid, I_HIGH: f_hi, I_CLIPPED: 60.0}[u]
            x = make_utterance(SEED[u], f, nx=nx, fs=fs)
            f0 = np.full(max(int(nx / fs / thop), 3), f, np.float32)
        elif u == I_SHORT:
            x = make_speechlike(599, nx=4000, fs=fs, thop=thop)[0][1000:1100].copy()
            f0 = np.array([150.0, 0.0, 150.0], np.float32)
        else:
            x = np.zeros(nx, np.float32)
            f0 = np.full(9, 120.0, np.float32)
        xs.append(np.ascontiguousarray(x * np.float32(LEVEL[u]), np.float32)); f0s.append(np.asarray(f0, np.float32))
        off += len(x)
    return xs, f0s


def loud_inputs(xs):
    """another signal per utterance at ten times the level (and off zero): what a batch is analysed on first, so that a
    row the second analysis leaves unwritten holds a value far outside any bound"""
    out = []
    for u, x in enumerate(xs):
        rng = np.random.default_rng(8800 + u)
        out.append((3.0 + 3.0 * rng.standard_normal(len(x))).astype(np.float32))
    return out


def offsets(arrs):
    return np.concatenate([[0], np.cumsum([len(a) for a in arrs])]).astype(np.int64)


def band_edges(opt, fs):
    cf, nch = opt["chanfreq"], opt["nchannel"]
    return [(0.0 if c == 0 else cf[c - 1], fs / 2.0 if c == nch - 1 else cf[c]) for c in range(nch)]
