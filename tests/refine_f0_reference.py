"""Plain numpy restatement of the F0 refinement, the checker built on it, and the inputs both of its test modules use.

    x (one utterance), F0 (float32 per frame) -> F0 refined in place                      (k_refine_f0)

refine_ref restates o_refine_f0 (oracle/llsm_oracle.c, the estimator of DESIGN.md "F0 refinement") in float64:  frame
centre c = round(i thop fs) (float32 products, plan.h center); fres = F0 / fs; nh = round(4 / fres); the frame
x[c - nh/2 + t], t < nh, zero outside [0, nx); the SYMMETRIC Hann window of nh - 1 points (denominator nh - 2); for
j = 1 .. 3 two single-bin sums one sample apart,
    C0_j = sum_{t < nh-1} w_t x_t e^{-i 2 pi j fres t},   C1_j = sum_{t < nh-1} w_t x_{t+1} e^{-i 2 pi j fres t},
f_j = arg(C1_j conj C0_j) / (2 pi j)  (cycles per sample; atan2(0, 0) = 0);  the gate |f_j - fres| < 0.1 fres;  the new
F0 = (mean of the accepted f_j) fs, or the old one -- the uploaded BITS -- where none is accepted.  No GPU, no
libllsm2_amd, no oracle in this file: tests/test_refine_f0_host.py proves refine_ref against the float64 oracle before
tests/test_gpu_refine_f0.py judges the kernel with refine_check.

The metric and the bound.  Per voiced frame with at least one accepted estimate (in float64), in Hz:
    |f_got - f_64| <= 4 Y_u + A,     A = 16 EPS f_64,  EPS = 2^-24,
Y_u: the largest |f_32 - f_64| of the utterance's frames, f_32 the float32 yardstick below.  The margin 4 is the project's
(harm_env_reference, psd_stage_reference).  A is what the kernel does after its four sums that the yardstick cannot stand
for, each step a relative error of the result, counted at one unit in the last place (2 EPS) where the operation is
only faithfully rounded and at half a unit (EPS) where it is correctly rounded:
    atan2f                      2 units (the documented bound of the device library)           4 EPS
    / 2 pi                      one division, and the float32 constant itself (0.5 EPS)        3 EPS
    / j                         one division                                                   2 EPS
    the mean over nf <= 3       two additions (EPS each) and one division                      4 EPS
    x fs, stored                one multiplication; its rounding IS the store                  1 EPS
                                                                                        sum   14 EPS  ->  16 EPS
The yardstick performs one rounding of each of these too; as in harm_env_reference the additive term counts them again,
on the kernel's side.  Nothing here is calibrated on the kernel.

Conditions on the INPUTS (not measurements; an input that fails one is to be replaced, never masked):
  * cap: no frame's bound may exceed 1e-3 F0, the "< 0.1 %" DESIGN.md / LAB.md state for the estimator.  Reported as
    "cap" by refine_check.
  * gate margin: for every voiced frame and every j the float64 gate distance | |f_j - fres| - 0.1 fres | fs (Hz) is at
    least 10 x that frame's bound, so that no correct float32 evaluation can decide the gate differently from float64
    (gate_margins; asserted by tests/test_refine_f0_host.py for every input).

Unvoiced frames (F0 == 0) and frames whose three estimates are all rejected must hold the uploaded bits.  Every
non-finite value is listed.  Nothing is excluded; no share of frames may miss.

The float32 yardstick is the PLAIN form: window and phasors evaluated in float64 (phase reduced mod one turn first) and
rounded to float32, float32 products, float32 accumulation sequential in sample order (np.cumsum), the cross product,
atan2, the divisions, the gate, the mean and the product with fs in float32.  It knows nothing about lanes."""
import numpy as np

from harm_env_reference import _iround, loud_inputs, offsets  # noqa: F401  (re-exported for the test modules)

EPS = 2.0 ** -24
MARGIN = 4.0
ADD_REL = 16.0 * EPS
CAP_REL = 1e-3
GATE_FACTOR = 10.0
GATE = 0.1

# Wrong variants of the restatement (host test only: the checker must notice each):
#   late       every frame one sample late
#   nh_points  the window computed for nh points (its first nh - 1 used) instead of nh - 1
#   periodic   Hann window with denominator nh - 1 instead of nh - 2
#   clamp      samples outside [0, nx) read as the nearest sample inside instead of zero
#   neighbour  samples outside [0, nx) read from the neighbouring utterances of the batch
#   gate9      the gate at 9 % of F0
#   gate11     the gate at 11 % of F0
#   div3       the sum of the accepted estimates always divided by 3
#   jplus1     the phase advance of harmonic j divided by j + 1
#   rewrite    a frame with no accepted estimate rewritten as fl(fl(F0 / fs) fs) instead of being left alone (a round
#              trip of the VALUE through float64 returns the same bits and is no error; one through the normalised
#              frequency is)
FAULTS = ("late", "nh_points", "periodic", "clamp", "neighbour", "gate9", "gate11", "div3", "jplus1", "rewrite")


def center(i, thop, fs):
    """round(i thop fs) with float32 products (csrc/plan.h center, oracle o_idx_center)"""
    a = np.float32(np.float32(i) * np.float32(thop))
    return int(_iround(np.float64(np.float32(a * np.float32(fs)))))


def hann(n, periodic=False):
    if n <= 1:
        return np.ones(max(n, 0))
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / (n if periodic else n - 1))


def _fetch(x, base, n, mode=None, left=None, right=None):
    """x[base : base + n] as float64; outside [0, nx): zero, or the nearest sample inside (mode "clamp"), or the samples of
    the batch around the utterance (mode "neighbour": left / right, zero beyond them)"""
    nx = len(x)
    idx = base + np.arange(n)
    if mode == "clamp" and nx > 0:
        return np.asarray(x, np.float64)[np.clip(idx, 0, nx - 1)]
    if mode == "neighbour":
        le = np.zeros(0) if left is None else np.asarray(left, np.float64)
        ri = np.zeros(0) if right is None else np.asarray(right, np.float64)
        cat = np.concatenate([le, np.asarray(x, np.float64), ri])
        k = idx + len(le)
        ok = (k >= 0) & (k < len(cat))
        out = np.zeros(n)
        out[ok] = cat[k[ok]]
        return out
    out = np.zeros(n)
    ok = (idx >= 0) & (idx < nx)
    out[ok] = np.asarray(x, np.float64)[idx[ok]]
    return out


def _refine(x, fs, f0, thop, dtype, fault=None, left=None, right=None):
    f32 = np.dtype(dtype) == np.float32
    T = np.float32 if f32 else np.float64
    f0 = np.asarray(f0, np.float32)
    n_f = len(f0)
    fsd = float(np.float32(fs))
    out = f0.astype(T)
    est = np.zeros((n_f, 3)); dist = np.zeros((n_f, 3)); acc = np.zeros((n_f, 3), bool)
    gate = {"gate9": 0.09, "gate11": 0.11}.get(fault, GATE)
    fetch_mode = fault if fault in ("clamp", "neighbour") else None
    for i in range(n_f):
        if f0[i] == 0:
            continue
        f = float(f0[i])
        fres = f / fsd
        nh = int(_iround(4.0 / fres))
        c = center(i, thop, fs) + (1 if fault == "late" else 0)
        n = nh - 1
        if fault == "nh_points":
            w = hann(nh)[:max(n, 0)]
        else:
            w = hann(n, periodic=fault == "periodic")
        xf = _fetch(x, c - nh // 2, nh, fetch_mode, left, right)
        t = np.arange(max(n, 0), dtype=np.float64)
        favg, nf = T(0), 0
        for j in (1, 2, 3):
            turns = (fres * j) * t
            if f32:
                ang = 2.0 * np.pi * (turns - np.rint(turns))
                co, si = np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)
                w32, x32 = w.astype(np.float32), xf.astype(np.float32)
                a, b = x32[:n] * w32, x32[1:n + 1] * w32
                s = [np.cumsum(p, dtype=np.float32)[-1] if n > 0 else np.float32(0) for p in (a * co, -a * si, b * co, -b * si)]
                c0r, c0i, c1r, c1i = s
                pr = c1r * c0r + c1i * c0i
                pi = c1i * c0r - c1r * c0i
                fj = np.arctan2(pi, pr) / np.float32(2.0 * np.pi) / np.float32(j + 1 if fault == "jplus1" else j)
                assert fj.dtype == np.float32
                d = abs(fj - np.float32(f) / np.float32(fs))
                ok = d < np.float32(f) * np.float32(gate) / np.float32(fs)
            else:
                ang = 2.0 * np.pi * turns
                co, si = np.cos(ang), np.sin(ang)
                a, b = xf[:n] * w, xf[1:n + 1] * w
                c0r, c0i, c1r, c1i = np.sum(a * co), -np.sum(a * si), np.sum(b * co), -np.sum(b * si)
                pr = c1r * c0r + c1i * c0i
                pi = c1i * c0r - c1r * c0i
                fj = np.arctan2(pi, pr) / (2.0 * np.pi) / (j + 1 if fault == "jplus1" else j)
                d = abs(fj - f / fsd)
                ok = d < f * gate / fsd
            est[i, j - 1], dist[i, j - 1], acc[i, j - 1] = float(fj), float(d), bool(ok)
            if ok:
                favg = T(favg + fj); nf += 1
        if nf > 0:
            out[i] = T(T(favg / T(3 if fault == "div3" else nf)) * T(fs))
        elif fault == "rewrite":
            out[i] = np.float32(np.float32(np.float32(f) / np.float32(fs)) * np.float32(fs))
    assert out.dtype == T
    return dict(f=out, est=est, dist=dist, acc=acc, nf=acc.sum(axis=1))


def refine_ref(x, fs, f0, thop):
    """float64 restatement of o_refine_f0 for one utterance.  Returns a dict: f [nfrm] the refined track (float64; the
    input value where nothing is accepted or the frame is unvoiced), est [nfrm][3] the per-harmonic estimates f_j in
    cycles per sample, dist [nfrm][3] the gate distances |f_j - F0 / fs|, acc [nfrm][3] the gate's decisions, nf."""
    return _refine(x, fs, f0, thop, np.float64)


def refine_f32(x, fs, f0, thop, fault=None, left=None, right=None):
    """the float32 yardstick (module docstring); fault: one of FAULTS (the host test's wrong variants)"""
    return _refine(x, fs, f0, thop, np.float32, fault, left, right)


def frame_bounds(r64, r32, f0):
    """(Y_u, bound [nfrm] in Hz) of one utterance from its float64 and float32 evaluations"""
    v = np.asarray(f0) > 0
    Y = float(np.max(np.abs(r32["f"].astype(np.float64) - r64["f"])[v])) if v.any() else 0.0
    return Y, MARGIN * Y + ADD_REL * np.abs(r64["f"])


def gate_margins(xs, f0s, fs, thop):
    """per utterance: the smallest ratio, over its voiced frames and j = 1 .. 3, of the float64 gate distance
    | |f_j - fres| - 0.1 fres | fs (Hz) to the frame's bound (inf where no frame is voiced), with the frame and j"""
    out = []
    for x, f0 in zip(xs, f0s):
        r64, r32 = refine_ref(x, fs, f0, thop), refine_f32(x, fs, f0, thop)
        _, bound = frame_bounds(r64, r32, f0)
        v = np.asarray(f0) > 0
        if not v.any():
            out.append((np.inf, -1, -1)); continue
        fres = np.asarray(f0, np.float64) / float(np.float32(fs))
        ratio = np.abs(r64["dist"] - GATE * fres[:, None]) * float(np.float32(fs)) / bound[:, None]
        ratio[~v] = np.inf
        w = np.unravel_index(int(np.argmin(ratio)), ratio.shape)
        out.append((float(ratio[w]), int(w[0]), int(w[1]) + 1))
    return out


def refine_check(got, xs, f0s, fs, thop):
    """The F0 row `got` (float32, all utterances, flat) of a batch whose waveforms were xs and whose uploaded F0 rows were
    f0s, against refine_ref of each utterance under the bound of the module docstring.
    Returns (bad, stats).  bad: a list of (utterance, kind, frame within it, value, bound) -- kind "err": the utterance's
    worst error / bound ratio is over 1 (value: the error in Hz, plus the count as a sixth entry); "bits": a frame that
    must hold the uploaded bits and does not; "nonfinite": every one; "cap": the utterance's largest bound / F0 is over
    1e-3.  stats: per utterance Y (Hz), Y_rel (relative to F0), the worst error and ratio, the largest bound / F0."""
    got = np.asarray(got, np.float32)
    frm_off = offsets(f0s)
    assert got.shape == (int(frm_off[-1]),), (got.shape, int(frm_off[-1]))
    bad, per = [], []
    tot = dict(ratio=0.0, err_rel=0.0, y_rel=0.0, bound_rel=0.0, frames=0)
    for u, (x, f0) in enumerate(zip(xs, f0s)):
        f0 = np.asarray(f0, np.float32)
        g = got[int(frm_off[u]):int(frm_off[u + 1])]
        if len(f0) == 0:
            continue
        r64, r32 = refine_ref(x, fs, f0, thop), refine_f32(x, fs, f0, thop)
        Y, bound = frame_bounds(r64, r32, f0)
        v = f0 > 0
        judged = v & (r64["nf"] > 0)
        fsafe = np.where(v, f0, 1.0).astype(np.float64)
        y_rel = float(np.max((np.abs(r32["f"].astype(np.float64) - r64["f"]) / fsafe)[v])) if v.any() else 0.0
        b_rel = float(np.max((bound / fsafe)[judged])) if judged.any() else 0.0
        rec = dict(utt=u, frames=len(f0), judged=int(judged.sum()), held=int((~judged).sum()), Y=Y, Y_rel=y_rel, bound_rel=b_rel,
                   err=0.0, err_rel=0.0, ratio=0.0, at=-1)
        if b_rel > CAP_REL:
            bad.append((u, "cap", -1, b_rel, CAP_REL))
        for i in np.flatnonzero(~np.isfinite(g)):
            bad.append((u, "nonfinite", int(i), float(g[i]), 0.0))
        for i in np.flatnonzero(~judged & (g.view(np.int32) != f0.view(np.int32))):
            bad.append((u, "bits", int(i), float(g[i]), float(f0[i])))
        fin = judged & np.isfinite(g)
        if fin.any():
            e = np.where(fin, np.abs(np.where(fin, g, 0).astype(np.float64) - r64["f"]), 0.0)
            ratio = np.where(fin, e / bound, 0.0)
            w = int(np.argmax(ratio))
            rec.update(err=float(e[w]), err_rel=float(e[w] / fsafe[w]), ratio=float(ratio[w]), at=w)
            if not ratio[w] <= 1.0:
                bad.append((u, "err", w, float(e[w]), float(bound[w]), int(np.count_nonzero(ratio > 1.0))))
        tot["ratio"] = max(tot["ratio"], rec["ratio"]); tot["err_rel"] = max(tot["err_rel"], rec["err_rel"])
        tot["y_rel"] = max(tot["y_rel"], y_rel); tot["bound_rel"] = max(tot["bound_rel"], b_rel); tot["frames"] += len(f0)
        per.append(rec)
    tot["utterances"] = per
    return bad, tot


# =====================================================================
# The inputs of tests/test_gpu_refine_f0.py (built here so that tests/test_refine_f0_host.py sees the same ones)
# =====================================================================
HMPP, HMCZT = 0, 1
# id: (fs, hop, the top of the high-F0 ramp -- its third harmonic stays under Nyquist --, F0 of `low`, (F0, dB) of `cond`)
CONFIGS = {
    "8k_5ms": (8000.0, 0.005, 1300.0, 30.0, (40.0, 30.0)),
    "16k_5ms": (16000.0, 0.005, 2600.0, 30.0, (40.0, 30.0)),
    "44k_5ms": (44100.0, 0.005, 3000.0, 30.0, (40.0, 20.0)),
    "44k_hop128": (44100.0, 128.0 / 44100.0, 3000.0, 30.0, (40.0, 20.0)),
    "96k_10ms": (96000.0, 0.010, 3000.0, 50.0, (100.0, 20.0)),
}
GATE_CONFIG = "44k_gate"
NAMES = ("speech_a", "low", "cond", "short", "high", "zero", "speech_b")
I_SPEECH, I_LOW, I_COND, I_SHORT, I_HIGH, I_ZERO, I_SPEECH_B = range(7)
# low and short sit between neighbours of ten times their level
LEVEL = (10.0, 1.0, 10.0, 1.0, 10.0, 0.0, 10.0)
SEED = {I_SPEECH: 620, I_SPEECH_B: 623, I_LOW: 51, I_COND: 52, I_HIGH: 54}
F_SHORT = 80.0
MAX_FRAMES = 64


def perturb(f0, rel=0.015):
    """the soak's pattern (tools/fuzz_soak.py): every frame off by +- rel, the sign that of sin(frame index)"""
    f0 = np.asarray(f0, np.float64)
    return (f0 * (1.0 + rel * np.sign(np.sin(np.arange(len(f0)))))).astype(np.float32)


def partials(nx, fs, f, mult, ampl, seed, sigma=0.0):
    """sum_k ampl_k cos(2 pi mult_k f t + phi_k) (+ white noise of deviation sigma), float32"""
    rng = np.random.default_rng(31000 + seed)
    t = np.arange(nx) / fs
    x = np.zeros(nx)
    for m, a in zip(mult, ampl):
        x += a * np.cos(2.0 * np.pi * m * f * t + rng.uniform(-np.pi, np.pi))
    if sigma:
        x += sigma * rng.standard_normal(nx)
    return x.astype(np.float32)


def nfrm_of(nx, fs, thop):
    return max(int(nx / fs / thop), 3)


def refine_inputs(cid):
    """(xs, f0s, names) of configuration cid, float32 each; f0s are the UPLOADED tracks (off the signal's pitch).
      speech_a, speech_b  conftest.make_speechlike, the track perturbed by +-1.5 % in the soak's pattern: voiced and
                          unvoiced runs, moving F0
      low                 30 Hz (50 Hz at 96 kHz) in 0.12 s (0.072 s), shorter than its window of 4 periods: every frame is
                          clipped, most at both ends
      cond                the conditioned case: a low fundamental 20 ... 30 dB under harmonics 2 and 3, noise 56 dB under
                          them; the phase advance 2 pi j F0 / fs is a few 1e-3 rad and the float32 cross product cancels.
                          Voiced only where the window lies inside the signal (clipping is low's job).  F0 and level per
                          configuration (CONFIGS) are the hardest that meet the two conditions of the module docstring: 30 Hz
                          at 96 kHz with the fundamental 30 dB down, the case this input stands for, lifts the plain
                          float32 yardstick to 2e-3 F0 (bound 8e-3 F0) and 30 Hz alone, at full level, to 5e-4 F0 (bound
                          2.2e-3 F0): over the cap, hence replaced (LAB.md has the scan)
      short               100 samples, 3 voiced frames at 80 Hz, between neighbours of ten times its level
      high                a ramp 1000 Hz ... 1300 / 2600 / 3000 Hz: windows of 25 ... 180 samples, at the top fewer than a
                          wavefront has lanes
      zero                all-zero samples under a voiced track: atan2(0, 0) = 0, every f_j = 0 is rejected, the bits stay
    Lengths ragged so that the sample offsets take every residue mod 4; no utterance over 0.35 s or 64 frames.
    GATE_CONFIG: gate_inputs()."""
    if cid == GATE_CONFIG:
        return gate_inputs()
    from conftest import make_speechlike, make_utterance
    fs, thop, f_hi, f_low, (f_cond, db_cond) = CONFIGS[cid]
    dur = min(0.35 if thop >= 0.01 else 0.3, MAX_FRAMES * thop)
    want = [int(dur * fs), int(0.12 * 30.0 / f_low * fs), int(dur * fs), 100, int(min(0.1, dur) * fs), int(round(9 * thop * fs)) + 7,
            int(min(0.27, 0.9 * dur) * fs)]
    nudge = {I_SPEECH: 1, I_LOW: 2, I_COND: 3}           # the offset after these, mod 4
    xs, f0s, off = [], [], 0
    for u, nx in enumerate(want):
        if u in nudge:
            nx += (nudge[u] - (off + nx)) % 4
        if u in (I_SPEECH, I_SPEECH_B):
            x, f0 = make_speechlike(SEED[u], nx=nx, fs=fs, thop=thop)
            f0 = perturb(f0)
        elif u == I_LOW:
            x = make_utterance(SEED[u], f_low, nx=nx, fs=fs)
            f0 = perturb(np.full(nfrm_of(nx, fs, thop), f_low))
        elif u == I_COND:
            x = partials(nx, fs, f_cond, (1, 2, 3), (0.3 * 10.0 ** (-db_cond / 20.0), 0.3, 0.3), SEED[u], sigma=0.0005)
            f0 = perturb(np.full(nfrm_of(nx, fs, thop), f_cond))
            f0 = np.where(inside(f0, nx, fs, thop), f0, 0.0).astype(np.float32)
        elif u == I_SHORT:
            x = make_speechlike(599, nx=4000, fs=fs, thop=thop)[0][1000:1100].copy()
            f0 = perturb(np.full(3, F_SHORT))
        elif u == I_HIGH:
            n_f = nfrm_of(nx, fs, thop)
            track = np.linspace(1000.0, f_hi, n_f)
            fsamp = np.interp(np.arange(nx) / fs, np.arange(n_f) * thop, track)
            ph = 2.0 * np.pi * np.cumsum(fsamp) / fs
            rng = np.random.default_rng(31000 + SEED[u])
            x = sum((0.3 / k) * np.cos(k * ph + rng.uniform(-np.pi, np.pi)) for k in (1, 2, 3)) + 0.002 * rng.standard_normal(nx)
            f0 = perturb(track)
        else:
            x = np.zeros(nx, np.float32)
            f0 = (120.0 + 1.7 * np.arange(9)).astype(np.float32)          # nine values: nine sets of bits to keep
        xs.append(np.ascontiguousarray(np.asarray(x, np.float32) * np.float32(LEVEL[u]), np.float32))
        f0s.append(np.ascontiguousarray(f0, np.float32))
        off += len(xs[-1])
    return xs, f0s, NAMES


# The gate cases: three exact partials at (m1, m2, m3) x 200 Hz, no noise, 44.1 kHz; the uploaded F0 is `up` x 200 Hz.
#   name: (multipliers, up, the j accepted in every frame whose window lies inside the signal)
F_GATE = 200.0
GATE_CASES = {
    "acc_up8": ((1.0, 2.0, 3.0), 1.08, (1, 2, 3)),               # the signal 7.4 % under the uploaded F0
    "acc_dn95": ((1.0, 2.0, 3.0), 1.0 / 1.095, (1, 2, 3)),       # 9.5 % over it: a gate at 9 % would reject
    "rej_13": ((1.0, 2.0, 3.0), 1.0 / 0.865, ()),                # 13.5 % under: all rejected, bits unchanged
    "rej_105": ((1.0, 2.0, 3.0), 1.0 / 0.895, ()),               # 10.5 % under: a gate at 11 % would accept
    "only_23": ((1.2, 2.0, 3.0), 1.015, (2, 3)),                 # partial 1 at 1.2 F0
    "only_3": ((1.2, 2.4, 3.0), 1.015, (3,)),                    # partials 1 and 2 displaced
    "only_2": ((1.2, 2.0, 3.6), 0.985, (2,)),                    # partials 1 and 3 displaced
    "only_1": ((1.0, 2.6, 3.9), 1.015, (1,)),                    # partials 2 and 3 displaced
}


def gate_inputs():
    fs, thop = 44100.0, 0.005
    xs, f0s, off = [], [], 0
    for k, (name, (mult, up, _)) in enumerate(GATE_CASES.items()):
        nx = int(0.12 * fs)
        nx += ((k + 1) - (off + nx)) % 4
        x = partials(nx, fs, F_GATE, mult, (0.3, 0.15, 0.1), 70 + k)
        xs.append(np.ascontiguousarray(x * np.float32(10.0 if k % 2 else 1.0), np.float32))
        f0s.append(np.full(nfrm_of(nx, fs, thop), F_GATE * up, np.float32))
        off += nx
    return xs, f0s, tuple(GATE_CASES)


def config_rate(cid):
    return (44100.0, 0.005) if cid == GATE_CONFIG else CONFIGS[cid][:2]


def inside(f0, nx, fs, thop):
    """per frame: its window [c - nh/2, c - nh/2 + nh) lies inside [0, nx) (False for unvoiced frames)"""
    out = np.zeros(len(f0), bool)
    for i, f in enumerate(np.asarray(f0, np.float32)):
        if f > 0:
            nh = int(_iround(4.0 / (float(f) / float(np.float32(fs)))))
            b = center(i, thop, fs) - nh // 2
            out[i] = b >= 0 and b + nh <= nx
    return out


# ---- downstream of the refined track (stages B and C of tests/test_gpu_refine_f0.py) ----
# id: (fs, hop, analysis options)
DOWN_CONFIGS = {
    "8k_2ch": (8000.0, 0.005, dict(nchannel=2, chanfreq=[1500.0], maxnhar=60)),     # tests/test_gpu_configs.py "8k_2ch", HMCZT
    "44k_hmpp": (44100.0, 0.005, dict(hm_method=HMPP)),
}
# the utterance whose harmonic count depends on the refinement: 8 kHz, the signal at 199 Hz (floor(8000 / 199 / 2) = 20),
# uploaded at 202 Hz (19)
NHAR_TRUE, NHAR_UP = 199.0, 202.0


def downstream_inputs(cid):
    """(xs, f0s): a make_speechlike utterance with its track perturbed, and for "8k_2ch" the nhar-crossing one"""
    from conftest import make_speechlike, make_utterance
    fs, thop, _ = DOWN_CONFIGS[cid]
    x, f0 = make_speechlike(631, nx=int(0.35 * fs), fs=fs, thop=thop)
    xs, f0s = [x], [perturb(f0)]
    if cid == "8k_2ch":
        nx = int(0.2 * fs) + 1
        xs.append(make_utterance(61, NHAR_TRUE, nx=nx, fs=fs))
        f0s.append(np.full(nfrm_of(nx, fs, thop), NHAR_UP, np.float32))
    return xs, f0s


# stage C: uploaded 100 Hz; first waveform at 92 Hz, second at 84.6 Hz, 44.1 kHz.  0.9 x 100 Hz has a window of 1960
# samples (2048-point transform), 84.6 Hz one of 2085 (4096): the analysis window crosses a power of two between the
# margin taken from the UPLOAD and the twice-refined value.
STATE_FS, STATE_THOP, STATE_UP, STATE_STEP = 44100.0, 0.005, 100.0, 0.92


def state_inputs():
    """(x1, x2, f0): the two waveforms and the uploaded track of stage C"""
    from conftest import make_utterance
    nx = int(0.3 * STATE_FS)
    x1 = make_utterance(71, STATE_UP * STATE_STEP, nx=nx, fs=STATE_FS)
    x2 = make_utterance(72, STATE_UP * STATE_STEP * STATE_STEP, nx=nx, fs=STATE_FS)
    return x1, x2, np.full(nfrm_of(nx, STATE_FS, STATE_THOP), STATE_UP, np.float32)
