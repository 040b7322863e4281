"""numpy restatement of llsm_gpu_batch_smooth (rules S1 - S9 of include/llsm_gpu.h) and of llsm_gpu_join_radii, written from
the header's words: float64 sums in ascending frame order with one addition per term (plain Python loops where the order
matters), the voicing-run shrinking of rule S2 by brute force, the distance rule of join_radii frame by frame against every
join.  Rows are dicts {array id: [total_frames, ...] array}, as tests/test_gpu_retime.py's rows_of gives them."""
import numpy as np

import libllsm2_amd as llsm

A = llsm
F0, RD, VTMAGN, PSD, EDC, ALL = 1, 2, 4, 8, 16, 31
MAX_RADIUS = 32
TRACKS = ((F0, A.A_F0), (RD, A.A_RD), (VTMAGN, A.A_VTMAGN), (PSD, A.A_PSD), (EDC, A.A_EDC))
# never written: the rows of rule S7, and AMPL and PHSE (rule S5)
NEVER = (A.A_VSPHSE, A.A_NVSPHSE, A.A_PSDRES, A.A_HAS_PSDRES, A.A_EENV_AMPL, A.A_EENV_PHSE, A.A_NHAR_E, A.A_PBPSYN,
         A.A_AMPL, A.A_PHSE)


def window(f0, o, n, i, R):
    """rule S2: [lo, hi] of frame i (within its utterance of n frames at flat offset o), by brute force: the largest
    interval around i inside [max(0, i - R), min(n - 1, i + R)] whose frames all have frame i's voicing"""
    voi = [bool(x != 0) for x in f0[o:o + n]]
    best = (i, i)
    for lo in range(max(0, i - R), i + 1):
        for hi in range(i, min(n - 1, i + R) + 1):
            if hi - lo > best[1] - best[0] and voi[lo:hi + 1].count(voi[i]) == hi - lo + 1:
                best = (lo, hi)
    return best


def mean(x, o, i, R, lo, hi):
    """rule S4 on track x (float32 [total_frames] or [total_frames, width]): float64, from 0.0, ascending j, one addition per
    term; then one division and one rounding to float32"""
    acc = np.zeros(x.shape[1:], np.float64)
    W = 0
    for j in range(lo, hi + 1):
        w = R + 1 - abs(j - i)
        acc = acc + np.float64(w) * x[o + j].astype(np.float64)
        W += w
    return (acc / np.float64(W)).astype(np.float32)


def smooth(rows, nfrm, radius, flags=ALL, in_place=False):
    """expected rows after llsm_gpu_batch_smooth(radius, flags) on `rows`, and the frames it changed the state of (bool
    [total_frames]: a window of more than one frame).  in_place: NOT the rule -- every frame reads what the frames before
    it have written (the sequential edit the snapshot rule excludes); for the test that tells the two apart."""
    out = {aid: np.array(v, copy=True) for aid, v in rows.items()}
    src = out if in_place else rows
    radius = np.asarray(radius)
    hit = np.zeros(len(radius), bool)
    o = 0
    for n in [int(v) for v in nfrm]:
        for i in range(n):
            g, R = o + i, int(radius[o + i])
            if R == 0:                                              # S1
                continue
            lo, hi = window(src[A.A_F0], o, n, i, R)
            if lo == hi:                                            # S3
                continue
            hit[g] = True
            voiced = src[A.A_F0][g] != 0
            new = {}
            for bit, aid in TRACKS:                                 # S5, S6
                if flags & bit and (voiced or bit in (PSD, EDC)):
                    new[aid] = mean(src[aid], o, i, R, lo, hi)
            for aid, v in new.items():
                out[aid][g] = v
            if voiced and flags & (F0 | RD | VTMAGN):
                out[A.A_NHAR][g] = 0
                out[A.A_HAS_HM][g] = 0
        o += n
    return out, hit


def join_radii(nfrm, pos_a, utt_a=None, reach=8):
    """(radius, n_joins) of llsm_gpu_join_radii, every frame against every join of its utterance"""
    pos = np.asarray(pos_a, np.float32)
    radius = np.zeros(len(pos), np.int32)
    joins = 0
    o = 0
    for n in [int(v) for v in nfrm]:
        at = []
        for i in range(1, n):
            same = utt_a is None or utt_a[o + i] == utt_a[o + i - 1]
            cont = same and pos[o + i] == np.float32(pos[o + i - 1] + np.float32(1))
            if not cont:
                at.append(i)
        joins += len(at)
        for i in range(n):
            if at:
                d = min(i - ij if i >= ij else ij - 1 - i for ij in at)
                radius[o + i] = max(0, reach - d)
        o += n
    return radius, joins
