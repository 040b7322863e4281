"""Rules C1 - C6 of llsm_gpu_batch_select_chain (llsm_gpu.h) restated in numpy, on top of tests/select_reference.py: the
reference of tests/test_select_chain_host.py and tests/test_gpu_select_chain.py.  Every operation is an elementwise numpy
operation in the dtype given, so float32 is bit-faithful to the rules (one rounding per operation, no contraction) and the
same code in float64 is the comparison chain.

  chain             CODE -> (utt, pos, cost, plane 10, plane 11)
  path_from_planes  (planes 10, 11) -> (utt, pos, cost, the follower frames rule C3 gives on the planes' own costs)
  joins_of          the joins of a result: frames whose bank frame does not continue the one before

t_off and b_off are the frame offsets of the target's and the bank's utterances, n_utt + 1 entries each (Batch.frm_off)."""
import numpy as np

import select_reference as sref

K = sref.K                                                          # near slots
S = 16                                                              # states per frame: K near and up to K followers
CAP = sref.CAP


def followers(f_prev, acc_prev, near_f, b_end):
    """C3: the parents (states of frame i - 1) of slots 8, 9, ... of frame i, in slot order.  f_prev [16] bank frames
    (-1 absent), acc_prev [16] as rule C5 left it, near_f [8] the near frames of frame i, b_end [N] the end (exclusive) of
    every bank frame's utterance"""
    pool = [a for a in range(S) if f_prev[a] >= 0 and f_prev[a] + 1 < b_end[f_prev[a]] and f_prev[a] + 1 not in near_f]
    # (acc, a) ascending: a float comparison, equal values (+infinity included) to the smaller a; acc is never NaN
    for n in range(1, len(pool)):                                   # insertion sort by strict float comparison: stable
        a = pool[n]; m = n
        while m > 0 and acc_prev[a] < acc_prev[pool[m - 1]]:
            pool[m] = pool[m - 1]; m -= 1
        pool[m] = a
    return pool[:K]


def join_row(B, v, f_prev, f_cur, b_end, first, count, voicing_cost, join_cost, join_weight, dtype):
    """C4: J [16][16] in dtype between the states of frame i - 1 and of frame i; absent entries 0"""
    J = np.zeros((S, S), dtype)
    ia = [a for a in range(S) if f_prev[a] >= 0]; ij = [j for j in range(S) if f_cur[j] >= 0]
    if not ia or not ij:
        return J
    fa = np.array([f_prev[a] for a in ia], np.int64); fb = np.array([f_cur[j] for j in ij], np.int64)
    has = fa + 1 < b_end[fa]
    s = np.where(has, fa + 1, fa)
    x = B[s][:, first:first + count]; y = B[fb][:, first:first + count]
    d = np.zeros((len(ia), len(ij)), dtype)
    with np.errstate(all="ignore"):
        for k in range(count):
            t = x[:, None, k] - y[None, :, k]
            d = d + t * t
        d = np.where(v[s][:, None] != v[fb][None, :], d + dtype(voicing_cost), d)
        val = dtype(join_cost) + dtype(join_weight) * sref.cap(d, dtype)
    natural = has[:, None] & (fb[None, :] == fa[:, None] + 1)
    J[np.ix_(ia, ij)] = np.where(natural, dtype(0), val)
    return J


def step(acc_prev, f_prev, J, c_cur, f_cur):
    """C5: (acc [16], back [16]) of frame i; absent states hold +infinity and 0"""
    dtype = c_cur.dtype.type
    pa = [a for a in range(S) if f_prev[a] >= 0]
    with np.errstate(all="ignore"):
        m = acc_prev[pa[0]] + J[pa[0]]; arg = np.full(S, pa[0], np.int64)
        for a in pa[1:]:                                            # a ascending: only a strictly smaller value replaces
            val = acc_prev[a] + J[a]
            better = val < m
            m = np.where(better, val, m); arg[better] = a
        acc = (m + c_cur).astype(dtype)
    live = np.asarray(f_cur) >= 0
    return np.where(live, acc, dtype(np.inf)).astype(dtype), np.where(live, arg, 0)


def walk_back(acc, frames, backs, bu, b_off, g0, utt, pos):
    """the end of C5, and C6: fills utt and pos of the utterance at g0; returns its cost"""
    present = [j for j in range(S) if frames[-1][j] >= 0]
    s = present[0]
    for j in present[1:]:
        if acc[j] < acc[s]:
            s = j
    total = acc[s]
    for i in range(len(frames) - 1, -1, -1):
        f = int(frames[i][s])
        utt[g0 + i] = bu[f]; pos[g0 + i] = np.float32(f - b_off[bu[f]])
        s = int(backs[i][s])
    return total


def chain(code_t, t_off, code_b, b_off, first, count, voicing_cost=0.0, join_cost=0.0, join_weight=1.0, skip_own=False,
          dtype=np.float32):
    """the whole chain: (utt int32 [T], pos float32 [T], cost [n_utt] in dtype, plane 10 [T][32], plane 11 [T][256])"""
    code_t = np.asarray(code_t); code_b = np.asarray(code_b)
    t_off = np.asarray(t_off, np.int64); b_off = np.asarray(b_off, np.int64)
    T = len(code_t)
    near = sref.candidates(code_t, t_off, code_b, b_off, first, count, voicing_cost, skip_own, dtype)   # C1
    B = code_b.astype(dtype); v = code_b[:, 0] > np.float32(0.5)
    bu = sref.frame_utt(b_off); b_end = b_off[bu + 1] if len(bu) else np.zeros(0, np.int64)
    p10 = np.zeros((T, 2 * S), dtype); p10[:, :S] = dtype(CAP); p10[:, S:] = -1
    p11 = np.zeros((T, S * S), dtype)
    utt = np.zeros(T, np.int32); pos = np.zeros(T, np.float32); total = np.zeros(len(t_off) - 1, dtype)
    for u in range(len(t_off) - 1):
        g0, n = int(t_off[u]), int(t_off[u + 1] - t_off[u])
        if n == 0:
            continue
        frames, backs = [], []
        acc = f_prev = None
        for i in range(n):
            g = g0 + i
            c = np.full(S, dtype(CAP), dtype); f = np.full(S, -1, np.int64)
            c[:K] = near[g, :K]; f[:K] = near[g, K:].astype(np.int64)
            if i == 0:                                              # C2
                acc = np.where(f >= 0, c, dtype(np.inf)).astype(dtype); back = np.zeros(S, np.int64)
            else:
                par = followers(f_prev, acc, list(f[:K]), b_end)    # C3
                for r, a in enumerate(par):
                    f[K + r] = f_prev[a] + 1
                if par:
                    fs = f[K:K + len(par)]
                    c[K:K + len(par)] = sref.cost(code_t[g:g + 1], code_b[fs], first, count, voicing_cost, dtype)[0]
                J = join_row(B, v, f_prev, f, b_end, first, count, voicing_cost, join_cost, join_weight, dtype)
                p11[g] = J.ravel()
                acc, back = step(acc, f_prev, J, c, f)
            p10[g, :S] = c; p10[g, S:] = f
            frames.append(f); backs.append(back); f_prev = f
        total[u] = walk_back(acc, frames, backs, bu, b_off, g0, utt, pos)
    return utt, pos, total, p10, p11


def path_from_planes(p10, p11, t_off, b_off):
    """C3's ranking and C5 - C6 rerun on given planes: (utt, pos, cost, want) where want [T][8] holds the bank frames rule
    C3 puts into slots 8 ... 15 of every frame, given the planes' own costs and joins up to the frame before (-1: none)"""
    p10 = np.asarray(p10); p11 = np.asarray(p11)
    dtype = p10.dtype.type
    t_off = np.asarray(t_off, np.int64); b_off = np.asarray(b_off, np.int64)
    bu = sref.frame_utt(b_off); b_end = b_off[bu + 1] if len(bu) else np.zeros(0, np.int64)
    T = len(p10)
    utt = np.zeros(T, np.int32); pos = np.zeros(T, np.float32); total = np.zeros(len(t_off) - 1, dtype)
    want = np.full((T, K), -1, np.int64)
    for u in range(len(t_off) - 1):
        g0, n = int(t_off[u]), int(t_off[u + 1] - t_off[u])
        if n == 0:
            continue
        frames, backs = [], []
        acc = f_prev = None
        for i in range(n):
            g = g0 + i
            c = p10[g, :S]; f = p10[g, S:].astype(np.int64)
            if i == 0:
                acc = np.where(f >= 0, c, dtype(np.inf)).astype(dtype); back = np.zeros(S, np.int64)
            else:
                par = followers(f_prev, acc, list(f[:K]), b_end)
                want[g, :len(par)] = [f_prev[a] + 1 for a in par]
                acc, back = step(acc, f_prev, p11[g].reshape(S, S), c, f)
            frames.append(f); backs.append(back); f_prev = f
        total[u] = walk_back(acc, frames, backs, bu, b_off, g0, utt, pos)
    return utt, pos, total, want


def joins_of(utt, pos, t_off, b_off):
    """per target utterance the frames i >= 1 whose bank frame is not the one after frame i - 1's in one bank utterance"""
    f = sref.flat(utt, pos, b_off)
    utt = np.asarray(utt)
    out = []
    for u in range(len(t_off) - 1):
        a, b = int(t_off[u]), int(t_off[u + 1])
        out.append(int(np.count_nonzero((np.diff(f[a:b]) != 1) | (utt[a + 1:b] != utt[a:b - 1]))) if b - a > 1 else 0)
    return np.array(out, np.int64)
