"""Rules S1 - S5 of llsm_gpu_batch_select (llsm_gpu.h) restated in numpy: the reference of tests/test_select_host.py and
tests/test_gpu_select.py.  Every operation is an elementwise numpy operation in the dtype given, so float32 is bit-faithful
to the rules (one rounding per operation, no contraction) and the same code in float64 is the comparison chain.  Each
layer has its own entry point: candidates (CODE -> plane 7), joins ((CODE, plane 7) -> plane 8), path ((planes 7, 8) ->
utt, pos, cost); select is the whole chain.

t_off and b_off are the frame offsets of the target's and the bank's utterances, n_utt + 1 entries each (Batch.frm_off)."""
import numpy as np

import align_reference as aref

K = 8
CAP = np.float32(1e30)


def cap(d, dtype=np.float32):
    """S1: c = d if d < 1e30f, else 1e30f (NaN and infinity included)"""
    with np.errstate(all="ignore"):
        return np.where(d < dtype(CAP), d, dtype(CAP)).astype(dtype)


def cost(x, y, first, count, voicing_cost=0.0, dtype=np.float32):
    """S1: c(x[i], y[j]) for all rows of x [n][dim] and y [m][dim] -> [n][m]"""
    return cap(aref.dist(x, y, first, count, voicing_cost, dtype), dtype)


def frame_utt(off):
    off = np.asarray(off, np.int64)
    return np.repeat(np.arange(len(off) - 1), np.diff(off))


def candidates(code_t, t_off, code_b, b_off, first, count, voicing_cost=0.0, skip_own=False, dtype=np.float32, chunk=256):
    """S2: plane 7 [T][16] in dtype: c[0..7], then the bank frame indices; absent slots 1e30 and -1"""
    code_t = np.asarray(code_t); code_b = np.asarray(code_b)
    T, N = len(code_t), len(code_b)
    tu = frame_utt(t_off)
    b_off = np.asarray(b_off, np.int64)
    out = np.zeros((T, 16), dtype)
    for g0 in range(0, T, chunk):
        g1 = min(T, g0 + chunk)
        c = cost(code_t[g0:g1], code_b, first, count, voicing_cost, dtype)
        key = c.astype(np.float64)                                  # (exact; infinity marks a frame that is not eligible)
        if skip_own:
            f = np.arange(N)[None, :]
            u = tu[g0:g1, None]
            key[(f >= b_off[u]) & (f < b_off[u + 1])] = np.inf
        order = np.argsort(key, axis=1, kind="stable")[:, :K]       # stable: equal c in ascending f -- the order (c, f)
        rows = np.arange(g1 - g0)[:, None]
        there = np.isfinite(key[rows, order])
        n = order.shape[1]
        out[g0:g1, :K] = dtype(CAP); out[g0:g1, K:] = -1
        out[g0:g1, :n] = np.where(there, c[rows, order], dtype(CAP))
        out[g0:g1, K:K + n] = np.where(there, order, -1)
    return out


def joins(code_b, b_off, p7, t_off, first, count, voicing_cost=0.0, join_cost=0.0, join_weight=1.0, dtype=np.float32):
    """S3: plane 8 [T][64] in dtype from plane 7; entry 8 a + j"""
    code_b = np.asarray(code_b)
    B = code_b.astype(dtype)
    N, T = len(B), len(p7)
    bu = frame_utt(b_off)
    idx = np.asarray(p7)[:, K:].astype(np.int64)
    head = np.zeros(T, bool); head[np.asarray(t_off, np.int64)[:-1][np.diff(t_off) > 0]] = True
    fa = np.vstack([np.full((1, K), -1, np.int64), idx[:-1]])       # slot a of the frame before
    fa[head] = -1
    fb = idx
    fa0 = np.maximum(fa, 0); fb0 = np.maximum(fb, 0)
    nxt = np.minimum(fa0 + 1, N - 1)
    s = np.where((fa0 + 1 < N) & (bu[nxt] == bu[fa0]), fa0 + 1, fa0)
    x = B[s][:, :, first:first + count]; y = B[fb0][:, :, first:first + count]        # [T][8][count]
    d = np.zeros((T, K, K), dtype)
    with np.errstate(all="ignore"):
        for k in range(count):
            t = x[:, :, None, k] - y[:, None, :, k]
            d = d + t * t
        differ = (code_b[s][:, :, None, 0] > np.float32(0.5)) != (code_b[fb0][:, None, :, 0] > np.float32(0.5))
        d = np.where(differ, d + dtype(voicing_cost), d)
        c = cap(d, dtype)
        J = dtype(join_cost) + dtype(join_weight) * c
    natural = (fb[:, None, :] == fa[:, :, None] + 1) & (bu[fb0][:, None, :] == bu[fa0][:, :, None])
    absent = (fa[:, :, None] < 0) | (fb[:, None, :] < 0)
    J = np.where(natural | absent, dtype(0), J).astype(dtype)
    return J.reshape(T, K * K)


def path(p7, p8, t_off, b_off):
    """S4 - S5: (utt int32 [T], pos float32 [T], cost [n_utt] in the planes' dtype)"""
    p7 = np.asarray(p7); p8 = np.asarray(p8)
    dtype = p7.dtype.type
    t_off = np.asarray(t_off, np.int64); b_off = np.asarray(b_off, np.int64)
    bu = frame_utt(b_off)
    T = len(p7)
    utt = np.zeros(T, np.int32); pos = np.zeros(T, np.float32); total = np.zeros(len(t_off) - 1, dtype)
    for u in range(len(t_off) - 1):
        g0, n = int(t_off[u]), int(t_off[u + 1] - t_off[u])
        if n == 0:
            continue
        nu = int(np.count_nonzero(p7[g0, K:] >= 0))
        assert nu >= 1
        acc = p7[g0, :nu].copy()
        back = np.zeros((n, nu), np.int64)
        for i in range(1, n):
            J = p8[g0 + i].reshape(K, K)
            m = acc[0] + J[0, :nu]; arg = np.zeros(nu, np.int64)
            for a in range(1, nu):
                v = acc[a] + J[a, :nu]
                better = v < m
                m = np.where(better, v, m); arg[better] = a
            acc = (m + p7[g0 + i, :nu]).astype(dtype); back[i] = arg
        s = int(np.argmin(acc))                                     # the first of the least
        total[u] = acc[s]
        for i in range(n - 1, -1, -1):
            f = int(p7[g0 + i, K + s])
            utt[g0 + i] = bu[f]; pos[g0 + i] = np.float32(f - b_off[bu[f]])
            s = int(back[i, s])
    return utt, pos, total


def select(code_t, t_off, code_b, b_off, first, count, voicing_cost=0.0, join_cost=0.0, join_weight=1.0, skip_own=False,
           dtype=np.float32):
    """the whole chain: (utt, pos, cost, plane 7, plane 8)"""
    p7 = candidates(code_t, t_off, code_b, b_off, first, count, voicing_cost, skip_own, dtype)
    p8 = joins(code_b, b_off, p7, t_off, first, count, voicing_cost, join_cost, join_weight, dtype)
    return path(p7, p8, t_off, b_off) + (p7, p8)


def offsets(nfrm):
    return np.concatenate([[0], np.cumsum(nfrm)]).astype(np.int64)


def flat(utt, pos, b_off):
    """the flat bank frame of every (utt, pos)"""
    return np.asarray(b_off, np.int64)[np.asarray(utt)] + np.asarray(pos).astype(np.int64)
