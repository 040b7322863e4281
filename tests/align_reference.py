"""Rules D1 - D3 of llsm_gpu_batch_align (llsm_gpu.h) restated in numpy: the reference of tests/test_align_host.py and
tests/test_gpu_align.py.  Every operation is an elementwise numpy operation in the dtype given, so float32 is bit-faithful
to the rules (one rounding per operation, no contraction) and the same code in float64 is the comparison chain.  dtw walks
the anti-diagonals, on which the cells do not depend on each other, so each is one vector operation."""
import numpy as np


def dist(fa, fb, first, count, voicing_cost, dtype=np.float32):
    """D1: the distance plane [na][nb] of the rows fa [na][dim] and fb [nb][dim]"""
    a = np.asarray(fa, dtype); b = np.asarray(fb, dtype)
    d = np.zeros((len(a), len(b)), dtype)
    with np.errstate(all="ignore"):
        for k in range(first, first + count):
            t = a[:, k, None] - b[None, :, k]
            d = d + t * t
        differ = (np.asarray(fa)[:, 0, None] > np.float32(0.5)) != (np.asarray(fb)[None, :, 0] > np.float32(0.5))
        return np.where(differ, d + dtype(voicing_cost), d).astype(dtype)


def accumulate(D, step_cost):
    """D2: (acc, moves) of the plane D in D's dtype"""
    dtype = D.dtype.type
    na, nb = D.shape
    step = dtype(step_cost)
    acc = np.zeros((na, nb), dtype); mv = np.zeros((na, nb), np.int8)
    acc[0, 0] = D[0, 0]
    with np.errstate(all="ignore"):
        for s in range(1, na + nb - 1):
            i = np.arange(max(0, s - nb + 1), min(na - 1, s) + 1); j = s - i
            up = acc[i - 1, j] + step                              # (index -1 wraps on a border: replaced below)
            lf = acc[i, j - 1] + step
            m = acc[i - 1, j - 1].copy(); move = np.zeros(len(i), np.int8)
            c = up < m; m[c] = up[c]; move[c] = 1
            c = lf < m; m[c] = lf[c]; move[c] = 2
            c = i == 0; m[c] = lf[c]; move[c] = 2                  # the borders are forced, not compared
            c = j == 0; m[c] = up[c]; move[c] = 1
            acc[i, j] = m + D[i, j]; mv[i, j] = move
    return acc, mv


def backtrack(mv):
    """D3: pos of the path through the moves, and the number of moves it took"""
    na, nb = mv.shape
    i, j, n = na - 1, nb - 1, 0
    lo = np.full(na, nb, np.int64); hi = np.full(na, -1, np.int64)
    while True:
        lo[i] = min(lo[i], j); hi[i] = max(hi[i], j)
        if i == 0 and j == 0:
            break
        m = mv[i, j]
        assert m in (0, 1, 2) and n <= na + nb - 2
        if m != 2:
            i -= 1
        if m != 1:
            j -= 1
        n += 1
    return (lo + hi).astype(np.float32) * np.float32(0.5), n


def dtw(D, step_cost):
    """D2 - D3: (pos float32 [na], cost in D's dtype) of the plane D"""
    acc, mv = accumulate(np.asarray(D), step_cost)
    return backtrack(mv)[0], acc[-1, -1]


def align(fa, fb, first, count, step_cost=0.0, voicing_cost=0.0, dtype=np.float32):
    """the whole chain: (pos, cost)"""
    return dtw(dist(fa, fb, first, count, voicing_cost, dtype), step_cost)


def make(seed, na, nb, dim, noise):
    """two renditions of one smooth trajectory in dim dimensions, the second on a warped clock: (A [na][dim], B [nb][dim],
    truth [na]: where in frames of B each frame of A belongs), float64"""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((12, dim)) * 10
    h = np.arange(1, 13)

    def traj(t):
        return (np.cos(np.pi * np.outer(t, h)) / np.sqrt(h)) @ c
    ta = np.linspace(0, 1, na)
    u = np.linspace(0, 1, nb)
    w = rng.uniform(-0.25, 0.25)
    tb = u + 0.5 * w * np.sin(np.pi * u) ** 2
    A = traj(ta) + noise * rng.standard_normal((na, dim))
    B = traj(tb) + noise * rng.standard_normal((nb, dim))
    return A, B, np.interp(ta, tb, np.arange(nb))
