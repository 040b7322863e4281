"""Rules L1 - L4 of llsm_gpu_batch_align_slope (llsm_gpu.h) restated in numpy: the reference of
tests/test_align_slope_host.py and tests/test_gpu_align_slope.py.  The region is plain Python integer arithmetic; the
accumulation works on a full [na][nb] plane of which only the cells of the region are written, in the dtype of the plane,
one elementwise numpy operation per rule operation, so float32 is bit-faithful to the rules and float64 is the comparison
chain.  The predecessors of a cell lie two and three anti-diagonals back, so the cells of an anti-diagonal do not depend on
each other and each is one vector operation, as in align_reference.accumulate."""
import numpy as np

from align_reference import dist, make  # noqa: F401  (L2 is D1; the generator of the pairs)


# ---------------------------------------------------------------- L1
def bound(na, nb):
    """None if the pair is admissible, else the bound that fails as (name of the larger side, its value, the limit)"""
    if nb - 1 > 2 * (na - 1):
        return "nb - 1", nb - 1, 2 * (na - 1)
    if na - 1 > 2 * (nb - 1):
        return "na - 1", na - 1, 2 * (nb - 1)
    return None


def admissible(na, nb):
    return na >= 1 and nb >= 1 and bound(na, nb) is None


def rows(na, nb):
    """(lo, hi) of every row, int64 arrays, in Python integers; lo > hi: no path stops on the row"""
    assert admissible(na, nb), (na, nb)
    lo = [max((i + 1) // 2, (nb - 1) - 2 * (na - 1 - i)) for i in range(na)]
    hi = [min(2 * i, (nb - 1) - (na - 1 - i + 1) // 2) for i in range(na)]
    return np.array(lo, np.int64), np.array(hi, np.int64)


def region(na, nb):
    """the cells of the region as a bool plane [na][nb]"""
    lo, hi = rows(na, nb)
    j = np.arange(nb)[None, :]
    return (j >= lo[:, None]) & (j <= hi[:, None])


# the moves: (rows back, columns back) of the predecessor, and of the cell passed on the way (None: none)
MOVES = (((1, 1), None), ((2, 1), (1, 0)), ((1, 2), (0, 1)))


# ---------------------------------------------------------------- L3
def accumulate(D, step_cost):
    """(acc, moves, inside) of the plane D in D's dtype; inside marks the cells of the region, the others are never
    written (acc NaN, move -1)"""
    D = np.asarray(D)
    dtype = D.dtype.type
    na, nb = D.shape
    inside = region(na, nb)
    step = dtype(step_cost)
    acc = np.full((na, nb), np.nan, dtype); mv = np.full((na, nb), -1, np.int8)
    acc[0, 0] = D[0, 0]; mv[0, 0] = 0
    with np.errstate(all="ignore"):
        for s in range(1, na + nb - 1):
            i = np.arange(max(0, s - nb + 1), min(na - 1, s) + 1); j = s - i
            keep = inside[i, j]
            i, j = i[keep], j[keep]
            if not len(i):
                continue
            m = np.zeros(len(i), dtype); move = np.zeros(len(i), np.int8); have = np.zeros(len(i), bool)
            for number, ((di, dj), mid) in enumerate(MOVES):
                ok = (i >= di) & (j >= dj)                           # (a negative index wraps: masked by `ok`)
                exists = ok & inside[i - di, j - dj]
                value = acc[i - di, j - dj]
                if mid is not None:
                    value = (value + D[i - mid[0], j - mid[1]]) + step
                take = exists & (~have | (value < m))                # the first that exists; a later one only if strictly smaller
                m[take] = value[take]; move[take] = number
                have |= exists
            assert have.all()                                        # every cell of the region has a predecessor inside
            acc[i, j] = m + D[i, j]; mv[i, j] = move
    return acc, mv, inside


# ---------------------------------------------------------------- L4
def path(mv):
    """(the cells from (na - 1, nb - 1) back to (0, 0), the cells passed between the ends of a move included; the
    number of moves)"""
    na, nb = mv.shape
    i, j, n = na - 1, nb - 1, 0
    cells = [(i, j)]
    while (i, j) != (0, 0):
        m = int(mv[i, j])
        assert m in (0, 1, 2) and n < min(na, nb) - 1, (i, j, m, n)
        (di, dj), mid = MOVES[m]
        if mid is not None:
            cells.append((i - mid[0], j - mid[1]))
        i -= di; j -= dj; n += 1
        assert i >= 0 and j >= 0
        cells.append((i, j))
    return cells, n


def positions(cells, na):
    """pos of rule L4 from the cells of a path"""
    lo = np.full(na, np.iinfo(np.int64).max, np.int64); hi = np.full(na, -1, np.int64)
    for i, j in cells:
        lo[i] = min(lo[i], j); hi[i] = max(hi[i], j)
    assert np.all(hi >= 0)                                           # every row is visited
    return (lo + hi).astype(np.float32) * np.float32(0.5)


def dtw(D, step_cost):
    """L3 - L4: (pos float32 [na], cost in D's dtype) of the plane D"""
    D = np.asarray(D)
    acc, mv, _ = accumulate(D, step_cost)
    return positions(path(mv)[0], D.shape[0]), acc[-1, -1]


def align(fa, fb, first, count, step_cost=0.0, voicing_cost=0.0, dtype=np.float32):
    """the whole chain: (pos, cost)"""
    return dtw(dist(fa, fb, first, count, voicing_cost, dtype), step_cost)


# ---------------------------------------------------------------- every path, for small planes
def brute_force(D, step_cost):
    """the least cost over all paths of moves 0 - 2 from (0, 0) to (na - 1, nb - 1), each summed in the order of L3, in D's
    dtype (exact on small integers), and the number of paths; (None, 0) if there is none"""
    D = np.asarray(D)
    dtype = D.dtype.type
    na, nb = D.shape
    step = dtype(step_cost)
    best, count = None, 0
    stack = [(0, 0, D[0, 0])]
    while stack:
        i, j, c = stack.pop()
        if (i, j) == (na - 1, nb - 1):
            count += 1
            best = c if best is None or c < best else best
            continue
        for (di, dj), mid in MOVES:
            ni, nj = i + di, j + dj
            if ni >= na or nj >= nb:
                continue
            m = c
            if mid is not None:
                m = (m + D[ni - mid[0], nj - mid[1]]) + step
            stack.append((ni, nj, m + D[ni, nj]))
    return best, count
