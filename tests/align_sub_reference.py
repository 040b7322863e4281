"""Rules Q1 - Q5 of llsm_gpu_batch_align_sub (llsm_gpu.h) restated in numpy: the reference of tests/test_align_sub_host.py
and tests/test_gpu_align_sub.py.  The region is plain Python integer arithmetic; the accumulation works on a full [na][nb]
plane, in the dtype of the plane, one elementwise numpy operation per rule operation, so float32 is bit-faithful to the rules
and the same code in float64 is the comparison chain.  Both patterns are one loop over a table of moves: the pattern of L3 is
align_slope_reference.MOVES, and D2 is the same loop over PLAIN, where the first candidate that exists is the diagonal, on
column 0 the upper one alone -- the forced border.  The predecessors of a cell lie one to three anti-diagonals back, so each
anti-diagonal is one vector operation, as in align_reference.accumulate."""
import numpy as np

from align_reference import dist, make
from align_slope_reference import MOVES

# D2's moves in the layout of MOVES: (rows back, columns back) of the predecessor, and whether step_cost is added
PLAIN = (((1, 1), False), ((1, 0), True), ((0, 1), True))


# ---------------------------------------------------------------- Q1
def admissible(na, nb, slope):
    return na >= 1 and nb >= 1 and (not slope or -(-(na - 1) // 2) <= nb - 1)


def rows(na, nb, slope):
    """(lo, hi) of every row, int64 arrays, in Python integers"""
    assert admissible(na, nb, slope), (na, nb, slope)
    lo = [-(-i // 2) if slope else 0 for i in range(na)]
    return np.array(lo, np.int64), np.full(na, nb - 1, np.int64)


def region(na, nb, slope):
    """the cells of the region as a bool plane [na][nb]"""
    lo, hi = rows(na, nb, slope)
    j = np.arange(nb)[None, :]
    return (j >= lo[:, None]) & (j <= hi[:, None])


# ---------------------------------------------------------------- Q3
def accumulate(D, step_cost, slope):
    """(acc, moves, inside) of the plane D in D's dtype; cells outside the region are never written (acc NaN, move -1),
    and row 0 has no moves (-1)"""
    D = np.asarray(D)
    dtype = D.dtype.type
    na, nb = D.shape
    inside = region(na, nb, slope)
    step = dtype(step_cost)
    acc = np.full((na, nb), np.nan, dtype); mv = np.full((na, nb), -1, np.int8)
    acc[0, :] = D[0, :]
    with np.errstate(all="ignore"):
        for s in range(1, na + nb - 1):
            i = np.arange(max(1, s - nb + 1), min(na - 1, s) + 1); j = s - i
            keep = inside[i, j]
            i, j = i[keep], j[keep]
            if not len(i):
                continue
            m = np.zeros(len(i), dtype); move = np.zeros(len(i), np.int8); have = np.zeros(len(i), bool)
            for number in range(3):
                if slope:
                    (di, dj), mid = MOVES[number]
                else:
                    (di, dj), stepped = PLAIN[number]
                ok = (i >= di) & (j >= dj)                           # (a negative index wraps: masked by `ok`)
                exists = ok & inside[i - di, j - dj]
                value = acc[i - di, j - dj]
                if slope and mid is not None:
                    value = (value + D[i - mid[0], j - mid[1]]) + step
                elif not slope and stepped:
                    value = value + step
                take = exists & (~have | (value < m))                # the first that exists; a later one only if strictly smaller
                m[take] = value[take]; move[take] = number
                have |= exists
            assert have.all()                                        # every cell of the region below row 0 has a predecessor inside
            acc[i, j] = m + D[i, j]; mv[i, j] = move
    return acc, mv, inside


# ---------------------------------------------------------------- Q4
def end_of(row, lo):
    """the smallest column of least acc of the last row from lo on; a NaN never replaces a candidate"""
    end = lo
    for j in range(lo + 1, len(row)):
        if row[j] < row[end]:
            end = j
    return end


# ---------------------------------------------------------------- Q5
def path(mv, end, slope):
    """(the cells from (na - 1, end) back to row 0, the cells passed between the ends of a move included; the number of
    moves)"""
    na, nb = mv.shape
    i, j, n = na - 1, end, 0
    cells = [(i, j)]
    while i > 0:
        m = int(mv[i, j])
        assert m in (0, 1, 2) and n < na - 1 + end, (i, j, m, n)
        if slope:
            (di, dj), mid = MOVES[m]
            if mid is not None:
                cells.append((i - mid[0], j - mid[1]))
        else:
            (di, dj), _ = PLAIN[m]
        i -= di; j -= dj; n += 1
        assert i >= 0 and j >= 0, (i, j)
        cells.append((i, j))
    return cells, n


def positions(cells, na):
    """pos of rules D3 / L4 from the cells of a path"""
    lo = np.full(na, np.iinfo(np.int64).max, np.int64); hi = np.full(na, -1, np.int64)
    for i, j in cells:
        lo[i] = min(lo[i], j); hi[i] = max(hi[i], j)
    assert np.all(hi >= 0)                                           # every row is visited
    return (lo + hi).astype(np.float32) * np.float32(0.5)


def dtw(D, step_cost, slope):
    """Q3 - Q5: (pos float32 [na], (begin, end), cost in D's dtype, last_row in D's dtype [nb]) of the plane D"""
    D = np.asarray(D)
    na, nb = D.shape
    acc, mv, _ = accumulate(D, step_cost, slope)
    lo = int(rows(na, nb, slope)[0][-1])
    end = end_of(acc[-1], lo)
    cells, _ = path(mv, end, slope)
    last = acc[-1].copy()
    last[:lo] = np.inf
    return positions(cells, na), (cells[-1][1], end), acc[-1, end], last


def align(fa, fb, first, count, step_cost=0.0, voicing_cost=0.0, slope=False, dtype=np.float32):
    """the whole chain: (pos, (begin, end), cost, last_row)"""
    return dtw(dist(fa, fb, first, count, voicing_cost, dtype), step_cost, slope)


# ---------------------------------------------------------------- every path, for small planes
def brute_force(D, step_cost, slope):
    """the least cost, over all paths of the pattern from any cell of row 0, of ending on each column of the last row, each
    path summed in the order of Q3, in D's dtype (exact on small integers): a list of nb costs, None where no path ends"""
    D = np.asarray(D)
    na, nb = D.shape
    step = D.dtype.type(step_cost)
    best = [None] * nb
    stack = [(0, j, D[0, j]) for j in range(nb)]
    while stack:
        i, j, c = stack.pop()
        if i == na - 1:
            best[j] = c if best[j] is None or c < best[j] else best[j]
            if slope or i == 0:                                      # (row 0 has no moves; under D2 a path may go on along the last row)
                continue
        for number in range(3):
            if slope:
                (di, dj), mid = MOVES[number]
            else:
                (di, dj), stepped = PLAIN[number]
            ni, nj = i + di, j + dj
            if ni >= na or nj >= nb or (i == 0 and di == 0):
                continue
            m = c
            if slope and mid is not None:
                m = (m + D[ni - mid[0], nj - mid[1]]) + step
            elif not slope and stepped:
                m = m + step
            stack.append((ni, nj, m + D[ni, nj]))
    return best


# ---------------------------------------------------------------- a query planted in a take
def plant(seed, na, nm, n0, n1, dim=24, noise=0.3):
    """a query of na frames and a take of n0 + nm + n1 frames that holds a warped rendition of it from frame n0 on, between
    n0 and n1 frames of another such trajectory: (A [na][dim], B [n0 + nm + n1][dim], truth [na] in frames of the take),
    float64"""
    A, M, truth = make(seed, na, nm, dim, noise)
    other = make(seed + 1000, 2, max(n0 + n1, 2), dim, noise)[1]
    B = np.concatenate([other[:n0], M, other[len(other) - n1:] if n1 else other[:0]])
    return A, B, truth + n0
