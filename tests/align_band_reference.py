"""Rules B1 - B4 of llsm_gpu_batch_align_band (llsm_gpu.h) restated in numpy: the reference of tests/test_align_band_host.py
and tests/test_gpu_align_band.py.  The band is plain Python integer arithmetic; the accumulation works on a full [na][nb]
plane of which only the cells inside the band are read or written, in the dtype of the plane, one elementwise numpy
operation per rule operation, so float32 is bit-faithful to the rules and float64 is the comparison chain.  Like
align_reference.accumulate it walks the anti-diagonals, on which the cells do not depend on each other."""
import numpy as np

from align_reference import dist, make  # noqa: F401  (B2 is D1; the generator of the pairs)


# ---------------------------------------------------------------- B1
def centers(na, nb):
    """c_i of every row: the diagonal rounded half up, in Python integers"""
    if na == 1:
        return [0]
    return [(2 * i * (nb - 1) + (na - 1)) // (2 * (na - 1)) for i in range(na)]


def rows(na, nb, band):
    """(lo, hi) of every row, int64 arrays"""
    c = centers(na, nb)
    return (np.array([max(0, x - band) for x in c], np.int64), np.array([min(nb - 1, x + band) for x in c], np.int64))


def connected(na, nb, band):
    lo, hi = rows(na, nb, band)
    return bool(np.all(lo[1:] <= hi[:-1] + 1) and hi[-1] == nb - 1)


def band_min(na, nb):
    """the least connected band, by trying them in turn"""
    band = 0
    while not connected(na, nb, band):
        band += 1
    return band


def to_band(D, band):
    """the plane [na][nb] in the band layout [na][2 band + 1]: entry q of row i is column c_i - band + q, +infinity where
    that column lies outside [lo_i, hi_i]"""
    na, nb = D.shape
    out = np.full((na, 2 * band + 1), np.inf, D.dtype)
    for i, c in enumerate(centers(na, nb)):
        lo, hi = max(0, c - band), min(nb - 1, c + band)
        out[i, lo - (c - band):hi - (c - band) + 1] = D[i, lo:hi + 1]
    return out


def from_band(P, nb):
    """the band layout [na][2 band + 1] back as a plane [na][nb]; the cells outside the band hold +infinity (no rule reads
    them)"""
    na, width = P.shape
    band = (width - 1) // 2
    D = np.full((na, nb), np.inf, P.dtype)
    for i, c in enumerate(centers(na, nb)):
        lo, hi = max(0, c - band), min(nb - 1, c + band)
        D[i, lo:hi + 1] = P[i, lo - (c - band):hi - (c - band) + 1]
    return D


# ---------------------------------------------------------------- B3
def accumulate(D, band, step_cost):
    """(acc, moves, inside) of the plane D in D's dtype; inside marks the cells of the band, the others are never touched"""
    dtype = D.dtype.type
    na, nb = D.shape
    assert connected(na, nb, band), (na, nb, band)
    lo, hi = rows(na, nb, band)
    step = dtype(step_cost)
    acc = np.full((na, nb), np.nan, dtype); mv = np.full((na, nb), -1, np.int8)
    inside = (np.arange(nb)[None, :] >= lo[:, None]) & (np.arange(nb)[None, :] <= hi[:, None])
    acc[0, 0] = D[0, 0]; mv[0, 0] = 0
    with np.errstate(all="ignore"):
        for s in range(1, na + nb - 1):
            i = np.arange(max(0, s - nb + 1), min(na - 1, s) + 1); j = s - i
            keep = inside[i, j]
            i, j = i[keep], j[keep]
            if not len(i):
                continue
            above = i > 0                                            # (index -1 wraps on row 0: masked by `above`)
            has = ((above & (j - 1 >= lo[i - 1]) & (j - 1 <= hi[i - 1]), acc[i - 1, j - 1]),
                   (above & (j >= lo[i - 1]) & (j <= hi[i - 1]), acc[i - 1, j] + step),
                   (j - 1 >= lo[i], acc[i, j - 1] + step))
            m = np.zeros(len(i), dtype); move = np.zeros(len(i), np.int8); have = np.zeros(len(i), bool)
            for number, (exists, value) in enumerate(has):
                take = exists & (~have | (value < m))                # the first that exists; a later one only if strictly smaller
                m[take] = value[take]; move[take] = number
                have |= exists
            assert have.all()                                        # a connected band: every cell has a predecessor inside
            acc[i, j] = m + D[i, j]; mv[i, j] = move
    return acc, mv, inside


# ---------------------------------------------------------------- B4
def path(mv):
    """the cells from (na - 1, nb - 1) back to (0, 0) along the moves"""
    na, nb = mv.shape
    i, j = na - 1, nb - 1
    cells = [(i, j)]
    while (i, j) != (0, 0):
        m = mv[i, j]
        assert m in (0, 1, 2) and len(cells) <= na + nb - 2, (i, j, m)
        if m != 2:
            i -= 1
        if m != 1:
            j -= 1
        assert i >= 0 and j >= 0
        cells.append((i, j))
    return cells


def positions(cells, na):
    """pos of rule D3 from the cells of a path"""
    lo = np.full(na, np.iinfo(np.int64).max, np.int64); hi = np.full(na, -1, np.int64)
    for i, j in cells:
        lo[i] = min(lo[i], j); hi[i] = max(hi[i], j)
    return (lo + hi).astype(np.float32) * np.float32(0.5)


def dtw(D, band, step_cost):
    """B3 - B4: (pos float32 [na], cost in D's dtype, the cells of the path) of the plane D"""
    acc, mv, _ = accumulate(np.asarray(D), band, step_cost)
    cells = path(mv)
    return positions(cells, D.shape[0]), acc[-1, -1], cells


def align(fa, fb, band, first, count, step_cost=0.0, voicing_cost=0.0, dtype=np.float32):
    """the whole chain: (pos, cost)"""
    return dtw(dist(fa, fb, first, count, voicing_cost, dtype), band, step_cost)[:2]
