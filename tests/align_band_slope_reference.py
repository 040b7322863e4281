"""Rules K1 - K4 of llsm_gpu_batch_align_band_slope (llsm_gpu.h) restated in numpy: the reference of
tests/test_align_band_slope_host.py and tests/test_gpu_align_band_slope.py.  The region is plain Python integer arithmetic.
Everything else works on band planes [na][2 band + 1] (entry q of row i is column c_i - band + q, the layout of plane 13)
and never holds an [na][nb] array, so pairs of 17 000 frames fit.  The accumulation is in the dtype of the plane, one
elementwise numpy operation per rule operation, so float32 is bit-faithful to the rules and float64 is the comparison
chain.  Every predecessor of a cell lies in an earlier row, so a row is one vector operation."""
import numpy as np

from align_band_reference import centers, to_band, from_band  # noqa: F401  (the band of K1 is that of B1)
from align_slope_reference import admissible, positions  # noqa: F401  (L1's bounds; pos of L4 from the cells of a path)

EMPTY = (1, 0)


# ---------------------------------------------------------------- K1
def band_rows(na, nb, band):
    """(p, q) of every row: the band of rule B1, lists of Python integers"""
    c = centers(na, nb)
    return [max(0, x - band) for x in c], [min(nb - 1, x + band) for x in c]


def _join(pieces):
    """from the least lower end to the largest upper end of the non-empty pieces"""
    pieces = [(a, b) for a, b in pieces if a <= b]
    return (min(a for a, _ in pieces), max(b for _, b in pieces)) if pieces else EMPTY


def sweeps(na, nb, band):
    """(F, G): the forward and backward intervals of every row, lists of (lower, upper); EMPTY where there is none"""
    assert admissible(na, nb) and band >= 0, (na, nb, band)
    p, q = band_rows(na, nb, band)
    F = [(0, 0)]
    for i in range(1, na):
        a, b = F[i - 1]
        pieces = []
        if a <= b:
            pieces += [(max(a + 1, p[i]), min(b + 1, q[i])), (max(a + 2, p[i] + 1), min(b + 2, q[i]))]
        if i >= 2 and F[i - 2][0] <= F[i - 2][1]:
            c, d = F[i - 2]
            pieces.append((max(c + 1, p[i], p[i - 1]), min(d + 1, q[i], q[i - 1])))
        F.append(_join(pieces))
    G = [EMPTY] * na
    G[na - 1] = (nb - 1, nb - 1) if q[na - 1] >= nb - 1 else EMPTY
    for i in range(na - 2, -1, -1):
        a, b = G[i + 1]
        pieces = []
        if a <= b:
            pieces += [(max(a - 1, p[i]), min(b - 1, q[i])), (max(a - 2, p[i], p[i + 1] - 1), min(b - 2, q[i]))]
        if i + 2 < na and G[i + 2][0] <= G[i + 2][1]:
            c, d = G[i + 2]
            pieces.append((max(c - 1, p[i], p[i + 1] - 1), min(d - 1, q[i], q[i + 1] - 1)))
        G[i] = _join(pieces)
    return F, G


def region_rows(na, nb, band):
    """(lo, hi) of every row of the region as lists, an empty row as (1, 0); the band need not be connected"""
    F, G = sweeps(na, nb, band)
    lo, hi = [], []
    for (a, b), (c, d) in zip(F, G):
        l, h = max(a, c), min(b, d)
        if a > b or c > d or l > h:
            l, h = EMPTY
        lo.append(l); hi.append(h)
    return lo, hi


def connected(na, nb, band):
    lo, hi = region_rows(na, nb, band)
    return lo[-1] <= hi[-1]


def band_min(na, nb):
    """the least band that is connected for the slope pattern, by trying them in turn"""
    band = 0
    while not connected(na, nb, band):
        band += 1
    return band


def rows(na, nb, band):
    """(lo, hi) of every row of the region, int64 arrays; lo > hi: no path stops on the row"""
    lo, hi = region_rows(na, nb, band)
    assert lo[-1] <= hi[-1], (na, nb, band)
    return np.array(lo, np.int64), np.array(hi, np.int64)


# the moves: (rows back, columns back) of the predecessor, and of the cell passed on the way (None: none)
MOVES = (((1, 1), None), ((2, 1), (1, 0)), ((1, 2), (0, 1)))


# ---------------------------------------------------------------- K3
def accumulate(P, nb, step_cost):
    """(acc, moves, lo, hi) of the band plane P [na][2 band + 1] in P's dtype.  acc and moves are in the band layout; only
    the cells of the region are written (elsewhere acc NaN, move -1)"""
    P = np.asarray(P)
    dtype = P.dtype.type
    na, width = P.shape
    band = (width - 1) // 2
    lo, hi = region_rows(na, nb, band)
    assert lo[-1] <= hi[-1], (na, nb, band)
    p, q = band_rows(na, nb, band)
    off = [c - band for c in centers(na, nb)]
    step = dtype(step_cost)
    acc = np.full((na, width), np.nan, dtype); mv = np.full((na, width), -1, np.int8)
    acc[0, 0 - off[0]] = P[0, 0 - off[0]]; mv[0, 0 - off[0]] = 0

    def at(plane, i, j):                                             # plane[i][column j], clamped: masked by `exists`
        return plane[i, np.clip(j - off[i], 0, width - 1)]

    with np.errstate(all="ignore"):
        for i in range(1, na):
            if lo[i] > hi[i]:
                continue
            j = np.arange(lo[i], hi[i] + 1)
            cands = [((j - 1 >= lo[i - 1]) & (j - 1 <= hi[i - 1]), lambda: at(acc, i - 1, j - 1))]
            if i >= 2:
                cands.append(((j - 1 >= lo[i - 2]) & (j - 1 <= hi[i - 2]) & (j >= p[i - 1]) & (j <= q[i - 1]),
                              lambda: (at(acc, i - 2, j - 1) + at(P, i - 1, j)) + step))
            else:
                cands.append((np.zeros(len(j), bool), lambda: np.zeros(len(j), dtype)))
            cands.append(((j - 2 >= lo[i - 1]) & (j - 2 <= hi[i - 1]) & (j - 1 >= p[i]),
                          lambda: (at(acc, i - 1, j - 2) + at(P, i, j - 1)) + step))
            m = np.zeros(len(j), dtype); move = np.zeros(len(j), np.int8); have = np.zeros(len(j), bool)
            for number, (exists, value) in enumerate(cands):
                value = value()
                take = exists & (~have | (value < m))                # the first that exists; a later one only if strictly smaller
                m[take] = value[take]; move[take] = number
                have |= exists
            assert have.all(), (i, lo[i], hi[i])                     # every cell of the region has a candidate
            acc[i, j - off[i]] = m + at(P, i, j); mv[i, j - off[i]] = move
    return acc, mv, np.array(lo, np.int64), np.array(hi, np.int64)


# ---------------------------------------------------------------- K4
def path(mv, nb):
    """(the cells from (na - 1, nb - 1) back to (0, 0), the cells passed between the ends of a move included; the number
    of moves) along the moves of a band plane"""
    na, width = mv.shape
    band = (width - 1) // 2
    off = [c - band for c in centers(na, nb)]
    i, j, n = na - 1, nb - 1, 0
    cells = [(i, j)]
    while (i, j) != (0, 0):
        assert 0 <= j - off[i] < width, (i, j)
        m = int(mv[i, j - off[i]])
        assert m in (0, 1, 2) and n < min(na, nb) - 1, (i, j, m, n)
        (di, dj), mid = MOVES[m]
        if mid is not None:
            cells.append((i - mid[0], j - mid[1]))
        i -= di; j -= dj; n += 1
        assert i >= 0 and j >= 0
        cells.append((i, j))
    return cells, n


def dtw(P, nb, step_cost):
    """K3 - K4: (pos float32 [na], cost in P's dtype) of the band plane P"""
    P = np.asarray(P)
    na, width = P.shape
    band = (width - 1) // 2
    acc, mv, _, _ = accumulate(P, nb, step_cost)
    c_last = centers(na, nb)[-1]
    return positions(path(mv, nb)[0], na), acc[-1, nb - 1 - (c_last - band)]


def dist_band(fa, fb, band, first, count, voicing_cost, dtype=np.float32):
    """K2: rule D1 for the cells of the band, as a band plane [na][2 band + 1]; +infinity outside the rows of the band"""
    a = np.asarray(fa, dtype); b = np.asarray(fb, dtype)
    na, nb = len(a), len(b)
    width = 2 * band + 1
    col = np.array(centers(na, nb), np.int64)[:, None] - band + np.arange(width)[None, :]
    ok = (col >= 0) & (col < nb)
    col = np.clip(col, 0, nb - 1)
    d = np.zeros((na, width), dtype)
    with np.errstate(all="ignore"):
        for k in range(first, first + count):
            t = a[:, k, None] - b[col, k]
            d = d + t * t
        differ = (np.asarray(fa)[:, 0, None] > np.float32(0.5)) != (np.asarray(fb)[col, 0] > np.float32(0.5))
        d = np.where(differ, d + dtype(voicing_cost), d).astype(dtype)
    d[~ok] = np.inf
    return d


def align(fa, fb, band, first, count, step_cost=0.0, voicing_cost=0.0, dtype=np.float32):
    """the whole chain: (pos, cost)"""
    return dtw(dist_band(fa, fb, band, first, count, voicing_cost, dtype), len(fb), step_cost)


# ---------------------------------------------------------------- every cell and every path, for small planes
def allowed(i, j, m, na, nb, p, q):
    """whether move m into (i, j) has both ends and the passed cell inside the band (and the matrix)"""
    (di, dj), mid = MOVES[m]
    cells = [(i, j), (i - di, j - dj)] + ([(i - mid[0], j - mid[1])] if mid else [])
    return all(0 <= x < na and 0 <= y < nb and p[x] <= y <= q[x] for x, y in cells)


def reachable(na, nb, band):
    """(forward, backward): bool planes [na][nb] of the cells reached from (0, 0) and reaching (na - 1, nb - 1) by allowed
    moves, cell by cell (a row at a time: every move changes the row).  Nothing of the sweeps of K1 is used: a cell is
    reached if it lies in the band and one of the three moves into it starts from a reached cell and passes a cell of the
    band"""
    p, q = band_rows(na, nb, band)
    col = np.arange(nb)
    inb = np.zeros((na + 2, nb + 2), bool)                           # the band, with two rows and columns of padding
    for i in range(na):
        inb[i, :nb] = (col >= p[i]) & (col <= q[i])

    def back(x, k):                                                  # x[j - k], False before the first column
        return np.concatenate([np.zeros(k, bool), x[:len(x) - k]])

    fwd = np.zeros((na + 2, nb + 2), bool); fwd[0, 0] = inb[0, 0]
    for i in range(1, na):
        fwd[i] = inb[i] & (back(fwd[i - 1], 1) |                                        # move 0
                           (back(fwd[i - 2], 1) & inb[i - 1] if i >= 2 else False) |    # move 1 passes (i - 1, j)
                           (back(fwd[i - 1], 2) & back(inb[i], 1)))                      # move 2 passes (i, j - 1)
    bwd = np.zeros((na + 2, nb + 2), bool); bwd[na - 1, nb - 1] = inb[na - 1, nb - 1]
    for i in range(na - 2, -1, -1):
        nxt = lambda x, k: np.concatenate([x[k:], np.zeros(k, bool)])                    # x[j + k]
        # moves 1 and 2 out of (i, j) both pass (i + 1, j + 1), on the way to (i + 2, j + 1) and to (i + 1, j + 2)
        bwd[i] = inb[i] & (nxt(bwd[i + 1], 1) | (nxt(inb[i + 1], 1) & (nxt(bwd[i + 2], 1) | nxt(bwd[i + 1], 2))))
    return fwd[:na, :nb], bwd[:na, :nb]


def brute_force(D, band, step_cost):
    """the least cost over all paths of allowed moves from (0, 0) to (na - 1, nb - 1) of the full plane D [na][nb], each
    summed in the order of K3, in D's dtype (exact on small integers), and the number of paths; (None, 0) if there is none"""
    D = np.asarray(D)
    dtype = D.dtype.type
    na, nb = D.shape
    p, q = band_rows(na, nb, band)
    step = dtype(step_cost)
    best, count = None, 0
    stack = [(0, 0, D[0, 0])]
    while stack:
        i, j, c = stack.pop()
        if (i, j) == (na - 1, nb - 1):
            count += 1
            best = c if best is None or c < best else best
            continue
        for m, ((di, dj), mid) in enumerate(MOVES):
            ni, nj = i + di, j + dj
            if ni >= na or nj >= nb or not allowed(ni, nj, m, na, nb, p, q):
                continue
            v = c
            if mid is not None:
                v = (v + D[ni - mid[0], nj - mid[1]]) + step
            stack.append((ni, nj, v + D[ni, nj]))
    return best, count
