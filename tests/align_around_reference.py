"""Rules A1 - A3 of llsm_gpu_batch_align_around (llsm_gpu.h) restated in numpy: the reference of
tests/test_align_around_host.py and tests/test_gpu_align_around.py.  The line, the band and the region are plain Python
integer arithmetic: rows, sweeps, accumulate and path of the four other references restated for a given centre line c.
The planes are band planes [na][2 band + 1] (entry q of row i is column c_i - band + q, the layout of plane 14).  The
accumulation is in the dtype of the plane, one elementwise numpy operation per rule operation, so float32 is bit-faithful to
the rules and float64 is the comparison chain."""
import numpy as np

from align_reference import dist, make  # noqa: F401  (A2 is D1; the generator of the pairs)
from align_band_reference import centers  # noqa: F401  (the line that gives the two straight calls)
from align_slope_reference import admissible, positions  # noqa: F401  (L1's bounds; pos from the cells of a path)

EMPTY = (1, 0)
# slope = 1: (rows back, columns back) of the predecessor, and of the cell passed on the way (None: none)
MOVES = (((1, 1), None), ((2, 1), (1, 0)), ((1, 2), (0, 1)))
# slope = 0: the predecessors of B3
PLAIN = ((1, 1), (1, 0), (0, 1))


# ---------------------------------------------------------------- A1
def valid(c, nb):
    c = [int(x) for x in c]
    return all(0 <= x <= nb - 1 for x in c) and all(y >= x for x, y in zip(c, c[1:]))


def band_rows(c, nb, band):
    """(p, q) of every row, lists of Python integers"""
    return [max(0, int(x) - band) for x in c], [min(nb - 1, int(x) + band) for x in c]


def connected_plain(c, nb, band):
    p, q = band_rows(c, nb, band)
    return p[0] == 0 and q[-1] == nb - 1 and all(p[i + 1] <= q[i] + 1 for i in range(len(c) - 1))


def band_min_plain(c, nb):
    """the closed form of A1"""
    c = [int(x) for x in c]
    return max([c[0], nb - 1 - c[-1]] + [(y - x) // 2 for x, y in zip(c, c[1:])])


def _join(pieces):
    """from the least lower end to the largest upper end of the non-empty pieces"""
    pieces = [(a, b) for a, b in pieces if a <= b]
    return (min(a for a, _ in pieces), max(b for _, b in pieces)) if pieces else EMPTY


def sweeps(c, nb, band):
    """(F, G): the forward and backward intervals of every row, lists of (lower, upper); EMPTY where there is none"""
    na = len(c)
    assert admissible(na, nb) and band >= 0, (na, nb, band)
    p, q = band_rows(c, nb, band)
    F = [(0, 0) if p[0] <= 0 else EMPTY]
    for i in range(1, na):
        a, b = F[i - 1]
        pieces = []
        if a <= b:
            pieces += [(max(a + 1, p[i]), min(b + 1, q[i])), (max(a + 2, p[i] + 1), min(b + 2, q[i]))]
        if i >= 2 and F[i - 2][0] <= F[i - 2][1]:
            e, f = F[i - 2]
            pieces.append((max(e + 1, p[i], p[i - 1]), min(f + 1, q[i], q[i - 1])))
        F.append(_join(pieces))
    G = [EMPTY] * na
    G[na - 1] = (nb - 1, nb - 1) if q[na - 1] >= nb - 1 else EMPTY
    for i in range(na - 2, -1, -1):
        a, b = G[i + 1]
        pieces = []
        if a <= b:
            pieces += [(max(a - 1, p[i]), min(b - 1, q[i])), (max(a - 2, p[i], p[i + 1] - 1), min(b - 2, q[i]))]
        if i + 2 < na and G[i + 2][0] <= G[i + 2][1]:
            e, f = G[i + 2]
            pieces.append((max(e - 1, p[i], p[i + 1] - 1), min(f - 1, q[i], q[i + 1] - 1)))
        G[i] = _join(pieces)
    return F, G


def region_rows(c, nb, band):
    """(lo, hi) of every row of the region as lists, an empty row as (1, 0); the band need not be connected"""
    F, G = sweeps(c, nb, band)
    lo, hi = [], []
    for (a, b), (e, f) in zip(F, G):
        l, h = max(a, e), min(b, f)
        if a > b or e > f or l > h:
            l, h = EMPTY
        lo.append(l); hi.append(h)
    return lo, hi


def connected_slope(c, nb, band):
    lo, hi = region_rows(c, nb, band)
    return lo[-1] <= hi[-1]


def connected(c, nb, band, slope):
    return connected_slope(c, nb, band) if slope else connected_plain(c, nb, band)


def band_min(c, nb, slope):
    """the least connected band, by trying them in turn"""
    band = 0
    while not connected(c, nb, band, slope):
        band += 1
    return band


def rows(c, nb, band, slope):
    """what llsm_gpu_align_around_rows fills: (lo, hi) int64 arrays of a connected band"""
    assert connected(c, nb, band, slope), (list(c), nb, band, slope)
    lo, hi = region_rows(c, nb, band) if slope else band_rows(c, nb, band)
    return np.array(lo, np.int64), np.array(hi, np.int64)


def center_line(pos_c, nb_c, na, nb):
    """llsm_gpu_align_center_line: float64, one operation at a time"""
    pos_c = np.asarray(pos_c, np.float64)
    na_c = len(pos_c)
    i = np.arange(na, dtype=np.float64)
    if na_c == 1 or na == 1:
        y = np.full(na, pos_c[0])
    else:
        x = (i * np.float64(na_c - 1)) / np.float64(na - 1)
        k = np.minimum(np.floor(x), na_c - 2).astype(np.int64)
        y = pos_c[k] + (pos_c[k + 1] - pos_c[k]) * (x - k)
    s = np.float64(nb - 1) / np.float64(nb_c - 1) if nb_c > 1 else np.float64(0)
    c = np.clip(np.floor(y * s + 0.5), 0, nb - 1).astype(np.int64)
    return np.maximum.accumulate(c)


# ---------------------------------------------------------------- A2
def to_band(D, c, band):
    """the plane [na][nb] in the band layout around c: +infinity where the column lies outside [p_i, q_i]"""
    na, nb = D.shape
    out = np.full((na, 2 * band + 1), np.inf, D.dtype)
    p, q = band_rows(c, nb, band)
    for i in range(na):
        off = int(c[i]) - band
        out[i, p[i] - off:q[i] - off + 1] = D[i, p[i]:q[i] + 1]
    return out


def dist_band(fa, fb, c, band, first, count, voicing_cost, dtype=np.float32):
    """rule D1 for the cells of the band, as a band plane [na][2 band + 1]; +infinity outside the rows of the band"""
    a = np.asarray(fa, dtype); b = np.asarray(fb, dtype)
    nb = len(b)
    width = 2 * band + 1
    col = np.asarray(c, np.int64)[:, None] - band + np.arange(width)[None, :]
    ok = (col >= 0) & (col < nb)
    col = np.clip(col, 0, nb - 1)
    d = np.zeros((len(a), width), dtype)
    with np.errstate(all="ignore"):
        for k in range(first, first + count):
            t = a[:, k, None] - b[col, k]
            d = d + t * t
        differ = (np.asarray(fa)[:, 0, None] > np.float32(0.5)) != (np.asarray(fb)[col, 0] > np.float32(0.5))
        d = np.where(differ, d + dtype(voicing_cost), d).astype(dtype)
    d[~ok] = np.inf
    return d


# ---------------------------------------------------------------- A3
def _take_first(cands, n, dtype):
    """m and move of B3 / K3: the first candidate that exists, a later one only if strictly smaller"""
    m = np.zeros(n, dtype); move = np.zeros(n, np.int8); have = np.zeros(n, bool)
    for number, (exists, value) in enumerate(cands):
        take = exists & (~have | (value < m))
        m[take] = value[take]; move[take] = number
        have |= exists
    return m, move, have


def accumulate_plain(P, c, nb, step_cost):
    """B3 over the rows of the band: (acc, moves) in the band layout, NaN / -1 outside the band.  The left candidate lies in
    the row itself, so a row is walked cell by cell; the two candidates of the row above are vectors"""
    P = np.asarray(P)
    dtype = P.dtype.type
    na, width = P.shape
    band = (width - 1) // 2
    assert connected_plain(c, nb, band), (list(c), nb, band)
    p, q = band_rows(c, nb, band)
    off = [int(x) - band for x in c]
    step = dtype(step_cost)
    acc = np.full((na, width), np.nan, dtype); mv = np.full((na, width), -1, np.int8)
    with np.errstate(all="ignore"):
        for i in range(na):
            j = np.arange(p[i], q[i] + 1)
            n = len(j)
            if i > 0:
                prev = acc[i - 1]
                has_dg = (j - 1 >= p[i - 1]) & (j - 1 <= q[i - 1]); has_up = (j >= p[i - 1]) & (j <= q[i - 1])
                dg = prev[np.clip(j - 1 - off[i - 1], 0, width - 1)]
                up = prev[np.clip(j - off[i - 1], 0, width - 1)] + step
            else:
                has_dg = has_up = np.zeros(n, bool); dg = up = np.zeros(n, dtype)
            d = P[i, j - off[i]]
            row = np.zeros(n, dtype); moves = np.zeros(n, np.int8)
            for x in range(n):
                if i == 0 and j[x] == 0:
                    row[x] = d[x]; moves[x] = 0
                    continue
                m, move, have = None, 0, False
                for number, (exists, value) in enumerate(((has_dg[x], dg[x]), (has_up[x], up[x]),
                                                           (x > 0, row[x - 1] + step if x > 0 else step))):
                    if exists and (not have or value < m):
                        m, move = value, number
                    have = have or bool(exists)
                assert have, (i, int(j[x]))                              # a connected band: every cell has a predecessor inside
                row[x] = m + d[x]; moves[x] = move
            acc[i, j - off[i]] = row; mv[i, j - off[i]] = moves
    return acc, mv


def path_plain(mv, c, nb):
    """B4: the cells from (na - 1, nb - 1) back to (0, 0) along the moves of a band plane"""
    na, width = mv.shape
    band = (width - 1) // 2
    i, j = na - 1, nb - 1
    cells = [(i, j)]
    while (i, j) != (0, 0):
        m = int(mv[i, j - (int(c[i]) - band)])
        assert m in (0, 1, 2) and len(cells) <= na + nb - 2, (i, j, m)
        i -= PLAIN[m][0]; j -= PLAIN[m][1]
        assert i >= 0 and j >= 0 and 0 <= j - (int(c[i]) - band) < width
        cells.append((i, j))
    return cells


def accumulate_slope(P, c, nb, step_cost):
    """K3 over the region inside the band around c: (acc, moves, lo, hi), band layout, NaN / -1 outside the region.  Every
    predecessor of a cell lies in an earlier row, so a row is one vector operation"""
    P = np.asarray(P)
    dtype = P.dtype.type
    na, width = P.shape
    band = (width - 1) // 2
    lo, hi = region_rows(c, nb, band)
    assert lo[-1] <= hi[-1], (list(c), nb, band)
    p, q = band_rows(c, nb, band)
    off = [int(x) - band for x in c]
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
            cands = [((j - 1 >= lo[i - 1]) & (j - 1 <= hi[i - 1]), at(acc, i - 1, j - 1))]
            if i >= 2:
                cands.append(((j - 1 >= lo[i - 2]) & (j - 1 <= hi[i - 2]) & (j >= p[i - 1]) & (j <= q[i - 1]),
                              (at(acc, i - 2, j - 1) + at(P, i - 1, j)) + step))
            else:
                cands.append((np.zeros(len(j), bool), np.zeros(len(j), dtype)))
            cands.append(((j - 2 >= lo[i - 1]) & (j - 2 <= hi[i - 1]) & (j - 1 >= p[i]),
                          (at(acc, i - 1, j - 2) + at(P, i, j - 1)) + step))
            m, move, have = _take_first(cands, len(j), dtype)
            assert have.all(), (i, lo[i], hi[i])                     # every cell of the region has a candidate
            acc[i, j - off[i]] = m + at(P, i, j); mv[i, j - off[i]] = move
    return acc, mv, np.array(lo, np.int64), np.array(hi, np.int64)


def path_slope(mv, c, nb):
    """K4: the cells from (na - 1, nb - 1) back to (0, 0), the cells passed between the ends of a move included"""
    na, width = mv.shape
    band = (width - 1) // 2
    off = [int(x) - band for x in c]
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
    return cells


def dtw(P, c, nb, slope, step_cost):
    """A3: (pos float32 [na], cost in P's dtype) of the band plane P around c"""
    P = np.asarray(P)
    na, width = P.shape
    band = (width - 1) // 2
    if slope:
        acc, mv, _, _ = accumulate_slope(P, c, nb, step_cost)
        cells = path_slope(mv, c, nb)
    else:
        acc, mv = accumulate_plain(P, c, nb, step_cost)
        cells = path_plain(mv, c, nb)
    return positions(cells, na), acc[-1, nb - 1 - (int(c[-1]) - band)]


def align(fa, fb, c, band, slope, first, count, step_cost=0.0, voicing_cost=0.0, dtype=np.float32):
    """the whole chain: (pos, cost, the band plane: plane 14)"""
    P = dist_band(fa, fb, c, band, first, count, voicing_cost, dtype)
    return dtw(P, c, len(fb), slope, step_cost) + (P,)


# ---------------------------------------------------------------- every cell and every path, for small planes
def reachable(na, nb, p, q):
    """(forward, backward): bool planes [na][nb] of the cells reached from (0, 0) and reaching (na - 1, nb - 1) by the moves
    of the slope pattern inside the rows p ... q, cell by cell (a row at a time: every move changes the row).  Nothing of the
    sweeps is used: a cell is reached if it lies in the band and one of the three moves into it starts from a reached cell
    and passes a cell of the band"""
    col = np.arange(nb)
    inb = np.zeros((na + 2, nb + 2), bool)                           # the band, with two rows and columns of padding
    for i in range(na):
        inb[i, :nb] = (col >= p[i]) & (col <= q[i])

    def back(x, k):                                                  # x[j - k], False before the first column
        return np.concatenate([np.zeros(k, bool), x[:len(x) - k]])

    def nxt(x, k):                                                   # x[j + k]
        return np.concatenate([x[k:], np.zeros(k, bool)])

    fwd = np.zeros((na + 2, nb + 2), bool); fwd[0, 0] = inb[0, 0]
    for i in range(1, na):
        fwd[i] = inb[i] & (back(fwd[i - 1], 1) |                                        # move 0
                           (back(fwd[i - 2], 1) & inb[i - 1] if i >= 2 else False) |    # move 1 passes (i - 1, j)
                           (back(fwd[i - 1], 2) & back(inb[i], 1)))                      # move 2 passes (i, j - 1)
    bwd = np.zeros((na + 2, nb + 2), bool); bwd[na - 1, nb - 1] = inb[na - 1, nb - 1]
    for i in range(na - 2, -1, -1):
        # moves 1 and 2 out of (i, j) both pass (i + 1, j + 1), on the way to (i + 2, j + 1) and to (i + 1, j + 2)
        bwd[i] = inb[i] & (nxt(bwd[i + 1], 1) | (nxt(inb[i + 1], 1) & (nxt(bwd[i + 2], 1) | nxt(bwd[i + 1], 2))))
    return fwd[:na, :nb], bwd[:na, :nb]


def brute_force(D, c, band, slope, step_cost):
    """the least cost over all paths of allowed moves from (0, 0) to (na - 1, nb - 1) of the full plane D [na][nb] inside
    the band around c, each summed in the order of B3 / K3, in D's dtype (exact on small integers), and the number of paths;
    (None, 0) if there is none"""
    D = np.asarray(D)
    dtype = D.dtype.type
    na, nb = D.shape
    p, q = band_rows(c, nb, band)
    step = dtype(step_cost)

    def inside(x, y):
        return 0 <= x < na and 0 <= y < nb and p[x] <= y <= q[x]

    best, count = None, 0
    stack = [(0, 0, D[0, 0])] if inside(0, 0) else []
    while stack:
        i, j, v = stack.pop()
        if (i, j) == (na - 1, nb - 1):
            count += 1
            best = v if best is None or v < best else best
            continue
        if slope:
            for (di, dj), mid in MOVES:
                ni, nj = i + di, j + dj
                if not inside(ni, nj) or (mid is not None and not inside(ni - mid[0], nj - mid[1])):
                    continue
                w = v if mid is None else (v + D[ni - mid[0], nj - mid[1]]) + step
                stack.append((ni, nj, w + D[ni, nj]))
        else:
            for number, (di, dj) in enumerate(PLAIN):
                ni, nj = i + di, j + dj
                if inside(ni, nj):
                    stack.append((ni, nj, (v if number == 0 else v + step) + D[ni, nj]))
    return best, count
