"""Host side of llsm_gpu_batch_align_band_slope (no GPU): llsm_gpu_align_band_slope_min / _rows against Python integers, and
the numpy restatement of rules K1 - K4 (tests/align_band_slope_reference.py) on its own: the sweeps of K1 against
reachability cell by cell -- rule K1 rests on that check, the interval property is measured and not proven --, every path of
small planes by enumeration, planes written by hand, NaN and infinite planes, the band that covers the matrix against rules
L1 - L4, the cost against the two rules it narrows, and float32 against the same code in float64.

Measured with align_reference.make(seed, na, nb, 24, 0.3), step_cost 1, seeds 0 ... 11, sizes (200, 170), (64, 65), (129, 90),
(300, 410) (printed by test_float32_against_float64): at band 8 the float32 chain differs from the float64 chain on 8 of
8 316 frames, cost within 5.3e-7 relative, and the cost is above that of the unbanded slope rule on 18 of the 48 pairs; at
band 25 no frame differs, cost within 5.6e-7."""
import numpy as np
import pytest

import libllsm2_amd as llsm
import align_reference as aref
import align_band_reference as bref
import align_slope_reference as sref
import align_band_slope_reference as kref
from align_common import COST_REL, DIFFER_CAP, band_slope_properties as check_properties

SIZES = [(200, 170), (64, 65), (129, 90), (300, 410)]
SEEDS = range(12)
BANDS = (8, 25)
LARGER = [(1000, 1999, 500), (5000, 4001, 500), (60000, 60000, 500)]


# ---------------------------------------------------------------- K1: the host calls
def raw_rows(na, nb, band, lo=True, hi=True):
    L = llsm.load()
    n = max(na, 1)
    a = np.full(n, -7, np.int32); b = np.full(n, -7, np.int32)
    rc = L.llsm_gpu_align_band_slope_rows(na, nb, band, a.ctypes.data_as(llsm.P_int) if lo else None,
                                          b.ctypes.data_as(llsm.P_int) if hi else None)
    return rc, L.llsm_gpu_last_error().decode(), a, b


def test_rows_and_min_against_python_integers():
    L = llsm.load()
    accepted = refused = not_admissible = 0
    for na in range(1, 71):
        for nb in range(1, 71):
            why = sref.bound(na, nb)
            if why is not None:
                name, value, limit = why
                needle = "%s = %d exceeds 2 (%s) = %d" % (name, value, "na - 1" if name == "nb - 1" else "nb - 1", limit)
                assert L.llsm_gpu_align_band_slope_min(na, nb) == -1
                msg = L.llsm_gpu_last_error().decode()
                assert msg.startswith("llsm_gpu_align_band_slope_min:") and needle in msg and ("%d x %d" % (na, nb)) in msg, msg
                rc, msg, lo, hi = raw_rows(na, nb, max(na, nb))
                assert rc == -1 and msg.startswith("llsm_gpu_align_band_slope_rows:") and needle in msg, msg
                assert np.all(lo == -7) and np.all(hi == -7)
                not_admissible += 1
                continue
            least = kref.band_min(na, nb)
            assert least in (0, 1) and L.llsm_gpu_align_band_slope_min(na, nb) == least == llsm.align_band_slope_min(na, nb), (na, nb)
            for band in range(0, max(na, nb) + 1):
                rc, msg, lo, hi = raw_rows(na, nb, band)
                if band < least:                                     # connectedness is monotone in the band
                    assert not kref.connected(na, nb, band)
                    assert rc == -1 and msg.startswith("llsm_gpu_align_band_slope_rows:") and np.all(lo == -7) and np.all(hi == -7)
                    assert ("a band of %d is not connected for the slope pattern on %d x %d frames" % (band, na, nb)) in msg, msg
                    assert ("llsm_gpu_align_band_slope_min is %d" % least) in msg, msg
                    assert L.llsm_gpu_align_band_slope_rows(na, nb, band, None, None) == -1
                    refused += 1
                    continue
                want_lo, want_hi = kref.rows(na, nb, band)
                assert rc == 0 and np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi), (na, nb, band)
                assert (lo[0], hi[0], lo[-1], hi[-1]) == (0, 0, nb - 1, nb - 1)
                accepted += 1
            band = max(na, nb) // 2
            if band >= least:
                want_lo, want_hi = kref.rows(na, nb, band)
                assert L.llsm_gpu_align_band_slope_rows(na, nb, band, None, None) == 0    # only asks whether it is connected
                for keep_lo in (True, False):                        # one of them alone
                    rc, _, l1, h1 = raw_rows(na, nb, band, lo=keep_lo, hi=not keep_lo)
                    assert rc == 0 and (np.array_equal(l1, want_lo) and np.all(h1 == -7) if keep_lo else
                                        np.array_equal(h1, want_hi) and np.all(l1 == -7)), (na, nb)
                lib_lo, lib_hi = llsm.align_band_slope_rows(na, nb, band)
                assert lib_lo.dtype == np.int32 and np.array_equal(lib_lo, want_lo) and np.array_equal(lib_hi, want_hi)
    assert accepted > 100000 and refused > 700 and not_admissible > 2400, (accepted, refused, not_admissible)
    lo, hi = llsm.align_band_slope_rows(3, 2, 0)
    assert list(lo) == [0, 1, 1] and list(hi) == [0, 0, 1]           # an empty row is (1, 0)
    with pytest.raises(llsm.LlsmError):
        llsm.align_band_slope_rows(63, 64, 0)
    with pytest.raises(llsm.LlsmError):
        llsm.align_band_slope_min(2, 4)


@pytest.mark.parametrize("na,nb,band", LARGER)
def test_rows_of_long_pairs(na, nb, band):
    lo, hi = llsm.align_band_slope_rows(na, nb, band)
    want_lo, want_hi = kref.rows(na, nb, band)
    assert np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi)
    assert llsm.align_band_slope_min(na, nb) == kref.band_min(na, nb)
    full = lo <= hi
    assert np.all(np.diff(lo[full]) >= 0) and np.all(np.diff(hi[full]) >= 0) and not np.any(~full[1:] & ~full[:-1])
    assert np.all(hi[full] - lo[full] <= 2 * band)


def test_rows_refuses_bad_sizes_and_bands():
    L = llsm.load()
    for na, nb in ((0, 1), (1, 0), (-3, 4), (4, -3), (0, 0)):
        rc, msg, lo, hi = raw_rows(na, nb, 3)
        assert rc == -1 and msg.startswith("llsm_gpu_align_band_slope_rows:") and "na < 1 or nb < 1" in msg, msg
        assert ("na = %d" % na) in msg and ("nb = %d" % nb) in msg and np.all(lo == -7)
        assert L.llsm_gpu_align_band_slope_min(na, nb) == -1
        assert L.llsm_gpu_last_error().decode().startswith("llsm_gpu_align_band_slope_min:")
    rc, msg, lo, hi = raw_rows(5, 5, -1)
    assert rc == -1 and "band < 0" in msg and "na = 5" in msg and "nb = 5" in msg and "band = -1" in msg and np.all(lo == -7)
    # more rows than a call has cells: refused before the sweeps ask for memory
    assert L.llsm_gpu_align_band_slope_rows(2 ** 31 - 1, 2 ** 31 - 1, 5, None, None) == -1
    assert "exceeds 2^28" in L.llsm_gpu_last_error().decode()
    assert L.llsm_gpu_align_band_slope_min(2 ** 28 + 1, 2 ** 28) == -1 and "exceeds 2^28" in L.llsm_gpu_last_error().decode()
    # a band far wider than the matrix: the integers are taken in 64 bits
    lo, hi = llsm.align_band_slope_rows(9, 7, 2 ** 31 - 1)
    want_lo, want_hi = sref.rows(9, 7)
    assert np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi)


# ---------------------------------------------------------------- K1: the sweeps against reachability cell by cell
def test_sweeps_against_reachability():
    """all admissible na, nb <= 40 at every band: the cells on some path of allowed moves are exactly the rows of the
    sweeps, so every row is an interval; the rows are monotone over the non-empty ones; no two consecutive rows are empty;
    every cell of the region but (0, 0) has a candidate of K3; the band that covers the matrix gives the rows of L1"""
    pairs = planes = 0
    for na in range(1, 41):
        for nb in range(1, 41):
            if not sref.admissible(na, nb):
                continue
            pairs += 1
            was_connected = False
            for band in range(0, max(na, nb) + 1):
                fwd, bwd = kref.reachable(na, nb, band)
                lo, hi = kref.region_rows(na, nb, band)
                lo = np.array(lo); hi = np.array(hi)
                col = np.arange(nb)[None, :]
                inside = (col >= lo[:, None]) & (col <= hi[:, None])
                assert np.array_equal(fwd & bwd, inside), (na, nb, band)
                F, G = kref.sweeps(na, nb, band)
                for i in range(na):                                  # each sweep alone gives the reachable set of its direction
                    assert np.array_equal(np.nonzero(fwd[i])[0], np.arange(F[i][0], F[i][1] + 1)), (na, nb, band, i)
                    assert np.array_equal(np.nonzero(bwd[i])[0], np.arange(G[i][0], G[i][1] + 1)), (na, nb, band, i)
                connected = bool(inside[-1].any())
                assert connected or not was_connected                # monotone in the band
                was_connected = connected
                if not connected:
                    assert not inside.any()
                    continue
                planes += 1
                full = lo <= hi
                assert (lo[0], hi[0], lo[-1], hi[-1]) == (0, 0, nb - 1, nb - 1)
                assert np.all(np.diff(lo[full]) >= 0) and np.all(np.diff(hi[full]) >= 0), (na, nb, band)
                assert not np.any(~full[1:] & ~full[:-1]), (na, nb, band)
                assert np.all(lo[~full] == 1) and np.all(hi[~full] == 0)
                p, q = kref.band_rows(na, nb, band)
                for i, j in zip(*np.nonzero(inside)):
                    if (i, j) != (0, 0):
                        assert any(kref.allowed(i, j, m, na, nb, p, q) and inside[i - di, j - dj]
                                   for m, ((di, dj), _) in enumerate(kref.MOVES)), (na, nb, band, i, j)
                if band >= nb - 1:
                    want_lo, want_hi = sref.rows(na, nb)
                    keep = want_lo <= want_hi
                    assert np.array_equal(full, keep) and np.array_equal(lo[keep], want_lo[keep]) and np.array_equal(hi[keep], want_hi[keep])
            assert was_connected
    assert pairs == 800 and planes > 20000, (pairs, planes)


# ---------------------------------------------------------------- K3 - K4 against every path
def test_reference_against_enumeration():
    cases = binding = 0
    for na in range(1, 9):
        for nb in range(1, 9):
            if not sref.admissible(na, nb):
                continue
            for band in range(kref.band_min(na, nb), max(nb - 1, 0) + 1):
                for seed in range(3):
                    D = np.random.default_rng(1000 * na + 100 * nb + 10 * band + seed).integers(0, 6, (na, nb)).astype(np.float32)
                    best, n = kref.brute_force(D, band, 2.0)
                    P = bref.to_band(D, band)
                    pos, cost = kref.dtw(P, nb, 2.0)
                    assert n >= 1 and cost == best, (na, nb, band, seed, cost, best)
                    acc, mv, lo, hi = kref.accumulate(P, nb, 2.0)
                    cells, moves = kref.path(mv, nb)
                    assert moves <= min(na, nb) - 1 and cells[0] == (na - 1, nb - 1) and cells[-1] == (0, 0)
                    p, q = kref.band_rows(na, nb, band)
                    assert all(p[i] <= j <= q[i] for i, j in cells)  # the passed cells too lie in the band
                    steps = len(cells) - 1 - moves
                    assert sum(D[c] for c in cells) + 2.0 * steps == cost
                    binding += cost > sref.brute_force(D, 2.0)[0]
                    cases += 1
    assert cases > 400 and binding > 20, (cases, binding)


# ---------------------------------------------------------------- planes written by hand
def test_ties_take_move_0_then_1_then_2():
    # 5 x 5 under band 2: cell (3, 3) has all three candidates: (2, 2), (1, 2) through (2, 3), (2, 1) through (3, 2)
    lo, hi = kref.rows(5, 5, 2)
    assert lo[2] <= 1 and hi[2] >= 2 and lo[1] <= 2 <= hi[1] and lo[3] <= 3 <= hi[3]
    for bump, move in (((), 0), (((2, 2), 1), 1), (((2, 2), 1, (2, 3), 1), 2), (((2, 2), 1, (3, 2), 1), 1)):
        D = np.zeros((5, 5), np.float32)
        for k in range(0, len(bump), 2):
            D[bump[k]] = bump[k + 1]
        acc, mv, _, _ = kref.accumulate(bref.to_band(D, 2), 5, 0.0)
        assert mv[3, 3 - (bref.centers(5, 5)[3] - 2)] == move, (bump, mv)
    # a constant plane, step_cost 0: every comparison ties; move 0 where it exists, then move 1, then move 2
    seen = set()
    for na, nb, band in ((5, 5, 1), (4, 6, 2), (6, 4, 1), (64, 65, 3), (40, 31, 0)):
        acc, mv, lo, hi = kref.accumulate(np.ones((na, 2 * band + 1), np.float32), nb, 0.0)
        p, q = kref.band_rows(na, nb, band)
        off = [c - band for c in bref.centers(na, nb)]
        for i in range(1, na):
            for j in range(lo[i], hi[i] + 1):
                has = [kref.allowed(i, j, m, na, nb, p, q) and lo[i - di] <= j - dj <= hi[i - di]
                       for m, ((di, dj), _) in enumerate(kref.MOVES)]
                assert mv[i, j - off[i]] == has.index(True), (na, nb, band, i, j)
                seen.add(has.index(True))
    assert seen == {0, 1, 2}


def test_a_move_is_refused_where_only_the_passed_cell_is_outside_the_band():
    # 4 x 3 under band 0: the band is (0, 0), (1, 1), (2, 1), (3, 2).  Move 1 from (1, 1) to (3, 2) has both ends in the band
    # and passes (2, 2), which is outside: it is refused, (1, 1) is on no path and row 1 is empty.  What is left is move 1
    # from (0, 0) through (1, 1) to (2, 1), then move 0
    assert kref.band_rows(4, 3, 0) == ([0, 1, 1, 2], [0, 1, 1, 2])
    lo, hi = kref.rows(4, 3, 0)
    assert list(zip(lo, hi)) == [(0, 0), (1, 0), (1, 1), (2, 2)]
    z = np.float32
    D = (np.array([[1, 90, 90], [90, 2, 90], [90, 50, 3], [90, 90, 4]], np.float32) * z(0.1)).astype(np.float32)
    # rule L3 on the whole matrix takes the cheap cell (2, 2) ...
    acc, mv, _ = sref.accumulate(D, 0.3)
    assert mv[3, 2] == 1 and acc[3, 2] == (((D[0, 0] + D[1, 1]) + D[2, 2]) + z(0.3)) + D[3, 2]
    # ... and K3 cannot, although the band plane does not even hold D[2][2]
    P = bref.to_band(D, 0)
    assert P.shape == (4, 1)
    pos, cost = kref.dtw(P, 3, 0.3)
    acc, mv, _, _ = kref.accumulate(P, 3, 0.3)
    assert list(mv[:, 0]) == [0, -1, 1, 0]
    assert cost == (((D[0, 0] + D[1, 1]) + z(0.3)) + D[2, 1]) + D[3, 2] and cost.dtype == np.float32
    assert list(pos) == [0.0, 1.0, 1.0, 2.0]
    assert cost == kref.brute_force(D, 0, 0.3)[0] and kref.brute_force(D, 0, 0.3)[1] == 1
    # one column more of band and the cell is back
    pos, cost = kref.dtw(bref.to_band(D, 1), 3, 0.3)
    assert cost == sref.dtw(D, 0.3)[1] and list(pos) == [0.0, 1.0, 2.0, 2.0]


def test_nan_and_infinite_planes_keep_the_walk_inside():
    rng = np.random.default_rng(5)
    for na, nb, band, bad_rows, value in ((9, 7, 1, [4], np.nan), (7, 9, 2, [0], np.nan), (6, 6, 0, [5], np.nan), (5, 8, 7, [0, 1, 2, 3, 4], np.nan),
                                          (64, 127, 1, [10, 11], np.nan), (9, 5, 1, [3, 4], np.inf), (40, 50, 3, [7, 20], -np.inf),
                                          (130, 200, 3, [64, 65, 128], np.nan)):
        P = bref.to_band(rng.random((na, nb)).astype(np.float32), band)
        P[bad_rows] = value
        acc, mv, lo, hi = kref.accumulate(P, nb, 1.0)
        cells, n = kref.path(mv, nb)                                 # (asserts the bound on the number of moves itself)
        assert n <= min(na, nb) - 1
        p, q = kref.band_rows(na, nb, band)
        assert all(p[i] <= j <= q[i] for i, j in cells)
        check_properties(kref.positions(cells, na), na, nb, band)
        cost = kref.dtw(P, nb, 1.0)[1]
        assert np.isnan(cost) if np.isnan(value) else np.isinf(cost)
    # scattered NaN and infinite cells
    for seed in range(40):
        rng = np.random.default_rng(seed)
        na = int(rng.integers(2, 60)); nb = int(rng.integers(max(2, (na + 2) // 2), 2 * na))
        assert sref.admissible(na, nb)
        band = int(rng.integers(kref.band_min(na, nb), 8))
        P = bref.to_band(rng.integers(0, 4, (na, nb)).astype(np.float32), band)
        P[rng.random(P.shape) < 0.2] = np.nan; P[rng.random(P.shape) < 0.1] = np.inf
        acc, mv, lo, hi = kref.accumulate(P, nb, float(rng.integers(0, 3)))
        cells, n = kref.path(mv, nb)
        check_properties(kref.positions(cells, na), na, nb, band)


# ---------------------------------------------------------------- against the rules it narrows
def test_a_band_that_covers_the_matrix_gives_the_bits_of_the_slope_rule():
    rng = np.random.default_rng(11)
    done = 0
    for na, nb in ((1, 1), (2, 2), (3, 2), (2, 3), (9, 7), (7, 9), (64, 65), (65, 129), (129, 65), (130, 200), (257, 300)):
        for kind in ("random", "integer", "nan"):
            D = rng.integers(0, 4, (na, nb)).astype(np.float32) if kind == "integer" else rng.random((na, nb)).astype(np.float32)
            if kind == "nan":
                D[rng.random((na, nb)) < 0.05] = np.nan
            for band in (max(nb - 1, 0), nb + 3):
                pos, cost = kref.dtw(bref.to_band(D, band), nb, 1.0)
                want_pos, want_cost = sref.dtw(D, 1.0)
                assert np.array_equal(pos.view(np.uint32), want_pos.view(np.uint32)), (na, nb, kind, band)
                assert np.array_equal(np.float32(cost).view(np.uint32), np.float32(want_cost).view(np.uint32)) or \
                    (np.isnan(cost) and np.isnan(want_cost)), (na, nb, kind, band)
                done += 1
    assert done == 66


_cases = {}


def case(size, seed, band):
    """(float32 chain, float64 chain, cost of rules L1 - L4 in float32, cost of rules B1 - B4 under the same band in
    float32) of one generated pair; the first two (pos, cost)"""
    key = (size, seed, band)
    if key not in _cases:
        A, B, _ = aref.make(seed, size[0], size[1], 24, 0.3)
        A = A.astype(np.float32); B = B.astype(np.float32)
        _cases[key] = (kref.align(A, B, band, 0, 24, step_cost=1.0), kref.align(A, B, band, 0, 24, step_cost=1.0, dtype=np.float64),
                       sref.align(A, B, 0, 24, step_cost=1.0)[1], bref.align(A, B, band, 0, 24, step_cost=1.0)[1])
    return _cases[key]


@pytest.mark.parametrize("band", BANDS)
def test_float32_against_float64(band):
    differ = total = dearer = 0
    worst = 0.0
    for size in SIZES:
        for seed in SEEDS:
            (p32, c32), (p64, c64), slope, _ = case(size, seed, band)
            assert p32.dtype == np.float32 and c32.dtype == np.float32 and c64.dtype == np.float64
            differ += int(np.count_nonzero(p32 != p64)); total += len(p32)
            worst = max(worst, abs(float(c32) - float(c64)) / float(c64))
            dearer += bool(c32 > slope)
            check_properties(p32, size[0], size[1], band)
    print("band %d, float32 against float64: %d of %d frames differ, cost within %.2g relative; dearer than the unbanded slope "
          "rule on %d of 48 pairs" % (band, differ, total, worst, dearer))
    assert total == 12 * (200 + 64 + 129 + 300)
    assert differ <= DIFFER_CAP * total
    assert worst <= COST_REL
    if band == 8:
        assert dearer >= 1                                          # the band really binds


@pytest.mark.parametrize("band", BANDS)
def test_cost_is_never_below_the_slope_rule_nor_the_band_rule(band):
    for size in SIZES:
        for seed in SEEDS:
            (_, c32), _, slope, banded = case(size, seed, band)
            assert c32.dtype == np.float32 and slope.dtype == np.float32 and banded.dtype == np.float32
            assert c32 >= slope and c32 >= banded, (size, seed, band, c32, slope, banded)
