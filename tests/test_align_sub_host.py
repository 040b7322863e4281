"""Host side of llsm_gpu_batch_align_sub (no GPU): llsm_gpu_align_sub_rows against Python integers, and the numpy
restatement of rules Q1 - Q5 (tests/align_sub_reference.py) on its own: the region, every path of small planes by
enumeration, planes written by hand, the consequences llsm_gpu.h states, float32 against the same code in float64, and
queries planted in longer takes, which the open-ended rule finds and rules D1 - D3 miss.

The bounds of the planted cases are the issue's: float32 leaves the float64 chain on at most DIFFER_CAP of the frames, costs
agree within COST_REL, begin and end lie within 2 frames of where the rendition was planted, the RMS distance to the truth is
at most 1.5 frames, and rules D1 - D3 on the same pair miss by more than ten times the open-ended RMS.  The figures are
printed by the tests."""
import numpy as np
import pytest

import libllsm2_amd as llsm
import align_reference as aref
import align_slope_reference as sref
import align_sub_reference as qref
from align_common import COST_REL, DIFFER_CAP, SEEDS

PLAIN_PLANTS = [(64, 65, 40, 70), (129, 100, 64, 1), (200, 170, 0, 90), (65, 128, 130, 0), (150, 200, 300, 250)]
SLOPE_PLANTS = [(64, 65, 40, 70), (129, 100, 64, 1), (200, 170, 0, 90), (65, 100, 130, 0), (150, 200, 300, 250)]
LARGER = [(64, 127), (129, 65), (127, 64), (65, 129), (1000, 1999), (1999, 1000), (2001, 1000), (2001, 1001), (2002, 1001)]


def shapes():
    return [(na, nb) for na in range(1, 41) for nb in range(1, 41)] + LARGER


# ---------------------------------------------------------------- Q1: the host call
def raw_rows(na, nb, slope, lo=True, hi=True):
    L = llsm.load()
    n = max(na, 1) if na <= 20000 else 1
    a = np.full(n, -7, np.int32); b = np.full(n, -7, np.int32)
    rc = L.llsm_gpu_align_sub_rows(na, nb, slope, a.ctypes.data_as(llsm.P_int) if lo else None, b.ctypes.data_as(llsm.P_int) if hi else None)
    return rc, L.llsm_gpu_last_error().decode(), a, b


def test_rows_against_python_integers():
    L = llsm.load()
    accepted = refused = 0
    for na, nb in shapes():
        for slope in (0, 1):
            rc, msg, lo, hi = raw_rows(na, nb, slope)
            if qref.admissible(na, nb, slope):
                want_lo, want_hi = qref.rows(na, nb, slope)
                assert rc == 0 and np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi), (na, nb, slope)
                assert lo[0] == 0 and np.all(hi == nb - 1) and np.all(np.diff(lo) >= 0) and lo[-1] <= nb - 1
                assert np.all(lo == 0) if not slope else np.array_equal(lo, (np.arange(na) + 1) // 2)
                assert L.llsm_gpu_align_sub_rows(na, nb, slope, None, None) == 0      # only asks whether it is admissible
                for keep_lo in (True, False):                                         # one of them alone
                    rc, _, l1, h1 = raw_rows(na, nb, slope, lo=keep_lo, hi=not keep_lo)
                    assert rc == 0 and (np.array_equal(l1, want_lo) and np.all(h1 == -7) if keep_lo else
                                        np.array_equal(h1, want_hi) and np.all(l1 == -7)), (na, nb)
                lib_lo, lib_hi = llsm.align_sub_rows(na, nb, bool(slope))
                assert np.array_equal(lib_lo, want_lo) and np.array_equal(lib_hi, want_hi)
                accepted += 1
            else:
                assert slope == 1
                needle = "ceil((na - 1) / 2) = %d exceeds nb - 1 = %d" % (-(-(na - 1) // 2), nb - 1)
                assert rc == -1 and msg.startswith("llsm_gpu_align_sub_rows:") and needle in msg, (na, nb, msg)
                assert ("%d x %d" % (na, nb)) in msg and np.all(lo == -7) and np.all(hi == -7)
                assert L.llsm_gpu_align_sub_rows(na, nb, 1, None, None) == -1
                with pytest.raises(llsm.LlsmError):
                    llsm.align_sub_rows(na, nb, True)
                refused += 1
    assert accepted > 2800 and refused > 350
    # a query is admissible in any take that is long enough, however long: L1 refuses 64 x 200, Q1 does not
    assert L.llsm_gpu_align_slope_rows(64, 200, None, None) == -1 and L.llsm_gpu_align_sub_rows(64, 200, 1, None, None) == 0
    lo, hi = llsm.align_sub_rows(5, 3, True)
    assert list(lo) == [0, 1, 1, 2, 2] and list(hi) == [2] * 5


def test_rows_refusals_and_64_bit_sizes():
    L = llsm.load()
    for na, nb in ((0, 1), (1, 0), (-3, 4), (4, -3), (0, 0)):
        for slope in (0, 1):
            rc, msg, lo, hi = raw_rows(na, nb, slope)
            assert rc == -1 and msg.startswith("llsm_gpu_align_sub_rows:") and "na < 1 or nb < 1" in msg, msg
            assert ("na = %d" % na) in msg and ("nb = %d" % nb) in msg and np.all(lo == -7) and np.all(hi == -7)
    for slope in (-1, 2, 7):
        rc, msg, lo, hi = raw_rows(5, 9, slope)
        assert rc == -1 and msg.startswith("llsm_gpu_align_sub_rows:") and ("slope = %d is neither 0 nor 1" % slope) in msg, msg
        assert "na = 5" in msg and "nb = 9" in msg and np.all(lo == -7) and np.all(hi == -7)
        assert L.llsm_gpu_align_sub_rows(5, 9, slope, None, None) == -1
    # sizes near 2^31: the bound is taken in 64-bit
    top = 2 ** 31 - 1
    assert L.llsm_gpu_align_sub_rows(top, top, 1, None, None) == 0
    assert L.llsm_gpu_align_sub_rows(top, 2 ** 30, 1, None, None) == 0              # ceil((2^31 - 2) / 2) = 2^30 - 1
    assert L.llsm_gpu_align_sub_rows(top, 2 ** 30 - 1, 1, None, None) == -1
    assert "ceil((na - 1) / 2) = %d exceeds nb - 1 = %d" % (2 ** 30 - 1, 2 ** 30 - 2) in L.llsm_gpu_last_error().decode()
    assert L.llsm_gpu_align_sub_rows(top, 1, 0, None, None) == 0 and L.llsm_gpu_align_sub_rows(1, top, 1, None, None) == 0
    # the last rows of a long query, through the arrays
    n = 20001
    lo = np.zeros(n, np.int32); hi = np.zeros(n, np.int32)
    assert L.llsm_gpu_align_sub_rows(n, 2 ** 31 - 1, 1, lo.ctypes.data_as(llsm.P_int), hi.ctypes.data_as(llsm.P_int)) == 0
    assert lo[-1] == 10000 and lo[-2] == 10000 and lo[-3] == 9999 and np.all(hi == 2 ** 31 - 2)


def test_every_region_cell_below_row_0_has_a_predecessor():
    for na, nb in shapes():
        if not qref.admissible(na, nb, True) or na > 300:
            continue
        inside = qref.region(na, nb, True)
        ii, jj = np.nonzero(inside)
        have = np.zeros(len(ii), bool)
        for (di, dj), _ in sref.MOVES:
            ok = (ii >= di) & (jj >= dj)
            have |= ok & inside[np.maximum(ii - di, 0), np.maximum(jj - dj, 0)]
        assert np.all(have[ii >= 1]) and not np.any(have[ii == 0]), (na, nb)
    # the region is the cells reached from some cell of row 0 under the moves, up to 30 x 30
    for na in range(1, 31):
        for nb in range(1, 31):
            fwd = np.zeros((na, nb), bool); fwd[0, :] = True
            for i in range(1, na):
                for j in range(nb):
                    fwd[i, j] = any(i >= di and j >= dj and fwd[i - di, j - dj] for (di, dj), _ in sref.MOVES)
            if not qref.admissible(na, nb, True):
                assert not fwd[-1].any(), (na, nb)                   # and no path at all where the pair is refused
            else:
                assert np.array_equal(fwd, qref.region(na, nb, True)), (na, nb)


# ---------------------------------------------------------------- Q3 - Q5 against every path
@pytest.mark.parametrize("slope", [False, True], ids=["plain", "slope"])
def test_reference_against_enumeration(slope):
    cases = 0
    for na in range(1, 7):
        for nb in range(1, 7):
            for seed in range(4):
                D = np.random.default_rng(100 * na + 10 * nb + seed).integers(0, 6, (na, nb)).astype(np.float32)
                best = qref.brute_force(D, 2.0, slope)
                if not qref.admissible(na, nb, slope):
                    assert all(b is None for b in best)
                    continue
                pos, (begin, end), cost, last = qref.dtw(D, 2.0, slope)
                least = min(b for b in best if b is not None)
                ends = {j for j, b in enumerate(best) if b is not None and b == least}
                assert cost == least and end == min(ends), (na, nb, seed, cost, least)
                assert {j for j in range(nb) if last[j] == cost} == ends
                for j in range(nb):                                  # the whole matching function, and +infinity where no path ends
                    assert (best[j] is None and last[j] == np.inf) or best[j] == last[j], (na, nb, seed, j)
                # the path of the reference costs what acc says, summed along its cells
                acc, mv, _ = qref.accumulate(D, 2.0, slope)
                cells, moves = qref.path(mv, end, slope)
                assert moves <= na - 1 + end and cells[0] == (na - 1, end) and cells[-1] == (0, begin)
                steps = len(cells) - 1 - moves if slope else sum(1 for c in cells[:-1] if mv[c] != 0)
                assert sum(D[c] for c in cells) + 2.0 * steps == cost
                cases += 1
    assert cases == (144 if not slope else 4 * sum(qref.admissible(na, nb, True) for na in range(1, 7) for nb in range(1, 7)))


# ---------------------------------------------------------------- planes written by hand
def test_ties_take_the_diagonal_then_up_then_left_and_the_smallest_end():
    # a constant plane, step_cost 0: every comparison ties
    for na, nb in ((5, 5), (4, 9), (6, 4), (64, 65)):
        acc, mv, _ = qref.accumulate(np.ones((na, nb), np.float32), 0.0, False)
        assert np.all(mv[0] == -1) and np.all(mv[1:, 0] == 1) and np.all(mv[1:, 1:] == 0)
        pos, (begin, end), cost, last = qref.dtw(np.ones((na, nb), np.float32), 0.0, False)
        assert (begin, end) == (0, 0) and cost == na and np.all(pos == 0) and np.all(last == na)   # straight up column 0
        acc, mv, inside = qref.accumulate(np.ones((na, nb), np.float32), 0.0, True)
        i, j = np.nonzero(inside)
        below = i >= 1
        dg = below & (j >= 1) & inside[i - 1, j - 1]
        assert np.all(mv[i[dg], j[dg]] == 0) and np.all(mv[~inside] == -1) and np.all(mv[0] == -1)
        up = below & ~dg                                             # lo of an even row: move 1 alone exists
        assert np.all(mv[i[up], j[up]] == 1) and np.all(i[up] % 2 == 0) and np.all(j[up] == i[up] // 2)
    # single cells: plain 3 x 3, the cell (2, 2) with the diagonal, then the upper, then the left predecessor the dearer
    for bump, move in (((), 0), (((1, 1), 1), 1), (((1, 1), 1, (1, 2), 1), 2), (((1, 1), 1, (2, 1), 1), 1)):
        D = np.zeros((3, 3), np.float32)
        for k in range(0, len(bump), 2):
            D[bump[k]] = bump[k + 1]
        assert qref.accumulate(D, 0.0, False)[1][2, 2] == move, bump
    # the pattern on 5 x 5: cell (3, 3) from (2, 2), from (1, 2) through (2, 3), from (2, 1) through (3, 2)
    for bump, move in (((), 0), (((2, 2), 1), 1), (((2, 2), 1, (2, 3), 1), 2), (((2, 2), 1, (3, 2), 1), 1)):
        D = np.zeros((5, 5), np.float32)
        for k in range(0, len(bump), 2):
            D[bump[k]] = bump[k + 1]
        assert qref.accumulate(D, 0.0, True)[1][3, 3] == move, bump
    # two equal minima of the last row: the smaller column ends the path; a NaN never replaces a candidate, nor is replaced
    D = np.array([[5, 1, 5, 1, 5], [5, 5, 2, 5, 2]], np.float32)
    for slope in (False, True):
        pos, (begin, end), cost, last = qref.dtw(D, 0.0, slope)
        assert (begin, end) == (1, 2) and cost == 3 and list(pos) == [1, 2]
    assert qref.end_of(np.array([np.nan, 1, 0], np.float32), 0) == 0
    assert qref.end_of(np.array([3, np.nan, 3, 2, np.nan, 2], np.float32), 0) == 3
    assert qref.end_of(np.array([9, 4, 1, 1], np.float32), 2) == 2


def test_row_0_is_free_and_column_0_is_forced():
    z = np.float32
    D = (np.array([[7, 1, 9, 3], [9, 9, 2, 9], [1, 9, 9, 4]], np.float32) * z(0.1)).astype(np.float32)
    acc, mv, _ = qref.accumulate(D, 0.3, False)
    assert acc.dtype == np.float32 and np.array_equal(acc[0], D[0])
    assert acc[1, 0] == (D[0, 0] + z(0.3)) + D[1, 0] and mv[1, 0] == 1 and mv[2, 0] == 1
    assert acc[2, 0] == (acc[1, 0] + z(0.3)) + D[2, 0]
    assert acc[1, 2] == D[0, 1] + D[1, 2] and mv[1, 2] == 0          # the diagonal pays no step
    pos, (begin, end), cost, last = qref.dtw(D, 0.3, False)
    assert (begin, end) == (1, 3) and cost == acc[2, 3] == (D[0, 1] + D[1, 2]) + D[2, 3] and list(pos) == [1, 2, 3]
    assert np.array_equal(last, acc[2])
    # one row and one column
    pos, span, cost, last = qref.dtw(np.array([[4, 2, 3, 2]], np.float32), 5.0, False)
    assert list(pos) == [1] and span == (1, 1) and cost == 2 and list(last) == [4, 2, 3, 2]
    pos, span, cost, last = qref.dtw(np.array([[4, 2, 3, 2]], np.float32), 5.0, True)
    assert list(pos) == [1] and span == (1, 1) and cost == 2
    pos, span, cost, last = qref.dtw(np.array([[1], [2], [4]], np.float32), 0.5, False)
    assert list(pos) == [0, 0, 0] and span == (0, 0) and cost == 8 and cost.dtype == np.float32
    assert qref.dtw(np.array([[3.25]]), 7.0, True)[2].dtype == np.float64
    with pytest.raises(AssertionError):
        qref.dtw(np.zeros((4, 2), np.float32), 0.0, True)            # ceil(3 / 2) = 2 > 1
    # the pattern: 3 x 2 from (0, 0) through (1, 1), step_cost after the cell in between and before the cell's own distance
    D = (np.array([[1, 9], [9, 2], [9, 4]], np.float32) * z(0.1)).astype(np.float32)
    pos, span, cost, last = qref.dtw(D, 0.3, True)
    assert span == (0, 1) and cost == ((D[0, 0] + D[1, 1]) + z(0.3)) + D[2, 1] and list(pos) == [0, 1, 1]
    assert last[0] == np.inf and last[1] == cost


@pytest.mark.parametrize("slope", [False, True], ids=["plain", "slope"])
def test_a_nan_row_keeps_the_walk_inside(slope):
    rng = np.random.default_rng(5)
    for na, nb, nan_rows in ((9, 7, [4]), (7, 9, [0]), (6, 6, [5]), (5, 8, [0, 1, 2, 3, 4]), (64, 127, [10, 11]), (9, 5, [3, 4])):
        D = rng.random((na, nb)).astype(np.float32)
        D[nan_rows] = np.nan
        pos, (begin, end), cost, last = qref.dtw(D, 1.0, slope)     # (path asserts the bound on the moves and the matrix itself)
        lo = int(qref.rows(na, nb, slope)[0][-1])
        assert end == lo and np.isnan(cost) and 0 <= begin <= end <= nb - 1  # a NaN is never strictly smaller: the first column stays
        assert not np.any(np.isnan(pos)) and pos[0] == begin and np.all(pos >= begin) and np.all(pos <= end)


def consequences(D, step_cost, slope):
    """what llsm_gpu.h states of the outputs, on a plane of finite values"""
    na, nb = D.shape
    pos, (begin, end), cost, last = qref.dtw(D, step_cost, slope)
    assert 0 <= begin <= end <= nb - 1 and pos[0] == begin
    assert np.all(pos >= begin) and np.all(pos <= end) and np.all(np.diff(pos) >= 0)
    assert cost == last[end] and np.all(~(last < cost)) and np.all(last[:end] > cost)
    if not slope:
        assert pos[-1] == end
        assert cost <= aref.dtw(D, step_cost)[1]
    else:
        assert pos[-1] in (end, end - 0.5)
        d1 = np.diff(pos)
        assert np.all(d1 <= 2) and np.all(pos[2:] - pos[:-2] >= 1) and np.all((pos * 2) % 1 == 0)
        if sref.admissible(na, nb):
            assert cost <= sref.dtw(D, step_cost)[1]
    return begin, end


def test_consequences_on_random_planes():
    rng = np.random.default_rng(77)
    done = 0
    while done < 300:
        na, nb = (int(x) for x in rng.integers(1, 41, 2))
        slope = bool(done % 2)
        if not qref.admissible(na, nb, slope):
            continue
        D = rng.integers(0, 4, (na, nb)).astype(np.float32) if done % 3 else rng.random((na, nb)).astype(np.float32)
        consequences(D, float(rng.integers(0, 3)), slope)
        done += 1


# ---------------------------------------------------------------- queries planted in takes
_plants = {}


def planted(shape, seed, slope):
    """(float32 chain, float64 chain, truth, pos of rules D1 - D3) of one planted query, computed once"""
    key = (shape, seed, slope)
    if key not in _plants:
        A, B, truth = qref.plant(seed, *shape)
        A = A.astype(np.float32); B = B.astype(np.float32)
        _plants[key] = (qref.align(A, B, 0, 24, step_cost=1.0, slope=slope),
                        qref.align(A, B, 0, 24, step_cost=1.0, slope=slope, dtype=np.float64), truth,
                        aref.align(A, B, 0, 24, step_cost=1.0)[0])
    return _plants[key]


def rms(x):
    return float(np.sqrt(np.mean(np.square(x))))


@pytest.mark.parametrize("slope", [False, True], ids=["plain", "slope"])
def test_planted_queries(slope):
    differ = total = 0
    worst_cost = worst_rms = 0.0
    least_ratio = np.inf
    for shape in (SLOPE_PLANTS if slope else PLAIN_PLANTS):
        na, nm, n0, n1 = shape
        for seed in SEEDS:
            (p32, s32, c32, l32), (p64, s64, c64, l64), truth, full = planted(shape, seed, slope)
            assert p32.dtype == np.float32 and c32.dtype == np.float32 and c64.dtype == np.float64 and l32.dtype == np.float32
            differ += int(np.count_nonzero(p32 != p64)); total += len(p32)
            worst_cost = max(worst_cost, abs(float(c32) - float(c64)) / float(c64))
            assert abs(s32[0] - n0) <= 2 and abs(s32[1] - (n0 + nm - 1)) <= 2, (shape, seed, s32)
            err = rms(p32.astype(np.float64) - truth); miss = rms(full.astype(np.float64) - truth)
            print("plant%s seed %d: span %s for [%d, %d], RMS %.3f frames, rules D1 - D3 %.1f" % (shape, seed, s32, n0, n0 + nm - 1, err, miss))
            assert err <= 1.5, (shape, seed, err)
            assert miss > 10 * err, (shape, seed, miss, err)
            worst_rms = max(worst_rms, err); least_ratio = min(least_ratio, miss / err)
    print("float32 against float64: %d of %d frames differ, cost within %.2g relative; RMS to the truth at most %.3f frames; rules D1 - D3 "
          "miss by at least %.0f times that" % (differ, total, worst_cost, worst_rms, least_ratio))
    assert total == 12 * sum(s[0] for s in PLAIN_PLANTS)
    assert differ <= DIFFER_CAP * total
    assert worst_cost <= COST_REL
