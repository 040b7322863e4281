"""Host side of llsm_gpu_batch_align_slope (no GPU): llsm_gpu_align_slope_rows against Python integers, and the numpy
restatement of rules L1 - L4 (tests/align_slope_reference.py) on its own: the region, every path of small planes by
enumeration, planes written by hand, the properties of pos that follow from the rules, float32 against the same code in
float64, the quality against the generator's truth, and the stall that the rule is there to remove.

Measured with align_reference.make(seed, na, nb, 24, 0.3), step_cost 1, seeds 0 ... 11: the float32 chain differs from the
float64 chain on 0 of 8 316 frames of (200, 170), (64, 65), (129, 90), (300, 410), cost within 5.2e-7 relative; against the
truth on (200, 170), (64, 65), (129, 90), (300, 360) the mean |error| is at most 0.27 frames and the largest 0.94 (printed
by the tests)."""
import numpy as np
import pytest

import libllsm2_amd as llsm
import align_reference as aref
import align_slope_reference as sref
from align_common import COST_REL, DIFFER_CAP, SEEDS, SLOPE_SIZES as SIZES, slope_case as case, slope_properties as check_properties

QUALITY_SIZES = [(200, 170), (64, 65), (129, 90), (300, 360)]      # the warp of (300, 410) exceeds slope 2 in places
LARGER = [(64, 127), (129, 65), (127, 64), (65, 129), (1000, 1999), (1999, 1000), (1000, 2000), (2001, 1000), (5000, 4001),
          (16400, 16400)]


def shapes():
    return [(na, nb) for na in range(1, 71) for nb in range(1, 71)] + LARGER


# ---------------------------------------------------------------- L1: the host call
def raw_rows(na, nb, lo=True, hi=True):
    L = llsm.load()
    n = max(na, 1) if na <= 20000 else 1
    a = np.full(n, -7, np.int32); b = np.full(n, -7, np.int32)
    rc = L.llsm_gpu_align_slope_rows(na, nb, a.ctypes.data_as(llsm.P_int) if lo else None, b.ctypes.data_as(llsm.P_int) if hi else None)
    return rc, L.llsm_gpu_last_error().decode(), a, b


def test_rows_against_python_integers():
    accepted = refused = single = 0
    for na, nb in shapes():
        rc, msg, lo, hi = raw_rows(na, nb)
        why = sref.bound(na, nb)
        if why is None:
            want_lo, want_hi = sref.rows(na, nb)
            assert rc == 0 and np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi), (na, nb)
            assert lo[0] == 0 and hi[0] == 0 and hi[-1] == nb - 1 and lo[-1] == nb - 1
            assert np.all(np.diff(lo) >= 0) and np.all(np.diff(hi) >= 0) and np.all(lo >= 0) and np.all(hi <= nb - 1)
            assert llsm.load().llsm_gpu_align_slope_rows(na, nb, None, None) == 0     # only asks whether it is admissible
            for keep_lo in (True, False):                                             # one of them alone
                rc, _, l1, h1 = raw_rows(na, nb, lo=keep_lo, hi=not keep_lo)
                assert rc == 0 and (np.array_equal(l1, want_lo) and np.all(h1 == -7) if keep_lo else
                                    np.array_equal(h1, want_hi) and np.all(l1 == -7)), (na, nb)
            lib_lo, lib_hi = llsm.align_slope_rows(na, nb)
            assert np.array_equal(lib_lo, want_lo) and np.array_equal(lib_hi, want_hi)
            accepted += 1
            single += bool(np.all(hi - lo <= 0))
        else:
            name, value, limit = why
            needle = "%s = %d exceeds 2 (%s) = %d" % (name, value, "na - 1" if name == "nb - 1" else "nb - 1", limit)
            assert rc == -1 and msg.startswith("llsm_gpu_align_slope_rows:") and needle in msg, (na, nb, msg)
            assert ("%d x %d" % (na, nb)) in msg and np.all(lo == -7) and np.all(hi == -7)
            assert llsm.load().llsm_gpu_align_slope_rows(na, nb, None, None) == -1
            with pytest.raises(llsm.LlsmError):
                llsm.align_slope_rows(na, nb)
            refused += 1
    assert accepted > 2400 and refused > 2400 and single > 60
    for na, nb in ((64, 127), (129, 65)):                           # every row a single cell or passed through
        lo, hi = llsm.align_slope_rows(na, nb)
        assert np.all(hi - lo <= 0)
    lo, hi = llsm.align_slope_rows(129, 65)
    assert np.all(lo[1::2] == hi[1::2] + 1) and np.all(lo[::2] == hi[::2])
    lo, hi = llsm.align_slope_rows(3, 2)
    assert list(lo) == [0, 1, 1] and list(hi) == [0, 0, 1]


def test_rows_refuses_sizes_below_one_and_takes_64_bits():
    L = llsm.load()
    for na, nb in ((0, 1), (1, 0), (-3, 4), (4, -3), (0, 0)):
        rc, msg, lo, hi = raw_rows(na, nb)
        assert rc == -1 and msg.startswith("llsm_gpu_align_slope_rows:") and "na < 1 or nb < 1" in msg, msg
        assert ("na = %d" % na) in msg and ("nb = %d" % nb) in msg and np.all(lo == -7)
    # bounds near 2^31: taken in 64-bit
    assert L.llsm_gpu_align_slope_rows(2 ** 30, 2 ** 31 - 1, None, None) == 0
    assert L.llsm_gpu_align_slope_rows(2 ** 30, 2 ** 30 + 5, None, None) == 0
    assert L.llsm_gpu_align_slope_rows(2 ** 30 - 1, 2 ** 31 - 1, None, None) == -1
    assert "nb - 1 = %d exceeds 2 (na - 1) = %d" % (2 ** 31 - 2, 2 ** 31 - 4) in L.llsm_gpu_last_error().decode()
    assert L.llsm_gpu_align_slope_rows(2 ** 31 - 1, 2 ** 30, None, None) == 0
    assert L.llsm_gpu_align_slope_rows(2 ** 31 - 1, 2 ** 30 - 1, None, None) == -1


def test_every_region_cell_has_a_predecessor_and_is_on_a_path():
    for na, nb in shapes():
        if not sref.admissible(na, nb) or na > 300:
            continue
        inside = sref.region(na, nb)
        ii, jj = np.nonzero(inside)
        have = np.zeros(len(ii), bool)
        for (di, dj), _ in sref.MOVES:
            ok = (ii >= di) & (jj >= dj)
            have |= ok & inside[np.maximum(ii - di, 0), np.maximum(jj - dj, 0)]
        assert have[0] == False and (ii[0], jj[0]) == (0, 0) and np.all(have[1:]), (na, nb)   # noqa: E712
    # the region is the cells on some path from (0, 0) to the end, by reachability both ways, up to 40 x 40
    count = 0
    for na in range(1, 41):
        for nb in range(1, 41):
            fwd = np.zeros((na, nb), bool); fwd[0, 0] = True
            for i in range(na):
                for j in range(nb):
                    fwd[i, j] |= any(i >= di and j >= dj and fwd[i - di, j - dj] for (di, dj), _ in sref.MOVES)
            if not sref.admissible(na, nb):
                assert not fwd[-1, -1], (na, nb)                     # and no path at all where the pair is refused
                continue
            bwd = np.zeros((na, nb), bool); bwd[-1, -1] = True
            for i in range(na - 1, -1, -1):
                for j in range(nb - 1, -1, -1):
                    bwd[i, j] |= any(i + di < na and j + dj < nb and bwd[i + di, j + dj] for (di, dj), _ in sref.MOVES)
            assert np.array_equal(fwd & bwd, sref.region(na, nb)), (na, nb)
            count += 1
    assert count == 800


# ---------------------------------------------------------------- L3 - L4 against every path
def test_reference_against_enumeration():
    cases = 0
    for na in range(1, 8):
        for nb in range(1, 8):
            for seed in range(5):
                D = np.random.default_rng(100 * na + 10 * nb + seed).integers(0, 6, (na, nb)).astype(np.float32)
                best, n = sref.brute_force(D, 2.0)
                if not sref.admissible(na, nb):
                    assert n == 0
                    continue
                pos, cost = sref.dtw(D, 2.0)
                assert n >= 1 and cost == best, (na, nb, seed, cost, best)
                # the path of the reference costs what acc says, summed along its cells
                acc, mv, _ = sref.accumulate(D, 2.0)
                cells, moves = sref.path(mv)
                assert moves <= min(na, nb) - 1 and cells[0] == (na - 1, nb - 1) and cells[-1] == (0, 0)
                steps = len(cells) - 1 - moves                       # the moves that pass a cell in between
                assert sum(D[c] for c in cells) + 2.0 * steps == cost
                cases += 1
    assert cases == 125


# ---------------------------------------------------------------- planes written by hand
def test_ties_take_move_0_then_1_then_2():
    # 5 x 5, step_cost 0: cell (3, 3) has all three predecessors inside: (2, 2), (1, 2) through (2, 3), (2, 1) through (3, 2)
    inside = sref.region(5, 5)
    assert inside[2, 2] and inside[1, 2] and inside[2, 1] and inside[3, 3]
    for bump, move in (((), 0),                                     # all equal: move 0
                       (((2, 2), 1), 1),                            # the diagonal dearer: 1 and 2 tie, 1 is compared first
                       (((2, 2), 1, (2, 3), 1), 2),                 # move 1 dearer as well
                       (((2, 2), 1, (3, 2), 1), 1)):
        D = np.zeros((5, 5), np.float32)
        for k in range(0, len(bump), 2):
            D[bump[k]] = bump[k + 1]
        acc, mv, _ = sref.accumulate(D, 0.0)
        assert mv[3, 3] == move, (bump, mv[3, 3], acc)
    # a constant plane, step_cost 0: every comparison ties; the diagonal where the region has it
    for na, nb in ((5, 5), (4, 6), (6, 4), (64, 65)):
        acc, mv, inside = sref.accumulate(np.ones((na, nb), np.float32), 0.0)
        i, j = np.nonzero(inside)
        dg = (i >= 1) & (j >= 1) & inside[i - 1, j - 1]
        assert np.all(mv[i[dg], j[dg]] == 0) and np.all(mv[~inside] == -1)
        up = ~dg & (i >= 2) & (j >= 1) & inside[i - 2, j - 1]
        assert np.all(mv[i[up], j[up]] == 1)
        rest = ~dg & ~up; rest[0] = False
        assert np.all(mv[i[rest], j[rest]] == 2)


def test_step_cost_comes_after_the_cell_between_and_before_the_cells_own_distance():
    z = np.float32
    # 3 x 2: (0, 0) -> (2, 1) through (1, 1) is the only path; row 1 is empty
    D = (np.array([[1, 9], [9, 2], [9, 4]], np.float32) * z(0.1)).astype(np.float32)
    acc, mv, inside = sref.accumulate(D, 0.3)
    assert acc.dtype == np.float32 and mv[2, 1] == 1 and not inside[1].any()
    assert acc[2, 1] == ((D[0, 0] + D[1, 1]) + z(0.3)) + D[2, 1]
    # 2 x 3: move 2 from (0, 0) to (1, 2) through (1, 1)
    acc, mv, _ = sref.accumulate(np.ascontiguousarray(D.T), 0.3)
    assert mv[1, 2] == 2 and acc[1, 2] == ((D[0, 0] + D[1, 1]) + z(0.3)) + D[2, 1]


def test_three_by_two_and_one_by_one():
    D = np.array([[1, 50], [60, 2], [70, 4]], np.float32)
    pos, cost = sref.dtw(D, 0.5)
    assert pos.dtype == np.float32 and list(pos) == [0.0, 1.0, 1.0] and cost == 7.5
    cells, n = sref.path(sref.accumulate(D, 0.5)[1])
    assert cells == [(2, 1), (1, 1), (0, 0)] and n == 1
    pos, cost = sref.dtw(np.ascontiguousarray(D.T), 0.5)
    assert list(pos) == [0.0, 1.5] and cost == 7.5
    pos, cost = sref.dtw(np.array([[3.25]], np.float32), 7.0)
    assert list(pos) == [0.0] and cost == np.float32(3.25) and cost.dtype == np.float32
    assert sref.dtw(np.array([[3.25]]), 7.0)[1].dtype == np.float64
    with pytest.raises(AssertionError):
        sref.dtw(np.zeros((1, 2), np.float32), 0.0)


def test_a_nan_row_keeps_the_walk_inside():
    rng = np.random.default_rng(5)
    for na, nb, nan_rows in ((9, 7, [4]), (7, 9, [0]), (6, 6, [5]), (5, 8, [0, 1, 2, 3, 4]), (64, 127, [10, 11]), (9, 5, [3, 4])):
        D = rng.random((na, nb)).astype(np.float32)
        D[nan_rows] = np.nan
        acc, mv, inside = sref.accumulate(D, 1.0)
        cells, n = sref.path(mv)                      # (asserts the bound on the number of moves itself)
        assert n <= min(na, nb) - 1 and inside[cells[0]] and inside[cells[-1]]
        pos = sref.positions(cells, na)
        check_properties(pos, na, nb)
        assert np.isnan(acc[-1, -1])


def test_properties_of_pos_on_random_planes():
    rng = np.random.default_rng(77)
    shapes_done = 0
    while shapes_done < 292:
        na, nb = (int(x) for x in rng.integers(1, 41, 2))
        if not sref.admissible(na, nb):
            continue
        D = rng.integers(0, 4, (na, nb)).astype(np.float32)
        if shapes_done % 10 == 0:
            D[rng.random((na, nb)) < 0.3] = np.nan                  # every tenth plane has NaN cells
        acc, mv, inside = sref.accumulate(D, float(rng.integers(0, 3)))
        cells, n = sref.path(mv)
        assert n <= min(na, nb) - 1
        ends = [c for c in cells if mv[c] >= 0]
        assert all(inside[c] for c in ends[:1] + ends[-1:])
        pos = sref.positions(cells, na)
        check_properties(pos, na, nb)
        shapes_done += 1


# ---------------------------------------------------------------- float32 against float64, the truth, the full rule
def test_float32_against_float64():
    differ = total = 0
    worst = 0.0
    for size in SIZES:
        for seed in SEEDS:
            (p32, c32), (p64, c64), _, _ = case(size, seed)
            assert p32.dtype == np.float32 and c32.dtype == np.float32 and c64.dtype == np.float64
            differ += int(np.count_nonzero(p32 != p64)); total += len(p32)
            worst = max(worst, abs(float(c32) - float(c64)) / float(c64))
    print("float32 against float64: %d of %d frames differ, cost within %.2g relative" % (differ, total, worst))
    assert total == 12 * (200 + 64 + 129 + 300)
    assert differ <= DIFFER_CAP * total
    assert worst <= COST_REL


@pytest.mark.parametrize("size", QUALITY_SIZES, ids=lambda s: "%dx%d" % s)
def test_quality_against_the_truth(size):
    for seed in SEEDS:
        if size in SIZES:
            pos = case(size, seed)[0][0]
        else:
            A, B, _ = aref.make(seed, size[0], size[1], 24, 0.3)
            pos = sref.align(A.astype(np.float32), B.astype(np.float32), 0, 24, step_cost=1.0)[0]
        truth = aref.make(seed, size[0], size[1], 24, 0.3)[2]
        err = np.abs(pos.astype(np.float64) - truth)
        print("make(%d, %d, %d): mean |error| %.3f frames, max %.3f" % (seed, size[0], size[1], err.mean(), err.max()))
        assert err.mean() <= 0.5 and err.max() <= 2.5, (size, seed)
        check_properties(pos, *size)


def test_cost_is_never_below_the_full_rule():
    for size in SIZES:
        for seed in SEEDS:
            (_, c32), _, _, (_, full) = case(size, seed)
            assert c32.dtype == np.float32 and full.dtype == np.float32 and c32 >= full, (size, seed, c32, full)


def test_the_stall_that_the_rule_removes():
    """one frame of B held twelve times: rule D2 crosses the held stretch inside one row of A, this rule at slope 2"""
    A, B, _ = aref.make(3, 120, 120, 24, 0.05)
    B = np.concatenate([B[:60], np.repeat(B[60:61], 12, 0), B[61:]])
    assert B.shape == (131, 24)
    A = A.astype(np.float32); B = B.astype(np.float32)
    full = aref.align(A, B, 0, 24, step_cost=0.0)[0]
    slope = sref.align(A, B, 0, 24, step_cost=0.0)[0]
    print("largest step of pos: D2 %.1f, slope pattern %.1f" % (np.diff(full).max(), np.diff(slope).max()))
    assert np.diff(full).max() >= 6
    assert np.diff(slope).max() <= 2
    check_properties(slope, 120, 131)
