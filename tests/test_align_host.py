"""Host side of llsm_gpu_batch_align (no GPU): the default options, the refusals of llsm_gpu_align_check, and the numpy
restatement of rules D1 - D3 (tests/align_reference.py) on its own: planes written by hand, float32 against the same code
in float64, and the quality of the alignment against the generator's truth -- a property of the rules, checked here and
not on the device.

Measured with align_reference.make(seed, na, nb, 24, 0.3), step_cost 1, the four sizes below, seeds 0 ... 11: the float32
chain differs from the float64 chain on 0 of 8 316 frames, cost agrees to 4e-7 relative; against the truth the mean |error|
is 0.12 ... 0.27 frames and the largest 0.46 ... 1.64 (printed by the tests)."""
import ctypes as C

import numpy as np
import pytest

import libllsm2_amd as llsm
import align_reference as aref
from align_common import COST_REL, DIFFER_CAP, FULL_SIZES as SIZES, SEEDS, full_case as case


def test_default_options():
    o = llsm.AlignOptions()
    llsm.load().llsm_gpu_align_default_options(C.byref(o))
    assert (o.first, o.count, o.step_cost, o.voicing_cost) == (3, 0, 0.0, 0.0)
    m = llsm.make_align_options(step_cost=1.0, count=7)
    assert (m.first, m.count, m.step_cost, m.voicing_cost) == (3, 7, 1.0, 0.0)
    with pytest.raises(TypeError):
        llsm.make_align_options(threshold=0.1)


nan, inf = float("nan"), float("inf")
# with orders 8 + 2 the vectors have 13 columns; a count <= 0 stands for order_spec = 8, so first = 12 alone means [12, 20)
REFUSED = [dict(first=-1), dict(first=13), dict(first=12), dict(first=3, count=11), dict(first=0, count=14), dict(first=12, count=2),
           dict(first=2 ** 31 - 1, count=2 ** 31 - 1),
           dict(step_cost=nan), dict(voicing_cost=nan), dict(step_cost=inf), dict(voicing_cost=inf), dict(step_cost=-inf),
           dict(step_cost=-1e-6), dict(voicing_cost=-1.0)]


@pytest.mark.parametrize("kw", REFUSED, ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()))
def test_check_refusals(kw):
    L = llsm.load()
    o = llsm.make_align_options(**kw)
    assert L.llsm_gpu_align_check(C.byref(o), 8, 2) == -1
    assert L.llsm_gpu_last_error().decode().startswith("llsm_gpu_batch_align:")


@pytest.mark.parametrize("orders", [(0, 2), (8, 0), (-1, 2)])
def test_check_refuses_a_coder_that_is_not_enabled(orders):
    L = llsm.load()
    assert L.llsm_gpu_align_check(None, *orders) == -1
    assert L.llsm_gpu_last_error().decode().startswith("llsm_gpu_batch_align:")


def test_check_accepts_edges_and_null():
    L = llsm.load()
    assert L.llsm_gpu_align_check(None, 8, 2) == 0
    for kw in (dict(), dict(first=0, count=13), dict(first=12, count=1), dict(first=3, count=-5), dict(first=5),
               dict(step_cost=0.0, voicing_cost=0.0), dict(step_cost=1e30, voicing_cost=1e30)):
        o = llsm.make_align_options(**kw)
        assert L.llsm_gpu_align_check(C.byref(o), 8, 2) == 0, kw


def test_align_refuses_null_batch():
    L = llsm.load()
    pos = np.full(4, -7, np.float32)
    assert L.llsm_gpu_batch_align(None, None, 0, None, None, None, pos.ctypes.data_as(llsm.P_fp), None) == -1
    assert L.llsm_gpu_last_error().decode().startswith("llsm_gpu_batch_align:")
    assert np.all(pos == -7)


# ---------------------------------------------------------------- planes written by hand
def test_ties_take_the_diagonal_then_move_1():
    """a constant plane with step_cost 0: every comparison ties, so the diagonal wins wherever there is one; the path is
    the diagonal from the end and then the forced border"""
    for na, nb in ((5, 5), (3, 7), (7, 3)):
        D = np.ones((na, nb), np.float32)
        acc, mv = aref.accumulate(D, 0.0)
        assert np.all(mv[1:, 1:] == 0) and np.all(mv[0, 1:] == 2) and np.all(mv[1:, 0] == 1) and mv[0, 0] == 0
        pos, n = aref.backtrack(mv)
        assert n == max(na, nb) - 1
        if na <= nb:                                  # row 0 covers columns 0 ... nb - na
            want = np.arange(na) + (nb - na); want = want.astype(np.float32); want[0] = (nb - na) * 0.5
        else:                                         # column 0 covers rows 0 ... na - nb
            want = np.maximum(np.arange(na) - (na - nb), 0).astype(np.float32)
        assert np.array_equal(pos, want), (na, nb, pos)
    # 2 x 2, step_cost 0: cell (1, 1) compares acc[0][0] = 9, then up = acc[0][1], then left = acc[1][0]
    for D, move, value in (([[9, 1], [1, 1]], 0, 10),           # 10 and 10 do not beat 9
                           ([[9, -5], [-5, 1]], 1, 5),          # up = left = 4: up is compared first and "<" keeps it
                           ([[9, -6], [-5, 1]], 1, 4),          # up = 3, left = 4
                           ([[9, -5], [-6, 1]], 2, 4)):         # up = 4, left = 3
        acc, mv = aref.accumulate(np.array(D, np.float32), 0.0)
        assert mv[1, 1] == move and acc[1, 1] == value, D


def test_step_cost_is_added_before_the_distance():
    D = np.array([[1, 2, 4]], np.float32) * np.float32(0.1)
    acc, mv = aref.accumulate(D, 0.3)
    z = np.float32
    assert acc[0, 1] == (D[0, 0] + z(0.3)) + D[0, 1] and acc[0, 2] == (acc[0, 1] + z(0.3)) + D[0, 2]
    assert acc.dtype == np.float32


@pytest.mark.parametrize("n", [1, 2, 9])
def test_single_row_and_single_column(n):
    rng = np.random.default_rng(n)
    D = rng.random((1, n)).astype(np.float32)
    pos, cost = aref.dtw(D, 0.0)
    assert pos.dtype == np.float32 and list(pos) == [np.float32((n - 1) * 0.5)]
    s = D[0, 0]
    for j in range(1, n):
        s = np.float32(s + np.float32(0.0)) + D[0, j]
    assert cost == s
    pos, cost = aref.dtw(np.ascontiguousarray(D.T), 0.0)
    assert list(pos) == [0.0] * n and cost == s


def test_a_nan_row_keeps_the_walk_inside():
    rng = np.random.default_rng(5)
    for na, nb, rows in ((9, 7, [4]), (7, 9, [0]), (6, 6, [5]), (5, 8, [0, 1, 2, 3, 4])):
        D = rng.random((na, nb)).astype(np.float32)
        D[rows] = np.nan
        acc, mv = aref.accumulate(D, 1.0)
        pos, n = aref.backtrack(mv)                   # (asserts the bound on the number of moves itself)
        assert n <= na + nb - 2
        assert np.all(pos >= 0) and np.all(pos <= nb - 1) and not np.any(np.isnan(pos))
        assert np.all(np.diff(pos) >= 0)


def test_dist_by_hand():
    z = np.float32
    fa = np.array([[1, 0, 0, 0.1, 0.2, 0.3], [0, 0, 0, 1.5, -2.5, 3.5]], np.float32)
    fb = np.array([[0.6, 9, 9, 0.3, 0.1, 0.1], [0.5, 9, 9, 0, 0, 0], [np.nan, 9, 9, 1.5, -2.5, 3.5]], np.float32)
    D = aref.dist(fa, fb, 3, 3, 5.0)
    assert D.dtype == np.float32 and D.shape == (2, 3)
    t = [fa[0, k] - fb[0, k] for k in (3, 4, 5)]
    assert D[0, 0] == (z(0) + t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]           # both voiced: no voicing cost
    assert D[1, 2] == 0 and D[1, 1] == (z(1.5) * z(1.5) + z(2.5) * z(2.5)) + z(3.5) * z(3.5)   # 0.5 and NaN are not > 0.5
    assert D[0, 1] == ((fa[0, 3] * fa[0, 3] + fa[0, 4] * fa[0, 4]) + fa[0, 5] * fa[0, 5]) + z(5)
    assert D[1, 0] > 5 and aref.dist(fa, fb, 0, 1, 0.0)[0, 1] == z(0.25)
    assert np.isnan(aref.dist(fa, fb, 0, 1, 0.0)[0, 2])


# ---------------------------------------------------------------- float32 against float64, and against the truth
def test_float32_against_float64():
    differ = total = 0
    worst = 0.0
    for size in SIZES:
        for seed in SEEDS:
            (p32, c32), (p64, c64), _ = case(size, seed)
            assert p32.dtype == np.float32 and c32.dtype == np.float32 and c64.dtype == np.float64
            differ += int(np.count_nonzero(p32 != p64)); total += len(p32)
            worst = max(worst, abs(float(c32) - float(c64)) / float(c64))
    print("float32 against float64: %d of %d frames differ, cost within %.2g relative" % (differ, total, worst))
    assert total == 12 * (200 + 64 + 129 + 300)
    assert differ <= DIFFER_CAP * total
    assert worst <= COST_REL


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_quality_against_the_truth(size):
    for seed in SEEDS:
        (pos, _), _, truth = case(size, seed)
        err = np.abs(pos.astype(np.float64) - truth)
        print("make(%d, %d, %d): mean |error| %.3f frames, max %.3f" % (seed, size[0], size[1], err.mean(), err.max()))
        assert err.mean() <= 0.5 and err.max() <= 2.5, (size, seed)
        assert np.all(np.diff(pos) >= 0) and pos[0] >= 0 and pos[-1] <= size[1] - 1
