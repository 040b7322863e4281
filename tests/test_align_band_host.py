"""Host side of llsm_gpu_batch_align_band (no GPU): llsm_gpu_align_band_min and llsm_gpu_align_band_rows against Python
integer arithmetic (rule B1), and the numpy restatement of rules B1 - B4 (tests/align_band_reference.py) on its own: where
the band covers the matrix it is the full reference (tests/align_reference.py) bit for bit, at the least band every cell of
the path lies inside the band, and on the generated pairs a band of 15 % of nb finds the path and the cost of the full
search -- a property of the rules and the generator, checked here and not on the device."""
import ctypes as C
import math

import numpy as np
import pytest

import libllsm2_amd as llsm
import align_reference as aref
import align_band_reference as bref
from align_common import BAND_SIZES as SIZES, SEEDS

SHAPES = [(na, nb) for na in range(1, 71) for nb in range(1, 71)] + [(129, 200), (200, 129), (10, 1000), (2, 63), (60000, 59000)]
SMALL = [(1, 1), (1, 7), (7, 1), (2, 63), (63, 64), (64, 65), (65, 129), (5, 5)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def beq(a, b):
    a = np.asarray(a); b = np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------- B1: the two host functions
def least_band(na, nb):
    """the least connected band from the largest step of the centre: rows i and i + 1 touch iff 2 band + 1 >= c_{i+1} - c_i,
    and the last row ends on nb - 1 by itself unless it is the only one"""
    if na == 1:
        return nb - 1
    c = np.array(bref.centers(na, nb) if na < 1000 else [(2 * i * (nb - 1) + (na - 1)) // (2 * (na - 1)) for i in range(na)])
    return int(max(0, np.diff(c).max())) // 2


def test_band_min_by_trying():
    """the closed form above against the definition (try bands in turn), on the shapes where that is quick"""
    for na, nb in [(na, nb) for na in range(1, 24) for nb in range(1, 24)] + [(129, 200), (200, 129), (10, 1000), (2, 63)]:
        assert least_band(na, nb) == bref.band_min(na, nb), (na, nb)


def test_band_min_and_rows():
    L = llsm.load()
    assert [llsm.align_band_min(*s) for s in ((5, 3), (3, 3), (1, 9), (63, 64), (2, 63))] == [0, 0, 8, 1, 31]
    for na, nb in SHAPES:
        least = least_band(na, nb)
        assert llsm.align_band_min(na, nb) == least, (na, nb)
        for band in (least, least + 3):
            lo, hi = llsm.align_band_rows(na, nb, band)
            want_lo, want_hi = bref.rows(na, nb, band)
            assert lo.dtype == np.int32 and np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi), (na, nb, band)
            assert lo[0] == 0 and hi[-1] == nb - 1 and np.all(lo[1:] <= hi[:-1] + 1) and np.all(lo <= hi)
        if least > 0:                                               # one less is not connected: refused, and the least is named
            lo = np.full(na, -7, np.int32); hi = np.full(na, -7, np.int32)
            rc = L.llsm_gpu_align_band_rows(na, nb, least - 1, lo.ctypes.data_as(llsm.P_int), hi.ctypes.data_as(llsm.P_int))
            msg = L.llsm_gpu_last_error().decode()
            assert rc == -1 and msg.startswith("llsm_gpu_align_band_rows:") and str(least) in msg.split("least")[-1], (na, nb, msg)
            assert np.all(lo == -7) and np.all(hi == -7)
            assert not bref.connected(na, nb, least - 1)


def test_band_refusals():
    L = llsm.load()
    for na, nb in ((0, 5), (5, 0), (-1, 5), (5, -3)):
        assert L.llsm_gpu_align_band_min(na, nb) == -1
        assert L.llsm_gpu_last_error().decode().startswith("llsm_gpu_align_band_min:")
        with pytest.raises(llsm.LlsmError):
            llsm.align_band_min(na, nb)
        with pytest.raises(llsm.LlsmError):
            llsm.align_band_rows(na, nb, 3)
    with pytest.raises(llsm.LlsmError, match="band < 0"):
        llsm.align_band_rows(5, 5, -1)
    with pytest.raises(llsm.LlsmError, match="31"):
        llsm.align_band_rows(2, 63, 30)
    lo = np.zeros(5, np.int32)
    assert L.llsm_gpu_align_band_rows(5, 5, 1, None, lo.ctypes.data_as(llsm.P_int)) == -1
    assert L.llsm_gpu_align_band_rows(5, 5, 1, lo.ctypes.data_as(llsm.P_int), None) == -1


def test_align_band_refuses_null_batch():
    L = llsm.load()
    pos = np.full(4, -7, np.float32)
    band = np.zeros(1, np.int32)
    assert L.llsm_gpu_batch_align_band(None, None, 0, None, None, band.ctypes.data_as(llsm.P_int), None,
                                       pos.ctypes.data_as(llsm.P_fp), None) == -1
    assert L.llsm_gpu_last_error().decode().startswith("llsm_gpu_batch_align_band:")
    assert np.all(pos == -7)


# ---------------------------------------------------------------- the reference against the full reference
def planes(na, nb, seed):
    """float32 planes of one shape: random, small integers (accumulated costs tie often), 10 % NaN"""
    rng = np.random.default_rng(seed)
    out = dict(random=rng.random((na, nb)).astype(np.float32), integer=rng.integers(0, 3, (na, nb)).astype(np.float32))
    holes = rng.random((na, nb)).astype(np.float32)
    holes[rng.random((na, nb)) < 0.1] = np.nan
    out["nan"] = holes
    return out


@pytest.mark.parametrize("step_cost", [0.0, 1.0])
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "%dx%d" % s)
def test_a_band_over_the_whole_matrix_is_the_full_reference(shape, step_cost):
    na, nb = shape
    for kind, D in planes(na, nb, 100 * na + nb).items():
        want_pos, want_cost = aref.dtw(D, step_cost)
        for band in (max(nb - 1, 0), nb + 4):
            lo, hi = bref.rows(na, nb, band)
            assert np.all(lo == 0) and np.all(hi == nb - 1)
            pos, cost, cells = bref.dtw(D, band, step_cost)
            assert pos.dtype == np.float32 and cost.dtype == np.float32
            assert beq(pos, want_pos) and beq(cost, want_cost), (shape, kind, band)       # (NaN equals NaN: the bits)
            acc, mv, _ = bref.accumulate(D, band, step_cost)
            full_acc, full_mv = aref.accumulate(D, step_cost)
            assert beq(acc, full_acc) and np.array_equal(mv, full_mv), (shape, kind, band)
            # the band layout and back
            assert beq(bref.from_band(bref.to_band(D, band), nb), D)


@pytest.mark.parametrize("shape", SMALL + [(129, 200), (200, 129), (10, 1000)], ids=lambda s: "%dx%d" % s)
def test_at_the_least_band_the_path_stays_inside(shape):
    na, nb = shape
    least = bref.band_min(na, nb)
    lo, hi = bref.rows(na, nb, least)
    for kind, D in planes(na, nb, 7 * na + nb).items():
        for step_cost in (0.0, 1.0):
            pos, cost, cells = bref.dtw(D, least, step_cost)
            assert cells[0] == (na - 1, nb - 1) and cells[-1] == (0, 0) and len(cells) - 1 <= na + nb - 2
            assert all(lo[i] <= j <= hi[i] for i, j in cells), (shape, kind)
            assert np.all(pos >= lo) and np.all(pos <= hi) and np.all(np.diff(pos) >= 0) and not np.any(np.isnan(pos))
            # the cells outside the band are not read: garbage there changes nothing
            _, _, inside = bref.accumulate(D, least, step_cost)
            E = np.where(inside, D, np.float32(-1e30))
            pos2, cost2, cells2 = bref.dtw(E, least, step_cost)
            assert cells2 == cells and beq(pos2, pos) and beq(cost2, cost)
            P = bref.to_band(D, least)
            assert P.shape == (na, 2 * least + 1) and np.count_nonzero(np.isposinf(P)) == P.size - np.count_nonzero(inside)


def test_float64():
    D = planes(40, 57, 3)["random"].astype(np.float64)
    pos, cost, _ = bref.dtw(D, 56, 0.5)
    want_pos, want_cost = aref.dtw(D, 0.5)
    assert cost.dtype == np.float64 and beq(cost, want_cost) and beq(pos, want_pos)
    pos, cost, _ = bref.dtw(D, bref.band_min(40, 57) + 2, 0.5)
    assert cost.dtype == np.float64 and cost >= want_cost


# ---------------------------------------------------------------- generated pairs
_cases = {}


def case(size, seed):
    """(the float32 plane, (pos, cost) of the full reference) of one generated pair; computed once"""
    key = (size, seed)
    if key not in _cases:
        A, B, _ = aref.make(seed, size[0], size[1], 24, 0.3)
        D = aref.dist(A.astype(np.float32), B.astype(np.float32), 0, 24, 0.0)
        _cases[key] = (D, aref.dtw(D, 1.0))
    return _cases[key]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_a_band_of_15_percent_finds_the_full_path(size):
    """a condition, not a tolerance: the full path of every one of these pairs stays within ceil(0.15 nb) columns of the
    centres c_i (within 0.127 nb of them, 0.124 nb of the unrounded diagonal: printed), so the band holds it, and then the
    banded search gives its bits"""
    na, nb = size
    band = math.ceil(0.15 * nb)
    c = np.array(bref.centers(na, nb))
    line = np.arange(na) * ((nb - 1) / max(na - 1, 1))
    worst = worst_line = 0
    for seed in SEEDS:
        D, (want_pos, want_cost) = case(size, seed)
        _, mv = aref.accumulate(D, 1.0)
        cells = bref.path(mv)
        worst = max(worst, max(abs(j - c[i]) for i, j in cells))
        worst_line = max(worst_line, max(abs(j - line[i]) for i, j in cells))
        pos, cost, _ = bref.dtw(D, band, 1.0)
        assert beq(pos, want_pos) and beq(cost, want_cost), (size, seed)
    print("%d x %d: the full path stays within %d columns = %.3f nb of the centres (%.3f nb of the diagonal); band %d = %.3f nb"
          % (na, nb, worst, worst / nb, worst_line / nb, band, band / nb))
    assert worst <= band


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_a_narrow_band_costs_no_less(size):
    na, nb = size
    band = max(bref.band_min(na, nb), math.ceil(0.04 * nb))
    for seed in SEEDS:
        D, (_, want_cost) = case(size, seed)
        pos, cost, cells = bref.dtw(D, band, 1.0)
        assert cost >= want_cost, (size, seed, cost, want_cost)
        lo, hi = bref.rows(na, nb, band)
        assert all(lo[i] <= j <= hi[i] for i, j in cells)
