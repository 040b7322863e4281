"""Host side of llsm_gpu_batch_align_around (no GPU): llsm_gpu_align_around_rows / _around_min / _center_line against Python
integers and numpy float64, and the numpy restatement of rules A1 - A3 (tests/align_around_reference.py) on its own: the
sweeps of A1 against reachability cell by cell under straight and random centre lines -- the interval property of rule A1 is
measured here and not proven --, the closed form of the plain band against a search, the straight diagonal against the host
calls of the two straight bands, every path of small planes by enumeration, and every refusal with its message.

Measured by test_sweeps_against_reachability_*: no mismatch between the sweeps and the cell-by-cell sets, no two consecutive
empty rows in a connected region, lo and hi non-decreasing over the non-empty rows under every non-decreasing line."""
import numpy as np
import pytest

import libllsm2_amd as llsm
import align_band_reference as bref
import align_slope_reference as sref
import align_around_reference as rref


def raw_rows(na, nb, c, band, slope, lo=True, hi=True):
    L = llsm.load()
    n = max(na, 1) if lo or hi else 1
    a = np.full(n, -7, np.int32); b = np.full(n, -7, np.int32)
    cc = None if c is None else np.ascontiguousarray(c, np.int32)
    rc = L.llsm_gpu_align_around_rows(na, nb, None if cc is None else cc.ctypes.data_as(llsm.P_int), band, slope,
                                      a.ctypes.data_as(llsm.P_int) if lo else None, b.ctypes.data_as(llsm.P_int) if hi else None)
    return rc, L.llsm_gpu_last_error().decode(), a, b


def raw_min(na, nb, c, slope):
    L = llsm.load()
    cc = None if c is None else np.ascontiguousarray(c, np.int32)
    rc = L.llsm_gpu_align_around_min(na, nb, None if cc is None else cc.ctypes.data_as(llsm.P_int), slope)
    return rc, L.llsm_gpu_last_error().decode()


def random_line(rng, na, nb, monotone=True):
    """a centre line of na rows within [0, nb - 1]: increments 0 ... 5 from a small start, or with monotone=False any columns"""
    if not monotone:
        return rng.integers(0, nb, na)
    c = np.cumsum(np.concatenate([[rng.integers(0, 3)], rng.integers(0, 6, na - 1)]))
    return np.minimum(c, nb - 1)


def check_region(c, nb, band, monotone):
    """the sweeps against the cell-by-cell sets of one line and band; returns whether the band is connected"""
    na = len(c)
    p, q = rref.band_rows(c, nb, band)
    fwd, bwd = rref.reachable(na, nb, p, q)
    F, G = rref.sweeps(c, nb, band)
    for i in range(na):                                              # each sweep alone gives the reachable set of its direction
        assert np.array_equal(np.nonzero(fwd[i])[0], np.arange(F[i][0], F[i][1] + 1)), (list(c), nb, band, i)
        assert np.array_equal(np.nonzero(bwd[i])[0], np.arange(G[i][0], G[i][1] + 1)), (list(c), nb, band, i)
    lo, hi = (np.array(x) for x in rref.region_rows(c, nb, band))
    col = np.arange(nb)[None, :]
    inside = (col >= lo[:, None]) & (col <= hi[:, None])
    assert np.array_equal(fwd & bwd, inside), (list(c), nb, band)
    if not inside[-1].any():
        assert not inside.any()
        return False
    full = lo <= hi
    assert (lo[0], hi[0], lo[-1], hi[-1]) == (0, 0, nb - 1, nb - 1)
    assert not np.any(~full[1:] & ~full[:-1]), (list(c), nb, band)      # no two consecutive empty rows
    if monotone:
        assert np.all(np.diff(lo[full]) >= 0) and np.all(np.diff(hi[full]) >= 0), (list(c), nb, band)
    return True


# ---------------------------------------------------------------- A1: the sweeps against reachability cell by cell
def test_sweeps_against_reachability_straight_lines():
    """every admissible na, nb <= 40 under the straight diagonal, every band up to connected + 2; the library's rows on the
    connected ones"""
    planes = 0
    for na in range(1, 41):
        for nb in range(1, 41):
            if not sref.admissible(na, nb):
                continue
            c = bref.centers(na, nb)
            band, beyond = 0, 0
            while beyond < 3:
                ok = check_region(c, nb, band, True)
                rc, msg, lo, hi = raw_rows(na, nb, c, band, 1)
                if ok:
                    want_lo, want_hi = rref.rows(c, nb, band, 1)
                    assert rc == 0 and np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi), (na, nb, band)
                    beyond += 1; planes += 1
                else:
                    assert beyond == 0 and rc == -1 and np.all(lo == -7) and np.all(hi == -7), (na, nb, band, msg)
                band += 1
    assert planes > 2000, planes                                     # (three bands of some 800 admissible pairs)


def test_sweeps_against_reachability_random_lines():
    """seeded lines, four in five non-decreasing with increments 0 ... 5 and one in five arbitrary (which the library refuses
    and the reference alone sweeps), at every band up to connected + 2"""
    rng = np.random.default_rng(2024)
    connected = lines = 0
    while lines < 1500:
        na, nb = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        if not sref.admissible(na, nb):
            continue
        monotone = lines % 5 != 4
        c = random_line(rng, na, nb, monotone)
        lines += 1
        band, beyond, was = 0, 0, False
        while beyond < 3 and band <= nb:
            ok = check_region(c, nb, band, monotone)
            assert ok or not was, (list(c), nb, band)                # monotone in the band
            was = ok
            if monotone:
                rc, msg, lo, hi = raw_rows(na, nb, c, band, 1)
                if ok:
                    want_lo, want_hi = rref.rows(c, nb, band, 1)
                    assert rc == 0 and np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi), (list(c), nb, band)
                else:
                    assert rc == -1 and "is not connected for the slope pattern around this line" in msg, msg
            beyond += ok; connected += ok
            band += 1
        if monotone:
            least = rref.band_min(c, nb, 1)
            assert raw_min(na, nb, c, 1)[0] == least == llsm.align_around_min(na, nb, c, slope=True), (list(c), nb)
            rc, msg, _, _ = raw_rows(na, nb, c, least - 1, 1) if least > 0 else (-1, "llsm_gpu_align_around_min is 0", 0, 0)
            assert rc == -1 and ("llsm_gpu_align_around_min is %d" % least) in msg, msg
    assert connected > 3000, connected


# ---------------------------------------------------------------- A1: the plain band
def test_plain_rows_and_min_against_closed_form_and_search():
    rng = np.random.default_rng(7)
    cases = 0
    for _ in range(1500):
        na, nb = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        c = random_line(rng, na, nb)
        least = rref.band_min(c, nb, 0)
        assert least == rref.band_min_plain(c, nb), (list(c), nb)
        assert raw_min(na, nb, c, 0)[0] == least == llsm.align_around_min(na, nb, c), (list(c), nb)
        for band in range(0, least + 3):
            rc, msg, lo, hi = raw_rows(na, nb, c, band, 0)
            if band < least:
                assert not rref.connected_plain(c, nb, band)
                assert rc == -1 and msg.startswith("llsm_gpu_align_around_rows:") and np.all(lo == -7) and np.all(hi == -7)
                assert ("a band of %d is not connected around this line on %d x %d frames" % (band, na, nb)) in msg, msg
                assert ("llsm_gpu_align_around_min is %d" % least) in msg, msg
                continue
            want_lo, want_hi = rref.rows(c, nb, band, 0)
            assert rc == 0 and np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi), (list(c), nb, band)
            assert lo[0] == 0 and hi[-1] == nb - 1 and np.all(lo[1:] <= hi[:-1] + 1)
            cases += 1
    assert cases > 4000, cases
    lo, hi = llsm.align_around_rows(4, 9, [2, 2, 6, 6], 2)
    assert lo.dtype == np.int32 and list(lo) == [0, 0, 4, 4] and list(hi) == [4, 4, 8, 8]
    # one of them alone, and none: only whether the band is connected
    rc, _, lo, hi = raw_rows(4, 9, [2, 2, 6, 6], 2, 0, hi=False)
    assert rc == 0 and list(lo) == [0, 0, 4, 4] and np.all(hi == -7)
    assert raw_rows(4, 9, [2, 2, 6, 6], 2, 0, lo=False, hi=False)[0] == 0
    assert raw_rows(4, 9, [2, 2, 6, 6], 1, 0, lo=False, hi=False)[0] == -1
    # a band far wider than the matrix: the integers are taken in 64 bits
    lo, hi = llsm.align_around_rows(3, 7, [0, 3, 6], 2 ** 31 - 1)
    assert list(lo) == [0, 0, 0] and list(hi) == [6, 6, 6]


def test_straight_diagonal_gives_the_straight_calls():
    """every pair up to 70 x 70: rows and min around B1's diagonal are those of the two straight bands"""
    L = llsm.load()
    plain = slope = 0
    for na in range(1, 71):
        for nb in range(1, 71):
            c = bref.centers(na, nb)
            least = L.llsm_gpu_align_band_min(na, nb)
            assert raw_min(na, nb, c, 0)[0] == least, (na, nb)
            for band in {least, least + 1, max(na, nb) // 2 + least}:
                rc, _, lo, hi = raw_rows(na, nb, c, band, 0)
                want_lo, want_hi = llsm.align_band_rows(na, nb, band)
                assert rc == 0 and np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi), (na, nb, band)
                plain += 1
            if least > 0:
                assert raw_rows(na, nb, c, least - 1, 0)[0] == -1
            if not sref.admissible(na, nb):
                rc, msg = raw_min(na, nb, c, 1)
                assert rc == -1 and "frames are not admissible" in msg and ("%d x %d" % (na, nb)) in msg, msg
                continue
            least = L.llsm_gpu_align_band_slope_min(na, nb)
            assert raw_min(na, nb, c, 1)[0] == least, (na, nb)
            for band in {least, least + 1, max(na, nb) // 2 + least}:
                rc, _, lo, hi = raw_rows(na, nb, c, band, 1)
                want_lo, want_hi = llsm.align_band_slope_rows(na, nb, band)
                assert rc == 0 and np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi), (na, nb, band)
                slope += 1
            if least > 0:
                assert raw_rows(na, nb, c, least - 1, 1)[0] == -1
    assert plain > 9000 and slope > 4000, (plain, slope)


# ---------------------------------------------------------------- A3: every path of small planes
@pytest.mark.parametrize("slope", [0, 1])
def test_reference_against_brute_force(slope):
    """small integer planes (every sum exact), irregular lines: the reference's cost is the least over all paths"""
    rng = np.random.default_rng(31 + slope)
    done = 0
    while done < 150:
        na, nb = int(rng.integers(1, 7)), int(rng.integers(1, 8))
        if slope and not sref.admissible(na, nb):
            continue
        c = random_line(rng, na, nb)
        band = rref.band_min(c, nb, slope) + int(rng.integers(0, 3))
        D = rng.integers(0, 6, (na, nb)).astype(np.float32)
        step = float(rng.integers(0, 3))
        best, count = rref.brute_force(D, c, band, slope, step)
        pos, cost = rref.dtw(rref.to_band(D, c, band), c, nb, slope, step)
        assert count > 0 and best == cost, (list(c), nb, band, best, cost)
        p, q = rref.band_rows(c, nb, band)
        assert np.all(pos >= np.array(p)) and np.all(pos <= np.array(q)) and np.all(np.diff(pos) >= 0)
        done += 1
    # below the least band there is no path at all
    assert rref.brute_force(np.zeros((4, 9), np.float32), [2, 2, 6, 6], 1, 0, 0.0) == (None, 0)


# ---------------------------------------------------------------- llsm_gpu_align_center_line
def test_center_line():
    # the identity: the same sizes and whole positions
    pos = np.array([0, 0, 1, 3, 3, 4, 7], np.float32)
    assert list(llsm.align_center_line(pos, 8, 7, 8)) == [0, 0, 1, 3, 3, 4, 7]
    # scaling by 4: 6 x 5 coarse frames for 21 x 17 fine ones
    pc = np.array([0, 0.5, 1, 2.5, 3, 4], np.float32)
    c = llsm.align_center_line(pc, 5, 21, 17)
    assert np.array_equal(c, rref.center_line(pc, 5, 21, 17)) and c[0] == 0 and c[-1] == 16 and c[4] == 2 and c[12] == 10
    assert rref.valid(c, 17)
    # positions that go back are made monotone
    c = llsm.align_center_line(np.array([0, 3, 2, 2, 5], np.float32), 6, 5, 6)
    assert list(c) == [0, 3, 3, 3, 5]
    # one coarse row, one fine row, one coarse column
    assert list(llsm.align_center_line(np.array([2], np.float32), 4, 5, 10)) == [6] * 5
    assert list(llsm.align_center_line(np.array([1, 2, 3], np.float32), 4, 1, 10)) == [3]
    assert list(llsm.align_center_line(np.array([0, 0], np.float32), 1, 4, 9)) == [0] * 4
    # seeded: any positions inside the coarse matrix give a valid line, that of the float64 restatement
    rng = np.random.default_rng(5)
    for _ in range(300):
        na_c, nb_c, na, nb = (int(x) for x in rng.integers(1, 60, 4))
        pc = (rng.integers(0, 2 * nb_c - 1, na_c) / 2).astype(np.float32)
        c = llsm.align_center_line(pc, nb_c, na, nb)
        assert c.dtype == np.int32 and np.array_equal(c, rref.center_line(pc, nb_c, na, nb)) and rref.valid(c, nb), (na_c, nb_c, na, nb)


def test_center_line_refusals():
    L = llsm.load()
    pc = np.array([0, 1, 2], np.float32); out = np.full(4, -7, np.int32)

    def call(na_c, nb_c, p, na, nb, c):
        rc = L.llsm_gpu_align_center_line(na_c, nb_c, None if p is None else p.ctypes.data_as(llsm.P_fp), na, nb,
                                          None if c is None else c.ctypes.data_as(llsm.P_int))
        msg = L.llsm_gpu_last_error().decode()
        assert rc == -1 and msg.startswith("llsm_gpu_align_center_line:") and np.all(out == -7), msg
        return msg

    for sizes in ((0, 3, 4, 5), (3, 0, 4, 5), (3, 3, 0, 5), (3, 3, 4, 0), (-1, 3, 4, 5)):
        msg = call(sizes[0], sizes[1], pc, sizes[2], sizes[3], out)
        assert "a size below 1" in msg and ("na_c = %d, nb_c = %d, na = %d, nb = %d" % sizes) in msg, msg
    assert "NULL pos_c or center" in call(3, 3, None, 4, 5, out)
    assert "NULL pos_c or center" in call(3, 3, pc, 4, 5, None)
    msg = call(3, 3, np.array([0, np.nan, 2], np.float32), 4, 5, out)
    assert "pos_c[1]" in msg and "NaN or outside [0, 2]" in msg, msg
    msg = call(3, 3, np.array([0, 1, 2.5], np.float32), 4, 5, out)
    assert "pos_c[2] = 2.5" in msg and "outside [0, 2]" in msg, msg
    msg = call(3, 3, np.array([-0.5, 1, 2], np.float32), 4, 5, out)
    assert "pos_c[0] = -0.5" in msg, msg
    with pytest.raises(llsm.LlsmError):
        llsm.align_center_line(np.array([5], np.float32), 4, 3, 3)


# ---------------------------------------------------------------- the refusals of _around_rows and _around_min
def test_rows_and_min_refusals():
    def both(na, nb, c, slope, needle, band=3):
        rc, msg, lo, hi = raw_rows(na, nb, c, band, slope)
        assert rc == -1 and msg.startswith("llsm_gpu_align_around_rows:") and needle in msg, msg
        assert np.all(lo == -7) and np.all(hi == -7)
        rc, msg = raw_min(na, nb, c, slope)
        assert rc == -1 and msg.startswith("llsm_gpu_align_around_min:") and needle in msg, msg

    for na, nb in ((0, 1), (1, 0), (-3, 4), (4, -3)):
        both(na, nb, [0], 0, "na < 1 or nb < 1 (na = %d, nb = %d)" % (na, nb))
    L = llsm.load()
    assert L.llsm_gpu_align_around_rows(2 ** 28 + 1, 2 ** 28, np.zeros(1, np.int32).ctypes.data_as(llsm.P_int), 3, 1, None, None) == -1
    assert "exceeds 2^28" in L.llsm_gpu_last_error().decode()      # more rows than a call has cells: before the line is read
    assert raw_min(2 ** 28 + 1, 2 ** 28, [0], 1) [0] == -1 and "exceeds 2^28" in raw_min(2 ** 28 + 1, 2 ** 28, [0], 1)[1]
    both(3, 3, [0, 1, 2], 2, "slope = 2 is neither 0 nor 1")
    both(3, 3, [0, 1, 2], -1, "slope = -1 is neither 0 nor 1")
    both(3, 3, None, 0, "NULL center")
    both(2, 4, [0, 3], 1, "2 x 4 frames are not admissible: nb - 1 = 3 exceeds 2 (na - 1) = 2")
    assert raw_min(2, 4, [0, 3], 0)[0] == 1                            # (the plain moves admit every pair)
    both(4, 6, [0, 3, 2, 5], 0, "center[2] = 2 is below center[1] = 3")          # a decreasing line
    both(4, 6, [0, 3, 2, 5], 1, "center[2] = 2 is below center[1] = 3")
    both(4, 6, [0, 1, 2, 6], 0, "center[3] = 6 lies outside [0, 5]")             # a value outside the matrix
    both(4, 6, [-1, 1, 2, 5], 1, "center[0] = -1 lies outside [0, 5]")
    rc, msg, lo, hi = raw_rows(5, 5, [0, 1, 2, 3, 4], -1, 0)
    assert rc == -1 and "band < 0 (na = 5, nb = 5, band = -1)" in msg and np.all(lo == -7)
    # c_0 > band: row 0 does not hold column 0
    for slope in (0, 1):
        rc, msg, lo, hi = raw_rows(6, 8, [3, 3, 4, 5, 6, 7], 2, slope)
        assert rc == -1 and "a band of 2 is not connected" in msg and "6 x 8 frames" in msg and "llsm_gpu_align_around_min is 3" in msg, msg
        assert raw_min(6, 8, [3, 3, 4, 5, 6, 7], slope)[0] == 3
    # a gap above 2 band + 1 between two rows
    rc, msg, lo, hi = raw_rows(6, 12, [0, 1, 2, 8, 10, 11], 2, 0)
    assert rc == -1 and "a band of 2 is not connected around this line on 6 x 12 frames: llsm_gpu_align_around_min is 3" in msg, msg
    assert raw_rows(6, 12, [0, 1, 2, 8, 10, 11], 3, 0)[0] == 0
    # the last row does not reach the last column
    assert raw_min(3, 9, [0, 1, 2], 0)[0] == 6 and raw_rows(3, 9, [0, 1, 2], 5, 0)[0] == -1
    with pytest.raises(llsm.LlsmError):
        llsm.align_around_rows(4, 6, [0, 3, 2, 5], 3)
    with pytest.raises(llsm.LlsmError):
        llsm.align_around_min(2, 4, [0, 3], slope=True)
