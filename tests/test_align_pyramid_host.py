"""Host side of llsm_gpu_batch_pool_code and llsm_gpu_batch_align_pyramid (no GPU): llsm_gpu_pool_frames against its closed
form and its refusals, the refusals of the two batch calls that need no device, and the numpy restatement of rules P1 and
Y1 - Y5 (tests/align_pyramid_reference.py) on its own: how wide the fine band has to be for the coarse-to-fine chain to give
the path of the full call.

Measured by test_margin_at_which_the_chain_is_the_full_call, in float32, factor 4, SLOPE_SIZES x SEEDS of align_common (48
cases), the share of cases whose (pos, cost) equal the full call's bit for bit at margins 1, 2, 4, 8:
    slope = 1 (llsm_gpu_batch_align_slope):  48, 48, 48, 48 of 48
    slope = 0 (llsm_gpu_batch_align):        47, 48, 48, 48 of 48
so the condition fixed below is margin >= 1 under the slope pattern and margin >= 2 without it: the smallest margins at
which the float32 reference alone reaches every case.  (The band is max(margin x factor, llsm_gpu_align_around_min); on these
cases the first term decides: 4, 8, 16 and 32 columns.)"""
import ctypes as C

import numpy as np
import pytest

import libllsm2_amd as llsm
import align_reference as aref
import align_around_reference as rref
import align_pyramid_reference as yref
from align_common import SEEDS, SLOPE_SIZES, beq, same, slope_case

FACTOR = 4
MARGINS = (1, 2, 4, 8)
LEAST_MARGIN = {1: 1, 0: 2}                                         # slope -> the smallest margin that reaches every case (module head)


# ---------------------------------------------------------------- llsm_gpu_pool_frames
def test_pool_frames_closed_form_and_refusals():
    L = llsm.load()
    for f in (1, 2, 3, 7, 16, 64):
        for n in range(1, 201):
            want = -(-n // f)
            assert L.llsm_gpu_pool_frames(n, f) == want == llsm.pool_frames(n, f) == yref.pool_frames(n, f), (n, f)
            assert (want - 1) * f < n <= want * f                   # every group has a frame, the last may be short
    assert L.llsm_gpu_pool_frames(2 ** 31 - 1, 1) == 2 ** 31 - 1 and L.llsm_gpu_pool_frames(2 ** 31 - 1, 64) == 2 ** 25
    for n, f in ((0, 4), (-1, 4), (5, 0), (5, -2), (5, 65)):
        assert L.llsm_gpu_pool_frames(n, f) == -1
        msg = L.llsm_gpu_last_error().decode()
        assert msg.startswith("llsm_gpu_pool_frames:") and ("nfrm = %d, factor = %d" % (n, f)) in msg, msg
        with pytest.raises(llsm.LlsmError):
            llsm.pool_frames(n, f)


# ---------------------------------------------------------------- P1 in numpy: what the GPU module compares against
def test_pool_reference():
    rng = np.random.default_rng(3)
    code = rng.standard_normal((13, 5)).astype(np.float32)
    for f in (1, 2, 3, 5, 13, 64):
        out = yref.pool(code, f)
        assert out.dtype == np.float32 and out.shape == (yref.pool_frames(13, f), 5)
        assert np.allclose(out, [code[k * f:(k + 1) * f].astype(np.float64).mean(0) for k in range(len(out))], rtol=1e-6, atol=1e-6)
    assert beq(yref.pool(code, 1), code)                            # s = 0 + x; x / 1
    # the order is the rule: 2^24 + 1 + 1 stays 2^24 from the left, and is 2^24 + 2 from the right
    big = np.array([[2 ** 24], [1], [1]], np.float32)
    assert yref.pool(big, 3)[0, 0] == np.float32(2 ** 24) / np.float32(3)
    assert yref.pool(big[::-1], 3)[0, 0] == np.float32(2 ** 24 + 2) / np.float32(3)
    # -0 becomes +0 at factor 1; a NaN stays in its group and its column
    z = yref.pool(np.array([[-0.0, 1.0]], np.float32), 1)
    assert not np.signbit(z[0, 0]) and z[0, 1] == 1
    n = code.copy(); n[4, 2] = np.nan
    out = yref.pool(n, 3)
    assert np.isnan(out[1, 2]) and np.count_nonzero(np.isnan(out)) == 1
    # the voicing column is the voiced share: a majority vote under rule D1's > 0.5f
    v = np.array([[1], [1], [0], [0], [1], [0], [1]], np.float32)
    assert list(yref.pool(v, 3)[:, 0] > np.float32(0.5)) == [True, False, True]


# ---------------------------------------------------------------- the refusals that need no device
def test_refusals_without_a_device():
    L = llsm.load()
    pos = np.full(8, -7, np.float32); cost = np.full(2, -7, np.float32)
    center = np.full(8, -7, np.int32); band = np.full(2, -7, np.int32)
    utt = np.zeros(2, np.int32)
    o = llsm.make_align_options()
    # a NULL batch comes before everything else, a bad factor, margin and slope included
    for factor, margin, slope in ((4, 1, 0), (1, -1, 2), (65, 0, 1)):
        rc = L.llsm_gpu_batch_align_pyramid(None, None, 2, utt.ctypes.data_as(llsm.P_int), utt.ctypes.data_as(llsm.P_int), factor, margin, slope,
                                            C.byref(o), pos.ctypes.data_as(llsm.P_fp), cost.ctypes.data_as(llsm.P_fp),
                                            center.ctypes.data_as(llsm.P_int), band.ctypes.data_as(llsm.P_int))
        msg = L.llsm_gpu_last_error().decode()
        assert rc == -1 and msg == "llsm_gpu_batch_align_pyramid: NULL batch", msg
        assert np.all(pos == -7) and np.all(cost == -7) and np.all(center == -7) and np.all(band == -7)
    dst = np.full(8, -7, np.float32)
    for factor in (4, 0, 65):
        rc = L.llsm_gpu_batch_pool_code(None, factor, 2, utt.ctypes.data_as(llsm.P_int), dst.ctypes.data_as(llsm.P_fp))
        msg = L.llsm_gpu_last_error().decode()
        assert rc == -1 and msg == "llsm_gpu_batch_pool_code: NULL batch" and np.all(dst == -7), msg


# ---------------------------------------------------------------- the reference chain alone
def chain_case(size, seed, slope):
    """for every margin: (pos, cost, band) of rules Y1 - Y5 in float32 on a generated pair; the coarse pass, the line and the
    distances are computed once per pair"""
    na, nb = size
    A, B, _ = aref.make(seed, na, nb, 24, 0.3)
    A = A.astype(np.float32); B = B.astype(np.float32)
    pos_c, _, pb = yref.coarse(A, B, FACTOR, slope, 0, 24, 1.0)
    D = aref.dist(A, B, 0, 24, 0.0)                                 # A2 is D1 cell by cell: the band plane is cut from the full one
    out = {}
    for margin in MARGINS:
        c, band = yref.line_and_band(pos_c, len(pb), na, nb, FACTOR, margin, slope)
        assert rref.valid(c, nb) and rref.connected(c, nb, band, slope)
        out[margin] = rref.dtw(rref.to_band(D, c, band), c, nb, slope, 1.0) + (band,)
    return out


@pytest.mark.parametrize("slope", [1, 0])
def test_margin_at_which_the_chain_is_the_full_call(slope):
    reached = {m: 0 for m in MARGINS}
    cases = 0
    for size in SLOPE_SIZES:
        for seed in SEEDS:
            case = slope_case(size, seed)
            full_pos, full_cost = case[0] if slope else case[3]
            cases += 1
            for margin, (pos, cost, band) in chain_case(size, seed, slope).items():
                assert np.isfinite(cost) and cost >= full_cost, (size, seed, margin, cost, full_cost)   # unconditionally
                assert band >= min(margin * FACTOR, size[1] - 1)
                reached[margin] += bool(beq(pos, full_pos) and same(cost, full_cost))
    print("slope %d, factor %d: margin -> cases whose (pos, cost) are the full call's, of %d: %r" % (slope, FACTOR, cases, reached))
    assert cases == len(SLOPE_SIZES) * len(SEEDS) == 48
    for margin in MARGINS:
        if margin >= LEAST_MARGIN[slope]:
            assert reached[margin] == cases, (slope, margin, reached)


def test_chain_equals_its_parts():
    """align() of the reference module is the steps above with the band plane computed from the rows"""
    A, B, _ = aref.make(5, 64, 65, 24, 0.3)
    A = A.astype(np.float32); B = B.astype(np.float32)
    for slope in (0, 1):
        pos, cost, center, band = yref.align(A, B, FACTOR, 2, slope, 0, 24, 1.0)
        want = chain_case((64, 65), 5, slope)[2]
        assert beq(pos, want[0]) and same(cost, want[1]) and band == want[2] == 8 and len(center) == 64
    # a 1 x 1 coarse pair: an all-zero line, the band that covers the matrix, the full call
    pos, cost, center, band = yref.align(A[:30], B[:40], 64, 0, 0, 0, 24, 1.0)
    full = aref.align(A[:30], B[:40], 0, 24, step_cost=1.0)
    assert not center.any() and band == 39 and beq(pos, full[0]) and same(cost, full[1])
