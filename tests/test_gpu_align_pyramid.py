"""-m gpu: llsm_gpu_batch_pool_code and llsm_gpu_batch_align_pyramid against the numpy restatement of their rules
(tests/align_pyramid_reference.py) and against the public calls they are made of, bit for bit.

Pooling (rule P1): utterances of 1, 2, 63, 64, 65 and 129 frames at factors 1, 2, 3 and 64 -- n < f, n == f, a tail group of
one frame, three groups at the largest factor --, lists with repeats and out of order, a NaN and a row of -0.0f.
The driver (rules Y1 - Y5): one call over pairs on both sides of the 64 rows of a strip, the pair of one utterance with
itself among them, for factors 2, 4, 16, margins 0, 1, 4 and both patterns, against the chain run by hand through
pool_code, coarse batches of their own, align / align_slope, align_center_line, align_around_min and align_around, and against
the reference chain; coarse pairs of 1 x 1; a margin that covers the matrix against the full calls on features that tie;
a pair alone, among seven and in a reversed list; planes 6, 12 and 14 and every array of both batches untouched; every
refusal with its message and with nothing written or launched.

Not built here: the cap of the fine pass, which is known only after the coarse pass and takes more than 2^28 band cells to
reach.  Its check and its words are those of llsm_gpu_batch_align_around -- one function makes both passes and the five
calls -- and tests/test_gpu_align_around.py reaches them there (refusal 8)."""
import ctypes as C

import numpy as np
import pytest

import libllsm2_amd as llsm
import align_slope_reference as sref
import align_pyramid_reference as yref
from align_common import DIM, all_arrays, beq, coded, random_code, same, slices

pytestmark = pytest.mark.gpu

OPTS = dict(first=3, count=24, step_cost=1.0, voicing_cost=5.0)
REF = (OPTS["first"], OPTS["count"], OPTS["step_cost"], OPTS["voicing_cost"])

# ---------------------------------------------------------------- pooling
POOL_N = [1, 2, 63, 64, 65, 129]
POOL_LISTS = ([0, 1, 2, 3, 4, 5], [5, 0, 3, 3, 1, 5, 2], [4])


def pool_rows():
    code = random_code(21, sum(POOL_N))
    off = np.concatenate([[0], np.cumsum(POOL_N)])
    code[off[4] + 10, 7] = np.nan                                   # one value of one row of the 65
    code[off[5] + 64] = -0.0                                        # a whole row of the 129, the voicing column included
    code[off[2] + 62, 5] = -0.0                                     # the one-frame tail of 63 at factor 2
    return code


@pytest.fixture(scope="module")
def ctx():
    c = llsm.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pool_world(ctx):
    code = pool_rows()
    b = coded(ctx, POOL_N, code)
    yield b, slices(code, POOL_N)
    b.close()


@pytest.mark.parametrize("factor", [1, 2, 3, 64])
def test_pool_exact(pool_world, factor):
    b, rows = pool_world
    before = all_arrays(b)
    for utts in POOL_LISTS:
        got = b.pool_code(utts, factor)
        assert len(got) == len(utts)
        for u, g in zip(utts, got):
            want = yref.pool(rows[u], factor)
            assert g.dtype == np.float32 and g.shape == (llsm.pool_frames(POOL_N[u], factor), DIM) == want.shape
            assert same(g, want), (factor, u, np.argwhere(g != want)[:4])
    whole = b.pool_code(POOL_LISTS[0], factor)
    assert np.isnan(whole[4][10 // factor, 7]) and sum(int(np.count_nonzero(np.isnan(g))) for g in whole) == 1
    k = 64 // factor                                                # the group of the row of -0.0f
    if factor == 1:
        assert not whole[5][k].any() and not np.signbit(whole[5][k]).any() and np.signbit(rows[5][64]).all()
        for g, r in zip(whole, rows):                               # elsewhere factor 1 copies the rows
            keep = ~(np.signbit(r) & (r == 0))
            assert same(g[keep], r[keep])
    if factor == 2:
        assert whole[2].shape[0] == 32 and not np.signbit(whole[2][31, 5])      # (0 + -0) / 1
    after = all_arrays(b)
    assert before.keys() == after.keys() and all(same(before[k], after[k]) for k in before)
    assert b.pool_code([], factor) == []


def test_pool_refusals(ctx):
    L = llsm.load()
    b = coded(ctx, [5, 0, 9], random_code(1, 14))
    plain = coded(ctx, [5], coder=None)
    pi = lambda v: np.ascontiguousarray(v, np.int32).ctypes.data_as(llsm.P_int)

    def launches():
        return sum(v[1] for v in ctx.profile().values())

    def refused(x, factor, n, utts, needle, dst=True):
        out = np.full(16 * DIM, -7, np.float32)
        n0 = launches()
        rc = L.llsm_gpu_batch_pool_code(x.h if x else None, factor, n, None if utts is None else pi(utts),
                                        out.ctypes.data_as(llsm.P_fp) if dst else None)
        msg = L.llsm_gpu_last_error().decode()
        assert rc == -1 and msg.startswith("llsm_gpu_batch_pool_code:") and needle in msg and np.all(out == -7), (rc, msg)
        assert launches() == n0

    ctx.set_profiling(True); ctx.reset_profile()
    try:
        refused(None, 2, 1, [0], "NULL batch")
        refused(plain, 2, 1, [0], "the coder is not enabled")
        for f in (0, -1, 65):
            refused(b, f, 1, [0], "factor = %d lies outside [1, 64]" % f)
        refused(b, 2, -1, [0], "n < 0")
        refused(b, 2, 1, None, "NULL list or dst")
        refused(b, 2, 1, [0], "NULL list or dst", dst=False)
        refused(b, 2, 2, [0, 3], "entry 1: utterance 3 is outside the batch")
        refused(b, 2, 2, [-1, 0], "entry 0: utterance -1 is outside the batch")
        refused(b, 2, 3, [0, 2, 1], "entry 2: an utterance without frames")
        n0 = launches()
        assert L.llsm_gpu_batch_pool_code(b.h, 2, 0, None, None) == 0 and launches() == n0
        assert [g.shape for g in b.pool_code([2, 0], 4)] == [(3, DIM), (2, DIM)]
        assert launches() == n0 + 1 and ctx.profile()["k_pool_code"][1] == 1   # one launch serves the list
        with pytest.raises(llsm.LlsmError, match="llsm_gpu_batch_pool_code: factor = 65"):
            b.pool_code([0], 65)
    finally:
        ctx.set_profiling(False)
        b.close(); plain.close()


# ---------------------------------------------------------------- the driver
NA = [65, 129, 200, 1, 7, 64]
NB = [129, 90, 170, 1, 5, 65]
# one batch on both sides: utterance k against utterance 6 + k, and the 200 frames of utterance 2 against themselves
PAIR_A = [0, 1, 2, 3, 4, 5, 2]
PAIR_B = [6, 7, 8, 9, 10, 11, 2]
SIZES = [(x, y) for x, y in zip(NA, NB)] + [(200, 200)]
FACTORS, MARGINS = (2, 4, 16), (0, 1, 4)


def slope_list(factor):
    """the pairs whose fine and coarse sizes rule L1 admits"""
    return [p for p, (x, y) in enumerate(SIZES)
            if sref.admissible(x, y) and sref.admissible(yref.pool_frames(x, factor), yref.pool_frames(y, factor))]


@pytest.fixture(scope="module")
def world(ctx):
    code = np.concatenate([random_code(1, sum(NA)), random_code(2, sum(NB))])
    both = coded(ctx, NA + NB, code)
    w = dict(both=both, rows=slices(code, NA + NB), code=code, coarse={}, full={})
    yield w
    for x in w["coarse"].values():
        x.close()
    both.close()


def coarse_batch(ctx, w, factor):
    """the pooled vectors of all twelve utterances, by the public call, uploaded to two batches of their own: the sides of the
    coarse pass"""
    if (factor, 0) not in w["coarse"]:
        pooled = w["both"].pool_code(range(len(NA + NB)), factor)
        for side in (0, 1):
            w["coarse"][factor, side] = coded(ctx, [len(x) for x in pooled], np.concatenate(pooled))
    return w["coarse"][factor, 0], w["coarse"][factor, 1]


def by_hand(ctx, w, pairs, factor, margin, slope):
    """the five public calls in turn: (pos, cost, center, band)"""
    both = w["both"]
    small, small_b = coarse_batch(ctx, w, factor)
    ua, ub = [PAIR_A[p] for p in pairs], [PAIR_B[p] for p in pairs]
    pos_c, _ = (small.align_slope if slope else small.align)(small_b, ua, ub, **OPTS)
    lines, bands = [], []
    for n, p in enumerate(pairs):
        na, nb = SIZES[p]
        lines.append(llsm.align_center_line(pos_c[n], llsm.pool_frames(nb, factor), na, nb))
        bands.append(max(min(margin * factor, nb - 1), llsm.align_around_min(na, nb, lines[-1], slope=bool(slope))))
    pos, cost = both.align_around(both, ua, ub, lines, bands, slope=bool(slope), **OPTS)
    return pos, cost, lines, np.array(bands, np.int32)


def pyramid(w, pairs, factor, margin, slope, **kw):
    return w["both"].align_pyramid(w["both"], [PAIR_A[p] for p in pairs], [PAIR_B[p] for p in pairs], factor, margin,
                                   slope=bool(slope), **dict(OPTS, **kw))


def full_call(w, slope):
    """(pos, cost) of align / align_slope on all seven pairs, once"""
    if slope not in w["full"]:
        both = w["both"]
        w["full"][slope] = (both.align_slope if slope else both.align)(both, PAIR_A, PAIR_B, **OPTS)
    return w["full"][slope]


def test_the_pairs_are_what_they_claim():
    assert slope_list(2) == slope_list(4) == slope_list(16) == list(range(7))       # L1 admits every coarse pair here
    assert (yref.pool_frames(65, 16), yref.pool_frames(129, 16)) == (5, 9)          # ... some on its border
    assert not sref.admissible(yref.pool_frames(64, 64), yref.pool_frames(127, 64)) and sref.admissible(64, 127)


@pytest.mark.parametrize("slope", [0, 1])
@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("factor", FACTORS)
def test_composition(ctx, world, factor, margin, slope):
    pairs = slope_list(factor) if slope else list(range(7))
    pos, cost, center, band = pyramid(world, pairs, factor, margin, slope)
    hand = by_hand(ctx, world, pairs, factor, margin, slope)
    assert band.dtype == np.int32 and np.array_equal(band, hand[3]) and beq(cost, hand[1])
    full_pos, full_cost = full_call(world, slope)
    for n, p in enumerate(pairs):
        na, nb = SIZES[p]
        assert center[n].dtype == np.int32 and np.array_equal(center[n], hand[2][n]) and beq(pos[n], hand[0][n]), (p, factor, margin, slope)
        want = yref.align(world["rows"][PAIR_A[p]], world["rows"][PAIR_B[p]], factor, margin, slope, *REF)
        assert beq(pos[n], want[0]) and same(cost[n], want[1]) and np.array_equal(center[n], want[2]) and band[n] == want[3], (p, factor, margin, slope)
        assert band[n] >= min(margin * factor, nb - 1) and band[n] <= nb - 1
        assert np.isfinite(cost[n]) and cost[n] >= full_cost[p], (p, cost[n], full_cost[p])
        if band[n] == nb - 1:                                       # the band covers the matrix: the full call
            assert beq(pos[n], full_pos[p]) and beq(cost[n], full_cost[p]), p
    assert band[3] == 0                                             # 1 x 1


@pytest.mark.parametrize("slope", [0, 1])
def test_degenerate_coarse_pairs(ctx, slope):
    """30 x 40 at factor 64 is 1 x 1 coarse frames: an all-zero line and the band nb - 1; 1 x 17 at factor 4 is one coarse row"""
    a = coded(ctx, [30, 1], random_code(5, 31)); b = coded(ctx, [40, 17], random_code(6, 57))
    try:
        pos, cost, center, band = a.align_pyramid(b, [0], [0], 64, 0, slope=bool(slope), **OPTS)
        want = (a.align_slope if slope else a.align)(b, [0], [0], **OPTS)
        assert not center[0].any() and band[0] == 39 and beq(pos[0], want[0][0]) and beq(cost, want[1])
        if not slope:                                               # (L1 does not admit 1 x 17)
            pos, cost, center, band = a.align_pyramid(b, [1, 0], [1, 0], 4, 1, **OPTS)
            want = a.align(b, [1, 0], [1, 0], **OPTS)
            assert list(center[0]) == [8] and band[0] == 8 and beq(pos[0], want[0][0]) and beq(cost[0], want[1][0])
            assert beq(pos[0], np.array([8], np.float32))
            ref = yref.align(random_code(5, 31)[:30], random_code(6, 57)[:40], 4, 1, 0, *REF)
            assert beq(pos[1], ref[0]) and same(cost[1], ref[1]) and band[1] == ref[3]
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("slope", [0, 1])
def test_a_margin_that_covers_the_matrix_is_the_full_call(ctx, slope):
    """129 x 90 on small integers, where accumulated costs tie often: margin x factor >= nb - 1"""
    a = coded(ctx, [129], random_code(7, 129, integer=True)); b = coded(ctx, [90], random_code(8, 90, integer=True))
    try:
        for step_cost in (0.0, 1.0):
            opts = dict(OPTS, step_cost=step_cost)
            want_pos, want_cost = (a.align_slope if slope else a.align)(b, [0], [0], **opts)
            for factor, margin in ((16, 6), (2, 45), (64, 2), (4, 2 ** 30)):
                assert margin * factor >= 89
                pos, cost, center, band = a.align_pyramid(b, [0], [0], factor, margin, slope=bool(slope), **opts)
                assert band[0] == 89 and beq(pos[0], want_pos[0]) and beq(cost, want_cost), (factor, margin, step_cost)
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("slope", [0, 1])
def test_a_pair_has_the_bits_it_has_alone(world, slope):
    pairs = list(range(7))
    pos, cost, center, band = pyramid(world, pairs, 4, 1, slope)
    for n, p in enumerate(pairs):
        p1, c1, l1, b1 = pyramid(world, [p], 4, 1, slope)
        assert beq(p1[0], pos[n]) and beq(c1[0], cost[n]) and np.array_equal(l1[0], center[n]) and b1[0] == band[n], p
    pr, cr, lr, br = pyramid(world, pairs[::-1], 4, 1, slope)
    for n in range(7):
        assert beq(pr[6 - n], pos[n]) and beq(cr[6 - n], cost[n]) and np.array_equal(lr[6 - n], center[n]) and br[6 - n] == band[n], n
    # one utterance in several pairs of a call; cost, center_out and band_out left out
    pq, cq, lq, bq = pyramid(world, [2, 6, 2], 4, 1, slope)
    assert beq(pq[0], pos[2]) and beq(pq[2], pos[2]) and beq(pq[1], pos[6]) and beq(cq, cost[[2, 6, 2]])
    L = llsm.load()
    o = llsm.make_align_options(**OPTS)
    out = np.full(200, -7, np.float32)
    ua = np.array([2], np.int32); ub = np.array([8], np.int32)
    rc = L.llsm_gpu_batch_align_pyramid(world["both"].h, world["both"].h, 1, ua.ctypes.data_as(llsm.P_int), ub.ctypes.data_as(llsm.P_int), 4, 1, slope,
                                        C.byref(o), out.ctypes.data_as(llsm.P_fp), None, None, None)
    assert rc == 0 and beq(out, pos[2])


def test_nothing_else_changes(ctx):
    """planes 6, 12 and 14 of a, filled by earlier calls, and every array of both batches; no plane leads to the new scratch"""
    a = coded(ctx, [65, 40], random_code(11, 105)); b = coded(ctx, [70, 33], random_code(12, 103))
    try:
        a.align(b, [0, 1], [0, 1], **OPTS); a.align_slope(b, [1], [1], **OPTS)
        a.align_around(b, [1], [1], [llsm.align_center_line(np.arange(40, dtype=np.float32) * 0.8, 33, 40, 33)], 5, **OPTS)
        held = [a.debug_plane(n) for n in (6, 12, 14)]
        before = all_arrays(a), all_arrays(b)
        for slope in (0, 1):
            a.align_pyramid(b, [0, 1, 0], [0, 1, 1], 4, 2, slope=bool(slope), **OPTS)
        assert all(beq(a.debug_plane(n), h) for n, h in zip((6, 12, 14), held))
        for x, y in zip(before, (all_arrays(a), all_arrays(b))):
            assert x.keys() == y.keys() and llsm.A_CODE in x and all(beq(x[k], y[k]) for k in x)
        for which in (9, 13):                                       # the banded calls never ran on a
            with pytest.raises(llsm.LlsmError, match="has run on this batch"):
                a.debug_plane(which)
        for which in (16, 17, -1):
            with pytest.raises(llsm.LlsmError, match="bad arguments"):
                a.debug_plane(which)
    finally:
        a.close(); b.close()


def test_refusals_write_nothing(ctx):
    L = llsm.load()
    a = coded(ctx, [5, 0, 9, 64], random_code(1, 78)); b = coded(ctx, [7, 4, 127], random_code(2, 138))
    plain = coded(ctx, [5], coder=None)
    other = coded(ctx, [5], random_code(4, 5)[:, :40], coder=(32, 5))
    long = coded(ctx, [70000])
    ctx2 = llsm.Context(0)
    far = coded(ctx2, [5], random_code(5, 5))
    pi = lambda v: np.ascontiguousarray(v, np.int32).ctypes.data_as(llsm.P_int)

    def call(x, y, n, ua, ub, factor=2, margin=1, slope=0, pos=True, **kw):
        o = llsm.make_align_options(**kw)
        p = np.full(256, -7, np.float32); c = np.full(8, -7, np.float32)
        line = np.full(256, -7, np.int32); band = np.full(8, -7, np.int32)
        rc = L.llsm_gpu_batch_align_pyramid(x.h if x else None, y.h if y else None, n, None if ua is None else pi(ua),
                                            None if ub is None else pi(ub), factor, margin, slope, C.byref(o),
                                            p.ctypes.data_as(llsm.P_fp) if pos else None, c.ctypes.data_as(llsm.P_fp),
                                            line.ctypes.data_as(llsm.P_int), band.ctypes.data_as(llsm.P_int))
        clean = bool(np.all(p == -7) and np.all(c == -7) and np.all(line == -7) and np.all(band == -7))
        return rc, L.llsm_gpu_last_error().decode(), clean

    def launches():
        return sum(v[1] for v in ctx.profile().values())

    def refused(*args, needle="", **kw):
        n0 = launches()
        rc, msg, clean = call(*args, **kw)
        assert rc == -1 and msg.startswith("llsm_gpu_batch_align_pyramid:") and needle in msg and clean, (args[2:], kw, rc, msg, clean)
        assert launches() == n0                                     # nothing was launched

    ctx.set_profiling(True); ctx.reset_profile()
    try:
        # 1: everything llsm_gpu_batch_align refuses short of its cap, in its order
        refused(None, b, 1, [0], [0], needle="NULL batch")
        refused(a, None, 1, [0], [0], needle="NULL batch")
        refused(a, b, -1, [0], [0], needle="n_pairs")
        refused(a, far, 1, [0], [0], needle="context")
        refused(a, plain, 1, [0], [0], needle="coder")
        refused(plain, b, 1, [0], [0], needle="coder")
        refused(a, other, 1, [0], [0], needle="dimension")
        for kw in (dict(first=-1), dict(first=DIM), dict(first=3, count=DIM - 2)):
            refused(a, b, 1, [0], [0], needle="columns", **kw)
        nan, inf = float("nan"), float("inf")
        for kw in (dict(step_cost=nan), dict(voicing_cost=inf), dict(step_cost=-0.5)):
            refused(a, b, 1, [0], [0], needle="cost", **kw)
        refused(a, b, 1, None, [0], needle="NULL utterance list")
        refused(a, b, 1, [0], None, needle="NULL utterance list")
        refused(a, b, 1, [0], [0], pos=False, needle="NULL pos")
        refused(a, b, 2, [0, 4], [0, 0], needle="pair 1: utterance 4 is outside batch a")
        refused(a, b, 2, [0, 2], [0, 3], needle="pair 1: utterance 3 is outside batch b")
        refused(a, b, 2, [0, 1], [0, 0], needle="pair 1: an utterance without frames")
        # ... all of it before factor, margin and slope
        refused(a, b, 1, [0], [0], factor=1, margin=-1, slope=2, pos=False, needle="NULL pos")
        refused(a, b, 2, [0, 4], [0, 0], factor=1, needle="outside batch a")
        refused(a, b, 1, [0], [0], factor=65, step_cost=nan, needle="cost")
        # 2
        for f in (1, 0, -4, 65):
            refused(a, b, 1, [0], [0], factor=f, needle="factor = %d lies outside [2, 64]" % f)
        refused(a, b, 1, [0], [0], margin=-1, needle="margin < 0")
        refused(a, b, 1, [0], [0], slope=2, needle="slope = 2 is neither 0 nor 1")
        refused(a, b, 1, [0], [0], slope=-1, needle="slope = -1 is neither 0 nor 1")
        # 3: 9 x 4 is not admissible itself; 64 x 127 is, and pools to 1 x 2 at factor 64.  Without the pattern both are aligned
        refused(a, b, 2, [0, 2], [0, 1], slope=1, needle="pair 1: 9 x 4 frames are not admissible: na - 1 = 8 exceeds 2 (nb - 1) = 6")
        refused(a, b, 2, [0, 3], [0, 2], factor=64, slope=1,
                needle="pair 1: 64 x 127 frames pool to 1 x 2 at factor 64, which are not admissible: nb - 1 = 1 exceeds 2 (na - 1) = 0")
        assert call(a, b, 2, [2, 3], [1, 2], factor=64)[0] == 0
        # (the pair is on L1's border, and rounding up costs it at every factor that divides 64: 32 x 64, ..., 2 x 4)
        refused(a, b, 1, [3], [2], factor=32, slope=1, needle="pair 0: 64 x 127 frames pool to 2 x 4 at factor 32")
        assert call(a, b, 1, [3], [2], factor=3, slope=1)[0] == 0   # 22 x 43 coarse frames
        # 4: 70 000 frames pool to 35 000 at factor 2: 1 225 000 000 coarse cells
        refused(long, long, 1, [0], [0], needle="the coarse distance planes hold 1225000000 cells, more than 2^28")
        refused(long, long, 1, [0], [0], slope=1, needle="more than 2^28")
        # accepted: no pairs, whatever the rest; then a real call: one pooling launch for both sides, two passes
        n0 = launches()
        rc, msg, clean = call(a, b, 0, None, None, factor=1, pos=False)
        assert rc == 0 and clean and launches() == n0
        ctx.reset_profile()
        rc, msg, clean = call(a, b, 2, [2, 0], [0, 0], factor=2, margin=1, slope=1)
        prof = ctx.profile()
        assert rc == 0 and not clean and prof["k_pool_code"][1] == 1 and prof["k_align_slope_dtw"][1] == 1 and prof["k_align_line_slope_dtw"][1] == 1, (msg, prof)
        assert prof["k_align_dist"][1] == 1 and prof["k_align_line_dist"][1] == 1 and launches() == 5
        for which in (6, 12, 14):                                   # none of the five calls has run on a: the pyramid has no plane
            with pytest.raises(llsm.LlsmError, match="has run on this batch"):
                a.debug_plane(which)
        with pytest.raises(llsm.LlsmError, match="llsm_gpu_batch_align_pyramid: factor = 1 lies outside"):
            a.align_pyramid(b, [0], [0], 1, 1)
    finally:
        ctx.set_profiling(False)
        for x in (a, b, plain, other, long, far):
            x.close()
        ctx2.close()
