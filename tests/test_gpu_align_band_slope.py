"""-m gpu: llsm_gpu_batch_align_band_slope against the numpy restatement of its rules (tests/align_band_slope_reference.py).

The layers of tests/test_gpu_align.py, each exact because the rules fix every rounding: the band planes (plane 13) against
rule D1 in float32 inside the rows of the band and +infinity outside, bit for bit; pos and cost against rules K3 - K4 in
float32 applied to the device's own plane 13, bit for bit; then the whole chain from LLSM_GPU_CODE.  On top of them: NaN and
infinite rows, the band that covers the matrix against llsm_gpu_batch_align_slope on the device, invariance of a pair's bits
under everything around it (planes 6, 9 and 12 and every array of both batches untouched), one pair of 17 000 x 17 000 that
llsm_gpu_batch_align_slope refuses, the positions fed to splice, and every refusal.

Batches are those of tests/align_common.py: layer 1 at nfft 128, the coder at orders 64 + 5, no samples, synthetic
LLSM_GPU_CODE.  The pairs (na, nb, band) sit below, at and above the 64 rows of a strip of k_align_band_slope_dtw: an empty
row (3 x 2), a single line (64 x 64 under band 0), every row one cell (64 x 127), 64 empty rows (129 x 65), windows of a few
columns whose start moves with the strip, a window wider than a strip (band 70), and the band that covers the matrix.
test_inputs_cross_the_strips_with_both_moves shows that the paths enter rows 64, 65, 128 and 129 by move 1 and by move 2: the
two hand-over rows are read at both parities."""
import ctypes as C

import numpy as np
import pytest

import libllsm2_amd as llsm
import align_band_slope_reference as kref
from align_common import DIM, all_arrays, band_slope_properties as check_properties, band_widths, beq, bits, coded, planes_of, \
    random_code, rows_of, same, slices

pytestmark = pytest.mark.gpu

PAIRS = [(1, 1, 0), (2, 2, 0), (2, 3, 1), (3, 2, 0), (64, 64, 0), (63, 64, 1), (65, 64, 1), (64, 127, 1), (129, 65, 1), (65, 129, 1),
         (130, 200, 3), (200, 390, 2), (257, 300, 8), (300, 257, 70), (257, 300, 299)]
NA = [p[0] for p in PAIRS]
NB = [p[1] for p in PAIRS]
BAND = [p[2] for p in PAIRS]
COVER = 14                                                          # (257, 300, 299): the band covers the matrix
IDENT = np.arange(len(PAIRS), dtype=np.int32)
OPTS = dict(first=3, count=24, voicing_cost=5.0)
CODE_SEEDS = (1, 2)                                                 # chosen so that test_inputs_cross_the_strips_with_both_moves holds


def codes(kind):
    """the rows of batch a and of batch b of a world"""
    integer = kind == "integer"
    ca = random_code(CODE_SEEDS[0], sum(NA), integer); cb = random_code(CODE_SEEDS[1], sum(NB), integer)
    if kind == "nan":
        rng = np.random.default_rng(8)
        oa = np.concatenate([[0], np.cumsum(NA)]); ob = np.concatenate([[0], np.cumsum(NB)])
        ca[oa[2]:oa[3]] = np.nan                                    # every row of 2 x 3, voicing column included
        ca[oa[6] + 20:oa[6] + 23, 3:27] = np.nan                    # a few rows in the middle of 65 x 64
        cb[ob[7] + 70:ob[7] + 72, 3:27] = np.nan                    # ... and of the B side of 64 x 127
        cb[ob[9] + 64, 3:27] = np.inf                               # infinite rows on either side
        ca[oa[8] + 100, 3:27] = -np.inf
        ca[oa[10] + 64, 5] = np.inf; cb[ob[10] + 99, 5] = np.inf     # inf - inf in one cell of 130 x 200
        for p in (11, 12, 13):                                      # scattered over 200 x 390, 257 x 300 and 300 x 257
            ca[oa[p] + rng.integers(0, NA[p], 40), 3 + rng.integers(0, 24, 40)] = np.nan
    return ca, cb


@pytest.fixture(scope="module")
def ctx():
    c = llsm.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def world(ctx):
    out = {}
    for kind in ("random", "integer", "nan"):
        ca, cb = codes(kind)
        a = coded(ctx, NA, ca); b = coded(ctx, NB, cb)
        out[kind] = dict(a=a, b=b, ra=rows_of(a, ca), rb=rows_of(b, cb), ca=ca, cb=cb)
    yield out
    for w in out.values():
        w["a"].close(); w["b"].close()


_expected = {}


def expected(kind, step_cost):
    """the whole chain of the reference from the rows of a world, computed once: per pair (plane, pos, cost, moves)"""
    key = (kind, step_cost)
    if key not in _expected:
        ca, cb = codes(kind)
        out = []
        for (na, nb, band), fa, fb in zip(PAIRS, slices(ca, NA), slices(cb, NB)):
            P = kref.dist_band(fa, fb, band, OPTS["first"], OPTS["count"], OPTS["voicing_cost"])
            acc, mv, lo, hi = kref.accumulate(P, nb, step_cost)
            cells, _ = kref.path(mv, nb)
            out.append((P, kref.positions(cells, na), acc[-1, nb - 1 - (kref.centers(na, nb)[-1] - band)], mv, cells, (lo, hi)))
        _expected[key] = out
    return _expected[key]


# ---------------------------------------------------------------- 0: what the inputs contain (the reference alone)
def test_inputs_cross_the_strips_with_both_moves():
    entered = set()
    for kind in ("random", "integer"):
        for step_cost in (0.0, 1.0):
            for (na, nb, band), (P, _, _, mv, cells, (lo, hi)) in zip(PAIRS, expected(kind, step_cost)):
                off = [c - band for c in kref.centers(na, nb)]
                entered |= {(i, int(mv[i, j - off[i]])) for i, j in cells if lo[i] <= j <= hi[i] and (i, j) != (0, 0)}
    for row in (64, 65, 128, 129):
        assert (row, 1) in entered and (row, 2) in entered, (row, sorted(e for e in entered if e[0] == row))


# ---------------------------------------------------------------- 1: the planes
@pytest.mark.parametrize("voicing_cost", [0.0, 5.0])
@pytest.mark.parametrize("first", [0, 3])
@pytest.mark.parametrize("count", [1, 3, 24, 64])
def test_plane_exact(ctx, world, count, first, voicing_cost):
    w = world["random"]
    w["a"].align_band_slope(w["b"], IDENT, IDENT, BAND, first=first, count=count, voicing_cost=voicing_cost)
    got = planes_of(w["a"], 13, NA, band_widths(BAND))
    infinite = 0
    for p, (fa, fb) in enumerate(zip(w["ra"], w["rb"])):
        want = kref.dist_band(fa, fb, BAND[p], first, count, voicing_cost)     # rule D1 inside the rows of the band, +infinity outside
        assert beq(got[p], want), (PAIRS[p], int(np.count_nonzero(bits(got[p]) != bits(want))))
        infinite += int(np.count_nonzero(np.isinf(want)))
    assert infinite > 10000


# ---------------------------------------------------------------- 2: the paths
@pytest.mark.parametrize("kind", ["random", "integer", "nan"])
@pytest.mark.parametrize("step_cost", [0.0, 1.0])
def test_path_exact(ctx, world, step_cost, kind):
    w = world[kind]
    pos, cost = w["a"].align_band_slope(w["b"], IDENT, IDENT, BAND, step_cost=step_cost, **OPTS)
    planes = planes_of(w["a"], 13, NA, band_widths(BAND))
    assert cost.dtype == np.float32 and cost.shape == (len(PAIRS),)
    ties = 0
    for p, P in enumerate(planes):
        na, nb, band = PAIRS[p]
        want_pos, want_cost = kref.dtw(P, nb, step_cost)            # on the device's own plane
        assert pos[p].dtype == np.float32 and beq(pos[p], want_pos), (PAIRS[p], step_cost, np.nonzero(pos[p] != want_pos)[0][:8])
        assert same(cost[p], want_cost), (PAIRS[p], step_cost, cost[p], want_cost)
        check_properties(pos[p], na, nb, band)
        chain = expected(kind, step_cost)[p]                        # the whole chain from CODE
        assert same(P, chain[0]) and beq(pos[p], chain[1]) and same(cost[p], chain[2]), (PAIRS[p], step_cost)
        if kind == "integer":
            mv = chain[3]
            acc = kref.accumulate(P, nb, step_cost)[0]
            lo, hi = chain[5]
            off = [c - band for c in kref.centers(na, nb)]
            pq = kref.band_rows(na, nb, band)
            for i in range(2, na):
                for j in range(lo[i], hi[i] + 1):
                    if lo[i - 1] <= j - 1 <= hi[i - 1] and lo[i - 2] <= j - 1 <= hi[i - 2] and pq[0][i - 1] <= j <= pq[1][i - 1]:
                        q = (acc[i - 2, j - 1 - off[i - 2]] + P[i - 1, j - off[i - 1]]) + np.float32(step_cost)
                        ties += bool(q == acc[i - 1, j - 1 - off[i - 1]])
    if kind == "integer":
        assert ties > 100                                           # move 1 ties with the diagonal often: "<" is exercised
    if kind == "nan":
        assert sum(bool(np.any(np.isnan(P))) for P in planes) >= 6
        assert np.any(np.isnan(cost)) and not np.all(np.isnan(cost))
        clean_pos, clean_cost = world["random"]["a"].align_band_slope(world["random"]["b"], IDENT, IDENT, BAND, step_cost=step_cost, **OPTS)
        kept = 0
        for p in range(len(PAIRS)):                                 # the pairs without such rows keep their bits
            if beq(w["ra"][p], world["random"]["ra"][p]) and beq(w["rb"][p], world["random"]["rb"][p]):
                assert beq(pos[p], clean_pos[p]) and beq(cost[p], clean_cost[p]), p
                kept += 1
        assert kept >= 4


def test_a_band_that_covers_the_matrix_is_align_slope(ctx, world):
    for kind in ("random", "integer", "nan"):
        w = world[kind]
        for step_cost in (0.0, 1.0):
            pos, cost = w["a"].align_band_slope(w["b"], [COVER, 1, 3], [COVER, 1, 3], [BAND[COVER], 1, 0], step_cost=step_cost, **OPTS)
            want_pos, want_cost = w["a"].align_slope(w["b"], [COVER, 1, 3], [COVER, 1, 3], step_cost=step_cost, **OPTS)
            for k in range(3):
                assert beq(pos[k], want_pos[k]) and same(cost[k], want_cost[k]), (kind, step_cost, k)


# ---------------------------------------------------------------- 3: invariance
def test_a_pair_has_the_bits_it_has_alone(ctx, world):
    w = world["random"]
    a, b = w["a"], w["b"]
    opts = dict(step_cost=1.0, **OPTS)
    # planes 6, 9 and 12 of earlier calls of the other three kinds with a must stay what they are
    a.align(b, [10, 3], [10, 3], **opts); a.align_band(b, [11], [11], 40, **opts); a.align_slope(b, [12, 5], [12, 5], **opts)
    held = a.debug_plane(6), a.debug_plane(9), a.debug_plane(12)
    before = all_arrays(a), all_arrays(b)
    pos, cost = a.align_band_slope(b, IDENT, IDENT, BAND, **opts)
    planes = planes_of(a, 13, NA, band_widths(BAND))
    assert all(beq(a.debug_plane(n), h) for n, h in zip((6, 9, 12), held))
    # alone
    for p in range(len(PAIRS)):
        p1, c1 = a.align_band_slope(b, [p], [p], BAND[p], **opts)
        assert beq(p1[0], pos[p]) and beq(c1[0], cost[p]) and beq(planes_of(a, 13, [NA[p]], band_widths([BAND[p]]))[0], planes[p]), p
    # the list reversed
    pr, cr = a.align_band_slope(b, IDENT[::-1], IDENT[::-1], BAND[::-1], **opts)
    rplanes = planes_of(a, 13, NA[::-1], band_widths(BAND[::-1]))
    for p in range(len(PAIRS)):
        q = len(PAIRS) - 1 - p
        assert beq(pr[q], pos[p]) and beq(cr[q], cost[p]) and beq(rplanes[q], planes[p]), p
    # after unrelated calls of the other three kinds, which have scratch of their own; then a second call
    a.align(b, [12, 0], [12, 0], **opts)
    band_pos, band_cost = a.align_band(b, [12], [12], 8, **opts)
    slope_pos, slope_cost = a.align_slope(b, [12, 13], [12, 13], **opts)
    others = a.debug_plane(6), a.debug_plane(9), a.debug_plane(12)
    assert all(beq(x, y) for x, y in zip(planes_of(a, 13, NA[::-1], band_widths(BAND[::-1])), rplanes))      # none of them wrote plane 13
    p2, c2 = a.align_band_slope(b, IDENT, IDENT, BAND, **opts)
    assert all(beq(x, y) for x, y in zip(p2, pos)) and beq(c2, cost)
    assert all(beq(x, y) for x, y in zip(planes_of(a, 13, NA, band_widths(BAND)), planes))
    assert all(beq(a.debug_plane(n), h) for n, h in zip((6, 9, 12), others))
    assert not any(beq(x, y) for x, y in zip(held, others))          # (the other calls did write their own)
    # one pair several times in a row (equal neighbours share their rows of the region's table), the same shape under
    # another band in between
    rep = [12, 12, 12, 10, 12, 13, 13, 12, 12]
    bands = [BAND[p] for p in rep[:7]] + [299, 8]
    pr, cr = a.align_band_slope(b, rep, rep, bands, **opts)
    wide = a.align_band_slope(b, [12], [12], 299, **opts)
    for k, p in enumerate(rep):
        want = (wide[0][0], wide[1][0]) if bands[k] == 299 else (pos[p], cost[p])
        assert beq(pr[k], want[0]) and beq(cr[k], want[1]), k
    # never below the two rules it narrows, on the device
    assert cost[12] >= band_cost[0] and cost[12] >= slope_cost[0] and cost[13] >= slope_cost[1]
    # one batch on both sides
    both = coded(ctx, NA + NB, np.concatenate([w["ca"], w["cb"]]))
    try:
        kept = all_arrays(both)
        ps, cs = both.align_band_slope(both, IDENT, IDENT + len(PAIRS), BAND, **opts)
        assert all(beq(x, y) for x, y in zip(ps, pos)) and beq(cs, cost)
        assert all(beq(x, y) for x, y in zip(planes_of(both, 13, NA, band_widths(BAND)), planes))
        after = all_arrays(both)
        assert kept.keys() == after.keys() and all(beq(kept[k], after[k]) for k in kept)
    finally:
        both.close()
    # one utterance in many pairs and under many bands: 64 frames of a against every utterance of b that rule L1 admits
    ub = np.tile(np.array([u for u in IDENT if kref.admissible(64, NB[u])], np.int32), 3)
    ua = np.full(len(ub), 4, np.int32)
    bd = np.array([kref.band_min(64, NB[u]) + k % 5 for k, u in enumerate(ub)], np.int32)
    assert len(ub) >= 15
    pq, cq = a.align_band_slope(b, ua, ub, bd, **opts)
    for k, u in enumerate(ub):
        p1, c1 = a.align_band_slope(b, [4], [u], int(bd[k]), **opts)
        assert beq(pq[k], p1[0]) and beq(cq[k], c1[0]), k
    # no array of either batch changed
    after = all_arrays(a), all_arrays(b)
    for x, y in zip(before, after):
        assert x.keys() == y.keys() and llsm.A_CODE in x
        assert all(beq(x[k], y[k]) for k in x)


# ---------------------------------------------------------------- 4: a pair beyond the cap of align_slope, and on to splice
def test_a_long_pair_that_align_slope_refuses(ctx):
    n, band = 17000, 8
    rng = np.random.default_rng(17)
    base = np.cumsum(rng.standard_normal((n, 24)), 0) * 0.3         # a slow walk: neighbouring frames are close
    ca = np.zeros((n, DIM), np.float32); cb = np.zeros((n, DIM), np.float32)
    ca[:, 3:27] = base + 0.1 * rng.standard_normal((n, 24)); cb[:, 3:27] = base + 0.1 * rng.standard_normal((n, 24))
    ca[:, 0] = rng.random(n) < 0.5; cb[:, 0] = rng.random(n) < 0.5
    a = coded(ctx, [n], ca); b = coded(ctx, [n], cb)
    try:
        with pytest.raises(llsm.LlsmError, match="more than 2\\^28"):
            a.align_slope(b, [0], [0], step_cost=1.0, **OPTS)
        pos, cost = a.align_band_slope(b, [0], [0], band, step_cost=1.0, **OPTS)
        P = planes_of(a, 13, [n], band_widths([band]))[0]
        assert P.size == 289000
        want = kref.dist_band(ca, cb, band, OPTS["first"], OPTS["count"], OPTS["voicing_cost"])
        assert beq(P, want)
        want_pos, want_cost = kref.dtw(want, n, 1.0)
        assert beq(pos[0], want_pos) and beq(cost[0], want_cost) and np.isfinite(cost[0])
        check_properties(pos[0], n, n, band)
        assert np.count_nonzero(pos[0] != np.arange(n)) > 1000      # (not the straight diagonal)
    finally:
        a.close(); b.close()


def test_feeds_splice(ctx, world):
    w = world["random"]
    k = 10                                                          # 130 x 200 under band 3
    pos, _ = w["a"].align_band_slope(w["b"], [k], [k], BAND[k], step_cost=1.0, **OPTS)
    b = coded(ctx, NB, w["cb"])
    out = llsm.Batch(ctx, llsm.make_aoptions(f0_refine=0), 44100.0, [0], [NA[k]])
    try:
        # the rows of b are zeros apart from LLSM_GPU_CODE: splice only has to take the positions
        for aid, rows in all_arrays(b).items():
            if aid != llsm.A_CODE:
                b.upload(aid, np.zeros_like(rows))
        utt = np.full(NA[k], k, np.int32)
        out.splice(b, pos_a=pos[0], utt_a=utt, utt_b=utt, pos_b=pos[0], mix=np.full(NA[k], 0.5, np.float32))
        ctx.sync()
        assert np.all(np.isfinite(out.download(llsm.A_F0)))
    finally:
        b.close(); out.close()


# ---------------------------------------------------------------- 5: refusals
def test_refusals_write_nothing(ctx, world):
    L = llsm.load()
    a = coded(ctx, [5, 0, 9], random_code(1, 14)); b = coded(ctx, [7, 4], random_code(2, 11))
    plain = coded(ctx, [5], coder=None)                             # layer 1, no coder
    other = coded(ctx, [5], random_code(4, 5)[:, :40], coder=(32, 5))   # 40 columns
    long = coded(ctx, [70000])
    ctx2 = llsm.Context(0)
    far = coded(ctx2, [5], random_code(5, 5))
    pi = lambda v: np.ascontiguousarray(v, np.int32).ctypes.data_as(llsm.P_int)
    held = []

    def call(x, y, n, ua, ub, band, pos=True, cost=True, **kw):
        """the raw call with pos and cost pre-filled with a mark: (return code, message, marks untouched)"""
        o = llsm.make_align_options(**kw)
        p = np.full(4 * 70000, -7, np.float32); c = np.full(128, -7, np.float32)
        held[:] = [p, c]
        rc = L.llsm_gpu_batch_align_band_slope(x.h if x else None, y.h if y else None, n, None if ua is None else pi(ua),
                                               None if ub is None else pi(ub), None if band is None else pi(band), C.byref(o),
                                               p.ctypes.data_as(llsm.P_fp) if pos else None, c.ctypes.data_as(llsm.P_fp) if cost else None)
        return rc, L.llsm_gpu_last_error().decode(), bool(np.all(p == -7) and np.all(c == -7))

    def launches():
        return sum(v[1] for v in ctx.profile().values())

    def refused(*args, needle="", **kw):
        n0 = launches()
        rc, msg, clean = call(*args, **kw)
        assert rc == -1 and msg.startswith("llsm_gpu_batch_align_band_slope:") and needle in msg and clean, (args, kw, rc, msg, clean)
        assert launches() == n0                                     # nothing was launched
        with pytest.raises(llsm.LlsmError):
            a.debug_plane(13)                                       # no call has succeeded on a yet

    ctx.set_profiling(True); ctx.reset_profile()
    try:
        a.align(b, [0], [0]); a.align_band(b, [0], [0], 3); a.align_slope(b, [0], [0])   # the other calls do not make a plane 13
        refused(None, b, 1, [0], [0], [3], needle="NULL batch")
        refused(a, None, 1, [0], [0], [3], needle="NULL batch")
        refused(a, b, -1, [0], [0], [3], needle="n_pairs")
        refused(a, b, 1, None, [0], [3], needle="NULL")
        refused(a, b, 1, [0], None, [3], needle="NULL")
        refused(a, b, 1, [0], [0], None, needle="NULL band")
        refused(a, b, 1, [0], [0], [3], pos=False, needle="NULL pos")
        refused(a, far, 1, [0], [0], [3], needle="context")
        refused(a, plain, 1, [0], [0], [3], needle="coder")
        refused(plain, b, 1, [0], [0], [3], needle="coder")
        refused(a, other, 1, [0], [0], [3], needle="dimension")
        for kw in (dict(first=-1), dict(first=DIM), dict(first=3, count=DIM - 2), dict(first=DIM - 1, count=2)):
            refused(a, b, 1, [0], [0], [3], needle="columns", **kw)
        nan, inf = float("nan"), float("inf")
        for kw in (dict(step_cost=nan), dict(voicing_cost=nan), dict(step_cost=inf), dict(voicing_cost=inf),
                   dict(step_cost=-0.5), dict(voicing_cost=-1e-6), dict(voicing_cost=-inf)):
            refused(a, b, 1, [0], [0], [3], needle="cost", **kw)
        refused(a, b, 2, [0, 3], [0, 0], [3, 3], needle="outside batch a")
        refused(a, b, 2, [0, -1], [0, 0], [3, 3], needle="outside batch a")
        refused(a, b, 2, [0, 2], [0, 2], [3, 3], needle="outside batch b")
        refused(a, b, 2, [0, 1], [0, 0], [3, 3], needle="without frames")
        refused(a, b, 2, [0, 2], [0, 0], [3, -1], needle="pair 1: band < 0")
        # 9 x 4: na - 1 = 8 exceeds 2 (nb - 1) = 6, in the words of llsm_gpu_batch_align_slope; 5 x 7 and 9 x 7 are admissible
        refused(a, b, 3, [0, 2, 2], [0, 1, 0], [3, 3, 3], needle="pair 1: 9 x 4 frames are not admissible: na - 1 = 8 exceeds 2 (nb - 1) = 6")
        refused(b, a, 1, [1], [2], [9], needle="pair 0: 4 x 9 frames are not admissible: nb - 1 = 8 exceeds 2 (na - 1) = 6")
        # 5 x 7 is connected for the slope pattern from a band of 1 on, 9 x 7 from 0 on
        assert (kref.band_min(5, 7), kref.band_min(9, 7)) == (1, 0)
        refused(a, b, 2, [2, 0], [0, 0], [0, 0], needle="pair 1: a band of 0 is not connected for the slope pattern on 5 x 7 frames: "
                                                         "llsm_gpu_align_band_slope_min is 1")
        # the checks of llsm_gpu_batch_align come first, in its order: options before the pairs, a pair's utterances before
        # its shape and its band, pair by pair
        refused(a, b, 1, [2], [1], [3], step_cost=nan, needle="cost")
        refused(a, b, 2, [2, 0], [1, 9], [3, 3], needle="pair 0: 9 x 4")
        refused(a, b, 2, [0, 2], [9, 1], [0, 3], needle="pair 0: utterance 9 is outside batch b")
        refused(a, b, 2, [0, 2], [0, 1], [-1, 3], needle="pair 0: band < 0")
        # 4 pairs of 70 000 rows under a band of 500: 280 280 000 cells, refused on the host before anything is allocated
        refused(long, long, 4, [0] * 4, [0] * 4, [500] * 4, needle=str(4 * 70000 * 1001))
        refused(long, long, 2, [0] * 2, [0] * 2, [2 ** 31 - 1, 5], needle="more than 2^28")
        # accepted: no pairs (nothing is written or launched, and there is still no plane); then a real call, cost left out
        n0 = launches()
        rc, msg, clean = call(a, b, 0, None, None, None, pos=False, cost=False)
        assert rc == 0 and clean and launches() == n0
        with pytest.raises(llsm.LlsmError):
            a.debug_plane(13)
        rc, msg, clean = call(a, b, 2, [2, 0], [0, 0], [0, 2], cost=False)
        assert rc == 0 and np.all(held[1] == -7) and np.all(held[0][:14] != -7) and np.all(held[0][14:] == -7)
        assert launches() == n0 + 2
        prof = ctx.profile()
        assert prof["k_align_band_dist"][1] >= 1 and prof["k_align_band_slope_dtw"][1] == 1
        assert a.debug_plane(13).shape == (9 * 1 + 5 * 5,)
        pos, cost = a.align_band_slope(b, [2, 0], [0, 0], [0, 2])
        assert beq(np.concatenate(pos), held[0][:14])
        # a refusal after a success leaves the plane of the success in place
        plane = a.debug_plane(13)
        rc, msg, clean = call(a, b, 1, [1], [0], [3])
        assert rc == -1 and clean and beq(a.debug_plane(13), plane)
        rc, msg, clean = call(a, b, 1, [0], [0], [0])
        assert rc == -1 and clean and beq(a.debug_plane(13), plane)
        with pytest.raises(llsm.LlsmError):
            b.debug_plane(13)                                       # b was only ever the second batch
    finally:
        ctx.set_profiling(False)
        for x in (a, b, plain, other, long, far):
            x.close()
        ctx2.close()
