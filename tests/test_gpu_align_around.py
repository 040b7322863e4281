"""-m gpu: llsm_gpu_batch_align_around against the numpy restatement of its rules (tests/align_around_reference.py).

The layers of tests/test_gpu_align_band_slope.py, each exact because the rules fix every rounding: the band planes (plane 14)
against rule D1 in float32 inside the rows of the band and +infinity outside, bit for bit; pos and cost against rules A3 in
float32 applied to the device's own plane 14, bit for bit; then the whole chain from LLSM_GPU_CODE -- for the plain moves
(slope = 0) and for the slope pattern (slope = 1).  On top of them: NaN and infinite rows, the straight diagonal against the
two straight banded calls with planes 9 and 13, the band that covers the matrix against the two full calls, invariance of a
pair's bits under everything around it (planes 6, 9, 12 and 13 and every array of both batches untouched), every refusal in
the order of the header, and the coarse-to-fine recipe on a drifting pair.

Batches are those of tests/align_common.py.  The cases (na, nb, band, line) sit below, at and above the 64 rows of a strip of
the path kernels and the 64 x 64 cells of a tile of the distance kernel: 1, 2, 63, 64, 65, 129 and 200 rows; bands 0, 1, 3
and 70 (a strip window wider than a wavefront, tiles that hang over both sides of the matrix); straight lines, lines of
increments 0 / 1 under band 0, a staircase that is flat for 70 rows and then climbs by 2 band + 1 per row, the steepest lines
the slope pattern admits (the two borders of rule L1), and lines that start on column `band` and end on nb - 1 - band, so
that the clamps to both edges of the matrix bind exactly."""
import ctypes as C

import numpy as np
import pytest

import libllsm2_amd as llsm
import align_reference as aref
import align_band_reference as bref
import align_slope_reference as sref
import align_band_slope_reference as kref
import align_around_reference as rref
from align_common import DIM, all_arrays, band_widths, beq, bits, coded, planes_of, random_code, rows_of, same, slices

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- the lines
def straight(na, nb, band):
    return bref.centers(na, nb)


def zero_one(na, nb, band):
    """increments 0 / 1 from column 0 to column nb - 1, no two zeros in a row and a one first: connected under band 0 for
    both patterns (na - 1 <= 2 (nb - 1) - 1)"""
    zeros = na - nb
    assert 0 <= zeros <= nb - 2
    inc = np.ones(na - 1, np.int64)
    inc[1 + 2 * np.arange(zeros)] = 0                               # 1 0 1 0 ... 1 1 1
    inc[1:] = np.roll(inc[1:], (nb - 2 - zeros) // 2 * 2)           # (the zeros in the middle, across the first strip's end)
    return [0] + list(np.cumsum(inc))


def staircase(na, nb, band):
    """flat on column `band` for 70 rows, then 2 band + 1 columns up per row until column nb - 1 - band, flat again"""
    return [min(nb - 1 - band, band + (2 * band + 1) * max(0, i - 69)) for i in range(na)]


def edges(na, nb, band):
    """from column `band` to column nb - 1 - band, rounded half up: p_0 == 0 and q_{na-1} == nb - 1 exactly"""
    return [band + (2 * i * (nb - 1 - 2 * band) + (na - 1)) // (2 * (na - 1)) for i in range(na)]


def upper(na, nb, band):
    return list(sref.rows(na, nb)[1])                               # hi_i of rule L1: two columns per row, then one per two rows


def lower(na, nb, band):
    return list(sref.rows(na, nb)[0])


def wavy(na, nb, band):
    i = np.arange(na)
    c = np.round(i * (nb - 1) / (na - 1) + 12 * np.sin(2 * np.pi * i / (na - 1))).astype(np.int64)
    return list(np.maximum.accumulate(np.clip(c, 0, nb - 1)))


# (na, nb, band, slope, line)
CASES = [(1, 1, 0, 0, straight), (1, 3, 1, 0, lambda na, nb, band: [1]), (2, 3, 1, 0, lambda na, nb, band: [0, 2]),
         (63, 40, 0, 0, zero_one), (64, 64, 0, 0, straight), (65, 100, 1, 0, straight), (65, 37, 1, 0, edges),
         (129, 70, 3, 0, edges), (200, 300, 3, 0, staircase), (200, 150, 70, 0, straight), (129, 100, 70, 0, wavy),
         (200, 390, 70, 0, staircase), (200, 300, 14, 0, wavy),
         (1, 1, 0, 1, straight), (2, 2, 0, 1, straight), (2, 3, 1, 1, lambda na, nb, band: [0, 2]), (64, 64, 0, 1, straight),
         (63, 44, 0, 1, zero_one), (65, 129, 1, 1, upper), (129, 65, 1, 1, lower), (65, 120, 3, 1, lower), (129, 100, 3, 1, edges),
         (200, 150, 70, 1, straight), (129, 100, 70, 1, wavy), (200, 300, 14, 1, wavy), (200, 390, 3, 1, upper)]
NA = [c[0] for c in CASES]
NB = [c[1] for c in CASES]
BAND = [c[2] for c in CASES]
LINE = [[int(x) for x in c[4](c[0], c[1], c[2])] for c in CASES]
IDX = [np.array([k for k, c in enumerate(CASES) if c[3] == s], np.int32) for s in (0, 1)]
OPTS = dict(first=3, count=24, voicing_cost=5.0)
CODE_SEEDS = (1, 2)


def of(values, idx):
    return [values[k] for k in idx]


def test_the_cases_are_what_they_claim():
    """the reference alone: every line is valid and its band connected; the shapes the module head names are there"""
    for (na, nb, band, slope, _), c in zip(CASES, LINE):
        assert len(c) == na and rref.valid(c, nb) and rref.connected(c, nb, band, slope), (na, nb, band, slope)
    assert {(c[2], c[3]) for c in CASES} >= {(b, s) for b in (0, 1, 3, 70) for s in (0, 1)}
    assert {c[0] for c in CASES} >= {1, 2, 63, 64, 65, 129, 200}
    assert all(nb <= 2 * na + 1 and na <= 2 * nb for na, nb in zip(NA, NB))
    c = LINE[8]                                                     # the staircase: flat over a whole strip, then whole bands per row
    assert c[0] == c[69] == 3 and c[71] - c[70] == 7 and c[-1] == 300 - 1 - 3 and rref.band_min(c, 300, 0) == 3
    for k in (6, 7, 21):                                            # the clamps bind at both edges
        assert LINE[k][0] == BAND[k] and LINE[k][-1] == NB[k] - 1 - BAND[k]
    for k in (10, 23):                                              # rows that hang over both sides of the matrix
        assert any(x - 70 < 0 and x + 70 > NB[k] - 1 for x in LINE[k])
    assert all(set(np.diff(LINE[k])) <= {0, 1} for k, c in enumerate(CASES) if c[2] == 0 and c[0] > 1)
    assert rref.band_min(LINE[18], 129, 1) == 1                     # the one path of 65 x 129 passes a cell beside the line in every row


def codes(kind):
    """the rows of batch a and of batch b of a world"""
    integer = kind == "integer"
    ca = random_code(CODE_SEEDS[0], sum(NA), integer); cb = random_code(CODE_SEEDS[1], sum(NB), integer)
    if kind == "nan":
        rng = np.random.default_rng(8)
        oa = np.concatenate([[0], np.cumsum(NA)]); ob = np.concatenate([[0], np.cumsum(NB)])
        ca[oa[2]:oa[3]] = np.nan                                    # every row of 2 x 3, voicing column included
        ca[oa[5] + 20:oa[5] + 23, 3:27] = np.nan                    # a few rows in the middle of 65 x 100
        cb[ob[18] + 70:ob[18] + 72, 3:27] = np.nan                  # ... and of the B side of 65 x 129
        cb[ob[7] + 64, 3:27] = np.inf                               # infinite rows on either side
        ca[oa[19] + 100, 3:27] = -np.inf
        ca[oa[8] + 64, 5] = np.inf; cb[ob[8] + 3, 5] = np.inf        # inf - inf in one cell of 200 x 300
        for p in (9, 10, 12, 22, 23, 24):                           # scattered
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


def run(w, slope, idx=None, lines=None, bands=None, **options):
    """align_around over the cases of `slope` (or those of idx): (pos, cost, the planes of plane 14)"""
    idx = IDX[slope] if idx is None else idx
    lines = of(LINE, idx) if lines is None else lines
    bands = of(BAND, idx) if bands is None else bands
    pos, cost = w["a"].align_around(w["b"], idx, idx, lines, bands, slope=slope, **options)
    return pos, cost, planes_of(w["a"], 14, of(NA, idx), band_widths(bands))


_expected = {}


def expected(kind, step_cost, k):
    """the whole chain of the reference from the rows of a world for case k, computed once: (pos, cost, plane)"""
    key = (kind, step_cost, k)
    if key not in _expected:
        ca, cb = codes(kind)
        _expected[key] = rref.align(slices(ca, NA)[k], slices(cb, NB)[k], LINE[k], BAND[k], CASES[k][3], OPTS["first"], OPTS["count"],
                                    step_cost, OPTS["voicing_cost"])
    return _expected[key]


# ---------------------------------------------------------------- 1: the planes
@pytest.mark.parametrize("slope", [0, 1])
@pytest.mark.parametrize("voicing_cost", [0.0, 5.0])
@pytest.mark.parametrize("first,count", [(0, 5), (3, 32), (3, 37)])
def test_plane_exact(ctx, world, first, count, voicing_cost, slope):
    w = world["random"]
    _, _, got = run(w, slope, first=first, count=count, voicing_cost=voicing_cost)
    infinite = 0
    for n, k in enumerate(IDX[slope]):
        want = rref.dist_band(w["ra"][k], w["rb"][k], LINE[k], BAND[k], first, count, voicing_cost)
        assert beq(got[n], want), (CASES[k][:4], int(np.count_nonzero(bits(got[n]) != bits(want))))
        infinite += int(np.count_nonzero(np.isinf(want)))
    assert infinite > 10000                                         # the overhang of the wide bands


# ---------------------------------------------------------------- 2: the paths
@pytest.mark.parametrize("slope", [0, 1])
@pytest.mark.parametrize("kind", ["random", "integer", "nan"])
@pytest.mark.parametrize("step_cost", [0.0, 1.0])
def test_path_exact(ctx, world, step_cost, kind, slope):
    w = world[kind]
    pos, cost, planes = run(w, slope, step_cost=step_cost, **OPTS)
    assert cost.dtype == np.float32 and cost.shape == (len(IDX[slope]),)
    for n, k in enumerate(IDX[slope]):
        na, nb, band = CASES[k][:3]
        want_pos, want_cost = rref.dtw(planes[n], LINE[k], nb, slope, step_cost)      # on the device's own plane
        assert pos[n].dtype == np.float32 and beq(pos[n], want_pos), (CASES[k][:4], step_cost, np.nonzero(pos[n] != want_pos)[0][:8])
        assert same(cost[n], want_cost), (CASES[k][:4], step_cost, cost[n], want_cost)
        chain = expected(kind, step_cost, k)                        # the whole chain from CODE
        assert beq(pos[n], chain[0]) and same(cost[n], chain[1]) and same(planes[n], chain[2]), (CASES[k][:4], step_cost)
        p, q = rref.band_rows(LINE[k], nb, band)                    # NaN features included: every pos[i] within [p_i, q_i]
        assert not np.any(np.isnan(pos[n])) and np.all(pos[n] >= np.array(p)) and np.all(pos[n] <= np.array(q)), CASES[k][:4]
        assert np.all(np.diff(pos[n]) >= 0) and (na == 1 or pos[n][0] <= 0.5 * q[0]) and pos[n][-1] <= nb - 1
    if kind == "nan":
        assert sum(bool(np.any(np.isnan(P))) for P in planes) >= 4
        assert np.any(np.isnan(cost)) and not np.all(np.isnan(cost))
        clean_pos, clean_cost, _ = run(world["random"], slope, step_cost=step_cost, **OPTS)
        kept = 0
        for n, k in enumerate(IDX[slope]):                          # the pairs without such rows keep their bits
            if beq(w["ra"][k], world["random"]["ra"][k]) and beq(w["rb"][k], world["random"]["rb"][k]):
                assert beq(pos[n], clean_pos[n]) and beq(cost[n], clean_cost[n]), k
                kept += 1
        assert kept >= 4


# ---------------------------------------------------------------- 3: what follows from the rules
@pytest.mark.parametrize("slope", [0, 1])
def test_the_straight_diagonal_is_the_straight_call(ctx, world, slope):
    """center the diagonal of B1: pos, cost and plane 14 are those of align_band with plane 9 / align_band_slope with 13"""
    for kind in ("random", "integer", "nan"):
        w = world[kind]
        idx = IDX[slope]
        lines = [bref.centers(NA[k], NB[k]) for k in idx]
        call = w["a"].align_band_slope if slope else w["a"].align_band
        least = kref.band_min if slope else bref.band_min
        for extra, step_cost in ((0, 0.0), (2, 1.0), (70, 1.0)):
            bands = [least(NA[k], NB[k]) + extra for k in idx]
            pos, cost, planes = run(w, slope, lines=lines, bands=bands, step_cost=step_cost, **OPTS)
            want_pos, want_cost = call(w["b"], idx, idx, bands, step_cost=step_cost, **OPTS)
            want_planes = planes_of(w["a"], 13 if slope else 9, of(NA, idx), band_widths(bands))
            for n, k in enumerate(idx):
                assert beq(pos[n], want_pos[n]) and same(cost[n], want_cost[n]) and same(planes[n], want_planes[n]), (kind, CASES[k][:4], extra)


@pytest.mark.parametrize("slope", [0, 1])
def test_a_band_that_covers_the_matrix_is_the_full_call(ctx, world, slope):
    """band >= nb - 1 under any valid line: pos and cost of align / align_slope; and under the bands of the cases the cost is
    never below theirs"""
    for kind in ("random", "integer", "nan"):
        w = world[kind]
        idx = IDX[slope]
        call = w["a"].align_slope if slope else w["a"].align
        for step_cost in (0.0, 1.0):
            want_pos, want_cost = call(w["b"], idx, idx, step_cost=step_cost, **OPTS)
            bands = [NB[k] - 1 + (k % 3) for k in idx]
            pos, cost, _ = run(w, slope, bands=bands, step_cost=step_cost, **OPTS)
            for n, k in enumerate(idx):
                assert beq(pos[n], want_pos[n]) and same(cost[n], want_cost[n]), (kind, CASES[k][:4], step_cost)
            if kind != "nan":
                narrow = run(w, slope, step_cost=step_cost, **OPTS)[1]
                assert np.all(np.isfinite(narrow)) and np.all(narrow >= want_cost), (kind, step_cost, narrow, want_cost)
                assert np.count_nonzero(narrow > want_cost) >= 4    # (the bands of the cases do narrow the search)


# ---------------------------------------------------------------- 4: invariance
@pytest.mark.parametrize("slope", [0, 1])
def test_a_pair_has_the_bits_it_has_alone(ctx, world, slope):
    w = world["random"]
    a, b = w["a"], w["b"]
    idx = IDX[slope]
    opts = dict(step_cost=1.0, **OPTS)
    # planes 6, 9, 12 and 13 of earlier calls of the other four kinds with a must stay what they are
    a.align(b, [10, 3], [10, 3], **opts); a.align_band(b, [11], [11], 40, **opts); a.align_slope(b, [21, 5], [21, 5], **opts)
    a.align_band_slope(b, [22], [22], 9, **opts)
    held = [a.debug_plane(n) for n in (6, 9, 12, 13)]
    before = all_arrays(a), all_arrays(b)
    pos, cost, planes = run(w, slope, **opts)
    assert all(beq(a.debug_plane(n), h) for n, h in zip((6, 9, 12, 13), held))
    # alone
    for n, k in enumerate(idx):
        p1, c1, pl = run(w, slope, idx=[k], **opts)
        assert beq(p1[0], pos[n]) and beq(c1[0], cost[n]) and beq(pl[0], planes[n]), k
    # the list reversed
    pr, cr, rplanes = run(w, slope, idx=idx[::-1], **opts)
    for n in range(len(idx)):
        m = len(idx) - 1 - n
        assert beq(pr[m], pos[n]) and beq(cr[m], cost[n]) and beq(rplanes[m], planes[n]), n
    # the other pattern and the four other calls in between: one scratch set serves both values of slope, none of theirs
    run(w, 1 - slope, **opts)
    a.align(b, [12, 0], [12, 0], **opts); a.align_band(b, [12], [12], 20, **opts); a.align_slope(b, [21, 13], [21, 13], **opts)
    a.align_band_slope(b, [21], [21], 5, **opts)
    others = [a.debug_plane(n) for n in (6, 9, 12, 13)]
    assert not any(beq(x, y) for x, y in zip(held, others))          # (the other calls did write their own)
    p2, c2, planes2 = run(w, slope, **opts)
    assert all(beq(x, y) for x, y in zip(p2, pos)) and beq(c2, cost) and all(beq(x, y) for x, y in zip(planes2, planes))
    assert all(beq(a.debug_plane(n), h) for n, h in zip((6, 9, 12, 13), others))
    # one utterance in several pairs of one call, each under a line and a band of its own
    k = 24 if slope else 12                                         # 200 x 300 under the wavy line
    at = list(idx).index(k)
    na, nb = NA[k], NB[k]
    lines = [LINE[k], bref.centers(na, nb), LINE[k], [min(nb - 1, x + 5) for x in LINE[k]]]
    bands = [BAND[k], 20, 40, 30]
    pq, cq, plq = run(w, slope, idx=[k] * 4, lines=lines, bands=bands, **opts)
    assert beq(pq[0], pos[at]) and beq(cq[0], cost[at])
    for n in range(4):
        p1, c1, pl = run(w, slope, idx=[k], lines=[lines[n]], bands=[bands[n]], **opts)
        assert beq(pq[n], p1[0]) and beq(cq[n], c1[0]) and beq(plq[n], pl[0]), n
        want = rref.align(w["ra"][k], w["rb"][k], lines[n], bands[n], slope, OPTS["first"], OPTS["count"], 1.0, OPTS["voicing_cost"])
        assert beq(pq[n], want[0]) and beq(cq[n], want[1]), n
    assert len({float(c) for c in cq}) > 1
    # one flat array instead of the list
    pf, cf = a.align_around(b, idx, idx, np.concatenate(of(LINE, idx)).astype(np.int64), of(BAND, idx), slope=bool(slope), **opts)
    assert all(beq(x, y) for x, y in zip(pf, pos)) and beq(cf, cost)
    # one batch on both sides
    both = coded(ctx, NA + NB, np.concatenate([w["ca"], w["cb"]]))
    try:
        kept = all_arrays(both)
        ps, cs = both.align_around(both, idx, idx + len(CASES), of(LINE, idx), of(BAND, idx), slope=slope, **opts)
        assert all(beq(x, y) for x, y in zip(ps, pos)) and beq(cs, cost)
        assert all(beq(x, y) for x, y in zip(planes_of(both, 14, of(NA, idx), band_widths(of(BAND, idx))), planes))
        after = all_arrays(both)
        assert kept.keys() == after.keys() and all(beq(kept[k], after[k]) for k in kept)
    finally:
        both.close()
    # no array of either batch changed
    after = all_arrays(a), all_arrays(b)
    for x, y in zip(before, after):
        assert x.keys() == y.keys() and llsm.A_CODE in x
        assert all(beq(x[k], y[k]) for k in x)


# ---------------------------------------------------------------- 5: refusals
def test_refusals_write_nothing(ctx):
    L = llsm.load()
    a = coded(ctx, [5, 0, 9], random_code(1, 14)); b = coded(ctx, [7, 4], random_code(2, 11))
    plain = coded(ctx, [5], coder=None)                             # layer 1, no coder
    other = coded(ctx, [5], random_code(4, 5)[:, :40], coder=(32, 5))   # 40 columns
    long = coded(ctx, [70000])
    ctx2 = llsm.Context(0)
    far = coded(ctx2, [5], random_code(5, 5))
    pi = lambda v: np.ascontiguousarray(v, np.int32).ctypes.data_as(llsm.P_int)
    held = []
    l57 = [0, 1, 3, 4, 6]; l97 = [0, 1, 2, 2, 3, 4, 5, 5, 6]; l94 = [0, 0, 1, 1, 1, 2, 2, 3, 3]   # lines of 5 x 7, 9 x 7 and 9 x 4
    far_line = list(np.arange(70000))

    def call(x, y, n, ua, ub, center, band, slope=0, pos=True, cost=True, **kw):
        """the raw call with pos and cost pre-filled with a mark: (return code, message, marks untouched)"""
        o = llsm.make_align_options(**kw)
        p = np.full(4 * 70000, -7, np.float32); c = np.full(128, -7, np.float32)
        held[:] = [p, c]
        rc = L.llsm_gpu_batch_align_around(x.h if x else None, y.h if y else None, n, None if ua is None else pi(ua),
                                           None if ub is None else pi(ub), None if center is None else pi(center),
                                           None if band is None else pi(band), slope, C.byref(o),
                                           p.ctypes.data_as(llsm.P_fp) if pos else None, c.ctypes.data_as(llsm.P_fp) if cost else None)
        return rc, L.llsm_gpu_last_error().decode(), bool(np.all(p == -7) and np.all(c == -7))

    def launches():
        return sum(v[1] for v in ctx.profile().values())

    def refused(*args, needle="", **kw):
        n0 = launches()
        rc, msg, clean = call(*args, **kw)
        assert rc == -1 and msg.startswith("llsm_gpu_batch_align_around:") and needle in msg and clean, (args[2:], kw, rc, msg, clean)
        assert launches() == n0                                     # nothing was launched
        with pytest.raises(llsm.LlsmError, match="no llsm_gpu_batch_align_around has run"):
            a.debug_plane(14)                                       # no call has succeeded on a yet

    ctx.set_profiling(True); ctx.reset_profile()
    try:
        a.align(b, [0], [0]); a.align_band(b, [0], [0], 3); a.align_slope(b, [0], [0]); a.align_band_slope(b, [0], [0], 3)
        # 1: everything llsm_gpu_batch_align refuses, in its order
        refused(None, b, 1, [0], [0], l57, [3], needle="NULL batch")
        refused(a, None, 1, [0], [0], l57, [3], needle="NULL batch")
        refused(a, b, -1, [0], [0], l57, [3], needle="n_pairs")
        refused(a, far, 1, [0], [0], l57, [3], needle="context")
        refused(a, plain, 1, [0], [0], l57, [3], needle="coder")
        refused(plain, b, 1, [0], [0], l57, [3], needle="coder")
        refused(a, other, 1, [0], [0], l57, [3], needle="dimension")
        for kw in (dict(first=-1), dict(first=DIM), dict(first=3, count=DIM - 2), dict(first=DIM - 1, count=2)):
            refused(a, b, 1, [0], [0], l57, [3], needle="columns", **kw)
        nan, inf = float("nan"), float("inf")
        for kw in (dict(step_cost=nan), dict(voicing_cost=nan), dict(step_cost=inf), dict(voicing_cost=inf),
                   dict(step_cost=-0.5), dict(voicing_cost=-1e-6), dict(voicing_cost=-inf)):
            refused(a, b, 1, [0], [0], l57, [3], needle="cost", **kw)
        refused(a, b, 1, None, [0], l57, [3], needle="NULL")
        refused(a, b, 1, [0], None, l57, [3], needle="NULL")
        refused(a, b, 1, [0], [0], l57, [3], pos=False, needle="NULL pos")
        refused(a, b, 2, [0, 3], [0, 0], l57 + l57, [3, 3], needle="pair 1: utterance 3 is outside batch a")
        refused(a, b, 2, [0, -1], [0, 0], l57 + l57, [3, 3], needle="outside batch a")
        refused(a, b, 2, [0, 2], [0, 2], l57 + l97, [3, 3], needle="pair 1: utterance 2 is outside batch b")
        refused(a, b, 2, [0, 1], [0, 0], l57 + l57, [3, 3], needle="without frames")
        # ... all of it before the later checks: NULL pos, a pair's utterances and the options come before slope, band and line
        refused(a, b, 1, [0], [0], None, None, slope=2, pos=False, needle="NULL pos")
        refused(a, b, 2, [0, 3], [0, 0], None, None, slope=2, needle="outside batch a")
        refused(a, b, 1, [0], [0], l57, [-1], slope=2, step_cost=nan, needle="cost")
        # 2: slope
        refused(a, b, 1, [0], [0], None, None, slope=2, needle="slope = 2 is neither 0 nor 1")
        refused(a, b, 1, [0], [0], l57, [-1], slope=-1, needle="slope = -1 is neither 0 nor 1")
        # 3: NULL band or center
        refused(a, b, 1, [0], [0], l57, None, needle="NULL band or center")
        refused(a, b, 1, [0], [0], None, [-1], needle="NULL band or center")
        # 4: a negative band, before the shape, the line and the bands of every pair
        refused(a, b, 2, [2, 0], [1, 0], l94 + [9] * 5, [0, -1], slope=1, needle="pair 1: band < 0")
        # 5: 9 x 4: na - 1 = 8 exceeds 2 (nb - 1) = 6, in the words of llsm_gpu_batch_align_slope; with the plain moves it is aligned
        refused(a, b, 3, [0, 2, 2], [0, 1, 0], [9] * 5 + l94 + l97, [0, 3, 3], slope=1,
                needle="pair 1: 9 x 4 frames are not admissible: na - 1 = 8 exceeds 2 (nb - 1) = 6")
        refused(b, a, 1, [1], [2], [0, 2, 5, 8], [9], slope=1, needle="pair 0: 4 x 9 frames are not admissible: nb - 1 = 8 exceeds 2 (na - 1) = 6")
        # 6: a line that is not valid, before any band is looked at
        refused(a, b, 2, [2, 0], [0, 0], l97 + [0, 1, 3, 2, 6], [0, 3], needle="pair 1: center[3] = 2 is below center[2] = 3")
        refused(a, b, 2, [2, 0], [0, 0], l97 + [0, 1, 3, 4, 7], [0, 3], slope=1, needle="pair 1: center[4] = 7 lies outside [0, 6]")
        refused(a, b, 2, [0, 2], [0, 0], [-1, 1, 3, 4, 6] + l97, [0, 0], needle="pair 0: center[0] = -1 lies outside [0, 6]")
        # 7: a band that is not connected: 5 x 7 around 0 1 3 4 6 from a band of 1 on for either pattern, 9 x 7 from 0 on;
        #    c_0 > band; the last row short of the last column
        assert [rref.band_min(l57, 7, s) for s in (0, 1)] == [1, 1] and [rref.band_min(l97, 7, s) for s in (0, 1)] == [0, 0]
        refused(a, b, 2, [2, 0], [0, 0], l97 + l57, [0, 0], needle="pair 1: a band of 0 is not connected for 5 x 7 frames: llsm_gpu_align_around_min is 1")
        refused(a, b, 2, [2, 0], [0, 0], l97 + l57, [0, 0], slope=1,
                needle="pair 1: a band of 0 is not connected for the slope pattern on 5 x 7 frames: llsm_gpu_align_around_min is 1")
        refused(a, b, 1, [0], [0], [2, 2, 3, 4, 6], [1], needle="llsm_gpu_align_around_min is 2")
        refused(a, b, 1, [0], [0], [2, 2, 3, 4, 6], [1], slope=1, needle="llsm_gpu_align_around_min is 2")
        refused(a, b, 1, [0], [0], [0, 1, 2, 3, 3], [2], needle="llsm_gpu_align_around_min is 3")
        # 8: 4 pairs of 70 000 rows under a band of 500: 280 280 000 cells; an unconnected band of a later pair comes first
        refused(long, long, 4, [0] * 4, [0] * 4, far_line * 4, [500] * 4, needle=str(4 * 70000 * 1001))
        refused(long, long, 4, [0] * 4, [0] * 4, far_line * 4, [500] * 4, slope=1, needle="more than 2^28")
        refused(long, long, 2, [0] * 2, [0] * 2, far_line * 2, [2 ** 31 - 1, 5], needle="more than 2^28")
        refused(long, long, 4, [0] * 4, [0] * 4, far_line * 3 + [600] * 601 + far_line[601:], [500] * 4,
                needle="pair 3: a band of 500 is not connected for 70000 x 70000 frames: llsm_gpu_align_around_min is 600")
        # accepted: no pairs (nothing is written or launched, and there is still no plane); then a real call, cost left out
        n0 = launches()
        rc, msg, clean = call(a, b, 0, None, None, None, None, pos=False, cost=False)
        assert rc == 0 and clean and launches() == n0
        with pytest.raises(llsm.LlsmError):
            a.debug_plane(14)
        rc, msg, clean = call(a, b, 2, [2, 0], [0, 0], l97 + l57, [0, 2], slope=1, cost=False)
        assert rc == 0 and np.all(held[1] == -7) and np.all(held[0][:14] != -7) and np.all(held[0][14:] == -7), msg
        assert launches() == n0 + 2
        prof = ctx.profile()
        assert prof["k_align_line_dist"][1] >= 1 and prof["k_align_line_slope_dtw"][1] == 1
        assert a.debug_plane(14).shape == (9 * 1 + 5 * 5,)
        pos, cost = a.align_around(b, [2, 0], [0, 0], [l97, l57], [0, 2], slope=True)
        assert beq(np.concatenate(pos), held[0][:14])
        rc, msg, clean = call(a, b, 1, [0], [0], l57, [1])
        assert rc == 0 and ctx.profile()["k_align_line_dtw"][1] == 1 and a.debug_plane(14).shape == (5 * 3,)
        # a refusal after a success leaves the plane of the success in place
        plane = a.debug_plane(14)
        for args in ((1, [1], [0], l57, [3]), (1, [0], [0], l57, [0]), (1, [0], [0], [0, 1, 3, 2, 6], [3])):
            rc, msg, clean = call(a, b, *args)
            assert rc == -1 and clean and beq(a.debug_plane(14), plane), msg
        with pytest.raises(llsm.LlsmError):
            b.debug_plane(14)                                       # b was only ever the second batch
        with pytest.raises(ValueError):
            a.align_around(b, [0], [0], [l97], 3)                    # the binding counts the columns
    finally:
        ctx.set_profiling(False)
        for x in (a, b, plain, other, long, far):
            x.close()
        ctx2.close()


# ---------------------------------------------------------------- 6: coarse to fine
def drifting_pair():
    """na = 320, nb = 300, eight feature columns that are a random walk; B is A read along x + 0.08 sin(2 pi x) plus noise
    0.05, so that the path leaves the diagonal by 24 frames"""
    rng = np.random.default_rng(11)
    na, nb = 320, 300
    walk = np.cumsum(rng.standard_normal((na, 8)), 0)
    x = np.arange(nb) / (nb - 1)
    t = np.clip(x + 0.08 * np.sin(2 * np.pi * x), 0, 1) * (na - 1)
    k = np.minimum(np.floor(t).astype(int), na - 2)
    B = walk[k] + (walk[k + 1] - walk[k]) * (t - k)[:, None] + 0.05 * rng.standard_normal((nb, 8))
    ca = np.zeros((na, DIM), np.float32); cb = np.zeros((nb, DIM), np.float32)
    ca[:, 3:11] = walk; cb[:, 3:11] = B
    return ca, cb


def test_coarse_to_fine_recipe(ctx):
    ca, cb = drifting_pair()
    na, nb, half, opts = len(ca), len(cb), 10, dict(first=3, count=8, step_cost=0.0, voicing_cost=0.0)
    coarse_a, coarse_b = ca[::4], cb[::4]
    # the numpy references alone: the input must show what the recipe is for, or this test is mis-constructed
    ref_coarse = sref.align(coarse_a, coarse_b, 3, 8)[0]
    ref_line = rref.center_line(ref_coarse, len(coarse_b), na, nb)
    if not (rref.valid(ref_line, nb) and rref.connected(ref_line, nb, half, 1) and kref.connected(na, nb, half)):
        raise RuntimeError("mis-constructed: a band of %d is not connected" % half)
    ref_pos, ref_cost, _ = rref.align(ca, cb, ref_line, half, 1, 3, 8)
    full_pos, full_cost = sref.align(ca, cb, 3, 8)
    straight_cost = kref.align(ca, cb, half, 3, 8)[1]
    print("recipe: around %r, full %r, straight band %r, drift %d" % (ref_cost, full_cost, straight_cost,
                                                                       int(np.max(np.abs(ref_line - np.array(bref.centers(na, nb)))))))
    plain_pos, plain_cost, _ = rref.align(ca, cb, ref_line, half, 0, 3, 8)
    plain_full = aref.align(ca, cb, 3, 8)
    if not (same(ref_cost, full_cost) and beq(ref_pos, full_pos) and straight_cost > full_cost and
            same(plain_cost, plain_full[1]) and beq(plain_pos, plain_full[0])):
        raise RuntimeError("mis-constructed: around %r, full %r, straight band %r; plain moves %r, full %r" %
                           (ref_cost, full_cost, straight_cost, plain_cost, plain_full[1]))
    a = coded(ctx, [na, len(coarse_a)], np.concatenate([ca, coarse_a])); b = coded(ctx, [nb, len(coarse_b)], np.concatenate([cb, coarse_b]))
    try:
        pos_c, _ = a.align_slope(b, [1], [1], **opts)
        assert beq(pos_c[0], ref_coarse)
        line = llsm.align_center_line(pos_c[0], len(coarse_b), na, nb)
        assert np.array_equal(line, ref_line) and llsm.align_around_min(na, nb, line, slope=True) <= half
        pos, cost = a.align_around(b, [0], [0], [line], half, slope=True, **opts)
        assert beq(pos[0], ref_pos) and beq(cost[0], ref_cost)
        dev_full = a.align_slope(b, [0], [0], **opts)
        assert beq(pos[0], dev_full[0][0]) and beq(cost[0], dev_full[1][0])
        band_pos, band_cost = a.align_band_slope(b, [0], [0], half, **opts)
        assert beq(band_cost[0], straight_cost) and band_cost[0] > cost[0]
        # the plain moves through the same band: the path of the full call again
        pos0, cost0 = a.align_around(b, [0], [0], [line], half, **opts)
        assert beq(pos0[0], plain_pos) and beq(cost0[0], plain_cost)
    finally:
        a.close(); b.close()
