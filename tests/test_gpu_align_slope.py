"""-m gpu: llsm_gpu_batch_align_slope against the numpy restatement of its rules (tests/align_slope_reference.py).

The layers of tests/test_gpu_align.py, each exact because the rules fix every rounding: the distance planes (plane 12)
against rule D1 in float32, bit for bit; pos and cost against rules L3 - L4 in float32 applied to the device's own plane 12,
bit for bit; then the whole chain from LLSM_GPU_CODE.  On top of them: NaN and infinite rows, invariance of a pair's bits
under everything around it (planes 6 and 9 and every array of both batches untouched), the generated pairs of
tests/test_align_slope_host.py against float64 and against llsm_gpu_batch_align's cost, the positions fed to splice, and
every refusal.

Batches are those of tests/align_common.py: layer 1 at nfft 128, the coder at orders 64 + 5, no samples, synthetic
LLSM_GPU_CODE.  The pairs sit below, at and above the 64 rows of a strip of k_align_slope_dtw, at both ends of what rule L1
admits (64 x 127 and 129 x 65: every row a single cell or passed through; 3 x 2: an empty row), and with three to five strips
whose windows move.  test_inputs_cross_the_strips_with_both_moves shows that the paths enter rows 64, 65, 128 and 129 by
move 1 and by move 2: the two hand-over rows are read at both parities."""
import ctypes as C

import numpy as np
import pytest

import libllsm2_amd as llsm
import align_reference as aref
import align_slope_reference as sref
from gpu_common import report
from align_common import COST_REL, DIFFER_CAP, DIM, SEEDS, SLOPE_SIZES as SIZES, all_arrays, beq, bits, coded, planes_of, random_code, \
    rows_of, same, slices, slope_case as host_case, slope_properties as check_properties

pytestmark = pytest.mark.gpu

PAIRS = [(1, 1), (2, 2), (2, 3), (3, 2), (3, 5), (5, 3), (7, 4), (63, 64), (64, 64), (65, 64), (64, 127), (127, 64), (65, 129),
         (129, 65), (130, 200), (200, 390), (257, 300)]
NA = [p[0] for p in PAIRS]
NB = [p[1] for p in PAIRS]
IDENT = np.arange(len(PAIRS), dtype=np.int32)
OPTS = dict(first=3, count=24, voicing_cost=5.0)
CODE_SEEDS = (63, 64)                                               # chosen so that test_inputs_cross_the_strips_with_both_moves holds


def codes(kind):
    """the rows of batch a and of batch b of a world"""
    integer = kind == "integer"
    ca = random_code(CODE_SEEDS[0], sum(NA), integer); cb = random_code(CODE_SEEDS[1], sum(NB), integer)
    if kind == "nan":
        rng = np.random.default_rng(8)
        oa = np.concatenate([[0], np.cumsum(NA)]); ob = np.concatenate([[0], np.cumsum(NB)])
        ca[oa[4]:oa[5]] = np.nan                                    # every row of 3 x 5, voicing column included
        ca[oa[9] + 20:oa[9] + 23, 3:27] = np.nan                    # a few rows in the middle of 65 x 64
        cb[ob[10] + 70:ob[10] + 72, 3:27] = np.nan                  # ... and of the B side of 64 x 127
        cb[ob[12] + 64, 3:27] = np.inf                              # infinite rows on either side
        ca[oa[13] + 100, 3:27] = -np.inf
        ca[oa[14] + 64, 5] = np.inf; cb[ob[14] + 99, 5] = np.inf     # inf - inf in one cell
        for p in (15, 16):                                          # scattered over 200 x 390 and 257 x 300
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


# ---------------------------------------------------------------- 0: what the inputs contain (the reference alone)
def test_inputs_cross_the_strips_with_both_moves():
    entered = set()
    for kind in ("random", "integer"):
        ca, cb = codes(kind)
        for fa, fb in zip(slices(ca, NA), slices(cb, NB)):
            if len(fa) < 65:
                continue
            D = aref.dist(fa, fb, OPTS["first"], OPTS["count"], OPTS["voicing_cost"])
            for step_cost in (0.0, 1.0):
                mv = sref.accumulate(D, step_cost)[1]
                cells, _ = sref.path(mv)
                entered |= {(i, int(mv[i, j])) for i, j in cells if sref.region(*D.shape)[i, j] and (i, j) != (0, 0)}
    for row in (64, 65, 128, 129):
        assert (row, 1) in entered and (row, 2) in entered, (row, sorted(e for e in entered if e[0] == row))


# ---------------------------------------------------------------- 1: the planes
@pytest.mark.parametrize("voicing_cost", [0.0, 5.0])
@pytest.mark.parametrize("first", [0, 3])
@pytest.mark.parametrize("count", [1, 3, 24, 64])
def test_plane_exact(ctx, world, count, first, voicing_cost):
    w = world["random"]
    w["a"].align_slope(w["b"], IDENT, IDENT, first=first, count=count, voicing_cost=voicing_cost)
    got = planes_of(w["a"], 12, NA, NB)
    for p, (fa, fb) in enumerate(zip(w["ra"], w["rb"])):
        want = aref.dist(fa, fb, first, count, voicing_cost)
        assert beq(got[p], want), (PAIRS[p], int(np.count_nonzero(bits(got[p]) != bits(want))))


# ---------------------------------------------------------------- 2: the paths
@pytest.mark.parametrize("kind", ["random", "integer", "nan"])
@pytest.mark.parametrize("step_cost", [0.0, 1.0])
def test_path_exact(ctx, world, step_cost, kind):
    w = world[kind]
    pos, cost = w["a"].align_slope(w["b"], IDENT, IDENT, step_cost=step_cost, **OPTS)
    planes = planes_of(w["a"], 12, NA, NB)
    assert cost.dtype == np.float32 and cost.shape == (len(PAIRS),)
    ties = 0
    for p, D in enumerate(planes):
        want_pos, want_cost = sref.dtw(D, step_cost)                # on the device's own plane
        assert pos[p].dtype == np.float32 and beq(pos[p], want_pos), (PAIRS[p], step_cost, pos[p], want_pos)
        assert same(cost[p], want_cost), (PAIRS[p], step_cost, cost[p], want_cost)
        check_properties(pos[p], *PAIRS[p])
        chain_pos, chain_cost = sref.align(w["ra"][p], w["rb"][p], OPTS["first"], OPTS["count"], step_cost, OPTS["voicing_cost"])
        assert beq(pos[p], chain_pos) and same(cost[p], chain_cost), (PAIRS[p], step_cost)   # the whole chain from CODE
        if kind == "integer":
            acc, mv, inside = sref.accumulate(D, step_cost)
            i, j = np.nonzero(inside[2:, 1:]); i += 2; j += 1
            three = inside[i - 1, j - 1] & inside[i - 2, j - 1]
            q = (acc[i - 2, j - 1] + D[i - 1, j]) + np.float32(step_cost)
            ties += int(np.count_nonzero(three & (q == acc[i - 1, j - 1])))
    if kind == "integer":
        assert ties > 100                                           # move 1 ties with the diagonal often: "<" is exercised
    if kind == "nan":
        assert sum(bool(np.any(np.isnan(D))) for D in planes) >= 6 and sum(bool(np.any(np.isinf(D))) for D in planes) >= 2
        assert np.any(np.isnan(cost)) and not np.all(np.isnan(cost))
        clean_pos, clean_cost = world["random"]["a"].align_slope(world["random"]["b"], IDENT, IDENT, step_cost=step_cost, **OPTS)
        for p in range(len(PAIRS)):                                 # the pairs without such rows keep their bits
            if beq(w["ra"][p], world["random"]["ra"][p]) and beq(w["rb"][p], world["random"]["rb"][p]):
                assert beq(pos[p], clean_pos[p]) and beq(cost[p], clean_cost[p]), p


# ---------------------------------------------------------------- 3: invariance
def test_a_pair_has_the_bits_it_has_alone(ctx, world):
    w = world["random"]
    a, b = w["a"], w["b"]
    opts = dict(step_cost=1.0, **OPTS)
    # planes 6 and 9 of an earlier align / align_band with a must stay what they are
    a.align(b, [14, 3], [14, 3], **opts); a.align_band(b, [15], [15], 40, **opts)
    plane6, plane9 = a.debug_plane(6), a.debug_plane(9)
    before = all_arrays(a), all_arrays(b)
    pos, cost = a.align_slope(b, IDENT, IDENT, **opts)
    planes = planes_of(a, 12, NA, NB)
    # alone
    for p in range(len(PAIRS)):
        p1, c1 = a.align_slope(b, [p], [p], **opts)
        assert beq(p1[0], pos[p]) and beq(c1[0], cost[p]) and beq(planes_of(a, 12, [NA[p]], [NB[p]])[0], planes[p]), p
    # the list reversed
    pr, cr = a.align_slope(b, IDENT[::-1], IDENT[::-1], **opts)
    rplanes = planes_of(a, 12, NA[::-1], NB[::-1])
    for p in range(len(PAIRS)):
        q = len(PAIRS) - 1 - p
        assert beq(pr[q], pos[p]) and beq(cr[q], cost[p]) and beq(rplanes[q], planes[p]), p
    # after unrelated calls of the other two kinds, which have scratch of their own; then a second call
    full_pos, full_cost = a.align(b, [16, 0], [16, 0], **opts)
    a.align_band(b, [12], [12], 70, **opts)
    plane6b, plane9b = a.debug_plane(6), a.debug_plane(9)
    assert all(beq(x, y) for x, y in zip(planes_of(a, 12, NA[::-1], NB[::-1]), rplanes))   # neither wrote plane 12
    p2, c2 = a.align_slope(b, IDENT, IDENT, **opts)
    assert all(beq(x, y) for x, y in zip(p2, pos)) and beq(c2, cost)
    assert all(beq(x, y) for x, y in zip(planes_of(a, 12, NA, NB), planes))
    assert beq(a.debug_plane(6), plane6b) and beq(a.debug_plane(9), plane9b)
    assert cost[16] >= full_cost[0] and cost[0] == full_cost[1]
    # one batch on both sides
    both = coded(ctx, NA + NB, np.concatenate([w["ca"], w["cb"]]))
    try:
        held = all_arrays(both)
        ps, cs = both.align_slope(both, IDENT, IDENT + len(PAIRS), **opts)
        assert all(beq(x, y) for x, y in zip(ps, pos)) and beq(cs, cost)
        assert all(beq(x, y) for x, y in zip(planes_of(both, 12, NA, NB), planes))
        after = all_arrays(both)
        assert held.keys() == after.keys() and all(beq(held[k], after[k]) for k in held)
    finally:
        both.close()
    # one utterance in many pairs: 64 frames of a against every utterance of b that rule L1 admits, three times over
    ub = np.tile(np.array([u for u in IDENT if sref.admissible(64, NB[u])], np.int32), 3)
    ua = np.full(len(ub), 8, np.int32)
    assert len(ub) >= 15
    pq, cq = a.align_slope(b, ua, ub, **opts)
    alone = {u: a.align_slope(b, [8], [u], **opts) for u in set(ub)}
    for k, u in enumerate(ub):
        assert beq(pq[k], alone[u][0][0]) and beq(cq[k], alone[u][1][0]), k
    # no array of either batch changed
    after = all_arrays(a), all_arrays(b)
    for x, y in zip(before, after):
        assert x.keys() == y.keys() and llsm.A_CODE in x
        assert all(beq(x[k], y[k]) for k in x)
    assert not beq(plane6, plane6b) and not beq(plane9, plane9b)    # (the other calls did write their own)


# ---------------------------------------------------------------- 4: the generated pairs, and on to splice
def test_generated_pairs_float64_full_cost_and_splice(ctx):
    """the 48 generated pairs of tests/test_align_slope_host.py as one call: the device against the float64 chain under
    the caps of tests/test_align_host.py, against the float32 reference bit for bit, and its cost against
    llsm_gpu_batch_align's on the device; the positions of one pair go into splice"""
    cases = [(size, seed) for size in SIZES for seed in SEEDS]
    na = [s[0] for s, _ in cases]; nb = [s[1] for s, _ in cases]
    ca = np.zeros((sum(na), DIM), np.float32); cb = np.zeros((sum(nb), DIM), np.float32)
    ia = ib = 0
    for size, seed in cases:
        A, B, _ = aref.make(seed, size[0], size[1], 24, 0.3)
        ca[ia:ia + size[0], 3:27] = A.astype(np.float32); cb[ib:ib + size[1], 3:27] = B.astype(np.float32)
        ia += size[0]; ib += size[1]
    a = coded(ctx, na, ca); b = coded(ctx, nb, cb)
    k = 5                                                           # a pair of 200 x 170
    out = llsm.Batch(ctx, llsm.make_aoptions(f0_refine=0), 44100.0, [0], [na[k]])
    try:
        idx = np.arange(len(cases), dtype=np.int32)
        pos, cost = a.align_slope(b, idx, idx, first=3, count=24, step_cost=1.0)
        full_pos, full_cost = a.align(b, idx, idx, first=3, count=24, step_cost=1.0)
        assert np.all(np.isfinite(cost)) and np.all(cost >= full_cost), (cost, full_cost)
        differ = total = differ32 = 0
        worst = 0.0
        for n, (size, seed) in enumerate(cases):
            (p32, c32), (p64, c64), _, _ = host_case(size, seed)
            differ += int(np.count_nonzero(pos[n] != p64)); differ32 += int(np.count_nonzero(bits(pos[n]) != bits(p32)))
            differ32 += int(not beq(cost[n], c32))
            total += len(p64)
            worst = max(worst, abs(float(cost[n]) - float(c64)) / float(c64))
            check_properties(pos[n], *size)
        rep = dict(frames=total, differ_from_float64=differ, differ_from_float32_reference=differ32, cost_rel=worst,
                   pairs_dearer_than_full=int(np.count_nonzero(cost > full_cost)))
        print(rep)
        report("align_slope_float64", rep)
        assert total == 12 * (200 + 64 + 129 + 300)
        assert differ32 == 0
        assert differ <= DIFFER_CAP * total
        assert worst <= COST_REL
        # the rows of b are zeros apart from LLSM_GPU_CODE: splice only has to take the positions
        for aid, rows in all_arrays(b).items():
            if aid != llsm.A_CODE:
                b.upload(aid, np.zeros_like(rows))
        assert (na[k], nb[k]) == (200, 170)
        utt = np.full(na[k], k, np.int32)
        out.splice(b, pos_a=pos[k], utt_a=utt, utt_b=utt, pos_b=pos[k], mix=np.full(na[k], 0.5, np.float32))
        ctx.sync()
        assert np.all(np.isfinite(out.download(llsm.A_F0)))
    finally:
        a.close(); b.close(); out.close()


# ---------------------------------------------------------------- 5: refusals
def test_refusals_write_nothing(ctx, world):
    L = llsm.load()
    a = coded(ctx, [5, 0, 9], random_code(1, 14)); b = coded(ctx, [7, 4], random_code(2, 11))
    plain = coded(ctx, [5], coder=None)                             # layer 1, no coder
    other = coded(ctx, [5], random_code(4, 5)[:, :40], coder=(32, 5))   # 40 columns
    long = coded(ctx, [2048])
    ctx2 = llsm.Context(0)
    far = coded(ctx2, [5], random_code(5, 5))
    pi = lambda v: np.ascontiguousarray(v, np.int32).ctypes.data_as(llsm.P_int)
    held = []

    def call(x, y, n, ua, ub, pos=True, cost=True, **kw):
        """the raw call with pos and cost pre-filled with a mark: (return code, message, marks untouched)"""
        o = llsm.make_align_options(**kw)
        p = np.full(64 * 2048, -7, np.float32); c = np.full(128, -7, np.float32)
        held[:] = [p, c]
        rc = L.llsm_gpu_batch_align_slope(x.h if x else None, y.h if y else None, n, None if ua is None else pi(ua),
                                          None if ub is None else pi(ub), C.byref(o), p.ctypes.data_as(llsm.P_fp) if pos else None,
                                          c.ctypes.data_as(llsm.P_fp) if cost else None)
        return rc, L.llsm_gpu_last_error().decode(), bool(np.all(p == -7) and np.all(c == -7))

    def launches():
        return sum(v[1] for v in ctx.profile().values())

    def refused(*args, needle="", **kw):
        n0 = launches()
        rc, msg, clean = call(*args, **kw)
        assert rc == -1 and msg.startswith("llsm_gpu_batch_align_slope:") and needle in msg and clean, (args, kw, rc, msg, clean)
        assert launches() == n0                                     # nothing was launched
        with pytest.raises(llsm.LlsmError):
            a.debug_plane(12)                                       # no call has succeeded on a yet

    ctx.set_profiling(True); ctx.reset_profile()
    try:
        a.align(b, [0], [0]); a.align_band(b, [0], [0], 3)          # the other calls do not make a plane 12
        refused(None, b, 1, [0], [0], needle="NULL batch")
        refused(a, None, 1, [0], [0], needle="NULL batch")
        refused(a, b, -1, [0], [0], needle="n_pairs")
        refused(a, b, 1, None, [0], needle="NULL")
        refused(a, b, 1, [0], None, needle="NULL")
        refused(a, b, 1, [0], [0], pos=False, needle="NULL pos")
        refused(a, far, 1, [0], [0], needle="context")
        refused(a, plain, 1, [0], [0], needle="coder")
        refused(plain, b, 1, [0], [0], needle="coder")
        refused(a, other, 1, [0], [0], needle="dimension")
        for kw in (dict(first=-1), dict(first=DIM), dict(first=3, count=DIM - 2), dict(first=DIM - 1, count=2)):
            refused(a, b, 1, [0], [0], needle="columns", **kw)
        nan, inf = float("nan"), float("inf")
        for kw in (dict(step_cost=nan), dict(voicing_cost=nan), dict(step_cost=inf), dict(voicing_cost=inf),
                   dict(step_cost=-0.5), dict(voicing_cost=-1e-6), dict(voicing_cost=-inf)):
            refused(a, b, 1, [0], [0], needle="cost", **kw)
        refused(a, b, 2, [0, 3], [0, 0], needle="outside batch a")
        refused(a, b, 2, [0, -1], [0, 0], needle="outside batch a")
        refused(a, b, 2, [0, 2], [0, 2], needle="outside batch b")
        refused(a, b, 2, [0, 1], [0, 0], needle="without frames")
        refused(long, long, 65, [0] * 65, [0] * 65, needle=str(65 * 2048 * 2048))
        # 9 x 4: na - 1 = 8 exceeds 2 (nb - 1) = 6; 5 x 7 and 9 x 7 are admissible
        refused(a, b, 3, [0, 2, 2], [0, 1, 0], needle="pair 1: 9 x 4 frames are not admissible: na - 1 = 8 exceeds 2 (nb - 1) = 6")
        refused(b, a, 1, [1], [2], needle="pair 0: 4 x 9 frames are not admissible: nb - 1 = 8 exceeds 2 (na - 1) = 6")
        # the checks of llsm_gpu_batch_align come first, in its order: options before the pairs, a pair's utterances before
        # its shape, pair by pair
        refused(a, b, 1, [2], [1], step_cost=nan, needle="cost")
        refused(a, b, 2, [2, 0], [1, 9], needle="pair 0: 9 x 4")
        refused(a, b, 2, [0, 2], [9, 1], needle="pair 0: utterance 9 is outside batch b")
        # accepted: no pairs (nothing is written or launched, and there is still no plane); then a real call, cost left out
        n0 = launches()
        rc, msg, clean = call(a, b, 0, None, None, pos=False, cost=False)
        assert rc == 0 and clean and launches() == n0
        with pytest.raises(llsm.LlsmError):
            a.debug_plane(12)
        rc, msg, clean = call(a, b, 2, [2, 0], [0, 0], cost=False)
        assert rc == 0 and np.all(held[1] == -7) and np.all(held[0][:14] != -7) and np.all(held[0][14:] == -7)
        assert launches() == n0 + 2
        prof = ctx.profile()
        assert prof["k_align_dist"][1] >= 1 and prof["k_align_slope_dtw"][1] == 1
        assert a.debug_plane(12).shape == (9 * 7 + 5 * 7,)
        pos, cost = a.align_slope(b, [2, 0], [0, 0])
        assert beq(np.concatenate(pos), held[0][:14])
        # a refusal after a success leaves the plane of the success in place
        plane = a.debug_plane(12)
        rc, msg, clean = call(a, b, 1, [1], [0])
        assert rc == -1 and clean and beq(a.debug_plane(12), plane)
        rc, msg, clean = call(a, b, 1, [2], [1])
        assert rc == -1 and clean and beq(a.debug_plane(12), plane)
        with pytest.raises(llsm.LlsmError):
            b.debug_plane(12)                                       # b was only ever the second batch
    finally:
        ctx.set_profiling(False)
        for x in (a, b, plain, other, long, far):
            x.close()
        ctx2.close()
