"""-m gpu: llsm_gpu_batch_align_sub against the numpy restatement of its rules (tests/align_sub_reference.py).

The layers of tests/test_gpu_align.py, each exact because the rules fix every rounding: the distance planes
(llsm_gpu_batch_align_sub_plane) against rule D1 in float32, bit for bit; pos, span, cost and last_row against rules Q3 - Q5
in float32 applied to the device's own planes, bit for bit or both NaN, for both patterns; then the whole chain from
LLSM_GPU_CODE.  On top of them: invariance of a pair's bits under everything around it, a query planted exactly in a longer
utterance, found and cut out again by llsm_gpu_batch_splice, the cost against llsm_gpu_batch_align and
llsm_gpu_batch_align_slope on generated pairs, and every refusal.

Batches are those of tests/align_common.py.  The pairs are every query of 1, 2, 63, 64, 65 and 129 frames against every take
of 1, 2, 64, 65 and 200 frames (under the pattern, those rule Q1 admits): below, at and above the 64 rows of a strip and the
64 stored steps of a block of moves, across the DTW_U = 8 steps loaded ahead, and the matrices of one row and one column."""
import ctypes as C

import numpy as np
import pytest

import libllsm2_amd as llsm
import align_reference as aref
import align_slope_reference as sref
import align_sub_reference as qref
from align_common import DIM, SLOPE_SIZES, all_arrays, beq, bits, coded, random_code, rows_of, same

pytestmark = pytest.mark.gpu

NA = [1, 2, 63, 64, 65, 129]                                        # the utterances of batch a, the queries
NB = [1, 2, 64, 65, 200]                                            # ... and of batch b, the takes
OPTS = dict(first=3, count=24, voicing_cost=5.0)


def pair_list(slope):
    """(utt_a, utt_b) of every admissible pair"""
    pairs = [(ua, ub) for ua, na in enumerate(NA) for ub, nb in enumerate(NB) if qref.admissible(na, nb, slope)]
    assert len(pairs) == (20 if slope else 30)
    return np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32)


def codes(kind):
    integer = kind == "integer"
    ca = random_code(71, sum(NA), integer); cb = random_code(72, sum(NB), integer)
    oa = np.concatenate([[0], np.cumsum(NA)]); ob = np.concatenate([[0], np.cumsum(NB)])
    if integer:                                                     # the takes of 200 and 64 say everything twice: two ends of least acc
        cb[ob[4] + 100:ob[4] + 200] = cb[ob[4]:ob[4] + 100]; cb[ob[2] + 32:ob[2] + 64] = cb[ob[2]:ob[2] + 32]
    if kind == "nan":
        ca[oa[1]:oa[2]] = np.nan                                    # every row of the query of 2 frames, voicing column included
        ca[oa[4] + 20:oa[4] + 23, 3:27] = np.nan                    # a few rows in the middle of the query of 65
        cb[ob[2] + 30:ob[2] + 32, 3:27] = np.nan                    # ... and of the take of 64
        cb[ob[4] + 150, 3:27] = np.inf                              # an infinite frame of the take of 200
        ca[oa[5] + 100, 5] = np.inf; cb[ob[3] + 40, 5] = np.inf      # inf - inf in one cell of 129 x 65
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


def equal_results(x, y):
    """two results of align_sub with last_row: pos, span, cost and rows bit for bit or both NaN"""
    return (len(x[0]) == len(y[0]) and all(beq(p, q) for p, q in zip(x[0], y[0])) and np.array_equal(x[1], y[1]) and same(x[2], y[2])
            and all(same(p, q) for p, q in zip(x[3], y[3])))


def pick(res, k):
    return [res[0][k]], res[1][k:k + 1], res[2][k:k + 1], [res[3][k]]


# ---------------------------------------------------------------- 1: the planes
@pytest.mark.parametrize("count", [3, 64])
def test_plane_exact(ctx, world, count):
    w = world["random"]
    ua, ub = pair_list(False)
    w["a"].align_sub(w["b"], ua, ub, first=3, count=count, voicing_cost=5.0)
    got = w["a"].align_sub_planes()
    assert len(got) == len(ua)
    for p, (u, v) in enumerate(zip(ua, ub)):
        want = aref.dist(w["ra"][u], w["rb"][v], 3, count, 5.0)
        assert got[p].shape == (NA[u], NB[v]) and beq(got[p], want), (NA[u], NB[v], int(np.count_nonzero(bits(got[p]) != bits(want))))


# ---------------------------------------------------------------- 2: the paths
@pytest.mark.parametrize("kind", ["random", "integer", "nan"])
@pytest.mark.parametrize("step_cost", [0.0, 1.0])
@pytest.mark.parametrize("slope", [False, True], ids=["plain", "slope"])
def test_path_exact(ctx, world, slope, step_cost, kind):
    w = world[kind]
    ua, ub = pair_list(slope)
    pos, span, cost, last = w["a"].align_sub(w["b"], ua, ub, slope=slope, last_row=True, step_cost=step_cost, **OPTS)
    planes = w["a"].align_sub_planes()
    assert cost.dtype == np.float32 and cost.shape == (len(ua),) and span.dtype == np.int32 and span.shape == (len(ua), 2)
    ties = 0
    for p, D in enumerate(planes):
        na, nb = NA[ua[p]], NB[ub[p]]
        want_pos, want_span, want_cost, want_last = qref.dtw(D, step_cost, slope)          # on the device's own plane
        where = (na, nb, slope, step_cost, kind)
        assert pos[p].dtype == np.float32 and beq(pos[p], want_pos), (where, pos[p], want_pos)
        assert tuple(span[p]) == want_span, (where, span[p], want_span)
        assert same(cost[p], want_cost), (where, cost[p], want_cost)
        assert last[p].shape == (nb,) and same(last[p], want_last), where
        chain = qref.align(w["ra"][ua[p]], w["rb"][ub[p]], OPTS["first"], OPTS["count"], step_cost, OPTS["voicing_cost"], slope)
        assert beq(pos[p], chain[0]) and tuple(span[p]) == chain[1] and same(cost[p], chain[2]) and same(last[p], chain[3]), where
        # what llsm_gpu.h states of the outputs
        begin, end = span[p]
        assert 0 <= begin <= end <= nb - 1 and pos[p][0] == begin and np.all(pos[p] >= begin) and np.all(pos[p] <= end)
        assert not np.any(np.isnan(pos[p])) and np.all(np.diff(pos[p]) >= 0)
        if slope:
            assert pos[p][-1] in (end, end - 0.5) and np.all(np.diff(pos[p]) <= 2) and np.all(pos[p][2:] - pos[p][:-2] >= 1)
            assert np.all(np.isposinf(last[p][:na // 2])) and not np.isposinf(last[p][na // 2]) or kind == "nan"
        elif kind != "nan":
            assert pos[p][-1] == end
        if kind == "integer":
            ties += int(np.count_nonzero(last[p] == cost[p])) - 1
    if kind == "integer":
        assert ties >= 3                                            # several columns of least acc: the smallest is the end
    if kind == "nan":
        assert sum(bool(np.any(np.isnan(D))) for D in planes) >= 8 and sum(bool(np.any(np.isinf(D))) for D in planes) >= 3
        assert np.any(np.isnan(cost)) and not np.all(np.isnan(cost))


# ---------------------------------------------------------------- 3: invariance
@pytest.mark.parametrize("slope", [False, True], ids=["plain", "slope"])
def test_a_pair_has_the_bits_it_has_alone(ctx, world, slope):
    w = world["random"]
    a, b = w["a"], w["b"]
    ua, ub = pair_list(slope)
    opts = dict(slope=slope, last_row=True, step_cost=1.0, **OPTS)
    res = a.align_sub(b, ua, ub, **opts)
    planes = a.align_sub_planes()
    for k in range(len(ua)):                                        # alone
        one = a.align_sub(b, ua[k:k + 1], ub[k:k + 1], **opts)
        assert equal_results(one, pick(res, k)) and beq(a.align_sub_planes()[0], planes[k]), k
    rev = a.align_sub(b, ua[::-1], ub[::-1], **opts)                # the list reversed
    rplanes = a.align_sub_planes()
    for k in range(len(ua)):
        q = len(ua) - 1 - k
        assert equal_results(pick(rev, q), pick(res, k)) and beq(rplanes[q], planes[k]), k
    both = coded(ctx, NA + NB, np.concatenate([w["ca"], w["cb"]]))  # one batch on both sides
    try:
        held = all_arrays(both)
        one = both.align_sub(both, ua, ub + len(NA), **opts)
        assert equal_results(one, res) and all(beq(x, y) for x, y in zip(both.align_sub_planes(), planes))
        after = all_arrays(both)
        assert held.keys() == after.keys() and all(beq(held[k], after[k]) for k in held)
    finally:
        both.close()
    # one query in many pairs, three times over
    many = a.align_sub(b, np.tile(ua, 3), np.tile(ub, 3), **opts)
    for k in range(3 * len(ua)):
        assert equal_results(pick(many, k), pick(res, k % len(ua))), k
    # without the optional outputs the others are the same
    L = llsm.load()
    o = llsm.make_align_options(step_cost=1.0, **OPTS)
    flat = np.full(int(sum(NA[u] for u in ua)), -7, np.float32)
    rc = L.llsm_gpu_batch_align_sub(a.h, b.h, len(ua), ua.ctypes.data_as(llsm.P_int), ub.ctypes.data_as(llsm.P_int), int(slope),
                                    C.byref(o), flat.ctypes.data_as(llsm.P_fp), None, None, None)
    assert rc == 0 and beq(flat, np.concatenate(res[0]))


# ---------------------------------------------------------------- 4: find a query, and cut it out
@pytest.mark.parametrize("slope", [False, True], ids=["plain", "slope"])
def test_find_and_cut(ctx, slope):
    nb = [200, 300, 129]
    plants = [(0, 0, 63), (0, 137, 63), (1, 70, 129), (1, 5, 64), (2, 0, 129), (1, 235, 65), (0, 100, 1), (1, 7, 2)]   # (take, n0, na)
    cb = random_code(91, sum(nb))
    ob = np.concatenate([[0], np.cumsum(nb)])
    ca = np.concatenate([cb[ob[u] + n0:ob[u] + n0 + na] for u, n0, na in plants])
    na = [p[2] for p in plants]
    a = coded(ctx, na, ca); b = coded(ctx, nb, cb)
    out = llsm.Batch(ctx, llsm.make_aoptions(f0_refine=0), 44100.0, [0] * len(na), na)
    try:
        rng = np.random.default_rng(92)
        rows = {llsm.A_F0: rng.uniform(80, 300, b.shape(llsm.A_F0)), llsm.A_RD: rng.uniform(0.5, 2.5, b.shape(llsm.A_RD)),
                llsm.A_VTMAGN: rng.uniform(-100, 0, b.shape(llsm.A_VTMAGN))}
        rows = {aid: r.astype(np.float32) for aid, r in rows.items()}
        for aid, r in rows.items():
            b.upload(aid, r)
        ua = np.arange(len(plants), dtype=np.int32); ub = np.array([p[0] for p in plants], np.int32)
        for step_cost in (0.0, 1.0):
            pos, span, cost, last = a.align_sub(b, ua, ub, slope=slope, last_row=True, step_cost=step_cost, **OPTS)
            for k, (u, n0, n) in enumerate(plants):
                assert tuple(span[k]) == (n0, n0 + n - 1) and cost[k] == 0, (k, span[k], cost[k])
                assert beq(pos[k], np.arange(n0, n0 + n, dtype=np.float32)), (k, pos[k])
                assert last[k][n0 + n - 1] == 0 and np.count_nonzero(last[k] == 0) == 1     # the matching function dips to 0 once
        # the positions and utt_b, unchanged, into splice: the query's frames of the take come back
        out.splice(b, pos_a=np.concatenate(pos), utt_a=np.repeat(ub, na))
        ctx.sync()
        for aid, r in rows.items():
            got = out.download(aid)
            want = np.concatenate([r[ob[u] + n0:ob[u] + n0 + n] for u, n0, n in plants])
            assert beq(got, want), aid
    finally:
        a.close(); b.close(); out.close()


# ---------------------------------------------------------------- 5: the cost against the calls with fixed ends
def test_cost_is_never_above_the_calls_with_fixed_ends(ctx):
    """generated pairs as one call each: renditions of align_reference.make, which llsm_gpu_batch_align_slope admits, and
    queries planted in takes (tests/test_align_sub_host.py), where the device also gives the bits of the float32 reference
    and finds the ends"""
    cases = [(size, seed, 0, 0) for size in SLOPE_SIZES for seed in (0, 1, 2)] + \
            [((na, nm), seed, n0, n1) for na, nm, n0, n1 in ((64, 65, 40, 70), (129, 100, 64, 1), (150, 200, 300, 250)) for seed in (0, 1)]
    made = [qref.plant(seed, size[0], size[1], n0, n1) if n0 + n1 else aref.make(seed, size[0], size[1], 24, 0.3) for size, seed, n0, n1 in cases]
    na = [len(m[0]) for m in made]; nb = [len(m[1]) for m in made]
    ca = np.zeros((sum(na), DIM), np.float32); cb = np.zeros((sum(nb), DIM), np.float32)
    ca[:, 3:27] = np.concatenate([m[0] for m in made]).astype(np.float32)
    cb[:, 3:27] = np.concatenate([m[1] for m in made]).astype(np.float32)
    a = coded(ctx, na, ca); b = coded(ctx, nb, cb)
    try:
        idx = np.arange(len(cases), dtype=np.int32)
        opts = dict(first=3, count=24, step_cost=1.0)
        full = a.align(b, idx, idx, **opts)[1]
        fits = np.array([k for k in idx if sref.admissible(na[k], nb[k])], np.int32)
        assert len(fits) == 14                                      # the renditions, and 129 x 165 of the planted pairs
        under = a.align_slope(b, fits, fits, **opts)[1]
        pos0, span0, cost0 = a.align_sub(b, idx, idx, **opts)
        pos1, span1, cost1 = a.align_sub(b, idx, idx, slope=True, **opts)
        assert np.all(np.isfinite(cost0)) and np.all(cost0 <= full), (cost0, full)
        assert np.all(np.isfinite(cost1)) and np.all(cost1[fits] <= under), (cost1[fits], under)
        for k, (size, seed, n0, n1) in enumerate(cases):
            if n0 + n1 == 0:
                continue
            A = made[k][0].astype(np.float32); B = made[k][1].astype(np.float32)
            for slope, pos, span, cost in ((False, pos0, span0, cost0), (True, pos1, span1, cost1)):
                want = qref.align(A, B, 0, 24, step_cost=1.0, slope=slope)
                assert beq(pos[k], want[0]) and tuple(span[k]) == want[1] and beq(cost[k], want[2]), (cases[k], slope)
                assert abs(span[k][0] - n0) <= 2 and abs(span[k][1] - (n0 + size[1] - 1)) <= 2, (cases[k], slope, span[k])
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------- 6: refusals, and what an accepted call leaves alone
def test_refusals_write_nothing(ctx):
    L = llsm.load()
    a = coded(ctx, [5, 0, 9], random_code(1, 14)); b = coded(ctx, [7, 4], random_code(2, 11))
    plain = coded(ctx, [5], coder=None)                             # layer 1, no coder
    other = coded(ctx, [5], random_code(4, 5)[:, :40], coder=(32, 5))   # 40 columns
    long = coded(ctx, [2048])
    ctx2 = llsm.Context(0)
    far = coded(ctx2, [5], random_code(5, 5))
    pi = lambda v: np.ascontiguousarray(v, np.int32).ctypes.data_as(llsm.P_int)
    held = []

    def call(x, y, n, ua, ub, slope=0, pos=True, span=True, cost=True, last=True, **kw):
        """the raw call with the four outputs pre-filled with a mark: (return code, message, marks untouched)"""
        o = llsm.make_align_options(**kw)
        p = np.full(64 * 2048, -7, np.float32); s = np.full(256, -7, np.int32); c = np.full(128, -7, np.float32)
        r = np.full(64 * 2048, -7, np.float32)
        held[:] = [p, s, c, r]
        rc = L.llsm_gpu_batch_align_sub(x.h if x else None, y.h if y else None, n, None if ua is None else pi(ua),
                                        None if ub is None else pi(ub), slope, C.byref(o), p.ctypes.data_as(llsm.P_fp) if pos else None,
                                        s.ctypes.data_as(llsm.P_int) if span else None, c.ctypes.data_as(llsm.P_fp) if cost else None,
                                        r.ctypes.data_as(llsm.P_fp) if last else None)
        return rc, L.llsm_gpu_last_error().decode(), bool(np.all(p == -7) and np.all(s == -7) and np.all(c == -7) and np.all(r == -7))

    def launches():
        return sum(v[1] for v in ctx.profile().values())

    def no_plane(x):
        assert L.llsm_gpu_batch_align_sub_plane(x.h, None, 0) == -1
        assert L.llsm_gpu_last_error().decode().startswith("llsm_gpu_batch_align_sub_plane:")
        with pytest.raises(llsm.LlsmError):
            x.align_sub_planes()

    def refused(*args, needle="", **kw):
        n0 = launches()
        rc, msg, clean = call(*args, **kw)
        assert rc == -1 and msg.startswith("llsm_gpu_batch_align_sub:") and needle in msg and clean, (args, kw, rc, msg, clean)
        assert launches() == n0                                     # nothing was launched
        no_plane(a)                                                 # no call has succeeded on a yet

    ctx.set_profiling(True); ctx.reset_profile()
    try:
        # the other calls make no such planes; theirs are held below
        a.align(b, [0], [0]); a.align_band(b, [2], [0], 3); a.align_slope(b, [0, 2], [0, 0]); a.align_band_slope(b, [2], [0], 3)
        a.align_around(b, [0], [1], [np.array([0, 1, 2, 3, 3])], 2)
        planes = {which: a.debug_plane(which) for which in (6, 9, 12, 13, 14)}
        before = all_arrays(a), all_arrays(b)
        for slope in (0, 1):
            refused(None, b, 1, [0], [0], slope, needle="NULL batch")
            refused(a, None, 1, [0], [0], slope, needle="NULL batch")
            refused(a, b, -1, [0], [0], slope, needle="n_pairs")
            refused(a, b, 1, None, [0], slope, needle="NULL utterance list")
            refused(a, b, 1, [0], None, slope, needle="NULL utterance list")
            refused(a, b, 1, [0], [0], slope, pos=False, needle="NULL pos")
            refused(a, far, 1, [0], [0], slope, needle="context")
            refused(a, plain, 1, [0], [0], slope, needle="coder")
            refused(plain, b, 1, [0], [0], slope, needle="coder")
            refused(a, other, 1, [0], [0], slope, needle="dimension")
            refused(a, b, 1, [0], [0], slope, needle="columns", first=DIM)
            refused(a, b, 1, [0], [0], slope, needle="cost", step_cost=float("nan"))
            refused(a, b, 2, [0, 3], [0, 0], slope, needle="outside batch a")
            refused(a, b, 2, [0, 2], [0, 2], slope, needle="outside batch b")
            refused(a, b, 2, [0, 1], [0, 0], slope, needle="without frames")
            refused(long, long, 65, [0] * 65, [0] * 65, slope, needle=str(65 * 2048 * 2048))
        for slope in (-1, 2, 64):
            refused(a, b, 1, [0], [0], slope, needle="slope = %d is neither 0 nor 1" % slope)
        # 9 x 4: ceil(8 / 2) = 4 exceeds 3; 5 x 7, 9 x 7 and 5 x 4 are admissible, and without the pattern every pair is
        refused(a, b, 3, [0, 2, 2], [0, 1, 0], 1, needle="pair 1: 9 x 4 frames are not admissible: ceil((na - 1) / 2) = 4 exceeds nb - 1 = 3")
        # the checks of llsm_gpu_batch_align come first, its cap among them; then the slope; then the pairs
        refused(a, b, 1, [2], [1], 1, step_cost=float("nan"), needle="cost")
        refused(a, b, 2, [2, 0], [1, 9], 1, needle="pair 1: utterance 9 is outside batch b")
        refused(long, long, 65, [0] * 65, [0] * 65, 7, needle="2^28")
        refused(a, b, 1, [2], [1], 2, needle="neither 0 nor 1")
        # accepted: no pairs (nothing is written or launched, and there are still no planes), whatever the slope
        n0 = launches()
        rc, msg, clean = call(a, b, 0, None, None, 5, pos=False, span=False, cost=False, last=False)
        assert rc == 0 and clean and launches() == n0
        no_plane(a)
        # a real call, the optional outputs left out
        rc, msg, clean = call(a, b, 2, [2, 0], [1, 0], 0, span=False, cost=False, last=False)
        assert rc == 0 and np.all(held[0][:14] != -7) and np.all(held[0][14:] == -7) and all(np.all(h == -7) for h in held[1:])
        assert launches() == n0 + 2
        assert L.llsm_gpu_batch_align_sub_plane(a.h, None, 0) == 9 * 4 + 5 * 7
        small = np.zeros(10, np.float32)
        assert L.llsm_gpu_batch_align_sub_plane(a.h, small.ctypes.data, 10) == -1 and "too small" in L.llsm_gpu_last_error().decode()
        # ... and all of them
        rc, msg, clean = call(a, b, 2, [2, 0], [0, 1], 1)
        assert rc == 0 and launches() == n0 + 4
        p, s, c, r = held
        assert np.all(p[:14] != -7) and np.all(p[14:] == -7) and np.all(s[:4] >= 0) and np.all(s[4:] == -7)
        assert np.all(c[:2] != -7) and np.all(c[2:] == -7) and np.all(r[:11] != -7) and np.all(r[11:] == -7)
        prof = ctx.profile()
        assert prof["k_align_sub_dtw"][1] == 1 and prof["k_align_sub_slope_dtw"][1] == 1
        pos, span, cost, last = a.align_sub(b, [2, 0], [0, 1], slope=True, last_row=True)
        assert beq(np.concatenate(pos), p[:14]) and np.array_equal(span.reshape(-1), s[:4]) and beq(cost, c[:2]) and beq(np.concatenate(last), r[:11])
        assert [x.shape for x in a.align_sub_planes()] == [(9, 7), (5, 4)]
        # a refusal after a success leaves the planes of the success in place
        kept = np.concatenate([x.reshape(-1) for x in a.align_sub_planes()])
        rc, msg, clean = call(a, b, 1, [1], [0])
        assert rc == -1 and clean and L.llsm_gpu_batch_align_sub_plane(a.h, None, 0) == len(kept)
        rc, msg, clean = call(a, b, 1, [2], [1], 1)
        assert rc == -1 and clean
        got = np.zeros(len(kept), np.float32)
        assert L.llsm_gpu_batch_align_sub_plane(a.h, got.ctypes.data, len(got)) == len(kept) and beq(got, kept)
        no_plane(b)                                                 # b was only ever the second batch
        # the planes of the other calls and every array of both batches are what they were
        for which, plane in planes.items():
            assert beq(a.debug_plane(which), plane), which
        after = all_arrays(a), all_arrays(b)
        for x, y in zip(before, after):
            assert x.keys() == y.keys() and llsm.A_CODE in x and all(beq(x[k], y[k]) for k in x)
        with pytest.raises(llsm.LlsmError):
            a.debug_plane(16)                                       # the planes have no number
    finally:
        ctx.set_profiling(False)
        for x in (a, b, plain, other, long, far):
            x.close()
        ctx2.close()
