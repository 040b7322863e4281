"""-m gpu: llsm_gpu_batch_align_band against the numpy restatement of its rules (tests/align_band_reference.py).

The layers of tests/test_gpu_align.py, each exact because the rules fix every rounding: the band planes (plane 9) against
rule D1 in float32 in the band layout, bit for bit, +infinity outside the rows' ranges; pos and cost against rules B3 - B4
in float32 applied to the device's own plane 9, bit for bit.  On top of them: a band that covers the matrix against
llsm_gpu_batch_align on the device, invariance of a pair's bits under everything around it, the generated pairs of
tests/test_align_band_host.py under a band of 15 % against the full call, the positions fed to splice, and every refusal.

Batches are those of tests/align_common.py: layer 1 at nfft 128, the coder at orders 64 + 5, no samples, synthetic
LLSM_GPU_CODE.  The pairs sit below, at and above the 64 rows of a strip of k_align_band_dtw and the 64 x 64 tile of
k_align_band_dist, with three and five strips whose column windows move (129 x 200, 200 x 129, 257 x 300) and slopes well
above and below 1 (2 x 63, 10 x 1000, 7 x 1, 200 x 129)."""
import ctypes as C
import math

import numpy as np
import pytest

import libllsm2_amd as llsm
import align_reference as aref
import align_band_reference as bref
from align_common import BAND_SIZES as SIZES, DIM, SEEDS, all_arrays, band_widths, beq, coded, planes_of, random_code, rows_of

pytestmark = pytest.mark.gpu

PAIRS = [(1, 1), (1, 7), (7, 1), (2, 63), (63, 64), (64, 65), (65, 129), (129, 200), (200, 129), (257, 300), (10, 1000)]
NA = [p[0] for p in PAIRS]
NB = [p[1] for p in PAIRS]
IDENT = np.arange(len(PAIRS), dtype=np.int32)
LEAST = [bref.band_min(na, nb) for na, nb in PAIRS]
# the bands of one call, one per pair: the least, one more, 5 and 40 raised to the pair's least
BANDS = {"least": LEAST, "least+1": [m + 1 for m in LEAST], "5": [max(5, m) for m in LEAST], "40": [max(40, m) for m in LEAST]}
COVER = [nb - 1 for nb in NB]                                       # every row spans the whole matrix


@pytest.fixture(scope="module")
def ctx():
    c = llsm.Context(0)
    yield c
    c.close()


def make_world(ctx, ca, cb):
    a = coded(ctx, NA, ca); b = coded(ctx, NB, cb)
    return dict(a=a, b=b, ra=rows_of(a, ca), rb=rows_of(b, cb), ca=ca, cb=cb)


@pytest.fixture(scope="module")
def world(ctx):
    """batch a with the A sides and batch b with the B sides of PAIRS: random vectors, small integers (ties), one constant
    vector (every comparison ties), and random vectors with NaN rows in some utterances of a"""
    out = {}
    for kind in ("random", "integer"):
        out[kind] = make_world(ctx, random_code(21, sum(NA), kind == "integer"), random_code(22, sum(NB), kind == "integer"))
    const = np.tile(random_code(3, 1), (sum(NA) + sum(NB), 1))
    out["constant"] = make_world(ctx, const[:sum(NA)], const[sum(NA):])
    ca = out["random"]["ca"].copy()
    rng = np.random.default_rng(8)
    off = np.concatenate([[0], np.cumsum(NA)])
    ca[off[3]:off[4]] = np.nan                                      # every row of 2 x 63, voicing column included
    ca[off[6] + 20:off[6] + 23, 3:27] = np.nan                      # a few rows in the middle of 65 x 129
    for p in (8, 9):                                                # scattered over 200 x 129 and 257 x 300
        ca[off[p] + rng.integers(0, NA[p], 40), 3 + rng.integers(0, 24, 40)] = np.nan
    ca[off[10] + 4] = np.nan                                        # one row of 10 x 1000
    out["nan"] = make_world(ctx, ca, out["random"]["cb"])
    yield out
    for w in out.values():
        w["a"].close(); w["b"].close()


# ---------------------------------------------------------------- 1: the band planes
@pytest.mark.parametrize("voicing_cost", [0.0, 5.0])
@pytest.mark.parametrize("first", [0, 3])
@pytest.mark.parametrize("count", [1, 24, 64])
def test_plane_exact(ctx, world, count, first, voicing_cost):
    w = world["random"]
    want = [aref.dist(fa, fb, first, count, voicing_cost) for fa, fb in zip(w["ra"], w["rb"])]
    for name, bands in BANDS.items():
        w["a"].align_band(w["b"], IDENT, IDENT, bands, first=first, count=count, voicing_cost=voicing_cost)
        got = planes_of(w["a"], 9, NA, band_widths(bands))
        for p in range(len(PAIRS)):
            layout = bref.to_band(want[p], bands[p])
            assert beq(got[p], layout), (PAIRS[p], name, int(np.count_nonzero(got[p].view(np.uint32) != layout.view(np.uint32))))
    assert any(np.any(np.isposinf(bref.to_band(want[p], BANDS["40"][p]))) for p in range(len(PAIRS)))


# ---------------------------------------------------------------- 2: the paths
@pytest.mark.parametrize("kind", ["random", "integer", "constant", "nan"])
@pytest.mark.parametrize("step_cost", [0.0, 1.0])
@pytest.mark.parametrize("name", list(BANDS))
def test_path_exact(ctx, world, name, step_cost, kind):
    w = world[kind]
    bands = BANDS[name]
    pos, cost = w["a"].align_band(w["b"], IDENT, IDENT, bands, first=3, count=24, voicing_cost=5.0, step_cost=step_cost)
    planes = planes_of(w["a"], 9, NA, band_widths(bands))
    assert cost.dtype == np.float32 and cost.shape == (len(PAIRS),)
    for p, P in enumerate(planes):
        na, nb = PAIRS[p]
        want_pos, want_cost, _ = bref.dtw(bref.from_band(P, nb), bands[p], step_cost)
        assert pos[p].dtype == np.float32 and beq(pos[p], want_pos), (PAIRS[p], step_cost, pos[p], want_pos)
        assert beq(cost[p], want_cost), (PAIRS[p], step_cost, cost[p], want_cost)
        lo, hi = bref.rows(na, nb, bands[p])
        assert np.all(pos[p] >= lo) and np.all(pos[p] <= hi) and np.all(np.diff(pos[p]) >= 0), PAIRS[p]
    if kind == "nan":
        assert sum(bool(np.any(np.isnan(P))) for P in planes) >= 5 and np.any(np.isnan(cost))


# ---------------------------------------------------------------- 3: a band over the whole matrix is the full call
@pytest.mark.parametrize("kind", ["random", "integer", "nan"])
def test_full_coverage_is_align(ctx, world, kind):
    w = world[kind]
    for step_cost in (0.0, 1.0):
        opts = dict(first=3, count=24, voicing_cost=5.0, step_cost=step_cost)
        want_pos, want_cost = w["a"].align(w["b"], IDENT, IDENT, **opts)
        plane6 = w["a"].debug_plane(6)
        for bands in (COVER, [c + 3 for c in COVER]):
            pos, cost = w["a"].align_band(w["b"], IDENT, IDENT, bands, **opts)
            assert all(beq(x, y) for x, y in zip(pos, want_pos)) and beq(cost, want_cost), (kind, step_cost)
            assert beq(w["a"].debug_plane(6), plane6)               # plane 6 is the full call's alone
            full = planes_of(w["a"], 6, NA, NB)
            for p, P in enumerate(planes_of(w["a"], 9, NA, band_widths(bands))):
                assert beq(bref.from_band(P, NB[p]), full[p]), PAIRS[p]


# ---------------------------------------------------------------- 4: invariance
def test_a_pair_has_the_bits_it_has_alone(ctx, world):
    w = world["random"]
    a, b = w["a"], w["b"]
    opts = dict(first=3, count=24, step_cost=1.0, voicing_cost=5.0)
    bands = np.array(BANDS["5"], np.int32)
    before = all_arrays(a), all_arrays(b)
    pos, cost = a.align_band(b, IDENT, IDENT, bands, **opts)
    planes = planes_of(a, 9, NA, band_widths(bands))
    # alone
    for p in range(len(PAIRS)):
        p1, c1 = a.align_band(b, [p], [p], int(bands[p]), **opts)
        assert beq(p1[0], pos[p]) and beq(c1[0], cost[p]) and beq(planes_of(a, 9, [NA[p]], band_widths([bands[p]]))[0], planes[p]), p
    # the list reversed
    pr, cr = a.align_band(b, IDENT[::-1], IDENT[::-1], bands[::-1], **opts)
    rplanes = planes_of(a, 9, NA[::-1], band_widths(bands[::-1]))
    for p in range(len(PAIRS)):
        q = len(PAIRS) - 1 - p
        assert beq(pr[q], pos[p]) and beq(cr[q], cost[p]) and beq(rplanes[q], planes[p]), p
    # a second call, after other calls have used the scratch
    p2, c2 = a.align_band(b, IDENT, IDENT, bands, **opts)
    assert all(beq(x, y) for x, y in zip(p2, pos)) and beq(c2, cost)
    assert all(beq(x, y) for x, y in zip(planes_of(a, 9, NA, band_widths(bands)), planes))
    # one batch on both sides
    both = coded(ctx, NA + NB, np.concatenate([w["ca"], w["cb"]]))
    try:
        held = all_arrays(both)
        ps, cs = both.align_band(both, IDENT, IDENT + len(PAIRS), bands, **opts)
        assert all(beq(x, y) for x, y in zip(ps, pos)) and beq(cs, cost)
        assert all(beq(x, y) for x, y in zip(planes_of(both, 9, NA, band_widths(bands)), planes))
        after = all_arrays(both)
        assert held.keys() == after.keys() and all(beq(held[k], after[k]) for k in held)
    finally:
        both.close()
    # one pair (129 x 200) under different bands in one call: each has the bits it has alone under its band
    widths = np.array([LEAST[7], 3, 17, 64, 199, 250], np.int32)
    pq, cq = a.align_band(b, [7] * len(widths), [7] * len(widths), widths, **opts)
    qplanes = planes_of(a, 9, [NA[7]] * len(widths), band_widths(widths))
    D = aref.dist(w["ra"][7], w["rb"][7], 3, 24, 5.0)
    for k, width in enumerate(widths):
        p1, c1 = a.align_band(b, [7], [7], int(width), **opts)
        assert beq(pq[k], p1[0]) and beq(cq[k], c1[0]), width
        assert beq(qplanes[k], bref.to_band(D, int(width))), width
    assert len({c.tobytes() for c in cq}) > 1 and np.all(np.diff(cq) <= 0)   # a wider band costs no more
    # no array of either batch changed
    after = all_arrays(a), all_arrays(b)
    for x, y in zip(before, after):
        assert x.keys() == y.keys() and llsm.A_CODE in x
        assert all(beq(x[k], y[k]) for k in x)


# ---------------------------------------------------------------- 5: the generated pairs, and on to splice
def test_generated_pairs_and_splice(ctx):
    """the 48 generated pairs of tests/test_align_band_host.py as one call under a band of 15 % of nb: the bits of the full
    call on the device (the host test shows that the band holds the full path); the positions of one pair go into splice"""
    cases = [(size, seed) for size in SIZES for seed in SEEDS]
    na = [s[0] for s, _ in cases]; nb = [s[1] for s, _ in cases]
    ca = np.zeros((sum(na), DIM), np.float32); cb = np.zeros((sum(nb), DIM), np.float32)
    ia = ib = 0
    for size, seed in cases:
        A, B, _ = aref.make(seed, size[0], size[1], 24, 0.3)
        ca[ia:ia + size[0], 3:27] = A.astype(np.float32); cb[ib:ib + size[1], 3:27] = B.astype(np.float32)
        ia += size[0]; ib += size[1]
    a = coded(ctx, na, ca); b = coded(ctx, nb, cb)
    k = 40                                                          # a pair of 257 x 300
    out = llsm.Batch(ctx, llsm.make_aoptions(f0_refine=0), 44100.0, [0], [na[k]])
    try:
        idx = np.arange(len(cases), dtype=np.int32)
        bands = [math.ceil(0.15 * n) for n in nb]
        want_pos, want_cost = a.align(b, idx, idx, first=3, count=24, step_cost=1.0)
        pos, cost = a.align_band(b, idx, idx, bands, first=3, count=24, step_cost=1.0)
        assert all(beq(x, y) for x, y in zip(pos, want_pos)) and beq(cost, want_cost)
        assert a.debug_plane(9).size < 0.4 * a.debug_plane(6).size
        # the rows of b are zeros apart from LLSM_GPU_CODE: splice only has to take the positions
        for aid, rows in all_arrays(b).items():
            if aid != llsm.A_CODE:
                b.upload(aid, np.zeros_like(rows))
        assert (na[k], nb[k]) == (257, 300)
        utt = np.full(na[k], k, np.int32)
        out.splice(b, pos_a=pos[k], utt_a=utt, utt_b=utt, pos_b=pos[k], mix=np.full(na[k], 0.5, np.float32))
        ctx.sync()
        assert np.all(np.isfinite(out.download(llsm.A_F0)))
    finally:
        a.close(); b.close(); out.close()


# ---------------------------------------------------------------- 6: refusals
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
        rc = L.llsm_gpu_batch_align_band(x.h if x else None, y.h if y else None, n, None if ua is None else pi(ua),
                                         None if ub is None else pi(ub), None if band is None else pi(band), C.byref(o),
                                         p.ctypes.data_as(llsm.P_fp) if pos else None, c.ctypes.data_as(llsm.P_fp) if cost else None)
        return rc, L.llsm_gpu_last_error().decode(), bool(np.all(p == -7) and np.all(c == -7))

    def refused(*args, needle="", **kw):
        rc, msg, clean = call(*args, **kw)
        assert rc == -1 and msg.startswith("llsm_gpu_batch_align_band:") and needle in msg and clean, (args, kw, rc, msg, clean)
        with pytest.raises(llsm.LlsmError):
            a.debug_plane(9)                                        # no call has succeeded on a yet

    try:
        a.align(b, [0], [0])                                        # the full call does not make a plane 9
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
        refused(a, b, 2, [0, 2], [0, 1], [3, -1], needle="pair 1: band < 0")
        # b against a: 7 x 5 is connected from a band of 0 on, 4 x 9 from 1 on
        assert (bref.band_min(7, 5), bref.band_min(4, 9)) == (0, 1)
        refused(b, a, 2, [0, 1], [0, 2], [3, 0], needle="pair 1: a band of 0 is not connected for 4 x 9 frames: llsm_gpu_align_band_min is 1")
        # 4 pairs of 70 000 rows under a band of 500: 280 280 000 cells, refused on the host before anything is allocated
        refused(long, long, 4, [0] * 4, [0] * 4, [500] * 4, needle=str(4 * 70000 * 1001))
        refused(long, long, 2, [0] * 2, [0] * 2, [2 ** 31 - 1, 5], needle="more than 2^28")
        # accepted: no pairs (nothing is written, and there is still no plane); then a real call, cost left out
        rc, msg, clean = call(a, b, 0, None, None, None, pos=False, cost=False)
        assert rc == 0 and clean
        with pytest.raises(llsm.LlsmError):
            a.debug_plane(9)
        rc, msg, clean = call(a, b, 2, [2, 0], [1, 0], [1, 2], cost=False)
        assert rc == 0 and np.all(held[1] == -7) and np.all(held[0][:14] != -7) and np.all(held[0][14:] == -7)
        assert a.debug_plane(9).shape == (9 * 3 + 5 * 5,)
        pos, cost = a.align_band(b, [2, 0], [1, 0], [1, 2])
        assert beq(np.concatenate(pos), held[0][:14])
        # a refusal after a success leaves the plane of the success in place
        plane = a.debug_plane(9)
        rc, msg, clean = call(a, b, 1, [1], [0], [3])
        assert rc == -1 and clean and beq(a.debug_plane(9), plane)
        rc, msg, clean = call(a, b, 1, [0], [0], [-2])
        assert rc == -1 and clean and beq(a.debug_plane(9), plane)
        with pytest.raises(llsm.LlsmError):
            b.debug_plane(9)                                        # b was only ever the second batch
    finally:
        for x in (a, b, plain, other, long, far):
            x.close()
        ctx2.close()
