"""-m gpu: llsm_gpu_batch_align against the numpy restatement of its rules (tests/align_reference.py).

Two layers, each exact because the rules fix every rounding: the distance planes (plane 6) against rule D1 in float32,
bit for bit; pos and cost against rules D2 - D3 in float32 applied to the device's own plane 6, bit for bit.  On top of
them: ties and NaN rows, invariance of a pair's bits under everything around it, the whole chain against float64 under the
cap of tests/test_align_host.py (0.5 % of the frames; the float32 reference itself differs on 0 of 8 316), an analysed
utterance aligned with a retimed copy of itself and fed to splice, and every refusal.

Batches are tiny: layer 1 at nfft 128 and the coder at orders 64 + 5 (72 columns) enabled on batches without samples, and
synthetic LLSM_GPU_CODE rows uploaded; only the chain test analyses anything.  The pair sizes put 1, 2, 63, 64, 65, 129 and
200 frames on either side: below, at and above the 64 rows of a strip of k_align_dtw and the 64 x 64 tile of k_align_dist,
and above 128."""
import ctypes as C
import os

import numpy as np
import pytest

import libllsm2_amd as llsm
import align_reference as aref
from gpu_common import report
from align_common import DIFFER_CAP, DIM, FULL_SIZES as SIZES, SEEDS, all_arrays, beq, bits, coded, full_case as host_case, \
    planes_of, random_code, rows_of
from verify_utils import GOLDEN, read_wav

pytestmark = pytest.mark.gpu

PAIRS = [(1, 1), (1, 7), (7, 1), (2, 63), (63, 64), (64, 65), (65, 129), (129, 200)]
NA = [p[0] for p in PAIRS]
NB = [p[1] for p in PAIRS]
IDENT = np.arange(len(PAIRS), dtype=np.int32)


@pytest.fixture(scope="module")
def ctx():
    c = llsm.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def world(ctx):
    """batch a with the A sides and batch b with the B sides of PAIRS, once with random and once with small-integer vectors"""
    out = {}
    for kind in ("random", "integer"):
        ca = random_code(11, sum(NA), kind == "integer"); cb = random_code(12, sum(NB), kind == "integer")
        a = coded(ctx, NA, ca); b = coded(ctx, NB, cb)
        out[kind] = dict(a=a, b=b, ra=rows_of(a, ca), rb=rows_of(b, cb), ca=ca, cb=cb)
    yield out
    for w in out.values():
        w["a"].close(); w["b"].close()


# ---------------------------------------------------------------- 1: the planes
@pytest.mark.parametrize("voicing_cost", [0.0, 5.0])
@pytest.mark.parametrize("first", [0, 3])
@pytest.mark.parametrize("count", [1, 3, 24, 64])
def test_plane_exact(ctx, world, count, first, voicing_cost):
    w = world["random"]
    w["a"].align(w["b"], IDENT, IDENT, first=first, count=count, voicing_cost=voicing_cost)
    got = planes_of(w["a"], 6, NA, NB)
    for p, (fa, fb) in enumerate(zip(w["ra"], w["rb"])):
        want = aref.dist(fa, fb, first, count, voicing_cost)
        assert beq(got[p], want), (PAIRS[p], int(np.count_nonzero(bits(got[p]) != bits(want))))
    if voicing_cost:
        mixed = sum(int(np.count_nonzero((fa[:, 0, None] > 0.5) != (fb[None, :, 0] > 0.5))) for fa, fb in zip(w["ra"], w["rb"]))
        assert mixed > 1000                                         # the voicing term is exercised


# ---------------------------------------------------------------- 2: the paths
@pytest.mark.parametrize("kind", ["random", "integer"])
@pytest.mark.parametrize("step_cost", [0.0, 1.0])
def test_path_exact(ctx, world, step_cost, kind):
    w = world[kind]
    pos, cost = w["a"].align(w["b"], IDENT, IDENT, first=3, count=24, voicing_cost=5.0, step_cost=step_cost)
    planes = planes_of(w["a"], 6, NA, NB)
    assert cost.dtype == np.float32 and cost.shape == (len(PAIRS),)
    ties = 0
    for p, D in enumerate(planes):
        want_pos, want_cost = aref.dtw(D, step_cost)
        assert pos[p].dtype == np.float32 and beq(pos[p], want_pos), (PAIRS[p], step_cost, pos[p], want_pos)
        assert beq(cost[p], want_cost), (PAIRS[p], step_cost, cost[p], want_cost)
        assert pos[p].min() >= 0 and pos[p].max() <= PAIRS[p][1] - 1 and np.all(np.diff(pos[p]) >= 0)
        acc, _ = aref.accumulate(D, step_cost)
        ties += int(np.count_nonzero(acc[:-1, 1:] + np.float32(step_cost) == acc[:-1, :-1]))
    if kind == "integer":
        assert ties > 100                                           # up ties with the diagonal often: "<" is exercised


# ---------------------------------------------------------------- 3: ties and NaN
def test_ties_and_forced_borders(ctx, world):
    const = np.tile(random_code(3, 1), (sum(NA) + sum(NB), 1))
    a = coded(ctx, NA, const[:sum(NA)]); b = coded(ctx, NB, const[sum(NA):])
    try:
        pos, cost = a.align(b, IDENT, IDENT, first=0, count=DIM)
        for p, (na, nb) in enumerate(PAIRS):
            if na <= nb:                                            # the diagonal from the end, then row 0
                want = (np.arange(na) + (nb - na)).astype(np.float32); want[0] = (nb - na) * 0.5
            else:                                                   # ... then column 0
                want = np.maximum(np.arange(na) - (na - nb), 0).astype(np.float32)
            assert beq(pos[p], want), (PAIRS[p], pos[p])
        assert np.all(cost == 0) and np.all(a.debug_plane(6) == 0)
    finally:
        a.close(); b.close()
    # NaN in the rows of some utterances of a: the call succeeds, pos stays inside, the other pairs keep their bits
    w = world["random"]
    opts = dict(first=3, count=24, step_cost=1.0, voicing_cost=5.0)
    clean_pos, clean_cost = w["a"].align(w["b"], IDENT, IDENT, **opts)
    ca = w["ca"].copy()
    nan_pairs = (3, 5, 7)
    rng = np.random.default_rng(8)
    for p in nan_pairs:
        lo, hi = int(w["a"].frm_off[p]), int(w["a"].frm_off[p + 1])
        if p == 3:
            ca[lo:hi] = np.nan                                      # every row, voicing column included
        elif p == 5:
            ca[lo + 20:lo + 23, 3:27] = np.nan                      # a few rows in the middle
        else:
            ca[lo + rng.integers(0, hi - lo, 40), 3 + rng.integers(0, 24, 40)] = np.nan
    a = coded(ctx, NA, ca)
    try:
        pos, cost = a.align(w["b"], IDENT, IDENT, **opts)
        planes = planes_of(a, 6, NA, NB)
        for p in range(len(PAIRS)):
            if p in nan_pairs:
                assert not np.any(np.isnan(pos[p])) and pos[p].min() >= 0 and pos[p].max() <= NB[p] - 1, (p, pos[p])
                assert np.all(np.diff(pos[p]) >= 0)
                assert np.any(np.isnan(planes[p]))
                want_pos, want_cost = aref.dtw(planes[p], 1.0)      # NaN compares false on the device as in numpy
                assert beq(pos[p], want_pos) and beq(cost[p], want_cost), p
            else:
                assert beq(pos[p], clean_pos[p]) and beq(cost[p], clean_cost[p]), p
    finally:
        a.close()


# ---------------------------------------------------------------- 4: invariance
def test_a_pair_has_the_bits_it_has_alone(ctx, world):
    w = world["random"]
    a, b = w["a"], w["b"]
    opts = dict(first=3, count=24, step_cost=1.0, voicing_cost=5.0)
    before = all_arrays(a), all_arrays(b)
    pos, cost = a.align(b, IDENT, IDENT, **opts)
    planes = planes_of(a, 6, NA, NB)
    # alone
    for p in range(len(PAIRS)):
        p1, c1 = a.align(b, [p], [p], **opts)
        assert beq(p1[0], pos[p]) and beq(c1[0], cost[p]) and beq(planes_of(a, 6, [NA[p]], [NB[p]])[0], planes[p]), p
    # the list reversed
    pr, cr = a.align(b, IDENT[::-1], IDENT[::-1], **opts)
    rplanes = planes_of(a, 6, NA[::-1], NB[::-1])
    for p in range(len(PAIRS)):
        q = len(PAIRS) - 1 - p
        assert beq(pr[q], pos[p]) and beq(cr[q], cost[p]) and beq(rplanes[q], planes[p]), p
    # a second call, after other calls have used the scratch
    p2, c2 = a.align(b, IDENT, IDENT, **opts)
    assert all(beq(x, y) for x, y in zip(p2, pos)) and beq(c2, cost)
    assert all(beq(x, y) for x, y in zip(planes_of(a, 6, NA, NB), planes))
    # one batch on both sides
    both = coded(ctx, NA + NB, np.concatenate([w["ca"], w["cb"]]))
    try:
        held = all_arrays(both)
        ps, cs = both.align(both, IDENT, IDENT + len(PAIRS), **opts)
        assert all(beq(x, y) for x, y in zip(ps, pos)) and beq(cs, cost)
        assert all(beq(x, y) for x, y in zip(planes_of(both, 6, NA, NB), planes))
        after = all_arrays(both)
        assert held.keys() == after.keys() and all(beq(held[k], after[k]) for k in held)
    finally:
        both.close()
    # one query against a bank: utterance 5 of a (64 frames) against every utterance of b, four times over
    ub = np.tile(IDENT, 4)
    ua = np.full(32, 5, np.int32)
    pq, cq = a.align(b, ua, ub, **opts)
    qplanes = planes_of(a, 6, [NA[5]] * len(ub), [NB[u] for u in ub])
    alone = [a.align(b, [5], [u], **opts) for u in IDENT]
    for k, u in enumerate(ub):
        assert beq(pq[k], alone[u][0][0]) and beq(cq[k], alone[u][1][0]), k
        assert beq(qplanes[k], aref.dist(w["ra"][5], w["rb"][u], 3, 24, 5.0)), k
    assert beq(pq[5], pos[5]) and beq(cq[5], cost[5])
    # no array of either batch changed
    after = all_arrays(a), all_arrays(b)
    for x, y in zip(before, after):
        assert x.keys() == y.keys() and llsm.A_CODE in x
        assert all(beq(x[k], y[k]) for k in x)


# ---------------------------------------------------------------- 5: against float64
def test_against_float64(ctx):
    """the generated pairs of tests/test_align_host.py as one call: the device against the float64 chain"""
    cases = [(size, seed) for size in SIZES for seed in SEEDS]
    na = [s[0] for s, _ in cases]; nb = [s[1] for s, _ in cases]
    ca = np.zeros((sum(na), DIM), np.float32); cb = np.zeros((sum(nb), DIM), np.float32)
    ia = ib = 0
    for size, seed in cases:
        A, B, _ = aref.make(seed, size[0], size[1], 24, 0.3)
        ca[ia:ia + size[0], 3:27] = A.astype(np.float32); cb[ib:ib + size[1], 3:27] = B.astype(np.float32)
        ia += size[0]; ib += size[1]
    a = coded(ctx, na, ca); b = coded(ctx, nb, cb)
    try:
        idx = np.arange(len(cases), dtype=np.int32)
        pos, cost = a.align(b, idx, idx, first=3, count=24, step_cost=1.0)
    finally:
        a.close(); b.close()
    differ = total = differ32 = 0
    worst = 0.0
    for k, (size, seed) in enumerate(cases):
        (p32, c32), (p64, c64), _ = host_case(size, seed)
        differ += int(np.count_nonzero(pos[k] != p64)); differ32 += int(np.count_nonzero(bits(pos[k]) != bits(p32)))
        total += len(p64)
        worst = max(worst, abs(float(cost[k]) - float(c64)) / float(c64))
    out = dict(frames=total, differ_from_float64=differ, differ_from_float32_reference=differ32, cost_rel=worst)
    print(out)
    report("align_float64", out)
    assert differ32 == 0
    assert differ <= DIFFER_CAP * total
    assert worst <= 1e-5


# ---------------------------------------------------------------- 6: from an analysis to splice
def test_feeds_splice(ctx):
    x, fs = read_wav(os.path.join(GOLDEN, "arctic_a0001.wav"))
    f0 = np.load(os.path.join(GOLDEN, "arctic_a0001_f0_hop128.npy")).astype(np.float32)
    nfrm = len(f0)
    assert nfrm == 1154
    ao = llsm.make_aoptions(thop=128.0 / fs, f0_refine=0)
    src = llsm.Batch(ctx, ao, fs, [len(x)], [nfrm])
    nd = 1000
    dst = llsm.Batch(ctx, ao, fs, [0], [nd])
    out = llsm.Batch(ctx, ao, fs, [0], [nd])
    try:
        src.upload(llsm.A_X, x); src.upload(llsm.A_F0, f0)
        src.analyze(); src.tolayer1(2048)
        src.enable_coder(64, 5); src.encode()
        # a smooth non-uniform map of the nd output frames onto the source: its slope swings between 0.76 and 1.24 of the mean
        u = np.linspace(0, 1, nd)
        warp = np.minimum((u + 0.12 * np.sin(2 * np.pi * u) / (2 * np.pi) * 2) * (nfrm - 1), nfrm - 1).astype(np.float32)
        assert np.all(np.diff(warp) > 0) and warp[0] == 0
        dst.retime(src, warp)
        dst.enable_coder(64, 5); dst.encode()
        ctx.sync()
        pos, cost = dst.align(src, [0], [0])
        cd, cs = dst.download(llsm.A_CODE), src.download(llsm.A_CODE)
        want_pos, want_cost = aref.align(cd, cs, 3, 64)
        assert beq(dst.debug_plane(6).reshape(nd, nfrm), aref.dist(cd, cs, 3, 64, 0.0))
        assert beq(pos[0], want_pos) and beq(cost[0], want_cost)
        assert np.all(np.diff(pos[0]) >= 0) and pos[0][0] >= 0 and pos[0][-1] <= nfrm - 1
        err = np.abs(pos[0].astype(np.float64) - warp)
        rep = dict(frames=nd, source_frames=nfrm, mean_abs=float(err.mean()), max_abs=float(err.max()), cost=float(cost[0]))
        print(rep)
        report("align_retimed_arctic", rep)
        # side a: the retimed rendition again; side b: the source at the aligned positions; half and half
        zero = np.zeros(nd, np.int32)
        out.splice(src, pos_a=warp, utt_a=zero, utt_b=zero, pos_b=pos[0], mix=np.full(nd, 0.5, np.float32))
        ctx.sync()
        f0_out = out.download(llsm.A_F0)
        assert np.all(np.isfinite(f0_out)) and np.count_nonzero(f0_out) > 0
    finally:
        src.close(); dst.close(); out.close()


# ---------------------------------------------------------------- 7: refusals
def test_refusals_write_nothing(ctx, world):
    L = llsm.load()
    w = world["random"]
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
        rc = L.llsm_gpu_batch_align(x.h if x else None, y.h if y else None, n, None if ua is None else pi(ua),
                                    None if ub is None else pi(ub), C.byref(o), p.ctypes.data_as(llsm.P_fp) if pos else None,
                                    c.ctypes.data_as(llsm.P_fp) if cost else None)
        return rc, L.llsm_gpu_last_error().decode(), bool(np.all(p == -7) and np.all(c == -7))

    def refused(*args, needle="", **kw):
        rc, msg, clean = call(*args, **kw)
        assert rc == -1 and msg.startswith("llsm_gpu_batch_align:") and needle in msg and clean, (args, kw, rc, msg, clean)
        with pytest.raises(llsm.LlsmError):
            a.debug_plane(6)                                        # no call has succeeded on a yet

    try:
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
        # accepted: no pairs (nothing is written, and there is still no plane); then a real call, cost left out
        rc, msg, clean = call(a, b, 0, None, None, pos=False, cost=False)
        assert rc == 0 and clean
        with pytest.raises(llsm.LlsmError):
            a.debug_plane(6)
        rc, msg, clean = call(a, b, 2, [2, 0], [1, 0], cost=False)
        assert rc == 0 and np.all(held[1] == -7) and np.all(held[0][:14] != -7) and np.all(held[0][14:] == -7)
        assert a.debug_plane(6).shape == (9 * 4 + 5 * 7,)
        pos, cost = a.align(b, [2, 0], [1, 0])
        assert beq(np.concatenate(pos), held[0][:14])
        # a refusal after a success leaves the plane of the success in place
        plane = a.debug_plane(6)
        rc, msg, clean = call(a, b, 1, [1], [0])
        assert rc == -1 and clean and beq(a.debug_plane(6), plane)
        with pytest.raises(llsm.LlsmError):
            b.debug_plane(6)                                        # b was only ever the second batch
    finally:
        for x in (a, b, plain, other, long, far):
            x.close()
        ctx2.close()
