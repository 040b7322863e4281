"""-m gpu: llsm_gpu_batch_select_chain against the numpy restatement of its rules (tests/select_chain_reference.py).

Everything is exact because the rules fix every rounding: planes 10 and 11, utt, pos and cost against rules C1 - C6 from
the uploaded LLSM_GPU_CODE, bit for bit, and rule C3's ranking and rules C5 - C6 rerun on the device's own planes.  On top
of that the consequences P1 - P3 against llsm_gpu_batch_select on the same batches, ties in the ranking and in the minimum
(small-integer vectors, duplicated bank rows), NaN and infinite rows, an overflowing weight, invariance of an utterance's
bits under everything around it, the two calls leaving each other's planes alone, the quality case of
tests/test_select_chain_host.py, an analysed stretch selected back and rendered by splice, every refusal of the shared
check, and the chain against float64 under the cap of tests/test_align_host.py.

Batches are those of tests/test_gpu_select.py: target utterances of 0, 1, 2, 63, 64, 65 and 129 frames (the walk back
takes the back-pointer words 64 frames at a time), bank utterances of 1, 7, 63, 64 and 65 frames, banks of 1, 7, 8 and 9
frames, and one of 2 049 frames (three segments of k_select_knn).  count 72 is the one size at which k_select_chain
stages a second block of 64 columns."""
import ctypes as C
import os

import numpy as np
import pytest

import libllsm2_amd as llsm
import select_reference as sref
import select_chain_reference as cref
from gpu_common import report
from test_align_host import DIFFER_CAP
from test_gpu_align import DIM, all_arrays, beq, bits, coded, random_code
from test_gpu_select import B_NFRM, LONG_NFRM, OPTS, T_NFRM, ref_kw, with_duplicates
from test_select_chain_host import case as host_case, renditions
from test_select_host import COST_REL, OPTS as HOST_OPTS, SEEDS, SHAPES, gen as host_gen, join_cost_of
from verify_utils import GOLDEN, read_wav

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = llsm.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def world(ctx):
    """a target batch and a bank, once with random and once with small-integer vectors (the latter with duplicated bank rows)"""
    out = {}
    for kind in ("random", "integer"):
        ct = random_code(21, sum(T_NFRM), kind == "integer"); cb = random_code(22, sum(B_NFRM), kind == "integer")
        if kind == "integer":
            cb = with_duplicates(cb, 5, 60)
        out[kind] = dict(t=coded(ctx, T_NFRM, ct), bank=coded(ctx, B_NFRM, cb), ct=ct, cb=cb)
    yield out
    for w in out.values():
        w["t"].close(); w["bank"].close()


def run(t, bank, **o):
    utt, pos, cost = t.select_chain(bank, **o)
    F = t.layout.total_frames
    assert utt.dtype == np.int32 and pos.dtype == np.float32 and cost.dtype == np.float32
    assert utt.shape == (F,) and pos.shape == (F,) and cost.shape == (t.layout.n_utt,)
    return utt, pos, cost, t.debug_plane(10).reshape(F, 32), t.debug_plane(11).reshape(F, 256)


def check(t, ct, bank, cb, **o):
    """the call against the reference from CODE, and the reference's path on the device's own planes; returns what the
    device gave"""
    utt, pos, cost, p10, p11 = run(t, bank, **o)
    wu, wp, wc, w10, w11 = cref.chain(ct, t.frm_off, cb, bank.frm_off, **ref_kw(o))
    assert beq(p10, w10), (o, int(np.count_nonzero(bits(p10) != bits(w10))), np.argwhere(bits(p10) != bits(w10))[:4])
    assert beq(p11, w11), (o, int(np.count_nonzero(bits(p11) != bits(w11))), np.argwhere(bits(p11) != bits(w11))[:4])
    assert np.array_equal(utt, wu) and beq(pos, wp) and beq(cost, wc), o
    pu, pp, pc, want = cref.path_from_planes(p10, p11, t.frm_off, bank.frm_off)
    assert np.array_equal(utt, pu) and beq(pos, pp) and beq(cost, pc), o
    assert np.array_equal(want, p10[:, 24:].astype(np.int64))
    nfrm = np.diff(bank.frm_off)
    assert np.all((utt >= 0) & (utt < len(nfrm))) and np.all((pos >= 0) & (pos < nfrm[utt])) and np.all(pos == np.floor(pos))
    return utt, pos, cost, p10, p11


# ---------------------------------------------------------------- 1: the planes and the path
@pytest.mark.parametrize("count,first", [(1, 0), (1, 3), (3, 0), (3, 3), (24, 0), (24, 3), (64, 0), (64, 3), (72, 0)])
def test_exact(ctx, world, count, first):
    w = world["random"]
    utt, pos, cost, p10, p11 = check(w["t"], w["ct"], w["bank"], w["cb"], **dict(OPTS, first=first, count=count))
    assert np.all(p10[:, 16:24] >= 0) and np.all(cost >= 0) and cost[0] == 0
    assert int(np.count_nonzero(p10[:, 24:] >= 0)) > 1000           # followers nearly everywhere


def test_default_options_compare_the_spectrum_columns(ctx, world):
    w = world["random"]
    utt, pos, cost = w["t"].select_chain(w["bank"])
    cu, cp, cc, _, _ = cref.chain(w["ct"], w["t"].frm_off, w["cb"], w["bank"].frm_off, 3, 64)
    assert np.array_equal(utt, cu) and beq(pos, cp) and beq(cost, cc)
    u2, p2, c2 = w["t"].select_chain(w["bank"], llsm.make_select_options())
    assert np.array_equal(utt, u2) and beq(pos, p2) and beq(cost, c2)


@pytest.mark.parametrize("n", [1, 7, 8, 9])
def test_banks_below_at_and_above_k(ctx, world, n):
    w = world["integer"]
    cb = random_code(30 + n, n, True)
    bank = coded(ctx, [n], cb)
    try:
        utt, pos, cost, p10, p11 = check(w["t"], w["ct"], bank, cb, **OPTS)
        nu = min(8, n)
        assert np.all(p10[:, 16:16 + nu] >= 0) and np.all(p10[:, 16 + nu:24] == -1) and np.all(p10[:, nu:8] == sref.CAP)
        assert np.all(p10[:, 24 + max(0, n - 8):] == -1)
    finally:
        bank.close()


@pytest.mark.parametrize("kind", ["random", "integer"])
def test_a_bank_of_three_segments(ctx, world, kind):
    w = world[kind]
    cb = random_code(40, sum(LONG_NFRM), kind == "integer")
    if kind == "integer":
        cb = with_duplicates(cb, 6, 600)
    bank = coded(ctx, LONG_NFRM, cb)
    try:
        utt, pos, cost, p10, p11 = check(w["t"], w["ct"], bank, cb, **OPTS)
        assert set(np.unique(p10[:, 16:24] // 704)) == {0, 1, 2}
        assert np.all(p10[1:, 24:][np.diff(sref.frame_utt(w["t"].frm_off)) == 0][:, :4] >= 0)
    finally:
        bank.close()


# ---------------------------------------------------------------- 2: ties, NaN, overflow
def test_ties_in_the_ranking_and_in_the_minimum(ctx, world):
    w = world["integer"]
    for o in (dict(OPTS, join_cost=0.0, join_weight=1.0, voicing_cost=1.0), dict(OPTS, join_cost=1.0, join_weight=0.0),
              dict(OPTS, join_cost=0.0, join_weight=0.0)):
        utt, pos, cost, p10, p11 = check(w["t"], w["ct"], w["bank"], w["cb"], **o)
        P = p11.reshape(-1, 16, 16)
        assert int(np.count_nonzero((P[:, :-1] == P[:, 1:]) & (P[:, 1:] > 0))) > 50 or o["join_weight"] == 0
    # a constant bank and target: every cost ties -> near frames 0 ... 7 everywhere, and ties throughout the pool
    const = np.tile(random_code(3, 1), (sum(T_NFRM) + 40, 1))
    t = coded(ctx, T_NFRM, const[:sum(T_NFRM)]); bank = coded(ctx, [19, 21], const[:40])
    try:
        utt, pos, cost, p10, p11 = check(t, const[:sum(T_NFRM)], bank, const[:40], **OPTS)
        assert np.all(p10[:, :8] == 0) and np.all(p10[:, 16:24] == np.arange(8))
        # the utterance of 129 frames: the chains start at 8, the successor of near frame 7, and die at 18, the end of bank
        # utterance 0; one starts with every frame, so from frame 9 on every follower slot is taken
        g0 = int(t.frm_off[6])
        fol = p10[g0 + 9:g0 + 129, 24:]
        assert np.all((fol >= 8) & (fol <= 18)) and np.all(utt == 0)
    finally:
        t.close(); bank.close()


def test_nan_and_infinite_rows_on_either_side(ctx, world):
    w = world["random"]
    ct, cb = w["ct"].copy(), w["cb"].copy()
    rng = np.random.default_rng(8)
    ct[5:9] = np.nan
    ct[100 + rng.integers(0, 60, 20), 3 + rng.integers(0, 24, 20)] = np.nan
    ct[200, 10] = np.inf
    cb[3] = np.nan; cb[70:75, 3:27] = np.nan; cb[150, 5] = -np.inf
    cb[rng.integers(0, 200, 10), 3 + rng.integers(0, 24, 10)] = np.nan
    t = coded(ctx, T_NFRM, ct); bank = coded(ctx, B_NFRM, cb)
    try:
        utt, pos, cost, p10, p11 = check(t, ct, bank, cb, **OPTS)
        assert np.all(np.isfinite(p10)) and np.all(np.isfinite(p11)) and np.all(np.isfinite(cost))
        cn = np.full((9, DIM), np.nan, np.float32)
        allnan = coded(ctx, [4, 5], cn)
        try:
            check(t, ct, allnan, cn, **OPTS)
        finally:
            allnan.close()
    finally:
        t.close(); bank.close()


def test_a_weight_large_enough_to_overflow(ctx, world):
    w = world["random"]
    cb = w["cb"].copy()
    cb[::3, 3:27] = np.nan                                          # every third bank row: its distances are the cap
    bank = coded(ctx, B_NFRM, cb)
    try:
        utt, pos, cost, p10, p11 = check(w["t"], w["ct"], bank, cb, **dict(OPTS, join_weight=1e30))
        assert np.any(np.isinf(p11)) and not np.any(np.isnan(p11)) and not np.any(np.isnan(cost)) and np.all(np.isfinite(p10))
    finally:
        bank.close()


def test_skip_own_utterance(ctx, world):
    w = world["integer"]
    b, cb = w["bank"], w["cb"]
    held = all_arrays(b)
    utt, pos, cost, p10, p11 = check(b, cb, b, cb, skip_own_utterance=1, **OPTS)
    own = sref.frame_utt(b.frm_off)
    assert np.all(utt != own)
    f = p10[:, 16:]
    lo, hi = b.frm_off[own][:, None], b.frm_off[own + 1][:, None]
    assert np.all((f < 0) | (f < lo) | (f >= hi)) and np.all(f[:, :8] >= 0) and np.any(f[:, 8:] >= 0)
    after = all_arrays(b)
    assert held.keys() == after.keys() and all(beq(held[k], after[k]) for k in held)


# ---------------------------------------------------------------- 3: the consequences, against llsm_gpu_batch_select
def test_p1_p2_and_the_planes_of_the_two_calls(ctx, world):
    for kind in ("random", "integer"):
        w = world[kind]
        t, bank = w["t"], w["bank"]
        F = t.layout.total_frames
        for o in (OPTS, dict(OPTS, join_cost=0.0), dict(OPTS, join_cost=50.0, join_weight=0.0), dict(OPTS, join_weight=1e30)):
            su, sp, sc = t.select(bank, **o)
            p7, p8 = t.debug_plane(7), t.debug_plane(8)
            utt, pos, cost, p10, p11 = run(t, bank, **o)
            assert beq(t.debug_plane(7), p7) and beq(t.debug_plane(8), p8)          # the chain left planes 7 and 8 alone
            assert beq(p10[:, :8], p7.reshape(F, 16)[:, :8]) and beq(p10[:, 16:24], p7.reshape(F, 16)[:, 8:])      # P1
            assert beq(p11.reshape(F, 16, 16)[:, :8, :8], p8.reshape(F, 8, 8))
            assert np.all(cost <= sc), (o, cost, sc)                                # P2
            t.select(bank, first=0, count=5, join_cost=3.0)                         # select leaves planes 10 and 11 alone
            assert beq(t.debug_plane(10), p10.ravel()) and beq(t.debug_plane(11), p11.ravel())


def test_p3_a_bank_of_single_frames(ctx, world):
    w = world["integer"]
    cb = random_code(50, 150, True)
    bank = coded(ctx, [1] * 150, cb)
    try:
        su, sp, sc = w["t"].select(bank, **OPTS)
        utt, pos, cost, p10, p11 = check(w["t"], w["ct"], bank, cb, **OPTS)
        assert np.array_equal(utt, su) and beq(pos, sp) and beq(cost, sc)
        assert np.all(p10[:, 24:] == -1) and np.all(p10[:, 8:16] == sref.CAP)
        P = p11.reshape(-1, 16, 16)
        assert not np.any(P[:, 8:]) and not np.any(P[:, :, 8:])
    finally:
        bank.close()


# ---------------------------------------------------------------- 4: invariance
def test_an_utterance_has_the_bits_it_has_alone(ctx, world):
    w = world["random"]
    t, bank = w["t"], w["bank"]
    before = all_arrays(t), all_arrays(bank)
    utt, pos, cost = t.select_chain(bank, **OPTS)
    off = t.frm_off
    order = [6, 0, 3, 5, 1, 4, 2]                                   # the utterances placed elsewhere
    ct2 = np.concatenate([w["ct"][off[u]:off[u + 1]] for u in order])
    t2 = coded(ctx, [T_NFRM[u] for u in order], ct2)
    try:
        t2.select_chain(bank, first=0, count=5, join_cost=3.0)      # an unrelated earlier call with other options
        u2, p2, c2 = t2.select_chain(bank, **OPTS)
        for k, u in enumerate(order):
            a, b = int(t2.frm_off[k]), int(t2.frm_off[k + 1])
            assert np.array_equal(u2[a:b], utt[off[u]:off[u + 1]]) and beq(p2[a:b], pos[off[u]:off[u + 1]]) and beq(c2[k], cost[u]), u
    finally:
        t2.close()
    for u in (1, 4, 5, 6):                                          # alone
        t1 = coded(ctx, [T_NFRM[u]], w["ct"][off[u]:off[u + 1]])
        try:
            u1, p1, c1 = t1.select_chain(bank, **OPTS)
            assert np.array_equal(u1, utt[off[u]:off[u + 1]]) and beq(p1, pos[off[u]:off[u + 1]]) and beq(c1[0], cost[u]), u
        finally:
            t1.close()
    ua, pa, ca = t.select_chain(bank, **OPTS)                       # again, after the scratch has been used
    assert np.array_equal(ua, utt) and beq(pa, pos) and beq(ca, cost)
    after = all_arrays(t), all_arrays(bank)                         # the call wrote no array of either batch
    for x, y in zip(before, after):
        assert x.keys() == y.keys() and llsm.A_CODE in x
        assert all(beq(x[k], y[k]) for k in x)


# ---------------------------------------------------------------- 5: quality
@pytest.mark.parametrize("seed", range(4))
def test_one_rendition_carries_the_stretch(ctx, seed):
    tgt, bank, off = renditions(seed, dim=DIM)
    t = coded(ctx, [50], tgt); b = coded(ctx, [60] * 20, bank)
    try:
        o = dict(first=3, count=24, join_cost=join_cost_of(bank))
        su, sp, sc = t.select(b, **o)
        utt, pos, cost, p10, p11 = check(t, tgt, b, bank, voicing_cost=0.0, join_weight=1.0, **o)
        assert len(np.unique(utt)) == 1 and np.array_equal(pos, (5 + np.arange(50)).astype(np.float32))
        assert cref.joins_of(utt, pos, [0, 50], off)[0] == 0 and cref.joins_of(su, sp, [0, 50], off)[0] >= 1
        assert cost[0] < sc[0]
    finally:
        t.close(); b.close()


def test_feeds_splice(ctx):
    x, fs = read_wav(os.path.join(GOLDEN, "arctic_a0001.wav"))
    f0 = np.load(os.path.join(GOLDEN, "arctic_a0001_f0_hop128.npy")).astype(np.float32)
    nfrm = len(f0)
    voiced = f0 > 0
    run_len = np.zeros(nfrm, np.int64)                              # the longest voiced stretch
    for i in range(nfrm):
        run_len[i] = (run_len[i - 1] + 1 if i else 1) if voiced[i] else 0
    end = int(np.argmax(run_len)); nd = int(min(run_len[end], 60)); p = end - nd + 1
    assert nd >= 20 and np.all(voiced[p:p + nd])
    ao = llsm.make_aoptions(thop=128.0 / fs, f0_refine=0)
    bank = llsm.Batch(ctx, ao, fs, [len(x)], [nfrm])
    tgt = llsm.Batch(ctx, ao, fs, [0], [nd])
    dst = llsm.Batch(ctx, ao, fs, [0], [nd])
    try:
        bank.upload(llsm.A_X, x); bank.upload(llsm.A_F0, f0)
        bank.analyze(); bank.tolayer1(2048)
        bank.enable_coder(64, 5); bank.encode()
        zero = np.zeros(nd, np.int32)
        tgt.splice(bank, pos_a=(p + np.arange(nd)).astype(np.float32), utt_a=zero)
        tgt.enable_coder(64, 5); tgt.encode()
        ctx.sync()
        ct, cb = tgt.download(llsm.A_CODE), bank.download(llsm.A_CODE)
        utt, pos, cost, p10, p11 = check(tgt, ct, bank, cb, first=3, count=64, voicing_cost=0.0, join_cost=1.0, join_weight=1.0)
        assert np.all(cost == 0) and np.all(utt == 0)
        dst.splice(bank, pos_a=pos, utt_a=utt)                      # the map as it came back
        dst.enable_coder(64, 5); dst.encode()
        ctx.sync()
        cd = dst.download(llsm.A_CODE)
        assert beq(cd[:, 3:67], ct[:, 3:67])
    finally:
        bank.close(); tgt.close(); dst.close()


# ---------------------------------------------------------------- 6: refusals
def test_refusals_write_nothing(ctx):
    L = llsm.load()
    ca, cb = random_code(1, 14), random_code(2, 11)
    a = coded(ctx, [5, 0, 9], ca); b = coded(ctx, [7, 4], cb)
    plain = coded(ctx, [5], coder=None)                             # layer 1, no coder
    other = coded(ctx, [5], random_code(4, 5)[:, :40], coder=(32, 5))   # 40 columns
    empty = coded(ctx, [0, 0])
    one = coded(ctx, [6], random_code(6, 6))                        # its only utterance is the whole bank
    ctx2 = llsm.Context(0)
    far = coded(ctx2, [5], random_code(5, 5))
    everyone = (a, b, plain, other, empty, one)
    before = [all_arrays(x) for x in everyone]
    held = []

    def call(x, y, utt=True, pos=True, cost=True, **kw):
        """the raw call with the three arrays pre-filled with a mark: (return code, message, marks untouched)"""
        o = llsm.make_select_options(**kw)
        u = np.full(64, -7, np.int32); p = np.full(64, -7, np.float32); c = np.full(16, -7, np.float32)
        held[:] = [u, p, c]
        rc = L.llsm_gpu_batch_select_chain(x.h if x else None, y.h if y else None, C.byref(o),
                                           u.ctypes.data_as(llsm.P_int) if utt else None,
                                           p.ctypes.data_as(llsm.P_fp) if pos else None, c.ctypes.data_as(llsm.P_fp) if cost else None)
        return rc, L.llsm_gpu_last_error().decode(), bool(np.all(u == -7) and np.all(p == -7) and np.all(c == -7))

    def launches():
        return sum(v[1] for v in ctx.profile().values())

    def refused(x, y, needle="", **kw):
        n0 = launches()
        rc, msg, clean = call(x, y, **kw)
        assert rc == -1 and msg.startswith("llsm_gpu_batch_select_chain:") and needle in msg and clean, (kw, rc, msg, clean)
        assert launches() == n0                                     # nothing was launched
        for which in (10, 11):
            with pytest.raises(llsm.LlsmError, match="no llsm_gpu_batch_select_chain has run"):
                a.debug_plane(which)                                # no call has succeeded on a yet

    ctx.set_profiling(True); ctx.reset_profile()
    try:
        refused(None, b, needle="NULL batch")
        refused(a, None, needle="NULL batch")
        refused(a, far, needle="context")
        refused(a, plain, needle="coder")
        refused(plain, b, needle="coder")
        refused(a, other, needle="dimension")
        for kw in (dict(first=-1), dict(first=DIM), dict(first=3, count=DIM - 2), dict(first=DIM - 1, count=2)):
            refused(a, b, needle="columns", **kw)
        nan, inf = float("nan"), float("inf")
        for kw in (dict(voicing_cost=nan), dict(join_cost=nan), dict(voicing_cost=inf), dict(join_cost=inf), dict(join_cost=-0.5),
                   dict(voicing_cost=-1e-6), dict(voicing_cost=-inf)):
            refused(a, b, needle="cost", **kw)
        for kw in (dict(join_weight=nan), dict(join_weight=inf), dict(join_weight=-1.0)):
            refused(a, b, needle="join_weight", **kw)
        refused(a, b, needle="skip_own_utterance", skip_own_utterance=2)
        refused(a, b, needle="t == bank", skip_own_utterance=1)
        refused(a, b, needle="NULL utt", utt=False)
        refused(a, b, needle="NULL pos", pos=False)
        refused(a, empty, needle="no frames")
        refused(one, one, needle="without a bank frame", skip_own_utterance=1)
        assert launches() == 0
        # a select on a does not make planes 10 and 11 readable
        a.select(b, **OPTS)
        n_sel = launches()
        for which in (10, 11):
            with pytest.raises(llsm.LlsmError):
                a.debug_plane(which)
        # accepted: a target without frames (the costs are 0, nothing else is written, nothing is launched, no planes)
        rc, msg, clean = call(empty, b, utt=False, pos=False)
        assert rc == 0 and np.all(held[2][:2] == 0) and np.all(held[2][2:] == -7) and launches() == n_sel
        with pytest.raises(llsm.LlsmError):
            empty.debug_plane(10)
        # a real call, cost left out
        rc, msg, clean = call(a, b, cost=False, **OPTS)
        assert rc == 0 and np.all(held[2] == -7) and np.all(held[0][:14] != -7) and np.all(held[0][14:] == -7)
        assert np.all(held[1][:14] != -7) and np.all(held[1][14:] == -7) and launches() > n_sel
        assert "k_select_chain" in ctx.profile() and ctx.profile()["k_select_chain"][1] == 1
        got = held[0][:14].copy(), held[1][:14].copy()
        utt, pos, cost, p10, p11 = check(a, ca, b, cb, **OPTS)
        assert np.array_equal(utt, got[0]) and beq(pos, got[1]) and cost[1] == 0
        # a refusal after a success leaves the planes of the success in place
        rc, msg, clean = call(a, b, first=-1)
        assert rc == -1 and clean and beq(a.debug_plane(10), p10.ravel()) and beq(a.debug_plane(11), p11.ravel())
        for which in (10, 11):
            with pytest.raises(llsm.LlsmError):
                b.debug_plane(which)                                # b was only ever the bank
        after = [all_arrays(x) for x in everyone]                   # no array of any batch changed
        for x, y in zip(before, after):
            assert x.keys() == y.keys() and all(beq(x[k], y[k]) for k in x)
    finally:
        ctx.set_profiling(False)
        for x in everyone + (far,):
            x.close()
        ctx2.close()


# ---------------------------------------------------------------- 7: against float64
def test_against_float64(ctx):
    """the generated cases of tests/test_select_host.py: the device against the float64 chain"""
    differ = total = differ32 = 0
    worst = 0.0
    for k, shape in enumerate(SHAPES):
        for seed in SEEDS:
            ct, to, cb, bo = host_gen(shape, seed)
            t = coded(ctx, shape[0], ct); bank = coded(ctx, shape[1], cb)
            try:
                utt, pos, cost = t.select_chain(bank, **HOST_OPTS)
            finally:
                t.close(); bank.close()
            (u32, p32, c32, _, _), (u64, p64, c64, _, _) = host_case(k, seed)
            differ += int(np.count_nonzero((utt != u64) | (pos != p64)))
            differ32 += int(np.count_nonzero((utt != u32) | (bits(pos) != bits(p32)))) + int(np.count_nonzero(bits(cost) != bits(c32)))
            total += len(utt)
            live = c64 > 0
            worst = max(worst, float(np.max(np.abs(cost[live].astype(np.float64) - c64[live]) / c64[live])))
    out = dict(frames=total, differ_from_float64=differ, differ_from_float32_reference=differ32, cost_rel=worst)
    print(out)
    report("select_chain_float64", out)
    assert differ32 == 0
    assert differ <= DIFFER_CAP * total
    assert worst <= COST_REL
