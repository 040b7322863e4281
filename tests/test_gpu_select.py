"""-m gpu: llsm_gpu_batch_select against the numpy restatement of its rules (tests/select_reference.py).

Three layers, each exact because the rules fix every rounding: the candidate plane (plane 7) against rules S1 - S2 on the
uploaded LLSM_GPU_CODE, bit for bit; the join plane (plane 8) against rule S3 applied to the device's own plane 7; utt, pos
and cost against rules S4 - S5 applied to the device's own planes 7 and 8.  Then the whole chain from CODE, bit for bit.
On top of them: ties at all three layers (small-integer vectors, duplicated bank rows), NaN rows on either side,
invariance of an utterance's bits under everything around it, skip_own_utterance, a batch selected from itself, the chain
against float64 under the cap of tests/test_align_host.py (0.5 % of the frames; the float32 reference itself differs on 0
of 2 520), an analysed utterance whose stretch is selected back and rendered by splice, and every refusal: eleven on tiny
batches, the twelfth (a bank of more than 2^24 frames) on a bank of 2^24 + 1 frames of the smallest rows a batch takes,
beside a bank of exactly 2^24 frames that is searched to its last row.

Batches are tiny: layer 1 at nfft 128 and the coder at orders 64 + 5 (72 columns) enabled on batches without samples, and
synthetic LLSM_GPU_CODE rows uploaded; only the chain test analyses anything.  The target has utterances of 0, 1, 2, 63,
64, 65 and 129 frames: below, at and above the 64 target frames of a workgroup of k_select_knn and the 64 frames a
wavefront of k_select_path stores and walks back at a time.  The banks have utterances of 1, 7, 63, 64 and 65 frames (200
in all: four 64-row blocks, the last one partial), or 1, 7, 8 and 9 frames (below, at and above K = 8), or 2 049 frames.
The segment rule of k_select_knn is a rule of the bank's frames N alone: the bank is cut into min(64, ceil(N / 1024))
parts, a part rounded up to a multiple of 64 frames is the segment length, and as many segments of that length as cover
the bank are searched apart and merged: 2 049 frames are the smallest bank of three segments (of 704, 704 and 641)."""
import ctypes as C
import os

import numpy as np
import pytest

import libllsm2_amd as llsm
import select_reference as sref
from gpu_common import report
from test_align_host import DIFFER_CAP
from test_gpu_align import DIM, all_arrays, beq, bits, coded, random_code
from test_select_host import COST_REL, OPTS as HOST_OPTS, SEEDS, SHAPES, case as host_case, gen as host_gen
from verify_utils import GOLDEN, read_wav

pytestmark = pytest.mark.gpu

T_NFRM = [0, 1, 2, 63, 64, 65, 129]
B_NFRM = [1, 7, 63, 64, 65]
LONG_NFRM = [700, 700, 649]                                         # 2 049 frames: three segments
OPTS = dict(first=3, count=24, voicing_cost=5.0, join_cost=0.5, join_weight=0.75)


@pytest.fixture(scope="module")
def ctx():
    c = llsm.Context(0)
    yield c
    c.close()


def with_duplicates(code, seed, n):
    """n rows of code overwritten by copies of other rows"""
    rng = np.random.default_rng(seed)
    code = code.copy()
    dst = rng.choice(len(code), n, replace=False)
    code[dst] = code[rng.integers(0, len(code), n)]
    return code


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


def ref_kw(o):
    o = dict(o)
    o["skip_own"] = bool(o.pop("skip_own_utterance", 0))
    return o


def run(t, bank, **o):
    utt, pos, cost = t.select(bank, **o)
    F = t.layout.total_frames
    assert utt.dtype == np.int32 and pos.dtype == np.float32 and cost.dtype == np.float32
    assert utt.shape == (F,) and pos.shape == (F,) and cost.shape == (t.layout.n_utt,)
    return utt, pos, cost, t.debug_plane(7).reshape(F, 16), t.debug_plane(8).reshape(F, 64)


def check_layers(t, ct, bank, cb, **o):
    """the call against the reference, layer by layer and as a whole; returns what the device gave"""
    utt, pos, cost, p7, p8 = run(t, bank, **o)
    r = ref_kw(o)
    want7 = sref.candidates(ct, t.frm_off, cb, bank.frm_off, r["first"], r["count"], r["voicing_cost"], r["skip_own"])
    assert beq(p7, want7), (o, int(np.count_nonzero(bits(p7) != bits(want7))))
    want8 = sref.joins(cb, bank.frm_off, p7, t.frm_off, r["first"], r["count"], r["voicing_cost"], r["join_cost"], r["join_weight"])
    assert beq(p8, want8), (o, int(np.count_nonzero(bits(p8) != bits(want8))))
    wu, wp, wc = sref.path(p7, p8, t.frm_off, bank.frm_off)
    assert np.array_equal(utt, wu) and beq(pos, wp) and beq(cost, wc), o
    cu, cp, cc, _, _ = sref.select(ct, t.frm_off, cb, bank.frm_off, **r)
    assert np.array_equal(utt, cu) and beq(pos, cp) and beq(cost, cc), o
    nfrm = np.diff(bank.frm_off)
    assert np.all((utt >= 0) & (utt < len(nfrm))) and np.all((pos >= 0) & (pos < nfrm[utt])) and np.all(pos == np.floor(pos))
    return utt, pos, cost, p7, p8


# ---------------------------------------------------------------- 1: the three layers and the chain
@pytest.mark.parametrize("first", [0, 3])
@pytest.mark.parametrize("count", [1, 3, 24, 64])
def test_layers_exact(ctx, world, count, first):
    w = world["random"]
    o = dict(OPTS, first=first, count=count)
    utt, pos, cost, p7, p8 = check_layers(w["t"], w["ct"], w["bank"], w["cb"], **o)
    assert np.all(p7[:, 8:] >= 0) and np.all(cost >= 0) and cost[0] == 0 and (count == 1 or np.all(cost[1:] > 0))
    mixed = int(np.count_nonzero((w["ct"][:, 0, None] > 0.5) != (w["cb"][None, :, 0] > 0.5)))
    assert mixed > 1000                                             # the voicing term is exercised


def test_default_options_compare_the_spectrum_columns(ctx, world):
    w = world["random"]
    utt, pos, cost = w["t"].select(w["bank"])
    cu, cp, cc, _, _ = sref.select(w["ct"], w["t"].frm_off, w["cb"], w["bank"].frm_off, 3, 64)
    assert np.array_equal(utt, cu) and beq(pos, cp) and beq(cost, cc)
    u2, p2, c2 = w["t"].select(w["bank"], llsm.make_select_options())
    assert np.array_equal(utt, u2) and beq(pos, p2) and beq(cost, c2)


@pytest.mark.parametrize("n", [1, 7, 8, 9])
def test_banks_below_at_and_above_k(ctx, world, n):
    w = world["integer"]
    cb = random_code(30 + n, n, True)
    bank = coded(ctx, [n], cb)
    try:
        utt, pos, cost, p7, p8 = check_layers(w["t"], w["ct"], bank, cb, **OPTS)
        nu = min(8, n)
        assert np.all(p7[:, 8:8 + nu] >= 0) and np.all(p7[:, 8 + nu:] == -1) and np.all(p7[:, nu:8] == sref.CAP)
        assert np.all(p8.reshape(-1, 8, 8)[:, nu:] == 0) and np.all(p8.reshape(-1, 8, 8)[:, :, nu:] == 0)
    finally:
        bank.close()


@pytest.mark.parametrize("kind", ["random", "integer"])
def test_a_bank_of_three_segments(ctx, world, kind):
    w = world[kind]
    cb = random_code(40, sum(LONG_NFRM), kind == "integer")
    if kind == "integer":
        cb = with_duplicates(cb, 6, 600)                            # equal rows in different segments: the order (c, f) decides
    bank = coded(ctx, LONG_NFRM, cb)
    try:
        utt, pos, cost, p7, p8 = check_layers(w["t"], w["ct"], bank, cb, **OPTS)
        f = p7[:, 8:]
        seg = f // 704
        assert set(np.unique(seg)) == {0, 1, 2}
        assert int(np.count_nonzero(np.ptp(seg, axis=1) > 0)) > 100  # most lists draw on more than one segment
        if kind == "integer":
            tie = (p7[:, :7] == p7[:, 1:8]) & (seg[:, :-1] != seg[:, 1:])
            assert int(np.count_nonzero(tie)) > 50                  # equal costs from different segments
    finally:
        bank.close()


# ---------------------------------------------------------------- 2: ties and NaN
def test_ties_at_every_layer(ctx, world):
    w = world["integer"]
    for o in (dict(OPTS, join_cost=0.0, join_weight=1.0, voicing_cost=1.0), dict(OPTS, join_cost=1.0, join_weight=0.0)):
        utt, pos, cost, p7, p8 = check_layers(w["t"], w["ct"], w["bank"], w["cb"], **o)
        assert int(np.count_nonzero(p7[:, :7] == p7[:, 1:8])) > 200           # S2: equal costs, the smaller frame first
        assert np.all((p7[:, :7] < p7[:, 1:8]) | (p7[:, 8:15] < p7[:, 9:16]))
        P8 = p8.reshape(-1, 8, 8)
        assert int(np.count_nonzero((P8[:, :-1] == P8[:, 1:]) & (P8[:, 1:] > 0))) > 50   # S3 / S4: equal joins into one state
    # a constant bank and target: every distance ties -> the candidates are bank frames 0 ... 7 everywhere
    const = np.tile(random_code(3, 1), (sum(T_NFRM) + 20, 1))
    t = coded(ctx, T_NFRM, const[:sum(T_NFRM)]); bank = coded(ctx, [9, 11], const[:20])
    try:
        utt, pos, cost, p7, p8 = check_layers(t, const[:sum(T_NFRM)], bank, const[:20], **OPTS)
        assert np.all(p7[:, :8] == 0) and np.all(p7[:, 8:] == np.arange(8))
        assert np.all(utt == 0) and np.all(pos <= 7)
    finally:
        t.close(); bank.close()


def test_nan_rows_on_either_side(ctx, world):
    w = world["random"]
    ct, cb = w["ct"].copy(), w["cb"].copy()
    rng = np.random.default_rng(8)
    ct[5:9] = np.nan                                                # whole rows, the voicing column included
    ct[100 + rng.integers(0, 60, 20), 3 + rng.integers(0, 24, 20)] = np.nan
    ct[200, 10] = np.inf
    cb[3] = np.nan; cb[70:75, 3:27] = np.nan; cb[150, 5] = -np.inf
    cb[rng.integers(0, 200, 10), 3 + rng.integers(0, 24, 10)] = np.nan
    t = coded(ctx, T_NFRM, ct); bank = coded(ctx, B_NFRM, cb)
    try:
        utt, pos, cost, p7, p8 = check_layers(t, ct, bank, cb, **OPTS)   # returns 0, every index in the bank, the reference's bits
        assert np.all(np.isfinite(p7)) and np.all(np.isfinite(p8)) and np.all(np.isfinite(cost))
        assert np.all(p7[5:9, :8] == sref.CAP) and np.all(p7[5:9, 8:] == np.arange(8))
        # a bank of NaN rows alone
        cn = np.full((9, DIM), np.nan, np.float32)
        allnan = coded(ctx, [4, 5], cn)
        try:
            check_layers(t, ct, allnan, cn, **OPTS)
        finally:
            allnan.close()
    finally:
        t.close(); bank.close()


def test_a_weight_large_enough_to_overflow(ctx, world):
    """join_weight 1e30 on a join distance at the cap is +infinity in float32 (the note under S1 in llsm_gpu.h): no NaN
    arises, the planes, the path and the costs equal the reference's, and every index lies in the bank"""
    w = world["random"]
    cb = w["cb"].copy()
    cb[::3, 3:27] = np.nan                                          # every third bank row: its distances are the cap
    bank = coded(ctx, B_NFRM, cb)
    try:
        utt, pos, cost, p7, p8 = check_layers(w["t"], w["ct"], bank, cb, **dict(OPTS, join_weight=1e30))
        assert np.any(np.isinf(p8)) and not np.any(np.isnan(p8)) and not np.any(np.isnan(cost)) and np.all(np.isfinite(p7))
    finally:
        bank.close()


# ---------------------------------------------------------------- 3: invariance
def test_an_utterance_has_the_bits_it_has_alone(ctx, world):
    w = world["random"]
    t, bank = w["t"], w["bank"]
    before = all_arrays(t), all_arrays(bank)
    utt, pos, cost = t.select(bank, **OPTS)
    off = t.frm_off
    order = [6, 0, 3, 5, 1, 4, 2]                                   # the utterances placed elsewhere
    ct2 = np.concatenate([w["ct"][off[u]:off[u + 1]] for u in order])
    t2 = coded(ctx, [T_NFRM[u] for u in order], ct2)
    try:
        t2.select(bank, first=0, count=5, join_cost=3.0)            # an unrelated earlier call with other options
        u2, p2, c2 = t2.select(bank, **OPTS)
        for k, u in enumerate(order):
            a, b = int(t2.frm_off[k]), int(t2.frm_off[k + 1])
            assert np.array_equal(u2[a:b], utt[off[u]:off[u + 1]]) and beq(p2[a:b], pos[off[u]:off[u + 1]]) and beq(c2[k], cost[u]), u
    finally:
        t2.close()
    for u in (1, 4, 5, 6):                                          # alone
        t1 = coded(ctx, [T_NFRM[u]], w["ct"][off[u]:off[u + 1]])
        try:
            u1, p1, c1 = t1.select(bank, **OPTS)
            assert np.array_equal(u1, utt[off[u]:off[u + 1]]) and beq(p1, pos[off[u]:off[u + 1]]) and beq(c1[0], cost[u]), u
        finally:
            t1.close()
    ua, pa, ca = t.select(bank, **OPTS)                             # again, after the scratch has been used
    assert np.array_equal(ua, utt) and beq(pa, pos) and beq(ca, cost)
    # the call wrote no array of either batch
    after = all_arrays(t), all_arrays(bank)
    for x, y in zip(before, after):
        assert x.keys() == y.keys() and llsm.A_CODE in x
        assert all(beq(x[k], y[k]) for k in x)


# ---------------------------------------------------------------- 4: a batch against itself
def test_skip_own_utterance(ctx, world):
    w = world["integer"]
    b, cb = w["bank"], w["cb"]
    held = all_arrays(b)
    utt, pos, cost, p7, p8 = check_layers(b, cb, b, cb, skip_own_utterance=1, **OPTS)
    own = sref.frame_utt(b.frm_off)
    assert np.all(utt != own)
    f = p7[:, 8:]
    lo, hi = b.frm_off[own][:, None], b.frm_off[own + 1][:, None]
    assert np.all((f < lo) | (f >= hi)) and np.all(f >= 0)
    after = all_arrays(b)
    assert held.keys() == after.keys() and all(beq(held[k], after[k]) for k in held)


def test_a_batch_selects_itself(ctx, world):
    w = world["integer"]
    b, cb = w["bank"], w["cb"]
    for join_cost in (1.0, 0.0):
        o = dict(OPTS, first=3, count=64, voicing_cost=0.0, join_cost=join_cost)
        utt, pos, cost, p7, p8 = check_layers(b, cb, b, cb, **o)
        f = sref.flat(utt, pos, b.frm_off)
        g = np.arange(len(f))
        assert np.all(f <= g) and np.all(cost == 0)
        assert np.array_equal(bits(cb[f, 3:67]), bits(cb[g, 3:67]))  # itself, or an earlier bit-identical row
        assert np.all(p7[:, 0] == 0) and np.all(p7[:, 8] <= g)


# ---------------------------------------------------------------- 5: against float64
def test_against_float64(ctx):
    """the generated cases of tests/test_select_host.py: the device against the float64 chain"""
    differ = total = differ32 = 0
    worst = 0.0
    for k, shape in enumerate(SHAPES):
        for seed in SEEDS:
            ct, to, cb, bo = host_gen(shape, seed)
            t = coded(ctx, shape[0], ct); bank = coded(ctx, shape[1], cb)
            try:
                utt, pos, cost = t.select(bank, **HOST_OPTS)
            finally:
                t.close(); bank.close()
            (u32, p32, c32), (u64, p64, c64) = host_case(k, seed)
            differ += int(np.count_nonzero((utt != u64) | (pos != p64)))
            differ32 += int(np.count_nonzero((utt != u32) | (bits(pos) != bits(p32)))) + int(np.count_nonzero(bits(cost) != bits(c32)))
            total += len(utt)
            live = c64 > 0
            worst = max(worst, float(np.max(np.abs(cost[live].astype(np.float64) - c64[live]) / c64[live])))
    out = dict(frames=total, differ_from_float64=differ, differ_from_float32_reference=differ32, cost_rel=worst)
    print(out)
    report("select_float64", out)
    assert differ32 == 0
    assert differ <= DIFFER_CAP * total
    assert worst <= COST_REL


# ---------------------------------------------------------------- 6: from an analysis to splice
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
        utt, pos, cost, p7, p8 = check_layers(tgt, ct, bank, cb, first=3, count=64, voicing_cost=0.0, join_cost=1.0, join_weight=1.0)
        assert np.all(cost == 0) and np.all(utt == 0)
        rep = dict(frames=nd, bank_frames=nfrm, first=p, moved=int(np.count_nonzero(pos != p + np.arange(nd))), cost=float(cost[0]))
        print(rep)
        report("select_arctic_stretch", rep)
        dst.splice(bank, pos_a=pos, utt_a=utt)                      # the map as it came back
        dst.enable_coder(64, 5); dst.encode()
        ctx.sync()
        cd = dst.download(llsm.A_CODE)
        assert beq(cd[:, 3:67], ct[:, 3:67])
    finally:
        bank.close(); tgt.close(); dst.close()


# ---------------------------------------------------------------- 7: refusals
def test_refusals_write_nothing(ctx, world):
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
        rc = L.llsm_gpu_batch_select(x.h if x else None, y.h if y else None, C.byref(o), u.ctypes.data_as(llsm.P_int) if utt else None,
                                     p.ctypes.data_as(llsm.P_fp) if pos else None, c.ctypes.data_as(llsm.P_fp) if cost else None)
        return rc, L.llsm_gpu_last_error().decode(), bool(np.all(u == -7) and np.all(p == -7) and np.all(c == -7))

    def launches():
        return sum(v[1] for v in ctx.profile().values())

    def refused(x, y, needle="", **kw):
        n0 = launches()
        rc, msg, clean = call(x, y, **kw)
        assert rc == -1 and msg.startswith("llsm_gpu_batch_select:") and needle in msg and clean, (kw, rc, msg, clean)
        assert launches() == n0                                     # nothing was launched
        for which in (7, 8):
            with pytest.raises(llsm.LlsmError):
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
        # accepted: a target without frames (the costs are 0, nothing else is written, nothing is launched, no planes)
        rc, msg, clean = call(empty, b, utt=False, pos=False)
        assert rc == 0 and np.all(held[2][:2] == 0) and np.all(held[2][2:] == -7) and launches() == 0
        with pytest.raises(llsm.LlsmError):
            empty.debug_plane(7)
        # a real call, cost left out
        rc, msg, clean = call(a, b, cost=False, **OPTS)
        assert rc == 0 and np.all(held[2] == -7) and np.all(held[0][:14] != -7) and np.all(held[0][14:] == -7)
        assert np.all(held[1][:14] != -7) and np.all(held[1][14:] == -7) and launches() > 0
        got = held[0][:14].copy(), held[1][:14].copy()
        utt, pos, cost, p7, p8 = check_layers(a, ca, b, cb, **OPTS)
        assert np.array_equal(utt, got[0]) and beq(pos, got[1]) and cost[1] == 0
        # a refusal after a success leaves the planes of the success in place
        rc, msg, clean = call(a, b, first=-1)
        assert rc == -1 and clean and beq(a.debug_plane(7), p7.ravel()) and beq(a.debug_plane(8), p8.ravel())
        for which in (7, 8):
            with pytest.raises(llsm.LlsmError):
                b.debug_plane(which)                                # b was only ever the bank
        # no array of any batch changed
        after = [all_arrays(x) for x in everyone]
        for x, y in zip(before, after):
            assert x.keys() == y.keys() and all(beq(x[k], y[k]) for k in x)
    finally:
        ctx.set_profiling(False)
        for x in everyone + (far,):
            x.close()
        ctx2.close()


# ---------------------------------------------------------------- 8: the largest bank
MAX_BANK = 1 << 24


def largest(ctx, n):
    """a bank of one utterance of n frames at the smallest sizes a batch takes (a hop of 16 samples at 16 kHz, one harmonic,
    two PSD bins, one channel, layer 1 at nfft 64, coder orders 1 + 1: 5 columns): about 7 GB on the device for 2^24 frames"""
    ao = llsm.make_aoptions(thop=0.001, maxnhar=1, maxnhar_e=1, npsd=2, nchannel=1, f0_refine=0, chanfreq=[])
    b = llsm.Batch(ctx, ao, 16000.0, [0], [n])
    b.enable_layer1(64); b.enable_coder(1, 1)
    return b


def test_the_largest_bank_and_one_frame_more(ctx):
    """The twelfth refusal, and its edge.  A bank of 2^24 frames passes the size check: selected from itself with
    skip_own_utterance it is refused for the reason checked AFTER the size, and a small target finds its frames in the
    last three rows of it, whose indices 2^24 - 3 ... 2^24 - 1 are the largest plane 7 ever holds as floats.  A bank of
    2^24 + 1 frames is refused by the size check, with nothing launched, the three arrays untouched, no planes, and the
    arrays of the target and the CODE and F0 rows of the bank as they were (the other arrays of such a bank are gigabytes,
    and nothing was launched that could have written them)."""
    L = llsm.load()
    ct = np.zeros((3, 5), np.float32); ct[:, 3] = [1, 2, 3]
    t = coded(ctx, [3], ct, coder=(1, 1))
    held_t = all_arrays(t)

    def call(x, y, **kw):
        o = llsm.make_select_options(first=3, count=1, **kw)
        u = np.full(8, -7, np.int32); p = np.full(8, -7, np.float32); c = np.full(4, -7, np.float32)
        rc = L.llsm_gpu_batch_select(x.h, y.h, C.byref(o), u.ctypes.data_as(llsm.P_int), p.ctypes.data_as(llsm.P_fp),
                                     c.ctypes.data_as(llsm.P_fp))
        return rc, L.llsm_gpu_last_error().decode(), bool(np.all(u == -7) and np.all(p == -7) and np.all(c == -7))

    def launches():
        return sum(v[1] for v in ctx.profile().values())

    ctx.set_profiling(True); ctx.reset_profile()
    bank = None
    try:
        bank = largest(ctx, MAX_BANK + 1)
        assert bank.layout.total_frames == MAX_BANK + 1
        n0 = launches()
        for x in (t, bank):                                         # a small target, and the bank against itself
            rc, msg, clean = call(x, bank)
            assert rc == -1 and msg.startswith("llsm_gpu_batch_select:") and "more than 2^24 = 16777216" in msg and clean, (rc, msg, clean)
            assert "16777217 frames" in msg
            for which in (7, 8):
                with pytest.raises(llsm.LlsmError):
                    x.debug_plane(which)
        assert launches() == n0
        ctx.sync()
        assert not np.any(bank.download(llsm.A_CODE)) and not np.any(bank.download(llsm.A_F0))   # as enable_coder left them
        after = all_arrays(t)
        assert held_t.keys() == after.keys() and all(beq(held_t[k], after[k]) for k in held_t)
        bank.close(); bank = None

        bank = largest(ctx, MAX_BANK)
        n0 = launches()
        rc, msg, clean = call(bank, bank, skip_own_utterance=1)     # past the size check: refused by the check after it
        assert rc == -1 and "without a bank frame" in msg and "2^24" not in msg and clean, (rc, msg)
        assert launches() == n0
        cb = np.zeros((MAX_BANK, 5), np.float32); cb[-3:, 3] = [1, 2, 3]
        bank.upload(llsm.A_CODE, cb)
        utt, pos, cost, p7, p8 = run(t, bank, first=3, count=1, join_cost=1.0)
        want = MAX_BANK - 3 + np.arange(3)
        assert np.all(utt == 0) and np.array_equal(pos, want.astype(np.float32)) and np.all(cost == 0)
        assert np.array_equal(p7[:, 8], want.astype(np.float32)) and np.all(p7[:, 0] == 0)
        assert np.all((p7[:, 8:] >= 0) & (p7[:, 8:] < MAX_BANK)) and np.all(p7[:, 8:] == np.floor(p7[:, 8:]))
        assert p8[1, 0] == 0 and p8[2, 0] == 0                      # natural continuations at the end of the bank
        # the second slot, at c = 1 everywhere: for target frame 0 the zero rows, of which the smallest index wins; for
        # frames 1 and 2 the neighbour of their own row
        assert np.array_equal(p7[:, 1], np.float32([1, 1, 1])) and np.array_equal(p7[:, 9], np.float32([0, MAX_BANK - 3, MAX_BANK - 2]))
    finally:
        ctx.set_profiling(False)
        if bank is not None:
            bank.close()
        t.close()
