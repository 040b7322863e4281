"""Host side of llsm_gpu_batch_select (no GPU): the default options, the refusals of llsm_gpu_select_check with their
messages, and the numpy restatement of rules S1 - S5 (tests/select_reference.py) on its own: cases written by hand with a
tie at every comparison, banks below, at and above K = 8 frames, the end of a bank utterance, float32 against the same
code in float64, and the quality of the selection -- a property of the rules, checked here and not on the device.

Measured with the generated cases below (vectors normal x 3 in 24 columns, join_cost 1, SEEDS x SHAPES): the float32
chain differs from the float64 chain on 0 of 2 520 frames, cost agrees to 3.2e-7 relative (printed by the test)."""
import ctypes as C

import numpy as np
import pytest

import libllsm2_amd as llsm
import align_reference as aref
import select_reference as sref
from test_align_host import DIFFER_CAP

COST_REL = 1e-5
SEEDS = range(6)
SHAPES = [([40, 65, 1], [50, 64, 30]), ([129, 2], [7, 63, 65]), ([100, 83], [9])]   # (target utterances, bank utterances)
OPTS = dict(first=3, count=24, voicing_cost=0.0, join_cost=1.0, join_weight=1.0)
z = np.float32


def test_default_options():
    o = llsm.SelectOptions()
    llsm.load().llsm_gpu_select_default_options(C.byref(o))
    assert (o.first, o.count, o.voicing_cost, o.join_cost, o.join_weight, o.skip_own_utterance) == (3, 0, 0.0, 0.0, 1.0, 0)
    m = llsm.make_select_options(join_cost=2.0, count=7, skip_own_utterance=1)
    assert (m.first, m.count, m.voicing_cost, m.join_cost, m.join_weight, m.skip_own_utterance) == (3, 7, 0.0, 2.0, 1.0, 1)
    with pytest.raises(TypeError):
        llsm.make_select_options(step_cost=0.1)


nan, inf = float("nan"), float("inf")
# with orders 8 + 2 the vectors have 13 columns; a count <= 0 stands for order_spec = 8, so first = 12 alone means [12, 20)
REFUSED = [(dict(first=-1), "columns"), (dict(first=13), "columns"), (dict(first=12), "columns"),
           (dict(first=3, count=11), "columns"), (dict(first=0, count=14), "columns"), (dict(first=12, count=2), "columns"),
           (dict(first=2 ** 31 - 1, count=2 ** 31 - 1), "columns"),
           (dict(voicing_cost=nan), "NaN"), (dict(join_cost=nan), "NaN"), (dict(join_weight=nan), "NaN"),
           (dict(voicing_cost=inf), "infinite"), (dict(join_cost=inf), "infinite"), (dict(join_weight=inf), "infinite"),
           (dict(join_cost=-inf), "infinite"),
           (dict(voicing_cost=-1.0), "voicing_cost < 0"), (dict(join_cost=-1e-6), "join_cost < 0"),
           (dict(join_weight=-0.5), "join_weight < 0"),
           (dict(skip_own_utterance=2), "skip_own_utterance"), (dict(skip_own_utterance=-1), "skip_own_utterance")]


@pytest.mark.parametrize("kw,needle", REFUSED, ids=lambda v: ",".join("%s=%s" % i for i in v.items()) if isinstance(v, dict) else None)
def test_check_refusals(kw, needle):
    L = llsm.load()
    o = llsm.make_select_options(**kw)
    assert L.llsm_gpu_select_check(C.byref(o), 8, 2) == -1
    msg = L.llsm_gpu_last_error().decode()
    assert msg.startswith("llsm_gpu_batch_select:") and needle in msg, msg


@pytest.mark.parametrize("orders", [(0, 2), (8, 0), (-1, 2)])
def test_check_refuses_a_coder_that_is_not_enabled(orders):
    L = llsm.load()
    assert L.llsm_gpu_select_check(None, *orders) == -1
    msg = L.llsm_gpu_last_error().decode()
    assert msg.startswith("llsm_gpu_batch_select:") and "coder" in msg


def test_check_accepts_edges_and_null():
    L = llsm.load()
    assert L.llsm_gpu_select_check(None, 8, 2) == 0
    for kw in (dict(), dict(first=0, count=13), dict(first=12, count=1), dict(first=3, count=-5), dict(first=5),
               dict(voicing_cost=0.0, join_cost=0.0, join_weight=0.0), dict(voicing_cost=1e30, join_cost=1e30, join_weight=1e30),
               dict(skip_own_utterance=1)):                         # (t == bank is the call's to check)
        o = llsm.make_select_options(**kw)
        assert L.llsm_gpu_select_check(C.byref(o), 8, 2) == 0, kw


def test_select_refuses_null_batch():
    L = llsm.load()
    utt = np.full(4, -7, np.int32); pos = np.full(4, -7, np.float32); cost = np.full(4, -7, np.float32)
    assert L.llsm_gpu_batch_select(None, None, None, utt.ctypes.data_as(llsm.P_int), pos.ctypes.data_as(llsm.P_fp),
                                   cost.ctypes.data_as(llsm.P_fp)) == -1
    assert L.llsm_gpu_last_error().decode().startswith("llsm_gpu_batch_select: NULL batch")
    assert np.all(utt == -7) and np.all(pos == -7) and np.all(cost == -7)


# ---------------------------------------------------------------- cases written by hand
def rows(values, dim=6):
    """coder vectors whose column 3 holds `values`, everything else 0"""
    c = np.zeros((len(values), dim), np.float32); c[:, 3] = values
    return c


def test_duplicate_bank_rows_keep_the_smaller_index():
    bank = rows([5, 1, 5, 1, 1, 9, 5, 1, 1, 1, 1, 1])
    p7 = sref.candidates(rows([1, 5]), [0, 2], bank, [0, 12], 3, 1)
    assert p7.dtype == np.float32 and p7.shape == (2, 16)
    assert list(p7[0, 8:]) == [1, 3, 4, 7, 8, 9, 10, 11] and np.all(p7[0, :8] == 0)   # eight of the nine equal rows, ascending
    assert list(p7[1, 8:]) == [0, 2, 6, 1, 3, 4, 5, 7]              # (5 - 9)^2 ties with (5 - 1)^2
    assert list(p7[1, :8]) == [0, 0, 0, 16, 16, 16, 16, 16]


def test_a_nan_bank_row_lands_at_the_cap_and_last():
    bank = rows([2, nan, 7, inf])
    p7 = sref.candidates(rows([3]), [0, 1], bank, [0, 4], 3, 1)
    assert list(p7[0, 8:12]) == [0, 2, 1, 3] and list(p7[0, 12:]) == [-1] * 4
    assert list(p7[0, :4]) == [1, 16, sref.CAP, sref.CAP] and np.all(p7[0, 4:8] == sref.CAP)
    # a NaN target row: every distance is the cap, the order is f alone
    p7 = sref.candidates(rows([nan]), [0, 1], bank, [0, 4], 3, 1)
    assert list(p7[0, 8:12]) == [0, 1, 2, 3] and np.all(p7[0, :8] == sref.CAP)
    # with such rows the joins and the path stay finite
    utt, pos, cost, p7, p8 = sref.select(rows([3, nan, 2]), [0, 3], bank, [0, 2, 4], 3, 1, join_cost=1.0)
    assert np.all(np.isfinite(p8)) and np.all(np.isfinite(cost)) and np.all((utt >= 0) & (utt < 2)) and np.all((pos >= 0) & (pos < 2))


@pytest.mark.parametrize("n", [1, 7, 8, 9])
def test_banks_below_at_and_above_k(n):
    rng = np.random.default_rng(n)
    bank = rows(rng.permutation(n) * 2.0)
    tgt = rows(rng.random(5) * 2 * n)
    utt, pos, cost, p7, p8 = sref.select(tgt, [0, 2, 2, 5], bank, [0, n], 3, 1, join_cost=0.5)
    nu = min(8, n)
    assert np.all(p7[:, 8:8 + nu] >= 0) and np.all(p7[:, 8 + nu:] == -1) and np.all(p7[:, nu:8] == sref.CAP)
    for g in range(5):                                              # the nu nearest, in the order (c, f)
        d = (tgt[g, 3] - bank[:, 3]) ** 2
        want = sorted(range(n), key=lambda f: (d[f], f))[:nu]
        assert list(p7[g, 8:8 + nu]) == want and list(p7[g, :nu]) == [d[f] for f in want]
    P8 = p8.reshape(5, 8, 8)
    assert np.all(P8[[0, 2]] == 0) and np.all(P8[:, nu:] == 0) and np.all(P8[:, :, nu:] == 0)   # first frames, absent slots
    assert np.all(utt == 0) and np.all(pos < n) and cost.shape == (3,) and cost[1] == 0


def test_a_continuation_across_an_utterance_end_is_not_natural():
    bank = rows([0, 10, 20, 30, 40, 50])                           # two bank utterances of three frames
    tgt = rows([20, 30, 40])
    p7 = sref.candidates(tgt, [0, 3], bank, [0, 3, 6], 3, 1)
    assert list(p7[:, 8]) == [2, 3, 4]
    p8 = sref.joins(bank, [0, 3, 6], p7, [0, 3], 3, 1, join_cost=0.25, join_weight=2.0).reshape(3, 8, 8)
    # 2 -> 3 crosses the end of utterance 0: s = fa = 2, J = 0.25 + 2 * (20 - 30)^2; 3 -> 4 is natural
    assert p8[1, 0, 0] == z(0.25) + z(2) * z(100) and p8[2, 0, 0] == 0
    # the same frames in one bank utterance: both natural
    p8 = sref.joins(bank, [0, 6], p7, [0, 3], 3, 1, join_cost=0.25, join_weight=2.0).reshape(3, 8, 8)
    assert p8[1, 0, 0] == 0 and p8[2, 0, 0] == 0
    # s is the frame after fa where there is one: from slot 0 of frame 0 (fa = 2) to fb = 1 in one utterance: s = 3
    j = list(p7[1, 8:]).index(1)
    assert p8[1, 0, j] == z(0.25) + z(2) * z((30 - 10) ** 2)
    # the join is one multiplication and then one addition, each rounded
    p8 = sref.joins(rows([0.1, 0.4, 0.2]), [0, 3], np.array([[0] * 8 + [0] + [-1] * 7, [0] * 8 + [2] + [-1] * 7], np.float32), [0, 2], 3, 1,
                    join_cost=0.3, join_weight=0.7)
    t = z(0.4) - z(0.2)
    assert p8[1, 0] == z(0.3) + z(0.7) * (t * t) and p8.dtype == np.float32


def test_equal_accumulated_costs_keep_the_smaller_state():
    # two frames, three slots: every c and every J equal -> back pointer 0 and end state 0 everywhere
    p7 = np.full((2, 16), -1, np.float32); p7[:, :8] = sref.CAP
    p7[:, :3] = 1; p7[0, 8:11] = [4, 5, 6]; p7[1, 8:11] = [0, 2, 1]
    p8 = np.zeros((2, 64), np.float32); p8[1].reshape(8, 8)[:3, :3] = 0.5
    utt, pos, cost = sref.path(p7, p8, [0, 2], [0, 7])
    assert list(pos) == [4, 0] and list(utt) == [0, 0] and cost[0] == 2.5
    # a strictly smaller predecessor replaces; an equal one later does not
    P8 = p8[1].reshape(8, 8)
    P8[1, 0] = 0.25; P8[2, 0] = 0.25                                # into state 0: a = 1 and a = 2 tie below a = 0 -> a = 1
    utt, pos, cost = sref.path(p7, p8, [0, 2], [0, 7])
    assert list(pos) == [5, 0] and cost[0] == 2.25
    # the end state: the smallest of the least acc
    p7[1, :3] = [2, 1.75, 1.75]; P8[:] = 0; P8[:3, :3] = 0.5
    utt, pos, cost = sref.path(p7, p8, [0, 2], [0, 7])
    assert list(pos) == [4, 2] and cost[0] == 3.25
    # an absent slot is no predecessor and no end state, whatever its row holds
    p7[:, 2] = 0; p7[:, 10] = -1
    utt, pos, cost = sref.path(p7, p8, [0, 2], [0, 7])
    assert list(pos) == [4, 2] and cost[0] == 3.25


def test_an_utterance_without_frames_costs_nothing():
    utt, pos, cost, p7, p8 = sref.select(rows([1, 2]), [0, 0, 2, 2], rows([1, 2, 3]), [0, 3], 3, 1)
    assert list(cost) == [0, 0, 0] and list(pos) == [0, 1] and p7.shape == (2, 16) and p8.shape == (2, 64)


def test_skip_own_utterance():
    bank = rows([0, 1, 2, 0, 1, 2, 7])
    off = [0, 3, 6, 7]
    utt, pos, cost, p7, p8 = sref.select(bank, off, bank, off, 3, 1, skip_own=True)
    assert list(utt) == [1, 1, 1, 0, 0, 0, 0] and list(pos) == [0, 1, 2, 0, 1, 2, 2]
    assert np.all(p7[:6, 12:15] == -1) and np.all(p7[6, 14:] == -1)  # n_u = 4, 4 and 6
    utt, pos, cost, p7, p8 = sref.select(bank, off, bank, off, 3, 1)
    assert list(sref.flat(utt, pos, off)) == [0, 1, 2, 0, 1, 2, 6] and np.all(cost == 0)   # an earlier identical row wins


# ---------------------------------------------------------------- quality
def make_bank(seed, nfrm=(60, 45, 70, 52), dim=30, cols=24):
    """smooth trajectories (align_reference.make), one per bank utterance, in columns 3 ... 3 + cols"""
    code = np.zeros((sum(nfrm), dim), np.float32)
    at = 0
    for u, n in enumerate(nfrm):
        code[at:at + n, 3:3 + cols] = aref.make(100 * seed + u, n, n, cols, 0.3)[0]; at += n
    return code, sref.offsets(nfrm)


def join_cost_of(bank):
    """a join_cost above anything the spectral term of a join can be (twice the largest c between two bank frames, weight
    1): a path with k joins costs at least k x join_cost, the true one at most one join_cost, one spectral term and the
    noise, so a second join never pays -- where the path joins is then decided by the distances alone"""
    return 2.0 * float(sref.cost(bank, bank, 3, 24).max())


@pytest.mark.parametrize("seed", range(4))
def test_a_noisy_stretch_of_the_bank_comes_back(seed):
    bank, off = make_bank(seed)
    rng = np.random.default_rng(seed)
    spread = float(bank[:, 3:27].std())
    p, m = 11 + seed, 30
    want = off[2] + p + np.arange(m + 1)
    tgt = bank[want].copy()
    tgt[:, 3:27] += (0.01 * spread * rng.standard_normal((m + 1, 24))).astype(np.float32)
    utt, pos, cost, p7, p8 = sref.select(tgt, [0, m + 1], bank, off, 3, 24, join_cost=join_cost_of(bank))
    assert np.array_equal(sref.flat(utt, pos, off), want) and np.all(utt == 2)
    assert np.array_equal(pos, (p + np.arange(m + 1)).astype(np.float32)) and pos.dtype == np.float32 and utt.dtype == np.int32


@pytest.mark.parametrize("seed", range(4))
def test_two_stretches_come_back_with_one_join(seed):
    bank, off = make_bank(seed)
    rng = np.random.default_rng(seed + 10)
    spread = float(bank[:, 3:27].std())
    want = np.concatenate([off[0] + 5 + np.arange(25), off[3] + 20 + np.arange(18)])
    tgt = bank[want].copy()
    tgt[:, 3:27] += (0.01 * spread * rng.standard_normal((len(want), 24))).astype(np.float32)
    utt, pos, cost, p7, p8 = sref.select(tgt, [0, len(want)], bank, off, 3, 24, join_cost=join_cost_of(bank))
    got = sref.flat(utt, pos, off)
    assert np.array_equal(got, want)
    assert int(np.count_nonzero(np.diff(got) != 1)) == 1 and list(np.unique(utt)) == [0, 3]


# ---------------------------------------------------------------- float32 against float64
_cases = {}


def gen(shape, seed, dim=72):
    """continuous random vectors (normal x 3): (target CODE, target offsets, bank CODE, bank offsets)"""
    rng = np.random.default_rng(1000 + seed)
    nt, nb = shape
    ct = (rng.standard_normal((sum(nt), dim)) * 3).astype(np.float32)
    cb = (rng.standard_normal((sum(nb), dim)) * 3).astype(np.float32)
    return ct, sref.offsets(nt), cb, sref.offsets(nb)


def case(k, seed):
    """(float32 chain, float64 chain) of one generated case, each (utt, pos, cost); computed once"""
    key = (k, seed)
    if key not in _cases:
        ct, to, cb, bo = gen(SHAPES[k], seed)
        _cases[key] = (sref.select(ct, to, cb, bo, **OPTS)[:3], sref.select(ct, to, cb, bo, dtype=np.float64, **OPTS)[:3])
    return _cases[key]


def test_float32_against_float64():
    differ = total = 0
    worst = 0.0
    for k in range(len(SHAPES)):
        for seed in SEEDS:
            (u32, p32, c32), (u64, p64, c64) = case(k, seed)
            assert c32.dtype == np.float32 and c64.dtype == np.float64
            d = int(np.count_nonzero((u32 != u64) | (p32 != p64)))
            assert d <= DIFFER_CAP * len(u32), (k, seed, d)         # every case on its own stays within the cap
            differ += d; total += len(u32)
            live = c64 > 0
            worst = max(worst, float(np.max(np.abs(c32[live].astype(np.float64) - c64[live]) / c64[live])))
    print("float32 against float64: %d of %d frames differ, cost within %.2g relative" % (differ, total, worst))
    assert total == 6 * (106 + 131 + 183)
    assert differ <= DIFFER_CAP * total
    assert worst <= COST_REL
