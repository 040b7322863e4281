"""Host side of llsm_gpu_batch_select_chain (no GPU): the symbol and its refusal of a NULL batch, and the numpy
restatement of rules C1 - C6 (tests/select_chain_reference.py) on its own: cases written by hand (a successor that is
also a near frame, a chain that reaches the end of its bank utterance, a pool of more than eight, banks below, at and
above K = 8 frames, NaN and infinite rows, infinite accumulated costs, an utterance without frames, skip_own_utterance),
the consequences P1 - P3 of the rules against tests/select_reference.py, the quality the rules exist for, and float32
against the same code in float64.

Measured with the generated cases of tests/test_select_host.py (vectors normal x 3 in 24 columns, join_cost 1, SEEDS x
SHAPES): the float32 chain differs from the float64 chain on 0 of 2 520 frames, cost agrees to 4.2e-7 relative (printed
by the test).  Quality (20 renditions of one random walk, the target a noisy stretch of one of them, seeds 0 ... 3):
llsm_gpu_batch_select's rules pay 7, 4, 5 and 8 joins at costs of 1.3e4 ... 2.6e4; these rules return one utterance at
positions 5 ... 54 without a join at costs of 104 ... 128."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import libllsm2_amd as llsm
import select_reference as sref
import select_chain_reference as cref
from test_align_host import DIFFER_CAP
from test_select_host import COST_REL, OPTS, SEEDS, SHAPES, gen, join_cost_of, rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
nan, inf = float("nan"), float("inf")
z = np.float32


# ---------------------------------------------------------------- the symbol
def test_the_symbol_is_declared_and_exported():
    txt = open(os.path.join(ROOT, "include", "llsm_gpu.h")).read()
    assert re.search(r"\bint\s+llsm_gpu_batch_select_chain\s*\(", txt)
    assert "llsm_gpu_batch_select_chain" in llsm.EXPORTS
    assert hasattr(llsm.load(), "llsm_gpu_batch_select_chain") and hasattr(llsm.Batch, "select_chain")


def test_select_chain_refuses_null_batch():
    L = llsm.load()
    utt = np.full(4, -7, np.int32); pos = np.full(4, -7, np.float32); cost = np.full(4, -7, np.float32)
    assert L.llsm_gpu_batch_select_chain(None, None, None, utt.ctypes.data_as(llsm.P_int), pos.ctypes.data_as(llsm.P_fp),
                                         cost.ctypes.data_as(llsm.P_fp)) == -1
    assert L.llsm_gpu_last_error().decode().startswith("llsm_gpu_batch_select_chain: NULL batch")
    assert np.all(utt == -7) and np.all(pos == -7) and np.all(cost == -7)
    # the shared check keeps the name of the call it was made for
    assert L.llsm_gpu_select_check(C.byref(llsm.make_select_options(first=-1)), 8, 2) == -1
    assert L.llsm_gpu_last_error().decode().startswith("llsm_gpu_batch_select:")


# ---------------------------------------------------------------- helpers
def run(tgt, t_off, bank, b_off, count=1, **kw):
    """the chain from CODE with everything every case must satisfy: path_from_planes gives it back, no frame holds a bank
    frame twice, the followers are successors of states of the frame before, and P1 and P2 against select_reference"""
    t_off = np.asarray(t_off, np.int64); b_off = np.asarray(b_off, np.int64)
    utt, pos, cost, p10, p11 = cref.chain(tgt, t_off, bank, b_off, 3, count, **kw)
    assert utt.dtype == np.int32 and pos.dtype == np.float32 and cost.dtype == np.float32
    assert p10.shape == (len(tgt), 32) and p11.shape == (len(tgt), 256) and p10.dtype == np.float32 and p11.dtype == np.float32
    u2, p2, c2, want = cref.path_from_planes(p10, p11, t_off, b_off)
    assert np.array_equal(utt, u2) and np.array_equal(pos, p2) and np.array_equal(cost, c2)
    assert np.array_equal(want, p10[:, 24:].astype(np.int64))
    assert not np.any(np.isnan(p10)) and not np.any(np.isnan(p11)) and not np.any(np.isnan(cost))
    f = p10[:, 16:].astype(np.int64)
    head = set(int(g) for g in t_off[:-1])
    for g in range(len(tgt)):
        there = f[g][f[g] >= 0]
        assert len(set(there)) == len(there) and np.all(there < len(bank)), g
        assert np.all(p10[g, :16][f[g] < 0] == cref.CAP)
        fol = f[g, 8:][f[g, 8:] >= 0]
        if g in head:
            assert len(fol) == 0 and not np.any(p11[g])
        else:
            assert set(fol - 1) <= set(f[g - 1])
    check_p1_p2(utt, pos, cost, p10, p11, sref.select(tgt, t_off, bank, b_off, 3, count, **kw))
    return utt, pos, cost, p10, p11


def check_p1_p2(utt, pos, cost, p10, p11, sel):
    su, sp, sc, p7, p8 = sel
    P11 = p11.reshape(-1, 16, 16)
    assert np.array_equal(p10[:, :8].view(np.uint32), p7[:, :8].view(np.uint32)) and np.array_equal(p10[:, 16:24], p7[:, 8:])   # P1
    assert np.array_equal(np.ascontiguousarray(P11[:, :8, :8]).view(np.uint32), p8.reshape(-1, 8, 8).view(np.uint32))
    assert np.all(cost <= sc), (cost, sc)                                                                                     # P2


# ---------------------------------------------------------------- cases written by hand
def test_a_successor_that_is_a_near_frame_is_not_duplicated():
    # one bank utterance 0 ... 11, the target walks along it: every successor but one is among the near frames
    utt, pos, cost, p10, p11 = run(rows([2, 3, 4]), [0, 3], rows(range(12)), [0, 12])
    assert list(p10[0, 16:24]) == [2, 1, 3, 0, 4, 5, 6, 7] and list(p10[0, 24:]) == [-1] * 8
    assert list(p10[1, 16:24]) == [3, 2, 4, 1, 5, 0, 6, 7]
    # the successors of frame 0's states are 3, 2, 4, 1, 5, 6, 7 and 8: only 8 is no near frame of frame 1
    assert list(p10[1, 24:]) == [8] + [-1] * 7 and p10[1, 8] == 25 and np.all(p10[1, 9:16] == cref.CAP)
    P = p11[1].reshape(16, 16)
    assert P[7, 8] == 0                                             # the follower from its own parent (slot 7: frame 7)
    assert P[0, 0] == 0 and P[0, 2] == z(1)                         # a near slot whose frame is s_a: 2 -> 3; and s = 3 against 4
    assert np.all(P[8:] == 0) and np.all(P[:, 9:] == 0)             # absent
    assert list(pos) == [2, 3, 4] and cost[0] == 0


def test_a_chain_that_reaches_the_end_of_its_utterance_vanishes():
    bank = rows([50, 60, 70] + list(range(10)))                     # utterances of 3 and 10 frames
    utt, pos, cost, p10, p11 = run(rows([50, 0, 0, 0]), [0, 4], bank, [0, 3, 13])
    f = p10[:, 16:].astype(int)
    assert list(f[0, :8]) == [0, 1, 2, 12, 11, 10, 9, 8]
    # frame 1: frames 2 and 12 end their utterances, the successors of 9 and 8 are near frames; the rest by acc
    assert list(f[1, :8]) == list(range(3, 11)) and list(f[1, 8:]) == [1, 2, 12, 11] + [-1] * 4
    assert list(p10[1, 8:12]) == [60 * 60, 70 * 70, 81, 64]
    # frame 2: the chains at 2 and 12 have no successor; 1 -> 2 and 11 -> 12 go on, and near frame 10 brings 11
    assert set(f[2, 8:]) == {2, 12, 11, -1} and set(f[3, 8:]) == {11, 12, -1}
    assert np.count_nonzero(f[2, 8:] >= 0) == 3 and np.count_nonzero(f[3, 8:] >= 0) == 2


def test_a_pool_of_more_than_eight_is_pruned_by_acc_then_a():
    # without join costs acc_i[j] = min(acc_{i-1}) + c_i[j]: the pool is ordered by the parents' own c
    bank = rows(range(40))
    tgt = rows([20] * 12)
    utt, pos, cost, p10, p11 = run(tgt, [0, 12], bank, [0, 40], join_cost=0.0, join_weight=0.0)
    f = p10[:, 16:].astype(int)
    assert np.all(f[:, :8] == [20, 19, 21, 18, 22, 17, 23, 16])
    for i in range(1, 9):                                           # one more follower per frame: 24, 25, ...
        assert list(f[i, 8:8 + i]) == list(range(24, 24 + i)) and np.all(f[i, 8 + i:] == -1), i
    for i in range(9, 12):                                          # nine in the pool: the parent of 32 has the largest acc
        assert list(f[i, 8:]) == list(range(24, 32)), i
    # equal acc everywhere: the pool is ordered by a alone
    const = rows([1] * 40)
    utt, pos, cost, p10, p11 = run(rows([1] * 12), [0, 12], const, [0, 40], join_cost=0.0)
    f = p10[:, 16:].astype(int)
    assert np.all(f[:, :8] == np.arange(8)) and np.all(cost == 0)
    for i in range(1, 12):
        k = min(i, 8)
        assert list(f[i, 8:8 + k]) == list(range(8, 8 + k)) and np.all(f[i, 8 + k:] == -1), i
    # rule C3 itself: (acc, a) ascending, infinities included, eight at the most
    f_prev = np.array([10, 20, 30, 40, 50, 60, 70, 80, 90, 100, 110, 120, -1, -1, -1, -1])
    acc = np.array([inf, 1, inf, 0, inf, 1, 5, inf, 2, inf, 0, inf, 0, 0, 0, 0], np.float32)
    b_end = np.full(200, 200)
    assert cref.followers(f_prev, acc, [31, 500], b_end) == [3, 10, 1, 5, 8, 6, 0, 4]   # (a = 2 -> 31 is a near frame)
    b_end[40] = 41                                                  # frame 40 ends its utterance
    assert cref.followers(f_prev, acc, [], b_end) == [10, 1, 5, 8, 6, 0, 2, 4]
    assert cref.followers(f_prev, np.full(16, inf, np.float32), [], b_end) == [0, 1, 2, 4, 5, 6, 7, 8]


@pytest.mark.parametrize("n", [1, 7, 8, 9])
def test_banks_below_at_and_above_k(n):
    rng = np.random.default_rng(n)
    bank = rows(rng.permutation(n) * 2.0)
    tgt = rows(rng.random(6) * 2 * n)
    utt, pos, cost, p10, p11 = run(tgt, [0, 2, 2, 6], bank, [0, n], join_cost=0.5)
    nu = min(8, n)
    f = p10[:, 16:]
    assert np.all(f[:, :nu] >= 0) and np.all(f[:, nu:8] == -1)
    assert np.all(f[:, 8:] == -1) if n <= 8 else np.all(f[:, 9:] == -1)   # nine frames: at most the one that is not near
    assert np.all(utt == 0) and np.all(pos < n) and cost.shape == (3,) and cost[1] == 0
    # two bank utterances of n frames: followers across the whole bank
    bank2 = rows(list(rng.permutation(n) * 2.0) + list(rng.permutation(n) * 2.0 + 1))
    run(tgt, [0, 2, 2, 6], bank2, [0, n, 2 * n], join_cost=0.5)


def test_nan_and_infinite_rows_on_either_side():
    bank = rows([2, nan, 7, inf, 3, 4, -inf, 5, 6, 8, 9, 1, 0, 11])
    for tgt in (rows([3, nan, 2, 9, inf, 4]), rows([nan] * 5), rows([1, 2, 3, 4, 5, 6, 7])):
        utt, pos, cost, p10, p11 = run(tgt, [0, len(tgt)], bank, [0, 5, 14], join_cost=1.0)
        assert np.all(np.isfinite(p10)) and np.all(np.isfinite(p11)) and np.all(np.isfinite(cost))
    utt, pos, cost, p10, p11 = run(rows([1, 2, 3]), [0, 3], rows([nan] * 12), [0, 12], join_cost=1.0)
    assert np.all(p10[:, :8] == cref.CAP) and list(p10[2, 24:26]) == [8, 9]


def test_a_weight_that_makes_acc_infinite():
    """join_weight 1e30 on a join distance at the cap is +infinity: such acc compare and tie like any others"""
    big = 1e20                                                      # (big - -big)^2 overflows: the cap
    bank = rows([big] * 12 + [-big] * 12)
    utt, pos, cost, p10, p11 = run(rows([big, -big, -big, -big]), [0, 4], bank, [0, 12, 24], join_weight=1e30)
    f = p10[:, 16:].astype(int)
    assert np.any(np.isinf(p11)) and cost[0] == z(1e30) + z(1e30) + z(1e30)   # the path stays on the followers: 0 + three caps
    # frame 1: the near slots are frames 12 ... 19, reached only through joins at the cap: their acc is +infinity; the
    # followers 1 ... 8 continue frame 0's states at acc 1e30.  Frame 2: nine in the pool, the one of infinite acc is last
    assert list(f[1]) == list(range(12, 20)) + list(range(1, 9))
    assert np.all(np.isinf(p11[1].reshape(16, 16)[:8, :8])) and np.all(p11[1].reshape(16, 16)[np.arange(8), 8 + np.arange(8)] == 0)
    assert list(f[2, 8:]) == list(range(2, 10))
    # a bank of NaN rows in utterances of three frames, every join at the cap
    utt, pos, cost, p10, p11 = run(rows([1, 2, 3, 4, 5]), [0, 5], rows([nan] * 18), [0, 3, 6, 9, 12, 15, 18], join_weight=1e30)
    assert np.any(np.isinf(p11)) and np.all(utt >= 0)


def test_an_utterance_without_frames_costs_nothing():
    utt, pos, cost, p10, p11 = run(rows([1, 2]), [0, 0, 2, 2], rows([1, 2, 3]), [0, 3])
    assert list(cost) == [0, 0, 0] and list(pos) == [0, 1] and p10.shape == (2, 32) and p11.shape == (2, 256)


def test_skip_own_utterance():
    rng = np.random.default_rng(3)
    nfrm = [12, 15, 12, 1]
    walk = np.cumsum(rng.standard_normal(15))
    bank = rows(np.concatenate([walk[:12] + 0.01, walk, walk[:12] - 0.01, [0.0]]))
    off = sref.offsets(nfrm)
    utt, pos, cost, p10, p11 = run(bank, off, bank, off, skip_own=True, join_cost=10.0)
    own = sref.frame_utt(off)
    f = p10[:, 16:].astype(int)
    assert np.all(utt != own)
    lo, hi = off[own][:, None], off[own + 1][:, None]
    assert np.all((f < 0) | (f < lo) | (f >= hi))                   # followers too: their parents were eligible
    assert np.any(f[:, 8:] >= 0)
    assert cref.joins_of(utt, pos, off, off)[0] == 0                # utterance 0 is rendered from one other rendition


# ---------------------------------------------------------------- P1 - P3 on generated cases
_cases = {}


def case(k, seed):
    """(float32 chain, float64 chain) of one generated case of tests/test_select_host.py, each (utt, pos, cost, plane 10,
    plane 11); computed once"""
    key = (k, seed)
    if key not in _cases:
        ct, to, cb, bo = gen(SHAPES[k], seed)
        _cases[key] = (cref.chain(ct, to, cb, bo, **OPTS), cref.chain(ct, to, cb, bo, dtype=np.float64, **OPTS))
    return _cases[key]


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_p1_p2_on_generated_cases(k):
    for seed in SEEDS:
        ct, to, cb, bo = gen(SHAPES[k], seed)
        utt, pos, cost, p10, p11 = case(k, seed)[0]
        check_p1_p2(utt, pos, cost, p10, p11, sref.select(ct, to, cb, bo, **OPTS))
        u2, p2, c2, want = cref.path_from_planes(p10, p11, to, bo)
        assert np.array_equal(utt, u2) and np.array_equal(pos, p2) and np.array_equal(cost, c2)
        assert np.array_equal(want, p10[:, 24:].astype(np.int64))
        if k < 2:
            assert np.any(p10[:, 24:] >= 0)                         # (a bank of nine frames has few successors that are not near)


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_p3_a_bank_of_single_frames(k):
    for seed in SEEDS:
        ct, to, cb, bo = gen(SHAPES[k], seed)
        bo = np.arange(len(cb) + 1)                                 # every bank frame an utterance of its own
        utt, pos, cost, p10, p11 = cref.chain(ct, to, cb, bo, **OPTS)
        su, sp, sc, p7, p8 = sref.select(ct, to, cb, bo, **OPTS)
        assert np.array_equal(utt, su) and np.array_equal(pos.view(np.uint32), sp.view(np.uint32))
        assert np.array_equal(cost.view(np.uint32), sc.view(np.uint32))
        assert np.all(p10[:, 24:] == -1) and np.all(p10[:, 8:16] == cref.CAP)
        assert not np.any(p11.reshape(-1, 16, 16)[:, 8:]) and not np.any(p11.reshape(-1, 16, 16)[:, :, 8:])


# ---------------------------------------------------------------- quality
def renditions(seed, n_utt=20, n=60, cols=24, dim=30):
    """a bank of n_utt renditions of one random walk (steps normal(0, 1)) with independent noise of sigma 0.1, and frames
    5 ... 54 of rendition 7 with noise of sigma 0.3 as the target: (target CODE, bank CODE, bank offsets)"""
    rng = np.random.default_rng(seed)
    walk = np.cumsum(rng.standard_normal((n, cols)), axis=0)
    bank = np.zeros((n_utt * n, dim), np.float32)
    for u in range(n_utt):
        bank[u * n:(u + 1) * n, 3:3 + cols] = walk + 0.1 * rng.standard_normal((n, cols))
    tgt = bank[7 * n + 5:7 * n + 55].copy()
    tgt[:, 3:3 + cols] += (0.3 * rng.standard_normal((50, cols))).astype(np.float32)
    return tgt, bank, sref.offsets([n] * n_utt)


@pytest.mark.parametrize("seed", range(4))
def test_one_rendition_carries_the_stretch(seed):
    tgt, bank, off = renditions(seed)
    o = dict(first=3, count=24, join_cost=join_cost_of(bank))
    su, sp, sc, _, _ = sref.select(tgt, [0, 50], bank, off, **o)
    utt, pos, cost, p10, p11 = cref.chain(tgt, [0, 50], bank, off, **o)
    print("seed %d: select %d joins at %.4g, chain %d joins at %.4g" %
          (seed, cref.joins_of(su, sp, [0, 50], off)[0], sc[0], cref.joins_of(utt, pos, [0, 50], off)[0], cost[0]))
    assert len(np.unique(utt)) == 1 and np.array_equal(pos, (5 + np.arange(50)).astype(np.float32))
    assert cref.joins_of(utt, pos, [0, 50], off)[0] == 0
    assert cref.joins_of(su, sp, [0, 50], off)[0] >= 1
    assert cost[0] < sc[0]


# ---------------------------------------------------------------- float32 against float64
def test_float32_against_float64():
    differ = total = 0
    worst = 0.0
    for k in range(len(SHAPES)):
        for seed in SEEDS:
            (u32, p32, c32, _, _), (u64, p64, c64, _, _) = case(k, seed)
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
