"""CPU-side checks of the smoothing of parameter tracks around joins (llsm_gpu_batch_smooth, llsm_gpu_join_radii): both
symbols are declared, listed and exported with the header's constants; NULL arguments are refused with a message;
llsm_gpu_join_radii agrees with the brute-force restatement of its rule in tests/smooth_reference.py on random lists and at
every edge the rule has; and the binding expands a radius to the per-frame int32 array the C API takes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import libllsm2_amd as llsm
import smooth_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_int, P_fp = llsm.P_int, llsm.P_fp


def test_both_symbols_are_declared_listed_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llsm_gpu.h")).read(), flags=re.S)
    L = llsm.load()
    for name in ("llsm_gpu_batch_smooth", "llsm_gpu_join_radii"):
        assert re.search(r"\b" + name + r"\s*\(", txt), name
        assert name in llsm.EXPORTS, name
        assert hasattr(L, name), name
    want = dict(F0=1, RD=2, VTMAGN=4, PSD=8, EDC=16, ALL=31, MAX_RADIUS=32)
    for k, v in want.items():
        assert re.search(r"\bLLSM_GPU_SMOOTH_%s\s*=\s*%d\b" % (k, v), txt), k
        assert getattr(llsm, "SMOOTH_" + k) == v, k
    assert (ref.F0, ref.RD, ref.VTMAGN, ref.PSD, ref.EDC, ref.ALL, ref.MAX_RADIUS) == (1, 2, 4, 8, 16, 31, 32)


def test_smooth_refuses_null_arguments_with_a_message():
    L = llsm.load()
    r = np.zeros(4, np.int32)
    assert L.llsm_gpu_batch_smooth(None, r.ctypes.data_as(P_int), llsm.SMOOTH_ALL) == -1
    msg = L.llsm_gpu_last_error().decode()
    assert msg.startswith("llsm_gpu_batch_smooth:") and "NULL batch" in msg, msg
    assert L.llsm_gpu_batch_smooth(None, None, 0) == -1
    assert L.llsm_gpu_last_error().decode().startswith("llsm_gpu_batch_smooth:")
    # a NULL radius on a batch that exists: the check comes before anything touches the batch, so any non-NULL handle
    # shows it (the batch is not looked at before the radius is)
    fake = C.create_string_buffer(64)
    assert L.llsm_gpu_batch_smooth(C.cast(fake, C.c_void_p), None, llsm.SMOOTH_ALL) == -1
    msg = L.llsm_gpu_last_error().decode()
    assert msg.startswith("llsm_gpu_batch_smooth:") and "NULL radius" in msg, msg


# ------------------------------------------------------------------ llsm_gpu_join_radii
def c_join_radii(nfrm, pos, utt, reach):
    got, k = llsm.join_radii(nfrm, pos, utt, reach)
    assert got.dtype == np.int32 and got.shape == (int(np.sum(nfrm)),)
    return got, k


def random_lists(rng, nfrm, p_join=0.15):
    """index lists as select gives them: runs that continue by one frame, broken by hops to another utterance or place"""
    utt, pos = [], []
    for n in nfrm:
        u, p = int(rng.integers(0, 5)), float(rng.integers(0, 50))
        for i in range(int(n)):
            if i and rng.random() < p_join:
                kind = rng.integers(0, 3)
                if kind == 0:
                    u = (u + 1 + int(rng.integers(0, 4))) % 5              # another utterance, the position continues
                    p += 1
                elif kind == 1:
                    p += float(rng.choice([0.0, 2.0, -3.0, 7.0]))          # the same utterance, another place
                else:
                    u, p = int(rng.integers(0, 5)), float(rng.integers(0, 50))
            elif i:
                p += 1
            utt.append(u); pos.append(p)
    return np.array(utt, np.int32), np.array(pos, np.float32)


@pytest.mark.parametrize("reach", [0, 1, 3, 8, 32])
@pytest.mark.parametrize("with_utt", [True, False])
def test_join_radii_matches_the_rule_on_random_lists(reach, with_utt):
    rng = np.random.default_rng(100 + reach + with_utt)
    nfrm = np.array([1, 2, 3, 40, 0, 7, 70, 1, 200], np.int32)
    utt, pos = random_lists(rng, nfrm)
    u = utt if with_utt else None
    got, k = c_join_radii(nfrm, pos, u, reach)
    want, kw = ref.join_radii(nfrm, pos, u, reach)
    assert k == kw and np.array_equal(got, want), (k, kw, np.flatnonzero(got != want)[:8])
    assert k > 5 and got.max() == reach and got.min() == 0
    if with_utt:                                              # hops between utterances at continuing positions are joins
        _, k0 = c_join_radii(nfrm, pos, None, reach)
        assert k0 < k


def test_join_radii_at_the_edges_of_the_rule():
    # utterances of 1, 2 and 3 frames; a join at i = 1 and at i = n - 1; two joins closer than reach
    nfrm = np.array([1, 2, 3, 12, 12, 9], np.int32)
    pos = np.concatenate([[5], [5, 9], [1, 2, 7],
                          [0, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30],        # a join at i = 1
                          [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 40],                 # a join at i = n - 1
                          [0, 1, 2, 10, 11, 12, 30, 31, 32]]).astype(np.float32)  # joins at 3 and 6, closer than reach
    for reach in (0, 1, 4, 32):
        got, k = c_join_radii(nfrm, pos, None, reach)
        want, kw = ref.join_radii(nfrm, pos, None, reach)
        assert k == kw == 6 and np.array_equal(got, want), (reach, got, want)
    got, _ = c_join_radii(nfrm, pos, None, 4)
    assert got[0] == 0                                                            # one frame: no join
    assert list(got[1:3]) == [4, 4] and list(got[3:6]) == [3, 4, 4]
    assert list(got[6:18]) == [4, 4, 3, 2, 1, 0, 0, 0, 0, 0, 0, 0]
    assert list(got[18:30]) == [0, 0, 0, 0, 0, 0, 0, 1, 2, 3, 4, 4]
    assert list(got[30:39]) == [2, 3, 4, 4, 3, 4, 4, 3, 2]


def test_only_a_step_of_exactly_one_frame_is_a_continuation():
    # positions that continue by 1, by 0, by 2 and by 1 + 2^-20 (float32 holds 12 + 2^-20 exactly)
    pos = np.array([8, 9, 9, 11, 12 + 2.0 ** -20, 13 + 2.0 ** -20], np.float32)
    assert pos[4] != np.float32(12) and pos[4] - pos[3] != 1
    got, k = c_join_radii([6], pos, None, 1)
    assert k == 3 and list(got) == [0, 1, 1, 1, 1, 0]                  # joins at i = 2, 3 and 4; 1 and 5 continue
    want, kw = ref.join_radii([6], pos, None, 1)
    assert kw == 3 and np.array_equal(got, want)
    # a change of utterance alone is a join; utt_a NULL reads the same list as one recording
    utt = np.array([0, 0, 1, 1], np.int32)
    pos = np.array([3, 4, 5, 6], np.float32)
    assert c_join_radii([4], pos, utt, 2)[1] == 1 and c_join_radii([4], pos, None, 2)[1] == 0
    assert list(c_join_radii([4], pos, utt, 2)[0]) == [1, 2, 2, 1]
    assert list(c_join_radii([4], pos, None, 2)[0]) == [0, 0, 0, 0]
    # large positions: the sum is formed in float32 (2^24 + 1 is 2^24 there, so an equal position "continues")
    big = np.array([2.0 ** 24, 2.0 ** 24], np.float32)
    assert c_join_radii([2], big, None, 2)[1] == ref.join_radii([2], big, None, 2)[1] == 0


def test_join_radii_refusals():
    L = llsm.load()
    n = np.array([3], np.int32); pos = np.array([0, 1, 5], np.float32); rad = np.full(3, -7, np.int32)
    pn, pp, pr = n.ctypes.data_as(P_int), pos.ctypes.data_as(P_fp), rad.ctypes.data_as(P_int)
    cases = {"NULL nfrm": (1, None, None, pp, 2, pr), "NULL pos_a": (1, pn, None, None, 2, pr),
             "NULL radius": (1, pn, None, pp, 2, None), "n_utt": (-1, pn, None, pp, 2, pr),
             "reach = -1": (1, pn, None, pp, -1, pr), "reach = 33": (1, pn, None, pp, 33, pr)}
    for needle, args in cases.items():
        assert L.llsm_gpu_join_radii(*args) == -1, needle
        msg = L.llsm_gpu_last_error().decode()
        assert msg.startswith("llsm_gpu_join_radii:") and needle in msg, (needle, msg)
        assert np.all(rad == -7), needle
    neg = np.array([2, -1], np.int32)
    assert L.llsm_gpu_join_radii(2, neg.ctypes.data_as(P_int), None, pp, 2, pr) == -1
    assert "nfrm[1]" in L.llsm_gpu_last_error().decode() and np.all(rad == -7)
    with pytest.raises(llsm.LlsmError):
        llsm.join_radii([3], pos, None, 33)
    assert L.llsm_gpu_join_radii(1, pn, None, pp, 32, pr) == 1 and list(rad) == [31, 32, 32]
    assert L.llsm_gpu_join_radii(0, pn, None, pp, 2, pr) == 0


# ------------------------------------------------------------------ Batch.smooth's radius
def test_scalar_radius_covers_every_frame():
    for v in (3, np.int64(3), np.array(3), 3.0):
        got = llsm.per_frame_radius(v, 10)
        assert got.dtype == np.int32 and np.array_equal(got, np.full(10, 3, np.int32))


def test_per_frame_radius_is_taken_as_it_is():
    v = np.arange(10) % 4
    got = llsm.per_frame_radius(v, 10)
    assert got.dtype == np.int32 and got.flags.c_contiguous and np.array_equal(got, v)
    assert np.array_equal(llsm.per_frame_radius(list(v), 10), v)


@pytest.mark.parametrize("bad", [[1, 2], np.ones(9, np.int32), np.ones((2, 5), np.int32), np.ones(11, np.int32), 2.5])
def test_radius_of_another_shape_is_rejected(bad):
    with pytest.raises(ValueError):
        llsm.per_frame_radius(bad, 10)


def test_batch_smooth_checks_the_shape_before_it_calls_the_library():
    class Layout:
        total_frames = 10
    b = llsm.Batch.__new__(llsm.Batch)                         # no device: the shape is refused before the C call
    b.layout, b.L, b.h = Layout(), None, None
    with pytest.raises(ValueError):
        b.smooth(np.ones(9, np.int32))
    with pytest.raises(ValueError):
        b.smooth(np.ones((10, 1), np.int32), llsm.SMOOTH_F0)
