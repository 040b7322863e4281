"""Host side of llsm_gpu_batch_track_f0 (no GPU): the default track options, the refusals of llsm_gpu_f0_track_check, and the
numpy restatement of rules T1 - T5 (tests/f0_track_reference.py) on its own: what the path search buys over the
frame-by-frame estimator (tests/f0_reference.py) on the "trap" signals, and that it costs nothing on ordinary ones.

"gross" = a frame voiced on both sides whose F0 is more than 20 % from the true one.  Measured: trap(0..2) tracker 0, 0, 0
gross frames, estimator 19, 19, 21 (of about 100 voiced); make_speechlike(0, 1) tracker 0 gross, voicing differs from the
generator on 4 and 5 of 90 frames (estimator 5 and 6); golden WAVs 601 of 1 154 and 1 285 of 1 739 frames voiced."""
import ctypes as C

import numpy as np
import pytest

import libllsm2_amd as llsm
import f0_reference as ref
import f0_track_reference as tref
from conftest import make_speechlike

FS = 44100.0
THOP = np.float32(0.005)


def test_default_options():
    o = llsm.F0TrackOptions()
    llsm.load().llsm_gpu_f0_track_default_options(C.byref(o))
    d = tref.track_options()
    assert set(d) == {k for k, _ in llsm.F0TrackOptions._fields_}
    assert all(getattr(o, k) == float(d[k]) for k in d)
    assert [float(np.float32(v)) for v in (0.5, 0.2, 0.05, 0.5, 0.02)] == \
        [o.cand_threshold, o.unvoiced_cost, o.switch_cost, o.jump_cost, o.octave_cost]
    m = llsm.make_f0_track_options(jump_cost=1.0)
    assert m.jump_cost == 1.0 and m.switch_cost == o.switch_cost
    with pytest.raises(TypeError):
        llsm.make_f0_track_options(threshold=0.1)


nan, inf = float("nan"), float("inf")
REFUSED = [dict(cand_threshold=nan), dict(unvoiced_cost=nan), dict(switch_cost=nan), dict(jump_cost=nan), dict(octave_cost=nan),
           dict(cand_threshold=inf), dict(unvoiced_cost=inf), dict(switch_cost=inf), dict(jump_cost=inf), dict(octave_cost=inf),
           dict(unvoiced_cost=-inf),
           dict(cand_threshold=0.0), dict(cand_threshold=-0.5), dict(cand_threshold=1.0001),
           dict(unvoiced_cost=-0.1), dict(switch_cost=-0.1), dict(jump_cost=-1e-6), dict(octave_cost=-1.0)]


@pytest.mark.parametrize("kw", REFUSED, ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()))
def test_check_refusals(kw):
    L = llsm.load()
    o = llsm.make_f0_track_options(**kw)
    assert L.llsm_gpu_f0_track_check(C.byref(o)) == -1
    assert L.llsm_gpu_last_error().decode().startswith("llsm_gpu_batch_track_f0:")


def test_check_accepts_edges_and_null():
    L = llsm.load()
    assert L.llsm_gpu_f0_track_check(None) == 0
    for kw in (dict(), dict(cand_threshold=1.0), dict(unvoiced_cost=0.0, switch_cost=0.0, jump_cost=0.0, octave_cost=0.0),
               dict(cand_threshold=1e-6)):
        o = llsm.make_f0_track_options(**kw)
        assert L.llsm_gpu_f0_track_check(C.byref(o)) == 0, kw


def test_track_refuses_null_batch():
    L = llsm.load()
    assert L.llsm_gpu_batch_track_f0(None, None, None) == -1
    assert L.llsm_gpu_last_error().decode().startswith("llsm_gpu_batch_track_f0:")


@pytest.mark.parametrize("u", [0, 1, 2])
def test_trap(u):
    x, true = tref.trap(u)
    assert len(true) == 120 and len(x) == int(0.6 * FS)
    assert np.all(true[:8] == 0) and np.all(true[-8:] == 0) and np.all(true[8:-8] > 0)
    row = tref.track(x, FS, len(true), THOP)[0]
    est = ref.estimate(x, FS, len(true), THOP)[0]
    got, base = tref.gross_errors(row, true), tref.gross_errors(est, true)
    print("trap(%d): tracker %d gross frames, estimator %d" % (u, got, base))
    assert row.dtype == np.float32
    assert got <= 2
    assert base >= 15


@pytest.mark.parametrize("u", [0, 1])
def test_speechlike(u):
    x, true = make_speechlike(u, nx=int(0.45 * FS))
    assert len(true) == 90
    row = tref.track(x, FS, 90, THOP)[0]
    est = ref.estimate(x, FS, 90, THOP)[0]
    gross = tref.gross_errors(row, true)
    voicing, voicing_est = int(np.count_nonzero((row > 0) != (true > 0))), int(np.count_nonzero((est > 0) != (true > 0)))
    print("make_speechlike(%d): %d gross, voicing differs on %d (estimator %d)" % (u, gross, voicing, voicing_est))
    assert gross == 0
    assert voicing <= 6


@pytest.mark.parametrize("name,voiced", [("arctic_a0001", 601), ("are-you-ready", 1285)])
def test_golden_voiced_share(name, voiced):
    x, fs = ref.read_wav(name)
    nfrm = len(x) // 128
    row, cand, _, gated = tref.track(x, fs, nfrm, np.float32(128.0 / 44100.0))
    got = int(np.count_nonzero(row))
    print("%s: %d of %d frames voiced; candidates per frame %s" % (name, got, nfrm, np.bincount(cand[3], minlength=8)))
    assert abs(got - voiced) <= 0.02 * voiced
    assert np.all(row[gated] == 0)
    assert np.all(cand[3][gated] == 0)


def test_candidates_and_viterbi_by_hand():
    """a plane written by hand: the order of the slots, the tie between equal dips, the zeros, and a path that pays a
    switch rather than an octave"""
    z = np.float32
    lmin, lmax, fs = 4, 40, 8000.0
    cm = np.ones((3, lmax + 1), np.float32)
    cm[0, [9, 10, 11]] = [0.6, 0.30, 0.6]              # one dip at 10
    cm[0, [19, 20, 21]] = [0.5, 0.10, 0.10]            # a flat bottom: 20 counts (<= on the right), 21 does not (not < left)
    cm[1, [10, 20]] = [0.05, 0.05]                     # equal dips: the smaller lag first
    cm[1, 30] = 0.55                                   # above cand_threshold
    cm[2, 20] = 0.1                                    # gated below
    f0, cost, l2, n = tref.candidates(cm, np.array([False, False, True]), fs, lmin, lmax)
    assert list(n) == [2, 2, 0]
    assert np.all(l2[:, 7] == z(np.log2(8000.0 / 4))) and np.all(f0[:, 7] == 0) and np.all(cost[:, 7] == 0)
    assert list(cost[0, :3]) == [z(0.10), z(0.30), 0] and f0[0, 0] < 8000.0 / 20 and f0[0, 1] == z(800.0)
    assert list(cost[1, :3]) == [z(0.05), z(0.05), 0] and list(f0[1, :3]) == [z(800.0), z(400.0), 0]
    assert np.all(f0[2] == 0) and np.all(cost[2] == 0) and np.all(l2[2, :7] == 0)
    row = tref.viterbi(f0, cost, l2, n, l2[0, 7])
    # frame 0 takes its lowest dip (about 400 Hz); frame 1 stays there though 800 Hz comes first among equals
    assert row[0] == f0[0, 0] and row[1] == z(400.0) and row[2] == 0
    assert len(tref.viterbi(f0[:0], cost[:0], l2[:0], n[:0], l2[0, 7])) == 0
    assert tref.viterbi(f0[:1], cost[:1], l2[:1], n[:1], l2[0, 7])[0] == f0[0, 0]
