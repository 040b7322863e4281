"""CPU-side checks of the batch edits (llsm_gpu_batch_phasesync_rps / _phasepropagate / _retime): the symbols are
exported, the uniform retime map is the float32 map the header states, and NULL batches are refused with a message."""
import ctypes as C

import numpy as np
import pytest

import libllsm2_amd as llsm

NEW = ("llsm_gpu_batch_phasesync_rps", "llsm_gpu_batch_phasepropagate", "llsm_gpu_batch_retime",
       "llsm_gpu_retime_uniform_positions")


def test_edit_entry_points_are_exported():
    L = llsm.load()
    for s in NEW:
        assert s in llsm.EXPORTS, s
        assert hasattr(L, s), s


def uniform_map_np(ns, nd):
    i = np.arange(nd, dtype=np.float32)
    t = i * np.float32(ns) / np.float32(nd)                 # float32 throughout, left to right
    return np.minimum(t, np.float32(ns - 1)).astype(np.float32)


@pytest.mark.parametrize("ns,nd", [(200, 400), (200, 100), (200, 200), (1, 1), (1, 7), (7, 3), (13, 29), (199, 401),
                                   (1154, 2308), (3, 1000)])
def test_uniform_positions_match_a_float32_evaluation(ns, nd):
    got = llsm.retime_uniform_positions(ns, nd)
    want = uniform_map_np(ns, nd)
    assert got.dtype == np.float32 and got.shape == (nd,)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.flatnonzero(got != want)[:8]
    assert got[0] == 0 and got.max() <= ns - 1
    if ns == nd:
        assert np.array_equal(got, np.arange(nd, dtype=np.float32))     # the identity map is exact


def test_uniform_positions_zero_length_writes_nothing():
    L = llsm.load()
    buf = np.full(4, 7.0, np.float32)
    L.llsm_gpu_retime_uniform_positions(5, 0, buf.ctypes.data_as(llsm.P_fp))
    L.llsm_gpu_retime_uniform_positions(5, 3, None)                    # NULL output: a no-op, not a crash
    assert np.all(buf == 7.0)


def test_edits_refuse_null_batches_with_a_message():
    L = llsm.load()
    pos = np.zeros(4, np.float32)
    cases = [("phasesync_rps", lambda: L.llsm_gpu_batch_phasesync_rps(None, 0)),
             ("phasesync_rps", lambda: L.llsm_gpu_batch_phasesync_rps(None, 1)),
             ("phasepropagate", lambda: L.llsm_gpu_batch_phasepropagate(None, 1)),
             ("phasepropagate", lambda: L.llsm_gpu_batch_phasepropagate(None, -1)),
             ("retime", lambda: L.llsm_gpu_batch_retime(None, None, None, None)),
             ("retime", lambda: L.llsm_gpu_batch_retime(None, None, pos.ctypes.data_as(llsm.P_fp), None))]
    for name, call in cases:
        assert call() == -1, name
        msg = L.llsm_gpu_last_error().decode()
        assert name in msg and "NULL" in msg, (name, msg)
