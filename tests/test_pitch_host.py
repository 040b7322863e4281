"""CPU-side checks of the pitch and formant edit (llsm_gpu_batch_pitch_formant): the symbol is declared, listed and
exported, a NULL batch is refused with a message, and the binding expands scalar, per-utterance and per-frame ratios to
the per-frame float32 arrays the C API takes."""
import os
import re

import numpy as np
import pytest

import libllsm2_amd as llsm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pitch_formant_is_declared_listed_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llsm_gpu.h")).read(), flags=re.S)
    assert re.search(r"\bllsm_gpu_batch_pitch_formant\s*\(", txt)
    assert re.search(r"\bLLSM_GPU_WARP_PSD\s*=\s*1\b", txt)
    assert "llsm_gpu_batch_pitch_formant" in llsm.EXPORTS
    assert hasattr(llsm.load(), "llsm_gpu_batch_pitch_formant")
    assert llsm.WARP_PSD == 1


def test_pitch_formant_refuses_a_null_batch_with_a_message():
    L = llsm.load()
    r = np.full(4, 1.5, np.float32)
    for args in ((None, None, 0), (r.ctypes.data_as(llsm.P_fp), None, 0), (None, r.ctypes.data_as(llsm.P_fp), 1)):
        assert L.llsm_gpu_batch_pitch_formant(None, *args) == -1
        msg = L.llsm_gpu_last_error().decode()
        assert msg.startswith("llsm_gpu_batch_pitch_formant:") and "NULL" in msg, msg


NFRM = np.array([3, 1, 4, 2], np.int32)


def test_ratio_none_stays_none():
    assert llsm.per_frame_ratio(None, NFRM) is None


@pytest.mark.parametrize("v", [1.5, np.float32(0.7), np.float64(2.0), 1, np.array(1.25)])
def test_scalar_ratio_covers_every_frame(v):
    got = llsm.per_frame_ratio(v, NFRM)
    assert got.dtype == np.float32 and got.shape == (10,)
    assert np.array_equal(got, np.full(10, np.float32(v)))


def test_per_utterance_ratio_repeats_over_each_utterance():
    got = llsm.per_frame_ratio([1.5, 0.5, 2.0, 0.75], NFRM)
    want = np.array([1.5] * 3 + [0.5] + [2.0] * 4 + [0.75] * 2, np.float32)
    assert got.dtype == np.float32 and np.array_equal(got, want)


def test_per_frame_ratio_is_taken_as_it_is():
    v = np.linspace(0.5, 2.0, 10)
    got = llsm.per_frame_ratio(v, NFRM)
    assert got.dtype == np.float32 and np.array_equal(got, v.astype(np.float32))
    # one frame per utterance: the two readings agree
    assert np.array_equal(llsm.per_frame_ratio([1.5, 2.0], [1, 1]), np.array([1.5, 2.0], np.float32))


@pytest.mark.parametrize("bad", [[1.0, 2.0], np.ones(9), np.ones((2, 5)), np.ones(11)])
def test_ratio_of_another_shape_is_rejected(bad):
    with pytest.raises(ValueError):
        llsm.per_frame_ratio(bad, NFRM)
