"""CPU-side checks of the cross-utterance splice (llsm_gpu_batch_splice): the symbol is declared, listed and exported, the
map struct of the binding matches the header's, and a NULL batch or a NULL map is refused with the prefixed message before
anything touches a device."""
import ctypes as C
import os
import re

import numpy as np

import libllsm2_amd as llsm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llsm_gpu.h")).read(), flags=re.S)


def test_splice_is_declared_listed_and_exported():
    txt = header()
    assert re.search(r"\bint\s+llsm_gpu_batch_splice\s*\(\s*llsm_gpu_batch\s*\*\s*dst\s*,\s*const\s+llsm_gpu_batch\s*\*\s*src\s*,"
                     r"\s*const\s+llsm_gpu_splice_map\s*\*\s*map\s*\)", txt)
    assert "llsm_gpu_batch_splice" in llsm.EXPORTS
    assert hasattr(llsm.load(), "llsm_gpu_batch_splice")
    assert callable(getattr(llsm.Batch, "splice"))


def test_the_binding_lays_the_map_out_as_the_header_does():
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*llsm_gpu_splice_map\s*;", header()).group(1)
    fields = re.findall(r"const\s+(int|FP_TYPE)\s*\*\s*(\w+)\s*;", body)
    assert [n for _, n in fields] == ["utt_a", "pos_a", "utt_b", "pos_b", "mix"]
    want = [(n, llsm.P_int if t == "int" else llsm.P_fp) for t, n in fields]
    assert list(llsm.SpliceMap._fields_) == want
    assert C.sizeof(llsm.SpliceMap) == 5 * C.sizeof(C.c_void_p)


def test_splice_refuses_null_batches_and_a_null_map_with_a_message():
    L = llsm.load()
    pos = np.zeros(4, np.float32)
    m = llsm.SpliceMap(None, pos.ctypes.data_as(llsm.P_fp), None, None, None)
    fake, fake2 = C.c_void_p(16), C.c_void_p(32)           # never dereferenced: a NULL argument is refused first
    for args, word in (((None, None, C.byref(m)), "NULL batch"), ((None, fake, C.byref(m)), "NULL batch"),
                       ((fake, None, C.byref(m)), "NULL batch"), ((None, None, None), "NULL"),
                       ((fake, fake2, None), "NULL map")):
        assert L.llsm_gpu_batch_splice(*args) == -1
        msg = L.llsm_gpu_last_error().decode()
        assert msg.startswith("llsm_gpu_batch_splice:") and word in msg, msg
