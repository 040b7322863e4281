"""CPU-side checks of the device-resident frame coder (llsm_gpu_batch_enable_coder / _coder_dimension / _encode /
_decode): the symbols are declared, listed and exported, the array enum grew by LLSM_GPU_CODE at its end with every
existing id unchanged, the binding's A_CODE matches, and without a batch the calls are refused with a message (there is
no CPU fallback: DESIGN.md section 1)."""
import os
import re

import libllsm2_amd as llsm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("llsm_gpu_batch_enable_coder", "llsm_gpu_batch_coder_dimension", "llsm_gpu_batch_encode", "llsm_gpu_batch_decode")
# the array ids as they were before the coder (llsm_gpu.h); hosts compiled against them must keep working
EXISTING = ("X", "F0", "NHAR", "AMPL", "PHSE", "PSD", "PSDRES", "EDC", "NHAR_E", "EENV_AMPL", "EENV_PHSE", "XRES", "Y", "YSIN",
            "YNOISE", "WHITE", "HAS_PSDRES", "RD", "VTMAGN", "VSPHSE", "NVSPHSE", "PBPSYN", "HAS_HM")


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llsm_gpu.h")).read(), flags=re.S)


def test_symbols_are_declared_listed_and_exported():
    txt, L = header(), llsm.load()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, txt), s
        assert s in llsm.EXPORTS, s
        assert hasattr(L, s), s


def test_array_ids_are_unchanged_and_code_is_23():
    m = re.search(r"enum\s*\{\s*LLSM_GPU_X\s*=\s*0\s*,(.*?)\}", header(), flags=re.S)
    assert m
    names = ["LLSM_GPU_X"] + [n.strip() for n in m.group(1).split(",") if n.strip()]
    ids = {n: i for i, n in enumerate(names)}
    for i, n in enumerate(EXISTING):
        assert ids["LLSM_GPU_" + n] == i, n
        assert getattr(llsm, "A_" + n) == i, n
    assert ids["LLSM_GPU_CODE"] == 23 and ids["LLSM_GPU_NARRAYS"] == 24
    assert llsm.A_CODE == 23 and llsm.A_NARRAYS == 24
    assert llsm.A_CODE not in llsm._INT_ARRAYS


def test_calls_without_a_batch_are_refused_with_a_message():
    L = llsm.load()
    for name, args in (("llsm_gpu_batch_enable_coder", (None, 64, 5)), ("llsm_gpu_batch_encode", (None,)),
                       ("llsm_gpu_batch_decode", (None, 1)), ("llsm_gpu_batch_decode", (None, 0))):
        assert getattr(L, name)(*args) == -1, name
        msg = L.llsm_gpu_last_error().decode()
        assert msg.startswith(name + ":") and "NULL" in msg, msg
    assert L.llsm_gpu_batch_coder_dimension(None) == 0
