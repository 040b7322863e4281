"""CPU-side checks of the C-ABI library: it loads without a GPU, exports every
symbol include/*.h declares, refuses to compute without a device, and its
index plan agrees bit-for-bit with the oracle's."""
import os
import re

import numpy as np
import pytest

import libllsm2_amd as llsm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    syms = set()
    for h in ("llsm.h", "llsmrt.h", "llsm_gpu.h", "dsputils.h", "llsmutils.h"):
        txt = open(os.path.join(ROOT, "include", h)).read()
        txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
        txt = re.sub(r"#define[^\n]*(\\\n[^\n]*)*", "", txt)
        for m in re.finditer(r"\b(llsm_[a-z0-9_]+)\s*\(", txt):
            syms.add(m.group(1))
    return syms


def test_library_exports_every_declared_symbol():
    L = llsm.load()
    decl = declared_symbols()
    assert "llsm_analyze" in decl and "llsm_rtsynth_buffer_feed" in decl and "llsm_gpu_batch_analyze" in decl
    missing = sorted(s for s in decl if not hasattr(L, s))
    assert not missing, missing
    assert set(llsm.EXPORTS) <= decl | {"llsm_container_attach_"}


def test_no_cpu_fallback_without_device():
    L = llsm.load()
    if L.llsm_gpu_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(llsm.LlsmError):
        llsm.Context(0)
    import ctypes as C
    ao = llsm.make_aoptions()
    x = np.zeros(1000, np.float32); f0 = np.zeros(4, np.float32)
    ch = L.llsm_analyze(C.byref(ao), x.ctypes.data_as(llsm.P_fp), 1000, 44100.0, f0.ctypes.data_as(llsm.P_fp), 4, None)
    assert not bool(ch)
    assert b"no HIP device" in L.llsm_gpu_last_error()


def test_index_plan_matches_oracle(o32):
    L = llsm.load()
    ol = o32.lib
    for thop, fs in ((0.005, 44100.0), (128 / 44100.0, 44100.0), (100.5 / 44100.0, 44100.0),
                     (0.005, 48000.0), (0.01, 16000.0), (0.004, 22050.0)):
        thop = float(np.float32(thop))
        for i in range(0, 2500):
            assert L.llsm_gpu_plan_index(0, i, 0, 0, thop, fs, 4) == ol.o_idx_center(i, thop, fs)
            assert L.llsm_gpu_plan_index(5, i, 0, 0, thop, fs, 4) == ol.o_idx_ny(i, thop, fs)
            for j in (0, 1, 77, 300):
                assert L.llsm_gpu_plan_index(8, i, j, 0, thop, fs, 4) == ol.o_idx_env_ola(i, j, thop, fs)
        for w, fn in ((1, ol.o_idx_nwin_sin), (2, ol.o_idx_nwin_env), (3, ol.o_idx_nwin_filt), (4, ol.o_idx_nwin_psd)):
            assert L.llsm_gpu_plan_index(w, 0, 0, 0, thop, fs, 4) == fn(thop, fs)
        for f0 in np.linspace(35, 900, 800).astype(np.float32):
            f0 = float(f0)
            assert L.llsm_gpu_plan_index(6, 0, 0, f0, thop, fs, 4) == ol.o_idx_hwin(f0, fs, 4)
            assert L.llsm_gpu_plan_index(7, 100, 0, f0, thop, fs, 4) == ol.o_idx_nhar(f0, fs, 100)
            assert L.llsm_gpu_plan_index(9, 0, 0, f0, thop, fs, 4) == ol.o_idx_dcwin(f0, thop, fs)
            assert L.llsm_gpu_plan_index(10, 882, 0, f0, thop, fs, 4) == ol.o_idx_spgmwin(f0, fs, 882)


def test_stretch_index_closed_form(o64):
    """plan.h stretch_index == stretch_stationary_noise (dsputils.c:363-383) on a ramp."""
    L = llsm.load()
    for nx, ny in ((20000, 44321), (20000, 20000), (20000, 20100), (20000, 39872), (20000, 39873),
                   (20000, 59744), (20000, 59745), (5000, 5000), (20000, 147862)):
        ramp = np.arange(nx + 128, dtype=np.float64)
        ref = o64.bandlimited_noise  # noqa: F841  (documenting the caller)
        # reference tiling of an arbitrary template, re-stated in numpy
        y = np.zeros(ny); y[: min(nx, ny)] = ramp[: min(nx, ny)]
        if ny > nx:
            head = nx
            done = False
            while not done:
                for i in range(128):
                    r = i / 128.0
                    y[head - 128 + i] = (y[head - 128 + i] * (1 - r) + ramp[i] * r) / np.sqrt(2 * r * (r - 1) + 1)
                for i in range(nx - 128):
                    if head + i >= ny:
                        done = True
                        break
                    y[head + i] = ramp[i + 128]
                head += nx - 128
        got = np.zeros(ny)
        for p in list(range(0, ny, 97)) + list(range(max(0, ny - 300), ny)) + list(range(nx - 200, min(ny, nx + 200))):
            a = L.llsm_gpu_plan_index(11, p, nx, float(ny), 0, 0, 0)
            b = L.llsm_gpu_plan_index(12, p, nx, float(ny), 0, 0, 0)
            v = ramp[a]
            if b >= 0:
                r = b / 128.0
                v = (v * (1 - r) + ramp[b] * r) / np.sqrt(2 * r * (r - 1) + 1)
            got[p] = v
            assert abs(v - y[p]) < 1e-9 * max(1, abs(y[p])), (nx, ny, p, v, y[p])


def test_every_function_of_the_reference_headers_is_provided():
    """Drop-in completeness: every llsm_* function that the reference's five installed headers (makefile:132-135)
    declare is an exported symbol of the library or a header-inline function of include/*.h.  The names are read
    from tests/golden/ref_header_functions.txt (tests/golden/make_ref_fixtures.py)."""
    import re
    import subprocess
    heads = ["llsm.h", "llsmrt.h", "dsputils.h", "llsmutils.h", "buffer.h"]
    names = set(open(os.path.join(ROOT, "tests", "golden", "ref_header_functions.txt")).read().split())
    out = subprocess.run(["nm", "-D", "--defined-only", llsm.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    ours = "".join(open(os.path.join(ROOT, "include", h)).read() for h in heads)
    missing = sorted(n for n in names if n not in exported and not re.search(r"\b" + n + r"\s*\(", ours))
    assert len(names) > 100 and not missing, missing
