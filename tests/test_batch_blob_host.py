"""Export of a device-resident batch as chunk blobs (csrc/batch_blob.cpp, llsm_gpu.h): what can be checked without a
device -- the four symbols, llsm_blob_bytes against the sizes llsm_chunk_blob_size / llsm_chunk_to_blob give for chunks built
as tests/test_wire.py builds them, and the refusal of a NULL batch."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import libllsm2_amd as llsm
from test_wire import _bind, _make_chunk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["llsm_blob_bytes", "llsm_gpu_batch_blob_sizes", "llsm_gpu_batch_download_blobs",
           "llsm_gpu_batch_download_blob_block"]


def test_symbols_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "llsm_gpu.h")).read()
    L = llsm.load()
    dyn = subprocess.run(["nm", "-D", "--defined-only", llsm.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in llsm.EXPORTS, s
        assert re.search(r"\sT\s+%s$" % s, dyn, re.M), s
        assert getattr(L, s)


def _blob_of(L, ch):
    n = L.llsm_chunk_blob_size(ch)
    buf = (C.c_ubyte * n)()
    assert L.llsm_chunk_to_blob(ch, buf, n) == n
    return n, bytes(buf)


def _header(raw):
    """(nfrm, maxnhar, maxnhar_e, npsd, nchannel, nchanfreq, nspec, total_bytes) of a version-2 blob"""
    nfrm, mh, me, npsd, nch, ncf = struct.unpack_from("<6i", raw, 16)
    nspec = struct.unpack_from("<i", raw, 52)[0]
    total = struct.unpack_from("<Q", raw, 56)[0]
    return nfrm, mh, me, npsd, nch, ncf, nspec, total


def _check(L, ch):
    n, raw = _blob_of(L, ch)
    nfrm, mh, me, npsd, nch, ncf, nspec, total = _header(raw)
    assert total == n == len(raw)
    assert L.llsm_blob_bytes(nfrm, mh, me, npsd, nch, ncf, nspec) == n
    return nfrm, mh, me, nspec


def _plain_chunk(L, F, **kw):
    ao = llsm.make_aoptions(**kw)
    conf = L.llsm_aoptions_toconf(C.byref(ao), 22050.0)
    C.cast(L.llsm_container_get(conf, llsm.CONF_NFRM), llsm.P_int)[0] = F
    ch = L.llsm_create_chunk(conf, 1)
    L.llsm_delete_container(conf)
    return ch


def _add_layer1(L, ch, nspec=65):
    """layer-1 members by hand, as tests/test_wire.py attaches them"""
    vp = C.c_void_p
    L.llsm_container_attach_(ch.contents.conf, llsm.CONF_NSPEC, C.cast(L.llsm_create_int(nspec), vp),
                             C.cast(L.llsm_delete_int, vp), C.cast(L.llsm_copy_int, vp))
    nfrm = C.cast(L.llsm_container_get(ch.contents.conf, llsm.CONF_NFRM), llsm.P_int)[0]
    for i in range(nfrm):
        fr = ch.contents.frames[i]
        L.llsm_container_attach_(fr, llsm.FRAME_RD, C.cast(L.llsm_create_fp(0.5), vp), C.cast(L.llsm_delete_fp, vp),
                                 C.cast(L.llsm_copy_fp, vp))
        if C.cast(L.llsm_container_get(fr, llsm.FRAME_F0), llsm.P_fp)[0] > 0:
            hm = C.cast(L.llsm_container_get(fr, llsm.FRAME_HM), C.POINTER(llsm.HMFrame)).contents
            for idx, arr in ((llsm.FRAME_VTMAGN, L.llsm_create_fparray(nspec)), (llsm.FRAME_VSPHSE, L.llsm_create_fparray(hm.nhar + 1))):
                L.llsm_container_attach_(fr, idx, C.cast(arr, vp), C.cast(L.llsm_delete_fparray, vp), C.cast(L.llsm_copy_fparray, vp))


def test_blob_bytes_equals_the_serialiser():
    L = _bind(llsm.load())
    # analysis-shaped chunk, without and with layer-1 members (VSPHSE one longer than HM: it sets the row width)
    ch, _ = _make_chunk(L)
    nfrm, mh, me, nspec = _check(L, ch)
    assert (nfrm, mh, me, nspec) == (9, 12, 3, 0)
    _add_layer1(L, ch)
    assert _check(L, ch) == (9, 13, 3, 65)
    L.llsm_delete_chunk(ch)
    # odd shapes: array lengths that need the padding word
    ch, _ = _make_chunk(L, F=7, mh=5, me=1, npsd=15, nch=3, seed=2)
    _check(L, ch)
    L.llsm_delete_chunk(ch)
    # an empty chunk and an all-unvoiced one
    for F in (0, 5):
        ch = _plain_chunk(L, F)
        assert _check(L, ch) == (F, 0, 0, 0)
        L.llsm_delete_chunk(ch)
    # maxnhar_e = 0: envelope rows of width 1
    ch, _ = _make_chunk(L, me=0, seed=1)
    nfrm, mh, me, nspec = _check(L, ch)
    assert me == 0
    assert L.llsm_blob_bytes(nfrm, mh, 0, 16, 4, 3, 0) == L.llsm_blob_bytes(nfrm, mh, 1, 16, 4, 3, 0)
    L.llsm_delete_chunk(ch)
    # one channel: no band edges
    ch = _plain_chunk(L, 3, nchannel=1, chanfreq=[])
    _check(L, ch)
    L.llsm_delete_chunk(ch)
    assert L.llsm_blob_bytes(-1, 0, 0, 16, 4, 3, 0) == 0 and L.llsm_gpu_last_error()


def test_null_batch_is_refused_with_a_message():
    L = llsm.load()
    dst = np.full(64, 0xA5, np.uint8)
    ptrs = (C.c_void_p * 1)(dst.ctypes.data); caps = (C.c_size_t * 1)(64); offs = (C.c_size_t * 2)(7, 7)
    sizes = (C.c_size_t * 1)(7)
    for call, args in ((L.llsm_gpu_batch_blob_sizes, (None, 0, 1, sizes)),
                       (L.llsm_gpu_batch_download_blobs, (None, 0, 1, ptrs, caps)),
                       (L.llsm_gpu_batch_download_blob_block, (None, 0, 1, C.c_void_p(dst.ctypes.data), 64, offs))):
        assert call(*args) == -1
        assert b"NULL batch" in L.llsm_gpu_last_error()
    assert (dst == 0xA5).all() and sizes[0] == 7 and list(offs) == [7, 7]
