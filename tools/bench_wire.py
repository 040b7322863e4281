"""Flat chunk wire format throughput: llsm_chunk_to_blob, llsm_blob_view (validation only),
llsm_blob_to_chunk and llsm_gpu_batch_upload_blob + use of the rows by a synthesis, for config-2 chunks.

    python tools/bench_wire.py [--utts 256] [--reps 5]
    python tools/bench_wire.py --download [--utts 1024] [--reps 5]

--download: the other direction, llsm_gpu_batch_download_blob_block / _download_blobs (blobs packed on the device,
DESIGN.md section 19) against the host path they replace, at the bench shape (--utts x 200 frames, 120 Hz) and the sweep
shape (F0 from 80 to 400 Hz over the utterances), without and with layer 1; one JSON line per case.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import libllsm2_amd as llsm  # noqa: E402
from conftest import FS, make_utterance  # noqa: E402


def download_case(L, ctx, name, U, f0_of, nfft, reps):
    """one batch analysed (and taken to layer 1 when nfft > 0), then exported every way; returns the result dict"""
    nfrm, nx = 200, 44100
    ao = llsm.make_aoptions(f0_refine=0)
    kinds = sorted({f0_of(u) for u in range(U)})
    wave = {f: make_utterance(k % 8, f) for k, f in enumerate(kinds)}
    b = llsm.Batch(ctx, ao, FS, [nx] * U, [nfrm] * U)
    b.upload(llsm.A_X, np.concatenate([wave[f0_of(u)] for u in range(U)]))
    b.upload(llsm.A_F0, np.concatenate([np.full(nfrm, f0_of(u), np.float32) for u in range(U)]))
    b.analyze()
    if nfft:
        b.tolayer1(nfft)
    ctx.sync()
    sizes = b.blob_sizes()
    total = sum((s + 15) // 16 * 16 for s in sizes)
    L.llsm_gpu_alloc_host.restype = C.c_void_p; L.llsm_gpu_alloc_host.argtypes = [C.c_size_t]
    L.llsm_gpu_free_host.argtypes = [C.c_void_p]
    p = L.llsm_gpu_alloc_host(total)
    assert p, "llsm_gpu_alloc_host"
    pinned = np.frombuffer((C.c_ubyte * total).from_address(p), dtype=np.uint8)
    words = [np.zeros((s + 7) // 8, np.uint64) for s in sizes]
    ptrs = (C.c_void_p * U)(*[w.ctypes.data for w in words]); caps = (C.c_size_t * U)(*sizes)
    t_blk, t_pg, t_k = [], [], []
    for it in range(reps + 1):
        ctx.set_profiling(True, only="k_blob_pack"); ctx.reset_profile()
        t0 = time.perf_counter()
        offs = b.download_blob_block(pinned)
        t1 = time.perf_counter()
        prof = ctx.profile()
        ctx.set_profiling(False)
        t2 = time.perf_counter()
        assert L.llsm_gpu_batch_download_blobs(b.h, 0, U, ptrs, caps) == 0, L.llsm_gpu_last_error()
        t3 = time.perf_counter()
        if it:
            t_blk.append(t1 - t0); t_pg.append(t3 - t2); t_k.append(prof["k_blob_pack"][0] * 1e-3)
    launches = prof["k_blob_pack"][1]
    for k in (0, U // 2, U - 1):                              # the two ways out agree
        assert np.array_equal(pinned[offs[k]:offs[k] + sizes[k]], words[k].view(np.uint8)[:sizes[k]])
    # the host path this replaces: rows down at the batch's widths, container trees, llsm_chunk_to_blob, trees deleted
    L.llsm_delete_chunks.argtypes = [C.POINTER(C.POINTER(llsm.Chunk)), C.c_int]
    L.llsm_delete_chunks.restype = None
    ids = list(b.PARAM_IDS) + (list(b.L1_IDS) if nfft else [])
    t_host, row_bytes = [], 0
    for it in range(2):
        t0 = time.perf_counter()
        rows = {aid: b.download(aid) for aid in ids}
        t1 = time.perf_counter()
        row_bytes = sum(r.nbytes for r in rows.values())
        v = llsm.FlatParams()
        v.maxnhar, v.maxnhar_e, v.npsd, v.nchannel = ao.maxnhar, ao.maxnhar_e, ao.npsd, ao.nchannel
        fpp = lambda aid: rows[aid].ctypes.data_as(llsm.P_fp); ipp = lambda aid: rows[aid].ctypes.data_as(llsm.P_int)
        v.f0, v.nhar, v.ampl, v.phse, v.psd, v.psdres = fpp(llsm.A_F0), ipp(llsm.A_NHAR), fpp(llsm.A_AMPL), fpp(llsm.A_PHSE), fpp(llsm.A_PSD), fpp(llsm.A_PSDRES)
        v.has_psdres, v.edc, v.nhar_e = ipp(llsm.A_HAS_PSDRES), fpp(llsm.A_EDC), ipp(llsm.A_NHAR_E)
        v.eenv_ampl, v.eenv_phse = fpp(llsm.A_EENV_AMPL), fpp(llsm.A_EENV_PHSE)
        if nfft:
            has_rd = np.ones(U * nfrm, np.int32)
            q = llsm.FlatL1()
            q.nspec, q.maxnhar = nfft // 2 + 1, ao.maxnhar
            q.rd, q.has_rd, q.vtmagn, q.vsphse = fpp(llsm.A_RD), has_rd.ctypes.data_as(llsm.P_int), fpp(llsm.A_VTMAGN), fpp(llsm.A_VSPHSE)
            q.nvsphse, q.pbpsyn, q.has_hm = ipp(llsm.A_NVSPHSE), ipp(llsm.A_PBPSYN), ipp(llsm.A_HAS_HM)
        conf = L.llsm_aoptions_toconf(C.byref(ao), FS / 2.0)
        C.cast(L.llsm_container_get(conf, llsm.CONF_NFRM), llsm.P_int)[0] = nfrm
        if nfft:
            L.llsm_container_attach_(conf, llsm.CONF_NSPEC, C.cast(L.llsm_create_int(nfft // 2 + 1), C.c_void_p),
                                     C.cast(L.llsm_delete_int, C.c_void_p), C.cast(L.llsm_copy_int, C.c_void_p))
        chunks = (C.POINTER(llsm.Chunk) * U)()
        for u in range(U):
            ch = L.llsm_create_chunk(conf, 1)
            assert L.llsm_flat_to_chunk(C.byref(v), u * nfrm, ch) == 0
            if nfft:
                assert L.llsm_flat_l1_to_chunk(C.byref(q), u * nfrm, ch) == 0
            assert L.llsm_chunk_to_blob(ch, words[u].ctypes.data, sizes[u]) == sizes[u], (u, L.llsm_gpu_last_error())
            chunks[u] = ch
        L.llsm_delete_chunks(chunks, U)
        L.llsm_delete_container(conf)
        t2 = time.perf_counter()
        t_host.append((t1 - t0, t2 - t1))
    for k in (0, U // 2, U - 1):                              # ... and agree with the host path
        assert np.array_equal(pinned[offs[k]:offs[k] + sizes[k]], words[k].view(np.uint8)[:sizes[k]])
    L.llsm_gpu_free_host(p)
    b.close()
    med = lambda q: float(np.median(q))
    fr = U * nfrm
    return {"metric": "blob export, " + name, "utterances": U, "frames": fr, "layer1_nfft": nfft, "blob_bytes": total,
            "blob_bytes_per_frame": total / fr, "row_bytes_at_batch_widths": row_bytes, "pack_launches": launches,
            "k_blob_pack": {"ms": med(t_k) * 1e3, "unique_bytes": 2 * total, "TB_per_s": 2 * total / med(t_k) / 1e12},
            "download_blob_block_pinned": {"ms": med(t_blk) * 1e3, "GB_per_s": total / med(t_blk) / 1e9, "frames_per_s": fr / med(t_blk)},
            "download_blobs_pageable": {"ms": med(t_pg) * 1e3, "GB_per_s": total / med(t_pg) / 1e9, "frames_per_s": fr / med(t_pg)},
            "host_path": {"rows_down_ms": t_host[-1][0] * 1e3, "trees_and_blobs_ms": t_host[-1][1] * 1e3,
                          "frames_per_s": fr / sum(t_host[-1])}}


def download_leg(a):
    L = llsm.load()
    L.llsm_chunk_to_blob.restype = C.c_longlong
    L.llsm_chunk_to_blob.argtypes = [C.POINTER(llsm.Chunk), C.c_void_p, C.c_size_t]
    ctx = llsm.Context(0)
    U = a.utts
    steps = [float(np.float32(80.0 * 5.0 ** (k / 15.0))) for k in range(16)]    # 80 -> 400 Hz in 16 steps
    for name, f0_of in (("bench shape, 120 Hz", lambda u: 120.0), ("sweep shape, 80 -> 400 Hz", lambda u: steps[u * 16 // U])):
        for nfft in (0, 2048):
            print(json.dumps(download_case(L, ctx, name, U, f0_of, nfft, a.reps)), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--download", action="store_true")
    a = ap.parse_args()
    if a.download:
        a.utts = a.utts or 1024
        return download_leg(a)
    a.utts = a.utts or 256
    L = llsm.load()
    nfrm, U = 200, a.utts
    ao = llsm.make_aoptions(f0_refine=0)
    L.llsm_analyze.restype = C.POINTER(llsm.Chunk)
    L.llsm_chunk_blob_size.restype = C.c_size_t
    L.llsm_chunk_blob_size.argtypes = [C.POINTER(llsm.Chunk)]
    L.llsm_chunk_to_blob.restype = C.c_longlong
    L.llsm_chunk_to_blob.argtypes = [C.POINTER(llsm.Chunk), C.c_void_p, C.c_size_t]
    L.llsm_blob_to_chunk.restype = C.POINTER(llsm.Chunk)
    L.llsm_blob_to_chunk.argtypes = [C.c_void_p, C.c_size_t]
    L.llsm_blob_view.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(llsm.FlatParams), llsm.P_int, llsm.P_fp, llsm.P_fp]
    L.llsm_gpu_batch_upload_blob.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    chunks = []
    for u in range(U):
        x = make_utterance(u % 8, 120.0); f0 = np.full(nfrm, 120.0, np.float32)
        ch = L.llsm_analyze(C.byref(ao), x.ctypes.data_as(llsm.P_fp), len(x), FS, f0.ctypes.data_as(llsm.P_fp), nfrm, None)
        assert ch, L.llsm_gpu_last_error()
        chunks.append(ch)
    sizes = [L.llsm_chunk_blob_size(ch) for ch in chunks]
    bufs = [np.zeros((s + 7) // 8, np.uint64) for s in sizes]           # 8-byte aligned
    tot = sum(sizes)
    t_enc, t_view, t_dec, t_up, t_upb = [], [], [], [], []
    L.llsm_gpu_batch_upload_blobs.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    ptrs = (C.c_void_p * U)(*[bf.ctypes.data for bf in bufs]); szs = (C.c_size_t * U)(*sizes)
    ctx = llsm.Context(0)
    b = llsm.Batch(ctx, ao, FS, [44100] * U, [nfrm] * U)
    v = llsm.FlatParams(); nf = C.c_int(0); th = C.c_float(0); fn = C.c_float(0)
    for it in range(a.reps + 1):
        t0 = time.perf_counter()
        for ch, bf, s in zip(chunks, bufs, sizes):
            assert L.llsm_chunk_to_blob(ch, bf.ctypes.data, s) == s
        t1 = time.perf_counter()
        for bf, s in zip(bufs, sizes):
            assert L.llsm_blob_view(bf.ctypes.data, s, C.byref(v), C.byref(nf), C.byref(th), C.byref(fn)) == 0
        t2 = time.perf_counter()
        back = [L.llsm_blob_to_chunk(bf.ctypes.data, s) for bf, s in zip(bufs, sizes)]
        t3 = time.perf_counter()
        for c2 in back:
            assert c2
            L.llsm_delete_chunk(c2)
        t4 = time.perf_counter()
        for u, (bf, s) in enumerate(zip(bufs, sizes)):
            assert L.llsm_gpu_batch_upload_blob(b.h, u, bf.ctypes.data, s) == 0, L.llsm_gpu_last_error()
        ctx.sync()
        t5 = time.perf_counter()
        assert L.llsm_gpu_batch_upload_blobs(b.h, 0, U, ptrs, szs) == 0, L.llsm_gpu_last_error()
        ctx.sync()
        t6 = time.perf_counter()
        if it:
            t_enc.append(t1 - t0); t_view.append(t2 - t1); t_dec.append(t3 - t2); t_up.append(t5 - t4); t_upb.append(t6 - t5)
    b.synthesize(llsm.make_soptions(FS), seed=3); ctx.sync()
    y = b.download(llsm.A_Y)
    med = lambda q: float(np.median(q))
    fr = U * nfrm
    print(json.dumps({"metric": "wire format v2, config-2 chunks", "chunks": U, "frames": fr, "blob_bytes_per_frame": tot / fr,
                      "chunk_to_blob": {"MB_per_s": tot / med(t_enc) / 1e6, "frames_per_s": fr / med(t_enc)},
                      "blob_view_validate": {"MB_per_s": tot / med(t_view) / 1e6, "frames_per_s": fr / med(t_view)},
                      "blob_to_chunk": {"MB_per_s": tot / med(t_dec) / 1e6, "frames_per_s": fr / med(t_dec)},
                      "batch_upload_blob": {"MB_per_s": tot / med(t_up) / 1e6, "frames_per_s": fr / med(t_up)},
                      "batch_upload_blobs": {"MB_per_s": tot / med(t_upb) / 1e6, "frames_per_s": fr / med(t_upb)},
                      "synthesis_from_blob_rows_finite": bool(np.all(np.isfinite(y)) and float(np.abs(y).max()) > 0.05)}))
    b.close(); ctx.close()


if __name__ == "__main__":
    main()
