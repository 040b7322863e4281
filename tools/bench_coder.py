"""Frame coder throughput: llsm_coder_encode_frames / llsm_coder_decode_frames over the frames of
analysed + layer-1 converted config-2 utterances (containers in, containers out: the object model's host cost
included; the kernel times are in the rocprofv3 trace of this command, profiles/r02_*_coder_kernel_stats.txt).

    python tools/bench_coder.py [--utts 64] [--reps 5]

--resident: the same analysed utterances as ONE device-resident batch (--utts up to the bench's 1024 x 200 frames) through
llsm_gpu_batch_encode / _decode: kernel times from the context's HIP events, and the wall time of
the chain encode -> decode(1) -> tolayer0(1) -> phasepropagate(+1) -> synthesize.

    python tools/bench_coder.py --resident [--utts 1024] [--reps 5]
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


def resident(a):
    nfrm, osp, obap = 200, 64, 5
    ao = llsm.make_aoptions(f0_refine=0)
    so = llsm.make_soptions(FS)
    ctx = llsm.Context(0)
    xs = [make_utterance(u % 8, 120.0) for u in range(a.utts)]
    b = llsm.Batch(ctx, ao, FS, [len(x) for x in xs], [nfrm] * a.utts)
    b.upload(llsm.A_X, np.concatenate(xs)); b.upload(llsm.A_F0, np.full(a.utts * nfrm, 120.0, np.float32))
    b.analyze(); b.tolayer1(2048); b.enable_coder(osp, obap); ctx.sync()
    n, ns, lay = a.utts * nfrm, b.nspec, b.layout
    dim = b.coder_dimension

    def kernel_ms(fn, name):
        fn(); ctx.sync()                                    # warm-up
        ctx.reset_profile(); ctx.set_profiling(True, only=name)
        for _ in range(a.reps):
            fn()
        ctx.sync(); ctx.set_profiling(False)
        ms, k = ctx.profile()[name]
        return ms / k

    enc_ms = kernel_ms(b.encode, "k_coder_encode")
    code = b.download(llsm.A_CODE)
    dec1_ms = kernel_ms(lambda: b.decode(1), "k_coder_decode")
    dec0_ms = kernel_ms(lambda: b.decode(0), "k_coder_decode")

    def chain():
        b.encode(); b.decode(1); b.tolayer0(True); b.phasepropagate(+1); b.synthesize(so, seed=1)

    b.upload(llsm.A_CODE, code); b.decode(1); b.tolayer0(True); ctx.sync()
    chain(); ctx.sync()
    walls = []
    for _ in range(a.reps):
        t = time.perf_counter(); chain(); ctx.sync(); walls.append(time.perf_counter() - t)
    # unique row bytes per direction: what a frame's rows and its vector occupy
    rows_in = 4 * (3 + lay.npsd + ns)                       # F0, RD, NVSPHSE, PSD, VTMAGN
    rows_l1 = 4 * (10 + lay.npsd + ns + lay.maxnhar + lay.nchannel * (1 + 2 * max(lay.maxnhar_e, 1)))
    rows_l0 = rows_l1 - 4 * ns + 4 * lay.maxnhar
    med = lambda v: float(np.median(v))
    print(json.dumps({"metric": "resident frame coder (order_spec 64, order_bap 5, nfft 2048)", "frames": n, "dimension": dim,
                      "encode_kernel_ms": enc_ms, "decode_layer1_kernel_ms": dec1_ms, "decode_layer0_kernel_ms": dec0_ms,
                      "encode_ns_per_frame": enc_ms * 1e6 / n, "decode_layer1_ns_per_frame": dec1_ms * 1e6 / n,
                      "decode_layer0_ns_per_frame": dec0_ms * 1e6 / n,
                      "encode_unique_mb": n * (rows_in + 4 * dim) / 1e6, "decode_layer1_unique_mb": n * (rows_l1 + 4 * dim) / 1e6,
                      "decode_layer0_unique_mb": n * (rows_l0 + 4 * dim) / 1e6,
                      "chain_wall_ms": med(walls) * 1e3, "finite": bool(np.all(np.isfinite(code)))}))
    b.close(); ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--resident", action="store_true", help="the device-resident batch coder instead of the chunk API")
    a = ap.parse_args()
    if a.resident:
        return resident(a)
    L = llsm.load()
    nfrm = 200
    ao = llsm.make_aoptions(f0_refine=0)
    L.llsm_analyze.restype = C.POINTER(llsm.Chunk)
    chunks = []
    for u in range(a.utts):
        x = make_utterance(u % 8, 120.0); f0 = np.full(nfrm, 120.0, np.float32)
        ch = L.llsm_analyze(C.byref(ao), x.ctypes.data_as(llsm.P_fp), len(x), FS, f0.ctypes.data_as(llsm.P_fp), nfrm, None)
        assert ch, L.llsm_gpu_last_error()
        L.llsm_chunk_tolayer1(ch, 2048)
        chunks.append(ch)
    n = a.utts * nfrm
    frames = (C.POINTER(llsm.Container) * n)()
    for u, ch in enumerate(chunks):
        for i in range(nfrm):
            frames[u * nfrm + i] = ch.contents.frames[i]
    L.llsm_create_coder.restype = C.c_void_p
    coder = C.c_void_p(L.llsm_create_coder(chunks[0].contents.conf, 64, 5))
    L.llsm_coder_dimension.argtypes = [C.c_void_p]
    dim = L.llsm_coder_dimension(coder)
    enc = np.zeros((n, dim), np.float32)
    L.llsm_coder_encode_frames.argtypes = [C.c_void_p, C.POINTER(C.POINTER(llsm.Container)), C.c_int, llsm.P_fp]
    L.llsm_coder_decode_frames.argtypes = [C.c_void_p, llsm.P_fp, C.c_int, C.c_int, C.POINTER(C.POINTER(llsm.Container))]
    outs = (C.POINTER(llsm.Container) * n)()
    te, t0l, t1l = [], [], []
    for it in range(a.reps + 1):
        t = time.perf_counter()
        assert L.llsm_coder_encode_frames(coder, frames, n, enc.ctypes.data_as(llsm.P_fp)) == 0, L.llsm_gpu_last_error()
        t1 = time.perf_counter()
        assert L.llsm_coder_decode_frames(coder, enc.ctypes.data_as(llsm.P_fp), n, 0, outs) == 0, L.llsm_gpu_last_error()
        t2 = time.perf_counter()
        for i in range(n):
            L.llsm_delete_container(outs[i])
        t3 = time.perf_counter()
        assert L.llsm_coder_decode_frames(coder, enc.ctypes.data_as(llsm.P_fp), n, 1, outs) == 0, L.llsm_gpu_last_error()
        t4 = time.perf_counter()
        for i in range(n):
            L.llsm_delete_container(outs[i])
        if it:
            te.append(t1 - t); t0l.append(t2 - t1); t1l.append(t4 - t3)
    med = lambda v: float(np.median(v))
    print(json.dumps({"metric": "frames/s, frame coder (order_spec 64, order_bap 5)", "frames": n, "dimension": dim,
                      "encode_frames_per_s": n / med(te), "decode_layer0_frames_per_s": n / med(t0l),
                      "decode_layer1_frames_per_s": n / med(t1l),
                      "encode_ms": med(te) * 1e3, "decode_layer0_ms": med(t0l) * 1e3, "decode_layer1_ms": med(t1l) * 1e3,
                      "finite": bool(np.all(np.isfinite(enc)))}))


if __name__ == "__main__":
    main()
