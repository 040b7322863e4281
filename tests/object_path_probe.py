"""Everything the host object path returns, for ONE process, one library and one setting of the environment switches
(LLSM_PACKED_FRAMES, LLSM_FRAME_SLABS, LLSM_OUTPUT_POOL): a collector for tests/test_gpu_object_path.py, which runs it in
fresh child processes and compares the routes with one another, and for tools/ab_objects.py, which compares two
libraries route by route.

    python tests/object_path_probe.py --digests        one JSON line {key: [dtype, shape, sha1]} on stdout
    python tests/object_path_probe.py out.npz          the arrays themselves

Inputs, at the suite's FS: speech-like utterances of 0.15 s and 0.1 s (voiced / unvoiced boundaries inside) and, between
them, one utterance with samples and no frames.  Fan-out (1, 2, 2): two blocks, the first holding the frameless one.
  ana/r<f0_refine>/...   llsm_analyze_batch with x_ap: every frame member of every chunk, the F0 written back, the residuals
  one/r<f0_refine>/...   llsm_analyze of the first utterance: the same members
  syn/all, syn/pair      llsm_synthesize_batch of the three chunks / of the two with frames (one block of two), pinned seed
  syn/replaced           ... after one frame of the first chunk was replaced by a copy: its block falls back to rows
  syn/copies             ... of deep copies of the chunks (heap frames)
  syn/one                llsm_synthesize of the first chunk
  syn/l1                 use_l1 synthesis of a copy after llsm_chunk_tolayer1
  end/...                live slabs and slab bytes (llsm_slab_stats) and live output bytes once everything is deleted, minus
                         their values at the start: zeros
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

SECONDS = (0.15, 0.05, 0.1)          # the middle utterance keeps its samples and gets no frames
PARTS = ("y", "y_sin", "y_noise")


def collect():
    import libllsm2_amd as llsm
    from conftest import FS, make_speechlike
    L = llsm.load()
    P, PI = llsm.P_fp, llsm.P_int
    PC, PO = C.POINTER(llsm.Chunk), C.POINTER(llsm.Output)
    L.llsm_analyze_batch.argtypes = [C.POINTER(llsm.AOptions), C.POINTER(P), PI, C.c_float, C.POINTER(P), PI, C.c_int, C.POINTER(PC), C.POINTER(P)]
    L.llsm_synthesize_batch.argtypes = [C.POINTER(llsm.SOptions), C.POINTER(PC), C.c_int, C.POINTER(PO)]
    L.llsm_analyze.restype = PC
    L.llsm_analyze.argtypes = [C.POINTER(llsm.AOptions), P, C.c_int, C.c_float, P, C.c_int, C.POINTER(P)]
    L.llsm_synthesize.restype = PO
    L.llsm_synthesize.argtypes = [C.POINTER(llsm.SOptions), PC]
    L.llsm_delete_output.argtypes = [PO]
    L.llsm_slab_stats.argtypes = [C.POINTER(C.c_longlong)] * 3
    L.llsm_output_live_bytes.restype = C.c_longlong
    libc = C.CDLL(None); libc.free.argtypes = [C.c_void_p]
    out = {"library": np.array(llsm.LIB_PATH)}

    def live():
        n, b = C.c_longlong(0), C.c_longlong(0)
        L.llsm_slab_stats(C.byref(n), C.byref(b), None)
        return np.array([n.value, b.value, L.llsm_output_live_bytes()], np.int64)

    def arr(p, n, dtype=np.float32):
        return np.ctypeslib.as_array(p, (n,)).astype(dtype, copy=True) if n > 0 else np.zeros(0, dtype)

    def members(tag, ch, nfrm):
        """every member tests/test_gpu_round2.py's `members` reads, frame after frame (a missing object counts as -1)"""
        ints, f0, ampl, phse, psd, edc, ea, ep, res = [], [], [], [], [], [], [], [], []
        for i in range(nfrm):
            fr = ch.contents.frames[i]
            f0.append(C.cast(L.llsm_container_get(fr, llsm.FRAME_F0), P)[0])
            hm = C.cast(L.llsm_container_get(fr, llsm.FRAME_HM), C.POINTER(llsm.HMFrame))
            nm = C.cast(L.llsm_container_get(fr, llsm.FRAME_NM), C.POINTER(llsm.NMFrame))
            rp = C.cast(L.llsm_container_get(fr, llsm.FRAME_PSDRES), P)
            ints.append(hm.contents.nhar if hm else -1)
            if hm:
                ampl.append(arr(hm.contents.ampl, hm.contents.nhar)); phse.append(arr(hm.contents.phse, hm.contents.nhar))
            ints += [nm.contents.npsd, nm.contents.nchannel] if nm else [-1, -1]
            if nm:
                psd.append(arr(nm.contents.psd, nm.contents.npsd)); edc.append(arr(nm.contents.edc, nm.contents.nchannel))
                for c in range(nm.contents.nchannel):
                    e = nm.contents.eenv[c].contents
                    ints.append(e.nhar); ea.append(arr(e.ampl, e.nhar)); ep.append(arr(e.phse, e.nhar))
            n = L.llsm_fparray_length(rp) if rp else -1
            ints.append(n)
            if rp:
                res.append(arr(rp, n))
        cat = lambda v: np.concatenate(v + [np.zeros(0, np.float32)])
        out[f"{tag}/f0"] = np.asarray(f0, np.float32); out[f"{tag}/counts"] = np.asarray(ints, np.int64)
        for k, v in (("ampl", ampl), ("phse", phse), ("psd", psd), ("edc", edc), ("eenv_ampl", ea), ("eenv_phse", ep), ("psdres", res)):
            out[f"{tag}/{k}"] = cat(v)

    xs, f0s = [], []
    for u, sec in enumerate(SECONDS):
        x, f0 = make_speechlike(60 + u, nx=int(sec * FS))
        xs.append(np.ascontiguousarray(x, np.float32)); f0s.append(f0.astype(np.float32) if u != 1 else np.zeros(0, np.float32))
    U = len(xs)
    nx = np.array([len(x) for x in xs], np.int32); nf = np.array([len(f) for f in f0s], np.int32)
    so = llsm.make_soptions(FS)
    start = live()
    L.llsm_gpu_set_fanout(1, 2, 2)
    try:
        kept = None
        for refine in (0, 1):
            ao = llsm.make_aoptions(f0_refine=refine)
            f0_b = [f.copy() for f in f0s]
            xp = (P * U)(*[x.ctypes.data_as(P) for x in xs]); fp = (P * U)(*[f.ctypes.data_as(P) for f in f0_b])
            chunks = (PC * U)(); xap = (P * U)()
            assert L.llsm_analyze_batch(C.byref(ao), xp, nx.ctypes.data_as(PI), FS, fp, nf.ctypes.data_as(PI), U, chunks, xap) == 0, L.llsm_gpu_last_error()
            for u in range(U):
                members(f"ana/r{refine}/u{u}", chunks[u], int(nf[u]))
                out[f"ana/r{refine}/u{u}/f0_back"] = f0_b[u]
                out[f"ana/r{refine}/u{u}/x_ap"] = arr(xap[u], int(nx[u]))
                libc.free(C.cast(xap[u], C.c_void_p))
            f0_1 = f0s[0].copy(); ap = P()
            one = L.llsm_analyze(C.byref(ao), xs[0].ctypes.data_as(P), len(xs[0]), FS, f0_1.ctypes.data_as(P), len(f0_1), C.byref(ap))
            assert one, L.llsm_gpu_last_error()
            members(f"one/r{refine}", one, int(nf[0]))
            out[f"one/r{refine}/f0_back"] = f0_1; out[f"one/r{refine}/x_ap"] = arr(ap, int(nx[0]))
            libc.free(C.cast(ap, C.c_void_p)); L.llsm_delete_chunk(one)
            if refine == 0:
                kept = chunks                                                     # synthesised below
            else:
                for u in range(U):
                    L.llsm_delete_chunk(chunks[u])
        chunks = kept

        def synth(tag, cs, n, seed, opts=so):
            L.llsm_gpu_set_default_seed(seed)
            outs = (PO * n)()
            assert L.llsm_synthesize_batch(C.byref(opts), cs, n, outs) == 0, L.llsm_gpu_last_error()
            for u in range(n):
                for k in PARTS:
                    out[f"{tag}/u{u}/{k}"] = arr(getattr(outs[u].contents, k), outs[u].contents.ny)
            for u in reversed(range(n)):
                L.llsm_delete_output(outs[u])

        synth("syn/all", chunks, U, 700)
        synth("syn/pair", (PC * 2)(chunks[0], chunks[2]), 2, 701)
        L.llsm_gpu_set_default_seed(702)
        o = L.llsm_synthesize(C.byref(so), chunks[0]); assert o, L.llsm_gpu_last_error()
        for k in PARTS:
            out[f"syn/one/{k}"] = arr(getattr(o.contents, k), o.contents.ny)
        L.llsm_delete_output(o)
        copies = (PC * U)(*[L.llsm_copy_chunk(chunks[u]) for u in range(U)])
        synth("syn/copies", copies, U, 700)
        l1 = (PC * 1)(L.llsm_copy_chunk(chunks[0]))
        L.llsm_chunk_tolayer1(l1[0], 2048)
        synth("syn/l1", l1, 1, 703, llsm.make_soptions(FS, use_l1=1))
        # a frame of the first chunk replaced by a copy of its neighbour (a voiced one): that block is flattened the ordinary way
        fr = chunks[0].contents.frames
        i = int(np.flatnonzero((f0s[0][:-1] > 0) & (f0s[0][1:] > 0))[0])
        old = C.cast(fr[i], C.c_void_p).value                                # (the address: a ctypes pointer taken from the slot is a view of the slot)
        fr[i] = L.llsm_copy_container(fr[i + 1])
        L.llsm_delete_container(C.cast(C.c_void_p(old), C.POINTER(llsm.Container)))
        synth("syn/replaced", chunks, U, 704)
        for cs in (chunks, copies, l1):
            for ch in cs:
                L.llsm_delete_chunk(ch)
    finally:
        L.llsm_gpu_set_fanout(-1, -1, -1)
    for k, v in zip(("slabs", "slab_bytes", "output_bytes"), live() - start):
        out[f"end/{k}"] = np.array([v], np.int64)
    return out


def digests(res):
    return {k: [str(v.dtype), list(v.shape), hashlib.sha1(np.ascontiguousarray(v).tobytes()).hexdigest()]
            for k, v in res.items() if k != "library"}


if __name__ == "__main__":
    if len(sys.argv) != 2 or (sys.argv[1].startswith("-") and sys.argv[1] != "--digests"):
        sys.exit(__doc__)
    res = collect()
    if sys.argv[1] == "--digests":
        print(json.dumps(digests(res)))
    else:
        np.savez(sys.argv[1], **res)
        print(f"{len(res) - 1} arrays of {res['library']} -> {sys.argv[1]}")
