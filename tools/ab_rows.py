"""Bits and launches of one library over a fixed list of small configurations, for A/B runs of host-side engine changes.

    LLSM_AMD_LIB=/path/to/parent.so python tools/ab_rows.py parent.npz
    python tools/ab_rows.py new.npz
    python tools/ab_rows.py --compare parent.npz new.npz

One process, one library: every configuration runs once, every batch array it produces and the kernel names and launch
counts of llsm_gpu_get_profile go into the .npz.  --compare needs no GPU: it holds two such files to the same keys, the
same bytes in every array (NaNs included) and the same kernel names and counts, and exits 1 otherwise.

Configurations, each on three utterances of unequal length, the middle one frameless:
  ana/<hm>_r<f0_refine>_o<overlap>   llsm_gpu_batch_analyze under HMCZT / HMPP, f0_refine 0 / 1, second stream off / on,
                                     then llsm_gpu_batch_synthesize of the analysed rows
  frame/<hm>, frame/refine           llsm_harmonic_analysis / llsm_refine_f0 (llsm_engine_batch_harmonics with
                                     refine_only 0 / 1; default context: arrays only, its profile is not exposed)
  syn/<fused|n4096>_l<use_l1>_e<0|1> synthesis at the fused noise kernel (44.1 kHz, 5 ms) and at a 4096-point noise
                                     transform (96 kHz, 9 ms), use_l1 0 / 1, LLSM_GPU_EXCITE4 unset / set
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SECONDS = (0.15, 0.05, 0.1)         # the middle utterance keeps its samples and gets no frames
OUT_IDS = ("A_Y", "A_YSIN", "A_YNOISE")


def utterances(fs, thop, scale=1.0):
    from conftest import make_speechlike
    xs, f0s = [], []
    for u, sec in enumerate(SECONDS):
        x, f0 = make_speechlike(60 + u, nx=int(sec * scale * fs), fs=fs, thop=thop)
        xs.append(x); f0s.append(f0.astype(np.float32) if u != 1 else np.zeros(0, np.float32))
    return xs, f0s


def collect():
    import libllsm2_amd as llsm
    from conftest import FS
    L = llsm.load()
    ctx = llsm.Context(0)
    ctx.set_profiling(True)
    out = {"library": np.array(llsm.LIB_PATH)}

    def keep(tag, b, ids):
        for a in ids:
            out[f"{tag}/{a}"] = b.download(getattr(llsm, a) if isinstance(a, str) else a)
        prof = ctx.profile()
        out[f"{tag}/kernels"] = np.array(sorted(prof))
        out[f"{tag}/launches"] = np.array([prof[k][1] for k in sorted(prof)], np.int64)
        ctx.reset_profile()

    def analysed(ao, fs, xs, f0s):
        b = llsm.Batch(ctx, ao, fs, [len(x) for x in xs], [len(f) for f in f0s])
        b.upload(llsm.A_X, np.concatenate(xs)); b.upload(llsm.A_F0, np.concatenate(f0s))
        ctx.reset_profile()
        b.analyze(); ctx.sync()
        return b

    prev = L.llsm_gpu_analysis_overlap(-1)
    try:
        xs, f0s = utterances(FS, 0.005)
        for hm, name in ((llsm.HMCZT, "hmczt"), (llsm.HMPP, "hmpp")):
            for refine in (0, 1):
                for overlap in (0, 1):
                    L.llsm_gpu_analysis_overlap(overlap)
                    b = analysed(llsm.make_aoptions(f0_refine=refine, hm_method=hm), FS, xs, f0s)
                    b.synthesize(llsm.make_soptions(FS), seed=11); ctx.sync()
                    keep(f"ana/{name}_r{refine}_o{overlap}", b, list(llsm.Batch.PARAM_IDS) + [llsm.A_XRES] + list(OUT_IDS))
                    b.close()
    finally:
        L.llsm_gpu_analysis_overlap(prev)

    # per-frame API on the first utterance
    P, PI = llsm.P_fp, llsm.P_int
    L.llsm_harmonic_analysis.argtypes = [P, C.c_int, C.c_float, P, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, PI,
                                         C.POINTER(P), C.POINTER(P)]
    L.llsm_refine_f0.argtypes = [P, C.c_int, C.c_float, P, C.c_int, C.c_float]
    x, f0 = xs[0], f0s[0]
    for hm, name in ((llsm.HMCZT, "hmczt"), (llsm.HMPP, "hmpp")):
        n = len(f0)
        nhar = np.zeros(n, np.int32); pa = (P * n)(); pp = (P * n)()
        L.llsm_harmonic_analysis(x.ctypes.data_as(P), len(x), FS, f0.ctypes.data_as(P), n, 0.005, 4.0, 80, hm,
                                 nhar.ctypes.data_as(PI), pa, pp)
        out[f"frame/{name}/nhar"] = nhar
        for what, tab in (("ampl", pa), ("phse", pp)):
            out[f"frame/{name}/{what}"] = np.concatenate(
                [np.ctypeslib.as_array(tab[i], (int(nhar[i]),)).copy() for i in range(n) if bool(tab[i])] + [np.zeros(0, np.float32)])
    fr = f0.copy()
    L.llsm_refine_f0(x.ctypes.data_as(P), len(x), FS, fr.ctypes.data_as(P), len(fr), 0.005)
    out["frame/refine/f0"] = fr

    # synthesis: fused noise kernel, and a noise transform of 4096 points (hop 864 samples > 840)
    had = os.environ.pop("LLSM_GPU_EXCITE4", None)
    try:
        for (fs, thop, scale), name in (((FS, 0.005, 1.0), "fused"), ((96000.0, 0.009, 2.0), "n4096")):
            xs, f0s = utterances(fs, thop, scale)
            ao = llsm.make_aoptions(f0_refine=0, thop=thop)
            for use_l1 in (0, 1):
                for e4 in (0, 1):
                    os.environ.pop("LLSM_GPU_EXCITE4", None)
                    if e4:
                        os.environ["LLSM_GPU_EXCITE4"] = "1"
                    b = analysed(ao, fs, xs, f0s)
                    ids = list(OUT_IDS)
                    if use_l1:
                        b.tolayer1(2048)
                        b.upload(llsm.A_PBPSYN, (np.arange(b.layout.total_frames) % 20 > 10).astype(np.int32))
                        L.llsm_gpu_batch_set_maxnhar_conf(b.h, ao.maxnhar)
                        ids += list(llsm.Batch.L1_IDS)
                    ctx.reset_profile()
                    b.synthesize(llsm.make_soptions(fs, use_l1=use_l1), seed=5); ctx.sync()
                    keep(f"syn/{name}_l{use_l1}_e{e4}", b, ids)
                    b.close()
    finally:
        os.environ.pop("LLSM_GPU_EXCITE4", None)
        if had is not None:
            os.environ["LLSM_GPU_EXCITE4"] = had
    ctx.close()
    return out


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    print(f"A {pa}: {a['library']}\nB {pb}: {b['library']}")
    bad = [f"only in one file: {k}" for k in sorted(set(a.files) ^ set(b.files))]
    n = 0
    for k in sorted(set(a.files) & set(b.files)):
        if k == "library":
            continue
        u, v = a[k], b[k]
        n += 1
        if u.dtype != v.dtype or u.shape != v.shape:
            bad.append(f"{k}: {u.dtype}{u.shape} against {v.dtype}{v.shape}")
        elif u.dtype.kind == "U":
            if not np.array_equal(u, v):
                bad.append(f"{k}: kernel names {sorted(set(u) ^ set(v))}")
        elif u.tobytes() != v.tobytes():
            if k.endswith("/launches"):
                names = a[k[:-len("launches")] + "kernels"]
                bad.append(f"{k}: " + ", ".join(f"{m} {i} -> {j}" for m, i, j in zip(names, u, v) if i != j))
            else:
                d = np.flatnonzero(u.reshape(-1).view(np.uint32) != v.reshape(-1).view(np.uint32))
                bad.append(f"{k}: {d.size} of {u.size} words differ, first at {int(d[0])}")
    launches = sum(int(a[k].sum()) for k in a.files if k.endswith("/launches"))
    print(f"{n} arrays compared, {launches} launches counted in A")
    for line in bad:
        print("DIFFERS", line)
    print("identical" if not bad else f"{len(bad)} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2 or sys.argv[1].startswith("-"):
        sys.exit(__doc__)
    res = collect()
    np.savez(sys.argv[1], **res)
    print(f"{len(res) - 1} arrays of {res['library']} -> {sys.argv[1]}")
