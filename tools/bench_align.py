"""Times llsm_gpu_batch_align at the bench shape (1 024 pairs of 200 x 200 frames, coder orders 64 + 5, default options: the
64 mel-spectrum columns, no step or voicing cost) and, beside it on the same box, the host round trip the call replaces:
download LLSM_GPU_CODE of both batches, the numpy reference (tests/align_reference.py) on a few pairs SCALED to the
number of pairs, upload of the map.

The vectors are align_reference.make trajectories in the 64 compared columns (a warped pair per utterance), uploaded into
batches without samples; no analysis runs.

Prints one JSON object: ms per call (wall: min / median / max over the steps after the warm-up), ms per call of each kernel
from HIP events (llsm_gpu_get_profile: min / median / max of one profiled call each), cells and cell updates per second,
and the host round trip with its scaling stated.

    python tools/bench_align.py [--pairs 1024] [--frames 200] [--steps 10] [--warmup 2] [--cpu-pairs 4] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import libllsm2_amd as llsm  # noqa: E402
import align_reference as aref  # noqa: E402

FS = 44100.0
OSP, OBAP = 64, 5


def spread(v):
    return dict(min=float(min(v)), median=float(np.median(v)), max=float(max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-pairs", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, F = a.pairs, a.frames
    dim = OSP + OBAP + 3
    ca = np.zeros((n * F, dim), np.float32); cb = np.zeros((n * F, dim), np.float32)
    for p in range(n):                                     # 16 distinct trajectories, repeated: the time does not depend on the values
        if p < 16:
            A, B, _ = aref.make(p, F, F, OSP, 0.3)
            ca[p * F:(p + 1) * F, 3:3 + OSP] = A; cb[p * F:(p + 1) * F, 3:3 + OSP] = B
        else:
            ca[p * F:(p + 1) * F] = ca[(p % 16) * F:(p % 16 + 1) * F]; cb[p * F:(p + 1) * F] = cb[(p % 16) * F:(p % 16 + 1) * F]
    ctx = llsm.Context(0)
    batches = []
    for code in (ca, cb):
        b = llsm.Batch(ctx, llsm.make_aoptions(f0_refine=0), FS, [0] * n, [F] * n)
        b.enable_layer1(128); b.enable_coder(OSP, OBAP); b.upload(llsm.A_CODE, code)
        batches.append(b)
    qa, qb = batches
    idx = np.arange(n, dtype=np.int32)
    call = lambda: qa.align(qb, idx, idx)
    for _ in range(a.warmup):
        pos, cost = call()
    walls = []
    for _ in range(a.steps):                               # wall time of the (synchronous) call, no events
        t0 = time.perf_counter(); call(); walls.append((time.perf_counter() - t0) * 1e3)
    kern = {}
    ctx.set_profiling(True)
    for _ in range(a.steps):                               # one profiled call at a time: the spread of each kernel
        ctx.reset_profile(); call()
        for k, v in ctx.profile().items():
            if v[1] > 0:
                kern.setdefault(k, []).append(v[0] / v[1])
    ctx.set_profiling(False)
    cells = n * F * F
    wall = float(np.median(walls))
    out = dict(shape=dict(pairs=n, frames_a=F, frames_b=F, order_spec=OSP, order_bap=OBAP, first=3, count=OSP, cells=cells,
                          plane_bytes=4 * cells),
               wall_ms=spread(walls), kernels_ms={k: spread(v) for k, v in kern.items()},
               kernels_ms_sum=float(sum(np.median(v) for v in kern.values())),
               pairs_per_s=n / (wall * 1e-3), cells_per_s=cells / (wall * 1e-3))
    if "k_align_dist" in kern:
        out["dist_plane_write_GBps"] = 4 * cells / (np.median(kern["k_align_dist"]) * 1e-3) / 1e9
    if "k_align_dtw" in kern:
        out["dtw_cells_per_s"] = cells / (np.median(kern["k_align_dtw"]) * 1e-3)
    # the host round trip the call replaces
    if a.cpu_pairs > 0:
        m = min(a.cpu_pairs, n)
        t0 = time.perf_counter(); da = qa.download(llsm.A_CODE); db = qb.download(llsm.A_CODE); t_down = time.perf_counter() - t0
        t0 = time.perf_counter()
        ref = [aref.align(da[p * F:(p + 1) * F], db[p * F:(p + 1) * F], 3, OSP) for p in range(m)]
        t_ref = time.perf_counter() - t0
        same = all(np.array_equal(ref[p][0], pos[p]) and ref[p][1] == cost[p] for p in range(m))
        stage = np.concatenate(pos)
        t0 = time.perf_counter(); qa.upload(llsm.A_F0, stage); ctx.sync(); t_up = time.perf_counter() - t0   # (a map is one float per frame of a, like the F0 row)
        out["host_round_trip"] = dict(download_code_ms=t_down * 1e3, numpy_reference_pairs=m, numpy_reference_ms_measured=t_ref * 1e3,
                                      numpy_reference_ms_scaled_to_all_pairs=t_ref * 1e3 * n / m, upload_map_ms=t_up * 1e3,
                                      total_ms_scaled=t_down * 1e3 + t_ref * 1e3 * n / m + t_up * 1e3,
                                      note="the numpy time is measured on %d pairs on one CPU core and scaled by %d / %d" % (m, n, m),
                                      reference_equals_device=bool(same))
    qa.close(); qb.close(); ctx.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
