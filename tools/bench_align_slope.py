"""Times llsm_gpu_batch_align_slope against llsm_gpu_batch_align on the same pairs in the same process (pairs of frames x
frames, coder orders 64 + 5, default options: the 64 mel-spectrum columns, no step or voicing cost), the two calls taking
turns in one loop so that both see the same state of the machine.

The vectors are those of tools/bench_align_band.py: align_reference.make trajectories in the 64 compared columns (a warped
pair per utterance, 16 distinct pairs repeated), uploaded into batches without samples; no analysis runs.  The time does
not depend on the values.

Prints one JSON object: ms per call (wall: min / median / max over the steps after the warm-up), ms per call of each kernel
from HIP events (llsm_gpu_get_profile: min / median / max of one profiled call each; k_align_dist runs in both calls and is
listed per call), the cells of the planes, the cells of the region of rule L1, the steps of the path kernels COMPUTED from
the shapes by the rules of align.cpp, the ratio of the two medians, and how the results compare: on how many pairs the
positions are equal, the largest step of pos under either rule, and that no cost is below the full call's.

    python tools/bench_align_slope.py [--pairs 1024] [--frames 200] [--steps 12] [--warmup 3] [--out FILE]
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


def path_steps(F):
    """the steps of one pair of F x F frames in the two path kernels, over all strips of 64 rows: nb + rows - 1 per strip of
    the full call; hi of the last row - lo of the first + rows, one more where a strip follows, under the slope pattern"""
    lo, hi = llsm.align_slope_rows(F, F)
    full = slope = 0
    for i0 in range(0, F, 64):
        i1 = min(i0 + 63, F - 1)
        full += F + i1 - i0
        slope += int(hi[i1]) - int(lo[i0]) + 1 + i1 - i0 + (1 if i1 + 1 < F else 0)
    return full, slope, int(np.sum(np.maximum(hi - lo + 1, 0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
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
    calls = {"align": lambda: qa.align(qb, idx, idx), "align_slope": lambda: qa.align_slope(qb, idx, idx)}
    last = {}
    for _ in range(a.warmup):
        for name, call in calls.items():
            last[name] = call()
    walls = {name: [] for name in calls}
    for _ in range(a.steps):                               # wall time of the (synchronous) calls in turn, no events
        for name, call in calls.items():
            t0 = time.perf_counter(); call(); walls[name].append((time.perf_counter() - t0) * 1e3)
    kern = {name: {} for name in calls}
    ctx.set_profiling(True)
    for _ in range(a.steps):                               # one profiled call at a time: the spread of each kernel
        for name, call in calls.items():
            ctx.reset_profile(); call()
            for k, v in ctx.profile().items():
                if v[1] > 0:
                    kern[name].setdefault(k, []).append(v[0] / v[1])
    ctx.set_profiling(False)
    full_steps, slope_steps, region = path_steps(F)
    (pf, cf), (ps, cs) = last["align"], last["align_slope"]
    out = dict(shape=dict(pairs=n, frames_a=F, frames_b=F, order_spec=OSP, order_bap=OBAP, first=3, count=OSP, cells=n * F * F,
                          region_cells=n * region, path_steps_per_pair=dict(align=full_steps, align_slope=slope_steps)),
               align=dict(wall_ms=spread(walls["align"]), kernels_ms={k: spread(v) for k, v in kern["align"].items()}),
               align_slope=dict(wall_ms=spread(walls["align_slope"]), kernels_ms={k: spread(v) for k, v in kern["align_slope"].items()}),
               wall_ratio_slope_over_full=float(np.median(walls["align_slope"]) / np.median(walls["align"])),
               pairs_with_equal_positions=int(sum(np.array_equal(x, y) for x, y in zip(pf, ps))),
               largest_step_of_pos=dict(align=float(max(np.diff(x).max() for x in pf)), align_slope=float(max(np.diff(x).max() for x in ps))),
               costs_not_below_full=bool(np.all(cs >= cf)))
    qa.close(); qb.close(); ctx.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
