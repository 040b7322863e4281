"""Times llsm_gpu_batch_align_sub, under either pattern, against llsm_gpu_batch_align and llsm_gpu_batch_align_slope on the
same pairs in the same process (coder orders 64 + 5, default options: the 64 mel-spectrum columns, no step or voicing cost),
the calls taking turns in one loop so that all see the same state of the machine.

Two shapes: --pairs P --frames F alone gives P pairs of F x F frames, every query against a take of its own (the shape of
tools/bench_align_slope.py); with --take T there is ONE take of T frames in batch b and every one of the P queries of F
frames is searched in it.  llsm_gpu_batch_align_slope takes part where rule L1 admits the shape.  The vectors are
align_reference.make trajectories in the 64 compared columns, 16 distinct ones repeated; the time does not depend on the
values.  A library without the open-ended call (LLSM_AMD_LIB naming a build of an earlier commit) is timed on the calls it
has, which gives the yardstick kernels before the change in the same words.

Prints one JSON object: ms per call (wall: min / median / max over the steps after the warm-up), ms per call of each kernel
from HIP events (llsm_gpu_get_profile: min / median / max of one profiled call each), the cells of the planes, the steps of
the path kernels per pair COMPUTED from the shapes by the rules of align.cpp, the ratios of the medians of the path kernels,
and how the results compare: that no cost is above the call's with fixed ends.

    python tools/bench_align_sub.py [--pairs 1024] [--frames 200] [--take 0] [--steps 12] [--warmup 3] [--out FILE]
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
PATH_KERNEL = dict(align="k_align_dtw", align_slope="k_align_slope_dtw", align_sub="k_align_sub_dtw", align_sub_slope="k_align_sub_slope_dtw")


def spread(v):
    return dict(min=float(min(v)), median=float(np.median(v)), max=float(max(v)))


def path_steps(na, nb, admitted):
    """the steps of one pair of na x nb frames in the path kernels, over all strips of 64 rows: nb + rows - 1 per strip
    without the pattern, with fixed or free ends; under the pattern hi of the last row - lo of the first + rows, one more
    where a strip follows, over the rows of rule L1 or of rule Q1"""
    steps = dict(align=0, align_sub=0, align_sub_slope=0)
    if admitted:
        lo, hi = llsm.align_slope_rows(na, nb)
        steps["align_slope"] = 0
    for i0 in range(0, na, 64):
        i1 = min(i0 + 63, na - 1)
        more = 1 if i1 + 1 < na else 0
        steps["align"] += nb + i1 - i0; steps["align_sub"] += nb + i1 - i0
        steps["align_sub_slope"] += nb - 1 - (i0 + 1) // 2 + 1 + i1 - i0 + more
        if admitted:
            steps["align_slope"] += int(hi[i1]) - int(lo[i0]) + 1 + i1 - i0 + more
    return steps


def code_rows(n, F, seed0):
    """n utterances of F frames: 16 distinct trajectories, repeated"""
    c = np.zeros((n * F, OSP + OBAP + 3), np.float32)
    for p in range(min(n, 16)):
        c[p * F:(p + 1) * F, 3:3 + OSP] = aref.make(seed0 + p, F, 2, OSP, 0.3)[0]
    for p in range(16, n):
        c[p * F:(p + 1) * F] = c[(p % 16) * F:(p % 16 + 1) * F]
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--take", type=int, default=0)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, F, T = a.pairs, a.frames, a.take or a.frames
    nb_utt = 1 if a.take else n
    ca = code_rows(n, F, 0); cb = code_rows(nb_utt, T, 100)
    ctx = llsm.Context(0)
    batches = []
    for code, count, frames in ((ca, n, F), (cb, nb_utt, T)):
        b = llsm.Batch(ctx, llsm.make_aoptions(f0_refine=0), FS, [0] * count, [frames] * count)
        b.enable_layer1(128); b.enable_coder(OSP, OBAP); b.upload(llsm.A_CODE, code)
        batches.append(b)
    qa, qb = batches
    ua = np.arange(n, dtype=np.int32)
    ub = np.zeros(n, np.int32) if a.take else ua
    admitted = T - 1 <= 2 * (F - 1) and F - 1 <= 2 * (T - 1)       # rule L1
    has_sub = hasattr(llsm.load(), "llsm_gpu_batch_align_sub")
    calls = {"align": lambda: qa.align(qb, ua, ub)}
    if admitted:
        calls["align_slope"] = lambda: qa.align_slope(qb, ua, ub)
    if has_sub:
        calls["align_sub"] = lambda: qa.align_sub(qb, ua, ub)
        calls["align_sub_slope"] = lambda: qa.align_sub(qb, ua, ub, slope=True)
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
    steps = path_steps(F, T, admitted)
    path_ms = {name: float(np.median(kern[name][PATH_KERNEL[name]])) for name in calls}
    out = dict(shape=dict(pairs=n, frames_a=F, frames_b=T, takes=nb_utt, order_spec=OSP, order_bap=OBAP, first=3, count=OSP,
                          cells=n * F * T, path_steps_per_pair={k: v for k, v in steps.items() if k in calls}),
               path_kernel_ms=path_ms,
               path_kernel_us_per_step={name: 1e3 * path_ms[name] / steps[name] for name in calls})
    for name in calls:
        out[name] = dict(wall_ms=spread(walls[name]), kernels_ms={k: spread(v) for k, v in kern[name].items()})
    if has_sub:
        out["path_kernel_ratio"] = dict(sub_over_align=path_ms["align_sub"] / path_ms["align"])
        out["costs_not_above_align"] = bool(np.all(last["align_sub"][2] <= last["align"][1]))
        if admitted:
            out["path_kernel_ratio"]["sub_slope_over_align_slope"] = path_ms["align_sub_slope"] / path_ms["align_slope"]
            out["costs_not_above_align_slope"] = bool(np.all(last["align_sub_slope"][2] <= last["align_slope"][1]))
    qa.close(); qb.close(); ctx.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
