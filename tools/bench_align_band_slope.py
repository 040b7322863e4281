"""Times llsm_gpu_batch_align_band_slope against llsm_gpu_batch_align_band at the same band and llsm_gpu_batch_align_slope on
the same pairs in the same process (pairs of frames x frames, coder orders 64 + 5, default options: the 64 mel-spectrum
columns, no step or voicing cost), the calls taking turns in one loop so that all see the same state of the machine.  A call
that refuses the shape (llsm_gpu_batch_align_slope above 2^28 cells) is left out of the loop and its message is reported.

The vectors are those of tools/bench_align_band.py: align_reference.make trajectories in the 64 compared columns (a warped
pair per utterance, 16 distinct pairs repeated), uploaded into batches without samples; no analysis runs.  The time does
not depend on the values.

Prints one JSON object: ms per call (wall: min / median / max over the steps after the warm-up), ms per call of each kernel
from HIP events (llsm_gpu_get_profile: min / median / max of one profiled call each), the cells of the planes and of the
regions and the steps of the path kernels COMPUTED from the shapes by the rules of align.cpp, the ratios of the medians, and how
the results compare: the largest step of pos under each rule, and that no cost of the new call is below the other two's.

    python tools/bench_align_band_slope.py [--pairs 64] [--frames 2000] [--band 100] [--steps 12] [--warmup 3] [--out FILE]
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


def strips(F):
    return [(i0, min(i0 + 63, F - 1)) for i0 in range(0, F, 64)]


def window_steps(lo, hi, F, one_more):
    """the steps of a path kernel over all strips of 64 rows of a pair of F x F frames whose rows span lo ... hi (lo > hi: an
    empty row): the largest hi - the least lo + rows per strip, one more where a strip follows under the slope pattern"""
    total = 0
    for i0, i1 in strips(F):
        full = lo[i0:i1 + 1] <= hi[i0:i1 + 1]
        total += int(hi[i0:i1 + 1][full].max()) - int(lo[i0:i1 + 1][full].min()) + 1 + i1 - i0 + (1 if one_more and i1 + 1 < F else 0)
    return total


def cells_of(lo, hi):
    return int(np.sum(np.maximum(hi.astype(np.int64) - lo + 1, 0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--band", type=int, default=100)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, F, band = a.pairs, a.frames, a.band
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
    calls = {"align_band": lambda: qa.align_band(qb, idx, idx, band), "align_slope": lambda: qa.align_slope(qb, idx, idx),
             "align_band_slope": lambda: qa.align_band_slope(qb, idx, idx, band)}
    refused = {}
    for name in list(calls):                               # a call that refuses the shape takes no part
        try:
            calls[name]()
        except llsm.LlsmError as e:
            refused[name] = str(e); del calls[name]
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
    blo, bhi = llsm.align_band_rows(F, F, band)
    slo, shi = llsm.align_slope_rows(F, F)
    klo, khi = llsm.align_band_slope_rows(F, F, band)
    shape = dict(pairs=n, frames_a=F, frames_b=F, band=band, order_spec=OSP, order_bap=OBAP, first=3, count=OSP,
                 plane_cells=dict(align_band=n * F * (2 * band + 1), align_slope=n * F * F, align_band_slope=n * F * (2 * band + 1)),
                 region_cells=dict(align_band=n * cells_of(blo, bhi), align_slope=n * cells_of(slo, shi), align_band_slope=n * cells_of(klo, khi)),
                 path_steps_per_pair=dict(align_band=window_steps(blo, bhi, F, False), align_slope=window_steps(slo, shi, F, True),
                                          align_band_slope=window_steps(klo, khi, F, True)))
    out = dict(shape=shape)
    for name in ("align_band", "align_slope", "align_band_slope"):
        out[name] = dict(refused=refused[name]) if name in refused else \
            dict(wall_ms=spread(walls[name]), kernels_ms={k: spread(v) for k, v in kern[name].items()})
    new = np.median(walls["align_band_slope"])
    out["wall_ratio_new_over"] = {name: float(new / np.median(walls[name])) for name in calls if name != "align_band_slope"}
    out["largest_step_of_pos"] = {name: float(max(np.diff(x).max() for x in last[name][0])) for name in calls}
    out["smallest_step_of_pos"] = {name: float(min(np.diff(x).min() for x in last[name][0])) for name in calls}
    out["costs_not_below"] = {name: bool(np.all(last["align_band_slope"][1] >= last[name][1])) for name in calls if name != "align_band_slope"}
    qa.close(); qb.close(); ctx.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
