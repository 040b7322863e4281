"""Times llsm_gpu_batch_align_pyramid and k_pool_code.

long    one pair of two takes of --long-frames frames (tools/bench_align_around.py's drifting pair): coarse to fine in one
        call, llsm_gpu_batch_align_pyramid at --factor and --margin with slope = 1, beside the same chain run by hand through
        the public calls -- llsm_gpu_batch_pool_code of both takes, two coarse batches created and the pooled vectors
        uploaded, llsm_gpu_batch_align_slope, llsm_gpu_align_center_line, llsm_gpu_align_around_min, llsm_gpu_batch_align_around,
        the coarse batches deleted.  The two take turns in one loop so that both see the same state of the machine, and
        their results are compared bit for bit.  Wall time of the synchronous calls; the kernels of one profiled call each
        from HIP events.
pool    k_pool_code alone on --pool-utts utterances of --pool-frames frames at --factor: its HIP-event time over profiled
        calls of llsm_gpu_batch_pool_code, and the bytes it moves -- LLSM_GPU_CODE read once, 1 / factor of it written --
        per second.  (The wall time of that call is dominated by the copy of the pooled vectors to the host.)

Prints one JSON object.

    python tools/bench_align_pyramid.py [--long-frames 60000] [--drift 0.05] [--factor 16] [--margin 4] [--pool-utts 1024]
        [--pool-frames 1154] [--steps 12] [--warmup 3] [--skip-long] [--skip-pool] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import libllsm2_amd as llsm  # noqa: E402
from bench_align_around import DIM, batch_of, long_pair, spread  # noqa: E402


def same_bits(x, y):
    return bool(x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32)))


def long(ctx, a):
    F, f, margin = a.long_frames, a.factor, a.margin
    ca, cb, truth = long_pair(F, a.drift)
    fa, fb = batch_of(ctx, [F], ca), batch_of(ctx, [F], cb)
    one = np.zeros(1, np.int32)
    stages = {}

    def stage(name, t0):
        stages.setdefault(name, []).append((time.perf_counter() - t0) * 1e3)
        return time.perf_counter()

    def one_call():
        return fa.align_pyramid(fb, one, one, f, margin, slope=True)

    def by_hand():
        t = time.perf_counter()
        pa, pb = fa.pool_code(one, f)[0], fb.pool_code(one, f)[0]
        t = stage("pool_code_x2", t)
        ka, kb = batch_of(ctx, [len(pa)], pa), batch_of(ctx, [len(pb)], pb)
        t = stage("coarse_batches", t)
        pos_c = ka.align_slope(kb, one, one)[0][0]
        t = stage("coarse_align_slope", t)
        line = llsm.align_center_line(pos_c, len(pb), F, F)
        band = max(min(margin * f, F - 1), llsm.align_around_min(F, F, line, slope=True))
        t = stage("line_and_band", t)
        pos, cost = fa.align_around(fb, one, one, line, band, slope=True)
        t = stage("fine_align_around", t)
        ka.close(); kb.close()
        stage("delete_coarse_batches", t)
        return pos, cost, [line], np.array([band], np.int32)

    calls = {"pyramid": one_call, "by_hand": by_hand}
    last = {}
    for _ in range(a.warmup):
        for name, call in calls.items():
            last[name] = call()
    stages.clear()
    walls = {name: [] for name in calls}
    for _ in range(a.steps):
        for name, call in calls.items():
            t0 = time.perf_counter(); last[name] = call(); walls[name].append((time.perf_counter() - t0) * 1e3)
    kern = {name: {} for name in calls}
    kept = {k: list(v) for k, v in stages.items()}                  # (the profiled calls below are not part of the stage times)
    ctx.set_profiling(True)
    for _ in range(min(a.steps, 4)):
        for name, call in calls.items():
            ctx.reset_profile(); call()
            for k, v in ctx.profile().items():
                if v[1] > 0:
                    kern[name].setdefault(k, []).append(v[0])
    ctx.set_profiling(False)
    p, h = last["pyramid"], last["by_hand"]
    nc = llsm.pool_frames(F, f)
    out = dict(shape=dict(frames=F, drift=a.drift, factor=f, margin=margin, slope=1, coarse_frames=nc, coarse_cells=nc * nc,
                          band=int(p[3][0]), fine_plane_cells=F * (2 * int(p[3][0]) + 1), dim=DIM),
               pyramid=dict(wall_ms=spread(walls["pyramid"]), kernels_ms={k: spread(v) for k, v in kern["pyramid"].items()}),
               by_hand=dict(wall_ms=spread(walls["by_hand"]), stages_ms={k: spread(v) for k, v in kept.items()},
                            kernels_ms={k: spread(v) for k, v in kern["by_hand"].items()}),
               wall_ratio_pyramid_over_by_hand=float(np.median(walls["pyramid"]) / np.median(walls["by_hand"])),
               same_bits=bool(same_bits(p[0][0], h[0][0]) and same_bits(p[1], h[1]) and np.array_equal(p[2][0], h[2][0]) and
                              np.array_equal(p[3], h[3])),
               cost=float(p[1][0]),
               pos_from_warp=dict(max=float(np.max(np.abs(p[0][0] - truth))), median=float(np.median(np.abs(p[0][0] - truth)))),
               pos_from_line=float(np.max(np.abs(p[0][0] - p[2][0]))))
    fa.close(); fb.close()
    return out


def pool(ctx, a):
    n, F, f = a.pool_utts, a.pool_frames, a.factor
    rng = np.random.default_rng(4)
    code = rng.standard_normal((n * F, DIM)).astype(np.float32)
    b = batch_of(ctx, [F] * n, code)
    utts = np.arange(n, dtype=np.int32)
    for _ in range(a.warmup):
        got = b.pool_code(utts, f)
    ctx.set_profiling(True)
    ms = []
    for _ in range(a.steps):
        ctx.reset_profile(); b.pool_code(utts, f)
        v = ctx.profile()["k_pool_code"]
        assert v[1] == 1
        ms.append(v[0])
    ctx.set_profiling(False)
    nc = llsm.pool_frames(F, f)
    moved = (n * F + n * nc) * DIM * 4
    k = int(rng.integers(0, n))                                     # one utterance against float64 means: a sanity check, not the test
    want = np.stack([code[k * F + j * f:min(k * F + (j + 1) * f, (k + 1) * F)].astype(np.float64).mean(0) for j in range(nc)])
    out = dict(shape=dict(utterances=n, frames=F, factor=f, coarse_frames=nc, dim=DIM, bytes_read=n * F * DIM * 4, bytes_written=n * nc * DIM * 4),
               kernel_ms=spread(ms), bytes_per_second=dict(at_median=moved / (float(np.median(ms)) * 1e-3), at_min=moved / (min(ms) * 1e-3)),
               max_abs_error_vs_float64=float(np.max(np.abs(got[k] - want))))
    b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--long-frames", type=int, default=60000)
    ap.add_argument("--drift", type=float, default=0.05)
    ap.add_argument("--factor", type=int, default=16)
    ap.add_argument("--margin", type=int, default=4)
    ap.add_argument("--pool-utts", type=int, default=1024)
    ap.add_argument("--pool-frames", type=int, default=1154)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-long", action="store_true")
    ap.add_argument("--skip-pool", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = llsm.Context(0)
    out = {}
    if not a.skip_long:
        out["long"] = long(ctx, a)
    if not a.skip_pool:
        out["pool"] = pool(ctx, a)
    ctx.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
