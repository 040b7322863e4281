"""Times llsm_gpu_batch_align_around, the band around a centre line, in two settings.

small   pairs of frames x frames under the straight diagonal of rule B1 at one band, both patterns, against
        llsm_gpu_batch_align_band and llsm_gpu_batch_align_band_slope on the same pairs in the same process, the four calls
        taking turns in one loop so that all see the same state of the machine.  Only the source of a row's centre differs
        (a table read by the kernels against the computed diagonal), and the results are compared bit for bit.
long    one pair of two takes of --long-frames frames, the second the first read along x + drift sin(2 pi x) plus noise, so
        that the path leaves the diagonal by drift x frames.  Coarse to fine: every --decimate'th vector of both into small
        batches, llsm_gpu_batch_align_slope on them, llsm_gpu_align_center_line, llsm_gpu_batch_align_around with slope = 1 at
        a half-width of --around-band.  The whole pipeline is timed per stage, and the straight band that would hold the
        same drift is timed beside it if its plane fits the cap of 2^28 cells; else its cells are reported.

The vectors of `small` are those of tools/bench_align_band.py (align_reference.make, 16 distinct pairs repeated); those of
`long` are a random walk in the 64 compared columns.  No analysis runs; the time does not depend on the values.

Prints one JSON object: ms per call (wall: min / median / max over the steps after the warm-up), ms per call of each kernel
from HIP events (llsm_gpu_get_profile: min / median / max of one profiled call each), the cells searched, the ratios of the
medians and, for `long`, how far the found positions lie from the warp that made the pair.

    python tools/bench_align_around.py [--pairs 64] [--frames 2000] [--band 100] [--long-frames 60000] [--drift 0.05]
        [--decimate 16] [--around-band 64] [--steps 12] [--warmup 3] [--skip-small] [--skip-long] [--out FILE]
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
import align_band_reference as bref  # noqa: E402

FS = 44100.0
OSP, OBAP = 64, 5
DIM = OSP + OBAP + 3
CAP = 1 << 28


def spread(v):
    return dict(min=float(min(v)), median=float(np.median(v)), max=float(max(v)))


def batch_of(ctx, nfrm, code):
    b = llsm.Batch(ctx, llsm.make_aoptions(f0_refine=0), FS, [0] * len(nfrm), list(nfrm))
    b.enable_layer1(128); b.enable_coder(OSP, OBAP); b.upload(llsm.A_CODE, code)
    return b


def timed(ctx, calls, steps, warmup):
    """(wall ms, kernel ms, the last results) of calls that take turns"""
    last = {}
    for _ in range(warmup):
        for name, call in calls.items():
            last[name] = call()
    walls = {name: [] for name in calls}
    for _ in range(steps):                                 # wall time of the (synchronous) calls in turn, no events
        for name, call in calls.items():
            t0 = time.perf_counter(); call(); walls[name].append((time.perf_counter() - t0) * 1e3)
    kern = {name: {} for name in calls}
    ctx.set_profiling(True)
    for _ in range(steps):                                 # one profiled call at a time: the spread of each kernel
        for name, call in calls.items():
            ctx.reset_profile(); call()
            for k, v in ctx.profile().items():
                if v[1] > 0:
                    kern[name].setdefault(k, []).append(v[0] / v[1])
    ctx.set_profiling(False)
    return walls, kern, last


def small(ctx, a):
    n, F, band = a.pairs, a.frames, a.band
    ca = np.zeros((n * F, DIM), np.float32); cb = np.zeros((n * F, DIM), np.float32)
    for p in range(n):                                     # 16 distinct trajectories, repeated
        if p < 16:
            A, B, _ = aref.make(p, F, F, OSP, 0.3)
            ca[p * F:(p + 1) * F, 3:3 + OSP] = A; cb[p * F:(p + 1) * F, 3:3 + OSP] = B
        else:
            ca[p * F:(p + 1) * F] = ca[(p % 16) * F:(p % 16 + 1) * F]; cb[p * F:(p + 1) * F] = cb[(p % 16) * F:(p % 16 + 1) * F]
    qa, qb = batch_of(ctx, [F] * n, ca), batch_of(ctx, [F] * n, cb)
    idx = np.arange(n, dtype=np.int32)
    line = np.tile(np.array(bref.centers(F, F), np.int32), n)
    calls = {"align_band": lambda: qa.align_band(qb, idx, idx, band),
             "align_around_0": lambda: qa.align_around(qb, idx, idx, line, band),
             "align_band_slope": lambda: qa.align_band_slope(qb, idx, idx, band),
             "align_around_1": lambda: qa.align_around(qb, idx, idx, line, band, slope=True)}
    walls, kern, last = timed(ctx, calls, a.steps, a.warmup)
    out = dict(shape=dict(pairs=n, frames_a=F, frames_b=F, band=band, order_spec=OSP, order_bap=OBAP, first=3, count=OSP,
                          plane_cells=n * F * (2 * band + 1)))
    for name in calls:
        out[name] = dict(wall_ms=spread(walls[name]), kernels_ms={k: spread(v) for k, v in kern[name].items()})
    out["wall_ratio_around_over_straight"] = {"0": float(np.median(walls["align_around_0"]) / np.median(walls["align_band"])),
                                              "1": float(np.median(walls["align_around_1"]) / np.median(walls["align_band_slope"]))}
    out["same_bits"] = {s: bool(all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(last[u][0], last[v][0])) and
                                np.array_equal(last[u][1].view(np.uint32), last[v][1].view(np.uint32)))
                        for s, u, v in (("0", "align_around_0", "align_band"), ("1", "align_around_1", "align_band_slope"))}
    qa.close(); qb.close()
    return out


def long_pair(F, drift, seed=3):
    """(rows of take A, rows of take B, for every frame of A its position in B): B is A read along x + drift sin(2 pi x)"""
    rng = np.random.default_rng(seed)
    walk = np.cumsum(rng.standard_normal((F, OSP)).astype(np.float32), 0)
    x = np.arange(F) / (F - 1)
    t = np.clip(x + drift * np.sin(2 * np.pi * x), 0, 1) * (F - 1)      # frame of A that frame j of B shows
    k = np.minimum(np.floor(t).astype(np.int64), F - 2)
    w = (t - k).astype(np.float32)[:, None]
    ca = np.zeros((F, DIM), np.float32); cb = np.zeros((F, DIM), np.float32)
    ca[:, 3:3 + OSP] = walk
    cb[:, 3:3 + OSP] = walk[k] + (walk[k + 1] - walk[k]) * w + 0.05 * rng.standard_normal((F, OSP)).astype(np.float32)
    truth = np.interp(np.arange(F), t, np.arange(F))               # t is increasing for drift < 1 / (2 pi)
    return ca, cb, truth


def long(ctx, a):
    F, dec, half = a.long_frames, a.decimate, a.around_band
    ca, cb, truth = long_pair(F, a.drift)
    fa, fb = batch_of(ctx, [F], ca), batch_of(ctx, [F], cb)
    cca, ccb = np.ascontiguousarray(ca[::dec]), np.ascontiguousarray(cb[::dec])
    ka, kb = batch_of(ctx, [len(cca)], cca), batch_of(ctx, [len(ccb)], ccb)
    one = np.zeros(1, np.int32)
    state = {}

    def coarse():
        state["pos_c"] = ka.align_slope(kb, one, one)[0][0]
        return state["pos_c"]

    def line():
        state["line"] = llsm.align_center_line(state["pos_c"], len(ccb), F, F)
        return state["line"]

    def fine():
        return fa.align_around(fb, one, one, state["line"], half, slope=True)

    def pipeline():
        coarse(); line()
        return fine()

    calls = {"coarse_align_slope": coarse, "center_line": line, "fine_align_around": fine, "pipeline": pipeline}
    drift_frames = int(np.ceil(np.max(np.abs(truth - np.arange(F)))))
    straight_band = drift_frames + half                              # the straight band that holds the same paths
    straight_cells = F * (2 * straight_band + 1)
    if straight_cells <= CAP:
        calls["straight_align_band_slope"] = lambda: fa.align_band_slope(fb, one, one, straight_band)
    walls, kern, last = timed(ctx, calls, a.steps, a.warmup)
    pos, cost = last["pipeline"]
    lo, hi = llsm.align_around_rows(F, F, state["line"], half, slope=True)
    out = dict(shape=dict(frames=F, drift=a.drift, drift_frames=drift_frames, decimate=dec, coarse_frames=len(cca), around_band=half,
                          order_spec=OSP, order_bap=OBAP, first=3, count=OSP,
                          cells=dict(coarse_plane=len(cca) * len(ccb), fine_plane=F * (2 * half + 1),
                                     fine_region=int(np.sum(np.maximum(hi.astype(np.int64) - lo + 1, 0))),
                                     full_matrix=F * F, straight_band_plane=straight_cells),
                          straight_band=straight_band, straight_band_fits_cap=bool(straight_cells <= CAP), cap=CAP,
                          around_min=llsm.align_around_min(F, F, state["line"], slope=True),
                          line_from_diagonal=int(np.max(np.abs(state["line"].astype(np.int64) - np.arange(F))))))
    for name in calls:
        out[name] = dict(wall_ms=spread(walls[name]), kernels_ms={k: spread(v) for k, v in kern[name].items()})
    out["cost"] = float(cost[0])
    out["pos_from_warp"] = dict(max=float(np.max(np.abs(pos[0] - truth))), median=float(np.median(np.abs(pos[0] - truth))))
    out["pos_from_line"] = float(np.max(np.abs(pos[0] - state["line"])))      # (below around_band: the band did not bind)
    if "straight_align_band_slope" in calls:
        spos, scost = last["straight_align_band_slope"]
        out["straight_cost"] = float(scost[0])
        out["same_bits_as_straight"] = bool(np.array_equal(spos[0].view(np.uint32), pos[0].view(np.uint32)))
        out["wall_ratio_pipeline_over_straight"] = float(np.median(walls["pipeline"]) / np.median(walls["straight_align_band_slope"]))
    for b in (fa, fb, ka, kb):
        b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--band", type=int, default=100)
    ap.add_argument("--long-frames", type=int, default=60000)
    ap.add_argument("--drift", type=float, default=0.05)
    ap.add_argument("--decimate", type=int, default=16)
    ap.add_argument("--around-band", type=int, default=64)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-small", action="store_true")
    ap.add_argument("--skip-long", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = llsm.Context(0)
    out = {}
    if not a.skip_small:
        out["small"] = small(ctx, a)
    if not a.skip_long:
        out["long"] = long(ctx, a)
    ctx.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
