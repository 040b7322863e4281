"""Times llsm_gpu_batch_align_band (pairs of frames x frames, coder orders 64 + 5, default options: the 64 mel-spectrum
columns, no step or voicing cost) and, with --full, llsm_gpu_batch_align on the same pairs in the same process, the two calls
taking turns so that both see the same state of the machine.

The vectors are align_reference.make trajectories in the 64 compared columns (a warped pair per utterance, 16 distinct pairs
repeated), uploaded into batches without samples; no analysis runs.  The generator warps by up to an eighth of the length,
which a narrow band does not hold: the banded path then runs along the band's edge.  The time does not depend on the values.

Prints one JSON object: ms per call (wall: min / median / max over the steps after the warm-up), ms per call of each kernel
from HIP events (llsm_gpu_get_profile: min / median / max of one profiled call each), the cells and the scratch bytes of the
call COMPUTED from the shapes by the rules of align.cpp (not read from the allocator), and with --full the ratio of the two
medians and on how many pairs the banded positions equal the full ones.  --calls K gives the pairs to K calls of pairs / K
each, one after the other, for lists whose band planes pass the 2^28 cells of one call; the wall time is that of all K, the
kernel times are per launch, the scratch is that of one call.

    python tools/bench_align_band.py [--pairs 64] [--frames 2000] [--band 100] [--calls 1] [--full] [--steps 12] [--warmup 3]
                                     [--out FILE]
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


def band_scratch(n, F, band):
    """the scratch of a call of n pairs of F x F frames: planes, moves (16 bytes per anti-diagonal of a strip's window),
    hand-over rows, positions and costs"""
    lo, hi = llsm.align_band_rows(F, F, band)
    widest = max(int(hi[min(i + 63, F - 1)]) - int(lo[i]) + 1 + min(i + 63, F - 1) - i for i in range(0, F, 64))
    cells = n * F * (2 * band + 1)
    return cells, dict(plane=4 * cells, moves=16 * n * ((F + 63) // 64) * widest, hand_rows=4 * n * F, out=4 * n * (F + 1))


def full_scratch(n, F):
    cells = n * F * F
    return cells, dict(plane=4 * cells, moves=16 * n * ((F + 63) // 64) * (F + 63), hand_rows=4 * n * F, out=4 * n * (F + 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--band", type=int, default=100)
    ap.add_argument("--calls", type=int, default=1)
    ap.add_argument("--full", action="store_true")
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
    assert n % a.calls == 0
    parts = np.split(idx, a.calls)

    def align_band():
        got = [qa.align_band(qb, part, part, band) for part in parts]
        return sum((g[0] for g in got), []), np.concatenate([g[1] for g in got])
    calls = {"align_band": align_band}
    if a.full:
        calls["align"] = lambda: qa.align(qb, idx, idx)
    last = {}
    for _ in range(a.warmup):
        for name, call in calls.items():
            last[name] = call()
    walls = {name: [] for name in calls}
    for _ in range(a.steps):                               # wall time of the (synchronous) calls in turn, no events
        for name, call in calls.items():
            t0 = time.perf_counter(); call(); walls[name].append((time.perf_counter() - t0) * 1e3)
    kern = {}
    ctx.set_profiling(True)
    for _ in range(a.steps):                               # one profiled call at a time: the spread of each kernel
        for name, call in calls.items():
            ctx.reset_profile(); call()
            for k, v in ctx.profile().items():
                if v[1] > 0:
                    kern.setdefault(k, []).append(v[0] / v[1])
    ctx.set_profiling(False)
    cells, scratch = band_scratch(n // a.calls, F, band)
    out = dict(shape=dict(pairs=n, calls=a.calls, frames_a=F, frames_b=F, band=band, order_spec=OSP, order_bap=OBAP, first=3, count=OSP),
               align_band=dict(cells=cells, scratch_bytes_computed=scratch, scratch_bytes_computed_sum=sum(scratch.values()),
                               wall_ms=spread(walls["align_band"])),
               kernels_ms={k: spread(v) for k, v in kern.items()})
    if a.full:
        cells_full, scratch_full = full_scratch(n, F)
        out["align"] = dict(cells=cells_full, scratch_bytes_computed=scratch_full, scratch_bytes_computed_sum=sum(scratch_full.values()),
                            wall_ms=spread(walls["align"]))
        out["wall_ratio_full_over_band"] = float(np.median(walls["align"]) / np.median(walls["align_band"]))
        out["cells_ratio_full_over_band"] = cells_full / (cells * a.calls)
        out["pairs_with_equal_positions"] = int(sum(np.array_equal(x, y) for x, y in zip(last["align"][0], last["align_band"][0])))
    qa.close(); qb.close(); ctx.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
