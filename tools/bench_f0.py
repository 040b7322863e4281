"""Times llsm_gpu_batch_estimate_f0 at the bench shape (1 024 utterances x 200 frames, 44.1 kHz, thop = 5 ms, default
options: 2 048-point transforms) and, beside it on the same box, the frames per second of the Python estimator it replaces
(yin_track of tests/golden/make_f0_track.py on one CPU core, over a short stretch of one utterance).  With --track,
llsm_gpu_batch_track_f0 is timed the same way on the same batch in the same run, after the estimator.

Prints one JSON object: ms per call (wall, and the sum of the kernels' HIP events), ms per call of each kernel
(llsm_gpu_get_profile), frames per second of both, and the share of voiced frames found; with --track the same figures
of the tracker under "track" (its CMNDF kernel is listed as k_f0_cmndf_wf_cand).

    python tools/bench_f0.py [--utts 1024] [--steps 5] [--warmup 2] [--cpu-frames 40] [--keep-cmndf] [--track] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import libllsm2_amd as llsm  # noqa: E402
from bench import FS, NFRM, NX, THOP, make_batch_inputs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-frames", type=int, default=40)
    ap.add_argument("--keep-cmndf", action="store_true")
    ap.add_argument("--track", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n_utt = a.utts
    x = make_batch_inputs(list(range(n_utt)), lambda u: 120.0, "cuda:0")
    ctx = llsm.Context(0)
    b = llsm.Batch(ctx, llsm.make_aoptions(thop=THOP), FS, [NX] * n_utt, [NFRM] * n_utt)
    b.upload(llsm.A_X, x.ravel())
    opts = dict(keep_cmndf=int(a.keep_cmndf))
    plan = llsm.f0_plan(FS)
    F = n_utt * NFRM

    def measure(call):
        for _ in range(a.warmup):
            call()
        ctx.sync()
        walls = []
        for _ in range(a.steps):                           # wall time of the call, no events
            t0 = time.perf_counter(); call(); ctx.sync(); walls.append((time.perf_counter() - t0) * 1e3)
        ctx.set_profiling(True); ctx.reset_profile()
        for _ in range(a.steps):
            call()
        ctx.sync()
        prof = ctx.profile()
        ctx.set_profiling(False)
        kern = {k: v[0] / v[1] for k, v in prof.items() if v[1] > 0}
        f0 = b.download(llsm.A_F0)
        wall = float(np.median(walls))
        return dict(wall_ms=dict(min=min(walls), median=wall, max=max(walls)), kernels_ms=kern, kernels_ms_sum=sum(kern.values()),
                    frames_per_s=F / (wall * 1e-3), voiced_share=float(np.count_nonzero(f0)) / F,
                    f0_median=float(np.median(f0[f0 > 0])) if np.any(f0 > 0) else 0.0)

    out = dict(shape=dict(utterances=n_utt, frames=F, fs=FS, thop=THOP, **plan), keep_cmndf=bool(a.keep_cmndf),
               **measure(lambda: b.estimate_f0(**opts)))
    if a.track:
        out["track"] = measure(lambda: b.track_f0(opts))
    b.close(); ctx.close()
    if a.cpu_frames > 0:
        from make_f0_track import yin_track
        nhop = int(round(THOP * FS))
        seg = x[0, : a.cpu_frames * nhop].astype(np.float64)
        t0 = time.perf_counter(); yin_track(seg, FS, nhop=nhop); dt = time.perf_counter() - t0
        out["yin_track_cpu"] = dict(frames=a.cpu_frames, seconds=dt, frames_per_s=a.cpu_frames / dt)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
