"""Times llsm_gpu_batch_select at the bench shape (1 024 target utterances of 200 frames against a bank of 64 utterances of
200 frames, coder orders 64 + 5, the 64 mel-spectrum columns, join_cost 1) and against one larger bank, and, beside it on
the same box, the host round trip the call replaces: download LLSM_GPU_CODE of both batches, the numpy reference
(tests/select_reference.py) on a few target utterances against the whole bank SCALED to the number of utterances, upload
of the map.

The vectors are align_reference.make trajectories in the 64 compared columns (16 distinct ones, repeated: the time of the
search does not depend on the values), uploaded into batches without samples; no analysis runs.

Prints one JSON object: per bank the ms per call (wall: min / median / max over the steps after the warm-up), the ms per
call of each kernel from HIP events (llsm_gpu_get_profile: min / median / max of one profiled call each), and the rate of
k_select_knn as operations per second from 3 x count x T x N and as a fraction of the fp32 vector peak; and the host round
trip with its scaling stated.

With --chain every bank also gets a "chain" entry: llsm_gpu_batch_select_chain on the same batches with the same options,
timed the same way in the same process (wall and per-kernel spreads; k_select_chain stands where k_select_join and
k_select_path stand for select), whether every cost is at most select's, and the joins both results pay.

    python tools/bench_select.py [--utts 1024] [--frames 200] [--bank-utts 64] [--big-bank-utts 256] [--steps 10]
                                 [--warmup 2] [--cpu-utts 2] [--chain] [--out FILE]
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
import select_reference as sref  # noqa: E402
import select_chain_reference as cref  # noqa: E402

FS = 44100.0
OSP, OBAP = 64, 5
PEAK_FP32_VECTOR = 157.3e12                    # MI355X, a fused multiply-add counted as two operations


def spread(v):
    return dict(min=float(min(v)), median=float(np.median(v)), max=float(max(v)))


def code_of(n, F, which):
    dim = OSP + OBAP + 3
    c = np.zeros((n * F, dim), np.float32)
    for p in range(min(n, 16)):
        c[p * F:(p + 1) * F, 3:3 + OSP] = aref.make(p, F, F, OSP, 0.3)[which]
    for p in range(16, n):
        c[p * F:(p + 1) * F] = c[(p % 16) * F:(p % 16 + 1) * F]
    return c


def batch_of(ctx, n, F, code):
    b = llsm.Batch(ctx, llsm.make_aoptions(f0_refine=0), FS, [0] * n, [F] * n)
    b.enable_layer1(128); b.enable_coder(OSP, OBAP); b.upload(llsm.A_CODE, code)
    return b


def time_call(ctx, call, steps, warmup):
    for _ in range(warmup):
        res = call()
    walls = []
    for _ in range(steps):                                 # wall time of the (synchronous) call, no events
        t0 = time.perf_counter(); call(); walls.append((time.perf_counter() - t0) * 1e3)
    kern = {}
    ctx.set_profiling(True)
    for _ in range(steps):                                 # one profiled call at a time: the spread of each kernel
        ctx.reset_profile(); call()
        for k, v in ctx.profile().items():
            if v[1] > 0:
                kern.setdefault(k, []).append(v[0] / v[1])
    ctx.set_profiling(False)
    return res, walls, kern


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--bank-utts", type=int, default=64)
    ap.add_argument("--big-bank-utts", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-utts", type=int, default=2)
    ap.add_argument("--chain", action="store_true", help="time llsm_gpu_batch_select_chain at the same shapes as well")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, F = a.utts, a.frames
    ctx = llsm.Context(0)
    t = batch_of(ctx, n, F, code_of(n, F, 0))
    out = dict(shape=dict(target_utts=n, frames=F, target_frames=n * F, order_spec=OSP, order_bap=OBAP, first=3, count=OSP,
                          join_cost=1.0), banks=[])
    bank = None
    for nb in [a.bank_utts] + ([a.big_bank_utts] if a.big_bank_utts > 0 else []):
        if bank is not None:
            bank.close()
        bank = batch_of(ctx, nb, F, code_of(nb, F, 1))
        steps = a.steps if nb == a.bank_utts else max(2, a.steps // 3)
        r, walls, kern = time_call(ctx, lambda: t.select(bank, join_cost=1.0), steps, a.warmup if nb == a.bank_utts else 1)
        T, N = n * F, nb * F
        wall = float(np.median(walls))
        row = dict(bank_utts=nb, bank_frames=N, distances=T * N, wall_ms=spread(walls), kernels_ms={k: spread(v) for k, v in kern.items()},
                   kernels_ms_sum=float(sum(np.median(v) for v in kern.values())), target_frames_per_s=T / (wall * 1e-3))
        if "k_select_knn" in kern:
            ops = 3.0 * OSP * T * N / (np.median(kern["k_select_knn"]) * 1e-3)
            row["knn_ops_per_s"] = ops
            row["knn_fraction_of_fp32_vector_peak"] = ops / PEAK_FP32_VECTOR
            row["knn_note"] = ("3 x count x T x N operations; the peak of %.1f TFLOP/s counts a fused multiply-add as two, and the "
                               "rule forbids the fusion, so one half of it is the ceiling of this kernel" % (PEAK_FP32_VECTOR / 1e12))
        if a.chain:
            rc, cwalls, ckern = time_call(ctx, lambda: t.select_chain(bank, join_cost=1.0), steps, a.warmup if nb == a.bank_utts else 1)
            row["chain"] = dict(wall_ms=spread(cwalls), kernels_ms={k: spread(v) for k, v in ckern.items()},
                                kernels_ms_sum=float(sum(np.median(v) for v in ckern.values())),
                                target_frames_per_s=T / (float(np.median(cwalls)) * 1e-3),
                                every_cost_at_most_selects=bool(np.all(rc[2] <= r[2])),
                                joins_select=int(cref.joins_of(r[0], r[1], t.frm_off, bank.frm_off).sum()),
                                joins_chain=int(cref.joins_of(rc[0], rc[1], t.frm_off, bank.frm_off).sum()))
        out["banks"].append(row)
        if nb == a.bank_utts and a.cpu_utts > 0:           # the host round trip the call replaces, on this bank
            m = min(a.cpu_utts, n)
            t0 = time.perf_counter(); dt = t.download(llsm.A_CODE); db = bank.download(llsm.A_CODE); t_down = time.perf_counter() - t0
            t0 = time.perf_counter()
            ref = sref.select(dt[:m * F], t.frm_off[:m + 1], db, bank.frm_off, 3, OSP, join_cost=1.0)
            t_ref = time.perf_counter() - t0
            same = bool(np.array_equal(ref[0], r[0][:m * F]) and np.array_equal(ref[1], r[1][:m * F]) and np.array_equal(ref[2], r[2][:m]))
            # the map itself, utt (int32) and pos (float32), into rows of those types of a batch shaped like t, made for this
            scratch = llsm.Batch(ctx, llsm.make_aoptions(f0_refine=0, maxnhar=1, maxnhar_e=1, npsd=2), FS, [0] * n, [F] * n)
            ctx.sync()
            t0 = time.perf_counter(); scratch.upload(llsm.A_NHAR, r[0]); scratch.upload(llsm.A_F0, r[1]); ctx.sync()
            t_up = time.perf_counter() - t0
            scratch.close()
            out["host_round_trip"] = dict(download_code_ms=t_down * 1e3, numpy_reference_utts=m, numpy_reference_ms_measured=t_ref * 1e3,
                                          numpy_reference_ms_scaled_to_all_utts=t_ref * 1e3 * n / m, upload_map_ms=t_up * 1e3,
                                          total_ms_scaled=t_down * 1e3 + t_ref * 1e3 * n / m + t_up * 1e3,
                                          note="the numpy time is measured on %d utterances on one CPU core and scaled by %d / %d" % (m, n, m),
                                          reference_equals_device=same)
    t.close(); bank.close(); ctx.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
