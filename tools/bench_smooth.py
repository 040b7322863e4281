"""Times llsm_gpu_batch_smooth at the bench shape (1 024 utterances x 200 frames, F0 = 120 Hz, thop = 5 ms, layer 1 at
nfft = 2048), every track flagged, in three legs:

    joins      a join every 20 frames (llsm_gpu_join_radii on such an index list, reach 8)
    radius8    every frame at radius 8
    radius32   every frame at radius 32

Prints one JSON object: per leg the HIP-event ms per launch of k_smooth_rows and k_smooth_store (the context's per-launch
events), the wall time of a call, the unique bytes of the two kernels (every source row of a window once, the scratch rows
written and read, the batch rows written), the bytes k_smooth_rows gathers (every tile walks its own span of source rows),
TB/s on both counts, and beside them the host round trip the call replaces on the same box: the five rows downloaded,
smoothed in numpy by the same rule in the same order of additions, uploaded again -- and whether its rows equal the
device's bit for bit.

    python tools/bench_smooth.py [--utts 1024] [--steps 5] [--warmup 2] [--nfft 2048] [--host-reps 1] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import libllsm2_amd as llsm  # noqa: E402
from bench import FS, NFRM, NX, make_batch_inputs  # noqa: E402

TILE = 16                                                   # kSmoothTile of csrc/kernels.h
TRACKS = (llsm.A_F0, llsm.A_RD, llsm.A_VTMAGN, llsm.A_PSD, llsm.A_EDC)
EDITED = TRACKS + (llsm.A_NHAR, llsm.A_HAS_HM)              # what the call writes


def windows(f0, n_utt, nfrm, radius):
    """rule S2 for utterances of equal length: (lo, hi) flat frames of every frame's window"""
    F = n_utt * nfrm
    g = np.arange(F)
    v = f0 != 0
    first = (g % nfrm == 0) | np.concatenate([[True], v[1:] != v[:-1]])       # first frame of a voicing run
    run_lo = np.maximum.accumulate(np.where(first, g, 0))
    last = np.concatenate([first[1:], [True]])
    run_hi = np.minimum.accumulate(np.where(last, g, F)[::-1])[::-1]
    return np.maximum(run_lo, g - radius), np.minimum(run_hi, g + radius)


def numpy_smooth(s, n_utt, nfrm, radius, chunk=32):
    """the rule over every frame: float64, ascending j with one addition per term (offset d = j - i from -R to R), chunks of
    `chunk` utterances at a time; rows edited in place"""
    F = n_utt * nfrm
    lo, hi = windows(s[llsm.A_F0], n_utt, nfrm, radius)
    hit = (radius > 0) & (hi > lo)
    voiced = s[llsm.A_F0] != 0
    rmax = int(radius.max())
    src = {aid: s[aid].copy() for aid in TRACKS}                                 # the snapshot
    for c0 in range(0, n_utt, chunk):
        a, e = c0 * nfrm, min(n_utt, c0 + chunk) * nfrm
        g = np.arange(a, e)
        wsum = np.zeros(e - a, np.float64)
        acc = {aid: np.zeros((e - a,) + src[aid].shape[1:], np.float64) for aid in TRACKS}
        for d in range(-rmax, rmax + 1):
            j = g + d
            on = hit[a:e] & (j >= lo[a:e]) & (j <= hi[a:e])
            if not on.any():
                continue
            w = np.where(on, radius[a:e] + 1 - abs(d), 0).astype(np.float64)
            jj = np.clip(j, a, e - 1)                                            # (a window never leaves its utterance)
            wsum += w
            for aid in TRACKS:
                x = src[aid][jj].astype(np.float64)
                acc[aid][on] = acc[aid][on] + (w.reshape((-1,) + (1,) * (x.ndim - 1)) * x)[on]
        for aid in TRACKS:
            m = hit[a:e] & (voiced[a:e] if aid in (llsm.A_F0, llsm.A_RD, llsm.A_VTMAGN) else True)
            out = (acc[aid][m] / wsum[m].reshape((-1,) + (1,) * (acc[aid].ndim - 1))).astype(np.float32)
            s[aid][a:e][m] = out
    s[llsm.A_NHAR][hit & voiced] = 0; s[llsm.A_HAS_HM][hit & voiced] = 0
    return s


def traffic(f0, n_utt, nfrm, radius, row_w):
    """(unique, gathered) bytes of one call: tiles are runs of up to TILE consecutive listed frames of one utterance"""
    lo, hi = windows(f0, n_utt, nfrm, radius)
    listed = radius > 0
    n_listed = int(listed.sum())
    read = np.zeros(n_utt * nfrm + 1, np.int64)
    np.add.at(read, lo[listed], 1); np.add.at(read, hi[listed] + 1, -1)
    rows_read = int((np.cumsum(read)[:-1] > 0).sum())
    gathered = 0
    for u in range(n_utt):
        idx = np.flatnonzero(listed[u * nfrm:(u + 1) * nfrm]) + u * nfrm
        if not idx.size:
            continue
        for run in np.split(idx, np.flatnonzero(np.diff(idx) != 1) + 1):
            for t in range(0, len(run), TILE):
                fr = run[t:t + TILE]
                gathered += int(hi[fr].max() - lo[fr].min() + 1)
    fixed = 3 * n_listed * row_w * 4                          # scratch written, scratch read, batch rows written
    return rows_read * row_w * 4 + fixed, gathered * row_w * 4 + fixed, n_listed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nfft", type=int, default=2048)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n_utt = a.utts
    F = n_utt * NFRM
    x = make_batch_inputs(list(range(n_utt)), lambda u: 120.0, "cuda:0")
    ctx = llsm.Context(0)
    ao = llsm.make_aoptions(f0_refine=0)
    b = llsm.Batch(ctx, ao, FS, [NX] * n_utt, [NFRM] * n_utt)
    b.upload(llsm.A_X, x.ravel()); b.upload(llsm.A_F0, np.full(F, 120.0, np.float32))
    b.analyze(); b.tolayer1(a.nfft)
    ctx.sync()
    keep = {aid: b.download(aid) for aid in EDITED}

    def restore():
        for aid, arr in keep.items():
            b.upload(aid, arr)
        ctx.sync()

    # an index list that hops to the next utterance every 20 frames, as select returns one
    i = np.arange(NFRM)
    utt = ((np.arange(n_utt)[:, None] + i[None, :] // 20) % n_utt).astype(np.int32).ravel()
    pos = np.tile(i, n_utt).astype(np.float32)
    r_join, joins = llsm.join_radii([NFRM] * n_utt, pos, utt, reach=8)
    legs = dict(joins=r_join, radius8=np.full(F, 8, np.int32), radius32=np.full(F, 32, np.int32))
    nspec, l = a.nfft // 2 + 1, b.layout
    row_w = nspec + l.npsd + l.nchannel + 2
    out = dict(edit="smooth", flags=llsm.SMOOTH_ALL,
               shape=dict(utterances=n_utt, frames=F, nfft=a.nfft, nspec=nspec, npsd=l.npsd, row_bytes=4 * row_w,
                          joins=joins), legs={})
    for _ in range(a.warmup):
        for r in legs.values():
            b.smooth(r)
    ctx.sync()
    for name in legs:
        out["legs"][name] = dict(rows_ms=[], store_ms=[], wall_ms=[])
    for _ in range(a.steps):                                 # alternating, each leg's launches bracketed by events
        for name, r in legs.items():
            ctx.set_profiling(True); ctx.reset_profile()
            t0 = time.perf_counter(); b.smooth(r); ctx.sync(); wall = (time.perf_counter() - t0) * 1e3
            prof = ctx.profile(); ctx.set_profiling(False)
            d = out["legs"][name]
            d["rows_ms"].append(prof["k_smooth_rows"][0] / prof["k_smooth_rows"][1])
            d["store_ms"].append(prof["k_smooth_store"][0] / prof["k_smooth_store"][1])
            d["wall_ms"].append(wall)
    for name, r in legs.items():
        d = out["legs"][name]
        uniq, gath, n_listed = traffic(keep[llsm.A_F0], n_utt, NFRM, r, row_w)
        rows_ms, store_ms = float(np.median(d["rows_ms"])), float(np.median(d["store_ms"]))
        ms = rows_ms + store_ms
        d.update(listed_frames=n_listed, rows_ms_median=rows_ms, store_ms_median=store_ms, ms_median=ms,
                 wall_ms_median=float(np.median(d["wall_ms"])), unique_gb=uniq / 1e9, gathered_gb=gath / 1e9,
                 unique_tbs=uniq / ms / 1e9, gathered_tbs=gath / ms / 1e9)
        if a.host_reps > 0:
            hosts = []
            for _ in range(a.host_reps):
                restore()
                t0 = time.perf_counter()
                s = {aid: b.download(aid) for aid in EDITED}
                t1 = time.perf_counter()
                s = numpy_smooth(s, n_utt, NFRM, r)
                t2 = time.perf_counter()
                for aid in EDITED:
                    b.upload(aid, s[aid])
                ctx.sync()
                t3 = time.perf_counter()
                hosts.append(dict(download_ms=(t1 - t0) * 1e3, edit_ms=(t2 - t1) * 1e3, upload_ms=(t3 - t2) * 1e3,
                                  total_ms=(t3 - t0) * 1e3))
            d["host_round_trip"] = min(hosts, key=lambda h: h["total_ms"])
            restore(); b.smooth(r); ctx.sync()
            d["host_equals_device"] = all(np.array_equal(b.download(aid).view(np.uint32), s[aid].view(np.uint32))
                                          for aid in EDITED)
    restore()
    b.close(); ctx.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
