"""Times a device-side edit chain at the bench shape (1 024 utterances x 200 frames, F0 = 120 Hz, thop = 5 ms, layer 1 at
nfft = 2048).  --edit stretch (the default) stretches 2x:

    phasepropagate(-1) -> retime -> tolayer0(1) -> phasepropagate(+1) -> synthesize

--edit pitch shifts F0 by 1.5 and the formants by 1.2, PSD warped too:

    phasepropagate(-1) -> pitch_formant(1.5, 1.2, warp_psd) -> tolayer0(1) -> phasepropagate(+1) -> synthesize

--edit splice times llsm_gpu_batch_splice alone, beside retime on the same 2x map in the same process: the degenerate map
(no second side; its rows are compared bit for bit with retime's) and a full two-sided map (random utterances and
positions on both sides, mix in (0, 1)).

Each prints one JSON object: ms per call of each kernel of the chain (the context's per-launch HIP events), GB/s of the
edit kernels on unique bytes, the wall time of the chain, and the host round trip the device edit replaces (the rows
downloaded, edited in numpy by the same rules, uploaded again) on the same box.

    python tools/bench_modify.py [--edit stretch|pitch|splice] [--utts 1024] [--steps 5] [--warmup 2] [--nfft 2048] [--out FILE]
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

ROWS = llsm.Batch.PARAM_IDS + llsm.Batch.L1_IDS


def row_bytes(b, nspec):
    """bytes of one frame's parameter and layer-1 rows"""
    l = b.layout
    me = max(l.maxnhar_e, 1)
    words = 1 + 1 + 2 * l.maxnhar + 2 * l.npsd + 1 + l.nchannel + 1 + 2 * l.nchannel * me   # F0 .. EENV_PHSE
    words += 1 + nspec + l.maxnhar + 3                                                     # RD VTMAGN VSPHSE NVSPHSE PBPSYN HAS_HM
    return 4 * words


def numpy_retime(s, n_src, n_dst, n_utt, pos):
    """the retime rules vectorised over every output frame (uniform map: every utterance has the same frame counts)"""
    f32 = np.float32
    a = np.minimum(np.floor(pos).astype(np.int64), n_src - 2); b = a + 1
    r = (pos - a.astype(f32)).astype(f32)
    base = (np.arange(n_utt) * n_src)[:, None]
    ga, gb = (base + a[None, :]).ravel(), (base + b[None, :]).ravel()
    R = np.tile(r, n_utt)
    gr = (base + np.minimum(np.floor(pos).astype(np.int64), n_src - 1)[None, :]).ravel()
    out = {}
    col = lambda v, nd=2: v.reshape((-1,) + (1,) * (nd - 1))          # per-frame values against rows of nd dimensions
    lin = lambda x, y: x + (y - x) * col(R, x.ndim)
    fa, fb = s[llsm.A_F0][ga], s[llsm.A_F0][gb]
    va, vb = fa > 0, fb > 0
    both, one = va & vb, va ^ vb
    gv = np.where(va, ga, gb)
    copy = (R == 0) | (R == 1)
    gc = np.where(R == 1, gb, ga)
    for aid in ROWS:
        out[aid] = s[aid][gc].copy()
    out[llsm.A_PSDRES] = s[llsm.A_PSDRES][gr]; out[llsm.A_HAS_PSDRES] = s[llsm.A_HAS_PSDRES][gr]
    bl = ~copy
    w = np.where(va, f32(1) - R, R)
    fade = (20 * np.log10(np.maximum(1e-8, w))).astype(f32)
    vt = np.where(col(both), lin(s[llsm.A_VTMAGN][ga], s[llsm.A_VTMAGN][gb]),
                  np.where(col(one), s[llsm.A_VTMAGN][gv] + col(np.where(one, fade, f32(0))), s[llsm.A_VTMAGN][ga]))
    out[llsm.A_VTMAGN][bl] = np.maximum(vt, f32(-80))[bl]

    def circ(x, y):
        return np.arctan2(lin(np.sin(x), np.sin(y)), lin(np.cos(x), np.cos(y))).astype(f32)

    mh = s[llsm.A_VSPHSE].shape[1]
    nva, nvb = s[llsm.A_NVSPHSE][ga], s[llsm.A_NVSPHSE][gb]
    k = np.arange(mh)[None, :]
    vs_long = np.where(col(nva >= nvb), s[llsm.A_VSPHSE][ga], s[llsm.A_VSPHSE][gb])
    vs = np.where(k < np.minimum(nva, nvb)[:, None], circ(s[llsm.A_VSPHSE][ga], s[llsm.A_VSPHSE][gb]), vs_long)
    vs = np.where(col(both), vs, np.where(col(one), s[llsm.A_VSPHSE][gv], s[llsm.A_VSPHSE][ga]))
    out[llsm.A_VSPHSE][bl] = vs[bl]
    out[llsm.A_NVSPHSE][bl] = np.where(both, np.maximum(nva, nvb), np.where(one, s[llsm.A_NVSPHSE][gv], nva))[bl]
    out[llsm.A_F0][bl] = np.where(both, lin(fa, fb), np.where(one, s[llsm.A_F0][gv], 0))[bl]
    out[llsm.A_RD][bl] = np.where(both, lin(s[llsm.A_RD][ga], s[llsm.A_RD][gb]), np.where(one, s[llsm.A_RD][gv], 1))[bl]
    for aid in (llsm.A_PSD, llsm.A_EDC):
        out[aid][bl] = lin(s[aid][ga], s[aid][gb])[bl]
    nea, neb = s[llsm.A_NHAR_E][ga], s[llsm.A_NHAR_E][gb]
    ke = np.arange(s[llsm.A_EENV_AMPL].shape[2])[None, None, :]
    inner = ke < np.minimum(nea, neb)[:, None, None]
    gl = np.where(nea >= neb, ga, gb)
    out[llsm.A_EENV_AMPL][bl] = np.where(inner, lin(s[llsm.A_EENV_AMPL][ga], s[llsm.A_EENV_AMPL][gb]), s[llsm.A_EENV_AMPL][gl])[bl]
    out[llsm.A_EENV_PHSE][bl] = np.where(inner, circ(s[llsm.A_EENV_PHSE][ga], s[llsm.A_EENV_PHSE][gb]), s[llsm.A_EENV_PHSE][gl])[bl]
    out[llsm.A_NHAR_E][bl] = np.maximum(nea, neb)[bl]
    out[llsm.A_PBPSYN][bl] = s[llsm.A_PBPSYN][ga][bl]
    vo = bl & (va | vb)
    out[llsm.A_NHAR][vo] = 0; out[llsm.A_HAS_HM][vo] = 0; out[llsm.A_AMPL][vo] = 0; out[llsm.A_PHSE][vo] = 0
    uo = bl & ~(va | vb)
    for aid in (llsm.A_NHAR, llsm.A_AMPL, llsm.A_PHSE, llsm.A_HAS_HM):
        out[aid][uo] = s[aid][ga][uo]
    return out


def numpy_pitch(s, rho, alpha):
    """the pitch_formant rules for one F0 and one formant ratio over every frame, PSD warped (rows edited in place)"""
    rho, alpha = np.float32(rho), np.float32(alpha)         # the ratios as the C API takes them

    def warp(x):
        n = x.shape[1]
        p = np.arange(n, dtype=np.float64) / np.float64(alpha)
        i = np.floor(p).astype(np.int64)
        top = i >= n - 1
        ic = np.minimum(i, n - 2)
        r = (p - i).astype(np.float32)
        out = x[:, ic] + (x[:, ic + 1] - x[:, ic]) * r[None, :]
        out[:, top] = x[:, n - 1:n]
        return out
    v = s[llsm.A_F0] != 0
    s[llsm.A_PSD] = warp(s[llsm.A_PSD])
    vt = warp(s[llsm.A_VTMAGN][v]) if alpha != 1 else s[llsm.A_VTMAGN][v]
    s[llsm.A_VTMAGN][v] = (vt.astype(np.float64) - 20 * np.log10(np.float64(rho))).astype(np.float32)
    s[llsm.A_F0][v] *= np.float32(rho)
    s[llsm.A_NHAR][v] = 0; s[llsm.A_HAS_HM][v] = 0
    return s


PITCH_ROWS = (llsm.A_F0, llsm.A_NHAR, llsm.A_HAS_HM, llsm.A_VTMAGN, llsm.A_PSD)   # what pitch_formant reads and writes


def pitch_leg(a):
    n_utt, rho, alpha = a.utts, 1.5, 1.2
    x = make_batch_inputs(list(range(n_utt)), lambda u: 120.0, "cuda:0")
    ctx = llsm.Context(0)
    ao = llsm.make_aoptions(f0_refine=0)
    so = llsm.make_soptions(FS)
    b = llsm.Batch(ctx, ao, FS, [NX] * n_utt, [NFRM] * n_utt)
    b.upload(llsm.A_X, x.ravel()); b.upload(llsm.A_F0, np.full(n_utt * NFRM, 120.0, np.float32))
    b.analyze(); b.tolayer1(a.nfft)
    ctx.sync()
    # the rows the edit changes, kept in page-locked memory and put back between steps (outside the timed chains)
    keep = {aid: b.pinned_array(aid) for aid in PITCH_ROWS}
    for aid, arr in keep.items():
        b.download(aid, out=arr)

    def restore():
        for aid, arr in keep.items():
            b.upload(aid, arr)
        ctx.sync()

    def chain():
        b.phasepropagate(-1); b.pitch_formant(rho, alpha, warp_psd=True); b.tolayer0(True); b.phasepropagate(+1)
        b.synthesize(so, seed=1)

    for _ in range(a.warmup):
        restore(); chain()
    ctx.sync()
    walls = []
    for _ in range(a.steps):
        restore()
        t0 = time.perf_counter(); chain(); ctx.sync(); walls.append((time.perf_counter() - t0) * 1e3)
    ctx.set_profiling(True); ctx.reset_profile()
    for _ in range(a.steps):
        ctx.set_profiling(False); restore(); ctx.set_profiling(True)
        chain()
    ctx.sync()
    prof = ctx.profile()
    ctx.set_profiling(False)
    kern = {k: dict(ms_per_call=v[0] / v[1], calls_per_step=v[1] / a.steps) for k, v in prof.items() if v[1] > 0}
    F = n_utt * NFRM
    nspec, npsd = a.nfft // 2 + 1, b.layout.npsd
    nv = int((keep[llsm.A_F0] != 0).sum())
    # unique bytes of one call: both ratio rows and every F0 read; VTMAGN read + written, F0 written, NHAR and HAS_HM
    # written on voiced frames; PSD read + written on every frame
    uniq = F * (4 + 4 + 4) + nv * (2 * 4 * nspec + 4 + 4 + 4) + F * 2 * 4 * npsd
    out = dict(edit="pitch", rho=rho, alpha=alpha, warp_psd=True,
               shape=dict(utterances=n_utt, frames=F, voiced=nv, nfft=a.nfft, nspec=nspec, npsd=npsd),
               chain_wall_ms=dict(min=min(walls), median=float(np.median(walls)), max=max(walls)), kernels=kern)
    if "k_pitch_formant" in kern:
        t = kern["k_pitch_formant"]["ms_per_call"]
        out["pitch_formant"] = dict(ms=t, unique_gb=uniq / 1e9, gbs=uniq / t / 1e6)
    if a.host_reps > 0:
        # the host round trip the device edit replaces: the five rows down, numpy edit, rows up
        restore(); b.phasepropagate(-1); ctx.sync()
        hosts = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            s = {aid: b.download(aid) for aid in PITCH_ROWS}
            t1 = time.perf_counter()
            nbytes = sum(v.nbytes for v in s.values())
            s = numpy_pitch(s, rho, alpha)
            t2 = time.perf_counter()
            for aid in PITCH_ROWS:
                b.upload(aid, s[aid])
            ctx.sync()
            t3 = time.perf_counter()
            hosts.append(dict(download_ms=(t1 - t0) * 1e3, edit_ms=(t2 - t1) * 1e3, upload_ms=(t3 - t2) * 1e3,
                              total_ms=(t3 - t0) * 1e3, bytes=int(2 * nbytes)))
            restore(); b.phasepropagate(-1); ctx.sync()
        out["host_round_trip"] = min(hosts, key=lambda h: h["total_ms"])
        # the numpy rows agree with the device's
        b.pitch_formant(rho, alpha, warp_psd=True); ctx.sync()
        dev = {aid: b.download(aid) for aid in PITCH_ROWS}
        out["host_vs_device_max_abs"] = {str(k): float(np.abs(dev[k].astype(np.float64) - s[k]).max()) for k in dev}
    for arr in keep.values():
        b.free_pinned(arr)
    b.close(); ctx.close()
    return out


def splice_leg(a):
    n_utt, n2 = a.utts, 2 * NFRM
    x = make_batch_inputs(list(range(n_utt)), lambda u: 120.0, "cuda:0")
    ctx = llsm.Context(0)
    ao = llsm.make_aoptions(f0_refine=0)
    src = llsm.Batch(ctx, ao, FS, [NX] * n_utt, [NFRM] * n_utt)
    src.upload(llsm.A_X, x.ravel()); src.upload(llsm.A_F0, np.full(n_utt * NFRM, 120.0, np.float32))
    src.analyze(); src.tolayer1(a.nfft); src.phasepropagate(-1)
    ref = llsm.Batch(ctx, ao, FS, [0] * n_utt, [n2] * n_utt)
    dst = llsm.Batch(ctx, ao, FS, [0] * n_utt, [n2] * n_utt)
    ctx.sync()
    nspec = a.nfft // 2 + 1
    Fs, Fd = n_utt * NFRM, n_utt * n2
    rng = np.random.default_rng(1)
    pos = np.tile(llsm.retime_uniform_positions(NFRM, n2), n_utt)
    two = dict(utt_a=rng.integers(0, n_utt, Fd), pos_a=rng.uniform(0, NFRM - 1, Fd), utt_b=rng.integers(0, n_utt, Fd),
               pos_b=rng.uniform(0, NFRM - 1, Fd), mix=rng.uniform(0.01, 0.99, Fd))
    # a morph that keeps the locality of the stretch: both sides walk their utterances in order, side b one utterance on
    morph = dict(utt_a=np.repeat(np.arange(n_utt), n2), pos_a=pos, utt_b=np.repeat((np.arange(n_utt) + 1) % n_utt, n2),
                 pos_b=pos, mix=two["mix"])
    legs = dict(retime=lambda: ref.retime(src, pos), splice_one_side=lambda: dst.splice(src, pos),
                splice_morph=lambda: dst.splice(src, **morph), splice_two_sides_random=lambda: dst.splice(src, **two))
    for _ in range(a.warmup):
        for f in legs.values():
            f()
    ctx.sync()
    rb = row_bytes(src, nspec)
    out = dict(edit="splice", shape=dict(utterances=n_utt, frames_src=Fs, frames_dst=Fd, nfft=a.nfft, row_bytes=rb), legs={})
    for name, f in legs.items():                            # alternating, each leg's launches bracketed by events
        out["legs"][name] = dict(ms=[], wall_ms=[])
    for _ in range(a.steps):
        for name, f in legs.items():
            ctx.set_profiling(True); ctx.reset_profile()
            t0 = time.perf_counter(); f(); ctx.sync(); wall = (time.perf_counter() - t0) * 1e3
            prof = ctx.profile(); ctx.set_profiling(False)
            ms, calls = prof["k_splice"]                      # (every leg launches it: `retime` times retime's resolver)
            out["legs"][name]["ms"].append(ms / calls); out["legs"][name]["wall_ms"].append(wall)
    for name, d in out["legs"].items():
        # unique bytes: every source row read once, every output row written once, the map; the random two-sided map also
        # counts what it gathers (four source frames per output frame) since little of that is shared between neighbours
        words = 2 if name in ("retime", "splice_one_side") else 5
        uniq = Fs * rb + Fd * rb + Fd * 4 * words
        ms = float(np.median(d["ms"]))
        d.update(ms_median=ms, ms_min=min(d["ms"]), unique_gb=uniq / 1e9, tbs=uniq / ms / 1e9,
                 wall_ms_median=float(np.median(d["wall_ms"])))
        if name == "splice_two_sides_random":
            gath = 4 * Fd * rb + Fd * rb + Fd * 4 * words
            d.update(gathered_gb=gath / 1e9, gathered_tbs=gath / ms / 1e9)
    ref.retime(src, pos); dst.splice(src, pos); ctx.sync()
    ref.nspec = nspec
    out["one_side_equals_retime"] = all(np.array_equal(ref.download(aid).view(np.uint32), dst.download(aid).view(np.uint32))
                                        for aid in ROWS)
    if a.host_reps > 0:
        # the host round trip the call replaces: rows down, the same blend in numpy, rows up
        p1 = llsm.retime_uniform_positions(NFRM, n2)
        hosts = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            s = {aid: src.download(aid) for aid in ROWS}
            t1 = time.perf_counter()
            rows = numpy_retime(s, NFRM, n2, n_utt, p1)
            t2 = time.perf_counter()
            for aid in ROWS:
                dst.upload(aid, rows[aid])
            ctx.sync()
            t3 = time.perf_counter()
            hosts.append(dict(download_ms=(t1 - t0) * 1e3, blend_ms=(t2 - t1) * 1e3, upload_ms=(t3 - t2) * 1e3,
                              total_ms=(t3 - t0) * 1e3))
        out["host_round_trip"] = min(hosts, key=lambda h: h["total_ms"])
    for b in (src, ref, dst):
        b.close()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edit", choices=("stretch", "pitch", "splice"), default="stretch")
    ap.add_argument("--utts", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nfft", type=int, default=2048)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.edit in ("pitch", "splice"):
        line = json.dumps(pitch_leg(a) if a.edit == "pitch" else splice_leg(a))
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    n_utt, n2 = a.utts, 2 * NFRM
    x = make_batch_inputs(list(range(n_utt)), lambda u: 120.0, "cuda:0")
    ctx = llsm.Context(0)
    ao = llsm.make_aoptions(f0_refine=0)
    so = llsm.make_soptions(FS)
    src = llsm.Batch(ctx, ao, FS, [NX] * n_utt, [NFRM] * n_utt)
    src.upload(llsm.A_X, x.ravel()); src.upload(llsm.A_F0, np.full(n_utt * NFRM, 120.0, np.float32))
    src.analyze(); src.tolayer1(a.nfft)
    dst = llsm.Batch(ctx, ao, FS, [0] * n_utt, [n2] * n_utt)
    ctx.sync()
    nspec = a.nfft // 2 + 1

    def chain():
        src.phasepropagate(-1); dst.retime(src); dst.tolayer0(True); dst.phasepropagate(+1); dst.synthesize(so, seed=1)
        src.phasepropagate(+1)                              # (src back where it was: every step sees the same rows)

    for _ in range(a.warmup):
        chain()
    ctx.sync()
    walls = []
    for _ in range(a.steps):                               # wall time of the chain, no events
        t0 = time.perf_counter(); chain(); ctx.sync(); walls.append((time.perf_counter() - t0) * 1e3)
    ctx.set_profiling(True); ctx.reset_profile()
    for _ in range(a.steps):
        chain()
    ctx.sync()
    prof = ctx.profile()
    ctx.set_profiling(False)
    kern = {k: dict(ms_per_call=v[0] / v[1], calls_per_step=v[1] / a.steps) for k, v in prof.items() if v[1] > 0}

    Fs, Fd = n_utt * NFRM, n_utt * n2
    rb = row_bytes(src, nspec)
    l = src.layout
    me = max(l.maxnhar_e, 1)
    phase_words = 2 * l.maxnhar + l.nchannel * me          # PHSE, VSPHSE, EENV_PHSE entries a shift reads and writes
    uniq = Fs * rb + Fd * rb + Fd * 4 * 2                  # every source row read once, every output row written once, the map
    out = dict(shape=dict(utterances=n_utt, frames_src=Fs, frames_dst=Fd, nfft=a.nfft, row_bytes=rb),
               chain_wall_ms=dict(min=min(walls), median=float(np.median(walls)), max=max(walls)), kernels=kern)
    if "k_splice" in kern:
        t = kern["k_splice"]["ms_per_call"]
        out["retime"] = dict(ms=t, unique_gb=uniq / 1e9, gbs=uniq / t / 1e6)
    if "k_phase_shift" in kern:
        t = kern["k_phase_shift"]["ms_per_call"]
        Fm = (2 * Fs + Fd) / 3                              # two calls on src, one on dst per step
        byt = Fm * (2 * 4 * phase_words + 4 * 6)            # phase rows read + written, counts and F0 read
        out["phase_shift"] = dict(ms=t, unique_gb_avg=byt / 1e9, gbs=byt / t / 1e6)
    if "k_prop_theta" in kern:
        out["prop_theta"] = dict(ms=kern["k_prop_theta"]["ms_per_call"])

    # ---- the host round trip the device retime replaces: rows down, numpy blend, rows up (--host-reps 0: skipped)
    if a.host_reps <= 0:
        src.close(); dst.close(); ctx.close()
        print(json.dumps(out))
        return
    src.phasepropagate(-1); ctx.sync()
    pos = llsm.retime_uniform_positions(NFRM, n2)
    src.nspec = dst.nspec = nspec
    hosts = []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        s = {aid: src.download(aid) for aid in ROWS}
        t1 = time.perf_counter()
        rows = numpy_retime(s, NFRM, n2, n_utt, pos)
        t2 = time.perf_counter()
        for aid in ROWS:
            dst.upload(aid, rows[aid])
        ctx.sync()
        t3 = time.perf_counter()
        hosts.append(dict(download_ms=(t1 - t0) * 1e3, blend_ms=(t2 - t1) * 1e3, upload_ms=(t3 - t2) * 1e3,
                          total_ms=(t3 - t0) * 1e3, bytes=int(sum(v.nbytes for v in s.values()) + sum(v.nbytes for v in rows.values()))))
    out["host_round_trip"] = min(hosts, key=lambda h: h["total_ms"])
    # the numpy rows agree with the device's (same rules; circular blends to float32 rounding)
    dst.retime(src); ctx.sync()
    dev = {aid: dst.download(aid) for aid in (llsm.A_F0, llsm.A_VTMAGN, llsm.A_PSD, llsm.A_NHAR)}
    out["host_vs_device_max_abs"] = {str(k): float(np.abs(dev[k].astype(np.float64) - rows[k]).max()) for k in dev}
    src.close(); dst.close(); ctx.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
