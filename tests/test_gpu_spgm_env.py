"""-m gpu: k_spgm_env_wf<LOGN, LOGF, FIX> and k_spgm_env on THEIR OWN input against float64, value by value.

Plane 0 of llsm_gpu_batch_debug_plane is the log envelope behind the Kalman process variance (layer0.c:324-345).  Its
input is what the caller uploads (A_X, A_F0), so the float64 reference needs no downloaded intermediate.  The whole-chain
PSD parity sees this plane through the smoother, with bounds up to 1 dB next to DC and Nyquist, and
tests/test_gpu_invariance.py looks at two points of one pinned frame per case: an error of 1e-3 nepers over a few bins
passes both.  Here every (frame, point) is held to spgm_env_ref(float64) under spgm_env_check
(tests/spgm_env_reference.py, whose docstring carries the bound B, the derivation of EPS_X and of the floor A term by
term, and KAPPA; proven against the oracle by tests/test_spgm_env_host.py):

    (a) |plane0 - ref| <= B at every point, nothing excluded;
    (b) rms_j(plane0 - ref) <= KAPPA rms_j(B) per frame.

No constant is calibrated on a kernel.  The configurations are the smallest that reach every instantiation of the
register-resident kernel and every path of the LDS one (spgm_env_reference.CONFIGS; the host test checks each against
the launcher's size rule), and the profile must show the kernel meant.  The utterances (spgm_env_inputs): an F0 that
changes every frame and a flat one (the seed cache misses and hits), exactly 200.0 Hz voiced beside unvoiced (the same
f0n bits, different window lengths), 50 Hz (time-aliased windows), windows over both ends, an utterance shorter than a
window between loud neighbours, silence, a single frame.  Every batch is first analysed on another signal of ten times
the level: a row left unwritten lands far outside the bound.

What the kernels measure against these bounds: the table in DESIGN.md section 8."""
import math

import numpy as np
import pytest

import libllsm2_amd as llsm
from gpu_common import report
from spgm_env_reference import (CONFIGS, I_LOW, I_SHORT, I_SPEECH, I_ZERO, NAMES, cache_pair, config_options, frame_index,
                                loud_inputs, offsets, spgm_env_bound, spgm_env_check, spgm_env_inputs)
from test_invariance_host import WF_REFERENCE_CASE, case_signal, takes_fallback

pytestmark = pytest.mark.gpu


def run_batch(ctx, fs, thop, kw, xs, f0s, stale_first=True):
    """one batch: analysed on the loud signal, then on xs with profiling on; plane 0 downloaded"""
    ao = llsm.make_aoptions(f0_refine=0, thop=thop, **kw)
    b = llsm.Batch(ctx, ao, fs, [len(x) for x in xs], [len(f) for f in f0s])
    try:
        b.upload(llsm.A_F0, np.concatenate(f0s))
        if stale_first:
            b.upload(llsm.A_X, np.concatenate(loud_inputs(xs)))
            b.analyze()
        b.upload(llsm.A_X, np.concatenate(xs))
        ctx.set_profiling(True); ctx.reset_profile()
        try:
            b.analyze(); ctx.sync()
            prof = ctx.profile()
        finally:
            ctx.set_profiling(False)
        F = sum(len(f) for f in f0s)
        assert np.array_equal(b.x_off, offsets(xs)) and np.array_equal(b.frm_off, offsets(f0s))
        assert np.array_equal(b.download(llsm.A_F0), np.concatenate(f0s))                    # (f0_refine = 0: F0 is an input)
        return dict(prof=prof, env=b.debug_plane(0).reshape(F, -1), frm_off=offsets(f0s))
    finally:
        b.close()


@pytest.fixture(scope="module")
def ctx():
    c = llsm.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def runs(ctx):
    """one batch per configuration, analysed once and shared"""
    cache = {}

    def get(cid):
        if cid not in cache:
            fs, thop, kw = config_options(cid)
            xs, f0s = spgm_env_inputs(cid)
            cache[cid] = run_batch(ctx, fs, thop, kw, xs, f0s)
        return cache[cid]
    return get


def _launches(prof, name):
    return prof.get(name, (0, 0))[1]


def _name_frames(st, frm_off):
    utt, idx = frame_index(frm_off)
    for key in ("ratio_point_at", "ratio_frame_at"):
        g = st[key][0] if isinstance(st[key], tuple) else st[key]
        st[key + "_utt"] = "%s[%d]" % (NAMES[int(utt[g])], int(idx[g]))


@pytest.mark.parametrize("cid", list(CONFIGS))
def test_envelope_on_its_own_input(runs, cid):
    """plane 0 of every frame and point against float64 of the uploaded samples and F0: (a) pointwise, (b) per frame"""
    fs, thop, kw = config_options(cid)
    xs, f0s = spgm_env_inputs(cid)
    r = runs(cid)
    kernel = CONFIGS[cid][2]
    other = "k_spgm_env" if kernel == "k_spgm_env_wf" else "k_spgm_env_wf"
    assert _launches(r["prof"], kernel) >= 1 and _launches(r["prof"], other) == 0, (cid, sorted(r["prof"]))
    assert takes_fallback(fs, thop) == (kernel == "k_spgm_env")
    ref, B = spgm_env_bound(xs, f0s, fs, thop)
    assert r["env"].shape == ref.shape and r["env"].dtype == np.float32
    bad, st = spgm_env_check(r["env"], ref, B)
    _name_frames(st, r["frm_off"])
    st["kernel"] = kernel
    print("spgm_env %-15s %-14s frames %d points %6d  point %.3f at %s %s (err %.2e, B %.2e)  frame %.4f at %s (median %.4f)  KAPPA %.3f" % (
        cid, kernel, st["frames"], st["points"], st["ratio_point"], st["ratio_point_at"], st["ratio_point_at_utt"], st["err_at_it"],
        st["bound_at_it"], st["ratio_frame"], st["ratio_frame_at_utt"], st["ratio_frame_median"], st["kappa"]))
    report("spgm_env_stage_" + cid, st)
    # the all-zero utterance: the value the float64 reference states for zero input, 2 log(1e-10), within one float32 ulp
    z = slice(int(r["frm_off"][I_ZERO]), int(r["frm_off"][I_ZERO + 1]))
    want = np.float32(2.0 * math.log(1e-10))
    assert np.abs(ref[z] - 2.0 * math.log(1e-10)).max() <= 1e-12
    dz = np.abs(r["env"][z].astype(np.float64) - float(want))
    assert dz.max() <= float(np.spacing(np.abs(want))), (cid, float(dz.max()))
    assert not bad, (cid, len(bad), bad[:8], {k: v for k, v in st.items()})


def test_fix_launch_runs_and_lands(ctx):
    """WF_REFERENCE_CASE (tests/test_invariance_host.py: a frame whose float64 DC bin lies 147 dB under its harmonics):
    the list-and-redo launch runs, and the whole utterance -- the pinned frame with it, all of its points -- is inside
    (a) and (b)"""
    fs, thop, kw, x, f0 = case_signal(WF_REFERENCE_CASE)
    assert not takes_fallback(fs, thop)
    r = run_batch(ctx, fs, thop, kw, [x], [f0])
    assert _launches(r["prof"], "k_spgm_env_wf") >= 1 and _launches(r["prof"], "k_spgm_env_fix") >= 1, sorted(r["prof"])
    ref, B = spgm_env_bound([x], [f0], fs, thop)
    bad, st = spgm_env_check(r["env"], ref, B)
    g = WF_REFERENCE_CASE["frame"]
    e = np.abs(r["env"][g].astype(np.float64) - ref[g])
    st.update(pinned_frame=g, pinned_ratio_point=float((e / B[g]).max()), pinned_edge_err=(float(e[0]), float(e[-1])),
              pinned_edge_bound=(float(B[g, 0]), float(B[g, -1])),
              pinned_ratio_frame=float(np.sqrt(np.mean(e * e)) / np.sqrt(np.mean(B[g] * B[g]))))
    report("spgm_env_stage_fix_case", st)
    assert not [b for b in bad if b[1] == g], [b for b in bad if b[1] == g]
    assert not bad, (len(bad), bad[:8])


def test_bits_do_not_depend_on_neighbours_or_cache(ctx, runs):
    """No tolerance.  The batch with its utterance order reversed; three utterances alone; one utterance after an utterance
    whose last frame -- alone in its pair, so its seeds are the cache's entry -- has the F0 bits and window length of its
    first, and after one that has not; and those three 210 times over in one batch of 4 200 pairs, where every wavefront
    of the 2 048 resident ones walks three pairs and a hit across pairs really occurs (a batch under 2 048 pairs gives
    each pair a wavefront of its own: only frame b of a pair can hit).  The bits of an utterance's plane-0 rows are the
    same in every arrangement."""
    cid = "wf_11_1"
    fs, thop, kw = config_options(cid)
    xs, f0s = spgm_env_inputs(cid)
    r = runs(cid)
    nu = len(xs)

    def rows(res, k):
        return res["env"][int(res["frm_off"][k]):int(res["frm_off"][k + 1])].view(np.int32)

    def same(a, b_, how):
        assert a.shape == b_.shape and np.array_equal(a, b_), (how, int(np.count_nonzero(a != b_)))
    rev = run_batch(ctx, fs, thop, kw, xs[::-1], f0s[::-1])
    for k in range(nu):
        same(rows(r, k), rows(rev, nu - 1 - k), "reversed, utterance %d (%s)" % (k, NAMES[k]))
    for k in (I_LOW, I_SHORT, I_SPEECH):
        solo = run_batch(ctx, fs, thop, kw, [xs[k]], [f0s[k]], stale_first=False)
        same(rows(r, k), rows(solo, 0), "alone, utterance %d (%s)" % (k, NAMES[k]))
    (xt, ft), (xa, fa), (xb, fb) = cache_pair(cid)
    alone = rows(run_batch(ctx, fs, thop, kw, [xt], [ft], stale_first=False), 0)
    same(rows(run_batch(ctx, fs, thop, kw, [xa, xt], [fa, ft]), 1), alone, "after an utterance ending on its F0 and window")
    same(rows(run_batch(ctx, fs, thop, kw, [xb, xt], [fb, ft]), 1), alone, "after an utterance ending on another F0")
    reps = 210
    big = run_batch(ctx, fs, thop, kw, [xa, xt, xb, xt] * reps, [fa, ft, fb, ft] * reps, stale_first=False)
    assert sum((len(f) + 1) // 2 for f in (fa, ft, fb, ft)) * reps > 2 * 2048
    for k in range(4 * reps):
        if k % 2 == 1:
            same(rows(big, k), alone, "copy %d of 420 in a batch whose wavefronts walk three pairs" % (k // 2))
    # the LDS kernel: reversed order
    cid = "lds_fold8"
    fs, thop, kw = config_options(cid)
    xs, f0s = spgm_env_inputs(cid)
    r = runs(cid)
    rev = run_batch(ctx, fs, thop, kw, xs[::-1], f0s[::-1])
    for k in range(nu):
        same(rows(r, k), rows(rev, nu - 1 - k), "k_spgm_env reversed, utterance %d (%s)" % (k, NAMES[k]))
