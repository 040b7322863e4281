"""-m gpu: k_refine_f0 against float64 frame by frame, and the analysis downstream of the track it leaves.

f0_refine = 1 is the library's default, yet the rest of the suite analyses with f0_refine = 0 and holds the refined track
to one flat 200 Hz utterance, its clipped frames left out, within 2e-2 Hz.  Three stages here:

  A  the F0 row on its own.  Every frame of every utterance of refine_f0_reference.refine_inputs -- moving tracks with
     unvoiced runs, frames clipped at one end and at both, a fundamental 20 ... 30 dB under its neighbours, windows shorter
     than a wavefront, a 100-sample utterance between loud neighbours, silence, and the acceptance gate with 0, 1, 2 and
     3 estimates accepted -- held to refine_ref (float64, proven against the oracle by tests/test_refine_f0_host.py)
     under refine_check: |f - f_64| <= 4 Y_u + 16 EPS f_64, Y_u the plain float32 evaluation's largest error in the
     utterance; unvoiced and all-rejected frames keep the uploaded BITS.  The bound and the derivation of its additive term
     are in the docstring of tests/refine_f0_reference.py; no bound may exceed 1e-3 F0 and none is calibrated on the
     kernel.  The batch, llsm_refine_f0 (the refine_only route) and the drop-in llsm_analyze give the same bits, as do the
     batch reversed and utterances alone.
  B  downstream of the device's OWN refined track: the float64 oracle runs with f0_refine = 0 on the downloaded row, so
     that the two estimators' difference (1e-4 F0 moves harmonic 100 by 1 % of F0) is not mistaken for an analysis error,
     and every row is held to the contract of tests/gpu_common.py exactly as tests/test_gpu_configs.py does.
  C  a second analysis of a refined row without a new F0 upload, the waveform's pitch 8 % lower again: the row after
     refinement lies under 0.9 x the uploaded minimum, which is what the batch's bookkeeping has to follow.

Every batch is first analysed on another signal of ten times the level.  What the kernel measures against these bounds:
the table in DESIGN.md section 8."""
import ctypes as C

import numpy as np
import pytest

import libllsm2_amd as llsm
from gpu_common import Yard, analysis_metrics, aopt_kwargs, assert_contract, assert_hmpp_contract, report
from harm_env_reference import plan_values
from refine_f0_reference import (CAP_REL, CONFIGS, DOWN_CONFIGS, GATE_CONFIG, GATE_FACTOR, HMPP, I_LOW, I_SHORT, I_SPEECH, STATE_FS,
                                 STATE_THOP, STATE_UP, config_rate, downstream_inputs, gate_margins, loud_inputs, offsets,
                                 refine_check, refine_inputs, state_inputs)

pytestmark = pytest.mark.gpu
P = llsm.P_fp

# the analysis options of each configuration of stage A (band edges under Nyquist; the F0 row does not depend on them)
A_OPTS = {"8k_5ms": dict(nchannel=2, chanfreq=[1500.0], maxnhar=60), "16k_5ms": dict(nchannel=3, chanfreq=[1000.0, 3000.0]),
          "44k_5ms": dict(), "44k_hop128": dict(), "96k_10ms": dict(), GATE_CONFIG: dict()}
ALL = list(CONFIGS) + [GATE_CONFIG]


@pytest.fixture(scope="module")
def ctx():
    c = llsm.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def L():
    L = llsm.load()
    L.llsm_refine_f0.argtypes = [P, C.c_int, C.c_float, P, C.c_int, C.c_float]
    return L


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def run_batch(ctx, fs, thop, opt, xs, f0s, stale_first=True, keep=False):
    """one batch with f0_refine = 1: analysed on the loud signal, the F0 row uploaded again (the first analysis refined it),
    then analysed on xs with profiling on.  Returns the refined row and the profile (keep: and the open batch)."""
    ao = llsm.make_aoptions(f0_refine=1, thop=thop, **opt)
    b = llsm.Batch(ctx, ao, fs, [len(x) for x in xs], [len(f) for f in f0s])
    try:
        assert np.array_equal(b.x_off, offsets(xs)) and np.array_equal(b.frm_off, offsets(f0s))
        if stale_first:
            b.upload(llsm.A_F0, np.concatenate(f0s)); b.upload(llsm.A_X, np.concatenate(loud_inputs(xs)))
            b.analyze()
        b.upload(llsm.A_F0, np.concatenate(f0s)); b.upload(llsm.A_X, np.concatenate(xs))
        ctx.set_profiling(True); ctx.reset_profile()
        try:
            b.analyze(); ctx.sync()
            prof = ctx.profile()
        finally:
            ctx.set_profiling(False)
        out = dict(row=b.download(llsm.A_F0), prof=prof, ao=ao)
        if keep:
            out["batch"] = b
        return out
    finally:
        if not keep:
            b.close()


@pytest.fixture(scope="module")
def runs(ctx):
    """one batch per configuration of stage A, analysed once and shared"""
    cache = {}

    def get(cid):
        if cid not in cache:
            fs, thop = config_rate(cid)
            xs, f0s, names = refine_inputs(cid)
            cache[cid] = dict(run_batch(ctx, fs, thop, A_OPTS[cid], xs, f0s), xs=xs, f0s=f0s, names=names, fs=fs, thop=thop)
        return cache[cid]
    return get


def judge(tag, row, xs, f0s, fs, thop, names=None):
    bad, st = refine_check(row, xs, f0s, fs, thop)
    for rec in st["utterances"]:
        rec["name"] = names[rec["utt"]] if names else str(rec["utt"])
        print("refine_f0 %-10s %-9s frames %2d (%2d held)  Y/F0 %.2e  bound/F0 %.2e  error/F0 %.2e = %.3f of its bound (frame %d)" % (
            tag, rec["name"], rec["frames"], rec["held"], rec["Y_rel"], rec["bound_rel"], rec["err_rel"], rec["ratio"], rec["at"]))
    report("refine_f0_" + tag, st)
    assert not bad, (tag, bad[:8], {k: st[k] for k in st if k != "utterances"})
    return st


# ====================================================================== stage A
@pytest.mark.parametrize("cid", ALL)
def test_refined_row_of_a_batch(runs, cid):
    """every frame of the multi-utterance batch under refine_check: nothing excluded, no share allowed to miss"""
    r = runs(cid)
    assert r["prof"].get("k_refine_f0", (0, 0))[1] >= 1, sorted(r["prof"])
    st = judge(cid, r["row"], r["xs"], r["f0s"], r["fs"], r["thop"], r["names"])
    f0 = np.concatenate(r["f0s"])
    assert np.array_equal(bits(r["row"])[f0 == 0], bits(f0)[f0 == 0]) and st["frames"] == len(f0)


@pytest.mark.parametrize("cid", ALL)
def test_three_routes_give_the_same_bits(L, runs, cid):
    """one utterance at a time through llsm_refine_f0 (refine_only: maxnhar = 1, npsd = 2, one channel) and through the
    drop-in llsm_analyze, which rewrites the caller's f0[]: the bits of the batch's row, which refine_check has judged"""
    r = runs(cid)
    frm = offsets(r["f0s"])
    ao = llsm.make_aoptions(f0_refine=1, thop=r["thop"], **A_OPTS[cid])
    for u, (x, f0) in enumerate(zip(r["xs"], r["f0s"])):
        want = bits(r["row"][frm[u]:frm[u + 1]])
        fa = f0.copy()
        L.llsm_refine_f0(x.ctypes.data_as(P), len(x), r["fs"], fa.ctypes.data_as(P), len(fa), r["thop"])
        assert np.array_equal(bits(fa), want), (cid, r["names"][u], "llsm_refine_f0", int(np.count_nonzero(bits(fa) != want)))
        fb = f0.copy()
        ch = L.llsm_analyze(C.byref(ao), x.ctypes.data_as(P), len(x), r["fs"], fb.ctypes.data_as(P), len(fb), None)
        assert bool(ch), L.llsm_gpu_last_error()
        L.llsm_delete_chunk(ch)
        assert np.array_equal(bits(fb), want), (cid, r["names"][u], "llsm_analyze", int(np.count_nonzero(bits(fb) != want)))


def test_bits_do_not_depend_on_neighbours(ctx, runs):
    """No tolerance.  The utterance order reversed, and the clipped low-F0 utterance, the 100-sample one and a
    make_speechlike one each alone: the same bits per utterance (which block of the grid a frame is, the alignment of its
    samples and what lies beyond its utterance's ends all change)."""
    cid = "44k_5ms"
    r = runs(cid)
    xs, f0s, fs, thop = r["xs"], r["f0s"], r["fs"], r["thop"]
    frm = offsets(f0s)
    rev = run_batch(ctx, fs, thop, A_OPTS[cid], xs[::-1], f0s[::-1])["row"]
    frm_r = offsets(f0s[::-1])
    nu = len(xs)
    for k in range(nu):
        a, b_ = bits(r["row"][frm[k]:frm[k + 1]]), bits(rev[frm_r[nu - 1 - k]:frm_r[nu - k]])
        assert np.array_equal(a, b_), ("reversed", r["names"][k], int(np.count_nonzero(a != b_)))
    for k in (I_LOW, I_SHORT, I_SPEECH):
        solo = run_batch(ctx, fs, thop, A_OPTS[cid], [xs[k]], [f0s[k]], stale_first=False)["row"]
        assert np.array_equal(bits(solo), bits(r["row"][frm[k]:frm[k + 1]])), ("alone", r["names"][k])


# ====================================================================== stage B
def oracle_on_row(o64, ao, kw, x, fs, row):
    """the float64 oracle with f0_refine = 0 on the device's refined row; returns (Params, residual, the oracle's options)"""
    okw = aopt_kwargs(ao)
    okw["f0_refine"] = 0
    if "chanfreq" in kw:
        okw["chanfreq"] = kw["chanfreq"]
    pr, xr = o64.analyze(o64.aoptions(**okw), x, fs, np.asarray(row, np.float32), want_res=True)
    return pr, xr, okw


def hold_downstream(o64, b, ao, kw, xs, fs, row, where):
    """every utterance's rows against the oracle run on its refined track: tests/test_gpu_configs.py's contract"""
    g, xres = b.download_params(), b.download(llsm.A_XRES)
    out = []
    for u, x in enumerate(xs):
        sl = slice(int(b.frm_off[u]), int(b.frm_off[u + 1]))
        pr, xr, okw = oracle_on_row(o64, ao, kw, x, fs, row[sl])
        m = analysis_metrics(g, sl, pr, xres[b.x_off[u]:b.x_off[u + 1]], xr)
        try:
            if ao.hm_method == HMPP:
                assert_hmpp_contract(m, Yard(okw, x, fs, row[sl]), "%s utt %d" % (where, u))
            else:
                assert_contract(m, Yard(okw, x, fs, row[sl]), "%s utt %d" % (where, u))
        finally:
            report("refine_f0_downstream_%s_utt%d" % (where, u), m)
        out.append(m)
    return g, out


def frame_members(L, fr):
    """(f0, nhar, ampl, phse, psd, edc, [envelope nhar, ampl, phse per channel], psdres) of one frame of a chunk"""
    f0 = C.cast(L.llsm_container_get(fr, llsm.FRAME_F0), P)[0]
    hm = C.cast(L.llsm_container_get(fr, llsm.FRAME_HM), C.POINTER(llsm.HMFrame))
    hm = hm.contents if hm else llsm.HMFrame(None, None, 0)
    nm = C.cast(L.llsm_container_get(fr, llsm.FRAME_NM), C.POINTER(llsm.NMFrame)).contents
    rp = L.llsm_container_get(fr, llsm.FRAME_PSDRES)
    take = lambda p, n: np.ctypeslib.as_array(p, (max(n, 1),))[:n].copy()          # noqa: E731
    env = []
    for c in range(nm.nchannel):
        e = nm.eenv[c].contents
        env.append((e.nhar, take(e.ampl, e.nhar), take(e.phse, e.nhar)))
    n = L.llsm_fparray_length(C.cast(rp, P)) if rp else 0
    return dict(f0=np.float32(f0), nhar=hm.nhar, ampl=take(hm.ampl, hm.nhar), phse=take(hm.phse, hm.nhar), psd=take(nm.psd, nm.npsd),
                edc=take(nm.edc, nm.nchannel), env=env, psdres=take(C.cast(rp, P), n) if rp else None)


@pytest.mark.parametrize("cid", sorted(DOWN_CONFIGS))
def test_downstream_of_the_refined_row(ctx, L, o64, cid):
    fs, thop, kw = DOWN_CONFIGS[cid]
    xs, f0s = downstream_inputs(cid)
    r = run_batch(ctx, fs, thop, kw, xs, f0s, keep=True)
    b, ao, row = r["batch"], r["ao"], r["row"]
    try:
        judge("down_" + cid, row, xs, f0s, fs, thop)
        # the kernels the refined track is there for
        assert r["prof"].get("k_refine_f0", (0, 0))[1] >= 1, sorted(r["prof"])
        if ao.hm_method != HMPP:
            assert r["prof"].get("k_harm_speech_rest", (0, 0))[1] >= 1, sorted(r["prof"])
        else:
            assert r["prof"].get("k_utt_fftsize", (0, 0))[1] >= 1 and r["prof"].get("k_harm_pp", (0, 0))[1] >= 1, sorted(r["prof"])
        g, ms = hold_downstream(o64, b, ao, kw, xs, fs, row, cid)
        me, nch, mh = b.layout.maxnhar_e, b.layout.nchannel, b.layout.maxnhar
        if cid == "8k_2ch":
            # the nhar-crossing utterance: the uploaded 202 Hz has 19 harmonics, the refined track 20, and after refinement
            # the flat track is no run of bit-identical frames any more (no tile: k_harm_speech_rest takes them)
            sl = slice(int(b.frm_off[1]), int(b.frm_off[2]))
            K_up = plan_values(f0s[1], np.arange(len(f0s[1])), thop, fs, 4.0, mh)[2]
            K = plan_values(row[sl], np.arange(len(f0s[1])), thop, fs, 4.0, mh)[2]
            assert np.all(K_up == 19) and np.count_nonzero(K == 20) >= 20
            assert np.array_equal(g[llsm.A_NHAR][sl], K)
            beyond = np.arange(mh)[None, :] >= K[:, None]
            assert not bits(g[llsm.A_AMPL][sl])[beyond].any() and not bits(g[llsm.A_PHSE][sl])[beyond].any()
            assert not bits(g[llsm.A_AMPL])[np.concatenate(f0s) == 0].any()
            same = bits(row[sl])[1:] == bits(row[sl])[:-1]
            run = max((len(s) for s in "".join("1" if v else "0" for v in same).split("0")), default=0) + 1
            assert run < 8, run
        # the chunk of the drop-in llsm_analyze (capi.cpp's non-prebuilt route under f0_refine): frame by frame the bits of
        # the batch's rows
        for u, (x, f0) in enumerate(zip(xs, f0s)):
            fc = f0.copy()
            ch = L.llsm_analyze(C.byref(ao), x.ctypes.data_as(P), len(x), fs, fc.ctypes.data_as(P), len(fc), None)
            assert bool(ch), L.llsm_gpu_last_error()
            try:
                lo = int(b.frm_off[u])
                assert np.array_equal(bits(fc), bits(row[lo:lo + len(f0)]))
                for i in range(len(f0)):
                    fr, k = frame_members(L, ch.contents.frames[i]), lo + i
                    assert bits(fr["f0"]) == bits(row[k]), (u, i)
                    if row[k] == 0:
                        continue
                    n = int(g[llsm.A_NHAR][k])
                    assert fr["nhar"] == n, (u, i)
                    assert np.array_equal(bits(fr["ampl"]), bits(g[llsm.A_AMPL][k, :n])) and np.array_equal(bits(fr["phse"]), bits(g[llsm.A_PHSE][k, :n])), (u, i)
                for i in range(len(f0)):
                    fr, k = frame_members(L, ch.contents.frames[i]), lo + i
                    assert np.array_equal(bits(fr["psd"]), bits(g[llsm.A_PSD][k])) and np.array_equal(bits(fr["edc"]), bits(g[llsm.A_EDC][k])), (u, i)
                    assert fr["psdres"] is not None and np.array_equal(bits(fr["psdres"]), bits(g[llsm.A_PSDRES][k])), (u, i)
                    ne = int(g[llsm.A_NHAR_E][k])
                    ea = g[llsm.A_EENV_AMPL][k].reshape(nch, max(me, 1)); ep = g[llsm.A_EENV_PHSE][k].reshape(nch, max(me, 1))
                    for c in range(nch):
                        en, a, p_ = fr["env"][c]
                        assert en == ne and np.array_equal(bits(a), bits(ea[c, :ne])) and np.array_equal(bits(p_), bits(ep[c, :ne])), (u, i, c)
            finally:
                L.llsm_delete_chunk(ch)
    finally:
        b.close()


# ====================================================================== stage C
@pytest.mark.parametrize("method", ["HMCZT", "HMPP"])
def test_second_analysis_without_a_new_f0(ctx, o64, method):
    """Uploaded 100 Hz; the first waveform at 92 Hz, the second -- uploaded alone -- at 84.6 Hz: the twice-refined track
    lies under 0.9 x the uploaded minimum, where the window (2085 samples) needs a 4096-point transform (HMPP:
    llsm_get_fftsize) and more window-table slots than 0.9 x 100 Hz provisions (HMCZT).  Both refinements under
    refine_check -- the second against the reference run on the once-refined row --, and the rows of the second analysis
    against the oracle on the twice-refined row."""
    fs, thop = STATE_FS, STATE_THOP
    kw = dict(hm_method=getattr(llsm, method))
    x1, x2, f0 = state_inputs()
    r = run_batch(ctx, fs, thop, kw, [x1], [f0], keep=True)
    b, ao, row1 = r["batch"], r["ao"], r["row"]
    try:
        judge("state_%s_first" % method, row1, [x1], [f0], fs, thop)
        b.upload(llsm.A_X, x2)                                    # no new F0
        b.analyze(); ctx.sync()
        row2 = b.download(llsm.A_F0)
        # the conditions on this input depend on the device's own once-refined row: checked here, before it is judged
        gm = gate_margins([x2], [row1], fs, thop)[0]
        assert gm[0] >= GATE_FACTOR, gm
        st = judge("state_%s_second" % method, row2, [x2], [row1], fs, thop)
        assert st["bound_rel"] <= CAP_REL
        v = row2 > 0
        mid = slice(15, len(f0) - 15)
        assert np.all(np.abs(row2[mid] / (STATE_UP * 0.92 * 0.92) - 1) < 5e-3)
        hw = lambda f: int(plan_values(np.float32([f]), [0], thop, fs, 4.0, 1)[1][0])           # noqa: E731
        assert float(row2[v].min()) < 0.9 * STATE_UP and hw(0.9 * STATE_UP) <= 2048 < hw(float(row2[v].min())) <= 4096
        hold_downstream(o64, b, ao, kw, [x2], fs, row2, "state_" + method)
    finally:
        b.close()
