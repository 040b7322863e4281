"""-m gpu: an utterance gets the same bits however it reaches the device.

* The zero-phase band filter cuts long signals into time segments (engine.cpp build_jobs).  Whether a signal is cut may
  depend on the signal alone: a long utterance alone, inside a resident batch of 255 utterances (1 020 band signals) and
  inside one of 256 (1 024 band signals) gives the same analysis rows and -- from the same parameters and templates --
  the same waveforms; llsm_analyze_batch / llsm_synthesize_batch give the same rows and samples for fan-out blocks of
  32, 256 and all utterances.
* The LDS spectrogram kernel k_spgm_env (4096-point transforms, folds of 8 and more, PSD windows longer than the
  spectrogram) forms the DC and Nyquist bins exactly, as the register-resident path does for the frames it lists: on the
  configurations pinned in test_invariance_host.py, each with a frame whose float64 edge bin lies >= 110 dB under its
  harmonics, the envelope plane there and the smoothed PSD after it stay at the float64 oracle.
* A batch follows the conventions in force at each call (llsm_gpu.h llsm_gpu_set_convention): a batch created, analysed
  and synthesised under one convention and then used again under another gives what a fresh batch gives under that one."""
import ctypes as C

import numpy as np
import pytest

import libllsm2_amd as llsm
from conftest import FS, make_speechlike
from gpu_common import gpu_analyze, report
from test_gpu_configs import _run_parity
from test_gpu_round2 import CONVENTIONS
from test_invariance_host import (FALLBACK_CASES, WF_REFERENCE_CASE, case_signal, oracle_stages, spgm_sizes,
                                  takes_fallback)

pytestmark = pytest.mark.gpu

ROW_IDS = (llsm.A_AMPL, llsm.A_PHSE, llsm.A_PSD, llsm.A_PSDRES, llsm.A_EDC, llsm.A_EENV_AMPL, llsm.A_EENV_PHSE,
           llsm.A_NHAR, llsm.A_NHAR_E)
LONG_NX = 150000                # 3.4 s at 44.1 kHz: four band signals long enough to be cut into time segments
FILLER_NX = (4410, 4631, 4852)  # 0.1 s and a little more: 20, 21 and 22 frames


@pytest.fixture(scope="module")
def ctx():
    c = llsm.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def long_utt():
    x, f0 = make_speechlike(4242, nx=LONG_NX)
    return x, f0.astype(np.float32)


def _fillers(n):
    out = []
    for u in range(n):
        x, f0 = make_speechlike(5000 + u % 16, nx=FILLER_NX[u % 3])
        out.append((x, f0.astype(np.float32)))
    return out


def _batch_with(long_utt, U, k):
    """U utterances: fillers, the long one at index k (an odd frame offset before it)"""
    fill = _fillers(U - 1)
    utts = fill[:k] + [long_utt] + fill[k:]
    assert sum(len(f) for _, f in utts[:k]) % 2 == 1
    return [x for x, _ in utts], [f for _, f in utts]


def _rows_of(b, g, xres, k):
    f0, f1 = int(b.frm_off[k]), int(b.frm_off[k + 1])
    r = {a: g[a][f0:f1] for a in ROW_IDS}
    r["xres"] = xres[int(b.x_off[k]):int(b.x_off[k + 1])]
    return r


def _assert_same(got, ref, where):
    for a in ref:
        assert got[a].shape == ref[a].shape, (where, a)
        if not np.array_equal(got[a], ref[a]):
            d = np.abs(got[a].astype(np.float64) - ref[a].astype(np.float64))
            raise AssertionError(f"{where}: array {a} differs in {np.count_nonzero(d)} values, max |diff| {d.max():.3g}")


@pytest.mark.parametrize("U", [255, 256])
def test_long_utterance_rows_do_not_depend_on_the_batch_size(ctx, long_utt, U):
    """A1: 255 utterances x 4 channels = 1 020 band signals, 256 x 4 = 1 024: the two sides of the old batch-size rule."""
    x, f0 = long_utt
    ao = llsm.make_aoptions(f0_refine=0)
    b1, g1, xr1 = gpu_analyze(ctx, ao, FS, [x], [f0])
    ref = _rows_of(b1, g1, xr1, 0); b1.close()
    k = 8
    xs, f0s = _batch_with(long_utt, U, k)
    b, g, xr = gpu_analyze(ctx, ao, FS, xs, f0s)
    try:
        assert b.layout.n_utt == U
        _assert_same(_rows_of(b, g, xr, k), ref, f"utterance {k} of {U}")
        assert np.abs(ref[llsm.A_EDC]).max() > 0 and np.abs(ref[llsm.A_EENV_AMPL]).max() > 0
    finally:
        b.close()


@pytest.mark.parametrize("U", [255, 256])
def test_long_utterance_synthesis_does_not_depend_on_the_batch_size(ctx, long_utt, U):
    """A2: the same rows and the same injected white templates give the same y_noise / y_sin / y."""
    x, f0 = long_utt
    ao = llsm.make_aoptions(f0_refine=0)
    so = llsm.make_soptions(FS)
    b1, g1, _ = gpu_analyze(ctx, ao, FS, [x], [f0])
    rows = {a: g1[a].copy() for a in llsm.Batch.PARAM_IDS}
    nt = b1.layout.ntemplate_ext
    white_long = np.random.default_rng(31).standard_normal((4, nt)).astype(np.float32)
    b1.upload(llsm.A_WHITE, white_long[None])
    b1.synthesize(so, seed=0, injected_white=True); ctx.sync()
    ref = {a: b1.download(a) for a in (llsm.A_YNOISE, llsm.A_YSIN, llsm.A_Y)}
    b1.close()
    assert np.abs(ref[llsm.A_YNOISE]).max() > 0
    k = 8
    xs, f0s = _batch_with(long_utt, U, k)
    b, g, _ = gpu_analyze(ctx, ao, FS, xs, f0s)
    try:
        f_a, f_b = int(b.frm_off[k]), int(b.frm_off[k + 1])
        for a in llsm.Batch.PARAM_IDS:                   # the long utterance's rows exactly as alone
            g[a][f_a:f_b] = rows[a]
        b.upload_params(g)
        white = np.random.default_rng(32).standard_normal((U, 4, nt)).astype(np.float32)
        white[k] = white_long
        b.upload(llsm.A_WHITE, white)
        b.synthesize(so, seed=0, injected_white=True); ctx.sync()
        y0, y1 = int(b.y_off[k]), int(b.y_off[k + 1])
        got = {a: b.download(a)[y0:y1] for a in ref}
        _assert_same(got, ref, f"utterance {k} of {U}")
    finally:
        b.close()


def test_fanout_block_size_does_not_change_long_utterances():
    """A3: llsm_analyze_batch / llsm_synthesize_batch over 300 utterances, six of them long, in blocks of 32, of 256 and
    in one block: every HM / NM row, the residual and y bit for bit (utterance u draws from seed + u in every plan).  Under
    the old batch-size rule a block of 32 (at most 128 band signals) cut the synthesis templates -- of fillers too: 4 538 ..
    4 980 samples give two segments in the 4 and 8 kHz bands -- and one block of 300 (1 200 signals) did not; y of four
    utterances moved by up to 3e-8."""
    L = llsm.load()
    AB = L.llsm_analyze_batch
    AB.argtypes = [C.POINTER(llsm.AOptions), C.POINTER(llsm.P_fp), llsm.P_int, C.c_float, C.POINTER(llsm.P_fp), llsm.P_int,
                   C.c_int, C.POINTER(C.POINTER(llsm.Chunk)), C.POINTER(llsm.P_fp)]
    SB = L.llsm_synthesize_batch
    SB.argtypes = [C.POINTER(llsm.SOptions), C.POINTER(C.POINTER(llsm.Chunk)), C.c_int, C.POINTER(C.POINTER(llsm.Output))]
    U = 300
    longs = {3: 4300, 40: 4301, 97: 4302, 150: 4303, 233: 4304, 299: 4305}
    xs, f0s = [], []
    for u in range(U):
        if u in longs:
            x, f0 = make_speechlike(longs[u], nx=LONG_NX - 977 * (u % 5))
        else:
            x, f0 = make_speechlike(6000 + u % 16, nx=FILLER_NX[u % 3])
        xs.append(np.ascontiguousarray(x, np.float32)); f0s.append(np.ascontiguousarray(f0, np.float32))
    ao = llsm.make_aoptions(f0_refine=0)
    so = llsm.make_soptions(FS)
    nx = np.array([len(x) for x in xs], np.int32); nf = np.array([len(f) for f in f0s], np.int32)
    xp = (llsm.P_fp * U)(*[x.ctypes.data_as(llsm.P_fp) for x in xs])
    fp_ = (llsm.P_fp * U)(*[f.ctypes.data_as(llsm.P_fp) for f in f0s])

    def rows(ch, n):
        out = []
        for i in range(n):
            fr = ch.contents.frames[i]
            nm = C.cast(L.llsm_container_get(fr, llsm.FRAME_NM), C.POINTER(llsm.NMFrame)).contents
            out.append(np.ctypeslib.as_array(nm.psd, (nm.npsd,)))
            out.append(np.ctypeslib.as_array(nm.edc, (nm.nchannel,)))
            for c in range(nm.nchannel):
                e = nm.eenv[c]
                if e and e.contents.nhar > 0:
                    out.append(np.ctypeslib.as_array(e.contents.ampl, (e.contents.nhar,)))
                    out.append(np.ctypeslib.as_array(e.contents.phse, (e.contents.nhar,)))
            hm = L.llsm_container_get(fr, llsm.FRAME_HM)
            if hm:
                h = C.cast(hm, C.POINTER(llsm.HMFrame)).contents
                if h.nhar > 0:
                    out.append(np.ctypeslib.as_array(h.ampl, (h.nhar,)))
                    out.append(np.ctypeslib.as_array(h.phse, (h.nhar,)))
        return np.concatenate(out).astype(np.float32)

    def run(block):
        L.llsm_gpu_set_fanout(1, 1, block)
        chunks = (C.POINTER(llsm.Chunk) * U)(); xap = (llsm.P_fp * U)()
        assert AB(C.byref(ao), xp, nx.ctypes.data_as(llsm.P_int), FS, fp_, nf.ctypes.data_as(llsm.P_int), U, chunks, xap) == 0, \
            L.llsm_gpu_last_error()
        L.llsm_gpu_set_default_seed(555)
        outs = (C.POINTER(llsm.Output) * U)()
        assert SB(C.byref(so), chunks, U, outs) == 0, L.llsm_gpu_last_error()
        res = []
        for u in range(U):
            res.append((rows(chunks[u], int(nf[u])), np.ctypeslib.as_array(xap[u], (int(nx[u]),)).copy(),
                        np.ctypeslib.as_array(outs[u].contents.y, (outs[u].contents.ny,)).copy()))
            L.llsm_delete_output(outs[u]); L.llsm_delete_chunk(chunks[u])
        return res

    try:
        ref = run(1000)
        for block in (32, 256):
            got = run(block)
            bad = []
            for u in range(U):
                for k, what in enumerate(("rows", "residual", "y")):
                    if not np.array_equal(got[u][k], ref[u][k]):
                        bad.append((u, what, float(np.abs(got[u][k].astype(np.float64) - ref[u][k]).max())))
            assert not bad, (block, bad[:12])
    finally:
        L.llsm_gpu_set_fanout(-1, -1, -1)


@pytest.mark.parametrize("hm_method", [llsm.HMCZT, llsm.HMPP], ids=["hmczt", "hmpp"])
def test_second_stream_does_not_change_the_analysis(ctx, hm_method):
    """A6: llsm_gpu_analysis_overlap(0) keeps every launch of the analysis on one stream, (1) forks the FIX launch of the
    spectrogram envelope and the smoother onto the second and joins them: the same kernels on the same inputs, so every
    analysed array is the same bit for bit.  A fork or join in the wrong place shows as stale or differing PSD rows."""
    L = llsm.load()
    utts = [make_speechlike(71, nx=6615), make_speechlike(72, nx=4410)]      # 0.15 s and 0.1 s: 30 and 20 frames
    xs, f0s = [x for x, _ in utts], [f.astype(np.float32) for _, f in utts]
    ao = llsm.make_aoptions(f0_refine=1, hm_method=hm_method)
    prev = L.llsm_gpu_analysis_overlap(-1)
    got = {}
    try:
        for on in (0, 1):
            L.llsm_gpu_analysis_overlap(on)
            b, g, xres = gpu_analyze(ctx, ao, FS, xs, f0s)
            b.close()
            got[on] = dict(g); got[on]["xres"] = xres
    finally:
        L.llsm_gpu_analysis_overlap(prev)
    assert set(got[0]) == set(llsm.Batch.PARAM_IDS) | {"xres"}
    assert np.abs(got[0][llsm.A_AMPL]).max() > 0 and np.ptp(got[0][llsm.A_PSD]) > 0 and np.abs(got[0][llsm.A_EDC]).max() > 0
    assert not np.array_equal(got[0][llsm.A_F0], np.concatenate(f0s))        # (the refinement ran)
    _assert_same(got[1], got[0], "second stream on against off")


# envelope plane at the edge points of the cancelling frame against the float64 oracle's resampled envelope (natural-log
# units).  The register-resident path with its list-and-redo launch meets it on WF_REFERENCE_CASE (seed 123208, frame 43:
# 1.0e-5 at both points on an MI355X); the LDS kernel without exact edge bins was 1.7e-3 .. 3.0e-2 off on the pinned cases.
ENV_EDGE_TOL = 5e-5


def _env_edges(ctx, o64, case):
    fs, thop, kw, x, f0 = case_signal(case)
    got, pr = oracle_stages(o64, fs, thop, kw, x, f0, stages=(2,))
    ao = llsm.make_aoptions(f0_refine=0, thop=thop, **kw)
    b, g, _ = gpu_analyze(ctx, ao, fs, [x], [f0])
    try:
        n = ctx.L.llsm_gpu_batch_debug_plane(b.h, 0, None, 0)
        a = np.zeros(n, np.float32)
        assert ctx.L.llsm_gpu_batch_debug_plane(b.h, 0, a.ctypes.data_as(C.c_void_p), n) == n
    finally:
        b.close()
    env = a.astype(np.float64).reshape(len(f0), -1)
    ref = got[2]
    assert env.shape == ref.shape
    fr = case["frame"]
    edge = np.abs(env[fr, [0, -1]] - ref[fr, [0, -1]])
    psd_near = np.abs(g[llsm.A_PSD][fr - 2:fr + 10].astype(np.float64) - pr.psd[fr - 2:fr + 10]).max()
    return dict(edge_dc=float(edge[0]), edge_nyq=float(edge[1]), env_frame_max=float(np.abs(env[fr] - ref[fr]).max()),
                env_max=float(np.abs(env - ref).max()), psd_db_near=float(psd_near))


def test_register_path_envelope_edges_reference(ctx, o64):
    """The bound of the fallback cases below, on the path it was measured on."""
    fs, thop, _, _, _ = case_signal(WF_REFERENCE_CASE)
    assert not takes_fallback(fs, thop)
    m = _env_edges(ctx, o64, WF_REFERENCE_CASE)
    report("invariance_env_wf_reference", m)
    assert m["edge_dc"] <= ENV_EDGE_TOL and m["edge_nyq"] <= ENV_EDGE_TOL, m


@pytest.mark.parametrize("cid", sorted(FALLBACK_CASES))
def test_fallback_spectrogram_envelope_at_a_cancelling_frame(ctx, o64, cid):
    """A4 (a): the product's envelope plane at the cancelling frame's edge points."""
    case = FALLBACK_CASES[cid]
    fs, thop, _, _, _ = case_signal(case)
    assert takes_fallback(fs, thop), spgm_sizes(fs, thop)
    m = _env_edges(ctx, o64, case)
    report("invariance_env_" + cid, m)
    assert m["edge_dc"] <= ENV_EDGE_TOL and m["edge_nyq"] <= ENV_EDGE_TOL, m
    assert m["psd_db_near"] <= 0.05, m


@pytest.mark.parametrize("cid", sorted(FALLBACK_CASES))
def test_fallback_spectrogram_full_contract(ctx, o64, cid):
    """A4 (b): the whole parity contract (CEILING included) on the pinned configuration, and the smoothed PSD at most
    0.05 dB off overall -- as test_the_configuration_that_was_outside_until_round_5 holds its own -- without consulting
    either yardstick."""
    fs, thop, kw, x, f0 = case_signal(FALLBACK_CASES[cid])
    m = _run_parity(ctx, o64, "invariance_" + cid, fs, thop, kw, x, f0, quiet=True)
    assert m["psd_db_max"] <= 0.05, m["psd_db_max"]
    assert "psd_db_max_f32_oracle" not in m


@pytest.mark.parametrize("name", sorted(CONVENTIONS))
def test_held_batch_follows_a_convention_change(ctx, o64, name):
    """A5: a batch analysed and synthesised under the defaults, then -- the convention flipped -- analysed and synthesised
    again, equals a fresh batch under the new convention bit for bit."""
    L = llsm.load()
    x, f0 = make_speechlike(91, nx=16000)
    ao = llsm.make_aoptions(f0_refine=0)
    so = llsm.make_soptions(FS)
    dflt, alt = CONVENTIONS[name]

    def outputs(b):
        b.analyze(); b.synthesize(so, seed=9); ctx.sync()
        r = {a: b.download(a) for a in ROW_IDS}
        for a in (llsm.A_XRES, llsm.A_YSIN, llsm.A_YNOISE, llsm.A_Y):
            r[a] = b.download(a)
        return r

    def fresh():
        b = llsm.Batch(ctx, ao, FS, [len(x)], [len(f0)])
        b.upload(llsm.A_X, x); b.upload(llsm.A_F0, f0)
        return b

    held = fresh()
    try:
        assert L.llsm_gpu_get_convention(name.encode()) == dflt
        before = outputs(held)
        try:
            assert L.llsm_gpu_set_convention(name.encode(), alt) == 0
            o64.set_convention(name, alt)
            again = outputs(held)
            b2 = fresh()
            try:
                want = outputs(b2)
            finally:
                b2.close()
        finally:
            L.llsm_gpu_set_convention(name.encode(), dflt); o64.set_convention(name, dflt)
        _assert_same(again, want, f"held batch after {name} = {alt}")
        if name in ("hann_periodic", "filtfilt_pad"):           # (windows of every stage; the band filter's padding)
            assert any(not np.array_equal(before[a], want[a]) for a in want), f"{name} changed nothing"
        # and back: the held batch follows the restored default too
        _assert_same(outputs(held), before, f"held batch after {name} restored")
    finally:
        held.close()
