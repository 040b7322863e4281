"""-m gpu: llsm_gpu_batch_track_f0 against the numpy restatement of its rules (tests/f0_track_reference.py).

Three layers, each exact where the rules make it so: the candidate plane (plane 5) against rule T1 applied to the device's
own CMNDF plane (plane 4) -- f0 and cost bit for bit, l2 and L within 2e-6 (about two float32 ulps at 8 ... 16: the
logarithm is the one operation of T1 whose last bit a library may round its own way); the F0 row against rules T2 - T5
applied to the device's own plane 5, bit for bit; and the row against the whole chain in float64 ("differ" = voicing
differs or F0 more than 1e-3 relative away, at most 0.5 % of the frames of a long utterance: the reference itself moves on
0 of 1 154 and at most 1 of 1 739 golden frames under CMNDF noise of sigma 3e-5, peak about 1.5e-4, and the device's CMNDF
is within 1.3e-4 of float64).  The counts measured on the MI355X are in DESIGN.md section 22."""
import ctypes as C

import numpy as np
import pytest

import libllsm2_amd as llsm
import f0_reference as ref
import f0_track_reference as tref
from conftest import make_speechlike, make_utterance
from gpu_common import report

pytestmark = pytest.mark.gpu

FS = 44100.0
REL = 1e-3                      # a frame differs beyond this relative F0 distance ...
CAP = 0.005                     # ... and at most this share of a long utterance's frames may
L2_TOL = 2e-6
# (fs, fmin, fmax, window_extra): transforms of 512, 1024, 2048 and 4096 points as in tests/test_gpu_f0.py, and of 256
CONFIGS = [(8000.0, 100.0, 500.0, 200), (16000.0, 50.0, 500.0, 200), (44100.0, 50.0, 500.0, 200), (44100.0, 40.0, 800.0, 200),
           (8000.0, 100.0, 500.0, 90)]
NFFT = [512, 1024, 2048, 4096, 256]
OTHER_IDS = (llsm.A_X, llsm.A_XRES, llsm.A_NHAR, llsm.A_AMPL, llsm.A_PHSE, llsm.A_PSD, llsm.A_PSDRES, llsm.A_HAS_PSDRES,
             llsm.A_EDC, llsm.A_NHAR_E, llsm.A_EENV_AMPL, llsm.A_EENV_PHSE, llsm.A_Y, llsm.A_YSIN, llsm.A_YNOISE, llsm.A_WHITE)


@pytest.fixture(scope="module")
def ctx():
    c = llsm.Context(0)
    yield c
    c.close()


def make_batch(ctx, fs, thop, xs, nfrms, **aopt):
    b = llsm.Batch(ctx, llsm.make_aoptions(thop=float(thop), **aopt), fs, [len(x) for x in xs], nfrms)
    if b.layout.total_samples:
        b.upload(llsm.A_X, np.concatenate(xs).astype(np.float32))
    return b


def split(b, a):
    return [a[int(b.frm_off[k]):int(b.frm_off[k + 1])] for k in range(b.layout.n_utt)]


def track(ctx, fs, thop, xs, nfrms, f0=None, **topt):
    """one batch, one call: per utterance the F0 row, the candidate rows [nfrm][24] and, with keep_cmndf, the CMNDF rows"""
    b = make_batch(ctx, fs, thop, xs, nfrms)
    try:
        b.track_f0(f0, **topt)
        ctx.sync()
        F = b.layout.total_frames
        out = dict(f0=split(b, b.download(llsm.A_F0)), cand=split(b, b.debug_plane(5).reshape(F, 24)) if F else None)
        if (f0 or {}).get("keep_cmndf"):
            out["cm"] = split(b, b.debug_plane(4).reshape(F, -1))
        return out
    finally:
        b.close()


def same_bits(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def compare(got, want):
    """(frames that differ, largest relative difference on frames voiced on both sides)"""
    got = np.asarray(got, np.float64); want = np.asarray(want, np.float64)
    both = (got > 0) & (want > 0)
    rel = np.zeros(len(got))
    rel[both] = np.abs(got[both] - want[both]) / want[both]
    bad = ((got > 0) != (want > 0)) | (rel > REL)
    return int(np.count_nonzero(bad)), float(rel.max()) if len(rel) else 0.0


# ---------------------------------------------------------------- the batches of tests 1 - 3, run once
_cases = {}


def case(ctx, name):
    """a batch by name, "golden" or an index into CONFIGS: the device's planes and rows, once per module"""
    if name in _cases:
        return _cases[name]
    if name == "golden":
        names = ("arctic_a0001", "are-you-ready")
        xs = [ref.read_wav(n)[0] for n in names]
        fs, thop, o = FS, np.float32(128.0 / 44100.0), {}
        nfrms = [len(x) // 128 for x in xs]
        assert nfrms == [1154, 1739]
    else:
        fs, fmin, fmax, extra = CONFIGS[name]
        xs = [make_speechlike(u, nx=int(0.45 * fs), fs=fs)[0] for u in (0, 1)]
        thop, o = np.float32(0.005), dict(fmin=fmin, fmax=fmax, window_extra=extra)
        nfrms = [90, 90]
        assert llsm.f0_plan(fs, **o)["nfft"] == NFFT[name]
    got = track(ctx, fs, thop, xs, nfrms, f0=dict(keep_cmndf=1, **o))
    p = llsm.f0_plan(fs, **o)
    _cases[name] = dict(fs=fs, thop=thop, o=o, xs=xs, nfrms=nfrms, lmin=p["lmin"], lmax=p["lmax"], **got)
    return _cases[name]


CASES = ["golden", 0, 1, 2, 3, 4]
case_ids = lambda c: c if c == "golden" else "fs%d_%d_%d_w%d" % CONFIGS[c]


# ---------------------------------------------------------------- tests
@pytest.mark.parametrize("name", CASES, ids=case_ids)
def test_candidates_exact(ctx, name):
    c = case(ctx, name)
    slots = np.zeros(8, np.int64)
    for u, (cm, cand) in enumerate(zip(c["cm"], c["cand"])):
        assert cm.shape[1] == c["lmax"] + 1
        gated = np.all(cm == 1.0, axis=1)                                  # (plane 4 holds ones on a gated row)
        f0, cost, l2, n = tref.candidates(cm, gated, c["fs"], c["lmin"], c["lmax"])
        assert same_bits(cand[:, 0:8], f0), (name, u)
        assert same_bits(cand[:, 8:16], cost), (name, u)
        assert np.abs(cand[:, 16:24].astype(np.float64) - l2).max() <= L2_TOL, (name, u)
        assert np.all(cand[:, 16:23][f0[:, :7] == 0] == 0)                 # unused slots: zero in l2 as well
        L = cand[:, 23]
        assert np.all(L == L[0]) and abs(float(L[0]) - np.log2(float(np.float32(c["fs"])) / c["lmin"])) <= L2_TOL
        slots += np.bincount(n, minlength=8)
    print("candidates per frame, 0 ... 7:", name, list(slots))
    assert slots[1:].sum() > 0
    if name == "golden":
        assert np.all(slots > 0)                                           # every count of slots occurs


@pytest.mark.parametrize("name", CASES, ids=case_ids)
def test_path_exact(ctx, name):
    c = case(ctx, name)
    for u, (cand, row) in enumerate(zip(c["cand"], c["f0"])):
        n = np.count_nonzero(cand[:, 0:7], axis=1)
        want = tref.viterbi(cand[:, 0:8], cand[:, 8:16], cand[:, 16:24], n, cand[0, 23])
        assert same_bits(row, want), (name, u, int(np.count_nonzero(row != want)))
        assert np.count_nonzero(row) > 20


def test_against_float64(ctx):
    c = case(ctx, "golden")
    out = {}
    for u, name in enumerate(("arctic_a0001", "are-you-ready")):
        want = tref.track(c["xs"][u], c["fs"], c["nfrms"][u], c["thop"])[0]
        n, rel = compare(c["f0"][u], want)
        out[name] = dict(frames=c["nfrms"][u], differ=n, rel_max=rel, voiced=int(np.count_nonzero(c["f0"][u])))
    report("f0_track_golden", out)
    for name, o in out.items():
        assert o["differ"] <= int(CAP * o["frames"]), out


def test_quality_on_trap(ctx):
    utts = [tref.trap(u) for u in range(3)]
    xs = [x for x, _ in utts]; nfrms = [len(f) for _, f in utts]
    b = make_batch(ctx, FS, 0.005, xs, nfrms)
    try:
        b.track_f0()
        tracked = split(b, b.download(llsm.A_F0))
        b.estimate_f0()
        estimated = split(b, b.download(llsm.A_F0))
    finally:
        b.close()
    out = {u: dict(tracker=tref.gross_errors(tracked[u], utts[u][1]), estimator=tref.gross_errors(estimated[u], utts[u][1]))
           for u in range(3)}
    report("f0_track_trap", out)
    for u in range(3):
        assert out[u]["tracker"] <= 2, out
        assert out[u]["estimator"] >= 15, out


def _edge_utterances():
    """the nine mixed utterances of tests/test_gpu_f0.py at 44.1 kHz, 5 ms hop, and frame counts around the 64 frames the
    back pointers are stored and walked by: (samples, frames)"""
    voiced = make_speechlike(3, nx=12000)[0][2000:]                     # starts inside the voiced stretch
    long = make_speechlike(3, nx=30000)[0]
    return [(make_speechlike(0, nx=9000)[0], 40),
            (voiced[:3000], 0),                                           # no frames
            (voiced[:100], 1), (voiced[:700], 4), (voiced[:1500], 5),     # shorter than W = 1082 or hardly longer
            (np.zeros(5000, np.float32), 22),                             # all zero
            (make_speechlike(1, nx=6000)[0], 27),                         # an odd number of frames
            (make_utterance(3, 233.7, nx=4000), 18),
            (make_speechlike(2, nx=8000)[0], 36)] + \
           [(long[2000: 2000 + 221 * n], n) for n in (2, 63, 64, 65, 129)]


def test_shape_edges_and_invariance(ctx):
    utts = _edge_utterances()
    xs = [x for x, _ in utts]; nfrms = [n for _, n in utts]
    b = make_batch(ctx, FS, 0.005, xs, nfrms)
    try:
        b.track_f0()
        first = b.download(llsm.A_F0)
        plane = b.debug_plane(5)
        b.track_f0()
        assert same_bits(b.download(llsm.A_F0), first)                     # a second call: the same bits
        assert same_bits(b.debug_plane(5), plane)
        rows = split(b, first)
        cands = split(b, plane.reshape(-1, 24))
    finally:
        b.close()
    assert len(rows[1]) == 0 and np.all(rows[5] == 0) and len(rows[5]) == 22
    assert np.count_nonzero(rows[0]) > 10 and np.count_nonzero(rows[7]) > 3
    assert all(np.count_nonzero(rows[k]) > nfrms[k] // 2 for k in (10, 11, 12, 13))
    for k, (x, n) in enumerate(utts):
        alone = track(ctx, FS, 0.005, [x], [n])
        assert same_bits(alone["f0"][0], rows[k]), k
        if n:
            assert same_bits(alone["cand"][0], cands[k]), k
            m = np.count_nonzero(cands[k][:, 0:7], axis=1)
            want = tref.viterbi(cands[k][:, 0:8], cands[k][:, 8:16], cands[k][:, 16:24], m, cands[k][0, 23])
            assert same_bits(rows[k], want), k                             # and every length walks its back pointers right


@pytest.mark.parametrize("refine", [0, 1])
def test_in_place_and_feeds_analysis(ctx, refine):
    utts = [make_speechlike(u, nx=9000) for u in (0, 1)]
    xs = [x for x, _ in utts]; nfrms = [len(f) for _, f in utts]
    sopt = llsm.make_soptions(FS)

    def everything(b):
        return {a: b.download(a) for a in OTHER_IDS}

    a = make_batch(ctx, FS, 0.005, xs, nfrms, f0_refine=refine)
    c = make_batch(ctx, FS, 0.005, xs, nfrms, f0_refine=refine)
    try:
        # every array filled by an analysis and a synthesis from the generator's track; then the call under test
        a.upload(llsm.A_F0, np.concatenate([f for _, f in utts]))
        a.analyze(); a.synthesize(sopt, seed=11)
        before = everything(a)
        a.track_f0()
        after = everything(a)
        for k in OTHER_IDS:
            assert same_bits(before[k], after[k]), k
        f0 = a.download(llsm.A_F0)
        assert np.count_nonzero(f0) > 10
        # device-written F0 against the same row uploaded from the host
        a.analyze(); a.synthesize(sopt, seed=11)
        c.upload(llsm.A_F0, f0)
        c.analyze(); c.synthesize(sopt, seed=11)
        ctx.sync()
        ra, rc = everything(a), everything(c)
        for k in OTHER_IDS:
            assert same_bits(ra[k], rc[k]), k
        assert same_bits(a.download(llsm.A_F0), c.download(llsm.A_F0))
    finally:
        a.close(); c.close()


def test_refusals_leave_the_row(ctx):
    L = llsm.load()
    prefix = "llsm_gpu_batch_track_f0:"
    x = make_speechlike(0, nx=4000)[0]
    b = make_batch(ctx, FS, 0.005, [x], [18])
    e = llsm.Batch(ctx, llsm.make_aoptions(), FS, [0, 0], [3, 2])         # frames but no samples
    z = make_batch(ctx, FS, 0.005, [x], [0])                              # no frames
    try:
        mark = np.linspace(100, 200, 18).astype(np.float32)
        b.upload(llsm.A_F0, mark)
        e.upload(llsm.A_F0, mark[:5])
        with pytest.raises(llsm.LlsmError):
            b.debug_plane(5)                                                # no call yet
        nan, inf = float("nan"), float("inf")
        bad_f0 = [dict(fmin=nan), dict(threshold=nan), dict(fmin=0.0), dict(fmin=600.0), dict(fmax=30000.0), dict(fmin=495.0),
                  dict(threshold=0.0), dict(threshold=1.5), dict(silence_rel=-1.0), dict(window_extra=0), dict(smooth=2),
                  dict(keep_cmndf=3), dict(fmin=10.0)]
        bad_track = [dict(cand_threshold=nan), dict(jump_cost=nan), dict(octave_cost=inf), dict(cand_threshold=0.0),
                     dict(cand_threshold=1.5), dict(unvoiced_cost=-0.1), dict(switch_cost=-0.1), dict(jump_cost=-0.1),
                     dict(octave_cost=-0.1)]
        for kw in bad_f0:
            o = llsm.make_f0_options(**kw)
            assert L.llsm_gpu_batch_track_f0(b.h, C.byref(o), None) == -1, kw
            assert L.llsm_gpu_last_error().decode().startswith(prefix), kw
        for kw in bad_track:
            t = llsm.make_f0_track_options(**kw)
            assert L.llsm_gpu_batch_track_f0(b.h, None, C.byref(t)) == -1, kw
            assert L.llsm_gpu_last_error().decode().startswith(prefix), kw
            with pytest.raises(llsm.LlsmError):
                b.track_f0(**kw)
        assert L.llsm_gpu_batch_track_f0(e.h, None, None) == -1
        assert L.llsm_gpu_last_error().decode().startswith(prefix)
        ctx.sync()
        assert same_bits(b.download(llsm.A_F0), mark) and same_bits(e.download(llsm.A_F0), mark[:5])
        with pytest.raises(llsm.LlsmError):
            b.debug_plane(5)                                                # still none
        assert L.llsm_gpu_batch_track_f0(z.h, None, None) == 0              # a batch without frames: nothing to do
        b.estimate_f0(keep_cmndf=1)                                         # the estimator does not make a candidate plane
        with pytest.raises(llsm.LlsmError):
            b.debug_plane(5)
        b.upload(llsm.A_F0, mark)
        assert L.llsm_gpu_batch_track_f0(b.h, None, None) == 0              # NULL, NULL: the defaults
        assert b.debug_plane(5).shape == (18 * 24,)
        assert not same_bits(b.download(llsm.A_F0), mark)
    finally:
        b.close(); e.close(); z.close()
