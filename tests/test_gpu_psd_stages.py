"""-m gpu: k_psd_frames* and k_kalman each on ITS OWN input against float64, value by value.

The whole-chain parity bounds on the smoothed PSD (tests/gpu_common.py CONDITIONED / CEILING: up to 1 dB next to DC and
Nyquist) are bounds on  x -> spectrogram -> envelope -> Q -> smoother, whose envelope stage is ill-conditioned.  The two
kernels after the envelope are not: given the planes they read, their output is determined to float32 rounding.  So

  Stage A  plane 1 of llsm_gpu_batch_debug_plane (the log periodogram k_psd_frames_wf<8..11> / k_psd_frames write)
           against psd_frames_ref of the DOWNLOADED residual;
  Stage B  PSD / PSDRES against kalman_ref(float64) of the DOWNLOADED planes 0 and 1, at every (frame, point) within
           4 Y + 5e-5 dB, Y that utterance's distance between the float32 and the float64 restatement on the same planes
           (tests/psd_stage_reference.py; proven against the oracle by tests/test_psd_stage_host.py).

Plane 0 (the envelope) is an input here and is never judged: tests/test_gpu_spgm_env.py is its judge, value by value
against float64 of the uploaded samples and F0.  Frame counts sit below, at and above one, two and three
chunks of KAL_CHUNK = 8 frames (the checkpoint spacing, the prefetch distance, the rotation of the register buffers) with
unlike neighbours, so that a wavefront straddling utterances has lanes of different length; the PSD sizes put a dozen
utterances, two, one or half of one on a wavefront.

Stage A bound.  tests/test_gpu_fft.py allows the transform 4e-6 of the RMS spectrum; d ln P = 2 dX / |X|, so a bin at
the RMS level moves by 8e-6, plus half an ulp (1e-6) of a stored logarithm of magnitude <= 23: about 1e-5 for the
metric |plane1 - ref| min(1, |X| / S) (psd_stage_reference.psd_frames_metric).  PSD_FRAMES_BOUND (psd_stage_reference.py) is 4 x the
worst value measured over the nine batches (the table in DESIGN.md section 8), and may never exceed 4e-5.

Stage B's additive 5e-5 dB covers what the numpy yardstick does not contain: hardware exp2 / log2 and the multiplication
of an exponent of magnitude up to 33 by log2 e, together about 1.5e-5 dB."""
import numpy as np
import pytest

import libllsm2_amd as llsm
from conftest import make_speechlike
from gpu_common import report
from psd_stage_reference import KAL_ADD_DB, PSD_FRAMES_BOUND, _iround, kalman_check, kalman_ref, psd_frames_full, psd_frames_metric

pytestmark = pytest.mark.gpu

COUNTS = [1, 2, 3, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 47, 48, 49, 0, 72, 73]        # 535 frames
COUNTS_BIG = [1, 2, 9, 24, 25]
K8 = dict(nchannel=2, chanfreq=[1500.0], maxnhar=60)
K16 = dict(nchannel=3, chanfreq=[1000.0, 3000.0])
# id: (fs, hop, nfft of the PSD window, kernel, npsd, frame counts, analysis options)
CONFIGS = {
    "8k_256_npsd300": (8000.0, 0.005, 256, "k_psd_frames_wf", 300, COUNTS, K8),       # more points than bins
    "16k_512_npsd5": (16000.0, 0.005, 512, "k_psd_frames_wf", 5, COUNTS, K16),         # a dozen utterances per wavefront
    "44k_1024_npsd129": (44100.0, 0.005, 1024, "k_psd_frames_wf", 129, COUNTS, {}),    # wavefronts straddle utterances
    "44k_1024_npsd64": (44100.0, 0.005, 1024, "k_psd_frames_wf", 64, COUNTS, {}),      # one utterance per wavefront
    "44k_1024_npsd128": (44100.0, 0.005, 1024, "k_psd_frames_wf", 128, COUNTS, {}),    # ... per workgroup
    "44k_2048": (44100.0, 0.010, 2048, "k_psd_frames_wf", 129, COUNTS, {}),
    "48k_4096": (48000.0, 0.020, 4096, "k_psd_frames", 129, COUNTS_BIG, {}),           # LDS
    "96k_8192": (96000.0, 0.020, 8192, "k_psd_frames", 129, COUNTS_BIG, {}),           # LDS, largest
    "96k_16384": (96000.0, 0.025, 16384, "k_psd_frames", 129, COUNTS_BIG, {}),         # global scratch
}
CONV = [(0, 0), (1, 0), (0, 1), (1, 1)]                 # (kalman_init, interp1u_exclusive)


def make_inputs(fs, thop, counts):
    """(xs, f0s, i_zero, i_short): make_speechlike cut to nx = round((n + 1) thop fs) with the F0 track cut or
    zero-padded to n, one per count; then an all-zero utterance of 9 frames and one of 100 samples with 3 frames."""
    hop = float(np.float32(thop) * np.float32(fs))
    xs, f0s = [], []
    for u, n in enumerate(counts):
        nx = int(_iround((n + 1) * hop))
        x, f0 = make_speechlike(300 + u, nx=max(nx, int(_iround(40 * hop))), fs=fs, thop=thop)
        f = np.zeros(n, np.float32)
        f[:min(n, len(f0))] = f0[:n]
        xs.append(np.ascontiguousarray(x[:nx])); f0s.append(f)
    xs.append(np.zeros(int(_iround(10 * hop)), np.float32)); f0s.append(np.zeros(9, np.float32))
    xs.append(make_speechlike(399, nx=4000, fs=fs, thop=thop)[0][1000:1100].copy()); f0s.append(np.zeros(3, np.float32))
    return xs, f0s, len(counts), len(counts) + 1


def run_batch(ctx, fs, thop, npsd, akw, xs, f0s, want_planes=True):
    ao = llsm.make_aoptions(f0_refine=0, thop=thop, npsd=npsd, **akw)
    b = llsm.Batch(ctx, ao, fs, [len(x) for x in xs], [len(f) for f in f0s])
    try:
        b.upload(llsm.A_X, np.concatenate(xs)); b.upload(llsm.A_F0, np.concatenate(f0s))
        ctx.set_profiling(True); ctx.reset_profile()
        try:
            b.analyze(); ctx.sync()
            prof = ctx.profile()
        finally:
            ctx.set_profiling(False)
        total = sum(len(f) for f in f0s)
        out = dict(prof=prof, frm_off=np.concatenate([[0], np.cumsum([len(f) for f in f0s])]),
                   nx_off=np.concatenate([[0], np.cumsum([len(x) for x in xs])]),
                   psd=b.download(llsm.A_PSD).reshape(total, npsd), psdres=b.download(llsm.A_PSDRES).reshape(total, npsd),
                   has=b.download(llsm.A_HAS_PSDRES))
        if want_planes:
            out["xres"] = b.download(llsm.A_XRES)
            out["env"] = b.debug_plane(0).reshape(total, -1); out["z"] = b.debug_plane(1).reshape(total, -1)
        return out
    finally:
        b.close()


@pytest.fixture(scope="module")
def ctx():
    c = llsm.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def runs(ctx):
    """one batch per configuration, analysed once and shared by the stage tests"""
    cache = {}

    def get(cid):
        if cid not in cache:
            fs, thop, nfft, kernel, npsd, counts, akw = CONFIGS[cid]
            xs, f0s, iz, ish = make_inputs(fs, thop, counts)
            r = run_batch(ctx, fs, thop, npsd, akw, xs, f0s)
            r.update(i_zero=iz, i_short=ish)
            cache[cid] = r
        return cache[cid]
    return get


def _assert_path(cid, r):
    """the row tests what it says: transform size from the plane width, kernel from the launch profile"""
    fs, thop, nfft, kernel, npsd, counts, akw = CONFIGS[cid]
    assert r["z"].shape[1] == nfft // 2 + 1 and r["env"].shape == r["z"].shape, (cid, r["z"].shape)
    other = "k_psd_frames" if kernel == "k_psd_frames_wf" else "k_psd_frames_wf"
    assert r["prof"].get(kernel, (0, 0))[1] >= 1 and other not in r["prof"], (cid, sorted(r["prof"]))
    assert r["prof"].get("k_kalman", (0, 0))[1] >= 1, (cid, sorted(r["prof"]))


@pytest.mark.parametrize("cid", list(CONFIGS))
def test_stage_a_log_periodogram(runs, cid):
    """k_psd_frames* on the downloaded residual: EVERY value of plane 1 within PSD_FRAMES_BOUND of float64 under the
    metric of the module docstring; nothing excluded, no share allowed to miss."""
    fs, thop = CONFIGS[cid][:2]
    r = runs(cid)
    _assert_path(cid, r)
    logp, mag = psd_frames_full(r["xres"], r["nx_off"], r["frm_off"], thop, fs)
    assert np.all(np.isfinite(r["z"]))
    met = psd_frames_metric(r["z"], logp, mag)
    w = np.unravel_index(int(np.argmax(met)), met.shape)
    raw = np.abs(r["z"].astype(np.float64) - logp)
    rec = dict(worst=float(met[w]), at_frame=int(w[0]), at_bin=int(w[1]), bound=PSD_FRAMES_BOUND, values=int(met.size),
               raw_worst=float(raw.max()), floor_values=int(np.count_nonzero(logp == np.log(1e-10))))
    report("psd_stage_a_" + cid, rec)
    assert met[w] <= PSD_FRAMES_BOUND, rec


def _stage_b(r, cid, fs, npsd, ki=0, ex=0, tag=""):
    total = int(r["frm_off"][-1])
    assert np.array_equal(r["has"], np.ones(total, np.int32))
    assert np.all(np.isfinite(r["psd"])) and np.all(np.isfinite(r["psdres"]))
    assert np.all(np.isfinite(r["env"]))                       # (an input: only that the reference can be formed)
    bad, st = kalman_check(r["psd"], r["psdres"], r["env"], r["z"], r["frm_off"], npsd, fs, ki, ex)
    # the all-zero utterance: Q at its floor, z at log 1e-10 -- the additive term alone
    zs = slice(int(r["frm_off"][r["i_zero"]]), int(r["frm_off"][r["i_zero"] + 1]))
    p64, r64 = kalman_ref(r["env"][zs], r["z"][zs], [0, zs.stop - zs.start], npsd, fs, ki, ex, np.float64)
    st["zero_utt_err_psd"] = float(np.max(np.abs(r["psd"][zs] - p64))); st["zero_utt_err_psdres"] = float(np.max(np.abs(r["psdres"][zs] - r64)))
    st["bound_add_db"] = KAL_ADD_DB
    report("psd_stage_b_" + cid + tag, st)
    assert not bad, (cid, ki, ex, bad[:8], st)
    assert st["zero_utt_err_psd"] <= KAL_ADD_DB and st["zero_utt_err_psdres"] <= KAL_ADD_DB, st
    return st


@pytest.mark.parametrize("cid", list(CONFIGS))
def test_stage_b_kalman(runs, cid):
    """k_kalman on the downloaded planes: every (frame, point) of PSD and PSDRES within 4 Y + 5e-5 dB of float64."""
    fs, npsd = CONFIGS[cid][0], CONFIGS[cid][4]
    r = runs(cid)
    _assert_path(cid, r)
    _stage_b(r, cid, fs, npsd)


@pytest.mark.parametrize("ki,ex", CONV[1:])
def test_stage_b_kalman_conventions(ctx, ki, ex):
    """the 1024-point / npsd = 129 batch under the other three combinations of kalman_init and interp1u_exclusive
    ((0, 0) is test_stage_b_kalman's)"""
    cid = "44k_1024_npsd129"
    fs, thop, nfft, kernel, npsd, counts, akw = CONFIGS[cid]
    xs, f0s, iz, ish = make_inputs(fs, thop, counts)
    L = llsm.load()
    assert L.llsm_gpu_get_convention(b"kalman_init") == 0 and L.llsm_gpu_get_convention(b"interp1u_exclusive") == 0
    try:
        assert L.llsm_gpu_set_convention(b"kalman_init", ki) == 0 and L.llsm_gpu_set_convention(b"interp1u_exclusive", ex) == 0
        r = run_batch(ctx, fs, thop, npsd, akw, xs, f0s)
    finally:
        L.llsm_gpu_set_convention(b"kalman_init", 0); L.llsm_gpu_set_convention(b"interp1u_exclusive", 0)
    r.update(i_zero=iz, i_short=ish)
    _assert_path(cid, r)
    _stage_b(r, cid, fs, npsd, ki, ex, tag="_init%d_excl%d" % (ki, ex))


def test_bits_do_not_depend_on_wavefront_neighbours(ctx, runs):
    """No tolerance: with npsd = 64 an utterance is one wavefront, and whether a chunk takes the branch-free path is a
    ballot over that wavefront -- but which workgroup it shares, and where its checkpoints lie, follows from its
    position in the batch.  The utterance order reversed, and the utterances of 8, 24 and 25 frames each alone: the
    PSD / PSDRES bits of an utterance are the same."""
    cid = "44k_1024_npsd64"
    fs, thop, nfft, kernel, npsd, counts, akw = CONFIGS[cid]
    r = runs(cid)
    xs, f0s, _, _ = make_inputs(fs, thop, counts)
    nu = len(xs)

    def rows(res, k):
        sl = slice(int(res["frm_off"][k]), int(res["frm_off"][k + 1]))
        return res["psd"][sl].view(np.int32), res["psdres"][sl].view(np.int32)
    rev = run_batch(ctx, fs, thop, npsd, akw, xs[::-1], f0s[::-1], want_planes=False)
    for k in range(nu):
        for a, b_, name in zip(rows(r, k), rows(rev, nu - 1 - k), ("psd", "psdres")):
            assert np.array_equal(a, b_), ("reversed", k, len(f0s[k]), name, int(np.count_nonzero(a != b_)))
    for n in (8, 24, 25):
        k = counts.index(n)
        solo = run_batch(ctx, fs, thop, npsd, akw, [xs[k]], [f0s[k]], want_planes=False)
        for a, b_, name in zip(rows(r, k), rows(solo, 0), ("psd", "psdres")):
            assert np.array_equal(a, b_), ("alone", n, name, int(np.count_nonzero(a != b_)))
