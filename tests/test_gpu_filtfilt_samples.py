"""k_filtfilt, sample by sample, against the float64 oracle's chebyfilt of the same float32 samples -- on every path the
kernel and its planner (engine.cpp build_jobs) have: the guarded first / last tile and the prefetched interior tiles of the
single-job path (llsm_subband_energy), pad = min(filtfilt_pad, n - 1), band-pass jobs fused into two passes over an interior
[M, n - M) with two end jobs in the reference's order, signals of >= 65 536 samples cut into time segments with halos, the
ragged signals of a batch at every 16-byte alignment, the analysis plane (squared band signals, llsm_gpu_batch_debug_plane 2)
and the synthesis plane (band-limited templates, plane 3).  EVERY sample of every plane is compared; thresholds (M, M', the
segments) come from the planner (llsm_gpu_plan_index case 16), not from a second derivation here.

The bound is derived, not measured.  The recursion is float64, so what separates the kernel from the oracle is the float32
STORES of a chain: a zero-phase pair F B stores its forward output (tmp) and its result -- S = 2 for a single section and
for a fused band-pass (both sections per pass, no store between them), S = 4 for the band-pass in the reference's order
(F_hp B_hp F_lp B_lp).  A store is off by at most 2^-24 of a value that is at most ||h||_1 max|x| after one pass and
||h||_1^2 max|x| after two, and what follows it amplifies by at most ||h||_1 per pass, so every store contributes at most
2^-24 ||h||_1^2 max|x| to the result: with the margin of 2 of the issue (the float64 arithmetic, the odd extension's values
beyond max|x|)

    |y_kernel - y_oracle| <= e = 2 S 2^-24 ||h||_1^2 max|x|   (+ 1e-9 ||h||_1^2 max|x| where the job is fused or cut:
                                                                 the transient the planner lets die to 1e-9)

||h||_1: the L1 norm of the ONE-PASS impulse response of the section -- of the cascade hp * lp for a band-pass --, computed
here in float64 from the oracle's own design (o_get_chebyshev_filter).  The analysis plane holds y^2, formed in float32 from
the stored y: |y_k^2 - y_o^2| <= 2 |y_o| e + e^2 + 2^-24 (|y_o| + e)^2, per sample.  Where a stage does not write (a
template row beyond min(20000, ny) + 128, the rows of channels from the synthesis Nyquist up -- layer0.c:562 generates no
template for them, so there is no value to hold them to) the plane must be UNTOUCHED: bit-identical before and after the run.

Every batch is first run on another signal of ten times the level: a sample the second run does not write keeps a value far
outside the bound.  Derived bounds and measured worst cases per path: LAB.md."""
import ctypes as C

import numpy as np
import pytest

import libllsm2_amd as llsm
from gpu_common import report

pytestmark = pytest.mark.gpu
P = llsm.P_fp
EPS = 2.0 ** -24
MARGIN = 2.0
TRANSIENT = 1e-9
TILE = 28 * 64                        # IIR_SEG x 64 lanes
DEFAULT_CF = [2000.0, 4000.0, 8000.0]
WORST = {}                            # path -> the case with the largest error / bound (written by gpu_common.report as parity_filtfilt_samples.json)


@pytest.fixture(scope="module")
def L():
    L = llsm.load()
    L.llsm_subband_energy.restype = P; L.llsm_subband_energy.argtypes = [P, C.c_int, C.c_float, C.c_float]
    import ctypes.util
    L._free = C.CDLL(ctypes.util.find_library("c")).free
    L._free.argtypes = [C.c_void_p]
    return L


@pytest.fixture(scope="module")
def ctx():
    c = llsm.Context(0)
    yield c
    c.close()


# ---- the reference design: ||h||_1 of a band ----
_H = {}


def _impulse(o64, cutoff, highpass, n=16384):
    """one-pass impulse response of the section chebyfilt uses for this normalised cutoff, float64 (every row has died to
    far below 1e-16 of its peak by n: the slowest one reaches 1e-9 after ~1000 samples)"""
    b, a = o64.get_chebyshev_filter(float(cutoff), highpass)
    key = (tuple(b), tuple(a))
    if key not in _H:
        b = b / a[0]; a = a / a[0]
        h = np.zeros(n); z = np.zeros(4)
        for t in range(n):
            x = 1.0 if t == 0 else 0.0
            y = b[0] * x + z[0]
            z[0] = b[1] * x + z[1] - a[1] * y; z[1] = b[2] * x + z[2] - a[2] * y
            z[2] = b[3] * x + z[3] - a[3] * y; z[3] = b[4] * x - a[4] * y
            h[t] = y
        assert np.abs(h[-64:]).max() < 1e-16 * np.abs(h).max()
        _H[key] = h
    return _H[key]


def band_edges(c1, c2):
    """chebyfilt's case split (dsputils.c:51-70) on float32 edges: (c1, c2, kind)"""
    c1 = np.float32(max(c1, 0.0)); c2 = np.float32(min(c2, 0.5))
    kind = "bp" if (c1 != 0 and c2 < np.float32(0.5)) else ("lp" if c1 == 0 else "hp")
    return float(c1), float(c2), kind


def band_l1(o64, c1, c2):
    c1, c2, kind = band_edges(c1, c2)
    if kind == "lp":
        return float(np.abs(_impulse(o64, c2, 0)).sum())
    if kind == "hp":
        return float(np.abs(_impulse(o64, c1, 1)).sum())
    return float(np.abs(np.convolve(_impulse(o64, c1, 1), _impulse(o64, c2, 0))).sum())


def y_bound(l1, xmax, stores, transient):
    """per-sample bound e on the filtered signal; stores: scalar or per-sample array of S"""
    return MARGIN * np.asarray(stores, np.float64) * EPS * l1 * l1 * xmax + (TRANSIENT * l1 * l1 * xmax if transient else 0.0)


def sq_bound(yo, e):
    a = np.abs(yo)
    return 2.0 * a * e + e * e + EPS * (a + e) ** 2


def check(path, where, got, yo, e, square, joints=()):
    """every sample of got against the oracle's yo (float64, unsquared) within the derived bound"""
    got = np.asarray(got, np.float64)
    assert got.shape == yo.shape, (where, got.shape, yo.shape)
    assert np.all(np.isfinite(got)), (where, "non-finite samples at", np.flatnonzero(~np.isfinite(got))[:8])
    e = np.broadcast_to(np.asarray(e, np.float64), yo.shape)
    want, bound = (yo * yo, sq_bound(yo, e)) if square else (yo, e)
    err = np.abs(got - want)
    ratio = err / bound
    k = int(np.argmax(ratio)) if len(ratio) else 0
    rec = dict(where=where, n=len(yo), index=k, err=float(err[k]), bound=float(bound[k]), ratio=float(ratio[k]),
               err_max=float(err.max()), bound_at_err_max=float(bound[int(np.argmax(err))]), index_err_max=int(np.argmax(err)),
               peak=float(np.abs(want).max()))
    if path not in WORST or rec["ratio"] > WORST[path]["ratio"]:
        WORST[path] = rec
        report("filtfilt_samples", WORST)
    bad = np.flatnonzero(err > bound)
    if len(bad):
        js = np.asarray(sorted(joints), np.int64)
        near = [(int(i), int(i) % TILE, int(js[np.argmin(np.abs(js - i))]) if len(js) else None) for i in bad[:8]]
        raise AssertionError((path, where, f"{len(bad)} of {len(yo)} samples over the bound; first (index, index mod tile, nearest joint): {near}",
                              rec))


# ---- signals ----
def noise_chirp(n, seed, level=1.0):
    """white noise at constant level + a chirp from 50 Hz to 0.45 of the rate: every band is excited everywhere"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / max(n, 1)
    return (level * (0.1 * rng.standard_normal(n) + 0.3 * np.sin(2 * np.pi * n * (0.001 * t + 0.2245 * t * t)))).astype(np.float32)


def dc_step(n, seed=0, level=1.0):
    """constant offset with a step in the middle: the low-pass holds the constant from sample 0 (zi), the others stay at 0"""
    x = np.full(n, 0.25, np.float32)
    x[n // 2:] = 0.75
    return (level * x).astype(np.float32)


def impulses(n, joints):
    """single impulses within +-2 samples of every joint (the offset cycles through -2 .. 2)"""
    x = np.zeros(n, np.float32)
    for k, j in enumerate(sorted(set(int(v) for v in joints))):
        p = j + (k % 5) - 2
        if 0 <= p < n:
            x[p] = 1.0 if k % 2 == 0 else -1.0
    if not x.any() and n:
        x[n // 2] = 1.0
    return x


# ---- the planner's view of one (signal, band) ----
class Plan:
    def __init__(self, L, n, fmin, fmax, fs):
        q = lambda k: L.llsm_gpu_plan_index(16, int(n), k, float(fmin), float(fmax), float(fs), 0.0)
        self.n, self.M, self.Mp, self.fused, self.H, self.S, self.lo, self.hi = n, q(0), q(1), q(2), q(3), q(4), q(5), q(6)
        self.w0 = [q(100 + s) for s in range(self.S + 1)]
        assert self.w0[0] == self.lo and self.w0[-1] == self.hi and all(a < b for a, b in zip(self.w0, self.w0[1:])), self.__dict__
        if self.fused:
            assert self.Mp == 2 * self.M + 64 and n >= 4 * self.Mp and (self.lo, self.hi) == (self.M, n - self.M), self.__dict__
        else:
            assert (self.lo, self.hi) == (0, n), self.__dict__

    def joints(self):
        j = list(self.w0[1:-1])
        if self.fused:
            j += [self.M, self.n - self.M]
        return j

    def stores(self, kind):
        """S per sample: 2 for one section and inside a fused band-pass, 4 where the band-pass runs in the reference's order"""
        if kind != "bp":
            return 2.0
        s = np.full(self.n, 4.0)
        if self.fused:
            s[self.lo:self.hi] = 2.0
        return s

    def transient(self):
        return bool(self.fused or self.S > 1)


def bands_of(chanfreq, fs):
    nch = len(chanfreq) + 1
    return [(0.0 if c == 0 else chanfreq[c - 1], fs / 2.0 if c == nch - 1 else chanfreq[c]) for c in range(nch)]


def norm_edges(fmin, fmax, fs):
    """the normalised edges as the product forms them (float32 division)"""
    return float(np.float32(fmin) / np.float32(fs)), float(np.float32(fmax) / np.float32(fs))


# =====================================================================
# single-job path: llsm_subband_energy (one job, never fused, never cut)
# =====================================================================
SINGLE_N = (2, 3, 15, 16, 17, 31, 1761, 1762, 1763, 3553, 3554, 3555, 5347, 5349)
SINGLE_BANDS = ((0.0, 2000.0), (2000.0, 4000.0), (8000.0, 22050.0))
FS = 44100.0


def _subband(L, x, c1, c2):
    p = L.llsm_subband_energy(x.ctypes.data_as(P), len(x), c1, c2)
    a = np.ctypeslib.as_array(p, (len(x),)).copy()
    L._free(C.cast(p, C.c_void_p))
    return a


@pytest.mark.parametrize("pad", (15, 7, 1))
def test_single_job_every_sample(L, o64, pad):
    """n around 1, 2 and 3 tiles of the extended signal (ne = n + 2 pad at the default pad: 1791 / 1792 / 1793, ...; three
    tiles: one is prefetched), the shortest signals (pad = n - 1), three paddings, low- / band- / high-pass"""
    assert L.llsm_gpu_get_convention(b"filtfilt_pad") == 15
    try:
        assert L.llsm_gpu_set_convention(b"filtfilt_pad", pad) == 0
        o64.set_convention("filtfilt_pad", pad)
        for n in SINGLE_N:
            for name, x in (("noise_chirp", noise_chirp(n, 100 + n)), ("dc_step", dc_step(n))):
                xmax = float(np.abs(x).max())
                for fmin, fmax in SINGLE_BANDS:
                    c1, c2 = norm_edges(fmin, fmax, FS)
                    _, _, kind = band_edges(c1, c2)
                    yo = o64.chebyfilt(x, c1, c2)
                    e = y_bound(band_l1(o64, c1, c2), xmax, 4.0 if kind == "bp" else 2.0, False)
                    check(f"single_{kind}", f"pad={pad} n={n} {name}", _subband(L, x, c1, c2), yo, e, True)
    finally:
        L.llsm_gpu_set_convention(b"filtfilt_pad", 15); o64.set_convention("filtfilt_pad", 15)


# =====================================================================
# batch path, analysis: plane 2
# =====================================================================
def _plane(b, which):
    n = b.L.llsm_gpu_batch_debug_plane(b.h, which, None, 0)
    assert n > 0, b.L.llsm_gpu_last_error()
    a = np.zeros(n, np.float32)
    assert b.L.llsm_gpu_batch_debug_plane(b.h, which, a.ctypes.data_as(C.c_void_p), n) == n
    return a


def _analysis_case(L, ctx, o64, tag, fs, chanfreq, lengths, signal):
    """signal(n, joints, u) -> float32[n].  Runs the batch on a louder other signal first, then on the signal, and holds
    every sample of plane 2 to the oracle."""
    ao = llsm.make_aoptions(f0_refine=0, nchannel=len(chanfreq) + 1, chanfreq=list(chanfreq))
    bands = bands_of(chanfreq, fs)
    plans = [[Plan(L, n, fmin, fmax, fs) for fmin, fmax in bands] for n in lengths]
    xs = [signal(n, [j for p in plans[u] for j in p.joints()], u) for u, n in enumerate(lengths)]
    nfrm = [2] * len(lengths)                         # all unvoiced: x_res = x and the stage is cheap
    b = llsm.Batch(ctx, ao, fs, lengths, nfrm)
    try:
        assert L.llsm_gpu_batch_debug_plane(b.h, 2, None, 0) == -1 and b"no analysis" in L.llsm_gpu_last_error()
        assert L.llsm_gpu_batch_debug_plane(b.h, 3, None, 0) == -1 and b"no synthesis" in L.llsm_gpu_last_error()
        b.upload(llsm.A_F0, np.zeros(sum(nfrm), np.float32))
        b.upload(llsm.A_X, np.concatenate([noise_chirp(n, 9000 + u, level=10.0) + np.float32(3.0) for u, n in enumerate(lengths)]))
        b.analyze()
        stale = _plane(b, 2)
        b.upload(llsm.A_X, np.concatenate(xs))
        b.analyze()
        ce = _plane(b, 2).reshape(len(bands), -1)
        assert ce.shape[1] == b.layout.total_samples and not np.array_equal(stale, ce.ravel())
        assert L.llsm_gpu_batch_debug_plane(b.h, 3, None, 0) == -1          # still no synthesis
        x_dev, xres_dev = b.download(llsm.A_X), b.download(llsm.A_XRES)
        assert np.array_equal(x_dev, np.concatenate(xs))
        for u, n in enumerate(lengths):
            o = int(b.x_off[u])
            for c, (fmin, fmax) in enumerate(bands):
                src = (x_dev if fmin > 6000.0 else xres_dev)[o:o + n]
                c1, c2 = norm_edges(fmin, fmax, fs)
                _, _, kind = band_edges(c1, c2)
                pl = plans[u][c]
                yo = o64.chebyfilt(src, c1, c2)
                e = y_bound(band_l1(o64, c1, c2), float(np.abs(src).max()), pl.stores(kind), pl.transient())
                path = "analysis_" + kind + ("_fused" if pl.fused else "") + ("_cut" if pl.S > 1 else "")
                check(path, f"{tag} u={u} n={n} x_off={o} c={c} M={pl.M} S={pl.S}", ce[c, o:o + n], yo, e, True, pl.joints())
        return plans
    finally:
        b.close()


SIGNALS = {
    "noise_chirp": lambda n, joints, u: noise_chirp(n, 500 + u),
    "dc_step": lambda n, joints, u: dc_step(n),
    "impulses": lambda n, joints, u: impulses(n, joints),
}


@pytest.mark.parametrize("sig", sorted(SIGNALS))
def test_analysis_ragged_batch(L, ctx, o64, sig):
    """lengths 4 M' - 1 (unfused) ... 4 M' + 3 (fused + end jobs) of the widest band-pass channel and two short ones: the
    lengths take every residue mod 4, so x_off and n - M' take every 16-byte alignment"""
    Mp = max(Plan(L, 1 << 15, fmin, fmax, FS).Mp for fmin, fmax in bands_of(DEFAULT_CF, FS))
    assert Mp > 0
    lengths = [4 * Mp - 1, 4 * Mp, 4 * Mp + 1, 4 * Mp + 2, 4 * Mp + 3, 1763, 2306]
    assert {n % 4 for n in lengths} == {0, 1, 2, 3} and {int(v) % 4 for v in np.cumsum([0] + lengths[:-1])} == {0, 1, 2, 3}
    plans = _analysis_case(L, ctx, o64, "ragged_" + sig, FS, DEFAULT_CF, lengths, SIGNALS[sig])
    wide = max(range(4), key=lambda c: plans[1][c].Mp)
    assert not plans[0][wide].fused and all(plans[u][wide].fused for u in range(1, 5))


@pytest.mark.parametrize("sig", sorted(SIGNALS))
@pytest.mark.parametrize("n", (65535, 65536, 65539))
def test_analysis_long_signal(L, ctx, o64, n, sig):
    """one utterance just below the cut length (whole) and at / above it (time segments with halos)"""
    plans = _analysis_case(L, ctx, o64, f"long_{n}_{sig}", FS, DEFAULT_CF, [n], SIGNALS[sig])
    if n < 65536:
        assert all(p.S == 1 for p in plans[0])
    else:
        assert all(p.S > 1 for p in plans[0]), [p.S for p in plans[0]]          # the cut happened, for every channel


@pytest.mark.parametrize("sig", ("impulses", "noise_chirp"))
def test_analysis_16k_last_channel_at_nyquist(L, ctx, o64, sig):
    """16 kHz with the default band plan: the last channel's fmin IS Nyquist (a high-pass on the table's last row)"""
    fs = 16000.0
    Mp = max(Plan(L, 1 << 15, fmin, fmax, fs).Mp for fmin, fmax in bands_of(DEFAULT_CF, fs))
    _analysis_case(L, ctx, o64, "16k_" + sig, fs, DEFAULT_CF, [4 * Mp - 1, 4 * Mp, 4 * Mp + 3, 65537], SIGNALS[sig])


@pytest.mark.parametrize("sig", ("impulses", "noise_chirp"))
def test_analysis_three_channels(L, ctx, o64, sig):
    cf = [1500.0, 5000.0]
    Mp = max(Plan(L, 1 << 15, fmin, fmax, FS).Mp for fmin, fmax in bands_of(cf, FS))
    _analysis_case(L, ctx, o64, "3ch_" + sig, FS, cf, [4 * Mp - 1, 4 * Mp, 4 * Mp + 1, 4 * Mp + 2, 4 * Mp + 3, 65538], SIGNALS[sig])


# =====================================================================
# batch path, synthesis: plane 3
# =====================================================================
def _silent_rows(b):
    l = b.layout
    F = l.total_frames
    rows = {aid: np.zeros(b.shape(aid), np.int32 if aid in (llsm.A_NHAR, llsm.A_NHAR_E, llsm.A_HAS_PSDRES) else np.float32)
            for aid in b.PARAM_IDS}
    rows[llsm.A_PSD][:] = -120.0
    rows[llsm.A_EDC][:] = 1e-5
    rows[llsm.A_HAS_PSDRES][:] = 1
    assert rows[llsm.A_F0].shape == (F,)
    return rows


@pytest.mark.parametrize("sig", sorted(SIGNALS))
@pytest.mark.parametrize("fs,thop,nfrm", ((16000.0, 0.00625, (2, 200)), (44100.0, 0.005, (1, 100))))
def test_synthesis_templates(L, ctx, o64, fs, thop, nfrm, sig):
    """ny = 300 (n = 428, unfused) and ny >= 20 000 (n = 20 128) at 16 kHz, where the last channel starts at Nyquist and is
    inactive; a short and a full template at 44.1 kHz, every channel active"""
    ao = llsm.make_aoptions(f0_refine=0, thop=thop)
    bands = bands_of(DEFAULT_CF, fs)
    nys = [L.llsm_gpu_plan_index(5, k, 0, 0.0, thop, fs, 4.0) for k in nfrm]
    ns = [min(20000, ny) + 128 for ny in nys]
    if fs == 16000.0:
        assert nys[0] == 300 and ns == [428, 20128]
    else:
        assert ns[1] == 20128
    b = llsm.Batch(ctx, ao, fs, [0] * len(nfrm), list(nfrm))
    try:
        b.upload_params(_silent_rows(b))
        so = llsm.make_soptions(fs)
        U, nch, ext = b.shape(llsm.A_WHITE)
        assert ext >= max(ns)
        plans = [[Plan(L, n, fmin, fmax, fs) for fmin, fmax in bands] for n in ns]
        active = [fmin < fs / 2.0 for fmin, _ in bands]
        assert any(p.fused for p in plans[1]) and not any(p.fused for p in plans[0])
        white = np.full((U, nch, ext), 5.0, np.float32)           # (beyond the template: nothing may read it)
        loud = np.zeros((U, nch, ext), np.float32)
        for u in range(U):
            for c in range(nch):
                white[u, c, :ns[u]] = SIGNALS[sig](ns[u], plans[u][c].joints(), 7 * u + c)
                loud[u, c] = noise_chirp(ext, 700 + 7 * u + c, level=10.0) + np.float32(3.0)
        b.upload(llsm.A_WHITE, loud)
        b.synthesize(so, 1, injected_white=True)
        stale = _plane(b, 3).reshape(U, nch, ext)
        b.upload(llsm.A_WHITE, white)
        b.synthesize(so, 1, injected_white=True)
        col = _plane(b, 3).reshape(U, nch, ext)
        for u in range(U):
            n = ns[u]
            for c, (fmin, fmax) in enumerate(bands):
                where = f"synth fs={fs} {sig} u={u} n={n} c={c}"
                if not active[c]:
                    # layer0.c:562 stops at the first channel that starts at Nyquist: no template exists for it, none is written
                    assert np.array_equal(col[u, c].view(np.uint32), stale[u, c].view(np.uint32)), where + ": inactive channel written"
                    continue
                assert np.array_equal(col[u, c, n:].view(np.uint32), stale[u, c, n:].view(np.uint32)), where + ": written beyond the template"
                src = white[u, c, :n]
                c1, c2 = norm_edges(fmin, fmax, fs)
                _, _, kind = band_edges(c1, c2)
                pl = plans[u][c]
                yo = o64.chebyfilt(src, c1, c2)
                e = y_bound(band_l1(o64, c1, c2), float(np.abs(src).max()), pl.stores(kind), pl.transient())
                check("synthesis_" + kind + ("_fused" if pl.fused else ""), where, col[u, c, :n], yo, e, False, pl.joints())
        assert active.count(False) == (1 if fs == 16000.0 else 0)
    finally:
        b.close()
