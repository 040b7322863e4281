"""The noise filter of the offline synthesis judged on its own input, in float64, from the reference alone (DESIGN.md
section 8, "noise filter on its own input").  Nothing here reads a kernel: the inputs, the scale T, the yardstick Y and the
additive term A come from the two builds of the oracle, the number formats and the geometry.

  T[n]   = sum of frame_rms[i] over the live frames whose N-sample output span holds n (float64 oracle)
  (a)    |y[n] - y64[n]| <= (4 Y_u + A_u) EPS T[n] at every sample, Y_u = max |y32 - y64| / (EPS T) of the utterance
  (b)    rms(y - y64) / rms(T) <= KAPPA EPS over every hop-long segment
  zeros  T[n] == 0  ->  y[n] is +0.0; every non-finite value is listed
"""
import math

import numpy as np

from oracle.oracle import Params

EPS = 2.0 ** -24
BOUND_MAX = 512.0          # no utterance may need a bound (4 Y_u + A_u) above this: 3.1e-5 of T
GATE_DB = -100.0           # layer0.c:578: a frame whose PSD peak is below this is dropped
GATE_MARGIN_DB = 1.0       # every frame's peak is at least this far from the gate
LOGRESBIAS_DB = 1.6286014  # LOG2IN(LOGRESBIAS): what the filter takes off a PSDRES row (llsm_oracle.c)
# KAPPA = 4 x the largest per-hop ratio rms(y32 - y64) / (EPS rms(T)) the float32 oracle reaches over every utterance of
# every configuration below (26.3), rounded up (tests/test_noise_filter_host.py recomputes and asserts it)
KAPPA = 106.0
CREST = 5.0                # largest |sample| / rms of a Gaussian over the 2^17 samples an utterance here has at most:
                           # sqrt(2 ln 2^17) = 4.85


def follow_product_conventions(oracles, names):
    """every switchable convention of the oracle builds set to the product's value (the builds are shared by the session)"""
    import libllsm2_amd as llsm
    L = llsm.load()
    for o in oracles:
        for name in names:
            o.set_convention(name, L.llsm_gpu_get_convention(name.encode()))


def _iround(v):
    v = np.asarray(v, np.float64)
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)


def geometry(o, thop, fs, nfrm):
    """(nwin, N, centres[nfrm], ny, hop) as the oracle's index functions give them"""
    nwin = o.lib.o_idx_nwin_filt(thop, fs)
    N = o.lib.o_nextpow2(nwin * 1.2 + 32)
    c = np.array([o.lib.o_idx_center(i, thop, fs) for i in range(nfrm)], np.int64)
    return nwin, N, c, o.ny(nfrm, thop, fs), float(np.float32(thop) * np.float32(fs))


def hop_edges(ny, hop):
    return np.unique(np.concatenate([_iround(np.arange(0.0, ny / hop + 1.0) * hop).clip(0, ny), [ny]]))


def scale(centres, N, ny, frame_rms):
    T = np.zeros(ny)
    for c, r in zip(centres, frame_rms):
        if r > 0:
            a, b = max(int(c) - N // 2, 0), min(int(c) + N // 2, ny)
            if a < b:
                T[a:b] += r
    return T


def additive_A(p, has, N, hop):
    """What the device does after its sums and a sequential float32 evaluation does not, in units of EPS T[n], term by term
    (DESIGN.md section 8 has the derivation):
      gain, independent per bin (bounds b EPS, summed in quadrature, the sample's error CREST standard deviations at most):
        two float32 products in the exponent's argument a = t ln 10 / 20 (the scaling by ln 10 / 20, then by log2 e in
        front of the hardware exp2): b = |a| each; the hardware exp2, 1 ulp: b = 2; fmaf(e, 44100 / fs, 1e-8): b = 1/2
        (under the root); the correctly rounded reciprocal root: b = 1; the product of the two: b = 1
      gain, common to all bins (a smooth change of the filter: |error| <= b EPS |y[n]| <= b EPS CREST T[n]):
        the float32 values of ln 10 / 20 (two roundings) and of log2 e: b = 3 |a|; 44100 / fs rounded: b = 1/2
      after the inverse transform: 1 / N is a power of two (exact); the fade is one product, b = 1 on |frame sample| <=
      CREST frame_rms; the ring adds round m - 1 times on a partial sum of at most CREST T[n], m = the frames over a sample
    with |a| the largest over the live frames' target levels psd [+ PSDRES - 1.6286] dB."""
    live = p.psd.max(axis=1) >= GATE_DB if p.nfrm else np.zeros(0, bool)
    if not live.any():
        return 0.0
    t = p.psd + np.where(np.asarray(has, bool)[:, None], p.psdres - LOGRESBIAS_DB, 0.0)
    a = float(np.abs(t[live]).max()) * math.log(10.0) / 20.0
    m = int(math.floor((N + 1) / max(hop, 1.0))) + 1
    independent = math.sqrt(2 * a * a + 2.0 ** 2 + 0.5 ** 2 + 1.0 + 1.0)
    common = 3 * a + 0.5
    return CREST * (independent + common + 1.0 + (m - 1))


class Ref:
    """float64 and float32 oracle on one utterance's excitation x (float32): y64, y32, T, Y, A, bound, per-hop yardstick"""

    def __init__(self, o64, o32, p, has, fs, x):
        self.p, self.has, self.fs = p, np.asarray(has, np.int32), fs
        x = np.asarray(x, np.float32)
        self.nwin, self.N, self.c, self.ny, self.hop = geometry(o64, p.thop, fs, p.nfrm)
        assert len(x) == self.ny, (len(x), self.ny)
        self.y64, self.frame_rms = o64.filter_noise(p, fs, x.astype(np.float64), self.has)
        y32, _ = o32.filter_noise(p.astype(np.float32), fs, x, self.has)
        self.y32 = y32.astype(np.float64)
        self.T = scale(self.c, self.N, self.ny, self.frame_rms)
        self.edges = hop_edges(self.ny, self.hop)
        self.A = additive_A(p, self.has, self.N, self.hop)
        m32 = measure(self.y32, self)
        self.Y, self.hop32 = m32["a_units"], m32["b_units"]
        self.bound = 4.0 * self.Y + self.A

    def conditions(self):
        """[] or what keeps this utterance from being a fair input"""
        bad = []
        if self.bound > BOUND_MAX:
            bad.append(("bound over %g" % BOUND_MAX, self.bound, self.Y, self.A))
        pk = self.p.psd.max(axis=1) if self.p.nfrm else np.zeros(0)
        near = np.flatnonzero(np.abs(pk - GATE_DB) < GATE_MARGIN_DB)
        if near.size:
            bad.append(("PSD peak within %g dB of the gate" % GATE_MARGIN_DB, near.tolist()))
        if not (np.all(np.isfinite(self.y64)) and np.all(np.isfinite(self.y32))):
            bad.append(("non-finite reference",))
        return bad


def measure(y, ref):
    """errors of candidate y against ref in units of EPS: a_units = max |y - y64| / (EPS T) where T > 0 (and where),
    b_units = max over hop-long segments of rms(y - y64) / (EPS rms(T)), the samples with T == 0 that are not +0.0, and
    the non-finite samples"""
    yf = np.asarray(y)
    y = yf.astype(np.float64)
    assert len(y) == ref.ny, (len(y), ref.ny)
    out = {"nonfinite": np.flatnonzero(~np.isfinite(y)).tolist()}
    d = np.abs(np.where(np.isfinite(y), y, 0.0) - ref.y64)
    pos = ref.T > 0
    zero_ok = (yf == 0) & ~np.signbit(yf)
    out["nonzero_uncovered"] = np.flatnonzero(~pos & ~zero_ok).tolist()
    if pos.any():
        r = d[pos] / (EPS * ref.T[pos])
        k = int(np.argmax(r))
        out["a_units"], out["a_at"] = float(r[k]), int(np.flatnonzero(pos)[k])
    else:
        out["a_units"], out["a_at"] = 0.0, -1
    e2 = np.concatenate([[0.0], np.cumsum(d * d)])
    t2 = np.concatenate([[0.0], np.cumsum(ref.T * ref.T)])
    worst, where = 0.0, -1
    for s, e in zip(ref.edges[:-1], ref.edges[1:]):
        if e <= s or t2[e] - t2[s] <= 0:
            continue                                      # (a hop without scale: the zeros rule covers it)
        v = math.sqrt((e2[e] - e2[s]) / (t2[e] - t2[s])) / EPS
        if v > worst:
            worst, where = v, int(s)
    out["b_units"], out["b_at"] = worst, where
    return out


def judge(y, ref):
    """measure() + the two ratios that must stay below 1 and the list of failed rules"""
    m = measure(y, ref)
    m["a_ratio"] = m["a_units"] / ref.bound if ref.bound > 0 else (0.0 if m["a_units"] == 0 else math.inf)
    m["b_ratio"] = m["b_units"] / KAPPA
    m["failed"] = [k for k, bad in (("a", m["a_ratio"] > 1.0), ("b", m["b_ratio"] > 1.0),
                                    ("zeros", bool(m["nonzero_uncovered"])), ("finite", bool(m["nonfinite"]))) if bad]
    return m


# ---------------------------------------------------------------- inputs

# (name, fs, thop, N, frames of the long utterance); the route each one is meant to reach is asserted by the GPU module
GEOMETRIES = [
    ("8k_5ms", 8000.0, 0.005, 128, 41),
    ("16k_5ms", 16000.0, 0.005, 256, 41),
    ("16k_10ms", 16000.0, 0.010, 512, 41),
    ("44k_5ms", 44100.0, 0.005, 1024, 41),
    ("44k_hop413", 44100.0, 413.0 / 44100.0, 1024, 41),
    ("44k_hop200_5", 44100.0, 200.5 / 44100.0, 1024, 41),
    ("44k_10ms", 44100.0, 0.010, 2048, 41),
    ("48k_20ms", 48000.0, 0.020, 4096, 41),
    ("96k_20ms", 96000.0, 0.020, 8192, 41),
    ("96k_36ms", 96000.0, 0.036, 16384, 8),
]
NPSD_1024 = (5, 64, 128, 129, 256, 257, 300)      # either side of TQ = 2, of TQ = NF_TQ and of the aliased form
FUSED_SIZES = (256, 512, 1024, 2048)
ROUTE_WF, ROUTE_LDS, ROUTE_SCRATCH, ROUTE_FUSED = 1, 2, 3, 100    # llsm_gpu_plan_index case 17 (100 + 10 ALIAS + TQ)


def configuration_names():
    """the names configurations() gives, without the product (for parametrising)"""
    out = []
    for name, fs, thop, N, nlong in GEOMETRIES:
        if name == "44k_5ms":
            out += ["%s_npsd%d" % (name, n) for n in NPSD_1024]
        elif name in ("16k_5ms", "16k_10ms", "44k_10ms"):
            out += [name + "_npsd64", name + "_fit", name + "_over"]
        else:
            out.append(name + "_npsd64")
    return out + [g + "_fnyq_" + t for g in ("44k_5ms", "48k_20ms") for t in ("below", "above")]


def configurations(route):
    """{name: dict(fs, thop, N, nlong, npsd, fnyq, route)} of the host and the GPU module; route: the kernel the
    configuration is meant to reach when the fused kernel is wanted.  The argument route(fused, npsd, thop, fs) is the
    product's route function (llsm_gpu_plan_index case 17): it only tells the widest row that still lands in the exchange
    buffer at the fused sizes other than 1024 (_fit; _over is one point wider)."""
    out = {}

    def add(name, g, npsd, code, fnyq=None):
        _, fs, thop, N, nlong = g
        out[name] = dict(name=name, fs=fs, thop=thop, N=N, nlong=nlong, npsd=npsd, fnyq=fnyq, route=code)

    for g in GEOMETRIES:
        name, fs, thop, N, nlong = g
        plain = ROUTE_FUSED + 12 if N in FUSED_SIZES else ROUTE_SCRATCH if N > 8192 else ROUTE_LDS
        if name == "44k_5ms":
            for n in NPSD_1024:
                add("%s_npsd%d" % (name, n), g, n, ROUTE_FUSED + (12 if n <= 128 else 14 if n <= 256 else 1))
            continue
        add(name + "_npsd64", g, 64, plain)
        if name in ("16k_5ms", "16k_10ms", "44k_10ms"):
            fit = max(n for n in range(2, 258) if route(1, n, thop, fs) >= ROUTE_FUSED + 10)
            add(name + "_fit", g, fit, ROUTE_FUSED + (12 if fit <= 128 else 14))
            add(name + "_over", g, fit + 1, ROUTE_FUSED + 1)
    for g in GEOMETRIES:                                    # PSD rows on another axis than the synthesis rate's
        if g[0] in ("44k_5ms", "48k_20ms"):
            for tag, k in (("below", 0.8), ("above", 1.25)):
                add("%s_fnyq_%s" % (g[0], tag), g, 64, ROUTE_FUSED + 12 if g[3] in FUSED_SIZES else ROUTE_LDS,
                    fnyq=float(np.float32(k * g[1] / 2)))
    assert list(out) == configuration_names()
    return out


def _rows(r, nfrm, npsd, level, rough=False):
    """speech-like target rows: a 12 dB tilt and a ripple of at most 1 dB per point (rough: +-10 dB per point up to 128
    points, the same swing per Hz beyond: the float32 interpolation position moves the gain by the slope per point, and
    300 points at +-10 dB put the float32 oracle itself at 115 EPS, a bound of 603)"""
    tilt = -12.0 * np.linspace(0.0, 1.0, npsd)
    swing = 10.0 * min(1.0, 128.0 / npsd)
    rip = r.uniform(-swing, swing, (nfrm, npsd)) if rough else r.uniform(-0.5, 0.5, (nfrm, npsd))
    return level + tilt[None, :] + rip


def make_utterances(fs, thop, npsd, N, nlong, fnyq=None):
    """[(name, Params float32-rounded in float64, has_psdres)] of one batch; every row value is a float32 number"""
    hop = float(np.float32(thop) * np.float32(fs))
    out = []

    def new(name, nfrm, seed, level=-20.0, rough=False, edc=1e-2):
        r = np.random.default_rng(seed)
        p = Params(nfrm, 4, 0, npsd, 2, thop, fs / 2 if fnyq is None else fnyq, [fs / 4], np.float64)
        if nfrm:
            p.psd[:] = _rows(r, nfrm, npsd, level, rough)
            p.psdres[:] = r.uniform(-2.0, 2.0, (nfrm, npsd))
            p.edc[:] = edc
        has = np.ones(nfrm, np.int32)
        out.append([name, p, has])
        return p, has

    # 60 dB PSD steps every third frame, edc steps of 60 dB elsewhere; has_psdres alternating within pairs in both orders,
    # then a run with and a run without
    p, has = new("steps", nlong, 1)
    for i in range(nlong):
        if (i // 3) % 2:
            p.psd[i] -= 60.0
        if ((i + 1) // 4) % 2:
            p.edc[i] = 1e-8
    q = max(nlong // 4, 1)
    has[:] = 0
    has[0:q:2] = 1; has[q + 1:2 * q:2] = 1; has[2 * q:3 * q] = 1
    # a dead frame as partner a and as partner b, then a dead run longer than N / hop (uncovered samples inside)
    run = int(math.ceil(N / hop)) + 2
    p, has = new("dead", 8 + run + 3, 2)
    p.psd[2] = -120.0; p.psd[5] = -120.0; p.psd[8:8 + run] = -120.0
    p, has = new("all_dead", 5, 3); p.psd[:] = -120.0
    new("one_frame", 1, 4); new("two_frames", 2, 5); new("three_frames", 3, 6)
    new("frameless", 0, 7)
    new("loud_before", 8, 8, level=-10.0)
    new("quiet", 8, 9, level=-70.0)                     # 1000 x below its neighbours
    new("loud_after", 8, 10, level=-10.0)
    new("rough", 8, 11, rough=True)
    p, has = new("near_gate", 4, 12, level=-97.0)       # live: the peak between 2 and 4 dB above the gate
    p.psd[:, 0] = -98.0
    for u in out:                                       # float32 numbers on both sides
        u[1] = u[1].astype(np.float32).astype(np.float64)
    return [tuple(u) for u in out]


def excitation_stand_in(o64, p, fs, seed):
    """the float64 oracle's own excitation, rounded to float32 (host test: the device's plane 15 is not there)"""
    return o64.noise_excitation(o64.soptions(fs), p, seed=seed).astype(np.float32)
