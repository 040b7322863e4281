"""Sample-by-sample yardsticks of the real-time synthesis (llsmrt): plain numpy.

What is here needs neither a GPU nor the oracle library: the hop schedule of llsmrt.c restated in float32 (rt_schedule), the
float32 error scale of every output sample of the harmonic part in the stream's geometry (rt_sin_scale), the metrics built
on it (rt_metrics), the synthetic cases that reach the branches of rt.cpp / kernels.hip no analysed waveform reaches
(rt_case), and named ways of spoiling a correct stream (FAULTS).  tests/test_rt_reference_host.py shows on the CPU that the
metrics flag every fault under the bounds of tests/test_gpu_rt_samples.py; that is what entitles the GPU module to them.
The two functions at the end that run an oracle take the oracle object from their caller.
"""
import numpy as np

F32 = np.float32
LOGRESBIAS_DB = 0.375 / 2.3025851 * 10.0                    # LOG2IN(LOGRESBIAS), llsmrt.c:513-520: 1.6286 dB

# The bounds of the GPU module (tests/test_gpu_rt_samples.py); the host module flags every fault under the same numbers.
# ysin_local: gpu_common.SYN_CEILING["ysin_local"] -- the real-time path runs the device function synth_frame of the offline
# path -- or the float32 oracle's own distance from float64 on the case, whichever is larger (KAPPA_F32 = 1).
# ynoise_local: gpu_common.SYN_CEILING["ynoise_local"]; the real-time filter is the offline noise_filter_pair.
YSIN_LOCAL, YNOISE_LOCAL = 60.0, 6e-5
# the one-ulp response of the float64 oracle that a case must stay under: a quarter of the noise bound
ULP_CONDITION = 1.5e-5


def _f(v):
    return F32(v)


def nextpow2(x):
    return int(2.0 ** np.ceil(np.log2(float(x))))


def rt_schedule(nfrm, thop, fs):
    """llsmrt.c:110-129 (update_cycle) and :157-191 (create) as oracle/rt_oracle.c restates them: every product and
    difference rounded to float32, then floored.  Returns a dict: h0 (the hop after create), curr_nhop[nfrm],
    next_nhop[nfrm] (feed i hands out next_nhop[i] samples), cycle[nfrm] (the cycle counter feed i synthesises with), nfft,
    sin_pos, latency, n (the stream's length)."""
    fs32, th = _f(fs), _f(thop)

    def update(cycle, curr):
        prev = curr
        c = _f(cycle + th)
        curr = int(np.floor(float(_f(c * fs32))))
        cycle = _f(c - _f(_f(prev) / fs32))
        nxt = int(np.floor(float(_f(_f(cycle + th) * fs32))))
        return cycle, curr, nxt

    _c, h0, _n = update(_f(0), 1)
    cycle = _f(0)                                              # llsmrt.c:190
    nfft = nextpow2(float(_f(th * fs32)) * 2.2 + 32)
    sin_pos = -2 * h0 - nfft // 2
    curr = h0
    cur_l, nxt_l, cyc_l = [], [], []
    for _ in range(nfrm):
        cycle, curr, nxt = update(cycle, curr)
        cur_l.append(curr); nxt_l.append(nxt); cyc_l.append(float(cycle))
    nxt_a = np.array(nxt_l, np.int64)
    return dict(h0=h0, curr_nhop=np.array(cur_l, np.int64), next_nhop=nxt_a, cycle=np.array(cyc_l), nfft=nfft,
                sin_pos=sin_pos, latency=-sin_pos - h0, n=int(nxt_a.sum()), fs=float(fs))


def _hann_larger(n):
    """the larger of the periodic and the symmetric Hann window of n points: only its first sample is 0"""
    if n == 1:
        return np.ones(1)
    j = np.arange(n, dtype=np.float64)
    return np.maximum(0.5 - 0.5 * np.cos(2 * np.pi * j / (n - 1)), 0.5 - 0.5 * np.cos(2 * np.pi * j / n))


def rt_sin_scale(params, sched):
    """S[o] for every output sample o of the harmonic part: the analogue of gpu_common.sin_error_scale in the stream's
    geometry.  The timeline's cell 0 is where the sinusoid ring stands after create; feed i advances it by h_i =
    curr_nhop[i] to T_i = sum_{j <= i} h_j and adds its frame to the cells [T_i - 2 h_i, T_i) (frame 0 reaches h_0 cells
    back before cell 0: blank ring cells that the stream hands out later); output sample o reads cell o + h_0 + sin_pos.
    A frame's weight: the larger Hann window of 2 h_i points times sum_k |a_ik| over k < min(nhar_i, nfft) (llsmrt.c:280);
    none for f0 = 0."""
    curr, h0, nfft = sched["curr_nhop"], sched["h0"], sched["nfft"]
    T = np.cumsum(curr)
    base = 2 * int(curr.max()) + 2 * h0                        # cells below 0 that a frame or a read can touch
    cells = np.zeros(int(T[-1]) + base + 1)
    for i in range(params.nfrm):
        if not params.f0[i] > 0:
            continue
        K = max(0, min(int(params.nhar[i]), nfft, params.maxnhar))
        asum = float(np.sum(np.abs(np.asarray(params.ampl[i, :K], np.float64))))
        h = int(curr[i])
        lo = int(T[i]) - 2 * h + base
        cells[lo:lo + 2 * h] += _hann_larger(2 * h) * asum
    c = np.arange(sched["n"]) + h0 + sched["sin_pos"] + base
    S = np.zeros(sched["n"])
    ok = (c >= 0) & (c < len(cells))
    S[ok] = cells[c[ok]]
    return S


def rel_rms(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    den = np.sqrt(np.mean(b ** 2))
    return float(np.sqrt(np.mean((a - b) ** 2)) / den) if den > 0 else float(np.sqrt(np.mean((a - b) ** 2)))


def rt_noise_local(yap, yap_ref, sched, floor_rel=1e-7):
    """gpu_common.noise_local over the stream's REAL hop boundaries (the cumulative sums of next_nhop): the largest, over
    hops, of rms(yap - yap_ref) over the hop against rms(yap_ref) over the hop and one window (2 h0) on either side, with a
    floor of floor_rel x max |yap_ref|.  Returns (value, first sample of the hop)."""
    yn = np.asarray(yap, np.float64); yo = np.asarray(yap_ref, np.float64)
    ny = len(yo)
    if ny == 0:
        return 0.0, -1
    edges = np.concatenate([[0], np.cumsum(sched["next_nhop"])]).astype(np.int64)
    nwin = 2 * sched["h0"]
    e2 = np.concatenate([[0.0], np.cumsum((yn - yo) ** 2)])
    r2 = np.concatenate([[0.0], np.cumsum(yo ** 2)])
    floor = floor_rel * float(np.max(np.abs(yo)))
    worst, where = 0.0, -1
    for s, e in zip(edges[:-1], edges[1:]):
        if e <= s:
            continue
        err = np.sqrt((e2[e] - e2[s]) / (e - s))
        if err == 0.0:
            continue
        a, b = max(s - nwin, 0), min(e + nwin, ny)
        ref = np.sqrt((r2[b] - r2[a]) / (b - a))
        v = err / (ref + floor) if ref + floor > 0 else np.inf
        if v > worst:
            worst, where = float(v), int(s)
    return worst, where


def rt_metrics(params, sched, yp, yp_ref, yap, yap_ref, S=None):
    """ysin_local = max_o |yp - yp_ref| / (2^-24 S[o]) over S > 0, and where; ysin_nonzero_uncovered: samples with S = 0
    where either side is not exactly 0; ynoise_local (rt_noise_local) and where; the two whole-stream relative RMS values."""
    yp = np.asarray(yp, np.float64); yp_ref = np.asarray(yp_ref, np.float64)
    if S is None:
        S = rt_sin_scale(params, sched)
    m = {}
    pos = S > 0
    r = np.abs(yp - yp_ref)[pos] / (2.0 ** -24 * S[pos])
    m["ysin_local"] = float(r.max()) if r.size else 0.0
    m["ysin_local_at"] = int(np.flatnonzero(pos)[int(np.argmax(r))]) if r.size else -1
    m["ysin_nonzero_uncovered"] = int(np.count_nonzero((yp[~pos] != 0.0) | (yp_ref[~pos] != 0.0)))
    m["ysin_uncovered_samples"] = int(np.count_nonzero(~pos))
    m["ynoise_local"], m["ynoise_local_at"] = rt_noise_local(yap, yap_ref, sched)
    m["p_rel_rms"] = rel_rms(yp, yp_ref)
    m["ap_rel_rms"] = rel_rms(yap, yap_ref)
    return m


def rt_violations(m, ysin_f32=0.0):
    """[(metric, value, bound)] of m outside the bounds of the GPU module; ysin_f32: the float32 oracle's ysin_local on the
    same case"""
    bad = []
    if not m["ysin_local"] <= max(YSIN_LOCAL, ysin_f32):
        bad.append(("ysin_local", m["ysin_local"], max(YSIN_LOCAL, ysin_f32), m["ysin_local_at"]))
    if m["ysin_nonzero_uncovered"] != 0:
        bad.append(("ysin_nonzero_uncovered", m["ysin_nonzero_uncovered"], 0))
    if not m["ynoise_local"] <= YNOISE_LOCAL:
        bad.append(("ynoise_local", m["ynoise_local"], YNOISE_LOCAL, m["ynoise_local_at"]))
    return bad


# ---------------------------------------------------------------- the cases
class RtParams:
    """The flat layer-0 rows of one stream, with the attributes of oracle.oracle.Params (so that Oracle.cparams and
    test_gpu_rt.chunk_from_oracle take it as it is)."""
    FIELDS = ("f0", "nhar", "ampl", "phse", "psd", "psdres", "edc", "nhar_e", "eenv_ampl", "eenv_phse")

    def __init__(self, nfrm, maxnhar, maxnhar_e, npsd, nchannel, thop, fnyq, chanfreq, dtype=np.float64):
        self.nfrm, self.maxnhar, self.maxnhar_e, self.npsd, self.nchannel = nfrm, maxnhar, maxnhar_e, npsd, nchannel
        self.thop, self.fnyq, self.chanfreq = thop, fnyq, list(chanfreq)
        self.dtype = d = np.dtype(dtype)
        self.f0 = np.zeros(nfrm, d); self.nhar = np.zeros(nfrm, np.int32)
        self.ampl = np.zeros((nfrm, maxnhar), d); self.phse = np.zeros((nfrm, maxnhar), d)
        self.psd = np.full((nfrm, npsd), -120.0, d); self.psdres = np.zeros((nfrm, npsd), d)
        self.edc = np.full((nfrm, nchannel), 1e-5, d); self.nhar_e = np.zeros(nfrm, np.int32)
        self.eenv_ampl = np.zeros((nfrm, nchannel, maxnhar_e), d); self.eenv_phse = np.zeros((nfrm, nchannel, maxnhar_e), d)

    def astype(self, dtype):
        q = RtParams(self.nfrm, self.maxnhar, self.maxnhar_e, self.npsd, self.nchannel, self.thop, self.fnyq, self.chanfreq, dtype)
        for f in self.FIELDS:
            a = getattr(self, f)
            setattr(q, f, np.ascontiguousarray(a.astype(q.dtype if a.dtype.kind == "f" else a.dtype)))
        return q

    def copy(self):
        return self.astype(self.dtype)


# name: synthesis rate, analysed rate (fnyq = half of it), thop, hops, nchannel, maxnhar_e, npsd, maxnhar, F0, band edges,
# the form rt_hop_form (kernels.hip) gives the hop under the default mode 3, and what the case reaches.
#   RT_HOP_CHIP (k_rt_hop2) wants a window 2 h <= 1024, nfft <= 2048, npsd <= 1024 and its LDS (rt_hop2_lds) within 64 KB;
#   RT_HOP_ONE (k_rt_hop) wants max(2 (min(nfft, 2048) + 4) x 8, (2 nfft + 1 + npsd) x 8 + 64) bytes within 64 KB;
#   else RT_HOP_TWO (k_rt_front + k_rt_back): nfft = 4096 alone is 8 bytes over.
CASES = {
    "bench": dict(fs=44100.0, fs_ana=44100.0, thop=0.005, nfrm=60, nch=4, me=4, npsd=256, maxnhar=100, f0=150.0,
                  chanfreq=[2000.0, 4000.0, 8000.0], form="RT_HOP_CHIP"),        # hops 220 / 221, nfft 1024
    "k400": dict(fs=44100.0, fs_ana=44100.0, thop=200.5 / 44100.0, nfrm=40, nch=2, me=3, npsd=129, maxnhar=400, f0=55.0,
                 chanfreq=[4000.0], form="RT_HOP_CHIP"),                         # K = 400 > 256: second trip of rt_stage_rows
    "clamp": dict(fs=44100.0, fs_ana=44100.0, thop=0.002, nfrm=60, nch=4, me=4, npsd=256, maxnhar=400, f0=55.0,
                  chanfreq=[2000.0, 4000.0, 8000.0], form="RT_HOP_CHIP"),        # nfft 256 < nhar 400; hops 86 .. 90
    "wide": dict(fs=48000.0, fs_ana=48000.0, thop=0.011, nfrm=30, nch=8, me=8, npsd=1100, maxnhar=300, f0=80.0,
                 chanfreq=[1000.0, 2000.0, 3000.0, 4000.0, 6000.0, 8000.0, 12000.0], form="RT_HOP_ONE"),
    "two_launch": dict(fs=48000.0, fs_ana=48000.0, thop=0.020, nfrm=25, nch=3, me=6, npsd=200, maxnhar=160, f0=110.0,
                       chanfreq=[2000.0, 6000.0], form="RT_HOP_TWO"),            # nfft 4096; <4, 8> envelope instantiation
    "syn16k": dict(fs=16000.0, fs_ana=44100.0, thop=0.005, nfrm=40, nch=4, me=4, npsd=256, maxnhar=100, f0=150.0,
                   chanfreq=[2000.0, 4000.0, 8000.0], form="RT_HOP_CHIP"),       # band 4 starts AT the synthesis Nyquist
    "syn12k": dict(fs=12000.0, fs_ana=44100.0, thop=0.005, nfrm=40, nch=4, me=4, npsd=256, maxnhar=100, f0=150.0,
                   chanfreq=[2000.0, 4000.0, 8000.0], form="RT_HOP_CHIP"),       # band 3 straddles it
    "mono": dict(fs=16000.0, fs_ana=16000.0, thop=77.25 / 16000.0, nfrm=50, nch=1, me=0, npsd=32, maxnhar=20, f0=140.0,
                 chanfreq=[], form="RT_HOP_CHIP"),                               # no band filter, no envelope harmonics
    "gates": dict(fs=44100.0, fs_ana=44100.0, thop=0.005, nfrm=60, nch=4, me=4, npsd=256, maxnhar=100, f0=150.0,
                  chanfreq=[2000.0, 4000.0, 8000.0], form="RT_HOP_CHIP"),
}
CASE_NAMES = tuple(CASES)
# gates: frames that are silent (-130 dB), the pair on either side of the -100 dB gate, voiced frames without harmonics
GATES_SILENT, GATES_BELOW, GATES_ABOVE, GATES_NHAR0 = (10, 11, 12, 13), 20, 21, (25, 33)
_cache = {}


def rt_expected_form(c, sched):
    """rt_hop_form (kernels.hip) under mode 3 for every hop of the schedule, from its conditions: the set of forms met"""
    N, npsd, nch, me_rt = sched["nfft"], c["npsd"], c["nch"], max(c["me"], 1)
    mh = min(N, 2048)
    cap, ntemplate = int(c["fs"] * 0.2), int(c["fs"])

    def pair_lds(extra=0):
        return ((N + N // 2 + N // 2 + 1 + npsd) * 8 + 64 + extra + 15) // 16 * 16

    forms = set()
    for nhop, nxt in zip(sched["curr_nhop"], sched["next_nhop"]):
        nwin = 2 * int(nhop)
        if max(2 * (mh + 4) * 8, pair_lds()) > 64 * 1024:
            forms.add("RT_HOP_TWO"); continue
        nx0 = max(N, 2 * (mh + 4))
        lds2 = pair_lds((nx0 - N) * 8 + (2 * nch * nwin + 5 * nwin + 2 * (nch + 2 * nch * me_rt) + 8) * 4)
        chip = nwin <= 1024 and nhop <= 512 and N <= 2048 and N > nhop and nxt <= 512 and nxt <= N and N < cap and \
            nwin < cap and nhop < ntemplate and nch * me_rt <= 256 and npsd <= 1024 and lds2 <= 64 * 1024
        forms.add("RT_HOP_CHIP" if chip else "RT_HOP_ONE")
    return forms


def rt_case(name):
    """(fs_synth, params, seed) of a case of CASES: synthetic rows, written directly, rounded to float32 and handed out as
    float64 (what both sides synthesise).  Voiced frames carry nhar = K harmonics, K = maxnhar or the last harmonic under
    0.999 of the synthesis Nyquist, with a_k = 0.3 / K x U(0.5, 1.5) -- every harmonic at least a third of its share, so one
    dropped harmonic of 400 costs 2^24 / 1200, about 1e4 units of ysin_local -- and uniform phases; F0 steps between the
    case's F0 and 5 % under it.  Envelope rows: random phases, amplitudes at most 3e-6, and in sum at most 6e-6 of a band's
    edc = 1e-5 (the band envelope stays above 0.4 edc, away from the knee of its 1e-8 floor, which would be a conditioning
    of the case and not an error of either side).  psd = -60 dB + N(0, 3 dB) per frame plus a slow ripple over the bins,
    psdres = N(0, 3 dB).  Frames 0 .. 2 and five frames mid-stream are unvoiced (gates: see below)."""
    if name in _cache:
        return _cache[name]
    c = CASES[name]
    seed = 7100 + CASE_NAMES.index(name) * 10
    rng = np.random.default_rng(20261021 + CASE_NAMES.index(name))
    n, K0, me, nch, npsd = c["nfrm"], c["maxnhar"], c["me"], c["nch"], c["npsd"]
    pr = RtParams(n, K0, me, npsd, nch, c["thop"], c["fs_ana"] / 2.0, c["chanfreq"])
    voiced = np.ones(n, bool)
    if name == "gates":
        voiced[40:46] = False                                  # frame 0 voiced; six unvoiced frames mid-stream
    else:
        voiced[:3] = False; voiced[n // 2: n // 2 + 5] = False
    nyq = c["fs"] / 2.0
    for i in range(n):
        f0 = c["f0"] * (1.0 - 0.05 * rng.integers(0, 2))
        ph = rng.uniform(-np.pi, np.pi, K0); u = rng.uniform(0.5, 1.5, K0)
        eph = rng.uniform(-np.pi, np.pi, (nch, me)); ea = rng.uniform(0.0, 1.0, (nch, me)) * min(3e-6, 6e-6 / max(me, 1))
        pr.psd[i] = -60.0 + 3.0 * rng.standard_normal() + 4.0 * np.sin(2 * np.pi * 1.5 * np.arange(npsd) / npsd + rng.uniform(0, 6.28))
        pr.psdres[i] = 3.0 * rng.standard_normal(npsd)
        if not voiced[i]:
            continue
        K = min(K0, int(np.floor(0.999 * nyq / f0)))
        pr.f0[i] = f0; pr.nhar[i] = K
        pr.ampl[i, :K] = 0.3 / K * u[:K]; pr.phse[i, :K] = ph[:K]
        pr.nhar_e[i] = me
        pr.eenv_ampl[i] = ea; pr.eenv_phse[i] = eph
    if name == "gates":
        for i in GATES_SILENT:
            pr.psd[i] -= 70.0                                  # -130 dB
        for i, peak in ((GATES_BELOW, -100.5), (GATES_ABOVE, -99.5)):
            lvl = pr.psd[i].astype(F32).astype(np.float64) + pr.psdres[i].astype(F32).astype(np.float64) - LOGRESBIAS_DB
            pr.psd[i] += peak - lvl.max()
        for i in GATES_NHAR0:
            pr.nhar[i] = 0; pr.ampl[i] = 0; pr.phse[i] = 0
    pr = pr.astype(F32).astype(np.float64)
    _cache[name] = (c["fs"], pr, seed)
    return _cache[name]


def rt_level_peak(pr, i):
    """the largest level llsmrt's gate sees for frame i: max_j psd + psdres - LOG2IN(LOGRESBIAS), in float32"""
    return float(np.max(pr.psd[i].astype(F32) + (pr.psdres[i].astype(F32) - F32(LOGRESBIAS_DB))))


def rt_perturb_noise_rows(pr, rng):
    """the psd, psdres, edc and envelope rows one float32 unit off: v (1 +- 2^-24), random signs, rounded to float32"""
    q = pr.copy()
    for f in ("psd", "psdres", "edc", "eenv_ampl", "eenv_phse"):
        a = getattr(q, f)
        b = (a.astype(F32) * (1 + rng.choice([-1, 1], size=a.shape) * 2.0 ** -24)).astype(F32)
        setattr(q, f, np.ascontiguousarray(b.astype(np.float64)))
    return q


# ---------------------------------------------------------------- faults
# A fault takes a context -- name, pr, sched, S, yp, yap (the correct float64 streams) and rerun(params) -> (yp, yap), a
# second synthesis on altered rows -- and returns the spoiled (yp, yap), or None where the case has nothing to spoil.
def _hop(ctx, k=None):
    """a voiced hop away from the stream's ends: [a, b) in output samples"""
    edges = np.concatenate([[0], np.cumsum(ctx["sched"]["next_nhop"])])
    S = ctx["S"]
    order = range(len(edges) // 3, len(edges) - 1) if k is None else [k]
    for j in order:
        if np.all(S[edges[j] + 1:edges[j + 1]] > 0):
            return int(edges[j]), int(edges[j + 1])
    raise AssertionError("no voiced hop")


def _fault_sample(ctx):
    """one sample off by 1e-3 of S there, where the stream is quiet: the covered sample with the largest S at which the
    whole-stream 1e-5 gate is still blind by a factor of two (1e-3 S <= 0.5e-5 rms(yp) sqrt(n): a voicing onset)"""
    S, yp = ctx["S"], ctx["yp"].copy()
    quiet = 0.5e-5 * np.sqrt(np.mean(yp ** 2)) * np.sqrt(len(yp)) / 1e-3
    cand = np.flatnonzero((S > 0) & (S <= quiet))
    o = int(cand[np.argmax(S[cand])])
    yp[o] += 1e-3 * S[o]
    return yp, ctx["yap"]


def _fault_sample_loud(ctx):
    a, b = _hop(ctx)
    o = a + int(np.argmax(ctx["S"][a:b]))
    yp = ctx["yp"].copy(); yp[o] += 1e-3 * ctx["S"][o]
    return yp, ctx["yap"]


def _fault_uncovered(ctx):
    z = np.flatnonzero(ctx["S"] == 0)
    z = z[z > ctx["sched"]["latency"] + 3 * ctx["sched"]["h0"]]
    if not z.size:
        return None
    yp = ctx["yp"].copy(); yp[z[len(z) // 2]] = 1e-9
    return yp, ctx["yap"]


def _fault_shift(ctx):
    a, b = _hop(ctx)
    yp = ctx["yp"].copy(); yp[a:b] = ctx["yp"][a - 1:b - 1]
    return yp, ctx["yap"]


def _voiced_frame(pr, minhar):
    idx = np.flatnonzero((pr.f0 > 0) & (pr.nhar > minhar))
    return int(idx[len(idx) // 2]) if idx.size else None


def _fault_nhar(limit, only):
    def f(ctx):
        if ctx["name"] != only:
            return None
        q = ctx["pr"].copy(); i = _voiced_frame(q, limit)
        q.nhar[i] = limit
        return ctx["rerun"](q)[0], ctx["yap"]
    return f


def _fault_noise_gain(ctx):
    a, b = _hop(ctx)
    yap = ctx["yap"].copy(); yap[a:b] *= 1 + 1e-3
    return ctx["yp"], yap


def _fault_prev_psd(ctx):
    q = ctx["pr"].copy(); i = q.nfrm // 3
    q.psd[i] = q.psd[i - 1]; q.psdres[i] = q.psdres[i - 1]
    return ctx["yp"], ctx["rerun"](q)[1]


def _fault_gate(ctx):
    if ctx["name"] != "gates":
        return None
    q = ctx["pr"].copy(); q.psd[GATES_ABOVE] -= 50.0
    return ctx["yp"], ctx["rerun"](q)[1]


FAULTS = {
    "sample_1e-3_of_S": _fault_sample,                  # one sample of yp off by 1e-3 of S there, at a voicing onset
    "nonzero_where_uncovered": _fault_uncovered,        # 1e-9 where no voiced frame reaches
    "sample_1e-3_of_S_loudest": _fault_sample_loud,     # the same where S is largest
    "hop_shifted_one_sample": _fault_shift,
    "k400_frame_with_256_harmonics": _fault_nhar(256, "k400"),      # the second trip of rt_stage_rows lost
    "clamp_at_half_nfft": _fault_nhar(128, "clamp"),    # llsmrt.c:280 with nfft / 2
    "noise_hop_gain_1e-3": _fault_noise_gain,
    "hop_filtered_with_previous_psd": _fault_prev_psd,
    "gate_m99p5_db_silent": _fault_gate,                # the frame just above the -100 dB gate treated as silent
}
# the faults the whole-stream 1e-5 gate of tests/test_gpu_rt.py lets through on every case that has them
FAULTS_OLD_GATE_PASSES = ("sample_1e-3_of_S", "nonzero_where_uncovered")


# ---------------------------------------------------------------- oracle runs, shared by the modules that use them
_runs = {}


def oracle_streams(o, name, seed_offset=0):
    """(yp, yap, latency) of oracle `o` (float64 or float32 build) on a case, seed + seed_offset; computed once"""
    key = (np.dtype(o.dtype).name, name, seed_offset)
    if key not in _runs:
        fs, pr, seed = rt_case(name)
        yp, yap, lat = o.rt_run(o.soptions(fs), pr.astype(o.dtype), capacity=4096, seed=seed + seed_offset)
        yp = np.asarray(yp, np.float64); yap = np.asarray(yap, np.float64)
        yp.setflags(write=False); yap.setflags(write=False)
        _runs[key] = (yp, yap, lat)
    return _runs[key]


def case_yardsticks(o64, o32, name):
    """(sched, S, ysin_local of the float32 oracle against float64) of a case; computed once"""
    key = ("yard", name)
    if key not in _runs:
        fs, pr, _seed = rt_case(name)
        sched = rt_schedule(pr.nfrm, pr.thop, fs)
        S = rt_sin_scale(pr, sched)
        S.setflags(write=False)
        yp, yap, _ = oracle_streams(o64, name)
        yp32, yap32, _ = oracle_streams(o32, name)
        m32 = rt_metrics(pr, sched, yp32, yp, yap32, yap, S)
        _runs[key] = (sched, S, m32)
    return _runs[key]
