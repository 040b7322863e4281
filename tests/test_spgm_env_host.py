"""CPU: the numpy restatement of tests/spgm_env_reference.py IS the float64 oracle's spectral-envelope stage, its plan
integers are the product's, its float32 form lies inside the bound formed from the float64 one on the very inputs the GPU
test uses, the bound is small where the caps say it must be, the inputs hold every branch the GPU test names, and the
checker notices errors the whole-chain parity bounds let through.

tests/test_gpu_spgm_env.py judges k_spgm_env_wf / k_spgm_env with spgm_env_ref / spgm_env_check; this module is what
entitles it to."""
import math

import numpy as np
import pytest

import libllsm2_amd as llsm
import spgm_env_reference as R
from spgm_env_reference import (CAP_1E2, CAP_1E3, CONFIGS, EPS, EPS_FFT, FAULTS, FLAT_F0, I_FLAT, I_LOW, I_LOWMIX, I_SHORT, I_SINGLE,
                                I_SPEECH, I_V200, I_ZERO, KAPPA, KAPPA_MEASURED, LEVEL, NAMES, NFRM, cache_pair, config_options,
                                frame_index, offsets, plan_values, sizes, spgm_env_bound, spgm_env_check, spgm_env_inputs,
                                spgm_env_ref)
from test_invariance_host import WF_REFERENCE_CASE, WF_SHAPES, case_signal, oracle_stages, spgm_sizes, takes_fallback

_CASES = {}


def _case(cid):
    """inputs, float64 reference, bound and float32 restatement of a configuration, formed once"""
    if cid not in _CASES:
        fs, thop, kw = config_options(cid)
        xs, f0s = spgm_env_inputs(cid)
        ref, B = spgm_env_bound(xs, f0s, fs, thop)
        _CASES[cid] = dict(fs=fs, thop=thop, kw=kw, xs=xs, f0s=f0s, ref=ref, B=B, r32=spgm_env_ref(xs, f0s, fs, thop, np.float32))
    return _CASES[cid]


# ---------------------------------------------------------------- the float64 restatement is the oracle
# float64's form of the bound: the unit 2^-53 for EPS, the transform's allowance scaled by the same factor
# (EPS_FFT / EPS = 67 units, for transforms of up to 4096 points and |L| <= 23.03), sine and window evaluated directly
# (two units).  It is a bound on the ORACLE's rounding against the restatement's: 1e-13 ... 1e-11 nepers.
EPS64 = 2.0 ** -53
F64 = dict(eps=EPS64, eps_fft=EPS_FFT / EPS * EPS64, eps_x=EPS_FFT / EPS * EPS64, ph=2.0)


@pytest.mark.parametrize("cid", list(CONFIGS))
def test_float64_restatement_is_the_oracle(o64, cid):
    """every utterance of every configuration through the oracle's analysis; its stage-2 hook (the resampled envelope)
    against spgm_env_ref(float64) with the oracle's float64 normaliser, at every point"""
    c = _case(cid)
    nb = R.norm_base_oracle()
    assert abs(nb / R.norm_base_product() - 1.0) <= 2.0 * EPS                  # (the product rounds the same sum to float32)
    worst = 0.0
    for u, (x, f0) in enumerate(zip(c["xs"], c["f0s"])):
        got, _ = oracle_stages(o64, c["fs"], c["thop"], c["kw"], x, f0, stages=(2,))
        mine, tol = spgm_env_bound([x], [f0], c["fs"], c["thop"], norm_base=nb, **F64)
        assert got[2].shape == mine.shape, (cid, NAMES[u])
        ratio = np.abs(got[2] - mine) / tol
        worst = max(worst, float(ratio.max()))
        assert tol.max() <= 1e-9 or u == I_ZERO or not x.any(), (cid, NAMES[u], tol.max())
        assert ratio.max() <= 1.0, (cid, NAMES[u], float(np.abs(got[2] - mine).max()), float(tol.min()))
    print("oracle %-15s worst |oracle - restatement| / float64 bound %.3f" % (cid, worst))


def test_the_pinned_fix_case_is_the_oracle_too(o64):
    fs, thop, kw, x, f0 = case_signal(WF_REFERENCE_CASE)
    got, _ = oracle_stages(o64, fs, thop, kw, x, f0, stages=(2,))
    mine, tol = spgm_env_bound([x], [f0], fs, thop, norm_base=R.norm_base_oracle(), **F64)
    assert np.all(np.abs(got[2] - mine) <= tol)


# ---------------------------------------------------------------- the plan integers are the product's
@pytest.mark.parametrize("cid", list(CONFIGS))
def test_plan_values_are_the_products(cid):
    """ws, centre, N, nfft_psd, nwin_psd: llsm_gpu_plan_index cases 10, 0 and 4 and the launcher's size rule"""
    L = llsm.load()
    fs, thop, _ = config_options(cid)
    _, f0s = spgm_env_inputs(cid)
    nwin, N, npsd = sizes(fs, thop)
    assert L.llsm_gpu_plan_index(4, 0, 0, 0.0, thop, fs, 0.0) == nwin
    assert spgm_sizes(fs, thop) == (N, npsd)
    kernel, shape = CONFIGS[cid][2:]
    assert takes_fallback(fs, thop) == (kernel == "k_spgm_env"), (cid, N, npsd)
    if shape is not None:
        assert shape in WF_SHAPES and (int(math.log2(N)), int(math.log2(N // npsd))) == shape
    f0 = np.concatenate(f0s)
    utt, idx = frame_index(offsets(f0s))
    ws, c = plan_values(f0, idx, fs, thop)
    for g in range(len(f0)):
        assert L.llsm_gpu_plan_index(10, nwin, 0, float(f0[g]), thop, fs, 4.0) == ws[g], (cid, g)
        assert L.llsm_gpu_plan_index(0, int(idx[g]), 0, 0.0, thop, fs, 4.0) == c[g], (cid, g)


def test_every_instantiation_is_reached():
    assert {CONFIGS[c][3] for c in CONFIGS if CONFIGS[c][3] is not None} == WF_SHAPES
    lds = {c: sizes(*CONFIGS[c][:2]) for c in CONFIGS if CONFIGS[c][2] == "k_spgm_env"}
    assert lds["lds_256"][1] == 256 and lds["lds_4096"][1] == 4096
    assert lds["lds_512_fold4"][1:] == (512, 128) and lds["lds_fold8"][1] // lds["lds_fold8"][2] == 8
    assert lds["lds_psd_longer"][2] > lds["lds_psd_longer"][1]


# ---------------------------------------------------------------- the float32 restatement is inside the bound; kappa; caps
def test_float32_restatement_is_inside_the_bound():
    """(a) and (b) on every configuration; the largest per-frame ratio is what KAPPA stands on (4 x, at most 1); the
    shares of B > 1e-3 and B > 1e-2 under their caps.  The rows printed here are the table of DESIGN.md section 8."""
    worst, where = 0.0, None
    for cid in CONFIGS:
        c = _case(cid)
        assert c["r32"].dtype == np.float32 and c["ref"].dtype == np.float64
        bad, st = spgm_env_check(c["r32"], c["ref"], c["B"])
        print("restatement %-15s frames %d points %6d  point %.3f at %s  frame %.4f at %d (median %.4f)  B > 1e-3: %.4f  B > 1e-2: %.5f"
              "  B median %.2e max %.2e" % (cid, st["frames"], st["points"], st["ratio_point"], st["ratio_point_at"], st["ratio_frame"],
                                           st["ratio_frame_at"], st["ratio_frame_median"], st["share_1e3"], st["share_1e2"],
                                           st["bound_median"], st["bound_max"]))
        assert not bad, (cid, bad[:6])
        assert st["share_1e3"] <= CAP_1E3 and st["share_1e2"] <= CAP_1E2, (cid, st["share_1e3"], st["share_1e2"])
        assert np.all(np.isfinite(c["B"])) and c["B"].min() > 0
        if st["ratio_frame"] > worst:
            worst, where = st["ratio_frame"], cid
        # float64 rounded to float32 is inside (a) by the store's term alone
        bad, _ = spgm_env_check(c["ref"].astype(np.float32), c["ref"], c["B"])
        assert not bad
    print("kappa: largest per-frame ratio of the float32 restatement %.5f (%s); 4 x = %.5f; KAPPA = %g" % (worst, where, 4 * worst, KAPPA))
    assert KAPPA <= 1.0
    assert KAPPA >= 4.0 * worst, (KAPPA, worst, where)
    assert abs(KAPPA_MEASURED - worst) <= 0.05 * worst, (KAPPA_MEASURED, worst)     # the constant is written beside its measured value
    assert KAPPA <= 4.0 * 1.06 * KAPPA_MEASURED                                       # ... and is not left loose: 4 x, rounded up


def test_reference_is_well_conditioned_under_one_ulp_of_input():
    """every input sample moved UP by one float32 ulp: the float64 reference stays inside B.  The kernel reads the very
    samples the reference reads, so B owes this nothing; it shows that the reference is not balanced on its input's last
    bit.  Moving every sample the same way is the coherent worst case: it adds 2 EPS |x_j| to each, a rectified copy of
    the signal whose DC bin, 2 EPS sum w |x|, can reach sqrt(ws) 2 EPS = 3e-6 ... 7e-6 of the RMS spectrum, the size of
    EPS_X itself; so the statement is a ratio below 1 (measured: 0.15 ... 0.33), not a small one."""
    for cid in ("wf_9_0", "wf_11_1", "lds_4096"):
        c = _case(cid)
        xs2 = [np.nextafter(x, np.float32(np.inf)) for x in c["xs"]]
        moved = spgm_env_ref(xs2, c["f0s"], c["fs"], c["thop"])
        ratio = np.abs(moved - c["ref"]) / c["B"]
        print("one ulp of input %-10s moves the reference by at most %.3f B" % (cid, ratio.max()))
        assert ratio.max() <= 1.0, (cid, ratio.max())


# ---------------------------------------------------------------- the inputs hold what the GPU test says
@pytest.mark.parametrize("cid", list(CONFIGS))
def test_inputs_hold_every_branch(cid):
    fs, thop, _ = config_options(cid)
    xs, f0s = spgm_env_inputs(cid)
    nwin, N, npsd = sizes(fs, thop)
    assert len(xs) == len(NAMES) == len(NFRM) and [len(f) for f in f0s] == list(NFRM)
    assert all(1 <= n <= 49 for n in NFRM) and sum(NFRM) < 600 and {n % 2 for n in NFRM} == {0, 1}
    f0 = np.concatenate(f0s)
    frm_off = offsets(f0s)
    utt, idx = frame_index(frm_off)
    ws, c = plan_values(f0, idx, fs, thop)
    nx = np.array([len(x) for x in xs])[utt]
    last = idx == np.array(NFRM)[utt] - 1
    # a pair with a missing second frame
    assert NFRM[I_SINGLE] == 1 and any(n % 2 == 1 and n > 1 for n in NFRM)
    # an F0 that changes every frame within its pairs: the seed cache misses for frame b
    sp = f0s[I_SPEECH]
    assert sp[0] > 0 and np.count_nonzero((sp[0::2][:len(sp) // 2] > 0) & (sp[1::2] > 0) & (sp[0::2][:len(sp) // 2] != sp[1::2])) >= 10
    # a flat stretch: the cache hits for frame b (same F0 bits and window length as frame a)
    assert np.all(f0s[I_FLAT] == np.float32(FLAT_F0)) and len(set(ws[utt == I_FLAT])) == 1
    # 200.0 Hz voiced beside unvoiced, both orders within a pair: the same f0n bits, different window lengths
    v = f0s[I_V200]
    pairs = {(float(v[i]), float(v[i + 1])) for i in range(0, len(v) - 1, 2)}
    assert {(200.0, 0.0), (0.0, 200.0), (200.0, 200.0), (0.0, 0.0)} <= pairs
    w200 = int(plan_values(np.float32([200.0]), [0], fs, thop)[0][0])
    assert w200 != nwin                                 # (an unvoiced frame's f0n is 200 / fs: the same bits by construction)
    assert set(ws[utt == I_V200]) == {w200, nwin}
    # a window longer than the transform (time-aliased), alone in its pair and beside a short one
    assert np.all(ws[utt == I_LOW] > N) and f0s[I_LOW][0] < 3.0 * fs / N
    wl = ws[utt == I_LOWMIX]
    assert wl[0] > N >= wl[1] and wl[3] > N and wl[4] > N
    # windows hanging over both ends of their utterances
    assert np.any((idx == 0) & (c - ws // 2 < 0) & (f0 > 0)) and np.any((idx == 0) & (f0 == 0) & (c - ws // 2 < 0))
    assert np.any(last & (c - ws // 2 + ws > nx) & (f0 > 0)) and np.any(last & (c - ws // 2 + ws > nx) & (f0 == 0))
    # an utterance shorter than one window between neighbours of ten times its level
    assert len(xs[I_SHORT]) == 100 and np.all(ws[utt == I_SHORT] > 100)
    assert LEVEL[I_SHORT - 1] == 10.0 * LEVEL[I_SHORT] and LEVEL[I_SHORT + 1] == 10.0 * LEVEL[I_SHORT]
    assert np.abs(xs[I_SHORT]).max() > 0
    # an all-zero utterance, voiced and unvoiced frames
    assert not xs[I_ZERO].any() and np.any(f0s[I_ZERO] > 0) and np.any(f0s[I_ZERO] == 0)
    # ws == 1 does not occur (F0 would have to reach 3 fs / 2), ws <= 1 is the kernels' guard only
    assert ws.min() > 1
    # the arrangement test's utterances: `same` ends, alone in its pair, on the F0 bits and window length the target starts on
    (xt, ft), (xa, fa), (xb, fb) = cache_pair(cid)
    assert len(fa) % 2 == 1 and fa[-1] == ft[0] and fb[-1] != ft[0] and np.array_equal(xa, xb)
    assert plan_values(fa[-1:], [0], fs, thop)[0][0] == plan_values(ft[:1], [0], fs, thop)[0][0]


def test_zero_input_gives_twice_the_log_floor():
    """what the GPU test holds the all-zero utterance to, from the float64 reference"""
    c = _case("wf_11_1")
    z = slice(int(offsets(c["f0s"])[I_ZERO]), int(offsets(c["f0s"])[I_ZERO + 1]))
    assert np.abs(c["ref"][z] - 2.0 * math.log(1e-10)).max() <= 1e-12


# ---------------------------------------------------------------- the checker notices
@pytest.mark.parametrize("fault", FAULTS)
def test_checker_flags_subtle_errors(fault):
    """every fault of spgm_env_reference.FAULTS in the float32 restatement, on every configuration"""
    for cid in CONFIGS:
        c = _case(cid)
        wrong = spgm_env_ref(c["xs"], c["f0s"], c["fs"], c["thop"], np.float32, fault=fault)
        bad, st = spgm_env_check(wrong, c["ref"], c["B"])
        assert bad, (fault, cid, st["ratio_point"], st["ratio_frame"])


def test_checker_catches_what_the_worst_case_form_lets_through():
    """an error of 1e-4 nepers over every bin of one frame is inside (a) almost everywhere and outside (b); a planted NaN
    and a frame left at the loud signal's values are reported"""
    c = _case("wf_11_1")
    g = int(offsets(c["f0s"])[I_SPEECH]) + 10
    r = c["r32"].copy()
    r[g] += np.float32(1e-4)
    bad, _ = spgm_env_check(r, c["ref"], c["B"])
    assert ("frame", g) in {b[:2] for b in bad} and {b[1] for b in bad} == {g}
    r = c["r32"].copy()
    r[g, 7] = np.nan
    bad, _ = spgm_env_check(r, c["ref"], c["B"])
    assert [b[:3] for b in bad if b[0] == "nonfinite"] == [("nonfinite", g, 7)]
    stale = spgm_env_ref(R.loud_inputs(c["xs"]), c["f0s"], c["fs"], c["thop"], np.float32)
    r = c["r32"].copy()
    r[g] = stale[g]
    bad, _ = spgm_env_check(r, c["ref"], c["B"])
    assert {b[0] for b in bad} == {"point", "frame"} and {b[1] for b in bad} == {g}
