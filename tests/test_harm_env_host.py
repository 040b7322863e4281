"""CPU: the numpy restatement of tests/harm_env_reference.py IS the float64 oracle's envelope analysis of a band plane,
its float32 form is a tight yardstick on the very inputs the GPU test uses, its plan values are the product's, and the
checker built on them notices errors the whole-chain parity bounds let through.

tests/test_gpu_harm_env.py judges k_harm_env with harm_env_ref / harm_env_check; this module is what entitles it to."""
import ctypes as C

import numpy as np
import pytest

import libllsm2_amd as llsm
from conftest import make_speechlike
from harm_env_reference import (ADD_D, ADD_Z, CAP_D, CAP_Z, CONFIGS, EPS, FAULTS, HMPP, I_CLIPPED, I_HIGH, I_LOW, I_MID, I_SHORT,
                                I_SPEECH, I_ZERO, MARGIN, NAMES, REL_CONFIGS, band_edges, config_options, frame_index,
                                harm_env_check, harm_env_inputs, harm_env_ref, offsets, plan_values, _core)

# id: (fs, hop, seed of make_speechlike, band edges)
ORACLE_INPUTS = {"44k": (44100.0, 0.005, 41, [2000.0, 4000.0, 8000.0]), "16k": (16000.0, 0.005, 42, [1000.0, 3000.0]),
                 "8k": (8000.0, 0.010, 43, [1500.0])}
ME = 4


def _subband(o, src, c1, c2):
    src = o.arr(src); y = np.zeros(len(src), o.dtype)
    o.lib.o_subband_energy(o.p(src), C.c_int(len(src)), o.f(c1), o.f(c2), o.p(y))
    return y


def _oracle_plan(o, f0, thop, fs, rel, me):
    """(c0, n, K, ndc) per frame from the oracle's own index functions"""
    L = o.lib
    c0 = np.array([L.o_idx_center(i, thop, fs) for i in range(len(f0))], np.int64)
    n = np.array([L.o_idx_hwin(float(f), fs, rel) if f > 0 else 0 for f in f0], np.int64)
    K = np.array([L.o_idx_nhar(float(f), fs, me) if f > 0 else 0 for f in f0], np.int64)
    ndc = np.array([L.o_idx_dcwin(float(f), thop, fs) for f in f0], np.int64)
    return c0, n, K, ndc


# ---------------------------------------------------------------- the float64 restatement is the oracle
@pytest.mark.parametrize("rel", (4.0, 2.0, 1.5))
@pytest.mark.parametrize("iid", sorted(ORACLE_INPUTS))
def test_float64_restatement_is_the_oracle(o64, iid, rel):
    fs, thop, seed, cf = ORACLE_INPUTS[iid]
    x, f0 = make_speechlike(seed, nx=int(0.35 * fs), fs=fs, thop=thop)
    nch = len(cf) + 1
    edges = band_edges(dict(chanfreq=cf, nchannel=nch), fs)
    ce = np.stack([_subband(o64, x, fmin / fs, fmax / fs) for fmin, fmax in edges])
    nx_off, frm_off = [0, len(x)], [0, len(f0)]
    nh, a, p, d, A0, M, Ks = _core(ce, nx_off, frm_off, f0, thop, fs, rel, ME, np.float64, scales=True)
    c0, n, K, ndc = _oracle_plan(o64, f0, thop, fs, rel, ME)
    for mine, theirs in zip(plan_values(f0, np.arange(len(f0)), thop, fs, rel, ME), (c0, n, K, ndc)):
        assert np.array_equal(mine, theirs)
    assert np.any(Ks > 0) and np.any(f0 == 0)
    for c in range(nch):
        nho, ao, po = o64.harmonic_analysis(ce[c], fs, f0, thop, rel, ME, 1)
        assert np.array_equal(nho, nh)
        assert np.max(np.abs(ao - a[:, c]) / np.maximum(A0[:, c, None], 1e-300)) <= 1e-12
        sel = ao > 1e-6 * A0[:, c, None]
        assert sel.any()
        dp = np.abs(np.angle(np.exp(1j * (po - p[:, c]))))
        assert dp[sel].max() <= 1e-9, dp[sel].max()
        dco = np.zeros(len(f0))
        ci = np.ascontiguousarray(c0, np.int32); wi = np.ascontiguousarray(ndc, np.int32)
        o64.lib.o_compute_dc(o64.p(o64.arr(ce[c])), C.c_int(len(x)), o64.pi(ci), o64.pi(wi), C.c_int(len(f0)), o64.p(dco))
        assert np.all(dco > 0)
        assert np.max(np.abs(dco - d[:, c]) / dco) <= 1e-12


# ---------------------------------------------------------------- the GPU module's inputs, filtered by the oracle
_RES = {}


def _case(o64, cid):
    """the configuration's inputs with the oracle's band planes (float32, as the product stores them)"""
    fs, thop, opt = config_options(cid)
    xs, f0s = harm_env_inputs(cid)
    key = (fs, opt["rel_winsize"], opt["hm_method"])
    if key not in _RES:
        res = []
        for x, f0 in zip(xs, f0s):
            ao = o64.aoptions(thop=thop, f0_refine=0, rel_winsize=opt["rel_winsize"], hm_method=opt["hm_method"])
            pr, xr = o64.analyze(ao, x, fs, f0, want_res=True)
            for name in ("ampl", "phse", "psd", "psdres", "edc", "eenv_ampl", "eenv_phse"):       # the analysis is defined
                assert np.all(np.isfinite(getattr(pr, name))), (cid, name)
            res.append(xr)
        _RES[key] = res
    edges = band_edges(opt, fs)
    ce = np.zeros((len(edges), sum(len(x) for x in xs)), np.float32)
    nx_off = offsets(xs)
    for u, (x, xr) in enumerate(zip(xs, _RES[key])):
        for c, (fmin, fmax) in enumerate(edges):
            ce[c, nx_off[u]:nx_off[u + 1]] = _subband(o64, x if fmin > 6000.0 else xr, fmin / fs, fmax / fs)
    return dict(cid=cid, fs=fs, thop=thop, opt=opt, xs=xs, f0s=f0s, ce=ce, nx_off=nx_off, frm_off=offsets(f0s),
                f0=np.concatenate(f0s), me=opt["maxnhar_e"], rel=opt["rel_winsize"], judge=opt["hm_method"] != HMPP)


@pytest.fixture(scope="module")
def cases(o64):
    cache = {}

    def get(cid):
        if cid not in cache:
            cache[cid] = _case(o64, cid)
        return cache[cid]
    return get


def _args(c):
    return (c["ce"], c["nx_off"], c["frm_off"], c["f0"], c["thop"], c["fs"], c["rel"], c["me"])


def test_inputs_are_what_the_gpu_test_says():
    """ragged offsets at every residue mod 4, odd and even ndc both present, the paths the table of configurations names"""
    for cid in CONFIGS:
        fs, thop, opt = config_options(cid)
        xs, f0s = harm_env_inputs(cid)
        assert len(xs) == len(NAMES)
        assert {int(v) % 4 for v in offsets(xs)[:-1]} == {0, 1, 2, 3}, cid
        assert all(0 < len(f) <= 64 for f in f0s) and sum(len(f) for f in f0s) <= 280
        utt, idx = frame_index(offsets(f0s))
        f0 = np.concatenate(f0s)
        c0, n, K, ndc = plan_values(f0, idx, thop, fs, opt["rel_winsize"], opt["maxnhar_e"])
        v = f0 > 0
        assert {int(a) % 2 for a in ndc[v]} == {0, 1} and np.any(~v), cid
        assert len(xs[I_SHORT]) == 100 and len(f0s[I_SHORT]) == 3
        if opt["rel_winsize"] == 4.0:
            assert n[v & (utt == I_CLIPPED)].min() > len(xs[I_CLIPPED])                   # both ends clipped at once
        assert not xs[I_ZERO].any() and f0s[I_ZERO].all()
        assert n[v & (utt == I_HIGH)].max() <= 2 * 64 + 2                                 # a single trip of 64 pairs
        if fs == 44100.0 and opt["rel_winsize"] == 4.0:
            assert np.all(n[utt == I_LOW] == 5880) and (5880 // 2 + 255) // 256 == 12 and len(xs[I_LOW]) < 5880 // 2
            lo_mid = n[utt == I_MID]
            assert np.all(lo_mid == 2206) and len(xs[I_MID]) > 2 * 2206                  # five trips, inside the signal
        bdc = c0 - ndc // 2
        inside = v & (bdc >= c0 - n // 2) & (bdc + ndc <= c0 - n // 2 + n)
        if cid in REL_CONFIGS:
            assert np.any(v & ~inside), cid                              # the mean gets its own pass on voiced frames
        if cid == "44k_rel2":
            assert np.any(v & (ndc != n)) and np.any(v & (ndc == n))     # the knife edge, both sides
        if cid == "44k_rel1p5":
            assert not np.any(inside)
        if cid not in REL_CONFIGS:
            assert np.all(inside[v])
        if cid in ("44k_2ch_me8", "8k_2ch"):
            assert np.any(v & (K > 0) & (K < opt["maxnhar_e"])), cid     # the live cut cuts
    assert plan_values(np.float32([3000.0]), [0], 0.005, 44100.0, 4.0, 8)[1:3] == (58, 7)
    assert plan_values(np.float32([30.0]), [0], 0.005, 44100.0, 4.0, 4)[1] == 5880
    assert plan_values(np.float32([40.0]), [0], 0.005, 96000.0, 4.0, 4)[1] == 9600


@pytest.mark.parametrize("cid", list(CONFIGS))
def test_plan_values_are_the_products(o64, cid):
    """c0, n, K, ndc of every frame of the inputs: the restatement's and the oracle's equal llsm_gpu_plan_index cases
    0, 6, 7, 9"""
    L = llsm.load()
    fs, thop, opt = config_options(cid)
    xs, f0s = harm_env_inputs(cid)
    utt, idx = frame_index(offsets(f0s))
    f0 = np.concatenate(f0s)
    rel, me = opt["rel_winsize"], opt["maxnhar_e"]
    c0, n, K, ndc = plan_values(f0, idx, thop, fs, rel, me)
    theirs = [np.concatenate(v) for v in zip(*[_oracle_plan(o64, f, thop, fs, rel, me) for f in f0s])]
    for mine, their in zip((c0, n, K, ndc), theirs):
        assert np.array_equal(mine, their)
    for g in range(len(f0)):
        f = float(f0[g])
        assert L.llsm_gpu_plan_index(0, int(idx[g]), 0, 0.0, thop, fs, rel) == c0[g]
        assert L.llsm_gpu_plan_index(9, 0, 0, f, thop, fs, rel) == ndc[g]
        if f > 0:
            assert L.llsm_gpu_plan_index(6, 0, 0, f, thop, fs, rel) == n[g]
            assert L.llsm_gpu_plan_index(7, me, 0, f, thop, fs, rel) == K[g]


@pytest.mark.parametrize("cid", list(CONFIGS))
def test_float32_yardstick_is_small(cases, cid):
    """Y_Z and Y_D of every utterance of every configuration, printed (the table of DESIGN.md section 8), and the bounds
    they give under the caps; the checker passes the yardstick itself with every ratio <= 1/4, and float64 rounded to
    float32."""
    c = cases(cid)
    r32 = harm_env_ref(*_args(c), dtype=np.float32)
    assert r32[1].dtype == np.float32 and r32[3].dtype == np.float32
    bad, st = harm_env_check(r32, *_args(c), judge_env=c["judge"])
    for rec in st["utterances"]:
        print("yardstick %-12s %-9s frames %3d  Y_Z %5.1f EPS  Y_D %5.1f EPS  bound_z %.2e  bound_d %.2e" % (
            cid, NAMES[rec["utt"]], rec["frames"], rec["Y_Z"] / EPS, rec["Y_D"] / EPS, rec["bound_z"], rec["bound_d"]))
        assert rec["bound_z"] <= CAP_Z and rec["bound_d"] <= CAP_D, rec
        assert rec["bound_z"] == MARGIN * rec["Y_Z"] + ADD_Z and rec["bound_d"] == MARGIN * rec["Y_D"] + ADD_D
    assert not bad, bad
    assert st["ratio_z"] <= 0.25 + 1e-12 and st["ratio_d"] <= 0.25 + 1e-12, st
    r64 = harm_env_ref(*_args(c), dtype=np.float64)
    bad, st = harm_env_check((r64[0], r64[1].astype(np.float32), r64[2].astype(np.float32), r64[3].astype(np.float32)),
                             *_args(c), judge_env=c["judge"])
    assert not bad, bad
    assert st["err_z"] <= 2.1 * EPS and st["err_d"] <= EPS, st                 # (the derivation of the additive terms)


def _qualifies(fault, c):
    """the inputs on which a fault changes a judged value: stated, not measured"""
    utt, idx = frame_index(c["frm_off"])
    c0, n, K, ndc = plan_values(c["f0"], idx, c["thop"], c["fs"], c["rel"], c["me"])
    v = c["f0"] > 0
    env = c["judge"] and c["me"] > 0
    if fault in ("periodic", "halfsample", "seed"):
        return env                                                           # the envelope rows are judged at all
    if fault == "live":
        return env and bool(np.any(v & (K > 0) & (K < c["me"])))              # K < me somewhere
    if fault == "dcpair":
        return bool(np.any(v & (ndc % 2 == 1)))                              # an odd ndc on a voiced frame
    if fault in ("clip", "dcdiv"):
        return bool(np.any(c0 - ndc // 2 < 0))                                # a window clipped at sample 0
    return True                                                              # centre, dcwin: every input with voiced frames


@pytest.mark.parametrize("fault", FAULTS)
def test_checker_flags_subtle_errors(cases, fault):
    """every fault of harm_env_reference.FAULTS in the float32 restatement, on every configuration where it changes a
    judged value"""
    hit = 0
    for cid in CONFIGS:
        c = cases(cid)
        if not _qualifies(fault, c):
            continue
        hit += 1
        wrong = harm_env_ref(*_args(c), dtype=np.float32, fault=fault)
        bad, st = harm_env_check(wrong, *_args(c), judge_env=c["judge"])
        assert bad, (fault, cid, st["ratio_z"], st["ratio_d"])
        rows = {b[1] for b in bad}
        if fault in ("periodic", "halfsample", "seed"):
            assert rows == {"eZ"}, (fault, cid, bad)
        if fault in ("dcdiv", "dcwin", "dcpair"):
            assert rows == {"eD"}, (fault, cid, bad)
    assert hit >= (2 if fault == "live" else 1), fault
    if fault == "live":
        assert _qualifies(fault, cases("44k_2ch_me8")) and _qualifies(fault, cases("8k_2ch"))


def test_checker_reports_a_planted_nan_and_wrong_rows(cases):
    c = cases("44k_default")
    r = [a.copy() for a in harm_env_ref(*_args(c), dtype=np.float32)]
    g = int(c["frm_off"][I_SPEECH]) + 20
    assert c["f0"][g] > 0
    r[1][g, 2, 1] = np.nan
    bad, _ = harm_env_check(r, *_args(c))
    assert [b[:5] for b in bad] == [(I_SPEECH, "ampl", g, 2, 1)], bad
    r = [a.copy() for a in harm_env_ref(*_args(c), dtype=np.float32)]
    r[3][g, 1] = np.inf
    r[0][g + 1] += 1
    gu = int(np.flatnonzero(c["f0"] == 0)[0])
    r[2][gu, 0, 3] = -0.0                                                        # (an unvoiced row: +0.0 bits)
    gz = int(c["frm_off"][I_ZERO])
    r[1][gz, 0, 0] = 1e-30                                                       # (a voiced frame of zeros: exactly 0)
    bad, _ = harm_env_check(r, *_args(c))
    assert sorted(b[:5] for b in bad) == sorted([(I_SPEECH, "edc", g, 1, -1), (I_SPEECH, "nhar_e", g + 1, -1, -1),
                                                 (int(frame_index(c["frm_off"])[0][gu]), "zero_phse", gu, 0, 3),
                                                 (I_ZERO, "zero_ampl", gz, 0, 0)]), bad


def test_cap_is_a_condition(cases):
    """a yardstick that lifts a bound over its cap is a failure of the input"""
    import harm_env_reference as H
    c = cases("8k_2ch")
    r32 = harm_env_ref(*_args(c), dtype=np.float32)
    old = H.CAP_Z, H.CAP_D
    try:
        H.CAP_Z, H.CAP_D = ADD_Z, ADD_D
        bad, _ = harm_env_check(r32, *_args(c))
    finally:
        H.CAP_Z, H.CAP_D = old
    assert {"cap_z", "cap_d"} <= {b[1] for b in bad}
