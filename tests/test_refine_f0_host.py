"""CPU: the numpy restatement of tests/refine_f0_reference.py IS the float64 oracle's F0 refinement, its float32 form is a
yardstick that keeps every bound under the documented 0.1 % on the very inputs the GPU test uses, no input lets the gate
be decided by rounding, and the checker built on them notices the errors the existing 2e-2 Hz tolerance lets through.

tests/test_gpu_refine_f0.py judges k_refine_f0 with refine_ref / refine_check; this module is what entitles it to."""
import numpy as np
import pytest

from harm_env_reference import plan_values
from refine_f0_reference import (ADD_REL, CAP_REL, CONFIGS, EPS, FAULTS, GATE, GATE_CASES, GATE_CONFIG, GATE_FACTOR, I_COND, I_HIGH,
                                 I_LOW, I_SHORT, I_ZERO, LEVEL, MARGIN, NAMES, NHAR_TRUE, NHAR_UP, DOWN_CONFIGS, STATE_FS, STATE_STEP,
                                 STATE_UP, config_rate, downstream_inputs, frame_bounds, gate_margins, inside, offsets,
                                 refine_check, refine_f32, refine_inputs, refine_ref, state_inputs)

ALL = list(CONFIGS) + [GATE_CONFIG]
_CASES = {}


def case(cid):
    if cid not in _CASES:
        fs, thop = config_rate(cid)
        xs, f0s, names = refine_inputs(cid)
        _CASES[cid] = dict(cid=cid, fs=fs, thop=thop, xs=xs, f0s=f0s, names=names,
                           r64=[refine_ref(x, fs, f, thop) for x, f in zip(xs, f0s)],
                           r32=[refine_f32(x, fs, f, thop) for x, f in zip(xs, f0s)])
    return _CASES[cid]


def flat(rows):
    return np.concatenate([np.asarray(r, np.float32) for r in rows])


def faulty_row(c, fault):
    """the float32 restatement with one fault, every utterance of the batch"""
    cat = np.concatenate(c["xs"])
    off = offsets(c["xs"])
    return flat([refine_f32(x, c["fs"], f, c["thop"], fault=fault, left=cat[:off[u]], right=cat[off[u + 1]:])["f"]
                 for u, (x, f) in enumerate(zip(c["xs"], c["f0s"]))])


# ---------------------------------------------------------------- the float64 restatement is the oracle
@pytest.mark.parametrize("cid", ALL)
def test_float64_restatement_is_the_oracle(o64, cid):
    """every utterance of every input: the refined track within 1e-10 relative of o_refine_f0 (both float64; the order of
    summation differs), unvoiced and rejected frames equal to the input"""
    c = case(cid)
    for u, (x, f0) in enumerate(zip(c["xs"], c["f0s"])):
        ref = o64.refine_f0(x, c["fs"], f0, c["thop"])
        mine = c["r64"][u]["f"]
        v = f0 > 0
        assert np.array_equal(ref[~v], np.zeros(int((~v).sum()))) and np.array_equal(mine[~v], ref[~v])
        assert np.max(np.abs(mine - ref)[v] / f0[v], initial=0.0) <= 1e-10, (cid, c["names"][u])
        held = v & (c["r64"][u]["nf"] == 0)
        assert np.array_equal(ref[held], f0[held].astype(np.float64)) and np.array_equal(mine[held], ref[held])


@pytest.mark.parametrize("name, j", [("only_1", 1), ("only_2", 2), ("only_3", 3)])
def test_each_harmonic_estimate_is_the_oracles(o64, name, j):
    """two partials displaced: the oracle's refined value is ONE estimate, f_j fs -- the restatement's per-harmonic
    estimates, one j at a time"""
    c = case(GATE_CONFIG)
    u = c["names"].index(name)
    x, f0, r = c["xs"][u], c["f0s"][u], c["r64"][u]
    ins = inside(f0, len(x), c["fs"], c["thop"])
    assert ins.sum() >= 15
    want = np.isin(np.arange(1, 4), [j])
    assert np.all(r["acc"][ins] == want)
    ref = o64.refine_f0(x, c["fs"], f0, c["thop"])
    assert np.max(np.abs(r["est"][ins, j - 1] * c["fs"] - ref[ins]) / f0[ins]) <= 1e-10
    assert np.max(np.abs(ref[ins] - 200.0)) < 2.0 and abs(float(f0[0]) - 200.0) > 2.9   # pulled onto the partial


def test_gate_cases_are_what_they_say():
    """in every frame whose window lies inside the signal the gate accepts exactly the j the case names; the rejected
    cases hold the uploaded bits there"""
    c = case(GATE_CONFIG)
    seen = set()
    for u, name in enumerate(c["names"]):
        mult, up, accepted = GATE_CASES[name]
        f0, r = c["f0s"][u], c["r64"][u]
        ins = inside(f0, len(c["xs"][u]), c["fs"], c["thop"])
        assert ins.sum() >= 15, name
        assert np.all(r["acc"][ins] == np.isin(np.arange(1, 4), accepted)), name
        seen.add(len(accepted))
        if not accepted:
            assert np.array_equal(r["f"][ins].astype(np.float32).view(np.int32), f0[ins].view(np.int32))
    assert seen == {0, 1, 2, 3}
    # what a gate at 9 % / 11 % would change: estimates on either side of 10 %, within one per cent of F0 of it
    d = {n: c["r64"][c["names"].index(n)]["dist"] / (c["f0s"][c["names"].index(n)][:, None] / c["fs"]) for n in ("acc_dn95", "rej_105")}
    assert np.all(np.any((d["acc_dn95"][3:-3] > 0.09) & (d["acc_dn95"][3:-3] < GATE), axis=1))       # some j, every frame
    assert np.all(np.any((d["rej_105"][3:-3] > GATE) & (d["rej_105"][3:-3] < 0.11), axis=1))


def test_inputs_are_what_the_gpu_test_says():
    for cid in CONFIGS:
        c = case(cid)
        fs, thop = c["fs"], c["thop"]
        assert c["names"] == NAMES and len(c["xs"]) <= 8
        assert {int(o) % 4 for o in offsets(c["xs"])[:-1]} == {0, 1, 2, 3}, cid
        assert all(len(x) <= 0.35 * fs + 4 for x in c["xs"]) and all(3 <= len(f) <= 70 for f in c["f0s"])
        for u in range(len(NAMES)):
            assert len(c["f0s"][u]) <= max(int(len(c["xs"][u]) / fs / thop), 3) + 9 * (u == I_ZERO)
        f_low = c["f0s"][I_LOW]
        assert np.all(f_low > 0) and not inside(f_low, len(c["xs"][I_LOW]), fs, thop).any()         # every frame clipped
        nh_low = int(round(4.0 * fs / float(f_low.max())))
        assert len(c["xs"][I_LOW]) < nh_low < 2 * len(c["xs"][I_LOW]) + 2 * nh_low                  # shorter than its window
        f_c = c["f0s"][I_COND]
        assert inside(f_c, len(c["xs"][I_COND]), fs, thop)[f_c > 0].all()                            # voiced where nothing is clipped
        assert (f_c > 0).sum() >= 15 and f_c[0] == 0 and f_c[-1] == 0
        assert len(c["xs"][I_SHORT]) == 100 and np.all(c["f0s"][I_SHORT] > 0) and len(c["f0s"][I_SHORT]) == 3
        rms = [float(np.sqrt(np.mean(np.square(x, dtype=np.float64)))) for x in c["xs"]]
        for u in (I_LOW, I_SHORT):                                                                  # loud neighbours
            assert LEVEL[u - 1] == LEVEL[u + 1] == 10.0 * LEVEL[u] and min(rms[u - 1], rms[u + 1]) > 4.0 * rms[u], (cid, u, rms)
        f_hi = c["f0s"][I_HIGH]
        assert f_hi.min() >= 980.0 and f_hi.max() <= 3050.0 and 3 * f_hi.max() < fs / 2 * 1.02
        assert round(4.0 * fs / float(f_hi.max())) < 64 or fs > 50000.0                             # fewer samples than lanes
        assert not c["xs"][I_ZERO].any() and np.all(c["f0s"][I_ZERO] > 0)
        assert np.all(c["r64"][I_ZERO]["nf"] == 0) and not c["r64"][I_ZERO]["est"].any()            # atan2(0, 0) = 0: rejected
        for u in (0, len(NAMES) - 1):
            assert (c["f0s"][u] == 0).any() and (c["f0s"][u] > 0).sum() >= 3
    assert {CONFIGS[k][:2] for k in CONFIGS} >= {(8000.0, 0.005), (44100.0, 0.005), (44100.0, 128.0 / 44100.0), (96000.0, 0.010)}
    assert any(CONFIGS[k][0] == 16000.0 for k in CONFIGS)
    c = case(GATE_CONFIG)
    assert len(c["xs"]) == 8 and {int(o) % 4 for o in offsets(c["xs"])[:-1]} == {0, 1, 2, 3}


# ---------------------------------------------------------------- the two conditions, every input, every frame
@pytest.mark.parametrize("cid", ALL)
def test_conditions_hold_on_every_input(cid):
    """cap: no frame's bound 4 Y_u + A over 1e-3 F0; gate margin: every float64 gate distance at least 10 bounds from the
    gate.  Printed per utterance (the table of LAB.md)."""
    c = case(cid)
    gm = gate_margins(c["xs"], c["f0s"], c["fs"], c["thop"])
    for u, (f0, r64, r32) in enumerate(zip(c["f0s"], c["r64"], c["r32"])):
        Y, bound = frame_bounds(r64, r32, f0)
        v = f0 > 0
        y_rel = float(np.max(np.abs(r32["f"] - r64["f"])[v] / f0[v]))
        b_rel = float(np.max(bound[v] / f0[v]))
        print("yardstick %-10s %-9s voiced %2d  nf %s  Y %.3g Hz  Y/F0 %.2e  bound/F0 %.2e  gate margin %.0f bounds (frame %d, j %d)" % (
            cid, c["names"][u], int(v.sum()), np.bincount(r64["nf"][v], minlength=4).tolist(), Y, y_rel, b_rel, gm[u][0], gm[u][1], gm[u][2]))
        assert np.allclose(bound, MARGIN * Y + ADD_REL * np.abs(r64["f"]), rtol=1e-15, atol=0)
        assert b_rel <= CAP_REL, (cid, c["names"][u], b_rel)
        assert gm[u][0] >= GATE_FACTOR, (cid, c["names"][u], gm[u])
        assert np.array_equal(r64["acc"], r32["acc"])                 # (what the margin is there for)


def test_conditions_hold_on_the_inputs_of_stages_b_and_c():
    """the same two conditions for the utterances whose refined row feeds the downstream comparison; stage C's second
    refinement starts from the device's once-refined row, stood in for here by the float32 yardstick's"""
    x1, x2, f0 = state_inputs()
    row1 = refine_f32(x1, STATE_FS, f0, 0.005)["f"]
    sets = [("down_" + cid, DOWN_CONFIGS[cid][0], DOWN_CONFIGS[cid][1]) + downstream_inputs(cid) for cid in sorted(DOWN_CONFIGS)]
    sets += [("state_first", STATE_FS, 0.005, [x1], [f0]), ("state_second", STATE_FS, 0.005, [x2], [row1])]
    for tag, fs, thop, xs, f0s in sets:
        gm = gate_margins(xs, f0s, fs, thop)
        bad, st = refine_check(flat([refine_f32(x, fs, f, thop)["f"] for x, f in zip(xs, f0s)]), xs, f0s, fs, thop)
        for rec, g in zip(st["utterances"], gm):
            print("yardstick %-12s utt %d  Y/F0 %.2e  bound/F0 %.2e  gate margin %.0f bounds" % (tag, rec["utt"], rec["Y_rel"], rec["bound_rel"], g[0]))
            assert rec["bound_rel"] <= CAP_REL and g[0] >= GATE_FACTOR, (tag, rec, g)
        assert not bad, (tag, bad)


@pytest.mark.parametrize("cid", ALL)
def test_checker_passes_the_yardstick_and_rounded_float64(cid):
    c = case(cid)
    args = (c["xs"], c["f0s"], c["fs"], c["thop"])
    bad, st = refine_check(flat([r["f"] for r in c["r32"]]), *args)
    assert not bad, bad
    assert st["ratio"] <= 1.0 / MARGIN + 1e-12, st["ratio"]
    bad, st = refine_check(flat([r["f"] for r in c["r64"]]), *args)
    assert not bad, bad
    assert st["err_rel"] <= EPS and st["ratio"] <= EPS / ADD_REL + 1e-12       # (one store: a sixteenth of the additive term)
    assert st["frames"] == sum(len(f) for f in c["f0s"])


# ---------------------------------------------------------------- the checker notices
# where each fault changes a judged value (stated from the inputs, not measured):
#   late        wherever F0 moves by more than the bound within one sample (the ramp of `high`: 2e4 Hz / s) or a window is
#               clipped (the sample entering at the edge is not a small change): every configuration
#   nh_points, periodic   the window's shape: every voiced frame, most where nh is small (`high`)
#   clamp, neighbour      the clipped frames of `low` and `short` (their neighbours are ten times as loud)
#   gate9, gate11, div3   the gate cases
#   jplus1      every accepted estimate
#   rewrite     the rejected frames (`zero`, rej_13, rej_105) whose value does not survive fl(fl(F0 / fs) fs)
def _faults_on(fault):
    if fault in ("gate9", "gate11", "div3"):
        return [GATE_CONFIG]
    return ALL if fault in ("jplus1", "rewrite") else list(CONFIGS)


@pytest.mark.parametrize("fault", FAULTS)
def test_checker_flags_subtle_errors(fault):
    flagged = {}
    for cid in _faults_on(fault):
        c = case(cid)
        bad, st = refine_check(faulty_row(c, fault), c["xs"], c["f0s"], c["fs"], c["thop"])
        flagged[cid] = sorted({(c["names"][b[0]], b[1]) for b in bad})
        print("fault %-9s %-10s ratio %.3g  %s" % (fault, cid, st["ratio"], flagged[cid]))
    if fault == "rewrite":
        hit = [k for k, v in flagged.items() if v]
        assert hit and all(kind == "bits" for k in hit for _, kind in flagged[k]), flagged
        return
    assert all(flagged.values()), (fault, flagged)
    names = {n for v in flagged.values() for n, _ in v}
    if fault in ("clamp", "neighbour"):
        for cid in CONFIGS:
            assert {"low", "short"} & {n for n, _ in flagged[cid]}, (fault, cid, flagged[cid])
    if fault == "gate9":
        assert ("acc_dn95", "err") in flagged[GATE_CONFIG]
    if fault == "gate11":
        assert ("rej_105", "bits") in flagged[GATE_CONFIG]
    if fault == "div3":
        assert {"only_1", "only_2", "only_3", "only_23"} <= names


def test_checker_reports_nonfinite_bits_and_cap():
    import refine_f0_reference as R
    c = case("8k_5ms")
    args = (c["xs"], c["f0s"], c["fs"], c["thop"])
    row = flat([r["f"] for r in c["r32"]])
    off = offsets(c["f0s"])
    g = int(off[0]) + int(np.flatnonzero(c["f0s"][0] > 0)[3])
    gu = int(off[0]) + int(np.flatnonzero(c["f0s"][0] == 0)[0])
    gz = int(off[I_ZERO]) + 4
    wrong = row.copy()
    wrong[g] = np.nan; wrong[gu] = np.float32(-0.0); wrong[gz] = np.nextafter(row[gz], np.float32(1e9))
    bad, _ = refine_check(wrong, *args)
    assert sorted(b[:3] for b in bad) == sorted([(0, "nonfinite", g - int(off[0])), (0, "bits", gu - int(off[0])), (I_ZERO, "bits", 4)]), bad
    old = R.CAP_REL
    try:
        R.CAP_REL = 2.0 * ADD_REL
        bad, _ = refine_check(row, *args)
    finally:
        R.CAP_REL = old
    assert {b[1] for b in bad} == {"cap"} and len(bad) >= 3


# ---------------------------------------------------------------- the inputs of stages B and C
def test_nhar_crossing_pair_and_state_inputs():
    """8 kHz: the uploaded 202 Hz has 19 harmonics, the float64-refined value 20 (lp::nhar as tests/harm_env_reference.py
    restates it); stage C: the analysis window crosses 2048 samples between 0.9 x the uploaded F0 and the signal's pitch"""
    fs, thop, kw = DOWN_CONFIGS["8k_2ch"]
    xs, f0s = downstream_inputs("8k_2ch")
    x, f0 = xs[1], f0s[1]
    r = refine_ref(x, fs, f0, thop)
    ins = inside(f0, len(x), fs, thop)
    assert ins.sum() >= 10 and np.all(r["nf"][ins] == 3)
    K_up = plan_values(f0, np.arange(len(f0)), thop, fs, 4.0, kw["maxnhar"])[2]
    K_ref = plan_values(r["f"].astype(np.float32), np.arange(len(f0)), thop, fs, 4.0, kw["maxnhar"])[2]
    assert np.all(K_up == 19) and np.all(K_ref[ins] == 20), (K_up, K_ref)
    assert np.all(np.abs(r["f"][ins] - NHAR_TRUE) < 0.5) and float(f0[0]) == NHAR_UP
    # stage C
    x1, x2, f0 = state_inputs()
    r1 = refine_ref(x1, STATE_FS, f0, 0.005)
    r2 = refine_ref(x2, STATE_FS, r1["f"].astype(np.float32), 0.005)
    ins = inside(r1["f"].astype(np.float32), len(x1), STATE_FS, 0.005)
    assert np.all(r1["nf"][ins] == 3) and np.all(r2["nf"][ins] == 3)
    assert np.all(np.abs(r1["f"][ins] / (STATE_UP * STATE_STEP) - 1) < 5e-3) and np.all(np.abs(r2["f"][ins] / (STATE_UP * STATE_STEP ** 2) - 1) < 5e-3)
    hw = lambda f: int(plan_values(np.float32([f]), [0], 0.005, STATE_FS, 4.0, 1)[1][0])        # noqa: E731
    assert hw(0.9 * STATE_UP) <= 2048 < hw(float(r2["f"][ins].max())) <= 4096
    assert float(r2["f"][ins].min()) < 0.9 * STATE_UP                                          # under the margin of the upload
