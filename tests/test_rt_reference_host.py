"""CPU: what entitles tests/test_gpu_rt_samples.py to its bounds.  For every case of rt_reference.CASES the restated hop
schedule equals the oracle's, the error scale S covers the float64 stream (and only it), the case's noise part is well
conditioned (a one-ulp move of its rows moves the float64 oracle by at most a quarter of the noise bound), and every fault
of rt_reference.FAULTS, applied to the float64 stream, is flagged by rt_metrics under the GPU module's bounds -- while the
first two pass the whole-stream 1e-5 gate of tests/test_gpu_rt.py (LAB.md, "llsmrt sample by sample")."""
import numpy as np
import pytest

import rt_reference as R


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_schedule_scale_and_form(o64, name):
    fs, pr, _seed = R.rt_case(name)
    yp, yap, lat = R.oracle_streams(o64, name)
    sched = R.rt_schedule(pr.nfrm, pr.thop, fs)
    assert sched["latency"] == lat and sched["n"] == len(yp) == len(yap), (sched["latency"], lat, sched["n"], len(yp))
    assert len(sched["curr_nhop"]) <= 60 and np.array_equal(sched["next_nhop"][:-1], sched["curr_nhop"][1:])
    S = R.rt_sin_scale(pr, sched)
    m = R.rt_metrics(pr, sched, yp, yp, yap, yap, S)
    assert m["ysin_nonzero_uncovered"] == 0 and m["ysin_local"] == 0.0 and m["ynoise_local"] == 0.0, m
    assert np.all(np.abs(yp) <= S * (1 + 1e-12)) and np.all(S[yp != 0] > 0)
    assert np.count_nonzero(yp) > 0.5 * len(yp) and m["ysin_uncovered_samples"] > sched["h0"]      # both kinds of sample exist
    # the case reaches what it is there for
    c = R.CASES[name]
    assert R.rt_expected_form(c, sched) == {c["form"]}, (name, R.rt_expected_form(c, sched))
    hops = set(sched["curr_nhop"].tolist())
    expect = dict(bench=({220, 221}, 1024), k400=({200, 201}, 512), clamp=(set(range(86, 91)), 256), wide=({528}, 2048),
                  two_launch=({960}, 4096), syn16k=({80}, 256), syn12k=({60}, 256), mono=({76, 77, 78}, 256),
                  gates=({220, 221}, 1024))[name]
    assert hops <= expect[0] and sched["nfft"] == expect[1], (hops, sched["nfft"])
    if name in ("bench", "k400", "clamp", "mono"):
        assert len(hops) >= 2, hops                                              # a fractional hop: rows change length
    if name == "k400":
        assert pr.nhar.max() == 400 > 256 and sched["nfft"] >= 400
    if name == "clamp":
        assert pr.nhar.max() == 400 > sched["nfft"]
    if name == "wide":
        assert 2 * 528 > 1024 and pr.npsd > 1024 and pr.nhar.max() == 300
    if name in ("syn16k", "syn12k"):
        # band 4 starts at (16 kHz) or above (12 kHz: band 3 straddles it) the synthesis Nyquist: three active bands
        assert pr.fnyq == 22050.0 and pr.chanfreq[1] < fs / 2 and (pr.chanfreq[2] == fs / 2 if name == "syn16k" else pr.chanfreq[2] > fs / 2)
        assert np.all(pr.nhar * pr.f0 < fs / 2)
    if name == "gates":
        assert pr.f0[0] > 0 and all(pr.f0[i] > 0 and pr.nhar[i] == 0 for i in R.GATES_NHAR0)
        assert all(R.rt_level_peak(pr, i) < -104 for i in R.GATES_SILENT)
        assert abs(R.rt_level_peak(pr, R.GATES_BELOW) + 100.5) < 1e-3 and abs(R.rt_level_peak(pr, R.GATES_ABOVE) + 99.5) < 1e-3
    # every harmonic at least 1 / (3 K) of its frame's sum: a dropped one is 2^24 / (3 K) units of ysin_local
    for i in np.flatnonzero(pr.nhar > 0):
        a = pr.ampl[i, :pr.nhar[i]]
        assert a.min() >= a.sum() / (3.0 * pr.nhar[i])


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_noise_rows_are_well_conditioned(o64, name):
    """A condition on the INPUT: the float64 oracle's ynoise_local response to v (1 +- 2^-24) on the psd, psdres, edc and
    envelope rows is at most a quarter of the noise bound -- conditioning cannot excuse a noise error on these cases."""
    fs, pr, seed = R.rt_case(name)
    yp, yap, _ = R.oracle_streams(o64, name)
    sched = R.rt_schedule(pr.nfrm, pr.thop, fs)
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(2):
        q = R.rt_perturb_noise_rows(pr, rng)
        _yp2, yap2, _ = o64.rt_run(o64.soptions(fs), q, seed=seed)
        v, at = R.rt_noise_local(yap2, yap, sched)
        worst = max(worst, v)
    print("[rt one-ulp] %-10s ynoise_local response %.3g (condition %.3g)" % (name, worst, R.ULP_CONDITION))
    assert worst <= R.ULP_CONDITION, (name, worst)


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_every_fault_is_flagged(o64, o32, name):
    fs, pr, seed = R.rt_case(name)
    yp, yap, _ = R.oracle_streams(o64, name)
    sched, S, m32 = R.case_yardsticks(o64, o32, name)
    print("[rt f32 oracle] %-10s ysin_local %.1f at %d (ynoise_local %.3g: not a yardstick)" % (
        name, m32["ysin_local"], m32["ysin_local_at"], m32["ynoise_local"]))
    assert m32["ysin_nonzero_uncovered"] == 0
    # the yardstick may lift the bound above 60 where K or the window exceed what 60 was calibrated on, never near a fault
    assert m32["ysin_local"] < 1000.0, m32

    def rerun(q):
        a, b, _ = o64.rt_run(o64.soptions(fs), q, seed=seed)
        return np.asarray(a, np.float64), np.asarray(b, np.float64)

    ctx = dict(name=name, pr=pr, sched=sched, S=S, yp=np.array(yp), yap=np.array(yap), rerun=rerun)
    applied = 0
    for fname, fault in R.FAULTS.items():
        got = fault(ctx)
        if got is None:
            continue
        applied += 1
        m = R.rt_metrics(pr, sched, got[0], yp, got[1], yap, S)
        bad = R.rt_violations(m, m32["ysin_local"])
        old5 = m["p_rel_rms"] <= 1e-5 and m["ap_rel_rms"] <= 1e-5
        old4 = m["p_rel_rms"] <= 1e-4 and m["ap_rel_rms"] <= 1e-4
        print("[rt fault] %-10s %-32s p_rel_rms %.2e ap_rel_rms %.2e | old gate 1e-5 %s, 1e-4 %s | ysin_local %.3g uncovered %d "
              "ynoise_local %.3g -> %s" % (name, fname, m["p_rel_rms"], m["ap_rel_rms"], "PASSES" if old5 else "fails",
                                           "PASSES" if old4 else "fails", m["ysin_local"], m["ysin_nonzero_uncovered"],
                                           m["ynoise_local"], "flagged" if bad else "MISSED"))
        assert bad, (name, fname, m)
        if fname in R.FAULTS_OLD_GATE_PASSES:
            assert old5, (name, fname, m)                 # the gap: the whole-stream gate lets it through
    assert applied >= 6 + (name in ("k400", "clamp", "gates"))
