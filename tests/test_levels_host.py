"""CPU checks of the level-resolved metrics of tests/gpu_common.py: harmonics and samples land in the right bands and
segments, and an error confined to one hop or to one weak harmonic -- small enough that the whole-utterance bounds
(SYN_TOL, the complex 1e-5 of CONTRACT) pass it -- is flagged by the new ceilings."""
import numpy as np
import pytest

import libllsm2_amd as llsm
from gpu_common import (CONTRACT, HARM_CEILING, SYN_CEILING, analysis_metrics, ceiling_violations, noise_local, rel_rms,
                        sin_error_scale, sin_geometry, synthesis_metrics, synthesis_violations)
from oracle.oracle import Params
from test_gpu_parity import SYN_TOL


def _params(nfrm=6, maxnhar=12, thop=0.005, fs=44100.0):
    p = Params(nfrm, maxnhar, 0, 16, 1, thop, fs / 2, [], np.float64)
    p.f0[:] = 150.0
    p.nhar[:] = maxnhar
    return p


def _rows(q):
    return {llsm.A_NHAR: q.nhar, llsm.A_NHAR_E: q.nhar_e, llsm.A_AMPL: q.ampl, llsm.A_PHSE: q.phse,
            llsm.A_PSD: q.psd, llsm.A_PSDRES: q.psdres, llsm.A_EDC: q.edc,
            llsm.A_EENV_AMPL: q.eenv_ampl, llsm.A_EENV_PHSE: q.eenv_phse}


def _metrics(p, q):
    return analysis_metrics(_rows(q), slice(0, p.nfrm), p, np.zeros(10), np.zeros(10))


def _levels(p):
    """amplitude of harmonic k (0-based) of every frame: 0 dB, -10 dB, ... -110 dB re 0.5"""
    p.ampl[:] = 0.5 * 10.0 ** (-10.0 * np.arange(p.maxnhar) / 20.0)
    p.phse[:] = np.random.default_rng(1).uniform(-np.pi, np.pi, p.ampl.shape)
    return p


def test_harmonic_bands_are_assigned_by_level():
    p = _levels(_params())
    m = _metrics(p, p.copy())
    # levels 0, -10, -20, -30 (above -40: strictly above 1e-2 of the maximum); -40 ... -70 (-40 dB itself is not above);
    # -80 dB itself is not above 1e-4 of the maximum either: -80 ... -110 below
    assert (m["harm_count_above_m40db"], m["harm_count_m80_to_m40db"], m["harm_count_below_m80db"]) == (24, 24, 24)
    assert m["harm_cplx_abs_over_max"] == 0 and m["phse_max_rad_m80_to_m40db"] == 0 and m["ampl_rel_max_m80_to_m40db"] == 0
    # an error on one harmonic at -50 dB is seen by the band metrics, and one at -90 dB is not (outside the band)
    q = p.copy(); q.ampl[2, 5] *= 1.01; q.phse[3, 6] += 0.02
    m = _metrics(p, q)
    assert m["ampl_rel_max_m80_to_m40db"] == pytest.approx(0.01, rel=1e-9)
    assert m["phse_max_rad_m80_to_m40db"] == pytest.approx(0.02, rel=1e-9)
    q = p.copy(); q.ampl[2, 9] *= 1.5; q.phse[2, 10] += 1.0
    m = _metrics(p, q)
    assert m["ampl_rel_max_m80_to_m40db"] == 0 and m["phse_max_rad_m80_to_m40db"] == 0


@pytest.mark.parametrize("what", ["ampl", "phse"])
def test_weak_harmonic_error_is_flagged_under_the_complex_bound(what):
    """one harmonic below -60 dB, 3 x its band ceiling off: inside CONTRACT's complex 1e-5, outside HARM_CEILING"""
    p = _levels(_params())
    h = 7                                                     # -70 dB ... make it -76 dB
    p.ampl[:, h] = 0.5 * 10.0 ** (-76.0 / 20.0)
    q = p.copy()
    if what == "ampl":
        q.ampl[4, h] *= 1.0 + 3.0 * HARM_CEILING["ampl_rel_max_m80_to_m40db"]
    else:
        q.phse[4, h] += 3.0 * HARM_CEILING["phse_max_rad_m80_to_m40db"]
    m = _metrics(p, q)
    assert m["harm_cplx_abs_over_max"] < CONTRACT["harm_cplx_abs_over_max"], m["harm_cplx_abs_over_max"]
    bad = [b[0] for b in ceiling_violations(m)]
    key = "ampl_rel_max_m80_to_m40db" if what == "ampl" else "phse_max_rad_m80_to_m40db"
    assert key + " (harmonic ceiling)" in bad, bad


@pytest.mark.parametrize("thop, fs", [(0.005, 44100.0), (200.5 / 44100.0, 44100.0), (77.25 / 44100.0, 44100.0),
                                      (0.025, 44100.0), (0.005, 96000.0), (128.0 / 22050.0, 22050.0), (0.0075, 11025.0)])
def test_sin_geometry_is_the_reference_plan(o64, thop, fs):
    c, nwin = sin_geometry(300, thop, fs)
    assert nwin == o64.lib.o_idx_nwin_sin(thop, fs)
    assert [int(v) for v in c] == [o64.lib.o_idx_center(i, thop, fs) for i in range(300)]


def _synth(o, p, fs, seed=5):
    q = p.astype(o.dtype)
    y, ys, yn = o.synthesize(o.soptions(fs), q, seed=seed)
    return np.asarray(y, np.float64), np.asarray(ys, np.float64), np.asarray(yn, np.float64)


def _voiced_params(nfrm=200, fs=44100.0, thop=0.005, seed=3):
    p = Params(nfrm, 40, 0, 64, 1, thop, fs / 2, [], np.float64)
    r = np.random.default_rng(seed)
    p.f0[:] = 130.0 + 20.0 * np.sin(np.arange(nfrm) / 9.0)
    p.f0[60:70] = 0.0
    p.nhar[:] = 40; p.nhar[60:70] = 0
    p.ampl[:] = 0.1 * r.uniform(0.5, 1.0, p.ampl.shape) / np.arange(1, 41)
    p.ampl[60:70] = 0.0
    p.phse[:] = r.uniform(-np.pi, np.pi, p.phse.shape)
    p.psd[:] = -50.0 - 10.0 * np.linspace(0, 1, 64)
    return p.astype(np.float32).astype(np.float64)


def test_error_scale_covers_exactly_the_voiced_windows(o64):
    p = _voiced_params()
    fs = 44100.0
    _, ys, _ = _synth(o64, p, fs)
    S, cover = sin_error_scale(p, len(ys), p.thop, fs)
    c, nwin = sin_geometry(p.nfrm, p.thop, fs)
    # the unvoiced stretch: frames 60 .. 69 -> samples no voiced window reaches are exactly 0 in the oracle's output
    gap = slice(int(c[59]) + nwin // 2, int(c[70]) - nwin // 2)
    assert gap.stop > gap.start and not cover[gap].any() and np.all(S[gap] == 0) and np.all(ys[gap] == 0)
    assert np.all(S[cover][1:] > 0) or np.count_nonzero(S[cover] == 0) <= p.nfrm    # (a window's first sample is 0)
    m = synthesis_metrics(p, ys, ys, np.zeros(3), np.zeros(3), p.thop, fs)
    assert m["ysin_local"] == 0 and m["ysin_nonzero_uncovered"] == 0
    ys2 = ys.copy(); ys2[(gap.start + gap.stop) // 2] = 1e-30                      # any value where nothing is voiced
    assert synthesis_metrics(p, ys2, ys, np.zeros(3), np.zeros(3), p.thop, fs)["ysin_nonzero_uncovered"] == 1


def _one_hop(n, c, nwin, i):
    return slice(int(c[i]) - nwin // 4, int(c[i]) + nwin // 4)


def test_one_hop_error_is_flagged_under_syn_tol(o64):
    """1e-3 relative error in one hop of 200: whole-utterance relative RMS under SYN_TOL (and the new global ceilings),
    per-sample / per-hop metric over its ceiling, located in that hop"""
    p = _voiced_params()
    fs = 44100.0
    y, ys, yn = _synth(o64, p, fs)
    c, nwin = sin_geometry(p.nfrm, p.thop, fs)
    hop = _one_hop(len(ys), c, nwin, 120)
    ys2 = ys.copy(); ys2[hop] *= 1.0 + 1e-3
    yn2 = yn.copy(); yn2[hop] *= 1.0 + 1e-3
    m = synthesis_metrics(p, ys2, ys, yn2, yn, p.thop, fs, ys2 + yn2, y)
    assert m["ysin_rel_rms"] < SYN_TOL and m["ynoise_rel_rms"] < SYN_TOL and m["y_rel_rms"] < SYN_TOL, m
    bad = {b[0] for b in synthesis_violations(m)}
    assert {"ysin_local", "ynoise_local"} <= bad, (bad, m)
    assert hop.start <= m["ysin_local_at"] < hop.stop
    assert hop.start - nwin <= m["ynoise_local_at"] < hop.stop


def test_weak_harmonic_synthesis_error_is_flagged(o64):
    """harmonics 40 dB below the strongest one 1 % off: whole-utterance RMS far under SYN_TOL, per-sample metric over"""
    p = _voiced_params()
    p.ampl[:, 20:] *= 1e-2 * p.ampl[:, 0].max() / p.ampl[:, 20:].max()
    fs = 44100.0
    _, ys, yn = _synth(o64, p, fs)
    q = p.copy(); q.ampl[100:103, 20:] *= 1.01
    _, ys2, _ = _synth(o64, q, fs)
    m = synthesis_metrics(p, ys2, ys, yn, yn, p.thop, fs)
    assert rel_rms(ys2, ys) < SYN_TOL
    assert "ysin_local" in {b[0] for b in synthesis_violations(m)}, m


def test_noise_segments_use_the_local_level():
    """a hop 60 dB quieter than its neighbours more than a window away: its own error counts against its own level"""
    fs, thop = 44100.0, 0.005
    r = np.random.default_rng(5)
    yno = r.standard_normal(int(round(50 * thop * fs)))
    yno[2000:3500] *= 1e-3
    yn = yno.copy(); yn[2600:2800] += 1e-7 * r.standard_normal(200)
    v, at = noise_local(yn, yno, thop, fs)
    assert v > 5e-5 and 2600 - 2 * 441 <= at <= 2800, (v, at)
    assert rel_rms(yn, yno) < 1e-6


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_float32_oracle_against_the_sinusoid_scale(o64, o32, seed):
    """S[n] is a float32 error scale that float32 arithmetic really reaches, but the reference's own float build is NOT
    held to SYN_CEILING: it evaluates every phase 2 pi (k + 1) f0 / fs t in float32, so its error grows with harmonic number
    times window offset (measured 1 780 ... 2 090 units of S[n] on these seeds), where the product seeds its phasors from
    float64 phases every 128 harmonics.  The limits bracket that measurement, independent of the ceiling."""
    p = _voiced_params(nfrm=120, seed=seed)
    fs = 44100.0
    _, ys, _ = _synth(o64, p, fs)
    _, ys3, _ = _synth(o32, p, fs)
    m = synthesis_metrics(p, ys3, ys, np.zeros(3), np.zeros(3), p.thop, fs)
    assert 500.0 <= m["ysin_local"] <= 8000.0, m
    assert m["ysin_nonzero_uncovered"] == 0, m
