"""Harmonic analysis at every level (tests/gpu_common.py HARM_CEILING): synthetic inputs whose harmonic levels fall steeply,
so that many harmonics sit in every band from 0 down to -90 dB re the strongest one.  Each case reaches one analysis path
(shared-F0 rows of k_harm_speech_tile, the per-frame k_harm_speech / k_harm_speech_rest, low F0 with long windows, high F0
with few harmonics) and is held to the float64 oracle with the layer-0 contract, HARM_CEILING included (not the PSD ceiling: see below); each also
asserts that the level bands it claims to test are populated."""
import numpy as np
import pytest

import libllsm2_amd as llsm
from gpu_common import HARM_CEILING, Yard, analysis_metrics, aopt_kwargs, contract_violations, gpu_analyze, report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = llsm.Context(0)
    yield c
    c.close()


def steep_input(seed, fs, thop, f0, maxnhar, span_db=90.0, sigma=1e-4):
    """x = sum_k 0.3 10^(-span_db (k - 1) / (20 (K - 1))) cos(k phase(t) + phi_k) + sigma noise, K = the harmonics below
    Nyquist (at most maxnhar) of the highest F0 of the track; f0: per-frame track (Hz, all voiced)."""
    rng = np.random.default_rng(seed)
    nfrm = len(f0)
    nx = int(round((nfrm + 1) * thop * fs))
    K = int(min(maxnhar, np.floor(0.5 * fs / float(np.max(f0)) - 1e-9)))
    ts = np.arange(nx) / fs
    f0s = np.interp(ts, np.arange(nfrm) * thop, f0)
    phase = 2 * np.pi * np.cumsum(f0s) / fs
    x = np.zeros(nx)
    step = span_db / max(K - 1, 1)
    for k in range(1, K + 1):
        x += 0.3 * 10.0 ** (-step * (k - 1) / 20.0) * np.cos(k * phase + rng.uniform(-np.pi, np.pi))
    x += sigma * rng.standard_normal(nx)
    return x.astype(np.float32), np.asarray(f0, np.float32), K


def _track(kind, nfrm):
    i = np.arange(nfrm)
    if kind == "flat":                   # every 16-frame block shares one F0: tile rows
        return np.full(nfrm, 120.0)
    if kind == "glide":                  # a new F0 every frame: k_harm_speech
        return 110.0 + 60.0 * i / nfrm + 3.0 * np.sin(0.9 * i)
    if kind == "mixed":                  # flat blocks with gliding stretches between them: tiles + the frames they leave
        return np.where((i // 23) % 2 == 0, 150.0, 150.0 + 0.7 * (i % 23))
    raise ValueError(kind)


# (fs, thop, F0 track kind or constant Hz, maxnhar, frames)
CASES = {
    "tile_flat_120hz": (44100.0, 0.005, "flat", 100, 64),
    "per_frame_glide": (44100.0, 0.005, "glide", 100, 48),
    "tiles_and_rest": (44100.0, 0.005, "mixed", 100, 70),
    "low_f0_55hz_long_windows": (44100.0, 0.01, 55.0, 100, 30),
    "many_harmonics_200": (44100.0, 0.005, 100.0, 200, 40),
    "high_f0_1000hz_16k": (16000.0, 0.005, 1000.0, 100, 48),
    "high_f0_glide_8k": (8000.0, 0.004, "glide", 60, 48),
}


@pytest.mark.parametrize("cid", sorted(CASES))
def test_harmonic_levels_against_oracle(ctx, o64, cid):
    fs, thop, kind, maxnhar, nfrm = CASES[cid]
    f0 = _track(kind, nfrm) if isinstance(kind, str) else np.full(nfrm, kind)
    if cid == "high_f0_glide_8k":
        f0 = 5.0 * f0                     # 550 ... 850 Hz at 8 kHz: 3 ... 6 harmonics
    x, f0, K = steep_input(sum(cid.encode()), fs, thop, f0, maxnhar)
    ao = llsm.make_aoptions(f0_refine=0, thop=thop, maxnhar=maxnhar)
    okw = aopt_kwargs(ao)
    pr, xr = o64.analyze(o64.aoptions(**okw), x, fs, f0, want_res=True)
    b, g, xres = gpu_analyze(ctx, ao, fs, [x], [f0])
    try:
        m = analysis_metrics(g, slice(0, len(f0)), pr, xres, xr)
    finally:
        b.close()
    m["harmonics_per_frame"] = K
    report("levels_" + cid, m)
    # the bands this case claims: every voiced frame has harmonics above -40 dB and between -80 and -40 dB
    assert m["harm_count_above_m40db"] >= nfrm, (cid, m["harm_count_above_m40db"])
    assert m["harm_count_m80_to_m40db"] >= nfrm, (cid, m["harm_count_m80_to_m40db"])
    if K >= 20:                           # ... and, where there are enough harmonics, many of them and some below -80 dB
        assert m["harm_count_m80_to_m40db"] >= 0.3 * m["harm_count"], (cid, m["harm_count_m80_to_m40db"], m["harm_count"])
        assert m["harm_count_below_m80db"] >= nfrm, (cid, m["harm_count_below_m80db"])
    for k in HARM_CEILING:
        assert k in m
    # The whole contract, CONDITIONED and HARM_CEILING included.  Not the noise-side CEILING (PSD, band energies): it was
    # calibrated on speech-like inputs, and on these nearly noise-free residuals the float64 oracle's own response to a
    # one-ulp input perturbation covers the band-energy and PSD errors (measured: band energies 2.3e-3 relative at 55 Hz,
    # 12 PSD values over 0.05 dB with 200 harmonics) -- the algorithm's conditioning, not the harmonic kernels under test.
    bad = [v for v in contract_violations(m, Yard(okw, x, fs, f0), ulp_response=Yard(okw, x, fs, f0).ulp)
           if not v[0].endswith(" (ceiling)")]
    assert not bad, (cid, bad)
