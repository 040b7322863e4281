"""Offline layer-0 synthesis at the edges where its kernels branch, sample by sample against the float64 oracle
(tests/gpu_common.py synthesis_metrics).  The parameters are built directly, float32-rounded, and the same on both sides.

Branches of the harmonic part: k_synth_ola4 (nwin <= 496 and maxnhar <= 128) keeps a phasor table for one F0 per group
of units (SYN_TAB_MAXKS = 32 k-steps of four harmonics); frames of another F0 run the recurrences; k_synth_ola<NT> takes
wider windows or more harmonics, and synth_frame re-seeds its recurrences every SYN_RESEED = 32 k-steps (128 harmonics)."""
import numpy as np
import pytest

import libllsm2_amd as llsm
from gpu_common import assert_synthesis, params_to_gpu_rows, report, sin_error_scale, sin_geometry, synthesis_metrics
from oracle.oracle import Params

pytestmark = pytest.mark.gpu

# the harmonic part alone is held to the per-sample bound; the whole-utterance RMS values stay with the parity tests
SIN_ONLY = ("ysin_local", "ysin_rel_rms")
NOISE_ONLY = ("ynoise_local", "ynoise_rel_rms")


@pytest.fixture(scope="module")
def ctx():
    c = llsm.Context(0)
    yield c
    c.close()


def make_params(nfrm, maxnhar, thop, fs, npsd=64, nchannel=1):
    p = Params(nfrm, maxnhar, 0, npsd, nchannel, thop, fs / 2, [], np.float64)
    return p


def random_rows(p, seed, nhar, f0, voiced=None, tilt_db=0.0):
    """f0: scalar or per-frame; nhar: scalar or per-frame; amplitudes 0.1 x 10^(-tilt_db (k - 1) / (20 (nhar - 1))), random
    phases; unvoiced frames (voiced False) get F0 0 and no harmonics."""
    r = np.random.default_rng(seed)
    p.f0[:] = np.broadcast_to(np.asarray(f0, np.float64), (p.nfrm,))
    p.nhar[:] = np.broadcast_to(np.asarray(nhar, np.int32), (p.nfrm,))
    if voiced is not None:
        p.f0[~voiced] = 0.0; p.nhar[~voiced] = 0
    for i in range(p.nfrm):
        K = int(p.nhar[i])
        k = np.arange(K)
        p.ampl[i, :K] = 0.1 * 10.0 ** (-tilt_db * k / (20.0 * max(K - 1, 1))) * r.uniform(0.8, 1.2, K)
        p.phse[i, :K] = r.uniform(-np.pi, np.pi, K)
    return p


def run_both(ctx, o64, p, fs, seed=5):
    """the same float32-rounded parameters through the device and the float64 oracle -> synthesis_metrics"""
    q = p.astype(np.float32).astype(np.float64)
    ao = llsm.make_aoptions(f0_refine=0, thop=p.thop, maxnhar=p.maxnhar, maxnhar_e=0, npsd=p.npsd, nchannel=p.nchannel)
    b = llsm.Batch(ctx, ao, fs, [0], [p.nfrm])
    try:
        b.upload_params(params_to_gpu_rows(q))
        b.synthesize(llsm.make_soptions(fs), seed=seed)
        ctx.sync()
        ys, yn = b.download(llsm.A_YSIN), b.download(llsm.A_YNOISE)
    finally:
        b.close()
    yo, yso, yno = o64.synthesize(o64.soptions(fs), q, seed=seed)
    assert len(ys) == len(yso)
    return synthesis_metrics(q, ys, yso, yn, yno, p.thop, fs), ys, yso


def check_sin(ctx, o64, name, p, fs):
    m, ys, yso = run_both(ctx, o64, p, fs)
    report("synth_edge_" + name, m)
    assert np.any(yso != 0), name                     # (a bound on silence proves nothing)
    assert_synthesis(m, name, SIN_ONLY)
    return m


FS = 44100.0
H_NYQ = 275                                          # 80 Hz at 44.1 kHz: harmonic 275 at 22 000 Hz, 276 above Nyquist


def per_harmonic_local(p, hs, nper, ys, yso, fs):
    """{h: max |ys - yso| / (2^-24 S)} over the samples that only the nper frames of harmonic h cover"""
    q = p.astype(np.float32).astype(np.float64)
    S, _ = sin_error_scale(q, len(yso), p.thop, fs)
    c, _ = sin_geometry(p.nfrm, p.thop, fs)
    d = np.abs(np.asarray(ys, np.float64) - yso)
    out = {}
    for j, h in enumerate(hs):
        a, b = int(c[j * nper]), int(c[(j + 1) * nper - 1])      # frame i covers [c_i - hop, c_i + hop)
        pos = S[a:b] > 0
        out[h] = float(np.max(d[a:b][pos] / (2.0 ** -24 * S[a:b][pos])))
    return out


# k_synth_ola<NT> re-seeds its phasor recurrences from float64 phases every SYN_RESEED = 32 k-steps: harmonics 129 and 257
# start a fresh recurrence, harmonics 127, 128, 255 and 256 sit at the end of one.  The error of a single harmonic, in units
# of its own scale, grows along a recurrence (measured 2.5 ... 4.7 at harmonics 1 ... 5, 129 and 257; 51 ... 79 at 127, 128,
# 255 and 256, flat and moving F0): a re-seed that is skipped or seeded wrong leaves harmonic 129 at the drift of 128 and
# harmonic 257 at twice it (a build without the re-seed: 56 and 105).  So the first harmonics of every recurrence --
# 1 ... 5, 129, 257 -- are bounded on their own, at 3.4 x their worst value, and every harmonic at 3.5 x the worst of all.
RESEED_FRESH = 16.0
SINGLE_H_LOCAL = 280.0


@pytest.mark.parametrize("maxnhar", [128, 300])
def test_single_harmonic_frames(ctx, o64, maxnhar):
    """One harmonic per frame, h in {1 .. 5, 127, 128, 129, 255, 256, 257, highest below Nyquist}: the output is one windowed
    sinusoid and the bound is relative to that harmonic alone.  maxnhar 128: k_synth_ola4 (table + recurrence, no re-seed
    within its 32 k-steps); 300: k_synth_ola<NT>, whose re-seeds at harmonics 129 and 257 are checked per harmonic."""
    hs = [h for h in (1, 2, 3, 4, 5, 127, 128, 129, 255, 256, 257, H_NYQ) if h <= maxnhar]
    nper = 6
    p = make_params(nper * len(hs), maxnhar, 0.005, FS)
    r = np.random.default_rng(3)
    for j, h in enumerate(hs):
        for i in range(j * nper, (j + 1) * nper):
            p.nhar[i] = h
            p.ampl[i, h - 1] = 0.2
            p.phse[i, h - 1] = r.uniform(-np.pi, np.pi)
    # a flat F0, and an F0 that moves every frame (the recurrence path of k_synth_ola4 on every frame)
    for tag, f0 in (("", np.full(p.nfrm, 80.0)), ("_glide", 80.0 - 0.01 * np.arange(p.nfrm))):
        p.f0[:] = f0
        m, ys, yso = run_both(ctx, o64, p, FS)
        ph = per_harmonic_local(p, hs, nper, ys, yso, FS)
        report("synth_edge_single_h_%d%s" % (maxnhar, tag), dict(m, per_harmonic=ph))
        assert np.any(yso != 0)
        assert_synthesis(m, "single_h_%d%s" % (maxnhar, tag), ("ysin_rel_rms",))
        assert m["ysin_local"] <= SINGLE_H_LOCAL, (maxnhar, tag, ph)
        fresh = {h: v for h, v in ph.items() if h <= 5 or (maxnhar > 128 and h in (129, 257))}
        assert max(fresh.values()) <= RESEED_FRESH, (maxnhar, tag, ph)


# maxnhar 128: k_synth_ola4 (the phasor table holds all 32 k-steps); 320: k_synth_ola<NT> (re-seeds at 129 and 257)
NHAR_CASES = [(128, n) for n in (1, 2, 3, 5, 127, 128, "maxnhar", "varying")] + \
             [(320, n) for n in (1, 2, 3, 5, 127, 128, 129, 300, "maxnhar", "varying")]


@pytest.mark.parametrize("maxnhar, nhar", NHAR_CASES)
def test_nhar_around_kstep_and_table(ctx, o64, maxnhar, nhar):
    p = make_params(40, maxnhar, 0.005, FS)
    if nhar == "maxnhar":
        nh = maxnhar
    elif nhar == "varying":                           # changes from frame to frame across 4, 128 (and 256)
        nh = np.array([1, 4, 5, 127, 128, 129, 3, 255, 256, 257, 300, 320] * 4)[:40]
        nh = np.minimum(nh, maxnhar)
    else:
        nh = nhar
    random_rows(p, 11, nh, 60.0)                       # 60 Hz: 367 harmonics below Nyquist
    check_sin(ctx, o64, "nhar_%d_%s" % (maxnhar, nhar), p, FS)


@pytest.mark.parametrize("maxnhar", [100, 128, 300])
def test_amplitude_tilt(ctx, o64, maxnhar):
    """Strong low harmonics, weak high ones down to -80 dB; then the weak ones alone (strong ones zeroed), held to the
    bound at their own scale: an error confined to weak harmonics is not hidden by the strong ones' scale."""
    p = make_params(40, maxnhar, 0.005, FS)
    random_rows(p, 17, maxnhar, 70.0, tilt_db=80.0)
    check_sin(ctx, o64, "tilt_%d" % maxnhar, p, FS)
    k = np.arange(maxnhar)
    weak = 0.1 * 10.0 ** (-80.0 * k / (20.0 * (maxnhar - 1))) < 0.1 * 10.0 ** (-40.0 / 20.0)
    p.ampl[:, ~weak] = 0.0
    check_sin(ctx, o64, "tilt_weak_only_%d" % maxnhar, p, FS)


def test_table_and_recurrence_paths(ctx, o64):
    """k_synth_ola4: a flat F0 (every frame reads the group's phasor table), an F0 one float32 ulp off the table's F0 on
    alternate frames (recurrences), and an F0 that changes every frame -- each against the oracle."""
    for name, mk in (("flat", lambda n: np.full(n, 130.0)),
                     ("one_ulp_off", lambda n: np.where(np.arange(n) % 2 == 1,
                                                        float(np.nextafter(np.float32(130.0), np.float32(200.0))), 130.0)),
                     ("every_frame", lambda n: 120.0 + 0.37 * np.arange(n))):
        p = make_params(64, 128, 0.005, FS)
        random_rows(p, 23, 128, mk(p.nfrm), tilt_db=40.0)
        check_sin(ctx, o64, "paths_" + name, p, FS)


# (name, fs, thop, nfrm, maxnhar, voiced pattern)
GEOMETRY = {
    "ola4_nwin_442": (44100.0, 0.005, 60, 100, "all"),
    "olaNT_25ms_44k": (44100.0, 0.025, 24, 100, "all"),
    "olaNT_96k": (96000.0, 0.005, 40, 100, "all"),
    "noninteger_hop": (44100.0, 200.5 / 44100.0, 50, 100, "all"),
    "noninteger_hop_77_25": (44100.0, 77.25 / 44100.0, 80, 60, "all"),
    "shorter_than_nwin": (44100.0, 200.5 / 44100.0, 1, 100, "all"),
    "voiced_first_last_only": (44100.0, 0.005, 40, 100, "ends"),
    "isolated_voiced_frame": (44100.0, 0.005, 40, 100, "isolated"),
    "run_at_unit_boundary": (44100.0, 0.005, 100, 100, "unit"),
    "run_at_unit_boundary_olaNT": (44100.0, 0.005, 100, 200, "unit"),
}


@pytest.mark.parametrize("gid", sorted(GEOMETRY))
def test_geometry(ctx, o64, gid):
    fs, thop, nfrm, maxnhar, pat = GEOMETRY[gid]
    p = make_params(nfrm, maxnhar, thop, fs)
    v = np.ones(nfrm, bool)
    if pat == "ends":
        v[:] = False; v[0] = v[-1] = True
    elif pat == "isolated":
        v[:] = False; v[nfrm // 2 + 1] = True
    elif pat == "unit":
        sz = llsm.load().llsm_gpu_plan_index(14, nfrm, maxnhar, 0.0, thop, fs, 4.0)   # the engine's own unit split
        assert 0 < 2 * sz < nfrm, sz
        v[:] = False; v[2 * sz: 2 * sz + 7] = True           # the run starts exactly at the third unit
    nh = min(maxnhar, int(0.5 * fs / 150.0))
    random_rows(p, 29, nh, 150.0, voiced=v, tilt_db=30.0)
    check_sin(ctx, o64, "geom_" + gid, p, fs)


def test_noise_psd_steps_and_bursts(ctx, o64):
    """Noise part, same seed on both sides: a PSD that steps by 60 dB between neighbouring frames, and a one-frame unvoiced
    burst inside a voiced run, each hop held to the noise level around it."""
    nfrm = 60
    p = make_params(nfrm, 40, 0.005, FS, npsd=64)
    v = np.ones(nfrm, bool); v[30] = False
    random_rows(p, 31, 40, 140.0, voiced=v, tilt_db=30.0)
    base = -40.0 - 20.0 * np.linspace(0.0, 1.0, p.npsd)
    for i in range(nfrm):
        p.psd[i] = base - (60.0 if (i // 3) % 2 else 0.0)   # 60 dB steps every third frame
    p.psd[30] = base + 20.0                                  # the unvoiced burst
    m, _, _ = run_both(ctx, o64, p, FS, seed=9)
    report("synth_edge_noise", m)
    assert_synthesis(m, "noise", NOISE_ONLY)
    assert_synthesis(m, "noise_sin", SIN_ONLY)
