"""-m gpu: the persistent noise-excitation kernel (k_excite_units, the default) gives y_noise bit-identical to the
per-sample kernel (k_excite_env, $LLSM_GPU_EXCITE4=0): the same (frame, offset) pairs, phasors, accumulation order,
square root and channel sum, with the complex amplitudes formed in the kernel by k_env_params' expression.

Geometries: the bench batch (1 s utterances, F0 120 Hz), ragged lengths (tiles and cross-fades, exactly the template,
shorter than it, not a multiple of four, empty), eight envelope harmonics on two channels, 16 kHz at a 200.5-sample
hop, and one long utterance alone and at index 8 of batches of 255 and 256 with injected white templates."""
import numpy as np
import pytest

import libllsm2_amd as llsm
from conftest import FS, make_speechlike, make_utterance
from gpu_common import gpu_analyze

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = llsm.Context(0)
    yield c
    c.close()


def _ynoise(ctx, b, monkeypatch, sel, fs, **kw):
    if sel is None:
        monkeypatch.delenv("LLSM_GPU_EXCITE4", raising=False)
    else:
        monkeypatch.setenv("LLSM_GPU_EXCITE4", sel)
    b.synthesize(llsm.make_soptions(fs), **kw); ctx.sync()
    return b.download(llsm.A_YNOISE)


def _assert_bits(got, ref, where):
    assert got.shape == ref.shape, where
    if not np.array_equal(got, ref):
        d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
        raise AssertionError(f"{where}: {np.count_nonzero(d)} samples differ, max |diff| {d.max():.3g}")


def _units_vs_per_sample(ctx, monkeypatch, ao, fs, xs, f0s):
    b, _, _ = gpu_analyze(ctx, ao, fs, xs, f0s)
    try:
        ref = _ynoise(ctx, b, monkeypatch, "0", fs, seed=21)
        got = _ynoise(ctx, b, monkeypatch, None, fs, seed=21)
        assert np.all(np.isfinite(got)) and np.abs(ref).max() > 0
        _assert_bits(got, ref, "y_noise")
    finally:
        b.close()


def test_bench_geometry(ctx, monkeypatch):
    xs = [make_utterance(u, 120.0) for u in range(64)]
    f0 = np.full(int(44100 / FS / 0.005), 120.0, np.float32)
    _units_vs_per_sample(ctx, monkeypatch, llsm.make_aoptions(f0_refine=0), FS, xs, [f0] * len(xs))


@pytest.mark.parametrize("case", ["ragged", "eight_envelope_harmonics", "hop_200_5_at_16k"])
def test_other_geometries(ctx, monkeypatch, case):
    fs, thop, kw = FS, 0.005, dict()
    lens = [int(3.1 * fs), 5003]
    if case == "ragged":
        lens = [int(1.0 * fs), int(1.55 * fs), 20000, 19999, 20131, 7001, 0]
    elif case == "eight_envelope_harmonics":
        kw = dict(maxnhar_e=8, nchannel=2, chanfreq=[3000.0])
    else:
        fs, thop, kw = 16000.0, 200.5 / 16000.0, dict(nchannel=2, chanfreq=[3000.0], maxnhar_e=3)
        lens = [int(1.0 * fs), int(3.1 * fs), 20131, 5003]
    xs, f0s = [], []
    for k, nx in enumerate(lens):
        if nx == 0:
            xs.append(np.zeros(0, np.float32)); f0s.append(np.zeros(0, np.float32)); continue
        x, f0 = make_speechlike(70 + k, nx=nx, fs=fs, thop=thop)
        xs.append(x); f0s.append(f0.astype(np.float32))
    _units_vs_per_sample(ctx, monkeypatch, llsm.make_aoptions(f0_refine=0, thop=thop, **kw), fs, xs, f0s)


def test_alone_and_inside_batches_of_255_and_256(ctx, monkeypatch):
    x, f0 = make_speechlike(4242, nx=150000)
    f0 = f0.astype(np.float32)
    ao = llsm.make_aoptions(f0_refine=0)
    b1, g1, _ = gpu_analyze(ctx, ao, FS, [x], [f0])
    rows = {a: g1[a].copy() for a in llsm.Batch.PARAM_IDS}
    nt = b1.layout.ntemplate_ext
    white_long = np.random.default_rng(31).standard_normal((4, nt)).astype(np.float32)
    try:
        b1.upload(llsm.A_WHITE, white_long[None])
        ref = _ynoise(ctx, b1, monkeypatch, "0", FS, seed=0, injected_white=True)
        alone = _ynoise(ctx, b1, monkeypatch, None, FS, seed=0, injected_white=True)
    finally:
        b1.close()
    assert np.abs(ref).max() > 0
    _assert_bits(alone, ref, "alone")
    k = 8
    for U in (255, 256):
        xs, f0s = [], []
        for u in range(U - 1):
            xf, ff = make_speechlike(5000 + u % 16, nx=(4410, 4631, 4852)[u % 3])
            xs.append(xf); f0s.append(ff.astype(np.float32))
        xs.insert(k, x); f0s.insert(k, f0)
        b, g, _ = gpu_analyze(ctx, ao, FS, xs, f0s)
        try:
            f_a, f_b = int(b.frm_off[k]), int(b.frm_off[k + 1])
            for a in llsm.Batch.PARAM_IDS:
                g[a][f_a:f_b] = rows[a]
            b.upload_params(g)
            white = np.random.default_rng(32).standard_normal((U, 4, nt)).astype(np.float32)
            white[k] = white_long
            b.upload(llsm.A_WHITE, white)
            got = _ynoise(ctx, b, monkeypatch, None, FS, seed=0, injected_white=True)
            _assert_bits(got[int(b.y_off[k]):int(b.y_off[k + 1])], ref, f"utterance {k} of {U}")
        finally:
            b.close()
