"""The noise-filter kernels on their own input, sample by sample against float64 (tests/noise_filter_reference.py, DESIGN.md
section 8).  Rows are built directly, float32-rounded; after the synthesis plane 15 (the excitation the filter read) and
y_noise come down, the oracle filters the downloaded plane, and the metric's rules (a), (b) and the zeros are applied to every
utterance.  Each configuration asserts the kernel it reaches (llsm_gpu_plan_index case 17), runs with the default units, with
units of 2 frames and with one unit per utterance (LLSM_GPU_NOISE_UNIT), and every fused size again with LLSM_GPU_NOISE_OLA=0 (k_noise_filter_wf + k_ola_noise_mix)."""
import numpy as np
import pytest

import libllsm2_amd as llsm
import noise_filter_reference as R
from gpu_common import CONVENTION_NAMES, params_to_gpu_rows, report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = llsm.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def oracles(o64, o32):
    R.follow_product_conventions((o64, o32), CONVENTION_NAMES)   # every convention set: nothing is left to an earlier test
    return o64, o32


def product_route(fused, npsd, thop, fs):
    return llsm.load().llsm_gpu_plan_index(17, int(fused), int(npsd), 0.0, thop, fs, 0.0)


def unit_count(total_frames, nfrm):
    """units the fused kernel cuts an utterance of nfrm frames into, under $LLSM_GPU_NOISE_UNIT as it stands"""
    sz = llsm.load().llsm_gpu_plan_index(18, int(total_frames), int(nfrm), 0.0, 0.0, 0.0, 0.0)
    assert sz >= 2
    return (nfrm + sz - 1) // sz


def _white(name, shape):
    """the injected template of an utterance: the same numbers wherever the utterance sits"""
    seed = sum(ord(ch) * (k + 1) for k, ch in enumerate(name))
    return np.random.default_rng(seed).standard_normal((shape[0], 20128)).astype(np.float32)[:, :shape[1]]


def synthesize(ctx, cfg, utts, monkeypatch, ola=True, unit=None):
    """{utterance name: (plane 15, y_noise)} of one batch"""
    for var, val in (("LLSM_GPU_NOISE_OLA", None if ola else "0"), ("LLSM_GPU_NOISE_UNIT", unit)):
        if val is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, str(val))
    fs = cfg["fs"]
    ao = llsm.make_aoptions(f0_refine=0, thop=cfg["thop"], maxnhar=4, maxnhar_e=0, npsd=cfg["npsd"], nchannel=2,
                            chanfreq=[fs / 4])
    b = llsm.Batch(ctx, ao, fs, [0] * len(utts), [p.nfrm for _, p, _ in utts])
    try:
        per = [params_to_gpu_rows(p) for _, p, _ in utts]
        rows = {aid: np.concatenate([r[aid] for r in per]) for aid in per[0]}
        rows[llsm.A_HAS_PSDRES] = np.concatenate([np.asarray(h, np.int32) for _, _, h in utts])
        b.upload_params(rows)
        if cfg["fnyq"] is not None:
            assert b.L.llsm_gpu_batch_set_fnyq(b.h, cfg["fnyq"]) == 0
        U, nch, ext = b.shape(llsm.A_WHITE)
        b.upload(llsm.A_WHITE, np.stack([_white(name, (nch, ext)) for name, _, _ in utts]))
        b.synthesize(llsm.make_soptions(fs), seed=0, injected_white=True)
        ctx.sync()
        exc, yn, off = b.debug_plane(15), b.download(llsm.A_YNOISE), np.array(b.y_off)
        assert len(exc) == len(yn) == off[-1]
    finally:
        b.close()
    return {name: (exc[off[u]:off[u + 1]], yn[off[u]:off[u + 1]]) for u, (name, _, _) in enumerate(utts)}


def judge_batch(tag, cfg, utts, got, refs, oracles):
    """rules (a), (b), zeros, finite on every utterance of one run; refs caches the references by utterance"""
    o64, o32 = oracles
    rep, bad = {}, []
    for name, p, has in utts:
        exc, yn = got[name]
        if name not in refs:
            refs[name] = (exc, R.Ref(o64, o32, p, has, cfg["fs"], exc))
        exc0, ref = refs[name]
        assert np.array_equal(exc, exc0), (tag, name, "plane 15 differs between runs")
        assert not ref.conditions(), (tag, name, ref.conditions())
        m = R.judge(yn, ref)
        rep[name] = dict(a_ratio=m["a_ratio"], a_units=m["a_units"], a_at=m["a_at"], b_ratio=m["b_ratio"], b_units=m["b_units"],
                         b_at=m["b_at"], bound=ref.bound, Y=ref.Y, A=ref.A, ny=ref.ny)
        if m["failed"]:
            bad.append((name, m["failed"], rep[name], m["nonzero_uncovered"][:8], m["nonfinite"][:8]))
    worst_a = max(rep, key=lambda n: rep[n]["a_ratio"]); worst_b = max(rep, key=lambda n: rep[n]["b_ratio"])
    report("noise_filter_" + tag, dict(worst_a=rep[worst_a]["a_ratio"], worst_a_utt=worst_a, worst_a_at=rep[worst_a]["a_at"],
                                       worst_b=rep[worst_b]["b_ratio"], worst_b_utt=worst_b, worst_b_at=rep[worst_b]["b_at"],
                                       utterances=rep))
    assert not bad, (tag, bad)
    return rep


def assert_bits(got, ref, names, where):
    for name in names:
        a, b = got[name][1], ref[name][1]
        assert a.shape == b.shape, (where, name)
        if not np.array_equal(a.view(np.uint32), b.view(np.uint32)):
            d = np.flatnonzero(a.view(np.uint32) != b.view(np.uint32))
            raise AssertionError("%s, %s: %d samples differ, first at %d" % (where, name, d.size, d[0]))


@pytest.mark.parametrize("cname", R.configuration_names())
def test_noise_filter_on_its_own_input(ctx, oracles, monkeypatch, cname):
    cfg = R.configurations(product_route)[cname]
    fused_size = cfg["N"] in R.FUSED_SIZES
    assert product_route(1, cfg["npsd"], cfg["thop"], cfg["fs"]) == cfg["route"], cname
    assert (cfg["route"] >= R.ROUTE_FUSED) == fused_size
    utts = R.make_utterances(cfg["fs"], cfg["thop"], cfg["npsd"], cfg["N"], cfg["nlong"], cfg["fnyq"])
    names = [u[0] for u in utts]
    refs = {}
    base = synthesize(ctx, cfg, utts, monkeypatch)
    assert any(np.any(base[n][1] != 0) for n in names)
    judge_batch(cname, cfg, utts, base, refs, oracles)
    # other cuts of the long utterance than the default's: units of 2 frames, shorter than every halo, and one unit for the
    # whole utterance with no halo at all -- each held to float64, and to the default run's bits
    total, nlong = sum(p.nfrm for _, p, _ in utts), utts[0][1].nfrm
    monkeypatch.delenv("LLSM_GPU_NOISE_UNIT", raising=False)
    cuts = {None: unit_count(total, nlong)}
    for unit in (2, 64):
        monkeypatch.setenv("LLSM_GPU_NOISE_UNIT", str(unit))
        cuts[unit] = unit_count(total, nlong)
        run = synthesize(ctx, cfg, utts, monkeypatch, unit=unit)
        judge_batch("%s_unit%d" % (cname, unit), cfg, utts, run, refs, oracles)
        assert_bits(run, base, names, "LLSM_GPU_NOISE_UNIT=%d against the default units" % unit)
    assert cuts[64] == 1 and cuts[2] == (nlong + 1) // 2 and len(set(cuts.values())) == 3, cuts
    # the batch reversed, and the long utterance alone: the same bits
    assert_bits(synthesize(ctx, cfg, utts[::-1], monkeypatch), base, names, "batch order reversed")
    assert_bits(synthesize(ctx, cfg, utts[:1], monkeypatch), base, names[:1], "long utterance alone")
    if fused_size:
        # the register kernel + the gathering mix, held to float64 like the fused kernel (not to its bits)
        assert product_route(0, cfg["npsd"], cfg["thop"], cfg["fs"]) == R.ROUTE_WF
        unfused = synthesize(ctx, cfg, utts, monkeypatch, ola=False)
        judge_batch(cname + "_unfused", cfg, utts, unfused, refs, oracles)
        assert_bits(synthesize(ctx, cfg, utts[::-1], monkeypatch, ola=False), unfused, names, "unfused, batch order reversed")


def test_plane_15_needs_a_synthesis(ctx):
    ao = llsm.make_aoptions(f0_refine=0, maxnhar_e=0, nchannel=1)
    b = llsm.Batch(ctx, ao, 44100.0, [0], [4])
    try:
        with pytest.raises(llsm.LlsmError, match="noise excitation"):
            b.debug_plane(15)
        with pytest.raises(llsm.LlsmError, match="bad arguments"):
            b.debug_plane(16)
    finally:
        b.close()
