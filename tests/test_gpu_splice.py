"""-m gpu: llsm_gpu_batch_splice -- frames gathered across the utterances of another batch and blended between two sides,
out = P(P(S[ua][a], S[ua][a + 1], ra), P(S[ub][b], S[ub][b + 1], rb), mix) with P the pair rule of llsm_gpu_batch_retime.
Checked against retime itself where retime applies (bit-identical), against exact copies (gather), against the numpy
restatement of P in test_gpu_retime.py at that file's bounds (lin and integer rows bit-identical, fades within 1e-4 dB,
circular blends |v| |e^{j phi} - e^{j phi_ref}| <= 2e-6), and, for the nesting, against retime run on the two sides' rows
interleaved on the device (bit-identical).  Synthetic layer-1 rows at nfft 1024 (nspec 513), npsd 129 / 256, maxnhar 77,
three channels, maxnhar_e 0 / 5; the end-to-end tests use analysed utterances."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import libllsm2_amd as llsm
from conftest import FS
from test_gpu_retime import INT, ROWS, analysed, assert_retime_rows, beq, bits, ref_retime, rows_of

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NFFT = 1024
SN = np.array([13, 1, 40, 7, 22, 2, 31], np.int32)          # src: seven utterances, one of a single frame
DN = np.array([9, 21, 1, 14, 16], np.int32)                 # dst: five utterances, 61 frames (not a multiple of four)


@pytest.fixture(scope="module")
def ctx():
    c = llsm.Context(0)
    yield c
    c.close()


def synthetic_src(ctx, ao, nfrm, seed, nfft=NFFT):
    """test_gpu_retime.synthetic_src restated, with voicing in runs: a layer-1 batch of plausible random rows (voiced
    runs, unvoiced gaps, varying counts) without an analysis"""
    rng = np.random.default_rng(seed)
    b = llsm.Batch(ctx, ao, FS, [0] * len(nfrm), nfrm)
    b.enable_layer1(nfft)
    F = b.layout.total_frames
    r = {}
    for aid in ROWS:
        shp = b.shape(aid)
        r[aid] = rng.uniform(-3, 3, shp).astype(np.float32) if aid not in INT else rng.integers(0, 2, shp).astype(np.int32)
    voiced = np.repeat(rng.random(F) < 0.7, rng.integers(1, 5, F))[:F]
    r[llsm.A_F0] = np.where(voiced, rng.uniform(80, 300, F), 0).astype(np.float32)
    r[llsm.A_NHAR] = rng.integers(0, b.layout.maxnhar + 1, F).astype(np.int32)
    r[llsm.A_NVSPHSE] = rng.integers(0, b.layout.maxnhar + 1, F).astype(np.int32)
    r[llsm.A_NHAR_E] = rng.integers(0, b.layout.maxnhar_e + 1, F).astype(np.int32)
    r[llsm.A_VTMAGN] = rng.uniform(-100, 0, b.shape(llsm.A_VTMAGN)).astype(np.float32)
    for aid, a in r.items():
        b.upload(aid, a)
    return b, r


@pytest.fixture(scope="module", params=[(129, 0), (256, 5)], ids=["npsd129-me0", "npsd256-me5"])
def world(ctx, request):
    npsd, me = request.param
    ao = llsm.make_aoptions(f0_refine=0, npsd=npsd, maxnhar=77, nchannel=3, maxnhar_e=me, chanfreq=[2000.0, 6000.0])
    src, rows = synthetic_src(ctx, ao, SN, 100 + npsd)
    yield ao, src, rows
    ctx.sync()
    after = rows_of(src)                                     # src is only read by every accepted call of this module
    for aid in ROWS:
        assert beq(after[aid], rows[aid]), aid
    src.close()


def new_dst(ctx, ao, dn=DN):
    return llsm.Batch(ctx, ao, FS, [0] * len(dn), dn)


def random_side(rng, sn, F, integer=False):
    """F (utterance, position) pairs over the utterances of sn, with end points and integral positions mixed in"""
    utt = rng.integers(0, len(sn), F).astype(np.int32)
    n = sn[utt]
    pos = (rng.random(F) * (n - 1)).astype(np.float32)
    kind = rng.integers(0, 6, F)
    pos[kind == 0] = np.floor(pos[kind == 0])
    pos[kind == 1] = (n - 1)[kind == 1]
    if integer:
        pos = np.floor(pos)
    return utt, np.minimum(pos, (n - 1).astype(np.float32)).astype(np.float32)


def spliced(ctx, ao, src, dn, **kw):
    d = new_dst(ctx, ao, dn)
    d.splice(src, **kw)
    ctx.sync()
    got = rows_of(d)
    d.close()
    return got


def assert_same(got, want, where, skip=()):
    for aid in ROWS:
        if aid in skip:
            continue
        bad = np.flatnonzero((bits(got[aid]) != bits(want[aid])).reshape(len(got[aid]), -1).any(1))
        assert bad.size == 0, (where, aid, bad[:8])


def ref_one_level(rows, src, utt, pos):
    """P(S[u][a], S[u][a + 1], r) of every output frame by test_gpu_retime.ref_retime: each output frame is an utterance of
    one frame whose source utterance is utt[g]"""
    F = len(utt)
    return ref_retime(rows, src.frm_off[utt], SN[utt], np.arange(F + 1), np.ones(F, np.int32), pos, None)


# ------------------------------------------------------------------ 2: splice equals retime where retime applies
@pytest.mark.parametrize("kind", ["random", "integer", "uniform"])
def test_splice_equals_retime_where_retime_applies(ctx, world, kind):
    ao, src, rows = world
    rng = np.random.default_rng(21)
    dn = np.array([20, 3, 23, 7, 9, 5, 34], np.int32)       # 101 frames, the utterance counts agree
    F = int(dn.sum())
    own = np.repeat(np.arange(len(dn)), dn).astype(np.int32)
    if kind == "uniform":
        pos = np.concatenate([llsm.retime_uniform_positions(n, m) for n, m in zip(SN, dn)])
    else:
        pos = (rng.random(F) * (SN[own] - 1)).astype(np.float32)
        pos[::5] = np.floor(pos[::5]); pos[3::11] = (SN[own] - 1)[3::11]
        if kind == "integer":
            pos = np.floor(pos)
    ref = new_dst(ctx, ao, dn)
    ref.retime(src, None if kind == "uniform" else pos, None)
    ctx.sync()
    want = rows_of(ref)
    ref.close()
    utt_b, pos_b = random_side(rng, SN, F)
    for where, kw in (("own utterance", dict(pos_a=pos)), ("identity utt_a", dict(pos_a=pos, utt_a=own)),
                      ("mix all zero", dict(pos_a=pos, utt_b=utt_b, pos_b=pos_b, mix=np.zeros(F, np.float32)))):
        assert_same(spliced(ctx, ao, src, dn, **kw), want, (kind, where))


# ------------------------------------------------------------------ 3: the gather
def test_integer_positions_gather_exact_copies(ctx, world):
    ao, src, rows = world
    rng = np.random.default_rng(31)
    F = int(DN.sum())
    utt, pos = random_side(rng, SN, F, integer=True)
    utt[:8] = [6, 6, 1, 0, 6, 1, 2, 2]; pos[:8] = [30, 0, 0, 12, 30, 0, 39, 0]     # repeats, end points, the one-frame utterance
    g = src.frm_off[utt] + pos.astype(np.int64)
    want = {aid: rows[aid][g] for aid in ROWS}
    assert_same(spliced(ctx, ao, src, DN, pos_a=pos, utt_a=utt), want, "side a")
    other_u, other_p = random_side(rng, SN, F)
    got = spliced(ctx, ao, src, DN, pos_a=other_p, utt_a=other_u, utt_b=utt, pos_b=pos, mix=np.ones(F, np.float32))
    assert_same(got, want, "side b at mix 1")


# ------------------------------------------------------------------ 4: the rules, one level
def test_one_level_follows_the_pair_rule(ctx, world):
    ao, src, rows = world
    rng = np.random.default_rng(41)
    dn = np.array([40, 1, 77, 23, 60], np.int32)            # 201 frames
    F = int(dn.sum())
    ua, pa = random_side(rng, SN, F)
    ub, pb = random_side(rng, SN, F)
    mix = (rng.random(F) < 0.5).astype(np.float32)
    got = spliced(ctx, ao, src, dn, pos_a=pa, utt_a=ua, utt_b=ub, pos_b=pb, mix=mix)
    utt, pos = np.where(mix == 1, ub, ua), np.where(mix == 1, pb, pa).astype(np.float32)
    want, aux = ref_one_level(rows, src, utt, pos)
    assert_retime_rows(got, want, aux, "one level")
    kinds = {k: aux["kinds"].count(k) for k in set(aux["kinds"])}
    for k in ("copy", "vv", "vv~", "vu", "uv", "uu"):
        assert kinds.get(k, 0) > 0, (k, kinds)                # every branch of the rule was exercised


# ------------------------------------------------------------------ 5: the nesting, device against device
def test_nesting_equals_retime_of_the_two_sides(ctx, world):
    ao, src, rows = world
    rng = np.random.default_rng(51)
    dn = np.array([50, 1, 90, 33, 63], np.int32)            # 237 frames (< 2^14: 2 g + mix is exact in float32)
    F = int(dn.sum())
    ua, pa = random_side(rng, SN, F)
    ub, pb = random_side(rng, SN, F)
    mix = (rng.integers(0, 257, F) / 256.0).astype(np.float32)
    mix[::7] = 0; mix[3::13] = 1; mix[5::17] = 0.5
    side_a = spliced(ctx, ao, src, dn, pos_a=pa, utt_a=ua)
    side_b = spliced(ctx, ao, src, dn, pos_a=pb, utt_a=ub, utt_b=ua, pos_b=pa, mix=np.zeros(F, np.float32))
    inter = llsm.Batch(ctx, ao, FS, [0], [2 * F]); inter.enable_layer1(NFFT)
    irows = {}
    for aid in ROWS:
        irows[aid] = np.stack([side_a[aid], side_b[aid]], 1).reshape((2 * F,) + side_a[aid].shape[1:])
        inter.upload(aid, irows[aid])
    g = np.arange(F)
    pos = (2 * g).astype(np.float32) + mix
    assert np.array_equal(pos.astype(np.float64), 2.0 * g + mix.astype(np.float64))
    res = (2 * g + (mix >= 0.5)).astype(np.int32)
    ref = llsm.Batch(ctx, ao, FS, [0], [F])
    ref.retime(inter, pos, res)
    ctx.sync()
    want = rows_of(ref)
    ref.close(); inter.close()
    got = spliced(ctx, ao, src, dn, pos_a=pa, utt_a=ua, utt_b=ub, pos_b=pb, mix=mix)
    assert_same(got, want, "nesting")
    # the frames between the two sides met every case, with differing counts too, and numpy agrees on them
    va, vb = side_a[llsm.A_F0] > 0, side_b[llsm.A_F0] > 0
    mid = (mix > 0) & (mix < 1)
    assert (mid & va & vb).any() and (mid & va & ~vb).any() and (mid & ~va & vb).any() and (mid & ~va & ~vb).any()
    assert (mid & (side_a[llsm.A_NVSPHSE] != side_b[llsm.A_NVSPHSE])).any()
    if ao.maxnhar_e > 0:
        assert (mid & (side_a[llsm.A_NHAR_E] != side_b[llsm.A_NHAR_E])).any()
    wnp, aux = ref_retime(irows, [0], [2 * F], [0, F], [F], pos, res)
    assert_retime_rows(got, wnp, aux, "nesting, numpy")


# ------------------------------------------------------------------ 6: invariance
@pytest.mark.parametrize("dn", [np.array([9, 21, 1, 14, 16], np.int32), np.array([9, 21, 1, 14, 19], np.int32)],
                         ids=["61-frames", "64-frames"])
def test_an_utterance_does_not_depend_on_the_rest(ctx, world, dn):
    ao, src, rows = world
    rng = np.random.default_rng(61)
    F = int(dn.sum())
    ua, pa = random_side(rng, SN, F)
    ub, pb = random_side(rng, SN, F)
    mix = rng.choice(np.array([0, 0.25, 0.5, 0.8125, 1], np.float32), F)
    whole = spliced(ctx, ao, src, dn, pos_a=pa, utt_a=ua, utt_b=ub, pos_b=pb, mix=mix)
    off = np.concatenate([[0], np.cumsum(dn)])
    for u in range(len(dn)):
        d0, d1 = int(off[u]), int(off[u + 1])
        named = np.unique(np.concatenate([ua[d0:d1], ub[d0:d1]]))
        sub = llsm.Batch(ctx, ao, FS, [0] * len(named), SN[named]); sub.enable_layer1(NFFT)
        pick = np.concatenate([np.arange(src.frm_off[v], src.frm_off[v + 1]) for v in named])
        for aid in ROWS:
            sub.upload(aid, rows[aid][pick])
        remap = {int(v): i for i, v in enumerate(named)}
        alone = spliced(ctx, ao, sub, dn[u:u + 1], pos_a=pa[d0:d1], utt_a=[remap[int(v)] for v in ua[d0:d1]],
                        utt_b=[remap[int(v)] for v in ub[d0:d1]], pos_b=pb[d0:d1], mix=mix[d0:d1])
        sub.close()
        assert_same(alone, {aid: whole[aid][d0:d1] for aid in ROWS}, ("utterance", u))


# ------------------------------------------------------------------ 7: identity gather down to the samples
def outputs(b, so, white, seed=9):
    b.tolayer0(True)
    b.upload(llsm.A_WHITE, white)
    b.synthesize(so, seed=seed, injected_white=True)
    return b.download(llsm.A_Y), b.download(llsm.A_YSIN), b.download(llsm.A_YNOISE)


def test_identity_gather_is_exact_down_to_the_samples(ctx):
    src, ao = analysed(ctx)                                  # four utterances of 30 000 samples, layer 1
    so = llsm.make_soptions(FS)
    s = rows_of(src)
    g0, g1 = int(src.frm_off[3]), int(src.frm_off[4])
    n = g1 - g0
    got = llsm.Batch(ctx, ao, FS, [0], [n])
    got.splice(src, pos_a=np.arange(n, dtype=np.float32), utt_a=np.full(n, 3, np.int32))
    one = llsm.Batch(ctx, ao, FS, [0], [n]); one.enable_layer1(2 * (src.nspec - 1))
    for aid in ROWS:
        one.upload(aid, s[aid][g0:g1])
    want = llsm.Batch(ctx, ao, FS, [0], [n])
    want.retime(one)                                         # the identity map of that utterance alone
    ctx.sync()
    assert_same(rows_of(got), rows_of(want), "rows")
    white = np.random.default_rng(7).standard_normal(got.shape(llsm.A_WHITE)).astype(np.float32)
    ya, yb = outputs(got, so, white), outputs(want, so, white)
    ctx.sync()
    for a, b_ in zip(ya, yb):
        assert a.shape == b_.shape and a.size > 0 and beq(a, b_)
    assert float(np.abs(ya[0]).max()) > 1e-3
    for b in (got, want, one, src):
        b.close()


# ------------------------------------------------------------------ 8: a join
def test_a_join_with_a_cross_fade(ctx):
    src, ao = analysed(ctx, n_utt=2)
    so = llsm.make_soptions(FS)
    src.phasepropagate(-1)
    ctx.sync()
    s = rows_of(src)
    # utterance 0 frames 0 .. 29, ten frames of both (0: 30 .. 39, 1: 80 .. 89, all voiced), utterance 1 frames 90 .. 135
    n_pre, n_fade, b0 = 30, 10, 80
    n1 = int(src.frm_off[2] - src.frm_off[1])
    n_post = n1 - (b0 + n_fade)
    F = n_pre + n_fade + n_post
    i = np.arange(F)
    pos_a = np.minimum(i, n_pre + n_fade - 1).astype(np.float32)
    pos_b = np.clip(i - n_pre + b0, 0, n1 - 1).astype(np.float32)
    mix = np.clip((i - n_pre + 1) / (n_fade + 1.0), 0, 1).astype(np.float32)
    mix[n_pre + n_fade:] = 1
    fade = (mix > 0) & (mix < 1)
    assert fade.sum() == n_fade and np.all(np.diff(mix[fade]) > 0)
    ga, gb = src.frm_off[0] + pos_a.astype(int), src.frm_off[1] + pos_b.astype(int)
    assert np.all(s[llsm.A_F0][ga[fade]] > 0) and np.all(s[llsm.A_F0][gb[fade]] > 0)
    dst = llsm.Batch(ctx, ao, FS, [0], [F])
    dst.splice(src, pos_a, np.zeros(F, np.int32), np.ones(F, np.int32), pos_b, mix)
    ctx.sync()
    got = rows_of(dst)
    for aid in ROWS:
        assert beq(got[aid][mix == 0], s[aid][ga[mix == 0]]), aid
        assert beq(got[aid][mix == 1], s[aid][gb[mix == 1]]), aid
    dst.tolayer0(True); dst.phasepropagate(+1); dst.synthesize(so, seed=5)
    y = dst.download(llsm.A_Y).astype(np.float64)
    ctx.sync()
    dst.close(); src.close()
    assert y.size > 0 and np.all(np.isfinite(y))
    hop = ao.thop * FS
    level = lambda f0, f1: 10 * np.log10(np.mean(y[int(f0 * hop):int(f1 * hop)] ** 2))
    la, lf, lb = level(n_pre - n_fade, n_pre), level(n_pre, n_pre + n_fade), level(n_pre + n_fade, n_pre + 2 * n_fade)
    print("join levels (dB): side a %.2f, fade %.2f, side b %.2f" % (la, lf, lb))
    assert min(la, lb) - 3.0 <= lf <= max(la, lb) + 3.0, (la, lf, lb)


# ------------------------------------------------------------------ 9: refusals
def test_refusals_leave_dst_untouched(ctx, world):
    L = llsm.load()
    ao, src, rows = world
    F = int(DN.sum())
    rng = np.random.default_rng(91)
    dst, before = synthetic_src(ctx, ao, DN, 5)              # prefilled rows, layer 1 of src's size
    plain = new_dst(ctx, ao)                                 # no layer 1: a refused call must not enable it
    ua, pa = random_side(rng, SN, F)
    ub, pb = random_side(rng, SN, F)
    mix = rng.random(F).astype(np.float32)
    keep = []

    def call(d, s, **kw):
        m = llsm.SpliceMap()
        for name, dt in (("utt_a", np.int32), ("pos_a", np.float32), ("utt_b", np.int32), ("pos_b", np.float32),
                         ("mix", np.float32)):
            if kw.get(name) is not None:
                a = np.ascontiguousarray(kw[name], dt); keep.append(a)
                setattr(m, name, a.ctypes.data_as(llsm.P_int if dt == np.int32 else llsm.P_fp))
        rc = L.llsm_gpu_batch_splice(None if d is None else d.h, None if s is None else s.h,
                                     None if kw.get("no_map") else C.byref(m))
        return rc, L.llsm_gpu_last_error().decode()

    full = dict(utt_a=ua, pos_a=pa, utt_b=ub, pos_b=pb, mix=mix)
    at = lambda a, i, v: np.where(np.arange(F) == i, v, a)
    other_opt = new_dst(ctx, llsm.make_aoptions(f0_refine=0, npsd=128, maxnhar=77, nchannel=3, maxnhar_e=ao.maxnhar_e,
                                                chanfreq=[2000.0, 6000.0]))
    other_fs = llsm.Batch(ctx, ao, 22050.0, [0] * len(DN), DN)
    ctx2 = llsm.Context(0)
    other_ctx = llsm.Batch(ctx2, ao, FS, [0] * len(DN), DN)
    no_l1 = llsm.Batch(ctx, ao, FS, [0] * len(SN), SN)
    l1_other = new_dst(ctx, ao); l1_other.enable_layer1(2048)
    l1_before = rows_of(l1_other)
    more_utt = llsm.Batch(ctx, ao, FS, [0] * 8, [2] * 8)
    gap_sn = np.array([5, 0, 6], np.int32)
    gap_src, _ = synthetic_src(ctx, ao, gap_sn, 6)           # utterance 1 has no frames
    zeros_i, zeros_f = np.zeros(F, np.int32), np.zeros(F, np.float32)
    cases = {
        "NULL dst": (None, src, full), "NULL src": (dst, None, full), "NULL map": (dst, src, dict(no_map=True)),
        "pos_a NULL": (dst, src, dict(utt_a=ua)), "same batch": (src, src, dict(pos_a=np.zeros(int(SN.sum())))),
        "context": (other_ctx, src, full), "options": (other_opt, src, full), "sampling rate": (other_fs, src, full),
        "no layer 1": (dst, no_l1, full), "layer 1 of another size": (l1_other, src, full),
        "utt_a NULL, more utterances": (more_utt, src, dict(pos_a=np.zeros(16))),
        "utt_a < 0": (dst, src, dict(full, utt_a=at(ua, 7, -1))), "utt_a >= n": (dst, src, dict(full, utt_a=at(ua, 60, 7))),
        "utt_b >= n": (dst, src, dict(full, utt_b=at(ub, 33, 7))), "utt_b < 0": (dst, src, dict(full, utt_b=at(ub, 0, -3))),
        "empty utterance": (dst, gap_src, dict(utt_a=at(zeros_i, 9, 1), pos_a=zeros_f)),
        "empty utterance (b)": (dst, gap_src, dict(utt_a=zeros_i, pos_a=zeros_f, utt_b=at(zeros_i, 60, 1), pos_b=zeros_f,
                                                   mix=zeros_f)),
        "pos_a NaN": (dst, src, dict(full, pos_a=at(pa, 5, np.nan))), "pos_a < 0": (dst, src, dict(full, pos_a=at(pa, 0, -1e-3))),
        "pos_a > n - 1": (dst, src, dict(full, utt_a=at(ua, 44, 3), pos_a=at(pa, 44, 6.01))),
        "pos_a on a one-frame utterance": (dst, src, dict(full, utt_a=at(ua, 2, 1), pos_a=at(pa, 2, 0.5))),
        "pos_b NaN": (dst, src, dict(full, pos_b=at(pb, 59, np.nan))), "pos_b < 0": (dst, src, dict(full, pos_b=at(pb, 1, -2.0))),
        "pos_b > n - 1": (dst, src, dict(full, utt_b=at(ub, 12, 5), pos_b=at(pb, 12, 1.5))),
        "mix NaN": (dst, src, dict(full, mix=at(mix, 8, np.nan))), "mix < 0": (dst, src, dict(full, mix=at(mix, 60, -1e-6))),
        "mix > 1": (dst, src, dict(full, mix=at(mix, 0, 1.0001))),
        "no utt_b": (dst, src, dict(full, utt_b=None)), "no pos_b": (dst, src, dict(full, pos_b=None)),
        "no mix": (dst, src, dict(full, mix=None)), "only mix": (dst, src, dict(utt_a=ua, pos_a=pa, mix=mix)),
        "only utt_b": (dst, src, dict(utt_a=ua, pos_a=pa, utt_b=ub)), "only pos_b": (dst, src, dict(utt_a=ua, pos_a=pa, pos_b=pb)),
    }
    frame_named = {"utt_a < 0": 7, "utt_a >= n": 60, "utt_b >= n": 33, "utt_b < 0": 0, "empty utterance": 9,
                   "empty utterance (b)": 60, "pos_a NaN": 5, "pos_a < 0": 0, "pos_a > n - 1": 44,
                   "pos_a on a one-frame utterance": 2, "pos_b NaN": 59, "pos_b < 0": 1, "pos_b > n - 1": 12, "mix NaN": 8,
                   "mix < 0": 60, "mix > 1": 0}
    for name, (d, s, kw) in cases.items():
        rc, msg = call(d, s, **kw)
        assert rc == -1 and msg.startswith("llsm_gpu_batch_splice:"), (name, rc, msg)
        if name in frame_named:
            assert "[%d]" % frame_named[name] in msg, (name, msg)
    # the same refusals with a dst that has no layer 1: it is not enabled
    for name in ("pos_a NaN", "mix > 1", "no mix", "utt_b >= n"):
        rc, msg = call(plain, src, **cases[name][2])
        assert rc == -1 and msg.startswith("llsm_gpu_batch_splice:"), (name, rc, msg)
    ctx.sync()
    after = rows_of(dst)
    for aid in ROWS:
        assert beq(after[aid], before[aid]), aid
    assert plain.L.llsm_gpu_batch_array_bytes(plain.h, llsm.A_RD) == 0
    l1_after = rows_of(l1_other)
    for aid in ROWS:
        assert beq(l1_after[aid], l1_before[aid]), aid
    # a dst without frames is accepted; and the valid call goes through
    empty = llsm.Batch(ctx, ao, FS, [0, 0], [0, 0])
    rc, msg = call(empty, src, pos_a=np.zeros(1, np.float32))
    assert rc == 0, msg
    rc, msg = call(dst, src, **full)
    assert rc == 0, msg
    rc, msg = call(plain, src, **full)
    assert rc == 0, msg
    plain.nspec = src.nspec
    ctx.sync()
    a, b = rows_of(dst), rows_of(plain)
    assert_same(a, b, "prefilled and fresh dst")
    assert not beq(a[llsm.A_VTMAGN], before[llsm.A_VTMAGN])
    for x in (other_opt, other_fs, other_ctx, no_l1, l1_other, more_utt, gap_src, empty, plain, dst):
        x.close()
    ctx2.close()


# ------------------------------------------------------------------ 10: the C host
def test_c_host_joins_two_utterances_through_the_batch_api(tmp_path):
    """tests/c_host/splice_batch_host.c: a join with a cross-fade through llsm_gpu.h alone, built strictly as C99"""
    from test_c_host import INC, LIBDIR
    llsm.load()
    exe = str(tmp_path / "splice_batch_host")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + INC, "-o", exe,
                           os.path.join(HERE, "c_host", "splice_batch_host.c"),
                           "-L" + LIBDIR, "-l:libllsm2_amd.so", "-Wl,-rpath," + LIBDIR, "-lm"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "splice_batch ok" in out.stdout, out.stdout + out.stderr
