"""-m gpu: the frame coder on a device-resident batch (llsm_gpu_batch_enable_coder / _encode / _decode,
csrc/batch_coder.cpp) against the float64 oracle (oracle/coder_oracle.c) at the bounds of tests/test_gpu_coder.py,
against the host API (llsm_coder_encode_frames / _decode_frames) on the same frames, for invariance under batching, for
what it may write, and end to end on arctic_a0001.

Bounds (from tests/test_gpu_coder.py): head values exact, spectrum points <= 2e-4, band aperiodicities <= 1e-4, decoded
PSD and VTMAGN <= 0.02 dB, AMPL <= 1e-4 of the frame's maximum, PHSE and VSPHSE <= 1e-3 rad; bins whose float64
aperiodicity lies within 1e-4 of 1 are left out of the VTMAGN comparison and frames with such a bin (3e-4) below their top
harmonic out of the layer-0 phase comparison, except inside runs of exact ones.  The exclusions are capped per case
(CAPS).  Batch against host API: both are float32 and each lies within the bound of the oracle, so twice the bound is
asserted whatever kernels the two sides run, and the measured values are reported (0 while they share their kernels).

The batch's rows are as wide as the largest harmonic count the vectors decode to (WIDE harmonics), so that the cap of nhar
at the batch's maxnhar -- the one documented difference from the host decoder -- does not enter the comparison."""
import ctypes as C
import os

import numpy as np
import pytest

import libllsm2_amd as llsm
from conftest import make_speechlike, wrap
from gpu_common import oracle_analyze, params_to_gpu_rows, report
from test_gpu_coder import CODER_CASES, coder_lib
from test_gpu_l1 import l1_chunk_from_oracle, l1_rows, q32
from verify_utils import GOLDEN, data_distribution_klds, read_wav

pytestmark = pytest.mark.gpu
A = llsm
WIDE = 320
BOUND = dict(spec=2e-4, bap=1e-4, psd_db=0.02, vtmagn_db=0.02, ampl_over_max=1e-4, phse_rad=1e-3, vsphse_rad=1e-3)
# case: (largest share of vocal-tract bins left out, voiced frames that may be left out of the layer-0 phase check (None: any),
#        voiced frames that must remain in it)
CAPS = {"16k_low_order": (1e-3, 0, 1), "22k_hop128": (1e-3, 0, 1), "default": (2e-3, None, 30)}
PARAM = (A.A_F0, A.A_NHAR, A.A_AMPL, A.A_PHSE, A.A_PSD, A.A_PSDRES, A.A_HAS_PSDRES, A.A_EDC, A.A_NHAR_E, A.A_EENV_AMPL, A.A_EENV_PHSE)
L1 = (A.A_RD, A.A_VTMAGN, A.A_VSPHSE, A.A_NVSPHSE, A.A_PBPSYN, A.A_HAS_HM)
ROWS = PARAM + L1
SIGNALS = (A.A_X, A.A_XRES, A.A_WHITE, A.A_Y, A.A_YSIN, A.A_YNOISE)


@pytest.fixture(scope="module")
def ctx():
    c = llsm.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def L():
    return coder_lib()


def beq(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def widen(a, n):
    out = np.zeros((a.shape[0], n), a.dtype)
    out[:, :a.shape[1]] = a
    return out


_cases = {}


def case_rows(o64, cid):
    """oracle rows of one case, widened to WIDE harmonics: (fs, nfft, orders, wide options, Params, L1Params, rows)"""
    if cid not in _cases:
        FS, thop, nfft, osp, obap, kw, useed = CODER_CASES[cid]
        x, f0 = make_speechlike(useed, nx=int(0.45 * FS), fs=FS, thop=thop)
        ao = llsm.make_aoptions(f0_refine=0, thop=thop, **kw)
        pr, _ = oracle_analyze(o64, ao, FS, x, f0.astype(np.float32))
        pr = pr.astype(np.float32).astype(np.float64)
        q = q32(o64.chunk_tolayer1(pr, nfft))
        rows = dict(params_to_gpu_rows(pr)); rows.update(l1_rows(q))
        for aid in (A.A_AMPL, A.A_PHSE, A.A_VSPHSE):
            rows[aid] = widen(rows[aid], WIDE)
        wide = llsm.make_aoptions(f0_refine=0, thop=thop, **dict(kw, maxnhar=WIDE))
        _cases[cid] = (FS, nfft, osp, obap, ao, wide, pr, q, rows)
    return _cases[cid]


def make_batch(ctx, wide, FS, nfft, rows, pieces):
    """a batch whose utterances are the frame ranges `pieces` of the rows; returns (batch, frame index of every row)"""
    idx = np.concatenate([np.arange(a, b) for a, b in pieces])
    b = llsm.Batch(ctx, wide, FS, [0] * len(pieces), [e - s for s, e in pieces])
    b.enable_layer1(nfft)
    for aid in ROWS:
        b.upload(aid, rows[aid][idx])
    return b, idx


def all_arrays(b):
    ids = [a for a in range(A.A_NARRAYS) if b.L.llsm_gpu_batch_array_bytes(b.h, a) > 0]
    return {a: b.download(a) for a in ids}


def assert_same(before, after, but=(), where=""):
    assert set(before) == set(after), where
    for a in before:
        if a not in but:
            assert beq(before[a], after[a]), (where, "array", a)


def decoded_metrics(got, po, qo, margin, inner, use_l1, FS, ns):
    """rows `got` (dict of arrays over the same frames as the oracle's po / qo) against the oracle, with the exclusions of
    tests/test_gpu_coder.py; the integer rows, flags and F0 are asserted equal here"""
    n_frm = len(po.f0)
    m = dict(psd_db=float(np.abs(got[A.A_PSD] - po.psd).max()))
    assert np.array_equal(got[A.A_F0], po.f0.astype(np.float32))
    da = dp = dv = ds = 0.0; n_ill = n_voiced = bins_ill = bins_all = 0
    for i in range(n_frm):
        if use_l1:
            n = int(qo.nvsphse[i])
            assert got[A.A_NVSPHSE][i] == n and got[A.A_NHAR][i] == 0 and got[A.A_HAS_HM][i] == (0 if n else 1), i
            if n:
                g = got[A.A_VTMAGN][i].astype(np.float64); o = qo.vtmagn[i]
                assert not np.isnan(g).any() and not np.isposinf(g).any(), i
                assert np.all(np.isneginf(g[inner[i]])) and np.all(np.isneginf(o[inner[i]])), i
                mg = margin[i].copy(); mg[0] = mg[1]
                well = mg >= 1e-4
                bins_ill += int(np.count_nonzero(~well & ~inner[i])); bins_all += ns
                assert np.all(np.isfinite(g[well])), i
                dv = max(dv, np.abs(g[well] - o[well]).max())
                ds = max(ds, np.abs(wrap(got[A.A_VSPHSE][i, :n] - qo.vsphse[i, :n])).max())
                assert not got[A.A_VSPHSE][i, n:].any(), i
        else:
            n = int(po.nhar[i])
            assert got[A.A_NHAR][i] == n and got[A.A_NVSPHSE][i] == 0 and got[A.A_HAS_HM][i] == 1, i
            assert not got[A.A_AMPL][i, n:].any() and not got[A.A_PHSE][i, n:].any(), i
            if n:
                a = got[A.A_AMPL][i, :n]; p = got[A.A_PHSE][i, :n]
                da = max(da, (np.abs(a - po.ampl[i, :n]) / po.ampl[i, :n].max()).max())
                e = np.abs(wrap(p - po.phse[i, :n]))
                big = po.ampl[i, :n] > 1e-4 * po.ampl[i, :n].max()
                jtop = min(int(np.ceil(n * po.f0[i] / (FS / 2) * (ns - 1))) + 1, ns)
                ill = bool(np.any((margin[i, :jtop] < 3e-4) & ~inner[i, :jtop]))
                n_voiced += 1; n_ill += ill
                if not ill:
                    dp = max(dp, e[big].max())
    if use_l1:
        m.update(vtmagn_db=float(dv), vsphse_rad=float(ds), bins_left_out=bins_ill, bins=bins_all)
    else:
        m.update(ampl_over_max=float(da), phse_rad=float(dp), frames_left_out=n_ill, frames_voiced=n_voiced)
    return m


def host_decoded_rows(L, coder, e32, use_l1, ns, npsd, nch):
    """llsm_coder_decode_frames on the vectors, its frames read into rows WIDE harmonics wide, plus the members the
    decoder leaves at their llsm_create_frame values"""
    n = len(e32)
    out = (C.POINTER(llsm.Container) * n)()
    assert L.llsm_coder_decode_frames(coder, e32.ctypes.data_as(llsm.P_fp), n, use_l1, out) == 0
    r = {A.A_F0: np.zeros(n, np.float32), A.A_RD: np.zeros(n, np.float32), A.A_NHAR: np.zeros(n, np.int32),
         A.A_NVSPHSE: np.zeros(n, np.int32), A.A_HAS_HM: np.zeros(n, np.int32), A.A_PSD: np.zeros((n, npsd), np.float32),
         A.A_AMPL: np.zeros((n, WIDE), np.float32), A.A_PHSE: np.zeros((n, WIDE), np.float32),
         A.A_VSPHSE: np.zeros((n, WIDE), np.float32), A.A_VTMAGN: np.zeros((n, ns), np.float32),
         A.A_EDC: np.zeros((n, nch), np.float32), A.A_NHAR_E: np.zeros(n, np.int32), A.A_HAS_PSDRES: np.zeros(n, np.int32),
         A.A_PBPSYN: np.zeros(n, np.int32)}
    eenv_zero = True
    for i in range(n):
        fr = out[i]
        nm = C.cast(L.llsm_container_get(fr, llsm.FRAME_NM), C.POINTER(llsm.NMFrame)).contents
        r[A.A_PSD][i] = np.ctypeslib.as_array(nm.psd, (nm.npsd,))
        r[A.A_EDC][i] = np.ctypeslib.as_array(nm.edc, (nm.nchannel,))
        ne = 0
        for c in range(nm.nchannel):
            e = nm.eenv[c].contents
            ne = max(ne, e.nhar)
            if e.nhar:
                eenv_zero &= not np.ctypeslib.as_array(e.ampl, (e.nhar,)).any() and not np.ctypeslib.as_array(e.phse, (e.nhar,)).any()
        r[A.A_NHAR_E][i] = ne
        r[A.A_HAS_PSDRES][i] = bool(L.llsm_container_get(fr, llsm.FRAME_PSDRES))
        r[A.A_PBPSYN][i] = bool(L.llsm_container_get(fr, llsm.FRAME_PBPSYN))
        r[A.A_F0][i] = C.cast(L.llsm_container_get(fr, llsm.FRAME_F0), llsm.P_fp)[0]
        r[A.A_RD][i] = C.cast(L.llsm_container_get(fr, llsm.FRAME_RD), llsm.P_fp)[0]
        hm = C.cast(L.llsm_container_get(fr, llsm.FRAME_HM), C.POINTER(llsm.HMFrame))
        r[A.A_HAS_HM][i] = bool(hm)
        if bool(hm) and hm.contents.nhar:
            k = hm.contents.nhar
            assert k <= WIDE, (i, k)
            r[A.A_NHAR][i] = k
            r[A.A_AMPL][i, :k] = np.ctypeslib.as_array(hm.contents.ampl, (k,)); r[A.A_PHSE][i, :k] = np.ctypeslib.as_array(hm.contents.phse, (k,))
        vs = C.cast(L.llsm_container_get(fr, llsm.FRAME_VSPHSE), llsm.P_fp)
        if bool(vs):
            k = L.llsm_fparray_length(vs)
            assert k <= WIDE, (i, k)
            r[A.A_NVSPHSE][i] = k
            r[A.A_VSPHSE][i, :k] = np.ctypeslib.as_array(vs, (k,))
            r[A.A_VTMAGN][i] = np.ctypeslib.as_array(C.cast(L.llsm_container_get(fr, llsm.FRAME_VTMAGN), llsm.P_fp), (ns,))
        L.llsm_delete_container(fr)
    assert eenv_zero
    return r


@pytest.mark.parametrize("cid", ["16k_low_order", "22k_hop128", "default"])
def test_parity_with_the_oracle_and_agreement_with_the_host_api(ctx, L, o64, cid):
    FS, nfft, osp, obap, ao, wide, pr, q, rows = case_rows(o64, cid)
    ns, dim, nfrm = nfft // 2 + 1, 3 + osp + obap, pr.nfrm
    # three utterances of different lengths in one batch: tiles of 16 frames straddle their boundaries
    pieces = [(0, nfrm), (0, 23), (10, 51)]
    b, idx = make_batch(ctx, wide, FS, nfft, rows, pieces)
    F = len(idx)
    b.enable_coder(osp, obap)
    assert b.coder_dimension == dim and b.L.llsm_gpu_batch_array_bytes(b.h, A.A_CODE) == F * dim * 4
    b.encode(); ctx.sync()
    enc = b.download(A.A_CODE)
    enco = o64.coder_encode_chunk(pr, q, osp, obap)
    m = dict(enc_head=float(np.abs(enc[:, :3] - enco[idx, :3]).max()), enc_spec=float(np.abs(enc[:, 3:3 + osp] - enco[idx, 3:3 + osp]).max()),
             enc_bap=float(np.abs(enc[:, 3 + osp:] - enco[idx, 3 + osp:]).max()))
    # the host API on the same frames
    ch = l1_chunk_from_oracle(L, ao, pr, q, FS, nfft=nfft)
    coder = L.llsm_create_coder(ch.contents.conf, osp, obap)
    assert coder
    ench = np.zeros((nfrm, dim), np.float32)
    assert L.llsm_coder_encode_frames(coder, ch.contents.frames, nfrm, ench.ctypes.data_as(llsm.P_fp)) == 0
    assert beq(enc[:, :3], ench[idx, :3])
    m["host_enc_spec"] = float(np.abs(enc[:, 3:3 + osp] - ench[idx, 3:3 + osp]).max())
    m["host_enc_bap"] = float(np.abs(enc[:, 3 + osp:] - ench[idx, 3 + osp:]).max())
    # decode the ORACLE's vectors on every side
    e32 = np.ascontiguousarray(enco.astype(np.float32))
    margin = 1.0 - o64.coder_aperiodicity_chunk(e32.astype(np.float64), pr, ns, ao.lip_radius, osp, obap)
    zero = margin == 0
    inner = zero & np.hstack([zero[:, :1], zero[:, :-1]]) & np.hstack([zero[:, 1:], zero[:, -1:]])
    me = max(ao.maxnhar_e, 1)
    for use_l1 in (1, 0):
        b.upload(A.A_CODE, e32[idx])
        prev = {aid: b.download(aid) for aid in ROWS}
        b.decode(use_l1); ctx.sync()
        got = {aid: b.download(aid) for aid in ROWS}
        po, qo = o64.coder_decode_chunk(e32.astype(np.float64), bool(use_l1), pr, ns, ao.lip_radius, osp, obap, WIDE)
        first = {aid: got[aid][:nfrm] for aid in ROWS}                 # utterance 0 is the whole oracle utterance
        mo = decoded_metrics(first, po, qo, margin, inner, use_l1, FS, ns)
        m.update({f"dec{use_l1}_{k}": v for k, v in mo.items()})
        assert np.abs(got[A.A_RD][:nfrm] - q32_rd(qo.rd)).max() == 0
        # ... and the host decoder: integer rows, flags, F0 and the rows it leaves at their defaults bit for bit
        h = host_decoded_rows(L, coder, e32, use_l1, ns, ao.npsd, ao.nchannel)
        for aid in (A.A_F0, A.A_RD, A.A_NHAR, A.A_NVSPHSE, A.A_HAS_HM, A.A_EDC, A.A_NHAR_E, A.A_HAS_PSDRES, A.A_PBPSYN):
            assert beq(got[aid], h[aid][idx]), (use_l1, aid)
        assert not got[A.A_EENV_AMPL].any() and not got[A.A_EENV_PHSE].any()
        assert got[A.A_EENV_AMPL].shape == (F, ao.nchannel, me)
        assert beq(got[A.A_PSDRES], prev[A.A_PSDRES])                 # not written
        m[f"host_dec{use_l1}_psd_db"] = float(np.abs(got[A.A_PSD] - h[A.A_PSD][idx]).max())
        if use_l1:
            v = h[A.A_NVSPHSE][idx] > 0
            mg = margin[idx].copy(); mg[:, 0] = mg[:, 1]
            well = (mg >= 1e-4) & v[:, None]
            with np.errstate(invalid="ignore"):                            # (-inf - -inf outside `well`)
                m["host_dec1_vtmagn_db"] = float(np.abs(got[A.A_VTMAGN].astype(np.float64) - h[A.A_VTMAGN][idx])[well].max())
            m["host_dec1_vsphse_rad"] = float(np.abs(wrap(got[A.A_VSPHSE].astype(np.float64) - h[A.A_VSPHSE][idx]))[v].max())
            assert beq(got[A.A_AMPL], prev[A.A_AMPL]) and beq(got[A.A_PHSE], prev[A.A_PHSE])      # not written
            u = ~v
            assert beq(got[A.A_VTMAGN][u], prev[A.A_VTMAGN][u]) and beq(got[A.A_VSPHSE][u], prev[A.A_VSPHSE][u])
        else:
            ha, hp = h[A.A_AMPL][idx].astype(np.float64), h[A.A_PHSE][idx].astype(np.float64)
            amax = np.maximum(ha.max(axis=1, keepdims=True), 1e-30)
            m["host_dec0_ampl_over_max"] = float((np.abs(got[A.A_AMPL] - ha) / amax).max())
            jtop = np.minimum(np.ceil(h[A.A_NHAR][idx] * h[A.A_F0][idx].astype(np.float64) / (FS / 2) * (ns - 1)).astype(int) + 1, ns)
            col = np.arange(ns)[None, :]
            ill = np.any((margin[idx] < 3e-4) & ~inner[idx] & (col < jtop[:, None]), axis=1)
            big = (ha > 1e-4 * amax) & ~ill[:, None]
            m["host_dec0_phse_rad"] = float(np.abs(wrap(got[A.A_PHSE] - hp))[big].max())
            assert beq(got[A.A_VTMAGN], prev[A.A_VTMAGN]) and beq(got[A.A_VSPHSE], prev[A.A_VSPHSE])  # not written
    report("batch_coder_" + cid, m)
    L.llsm_delete_coder(coder); L.llsm_delete_chunk(ch); b.close()
    # the exclusions cannot hide a failure
    share, max_out, min_left = CAPS[cid]
    assert m["dec1_bins_left_out"] <= share * m["dec1_bins"], m
    if max_out is not None:
        assert m["dec0_frames_left_out"] <= max_out, m
    assert m["dec0_frames_voiced"] - m["dec0_frames_left_out"] >= min_left, m
    # item 1: the oracle, at the existing bounds
    assert m["enc_head"] == 0 and m["enc_spec"] <= BOUND["spec"] and m["enc_bap"] <= BOUND["bap"], m
    assert m["dec0_psd_db"] <= BOUND["psd_db"] and m["dec1_psd_db"] <= BOUND["psd_db"], m
    assert m["dec0_ampl_over_max"] <= BOUND["ampl_over_max"] and m["dec0_phse_rad"] <= BOUND["phse_rad"], m
    assert m["dec1_vtmagn_db"] <= BOUND["vtmagn_db"] and m["dec1_vsphse_rad"] <= BOUND["vsphse_rad"], m
    # item 2: the host API, within twice those bounds
    assert m["host_enc_spec"] <= 2 * BOUND["spec"] and m["host_enc_bap"] <= 2 * BOUND["bap"], m
    assert m["host_dec0_psd_db"] <= 2 * BOUND["psd_db"] and m["host_dec1_psd_db"] <= 2 * BOUND["psd_db"], m
    assert m["host_dec1_vtmagn_db"] <= 2 * BOUND["vtmagn_db"] and m["host_dec1_vsphse_rad"] <= 2 * BOUND["vsphse_rad"], m
    assert m["host_dec0_ampl_over_max"] <= 2 * BOUND["ampl_over_max"] and m["host_dec0_phse_rad"] <= 2 * BOUND["phse_rad"], m


def q32_rd(rd):
    return rd.astype(np.float32)


def coded(ctx, wide, FS, nfft, rows, pieces, osp, obap):
    """encode, then decode(1) and decode(0) of the batch's own vectors; returns per utterance (code, rows after decode(1),
    rows after decode(0))"""
    b, _ = make_batch(ctx, wide, FS, nfft, rows, pieces)
    b.enable_coder(osp, obap)
    b.encode()
    code = b.download(A.A_CODE)
    b.decode(1); r1 = {aid: b.download(aid) for aid in ROWS}
    b.decode(0); r0 = {aid: b.download(aid) for aid in ROWS}
    off = b.frm_off
    b.close()
    return [(code[off[u]:off[u + 1]], {k: v[off[u]:off[u + 1]] for k, v in r1.items()}, {k: v[off[u]:off[u + 1]] for k, v in r0.items()})
            for u in range(len(pieces))]


@pytest.mark.parametrize("extra", [0, 5])
def test_an_utterance_has_the_bits_it_has_alone(ctx, o64, extra):
    """alone, and as utterance 17 of 64 of mixed lengths (frame total a multiple of 16, and with `extra` frames more)"""
    FS, nfft, osp, obap, ao, wide, pr, q, rows = case_rows(o64, "default")
    nfrm = pr.nfrm
    rng = np.random.default_rng(3)
    me = (7, 44)                                            # 37 frames, voiced and unvoiced
    assert np.count_nonzero(rows[A.A_F0][me[0]:me[1]] > 0) >= 8 and np.count_nonzero(rows[A.A_F0][me[0]:me[1]] == 0) >= 1
    pieces = []
    for u in range(64):
        n = int(rng.integers(1, 40)); s = int(rng.integers(0, nfrm - n))
        pieces.append((s, s + n))
    pieces[17] = me
    total = sum(e - s for s, e in pieces)
    s, e = pieces[63]
    pieces[63] = (0, (e - s) + (-total) % 16 + extra)
    assert sum(e - s for s, e in pieces) % 16 == extra and sum(e - s for s, e in pieces[:17]) % 16 != 0
    alone = coded(ctx, wide, FS, nfft, rows, [me], osp, obap)[0]
    among = coded(ctx, wide, FS, nfft, rows, pieces, osp, obap)[17]
    assert beq(alone[0], among[0])
    for k in (1, 2):
        for aid in ROWS:
            assert beq(alone[k][aid], among[k][aid]), (k, aid)
    assert np.count_nonzero(alone[0][:, 3:]) > 0 and np.count_nonzero(alone[1][A.A_NVSPHSE]) >= 8


def test_nothing_else_is_written_and_refusals_write_nothing(ctx, o64):
    FS, nfft, osp, obap, ao, wide, pr, q, rows = case_rows(o64, "default")
    Lb = llsm.load()
    x = np.random.default_rng(5).standard_normal(3000).astype(np.float32)
    idx = np.r_[np.arange(0, 30), np.arange(20, 41)]

    def fresh(l1=True):
        b = llsm.Batch(ctx, wide, FS, [2000, 1000], [30, 21])
        b.upload(A.A_X, x)
        for aid in PARAM:
            b.upload(aid, rows[aid][idx])
        if l1:
            b.enable_layer1(nfft)
            for aid in L1:
                b.upload(aid, rows[aid][idx])
        b.synthesize(llsm.make_soptions(FS), seed=3); ctx.sync()        # outputs and templates hold something
        return b

    def refused(b, fn, args, needle, before):
        rc = getattr(Lb, fn)(b.h, *args)
        msg = Lb.llsm_gpu_last_error().decode()
        assert rc == -1 and msg.startswith(fn + ":") and needle in msg, (fn, args, rc, msg)
        ctx.sync()
        assert_same(before, all_arrays(b), where=fn + repr(args))

    # no layer 1
    b = fresh(l1=False); before = all_arrays(b)
    refused(b, "llsm_gpu_batch_enable_coder", (osp, obap), "layer 1", before)
    refused(b, "llsm_gpu_batch_encode", (), "layer 1", before)
    refused(b, "llsm_gpu_batch_decode", (1,), "layer 1", before)
    assert b.coder_dimension == 0
    b.close()
    # coder not enabled; orders out of range
    b = fresh(); before = all_arrays(b)
    assert A.A_CODE not in before
    refused(b, "llsm_gpu_batch_encode", (), "not enabled", before)
    refused(b, "llsm_gpu_batch_decode", (0,), "not enabled", before)
    for o in ((0, obap), (nfft // 2 + 1, obap), (osp, 0), (-3, 2)):
        refused(b, "llsm_gpu_batch_enable_coder", o, "out of range", before)
    assert b.coder_dimension == 0
    # enabled: encode writes LLSM_GPU_CODE alone
    b.enable_coder(osp, obap); ctx.sync()
    before = all_arrays(b)
    assert A.A_CODE in before and not before[A.A_CODE].any()
    b.encode(); ctx.sync()
    after = all_arrays(b)
    assert_same(before, after, but=(A.A_CODE,), where="encode")
    assert np.count_nonzero(after[A.A_CODE][:, 3:]) > 0
    # the same orders again do nothing; refusals leave the vectors too
    ptr = b.device_ptr(A.A_CODE)
    b.enable_coder(osp, obap)
    assert b.device_ptr(A.A_CODE) == ptr
    before = all_arrays(b)
    for o in ((0, obap), (nfft // 2 + 1, obap), (osp, 0)):
        refused(b, "llsm_gpu_batch_enable_coder", o, "out of range", before)
    for bad in (2, -1, 7):
        refused(b, "llsm_gpu_batch_decode", (bad,), "not 0 or 1", before)
    assert b.coder_dimension == 3 + osp + obap
    # decode leaves the signals, PSDRES and the vectors
    for use_l1 in (1, 0):
        b.decode(use_l1); ctx.sync()
        after = all_arrays(b)
        for aid in SIGNALS + (A.A_PSDRES, A.A_CODE):
            assert beq(before[aid], after[aid]), (use_l1, aid)
        assert not beq(before[A.A_PSD], after[A.A_PSD])
    # other orders reallocate the array
    b.enable_coder(24, 3); ctx.sync()
    assert b.coder_dimension == 30 and b.download(A.A_CODE).shape == (51, 30)
    b.close()
    # rows too long for the kernel's LDS: the minimum-phase transform of 4096 harmonics beside three rows of 4097 bins
    big = llsm.make_aoptions(f0_refine=0, maxnhar=4096)
    b = llsm.Batch(ctx, big, FS, [0], [20]); b.enable_layer1(8192); b.enable_coder(64, 5); ctx.sync()
    before = all_arrays(b)
    refused(b, "llsm_gpu_batch_decode", (0,), "LDS", before)
    assert "163840" in Lb.llsm_gpu_last_error().decode()
    b.close()


def test_after_a_decode_the_lowest_f0_is_unknown_and_synthesis_still_agrees(ctx, o64):
    """decode writes the F0 row on the device: provisions sized by the lowest F0 must behave as after a partial upload.  The
    same rows uploaded whole (lowest F0 known) and produced by decode (unknown) synthesise the same samples."""
    FS, nfft, osp, obap, ao, wide, pr, q, rows = case_rows(o64, "default")
    so = llsm.make_soptions(FS)
    b, _ = make_batch(ctx, wide, FS, nfft, rows, [(0, pr.nfrm)])
    b.enable_coder(osp, obap); b.encode(); b.decode(0)
    got = {aid: b.download(aid) for aid in ROWS}
    b.synthesize(so, seed=11); y1 = b.download(A.A_Y); ctx.sync(); b.close()
    c = llsm.Batch(ctx, wide, FS, [0], [pr.nfrm]); c.enable_layer1(nfft)
    for aid in ROWS:
        c.upload(aid, got[aid])
    c.synthesize(so, seed=11); y2 = c.download(A.A_Y); ctx.sync(); c.close()
    assert np.isfinite(y1).all() and float(np.abs(y1).max()) > 0
    assert float(np.abs(y1 - y2).max()) <= 1e-4 * float(np.abs(y2).max())


def test_end_to_end_on_arctic(ctx, L):
    """analyse -> tolayer1(2048) -> encode(64, 5) -> decode -> (tolayer0) -> phasepropagate(+1) -> synthesise, as
    test_coder_acceptance_through_the_chunk_api does through chunks: KLD < 0.05 against the input, and the vectors are the
    host path's within twice the oracle bounds"""
    x, fs = read_wav(os.path.join(GOLDEN, "arctic_a0001.wav"))
    f0 = np.load(os.path.join(GOLDEN, "arctic_a0001_f0_hop128.npy")).astype(np.float32)
    nfrm = len(f0)
    ao = llsm.make_aoptions(thop=128.0 / fs, f0_refine=0)
    so = llsm.make_soptions(fs)
    b = llsm.Batch(ctx, ao, fs, [len(x)], [nfrm])
    b.upload(A.A_X, x); b.upload(A.A_F0, f0)
    b.analyze(); b.tolayer1(2048)
    b.enable_coder(64, 5); b.encode(); ctx.sync()
    enc = b.download(A.A_CODE)
    rep = {}
    for use_l1 in (1, 0):
        b.decode(use_l1)
        if use_l1:
            b.tolayer0(True)
        b.phasepropagate(+1); b.synthesize(so, seed=7)
        y = b.download(A.A_Y); ctx.sync()
        klds = data_distribution_klds(x, y)
        rep[f"layer{use_l1}"] = klds
        assert all(k < 0.05 for k in klds), (use_l1, klds)
        assert beq(b.download(A.A_CODE), enc)
    b.close()
    # the host path's vectors
    ch = L.llsm_analyze(C.byref(ao), x.ctypes.data_as(llsm.P_fp), len(x), fs, f0.ctypes.data_as(llsm.P_fp), nfrm, None)
    assert bool(ch), L.llsm_gpu_last_error()
    L.llsm_chunk_tolayer1(ch, 2048)
    coder = L.llsm_create_coder(ch.contents.conf, 64, 5)
    ench = np.zeros((nfrm, 72), np.float32)
    assert L.llsm_coder_encode_frames(coder, ch.contents.frames, nfrm, ench.ctypes.data_as(llsm.P_fp)) == 0
    L.llsm_delete_coder(coder); L.llsm_delete_chunk(ch)
    rep["vectors_head_equal"] = bool(beq(enc[:, :3], ench[:, :3]))
    rep["vectors_spec"] = float(np.abs(enc[:, 3:67] - ench[:, 3:67]).max()); rep["vectors_bap"] = float(np.abs(enc[:, 67:] - ench[:, 67:]).max())
    report("batch_coder_acceptance", rep)
    assert rep["vectors_head_equal"] and rep["vectors_spec"] <= 2 * BOUND["spec"] and rep["vectors_bap"] <= 2 * BOUND["bap"], rep
