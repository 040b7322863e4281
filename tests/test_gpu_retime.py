"""-m gpu: edits of a device-resident batch -- llsm_gpu_batch_phasesync_rps, llsm_gpu_batch_phasepropagate and
llsm_gpu_batch_retime (the middle of the reference's time-stretch recipe, test/demo-stretch.c) -- against the host's
chunk functions (phase operations: bit-identical) and against a numpy restatement of the retime rules of llsm_gpu.h
written here (lin rows and integer rows bit-identical; fades within 1e-4 dB; circular blends compared as complex numbers,
|v| |e^{j phi_gpu} - e^{j phi_ref}| <= 2e-6 with v the blended vector)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import libllsm2_amd as llsm
from conftest import FS, make_speechlike
from gpu_common import rel_rms, report
from verify_utils import GOLDEN, read_wav

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NFFT = 2048
PARAM = llsm.Batch.PARAM_IDS
L1 = llsm.Batch.L1_IDS
ROWS = PARAM + L1
INT = {llsm.A_NHAR, llsm.A_NHAR_E, llsm.A_HAS_PSDRES, llsm.A_NVSPHSE, llsm.A_PBPSYN, llsm.A_HAS_HM}


@pytest.fixture(scope="module")
def ctx():
    c = llsm.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def beq(a, b):
    return np.array_equal(bits(a), bits(b))


def rows_of(b, l1=True):
    return {aid: b.download(aid) for aid in (ROWS if l1 else PARAM)}


def analysed(ctx, n_utt=4, nx=30000, l1=True, ao=None):
    ao = ao or llsm.make_aoptions(f0_refine=0)
    xs, f0s = zip(*[make_speechlike(u, nx=nx) for u in range(n_utt)])
    b = llsm.Batch(ctx, ao, FS, [len(x) for x in xs], [len(f) for f in f0s])
    b.upload(llsm.A_X, np.concatenate(xs)); b.upload(llsm.A_F0, np.concatenate(f0s))
    b.analyze()
    if l1:
        b.tolayer1(NFFT)
    ctx.sync()
    return b, ao


# ------------------------------------------------------------------ host reference of the phase operations
def host_chunk(L, ao, fs, rows, g0, n, l1):
    """rows [g0, g0 + n) -> a product llsm_chunk (llsm_flat_to_chunk / llsm_flat_l1_to_chunk; HAS_HM = 0 frames lose HM)"""
    conf = L.llsm_aoptions_toconf(C.byref(ao), fs / 2.0)
    C.cast(L.llsm_container_get(conf, llsm.CONF_NFRM), llsm.P_int)[0] = n
    ch = L.llsm_create_chunk(conf, 1)
    L.llsm_delete_container(conf)
    sl = {aid: np.ascontiguousarray(a[g0:g0 + n]) for aid, a in rows.items()}
    v = flat_view(sl)
    assert L.llsm_flat_to_chunk(C.byref(v), 0, ch) == 0
    if l1:
        sl["has_rd"] = np.ones(n, np.int32)
        w = flat_l1_view(sl)
        assert L.llsm_flat_l1_to_chunk(C.byref(w), 0, ch) == 0
        for i in np.flatnonzero(sl[llsm.A_HAS_HM] == 0):
            L.llsm_container_attach_(ch.contents.frames[int(i)], llsm.FRAME_HM, None, None, None)
    return ch, sl


def flat_view(a):
    v = llsm.FlatParams()
    v.maxnhar, v.maxnhar_e, v.npsd, v.nchannel = a[llsm.A_AMPL].shape[1], a[llsm.A_EENV_AMPL].shape[2], \
        a[llsm.A_PSD].shape[1], a[llsm.A_EDC].shape[1]
    fp = lambda k: a[k].ctypes.data_as(llsm.P_fp)
    ip = lambda k: a[k].ctypes.data_as(llsm.P_int)
    v.f0, v.nhar, v.ampl, v.phse, v.psd, v.psdres = fp(llsm.A_F0), ip(llsm.A_NHAR), fp(llsm.A_AMPL), fp(llsm.A_PHSE), \
        fp(llsm.A_PSD), fp(llsm.A_PSDRES)
    v.has_psdres, v.edc, v.nhar_e = ip(llsm.A_HAS_PSDRES), fp(llsm.A_EDC), ip(llsm.A_NHAR_E)
    v.eenv_ampl, v.eenv_phse = fp(llsm.A_EENV_AMPL), fp(llsm.A_EENV_PHSE)
    return v


def flat_l1_view(a):
    w = llsm.FlatL1()
    w.nspec, w.maxnhar = a[llsm.A_VTMAGN].shape[1], a[llsm.A_VSPHSE].shape[1]
    w.rd, w.has_rd = a[llsm.A_RD].ctypes.data_as(llsm.P_fp), a["has_rd"].ctypes.data_as(llsm.P_int)
    w.vtmagn, w.vsphse = a[llsm.A_VTMAGN].ctypes.data_as(llsm.P_fp), a[llsm.A_VSPHSE].ctypes.data_as(llsm.P_fp)
    w.nvsphse, w.pbpsyn = a[llsm.A_NVSPHSE].ctypes.data_as(llsm.P_int), a[llsm.A_PBPSYN].ctypes.data_as(llsm.P_int)
    w.has_hm = a[llsm.A_HAS_HM].ctypes.data_as(llsm.P_int)
    return w


def chunk_rows(L, ch, like, l1):
    out = {aid: np.zeros_like(a) for aid, a in like.items()}
    assert L.llsm_chunk_to_flat(ch, C.byref(flat_view(out)), 0) == 0
    if l1:
        out["has_rd"] = np.zeros(len(out[llsm.A_F0]), np.int32)
        assert L.llsm_chunk_to_flat_l1(ch, C.byref(flat_l1_view(out)), 0) == 0
    return out


def phase_masks(r, l1):
    """entries a phase shift touches: PHSE / EENV_PHSE of voiced frames (PHSE only where HM is valid), VSPHSE"""
    mh, (nch, me) = r[llsm.A_PHSE].shape[1], r[llsm.A_EENV_PHSE].shape[1:]
    voiced = r[llsm.A_F0] != 0
    hm = voiced & ((r[llsm.A_HAS_HM] != 0) if l1 else True)
    nh = np.where(hm, np.clip(r[llsm.A_NHAR], 0, mh), 0)
    ne = np.where(voiced, np.clip(r[llsm.A_NHAR_E], 0, me), 0)
    m = {llsm.A_PHSE: np.arange(mh)[None, :] < nh[:, None],
         llsm.A_EENV_PHSE: np.broadcast_to(np.arange(me)[None, None, :] < ne[:, None, None], r[llsm.A_EENV_PHSE].shape)}
    if l1:
        m[llsm.A_VSPHSE] = np.arange(mh)[None, :] < np.clip(r[llsm.A_NVSPHSE], 0, mh)[:, None]
    return m


@pytest.mark.parametrize("l1", [False, True])
@pytest.mark.parametrize("op", ["sync0", "sync1", "prop+1", "prop-1"])
def test_phase_operations_are_bit_identical_to_the_host(ctx, l1, op):
    L = llsm.load()
    b, ao = analysed(ctx, l1=l1)
    if l1:                                                   # frames whose HM was dropped (layer 1 only)
        has = b.download(llsm.A_HAS_HM)
        has[np.random.default_rng(3).random(has.size) < 0.3] = 0
        b.upload(llsm.A_HAS_HM, has)
    before = rows_of(b, l1)
    if op.startswith("sync"):
        b.phasesync_rps(int(op[-1]))
    else:
        b.phasepropagate(int(op[4:]))
    ctx.sync()
    got = rows_of(b, l1)
    b.close()
    masks = phase_masks(before, l1)
    touched = 0
    for u in range(len(b.frm_off) - 1):
        g0, n = int(b.frm_off[u]), int(b.frm_off[u + 1] - b.frm_off[u])
        ch, sl = host_chunk(L, ao, FS, before, g0, n, l1)
        if op.startswith("sync"):
            L.llsm_chunk_phasesync_rps(ch, int(op[-1]))
        else:
            L.llsm_chunk_phasepropagate(ch, int(op[4:]))
        want = chunk_rows(L, ch, {k: v for k, v in sl.items() if k != "has_rd"}, l1)
        L.llsm_delete_chunk(ch)
        for aid, m in masks.items():
            mm = m[g0:g0 + n]
            assert beq(got[aid][g0:g0 + n][mm], want[aid][mm]), (op, l1, u, aid,
                np.abs(got[aid][g0:g0 + n][mm] - want[aid][mm]).max())
            touched += int(mm.sum())
    for aid in before:                                        # padding and every other row untouched
        if aid in masks:
            assert beq(got[aid][~masks[aid]], before[aid][~masks[aid]]), aid
        else:
            assert beq(got[aid], before[aid]), aid
    assert touched > 1000
    # the phases did move (not a vacuous pass)
    assert not beq(got[llsm.A_PHSE][masks[llsm.A_PHSE]], before[llsm.A_PHSE][masks[llsm.A_PHSE]])
    if l1:
        assert int((before[llsm.A_HAS_HM] == 0).sum()) > 0 and int((before[llsm.A_F0] == 0).sum()) > 0


# ------------------------------------------------------------------ numpy restatement of the retime rules
def ref_retime(s, soff, sn, doff, dn, pos, res):
    """expected dst rows, plus where the comparison is not bitwise: fade (frames), circ masks and |v| of VSPHSE / EENV_PHSE"""
    Fd = int(doff[-1])
    mh, ns = s[llsm.A_AMPL].shape[1], s[llsm.A_VTMAGN].shape[1]
    nch, me = s[llsm.A_EENV_AMPL].shape[1:]
    out = {aid: np.zeros((Fd,) + s[aid].shape[1:], s[aid].dtype) for aid in ROWS}
    aux = dict(fade=np.zeros(Fd, bool), cvs=np.zeros((Fd, mh), bool), vvs=np.zeros((Fd, mh)),
               ce=np.zeros((Fd, nch, me), bool), ve=np.zeros((Fd, nch, me)), kinds=[])
    f32 = np.float32

    def circ(pa, pb, r):
        pa, pb, r = np.float64(pa), np.float64(pb), np.float64(r)
        sn_, cs = np.sin(pa) + (np.sin(pb) - np.sin(pa)) * r, np.cos(pa) + (np.cos(pb) - np.cos(pa)) * r
        return np.arctan2(sn_, cs).astype(f32), np.hypot(sn_, cs)

    for u in range(len(dn)):
        n, o = int(sn[u]), int(soff[u])
        for i in range(int(dn[u])):
            g = int(doff[u]) + i
            t = f32(pos[g])
            fl = int(np.floor(t))
            if n > 1:
                a = min(fl, n - 2); r = f32(t - f32(a)); b = a + 1
            else:
                a = b = 0; r = f32(0)
            ga, gb = o + a, o + b
            gr = o + (int(res[g]) if res is not None else min(fl, n - 1))
            out[llsm.A_PSDRES][g] = s[llsm.A_PSDRES][gr]; out[llsm.A_HAS_PSDRES][g] = s[llsm.A_HAS_PSDRES][gr]
            if r == 0 or r == 1:
                gc = ga if r == 0 else gb
                for aid in ROWS:
                    if aid not in (llsm.A_PSDRES, llsm.A_HAS_PSDRES):
                        out[aid][g] = s[aid][gc]
                aux["kinds"].append("copy")
                continue
            lin = lambda x, y: x + (y - x) * r                # float32 operands: float32 arithmetic, no contraction
            fa, fb = s[llsm.A_F0][ga], s[llsm.A_F0][gb]
            va, vb = fa > 0, fb > 0
            nva, nvb = [int(np.clip(s[llsm.A_NVSPHSE][k], 0, mh)) for k in (ga, gb)]
            if va and vb:
                out[llsm.A_F0][g] = lin(fa, fb); out[llsm.A_RD][g] = lin(s[llsm.A_RD][ga], s[llsm.A_RD][gb])
                out[llsm.A_VTMAGN][g] = np.maximum(lin(s[llsm.A_VTMAGN][ga], s[llsm.A_VTMAGN][gb]), f32(-80))
                nmin = min(nva, nvb)
                out[llsm.A_VSPHSE][g] = s[llsm.A_VSPHSE][ga if nva >= nvb else gb]
                for k in range(nmin):
                    out[llsm.A_VSPHSE][g, k], aux["vvs"][g, k] = circ(s[llsm.A_VSPHSE][ga, k], s[llsm.A_VSPHSE][gb, k], r)
                aux["cvs"][g, :nmin] = True
                out[llsm.A_NVSPHSE][g] = max(nva, nvb)
                aux["kinds"].append("vv" + ("~" if nva != nvb else ""))
            elif va or vb:
                gv = ga if va else gb
                w = f32(1) - r if va else r
                fade = 20.0 * np.log10(max(1e-8, float(w)))
                out[llsm.A_F0][g] = s[llsm.A_F0][gv]; out[llsm.A_RD][g] = s[llsm.A_RD][gv]
                out[llsm.A_VTMAGN][g] = np.maximum(s[llsm.A_VTMAGN][gv] + fade, -80).astype(f32)
                out[llsm.A_VSPHSE][g] = s[llsm.A_VSPHSE][gv]
                out[llsm.A_NVSPHSE][g] = np.clip(s[llsm.A_NVSPHSE][gv], 0, mh)
                aux["fade"][g] = True
                aux["kinds"].append("vu" if va else "uv")
            else:
                out[llsm.A_F0][g] = 0; out[llsm.A_RD][g] = 1
                out[llsm.A_VTMAGN][g] = np.maximum(s[llsm.A_VTMAGN][ga], f32(-80))
                out[llsm.A_VSPHSE][g] = s[llsm.A_VSPHSE][ga]; out[llsm.A_NVSPHSE][g] = nva
                aux["kinds"].append("uu")
            out[llsm.A_PSD][g] = lin(s[llsm.A_PSD][ga], s[llsm.A_PSD][gb])
            out[llsm.A_EDC][g] = lin(s[llsm.A_EDC][ga], s[llsm.A_EDC][gb])
            nea, neb = [int(np.clip(s[llsm.A_NHAR_E][k], 0, me)) for k in (ga, gb)]
            nemin, gl = min(nea, neb), (ga if nea >= neb else gb)
            out[llsm.A_EENV_AMPL][g] = s[llsm.A_EENV_AMPL][gl]; out[llsm.A_EENV_PHSE][g] = s[llsm.A_EENV_PHSE][gl]
            out[llsm.A_EENV_AMPL][g][:, :nemin] = lin(s[llsm.A_EENV_AMPL][ga][:, :nemin], s[llsm.A_EENV_AMPL][gb][:, :nemin])
            for c in range(nch):
                for k in range(nemin):
                    out[llsm.A_EENV_PHSE][g, c, k], aux["ve"][g, c, k] = circ(s[llsm.A_EENV_PHSE][ga, c, k],
                                                                             s[llsm.A_EENV_PHSE][gb, c, k], r)
            aux["ce"][g, :, :nemin] = True
            out[llsm.A_NHAR_E][g] = max(nea, neb)
            out[llsm.A_PBPSYN][g] = s[llsm.A_PBPSYN][ga]
            if va or vb:
                out[llsm.A_NHAR][g] = 0; out[llsm.A_HAS_HM][g] = 0            # AMPL / PHSE rows stay zero
            else:
                for aid in (llsm.A_NHAR, llsm.A_AMPL, llsm.A_PHSE, llsm.A_HAS_HM):
                    out[aid][g] = s[aid][ga]
    return out, aux


def assert_retime_rows(got, want, aux, where=""):
    for aid in ROWS:
        if aid in (llsm.A_VTMAGN, llsm.A_VSPHSE, llsm.A_EENV_PHSE):
            continue
        assert beq(got[aid], want[aid]), (where, aid, np.flatnonzero((bits(got[aid]) != bits(want[aid])).reshape(len(got[aid]), -1).any(1))[:8])
    f = aux["fade"]
    assert beq(got[llsm.A_VTMAGN][~f], want[llsm.A_VTMAGN][~f]), where
    fade_err = float(np.abs(got[llsm.A_VTMAGN][f].astype(np.float64) - want[llsm.A_VTMAGN][f]).max()) if f.any() else 0.0
    assert fade_err <= 1e-4, (where, fade_err)
    circ_err = 0.0
    for aid, cm, vm in ((llsm.A_VSPHSE, aux["cvs"], aux["vvs"]), (llsm.A_EENV_PHSE, aux["ce"], aux["ve"])):
        assert beq(got[aid][~cm], want[aid][~cm]), (where, aid)
        if cm.any():
            d = vm[cm] * np.abs(np.exp(1j * got[aid][cm].astype(np.float64)) - np.exp(1j * want[aid][cm].astype(np.float64)))
            circ_err = max(circ_err, float(d.max()))
    assert circ_err <= 2e-6, (where, circ_err)
    return fade_err, circ_err


def perturb_counts(b, seed):
    """neighbours with different NVSPHSE / NHAR_E: lower the counts of a third of the frames (rows only read by retime)"""
    rng = np.random.default_rng(seed)
    nvs, nhe = b.download(llsm.A_NVSPHSE), b.download(llsm.A_NHAR_E)
    k = rng.random(nvs.size) < 0.33
    nvs[k] = (nvs[k] * rng.random(int(k.sum()))).astype(np.int32)
    k = rng.random(nhe.size) < 0.33
    nhe[k] = rng.integers(0, b.layout.maxnhar_e + 1, int(k.sum()))
    b.upload(llsm.A_NVSPHSE, nvs); b.upload(llsm.A_NHAR_E, nhe)


def test_retime_rows_match_the_rules(ctx):
    src, ao = analysed(ctx)
    perturb_counts(src, 11)
    s = rows_of(src)
    sn = np.diff(src.frm_off)
    rng = np.random.default_rng(5)
    report_rows = {}
    # four maps per utterance set: in order, out of order (with integral positions and both end points), explicit psdres
    for case in ("sorted", "shuffled", "psdres"):
        dn = np.array([2 * sn[0], sn[1] // 2 + 3, sn[2], 37], np.int32)
        dst = llsm.Batch(ctx, ao, FS, [0] * len(dn), dn)
        pos, res = [], []
        for u in range(len(dn)):
            n = int(sn[u])
            p = rng.uniform(0, n - 1, int(dn[u])).astype(np.float32)
            # end points, integral positions, and positions between frames of each voicing pair
            v = s[llsm.A_F0][src.frm_off[u]:src.frm_off[u + 1]] > 0
            uv, vu, uu = [np.flatnonzero(m)[:2] for m in (~v[:-1] & v[1:], v[:-1] & ~v[1:], ~v[:-1] & ~v[1:])]
            special = np.concatenate([[0, n - 1, 1, n - 2, np.floor(n / 2), n - 1.5], uv + 0.3, vu + 0.6, uu + 0.5])
            p[:len(special)] = special
            p = np.sort(p) if case == "sorted" else rng.permutation(p)
            pos.append(p)
            res.append(rng.integers(0, n, int(dn[u])).astype(np.int32))
        pos = np.concatenate(pos); res = np.concatenate(res) if case == "psdres" else None
        dst.retime(src, pos, res)
        ctx.sync()
        got = rows_of(dst)
        want, aux = ref_retime(s, src.frm_off, sn, dst.frm_off, dn, pos, res)
        fe, ce = assert_retime_rows(got, want, aux, case)
        kinds = {k: aux["kinds"].count(k) for k in set(aux["kinds"])}
        for k in ("copy", "vv", "vv~", "vu", "uv", "uu"):
            assert kinds.get(k, 0) > 0, (case, k, kinds)              # every branch of the rules was exercised
        assert dst.download(llsm.A_HAS_HM)[np.array(aux["kinds"]) == "vv"].sum() == 0
        report_rows[case] = dict(kinds=kinds, fade_db_max=fe, circ_max=ce)
        dst.close()
    src.close()
    report("retime_rows", report_rows)


def test_retime_on_source_frames_copies_them(ctx):
    """integral positions (and n == 1 utterances) give bit-exact copies of the source frames"""
    src, ao = analysed(ctx, n_utt=2)
    s = rows_of(src)
    sn = np.diff(src.frm_off)
    dn = np.array([3 * sn[0], 5], np.int32)
    dst = llsm.Batch(ctx, ao, FS, [0, 0], dn)
    rng = np.random.default_rng(2)
    idx = [rng.integers(0, sn[0], dn[0]), rng.integers(0, sn[1], dn[1])]
    idx[0][:2] = [0, sn[0] - 1]
    dst.retime(src, np.concatenate(idx).astype(np.float32))
    ctx.sync()
    got = rows_of(dst)
    g = np.concatenate([src.frm_off[u] + idx[u] for u in range(2)])
    for aid in ROWS:
        assert beq(got[aid], s[aid][g]), aid
    dst.close(); src.close()


def chain_tail(b, so, seed):
    b.tolayer0(True); b.phasepropagate(+1); b.synthesize(so, seed=seed)
    return b.download(llsm.A_Y), b.download(llsm.A_YSIN), b.download(llsm.A_YNOISE)


def test_identity_map_is_exact(ctx):
    src, ao = analysed(ctx)
    so = llsm.make_soptions(FS)
    src.phasepropagate(-1)
    dst = llsm.Batch(ctx, ao, FS, [0] * (len(src.frm_off) - 1), np.diff(src.frm_off))
    dst.retime(src)
    ctx.sync()
    s, d = rows_of(src), rows_of(dst)
    for aid in ROWS:
        assert beq(d[aid], s[aid]), aid
    ya = chain_tail(dst, so, 9)
    yb = chain_tail(src, so, 9)                              # the same chain without retime (src was not changed by it)
    for a, b_ in zip(ya, yb):
        assert a.shape == b_.shape and beq(a, b_)
    dst.close(); src.close()


def acf_f0(y, fs, lo=60.0, hi=400.0):
    y = y - y.mean()
    r = np.correlate(y, y, "full")[len(y) - 1:]
    a, b = int(fs / hi), int(fs / lo)
    k = a + int(np.argmax(r[a:b]))
    d = (r[k - 1] - r[k + 1]) / (2 * (r[k - 1] - 2 * r[k] + r[k + 1]))     # parabolic refinement
    return fs / (k + d)


def band_profile(y, fs, nb=8, nfft=2048):
    w = np.hanning(nfft)
    segs = [y[i:i + nfft] * w for i in range(0, len(y) - nfft, nfft // 2)]
    p = np.mean(np.abs(np.fft.rfft(segs, axis=1)) ** 2, axis=0)
    f = np.fft.rfftfreq(nfft, 1 / fs)
    edges = 100.0 * (80.0 ** (np.arange(nb + 1) / nb))
    return np.array([10 * np.log10(p[(f >= edges[i]) & (f < edges[i + 1])].mean()) for i in range(nb)])


def test_end_to_end_stretch_of_arctic(ctx):
    """2x stretch of arctic_a0001 on the device vs the same chain with the retime done in numpy on downloaded rows"""
    x, fs = read_wav(os.path.join(GOLDEN, "arctic_a0001.wav"))
    f0 = np.load(os.path.join(GOLDEN, "arctic_a0001_f0_hop128.npy")).astype(np.float32)
    ao = llsm.make_aoptions(thop=128.0 / fs, f0_refine=0)
    so = llsm.make_soptions(fs)
    nfrm = len(f0)
    src = llsm.Batch(ctx, ao, fs, [len(x)], [nfrm])
    src.upload(llsm.A_X, x); src.upload(llsm.A_F0, f0)
    src.analyze()
    src.synthesize(so, seed=3)
    y0 = src.download(llsm.A_Y)
    f0a = src.download(llsm.A_F0)
    src.tolayer1(NFFT); src.phasepropagate(-1)
    dev = llsm.Batch(ctx, ao, fs, [0], [2 * nfrm])
    dev.retime(src)
    yd = chain_tail(dev, so, 7)
    # the same with the frames blended in numpy
    s = rows_of(src)
    pos = llsm.retime_uniform_positions(nfrm, 2 * nfrm)
    want, _ = ref_retime(s, src.frm_off, [nfrm], dev.frm_off, [2 * nfrm], pos, None)
    host = llsm.Batch(ctx, ao, fs, [0], [2 * nfrm])
    host.enable_layer1(NFFT)
    for aid in ROWS:
        host.upload(aid, want[aid])
    yh = chain_tail(host, so, 7)
    ctx.sync()
    errs = [rel_rms(a, b) for a, b in zip(yd, yh)]
    ny2 = llsm.load().llsm_gpu_plan_index(5, 2 * nfrm, 0, 0.0, ao.thop, fs, ao.rel_winsize)
    lvl = 10 * np.log10(np.mean(yd[0].astype(np.float64) ** 2) / np.mean(y0.astype(np.float64) ** 2))
    bands = np.abs(band_profile(yd[0], fs) - band_profile(y0, fs))
    # F0 of the middle of the longest voiced run, by autocorrelation of the stretched output
    v = np.concatenate([[0], (f0a > 0).astype(np.int8), [0]])
    st, en = np.flatnonzero(np.diff(v) == 1), np.flatnonzero(np.diff(v) == -1)
    k = int(np.argmax(en - st)); mid = (st[k] + en[k]) // 2
    seg = yd[0][2 * mid * 128 - 1024: 2 * mid * 128 + 1024]
    f0_acf, f0_ref = acf_f0(seg, fs), float(np.median(f0a[mid - 4: mid + 4]))
    m = dict(rel_rms_y=errs[0], rel_rms_ysin=errs[1], rel_rms_ynoise=errs[2], ny=len(yd[0]), ny_plan=ny2,
             level_db=float(lvl), band_db_max=float(bands.max()), f0_acf=f0_acf, f0_analysed=f0_ref)
    report("retime_arctic_2x", m)
    for b in (src, dev, host):
        b.close()
    assert max(errs) <= 1e-4, m
    assert len(yd[0]) == ny2 and np.all(np.isfinite(yd[0])), m
    assert abs(lvl) <= 1.0 and bands.max() <= 2.0, m
    assert abs(f0_acf / f0_ref - 1) <= 0.03, m


def synthetic_src(ctx, ao, nfrm, seed, nfft=1024):
    """a layer-1 batch of plausible random rows (voiced runs, unvoiced gaps, varying counts) without an analysis"""
    rng = np.random.default_rng(seed)
    b = llsm.Batch(ctx, ao, FS, [0] * len(nfrm), nfrm)
    b.enable_layer1(nfft)
    F = b.layout.total_frames
    r = {}
    for aid in ROWS:
        shp = b.shape(aid)
        r[aid] = rng.uniform(-3, 3, shp).astype(np.float32) if aid not in INT else rng.integers(0, 2, shp).astype(np.int32)
    r[llsm.A_F0] = np.where(rng.random(F) < 0.75, rng.uniform(80, 300, F), 0).astype(np.float32)
    r[llsm.A_NHAR] = rng.integers(0, b.layout.maxnhar + 1, F).astype(np.int32)
    r[llsm.A_NVSPHSE] = rng.integers(0, b.layout.maxnhar + 1, F).astype(np.int32)
    r[llsm.A_NHAR_E] = rng.integers(0, b.layout.maxnhar_e + 1, F).astype(np.int32)
    r[llsm.A_VTMAGN] = rng.uniform(-100, 0, b.shape(llsm.A_VTMAGN)).astype(np.float32)
    for aid, a in r.items():
        b.upload(aid, a)
    return b, r


def test_retime_is_batch_invariant(ctx):
    ao = llsm.make_aoptions(f0_refine=0)
    rng = np.random.default_rng(17)
    sn = rng.integers(1, 300, 64).astype(np.int32)
    dn = np.maximum(1, (sn * rng.choice([0.5, 1.0, 1.37, 2.0, 3.0], 64)).astype(np.int32))
    src, rows = synthetic_src(ctx, ao, sn, 1)
    dst = llsm.Batch(ctx, ao, FS, [0] * 64, dn)
    pos = np.concatenate([rng.uniform(0, n - 1, m).astype(np.float32) for n, m in zip(sn, dn)])
    res = np.concatenate([rng.integers(0, n, m) for n, m in zip(sn, dn)]).astype(np.int32)
    dst.retime(src, pos, res)
    ctx.sync()
    whole = rows_of(dst)
    for u in (0, 1, 17, 40, 63, int(np.argmin(sn))):
        s0, s1, d0, d1 = src.frm_off[u], src.frm_off[u + 1], dst.frm_off[u], dst.frm_off[u + 1]
        one_src = llsm.Batch(ctx, ao, FS, [0], [sn[u]]); one_src.enable_layer1(1024)
        for aid in ROWS:
            one_src.upload(aid, rows[aid][s0:s1])
        one = llsm.Batch(ctx, ao, FS, [0], [dn[u]])
        one.retime(one_src, pos[d0:d1], res[d0:d1])
        ctx.sync()
        alone = rows_of(one)
        for aid in ROWS:
            assert beq(alone[aid], whole[aid][d0:d1]), (u, aid)
        one.close(); one_src.close()
    # and the rules hold on these rows too
    want, aux = ref_retime(rows, src.frm_off, sn, dst.frm_off, dn, pos, res)
    assert_retime_rows(whole, want, aux, "synthetic")
    dst.close(); src.close()
    # and on the smallest shape: a one-frame source, and groups of four output frames that straddle utterances (boundaries
    # at 3 and 8 of 14 frames), with psdres_src and without
    sn, dn = np.array([1, 2, 5], np.int32), np.array([3, 5, 6], np.int32)
    src, rows = synthetic_src(ctx, ao, sn, 2)
    pos = []
    for n, m in zip(sn, dn):
        p = rng.uniform(0, n - 1, m).astype(np.float32)
        p[:2] = [0, n - 1]                                   # both end points of every utterance
        pos.append(rng.permutation(p))
    pos = np.concatenate(pos)
    res = np.concatenate([rng.integers(0, n, m) for n, m in zip(sn, dn)]).astype(np.int32)
    for r in (res, None):
        dst = llsm.Batch(ctx, ao, FS, [0] * 3, dn)
        dst.retime(src, pos, r)
        ctx.sync()
        want, aux = ref_retime(rows, src.frm_off, sn, dst.frm_off, dn, pos, r)
        assert_retime_rows(rows_of(dst), want, aux, "smallest" if r is None else "smallest, psdres_src")
        dst.close()
    src.close()


def test_retime_refusals_leave_dst_untouched(ctx):
    L = llsm.load()
    ao = llsm.make_aoptions(f0_refine=0)
    src, _ = synthetic_src(ctx, ao, [20, 30], 4)
    dst = llsm.Batch(ctx, ao, FS, [0, 0], [40, 60])
    before = rows_of(dst, l1=False)
    ok_pos = np.concatenate([llsm.retime_uniform_positions(20, 40), llsm.retime_uniform_positions(30, 60)])

    def call(d, s, pos=None, res=None):
        p = None if pos is None else np.ascontiguousarray(pos, np.float32)
        r = None if res is None else np.ascontiguousarray(res, np.int32)
        rc = L.llsm_gpu_batch_retime(d.h, s.h, None if p is None else p.ctypes.data_as(llsm.P_fp),
                                     None if r is None else r.ctypes.data_as(llsm.P_int))
        return rc, L.llsm_gpu_last_error().decode()

    other_opt = llsm.Batch(ctx, llsm.make_aoptions(f0_refine=0, npsd=128), FS, [0, 0], [40, 60])
    other_fs = llsm.Batch(ctx, ao, 22050.0, [0, 0], [40, 60])
    other_n = llsm.Batch(ctx, ao, FS, [0, 0, 0], [40, 60, 5])
    ctx2 = llsm.Context(0)
    other_ctx = llsm.Batch(ctx2, ao, FS, [0, 0], [40, 60])
    no_l1 = llsm.Batch(ctx, ao, FS, [0, 0], [20, 30])
    empty_side = llsm.Batch(ctx, ao, FS, [0, 0], [40, 0])
    l1_other = llsm.Batch(ctx, ao, FS, [0, 0], [40, 60]); l1_other.enable_layer1(2048)
    l1_before = rows_of(l1_other)
    bad = lambda i, v: np.where(np.arange(100) == i, v, ok_pos).astype(np.float32)
    cases = {
        "options": (other_opt, src, None, None), "sampling rate": (other_fs, src, None, None),
        "utterance count": (other_n, src, None, None), "context": (other_ctx, src, None, None),
        "same batch": (src, src, None, None), "no layer 1": (dst, no_l1, None, None),
        "pos NaN": (dst, src, bad(5, np.nan), None), "pos < 0": (dst, src, bad(0, -1e-3), None),
        "pos > n - 1": (dst, src, bad(39, 19.5), None), "pos > n - 1 (utt 1)": (dst, src, bad(99, 29.01), None),
        "psdres < 0": (dst, src, None, np.where(np.arange(100) == 3, -1, 0)),
        "psdres >= n": (dst, src, None, np.where(np.arange(100) == 45, 30, 0)),
        "frames on one side": (empty_side, src, None, None), "layer 1 of another size": (l1_other, src, None, None),
    }
    for name, (d, s, p, r) in cases.items():
        rc, msg = call(d, s, p, r)
        assert rc == -1 and msg.startswith("llsm_gpu_batch_retime:"), (name, rc, msg)
    ctx.sync()
    after = rows_of(dst, l1=False)
    for aid in PARAM:
        assert beq(after[aid], before[aid]), aid
    assert dst.L.llsm_gpu_batch_array_bytes(dst.h, llsm.A_RD) == 0      # layer 1 was not enabled by a refused call
    l1_after = rows_of(l1_other)
    for aid in ROWS:
        assert beq(l1_after[aid], l1_before[aid]), aid
    rc, msg = call(dst, src, ok_pos)                                     # and the valid call goes through
    assert rc == 0, msg
    for b in (other_opt, other_fs, other_n, other_ctx, no_l1, empty_side, l1_other, dst, src):
        b.close()
    ctx2.close()


def test_c_host_stretches_through_the_batch_api(tmp_path):
    """tests/c_host/stretch_batch_host.c: the whole device chain through llsm_gpu.h alone, built with the flags of the
    other C-host tests"""
    from test_c_host import CFLAGS, LIBDIR
    llsm.load()
    exe = str(tmp_path / "stretch_batch_host")
    subprocess.check_call(CFLAGS + ["-o", exe, os.path.join(HERE, "c_host", "stretch_batch_host.c"),
                                    "-L" + LIBDIR, "-l:libllsm2_amd.so", "-Wl,-rpath," + LIBDIR, "-lm"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "stretch_batch ok" in out.stdout, out.stdout + out.stderr
