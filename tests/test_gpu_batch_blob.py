"""-m gpu: utterances of a device-resident batch as chunk blobs packed on the device (llsm_gpu_batch_blob_sizes,
llsm_gpu_batch_download_blobs, llsm_gpu_batch_download_blob_block; csrc/batch_blob.cpp, csrc/blob_kernels.hip).

The contract is byte equality with the host path the export replaces: the rows of an utterance downloaded, a chunk built
from them the way llsm_blob_to_chunk builds one (conf from llsm_aoptions_toconf(options, fnyq) with NFRM and, with layer 1,
LLSM_CONF_NSPEC; llsm_flat_to_chunk; llsm_flat_l1_to_chunk with has_rd = 1; HM removed where HAS_HM is 0), serialised by
llsm_chunk_to_blob.  Every comparison below is np.array_equal on uint8 or on the bit patterns of rows; nothing has a
tolerance."""
import ctypes as C

import numpy as np
import pytest

import libllsm2_amd as llsm
from conftest import FS
from test_gpu_retime import chunk_rows, flat_l1_view, flat_view
from test_wire import _bind

pytestmark = pytest.mark.gpu

PARAM = llsm.Batch.PARAM_IDS
L1 = llsm.Batch.L1_IDS
OTHER = (llsm.A_X, llsm.A_XRES, llsm.A_Y, llsm.A_YSIN, llsm.A_YNOISE, llsm.A_WHITE)
THOP = 0.005


@pytest.fixture(scope="module")
def ctx():
    c = llsm.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def L():
    lib = _bind(llsm.load())
    lib.llsm_blob_view_l1.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(llsm.FlatL1)]
    lib.llsm_gpu_batch_upload_blobs.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    lib.llsm_gpu_alloc_host.restype = C.c_void_p; lib.llsm_gpu_alloc_host.argtypes = [C.c_size_t]
    lib.llsm_gpu_free_host.argtypes = [C.c_void_p]
    return lib


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def beq(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def utterance(u, nx, base, dev, voiced_any=True):
    """conftest.make_speechlike with the F0 track around `base` Hz (+- dev, kept within 80 .. 400 Hz): voiced / unvoiced
    stretches, harmonics up to the Nyquist frequency; voiced_any = False: noise alone, F0 = 0 on every frame"""
    rng = np.random.default_rng(4100 + u)
    nfrm = int(nx / FS / THOP)
    t = np.arange(nfrm) * THOP
    f0 = np.clip(base + dev * np.sin(2 * np.pi * 1.3 * t + u) + 0.3 * dev * np.sin(2 * np.pi * 4.1 * t), 80.0, 400.0)
    voiced = np.ones(nfrm, bool)
    voiced[:6] = False; voiced[nfrm // 2 - 8: nfrm // 2 + 6] = False; voiced[-5:] = False
    if not voiced_any:
        voiced[:] = False
    f0 = np.where(voiced, f0, 0.0)
    ts = np.arange(nx) / FS
    f0s = np.interp(ts, t, np.where(voiced, f0, base)); vs = np.interp(ts, t, voiced.astype(float))
    phase = 2 * np.pi * np.cumsum(f0s) / FS
    x = np.zeros(nx)
    for k in range(1, int(FS / 2 / (base + 1.3 * dev))):
        x += 0.25 / k ** 1.2 * np.cos(k * phase + 0.37 * k * k)
    x = x * vs + (0.004 + 0.03 * (1 - vs)) * rng.standard_normal(nx)
    return x.astype(np.float32), f0.astype(np.float32)


# (samples, F0 centre, F0 swing, voiced): at 44.1 kHz a frame holds min(100, 22050 / F0) harmonics, so only F0 above 220 Hz
# narrows a row -- three of the four voiced utterances stay above it, each in its own band
SPEC = [(22000, 95.0, 12.0, True), (30000, 255.0, 18.0, True), (17000, 310.0, 25.0, True), (26000, 368.0, 30.0, True),
        (12000, 120.0, 0.0, False)]


@pytest.fixture(scope="module")
def src(ctx):
    """case 1: four speech-like utterances of different lengths, F0 between 80 and 400 Hz, and an all-unvoiced one;
    analysed, no layer 1.  Returns (batch, options); tests do not modify the batch"""
    ao = llsm.make_aoptions(f0_refine=0)
    xs, f0s = zip(*[utterance(u, *s) for u, s in enumerate(SPEC)])
    b = llsm.Batch(ctx, ao, FS, [len(x) for x in xs], [len(f) for f in f0s])
    b.upload(llsm.A_X, np.concatenate(xs)); b.upload(llsm.A_F0, np.concatenate(f0s))
    b.analyze(); ctx.sync()
    yield b, ao
    b.close()


def has_l1(b):
    return getattr(b, "nspec", 0) > 0


def rows_of(b):
    return {aid: b.download(aid) for aid in PARAM + (L1 if has_l1(b) else ())}


def all_arrays(b):
    ids = PARAM + OTHER + (L1 if has_l1(b) else ()) + ((llsm.A_CODE,) if b.coder_dimension > 0 else ())
    return {aid: b.download(aid) for aid in ids}


def clone(ctx, ao, rows, nfrm, nx=None, sel=None):
    """a batch with the given frame counts holding `rows` (the frames `sel` of them); layer 1 when the rows have it"""
    b = llsm.Batch(ctx, ao, FS, nx if nx is not None else [0] * len(nfrm), nfrm)
    pick = (lambda a: a) if sel is None else (lambda a: np.ascontiguousarray(a[sel]))
    if llsm.A_VTMAGN in rows:
        b.enable_layer1((rows[llsm.A_VTMAGN].shape[1] - 1) * 2)
    for aid, a in rows.items():
        b.upload(aid, pick(a))
    return b


# ------------------------------------------------------------------ the host path
def host_chunk(L, ao, fnyq, sl, nspec):
    """the chunk llsm_blob_to_chunk would build from the rows `sl` of one utterance"""
    n = len(sl[llsm.A_F0])
    conf = L.llsm_aoptions_toconf(C.byref(ao), fnyq)
    C.cast(L.llsm_container_get(conf, llsm.CONF_NFRM), llsm.P_int)[0] = n
    ch = L.llsm_create_chunk(conf, 1)
    L.llsm_delete_container(conf)
    assert L.llsm_flat_to_chunk(C.byref(flat_view(sl)), 0, ch) == 0
    if nspec > 0:
        vp = C.c_void_p
        L.llsm_container_attach_(ch.contents.conf, llsm.CONF_NSPEC, C.cast(L.llsm_create_int(nspec), vp),
                                 C.cast(L.llsm_delete_int, vp), C.cast(L.llsm_copy_int, vp))
        sl = dict(sl); sl["has_rd"] = np.ones(n, np.int32)
        assert L.llsm_flat_l1_to_chunk(C.byref(flat_l1_view(sl)), 0, ch) == 0
        for i in np.flatnonzero(sl[llsm.A_HAS_HM] == 0):
            L.llsm_container_attach_(ch.contents.frames[int(i)], llsm.FRAME_HM, None, None, None)
    return ch


def chunk_blob(L, ch):
    n = L.llsm_chunk_blob_size(ch)
    buf = np.zeros((n + 7) // 8, np.uint64).view(np.uint8)[:n]
    assert L.llsm_chunk_to_blob(ch, C.c_void_p(buf.ctypes.data), n) == n
    return buf


def host_blobs(L, b, ao, fnyq, utts):
    """per utterance: (llsm_chunk_to_blob bytes, the normalised rows chunk_rows gives at the batch's widths)"""
    rows = rows_of(b)
    out = []
    for u in utts:
        g0, g1 = int(b.frm_off[u]), int(b.frm_off[u + 1])
        sl = {aid: np.ascontiguousarray(a[g0:g1]) for aid, a in rows.items()}
        ch = host_chunk(L, ao, fnyq, sl, getattr(b, "nspec", 0))
        norm = chunk_rows(L, ch, sl, has_l1(b))
        norm.pop("has_rd", None)
        out.append((chunk_blob(L, ch), norm))
        L.llsm_delete_chunk(ch)
    return out


def pinned(L, n):
    p = L.llsm_gpu_alloc_host(max(n, 1))
    assert p
    return p, np.frombuffer((C.c_ubyte * max(n, 1)).from_address(p), dtype=np.uint8)


def check_export(ctx, L, b, ao, fnyq=FS / 2.0, utt0=0, n=None, what=""):
    """every way out against the host path, validity of the blobs, and that the batch did not move; returns
    (blobs, host results)"""
    n = b.layout.n_utt - utt0 if n is None else n
    ctx.sync()
    before = all_arrays(b)
    want = host_blobs(L, b, ao, fnyq, range(utt0, utt0 + n))
    sizes = b.blob_sizes(utt0, n)
    assert sizes == [len(w) for w, _ in want], (what, sizes, [len(w) for w, _ in want])
    got = b.download_blobs(utt0, n)
    for k in range(n):
        if not np.array_equal(got[k], want[k][0]):
            d = np.flatnonzero(got[k][:min(len(got[k]), len(want[k][0]))] != want[k][0][:min(len(got[k]), len(want[k][0]))])
            raise AssertionError("%s: blob %d differs from llsm_chunk_to_blob in %d bytes, first at %s (sizes %d / %d)"
                                 % (what, utt0 + k, d.size, d[:8], len(got[k]), len(want[k][0])))
    # the block forms, pageable and page-locked: same offsets, same bytes, gaps included
    total = sum((s + 15) // 16 * 16 for s in sizes)
    blk = np.full(total + 32, 0xA5, np.uint8)
    offs = b.download_blob_block(blk, utt0, n)
    assert len(offs) == n + 1 and offs[0] == 0 and offs[n] == total and all(o % 16 == 0 for o in offs), (what, offs)
    assert (blk[total:] == 0xA5).all()
    p, pblk = pinned(L, total + 32)
    pblk[:] = 0xA5
    offs2 = b.download_blob_block(pblk, utt0, n)
    assert offs2 == offs and np.array_equal(pblk, blk), what
    L.llsm_gpu_free_host(p)
    for k in range(n):
        assert np.array_equal(blk[offs[k]:offs[k] + sizes[k]], want[k][0]), (what, k)
        assert not blk[offs[k] + sizes[k]:offs[k + 1]].any(), (what, k)
    # validity: the views accept every blob; the chunk llsm_blob_to_chunk rebuilds serialises to the same bytes
    for k in range(n):
        v = llsm.FlatParams(); q = llsm.FlatL1(); nf = C.c_int(-1); fq = llsm.fp(0)
        addr = C.c_void_p(got[k].ctypes.data)
        assert L.llsm_blob_view(addr, sizes[k], C.byref(v), C.byref(nf), None, C.byref(fq)) == 0, L.llsm_gpu_last_error()
        assert nf.value == int(b.frm_off[utt0 + k + 1] - b.frm_off[utt0 + k]) and fq.value == np.float32(fnyq)
        assert L.llsm_blob_view_l1(addr, sizes[k], C.byref(q)) == 0 and q.nspec == getattr(b, "nspec", 0)
        ch = L.llsm_blob_to_chunk(addr, sizes[k])
        assert bool(ch)
        assert np.array_equal(chunk_blob(L, ch), got[k]), (what, k)
        L.llsm_delete_chunk(ch)
    after = all_arrays(b)
    for aid in before:
        assert beq(before[aid], after[aid]), (what, "array moved", aid)
    return got, want


def header_widths(blob):
    return tuple(int(x) for x in np.frombuffer(blob[20:28].tobytes(), np.int32))


# ------------------------------------------------------------------ the cases
def test_analysed_batch(ctx, L, src):
    """case 1 (and case 7, a sub-range): widths differ per utterance and are below the batch's"""
    b, ao = src
    got, _ = check_export(ctx, L, b, ao, what="analysed")
    w = [header_widths(g) for g in got]
    assert len({x[0] for x in w[:4]}) == 4 and all(0 < x[0] <= ao.maxnhar for x in w[:4]), w
    assert w[3][0] < w[2][0] < w[1][0] < w[0][0] and w[4] == (0, 0), w       # the higher the F0 the narrower; unvoiced: none
    sub, _ = check_export(ctx, L, b, ao, utt0=1, n=2, what="sub-range")
    assert np.array_equal(sub[0], got[1]) and np.array_equal(sub[1], got[2])
    assert b.blob_sizes(2, 0) == [] and b.download_blobs(5, 0) == []
    assert isinstance(b.download_blobs(0, 1, as_bytes=True)[0], bytes)


@pytest.mark.parametrize("nfft", [2048, 1024])
def test_layer1_batch(ctx, L, src, nfft):
    """case 2: tolayer1 and phasepropagate(-1); PBPSYN on some frames through an upload"""
    s, ao = src
    b = clone(ctx, ao, rows_of(s), np.diff(s.frm_off))
    b.tolayer1(nfft); b.phasepropagate(-1)
    check_export(ctx, L, b, ao, what="layer 1, nfft %d" % nfft)
    F = b.layout.total_frames
    b.upload(llsm.A_PBPSYN, (np.arange(F) % 40 > 20).astype(np.int32) * 3)
    got, _ = check_export(ctx, L, b, ao, what="layer 1 + PBPSYN, nfft %d" % nfft)
    q = llsm.FlatL1()
    assert L.llsm_blob_view_l1(C.c_void_p(got[0].ctypes.data), len(got[0]), C.byref(q)) == 0
    assert q.nspec == nfft // 2 + 1 and q.pbpsyn[25] == 3 and q.pbpsyn[5] == 0 and q.has_rd[0] == 1
    b.close()


def layer1_of(ctx, src, nfft=2048):
    s, ao = src
    b = clone(ctx, ao, rows_of(s), np.diff(s.frm_off), nx=np.diff(s.x_off))
    b.tolayer1(nfft); b.phasepropagate(-1)
    return b, ao


def test_retimed_batch(ctx, L, src):
    """case 3: retime to 1.7 x -- voiced frames without HM (HAS_HM = 0) -- and again after tolayer0 rebuilt them"""
    a, ao = layer1_of(ctx, src)
    nfrm = [int(round(1.7 * n)) for n in np.diff(a.frm_off)]
    d = llsm.Batch(ctx, ao, FS, [0] * len(nfrm), nfrm)
    d.retime(a)
    r = rows_of(d)
    assert int(((r[llsm.A_HAS_HM] == 0) & (r[llsm.A_F0] != 0)).sum()) > 100
    got, _ = check_export(ctx, L, d, ao, what="retimed, HM missing")
    d.tolayer0(True); d.phasepropagate(+1)
    check_export(ctx, L, d, ao, what="retimed, tolayer0")
    assert int((d.download(llsm.A_HAS_HM) == 0).sum()) == 0   # the harmonic rows are back
    a.close(); d.close()


def test_pitch_shifted_batch(ctx, L, src):
    """case 4: pitch_formant(rho = 0.7) and tolayer0"""
    b, ao = layer1_of(ctx, src)
    b.pitch_formant(f0_ratio=0.7)
    check_export(ctx, L, b, ao, what="pitch shifted, HM missing")
    b.tolayer0(True)
    check_export(ctx, L, b, ao, what="pitch shifted, tolayer0")
    b.close()


def test_decoded_batch(ctx, L, src):
    """case 5: after encode and decode(1) / decode(0): NVSPHSE = 0 rows, default envelopes"""
    b, ao = layer1_of(ctx, src)
    b.enable_coder(64, 5); b.encode()
    b.decode(1)
    check_export(ctx, L, b, ao, what="decode(1)")
    b.tolayer0(True)
    check_export(ctx, L, b, ao, what="decode(1), tolayer0")
    b.decode(0)
    got, _ = check_export(ctx, L, b, ao, what="decode(0)")
    assert int((b.download(llsm.A_NVSPHSE) != 0).sum()) == 0
    b.close()


def test_other_nyquist_and_no_envelopes(ctx, L, src):
    """case 6: llsm_gpu_batch_set_fnyq; options with maxnhar_e = 0 (envelope rows of width 1, count 0)"""
    s, ao = src
    b = clone(ctx, ao, rows_of(s), np.diff(s.frm_off))
    assert L.llsm_gpu_batch_set_fnyq(b.h, 16000.0) == 0
    check_export(ctx, L, b, ao, fnyq=16000.0, what="fnyq 16 kHz")
    b.close()
    ao0 = llsm.make_aoptions(f0_refine=0, maxnhar_e=0, nchannel=3, chanfreq=[1500.0, 5000.0], npsd=129, maxnhar=77)
    F = 53
    rng = np.random.default_rng(8)
    f0 = np.where(rng.random(F) < 0.7, rng.uniform(90, 380, F), 0).astype(np.float32)
    rows = {llsm.A_F0: f0, llsm.A_NHAR: np.where(f0 > 0, rng.integers(0, 60, F), rng.integers(0, 60, F)).astype(np.int32),
            llsm.A_AMPL: rng.random((F, 77), np.float32), llsm.A_PHSE: rng.random((F, 77), np.float32),
            llsm.A_PSD: rng.random((F, 129), np.float32), llsm.A_PSDRES: rng.random((F, 129), np.float32),
            llsm.A_HAS_PSDRES: (rng.random(F) < 0.5).astype(np.int32) * 7, llsm.A_EDC: rng.random((F, 3), np.float32),
            llsm.A_NHAR_E: np.zeros(F, np.int32), llsm.A_EENV_AMPL: rng.random((F, 3, 1), np.float32),
            llsm.A_EENV_PHSE: rng.random((F, 3, 1), np.float32)}
    b = clone(ctx, ao0, rows, [20, 0, 33])                  # odd widths, dirty padding, an utterance without frames
    got, _ = check_export(ctx, L, b, ao0, what="maxnhar_e = 0")
    assert header_widths(got[0])[1] == 0 and header_widths(got[1]) == (0, 0)
    b.close()


# ------------------------------------------------------------------ round trip, independence, refusals
@pytest.mark.parametrize("l1", [False, True])
def test_round_trip_through_upload_blobs(ctx, L, src, l1):
    """download_blobs -> upload_blobs into a fresh batch of the same shape: the normalised rows, and the same waveforms"""
    s, ao = src
    if l1:
        a, _ = layer1_of(ctx, src); a.phasepropagate(+1)
    else:
        a = clone(ctx, ao, rows_of(s), np.diff(s.frm_off), nx=np.diff(s.x_off))
    ctx.sync()
    blobs = a.download_blobs()
    want = host_blobs(L, a, ao, FS / 2.0, range(a.layout.n_utt))
    f = llsm.Batch(ctx, ao, FS, np.diff(a.x_off), np.diff(a.frm_off))
    n = len(blobs)
    ptrs = (C.c_void_p * n)(*[x.ctypes.data for x in blobs]); sz = (C.c_size_t * n)(*[len(x) for x in blobs])
    assert L.llsm_gpu_batch_upload_blobs(f.h, 0, n, ptrs, sz) == 0, L.llsm_gpu_last_error()
    if l1:
        f.nspec = a.nspec
    got = rows_of(f)
    for u in range(n):
        g0, g1 = int(a.frm_off[u]), int(a.frm_off[u + 1])
        for aid, ref in want[u][1].items():
            assert beq(got[aid][g0:g1], ref), (u, aid)
    white = np.random.default_rng(1).standard_normal(a.shape(llsm.A_WHITE)).astype(np.float32)
    so = llsm.make_soptions(FS)
    outs = []
    for b in (a, f):
        b.upload(llsm.A_WHITE, white)
        b.synthesize(so, seed=5, injected_white=True); ctx.sync()
        outs.append([b.download(x) for x in (llsm.A_Y, llsm.A_YSIN, llsm.A_YNOISE)])
    for name, p, q in zip("y y_sin y_noise".split(), *outs):
        assert np.sqrt(np.mean(p.astype(np.float64) ** 2)) > 1e-3, name
        assert beq(p, q), (name, float(np.abs(p - q).max()))
    a.close(); f.close()


@pytest.mark.parametrize("pad", [0, 3])
def test_an_utterance_has_the_bytes_it_has_alone(ctx, L, src, pad):
    """utterance 17 of 64 of mixed lengths, the frame total a multiple of 16 (pad = 0) and not"""
    a, ao = layer1_of(ctx, src)
    a.upload(llsm.A_HAS_HM, (np.arange(a.layout.total_frames) % 7 != 0).astype(np.int32))
    rows = rows_of(a); ctx.sync()
    F = a.layout.total_frames
    rng = np.random.default_rng(17)
    nfrm = [int(x) for x in rng.integers(1, 40, 64)]
    g0, g1 = int(a.frm_off[2]), int(a.frm_off[3])             # the 310 Hz utterance goes to place 17
    nfrm[17] = g1 - g0
    nfrm[63] += (16 - sum(nfrm) % 16) % 16 + pad
    assert sum(nfrm) % 16 == pad
    sel = np.concatenate([np.arange(g0, g1) if u == 17 else (rng.integers(0, F) + np.arange(nfrm[u])) % F for u in range(64)])
    big = clone(ctx, ao, rows, nfrm, sel=sel)
    alone = clone(ctx, ao, rows, [g1 - g0], sel=np.arange(g0, g1))
    one = alone.download_blobs()[0]
    assert np.array_equal(big.download_blobs(17, 1)[0], one)
    assert np.array_equal(big.download_blobs()[17], one)
    assert np.array_equal(one, a.download_blobs(2, 1)[0])
    check_export(ctx, L, big, ao, what="64 utterances")
    a.close(); big.close(); alone.close()


def test_refusals_write_nothing(ctx, L, src):
    b, ao = src
    sizes = b.blob_sizes()
    n = len(sizes)
    before = all_arrays(b)
    bufs = [np.full(s // 8 + 2, 0xA5A5A5A5A5A5A5A5, np.uint64).view(np.uint8) for s in sizes]
    offs = (C.c_size_t * (n + 1))(*[7] * (n + 1))
    total = sum((s + 15) // 16 * 16 for s in sizes)
    blk = np.full(total + 16, 0xA5, np.uint8)

    def blobs(utt0, cnt, ptr_of=lambda k: bufs[k].ctypes.data, cap_of=lambda k: sizes[k]):
        ptrs = (C.c_void_p * n)(*[ptr_of(k) for k in range(n)]); caps = (C.c_size_t * n)(*[cap_of(k) for k in range(n)])
        return L.llsm_gpu_batch_download_blobs(b.h, utt0, cnt, ptrs, caps)

    def refused(rc, *words):
        msg = L.llsm_gpu_last_error().decode()
        assert rc == -1 and all(w in msg for w in words), (rc, msg, words)
        assert all((x == 0xA5).all() for x in bufs) and (blk == 0xA5).all() and list(offs) == [7] * (n + 1), msg

    refused(blobs(0, n, cap_of=lambda k: sizes[k] - (k == 3)), "utterance 3", str(sizes[3]))      # one byte short
    refused(blobs(0, n, ptr_of=lambda k: bufs[k].ctypes.data + 4 * (k == 1)), "aligned")
    refused(blobs(0, n, ptr_of=lambda k: None if k == 2 else bufs[k].ctypes.data), "NULL")
    refused(blobs(3, 3), "not within")                                                          # past the last utterance
    refused(blobs(-1, 2), "not within")
    refused(L.llsm_gpu_batch_download_blobs(b.h, 0, n, None, None), "NULL")
    addr = C.c_void_p(blk.ctypes.data)
    refused(L.llsm_gpu_batch_download_blob_block(b.h, 0, n, addr, total - 1, offs), "need " + str(total))
    refused(L.llsm_gpu_batch_download_blob_block(b.h, 4, 2, addr, total, offs), "not within")
    refused(L.llsm_gpu_batch_download_blob_block(b.h, 0, n, C.c_void_p(blk.ctypes.data + 4), total, offs), "aligned")
    refused(L.llsm_gpu_batch_download_blob_block(b.h, 0, n, None, total, offs), "NULL")
    refused(L.llsm_gpu_batch_blob_sizes(b.h, 0, n + 1, (C.c_size_t * (n + 1))()), "not within")
    assert blobs(2, 0) == 0 and all((x == 0xA5).all() for x in bufs)                               # n == 0: nothing to do
    after = all_arrays(b)
    for aid in before:
        assert beq(before[aid], after[aid]), aid
    # and the accepted call still works on the same buffers
    assert blobs(0, n) == 0, L.llsm_gpu_last_error()
    want = host_blobs(L, b, ao, FS / 2.0, range(n))
    for k in range(n):
        assert np.array_equal(bufs[k][:sizes[k]], want[k][0]) and (bufs[k][sizes[k]:] == 0xA5).all()
