"""-m gpu: the pitch and formant edit of a device-resident layer-1 batch (llsm_gpu_batch_pitch_formant), the middle of the
reference's pitch-shift recipe (test/test-layer1-anasynth.c, "Shift pitch by 1.5x"), against a numpy restatement of the
rules of llsm_gpu.h written here: every row bit-identical, except VTMAGN of frames with an F0 ratio != 1, which may differ
by one float32 ulp (the device's and numpy's float64 log10 may round their last bit differently).  The end-to-end tests
compare the device chain with the same chain edited in numpy on downloaded rows."""
import os
import subprocess

import numpy as np
import pytest

import libllsm2_amd as llsm
from conftest import FS
from gpu_common import rel_rms, report
from test_gpu_retime import ROWS, analysed, beq, bits, rows_of, synthetic_src
from verify_utils import GOLDEN, read_wav

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NFFT = 2048
A = llsm


@pytest.fixture(scope="module")
def ctx():
    c = llsm.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------ numpy restatement of the rules
def warp_np(x, alpha):
    """row x (n bins on linspace(0, fnyq, n)) with the envelope at f moved to alpha f"""
    n = x.shape[0]
    p = np.arange(n, dtype=np.float64) / np.float64(alpha)      # correctly rounded float64 division
    i = np.floor(p).astype(np.int64)
    top = i >= n - 1
    ic = np.minimum(i, max(n - 2, 0))
    r = (p - i).astype(np.float32)
    a, b = x[ic], x[np.minimum(ic + 1, n - 1)]
    out = a + (b - a) * r                                           # float32, no contraction
    out[top] = x[n - 1]
    return out.astype(np.float32)


def ref_pitch(s, rho, alpha, warp_psd):
    """expected rows after pitch_formant, and the frames whose VTMAGN carries the log10 term"""
    F = len(s[A.A_F0])
    rho = np.ones(F, np.float32) if rho is None else np.asarray(rho, np.float32)
    alpha = np.ones(F, np.float32) if alpha is None else np.asarray(alpha, np.float32)
    out = {aid: v.copy() for aid, v in s.items()}
    comp = np.zeros(F, bool)
    for g in range(F):
        rh, al = rho[g], alpha[g]
        if rh == 1 and al == 1:
            continue
        if warp_psd and al != 1:
            out[A.A_PSD][g] = warp_np(s[A.A_PSD][g], al)
        if s[A.A_F0][g] == 0:
            continue
        out[A.A_F0][g] = s[A.A_F0][g] * rh                          # float32 product
        w = warp_np(s[A.A_VTMAGN][g], al) if al != 1 else s[A.A_VTMAGN][g].copy()
        out[A.A_VTMAGN][g] = (w.astype(np.float64) - 20.0 * np.log10(np.float64(rh))).astype(np.float32)
        out[A.A_NHAR][g] = 0
        out[A.A_HAS_HM][g] = 0
        comp[g] = rh != 1
    return out, comp


def assert_pitch_rows(got, want, comp, where=""):
    for aid in ROWS:
        if aid == A.A_VTMAGN:
            continue
        bad = np.flatnonzero((bits(got[aid]) != bits(want[aid])).reshape(len(got[aid]), -1).any(1))
        assert bad.size == 0, (where, aid, bad[:8])
    gv, wv = got[A.A_VTMAGN], want[A.A_VTMAGN]
    assert beq(gv[~comp], wv[~comp]), (where, np.flatnonzero((bits(gv) != bits(wv)).any(1) & ~comp)[:8])
    ulp = np.abs(gv[comp].astype(np.float64) - wv[comp]) / np.spacing(np.abs(wv[comp]))
    worst = float(ulp.max()) if ulp.size else 0.0
    assert worst <= 1.0, (where, worst)
    return worst, int((bits(gv[comp]) != bits(wv[comp])).sum())


def random_ratios(rng, F):
    """per-frame ratios with exact ones mixed in: untouched frames, pure formant and pure pitch edits"""
    rho = rng.uniform(0.5, 2.0, F).astype(np.float32)
    alpha = rng.uniform(0.7, 1.4, F).astype(np.float32)
    kind = rng.integers(0, 5, F)
    rho[(kind == 0) | (kind == 1)] = 1.0                  # 0: untouched, 1: formant only
    alpha[(kind == 0) | (kind == 2)] = 1.0                # 2: pitch only
    rho[:9] = 1.0; alpha[:9] = 1.0                        # a run of untouched frames covering whole groups of four
    return rho, alpha


@pytest.mark.parametrize("warp_psd", [False, True])
def test_rows_match_the_rules(ctx, warp_psd):
    b, _ = analysed(ctx)
    rng = np.random.default_rng(21 + warp_psd)
    F = b.layout.total_frames
    s = rows_of(b)
    rho, alpha = random_ratios(rng, F)
    b.pitch_formant(rho, alpha, warp_psd=warp_psd)
    ctx.sync()
    got = rows_of(b)
    b.close()
    want, comp = ref_pitch(s, rho, alpha, warp_psd)
    worst, n_ulp = assert_pitch_rows(got, want, comp, "warp_psd=%d" % warp_psd)
    voiced = s[A.A_F0] != 0
    touched = (rho != 1) | (alpha != 1)
    # every branch of the rules was exercised, and the edit did move the rows
    assert (voiced & ~touched).sum() > 10 and (~voiced & touched & (alpha != 1)).sum() > 3
    assert (voiced & (rho == 1) & (alpha != 1)).sum() > 10 and (voiced & (rho != 1) & (alpha == 1)).sum() > 10
    assert not beq(got[A.A_VTMAGN], s[A.A_VTMAGN]) and not beq(got[A.A_F0], s[A.A_F0])
    assert beq(got[A.A_PSD], s[A.A_PSD]) != warp_psd
    report("pitch_rows_psd%d" % warp_psd, dict(frames=F, edited_voiced=int((voiced & touched).sum()),
                                                vtmagn_ulp_max=worst, vtmagn_entries_off_by_one_ulp=n_ulp))


def test_identity_leaves_every_row_and_the_output(ctx):
    b, _ = analysed(ctx)
    F = b.layout.total_frames
    so = llsm.make_soptions(FS)
    s = rows_of(b)
    b.pitch_formant()
    b.pitch_formant(np.ones(F), np.ones(F), warp_psd=True)
    b.pitch_formant(1.0, 1.0, warp_psd=False)
    ctx.sync()
    got = rows_of(b)
    for aid in ROWS:
        assert beq(got[aid], s[aid]), aid

    def chain(edit):
        for aid in ROWS:
            b.upload(aid, s[aid])
        b.phasepropagate(-1)
        if edit:
            b.pitch_formant(np.ones(F), np.ones(F), warp_psd=True)
        b.tolayer0(True); b.phasepropagate(+1); b.synthesize(so, seed=4)
        return [b.download(k) for k in (A.A_Y, A.A_YSIN, A.A_YNOISE)]

    ya, yb = chain(True), chain(False)
    b.close()
    for u, v in zip(ya, yb):
        assert u.shape == v.shape and beq(u, v)


def test_edit_is_batch_invariant(ctx):
    ao = llsm.make_aoptions(f0_refine=0)
    rng = np.random.default_rng(31)
    n = rng.integers(1, 300, 64).astype(np.int32)
    src, rows = synthetic_src(ctx, ao, n, 2)
    off = src.frm_off
    F = int(off[-1])
    rho, alpha = random_ratios(rng, F)
    src.pitch_formant(rho, alpha, warp_psd=True)
    ctx.sync()
    whole = rows_of(src)
    for u in (0, 1, 17, 40, 63, int(np.argmin(n))):
        one = llsm.Batch(ctx, ao, FS, [0], [n[u]]); one.enable_layer1(1024)
        for aid in ROWS:
            one.upload(aid, rows[aid][off[u]:off[u + 1]])
        one.pitch_formant(rho[off[u]:off[u + 1]], alpha[off[u]:off[u + 1]], warp_psd=True)
        ctx.sync()
        alone = rows_of(one)
        for aid in ROWS:
            assert beq(alone[aid], whole[aid][off[u]:off[u + 1]]), (u, aid)
        one.close()
    want, comp = ref_pitch(rows, rho, alpha, True)
    assert_pitch_rows(whole, want, comp, "synthetic")
    src.close()


def test_refusals_write_nothing(ctx):
    L = llsm.load()
    ao = llsm.make_aoptions(f0_refine=0)
    b, _ = synthetic_src(ctx, ao, [20, 30], 4)
    no_l1 = llsm.Batch(ctx, ao, FS, [0, 0], [20, 30])
    before, before0 = rows_of(b), rows_of(no_l1, l1=False)
    ones = np.ones(50, np.float32)

    def call(bb, rho=None, alpha=None, flags=0):
        r = None if rho is None else np.ascontiguousarray(rho, np.float32)
        a = None if alpha is None else np.ascontiguousarray(alpha, np.float32)
        rc = L.llsm_gpu_batch_pitch_formant(bb, None if r is None else r.ctypes.data_as(llsm.P_fp),
                                            None if a is None else a.ctypes.data_as(llsm.P_fp), flags)
        return rc, L.llsm_gpu_last_error().decode()

    bad = lambda i, v: np.where(np.arange(50) == i, np.float32(v), ones * 1.5).astype(np.float32)
    cases = {
        "NULL batch": ((None, ones * 1.5, None, 0), "NULL"),
        "no layer 1": ((no_l1.h, ones * 1.5, None, 0), "layer 1"),
        "flag 2": ((b.h, ones * 1.5, None, 2), "flag"),
        "flag -1": ((b.h, ones * 1.5, None, -1), "flag"),
        "rho NaN": ((b.h, bad(7, np.nan), None, 0), "frame 7"),
        "rho inf": ((b.h, bad(49, np.inf), None, 0), "frame 49"),
        "rho > 16": ((b.h, bad(0, 16.001), None, 0), "frame 0"),
        "rho < 1/16": ((b.h, bad(22, 0.0624), None, 0), "frame 22"),
        "rho 0": ((b.h, bad(3, 0.0), None, 0), "frame 3"),
        "alpha NaN": ((b.h, None, bad(30, np.nan), 1), "frame 30"),
        "alpha -inf": ((b.h, None, bad(31, -np.inf), 1), "frame 31"),
        "alpha > 4": ((b.h, ones * 1.5, bad(11, 4.01), 1), "frame 11"),
        "alpha < 1/4": ((b.h, ones * 1.5, bad(12, 0.249), 0), "frame 12"),
    }
    for name, ((h, r, a, f), needle) in cases.items():
        rc, msg = call(h, r, a, f)
        assert rc == -1 and msg.startswith("llsm_gpu_batch_pitch_formant:") and needle in msg, (name, rc, msg)
        if "rho" in name:
            assert "f0_ratio" in msg, (name, msg)
        if "alpha" in name:
            assert "formant_ratio" in msg, (name, msg)
    ctx.sync()
    after, after0 = rows_of(b), rows_of(no_l1, l1=False)
    for aid in ROWS:
        assert beq(after[aid], before[aid]), aid
    for aid in before0:
        assert beq(after0[aid], before0[aid]), aid
    # the ends of both ranges are accepted
    edge = np.where(np.arange(50) % 2 == 0, 16.0, 1.0 / 16.0).astype(np.float32)
    edge_a = np.where(np.arange(50) % 3 == 0, 4.0, 0.25).astype(np.float32)
    rc, msg = call(b.h, edge, edge_a, 1)
    assert rc == 0, msg
    ctx.sync()
    want, comp = ref_pitch(before, edge, edge_a, True)
    assert_pitch_rows(rows_of(b), want, comp, "edges")
    b.close(); no_l1.close()


# ------------------------------------------------------------------ end to end on arctic_a0001
def acf_f0(seg, fs, lo=50.0, hi=700.0):
    seg = seg - seg.mean()
    r = np.correlate(seg, seg, "full")[len(seg) - 1:]
    a, b = int(fs / hi), int(fs / lo)
    k = a + int(np.argmax(r[a:b]))
    d = (r[k - 1] - r[k + 1]) / (2 * (r[k - 1] - 2 * r[k] + r[k + 1]))
    return fs / (k + d)


def centroid(y, fs, nfft=2048):
    w = np.hanning(nfft)
    segs = [y[i:i + nfft] * w for i in range(0, len(y) - nfft, nfft // 2)]
    p = np.mean(np.abs(np.fft.rfft(segs, axis=1)) ** 2, axis=0)
    f = np.fft.rfftfreq(nfft, 1 / fs)
    return float((f * p).sum() / p.sum())


def arctic(ctx):
    x, fs = read_wav(os.path.join(GOLDEN, "arctic_a0001.wav"))
    f0 = np.load(os.path.join(GOLDEN, "arctic_a0001_f0_hop128.npy")).astype(np.float32)
    ao = llsm.make_aoptions(thop=128.0 / fs, f0_refine=0)
    return x, f0, fs, ao


def edited_chain(ctx, rho, alpha, warp_psd, numpy_edit=False, edit=True):
    """analyse arctic_a0001, layer 1, phasepropagate(-1); the rows go to a fresh batch, where the edit is made (on the
    device, or in numpy before the upload); then tolayer0(1), phasepropagate(+1), synthesise.  Returns (y, y_sin,
    y_noise), the F0 row as analysed, the rows after tolayer0, and the sampling rate."""
    L = llsm.load()
    x, f0, fs, ao = arctic(ctx)
    so = llsm.make_soptions(fs)
    F = len(f0)
    a = llsm.Batch(ctx, ao, fs, [len(x)], [F])
    a.upload(A.A_X, x); a.upload(A.A_F0, f0)
    a.analyze(); a.tolayer1(NFFT)
    f0a = a.download(A.A_F0)
    a.phasepropagate(-1)
    s = rows_of(a)
    a.close()
    if edit and numpy_edit:
        s, _ = ref_pitch(s, llsm.per_frame_ratio(rho, [F]), llsm.per_frame_ratio(alpha, [F]), warp_psd)
    b = llsm.Batch(ctx, ao, fs, [len(x)], [F])
    b.upload(A.A_X, x); b.enable_layer1(NFFT)
    L.llsm_gpu_batch_set_maxnhar_conf(b.h, 60)
    for aid in ROWS:
        b.upload(aid, s[aid])
    if edit and not numpy_edit:
        b.pitch_formant(rho, alpha, warp_psd=warp_psd)
    b.tolayer0(True)
    after = rows_of(b)
    b.phasepropagate(+1); b.synthesize(so, seed=7)
    ys = [b.download(k) for k in (A.A_Y, A.A_YSIN, A.A_YNOISE)]
    ctx.sync()
    b.close()
    return ys, f0a, after, fs


def f0_ratio_median(y1, y0, f0a, fs, hop=128):
    """median over frames deep inside voiced runs of acf F0 of y1 over that of y0"""
    v = f0a > 0
    deep = np.array([v[max(0, i - 6):i + 7].all() for i in range(len(v))])
    idx = np.flatnonzero(deep)[::3]
    rat = [acf_f0(y1[i * hop - 1024:i * hop + 1024], fs) / acf_f0(y0[i * hop - 1024:i * hop + 1024], fs)
           for i in idx if i * hop >= 1024 and i * hop + 1024 <= min(len(y0), len(y1))]
    return float(np.median(rat)), len(rat)


@pytest.mark.parametrize("rho", [1.5, 0.7])
def test_end_to_end_pitch_shift_of_arctic(ctx, rho):
    y0, f0a, _, fs = edited_chain(ctx, None, None, False, edit=False)
    yd, _, dev_rows, _ = edited_chain(ctx, rho, None, False)
    yh, _, _, _ = edited_chain(ctx, rho, None, False, numpy_edit=True)
    errs = [rel_rms(a, b) for a, b in zip(yd, yh)]
    med, n = f0_ratio_median(yd[0], y0[0], f0a, fs)
    # tolayer0 on the shifted frames: NHAR = min(NVSPHSE, maxnhar_conf, floor(fnyq / F0')) (the documented band limit)
    f0e, nv = dev_rows[A.A_F0], dev_rows[A.A_NVSPHSE]
    vo = (f0e > 0) & (nv > 0)
    nq = (np.float32(fs / 2) / f0e[vo]).astype(np.int32)
    want_nhar = np.maximum(0, np.minimum.reduce([nv[vo], np.full(vo.sum(), 60), nq, np.full(vo.sum(), dev_rows[A.A_AMPL].shape[1])]))
    m = dict(rho=rho, rel_rms_y=errs[0], rel_rms_ysin=errs[1], rel_rms_ynoise=errs[2], f0_ratio_median=med, frames=n,
             nhar_mismatch=int((dev_rows[A.A_NHAR][vo] != want_nhar).sum()), voiced=int(vo.sum()))
    report("pitch_arctic_%g" % rho, m)
    assert all(np.all(np.isfinite(y)) for y in yd), m
    assert len(yd[0]) == len(y0[0]), m
    assert max(errs) <= 1e-4, m
    assert n >= 20 and abs(med / rho - 1) <= 0.02, m
    assert m["nhar_mismatch"] == 0 and vo.sum() > 50, m
    assert np.all(dev_rows[A.A_HAS_HM][vo] == 1), m


def test_formant_shift_moves_the_spectrum_up(ctx):
    y0, f0a, _, fs = edited_chain(ctx, None, None, False, edit=False)
    yd, _, _, _ = edited_chain(ctx, None, 1.2, True)
    yh, _, _, _ = edited_chain(ctx, None, 1.2, True, numpy_edit=True)
    errs = [rel_rms(a, b) for a, b in zip(yd, yh)]
    med, n = f0_ratio_median(yd[0], y0[0], f0a, fs)
    c0, c1 = centroid(y0[0], fs), centroid(yd[0], fs)
    m = dict(rel_rms_y=errs[0], rel_rms_ysin=errs[1], rel_rms_ynoise=errs[2], f0_ratio_median=med, frames=n,
             centroid_hz=c0, centroid_edited_hz=c1)
    report("formant_arctic_1.2", m)
    assert all(np.all(np.isfinite(y)) for y in yd), m
    assert max(errs) <= 1e-4, m
    assert n >= 20 and abs(med - 1) <= 0.02, m
    assert c1 > 1.02 * c0, m


def test_c_host_shifts_pitch_through_the_batch_api(tmp_path):
    """tests/c_host/pitch_batch_host.c: the whole device chain through llsm_gpu.h alone, built with the flags of the
    other C-host tests"""
    from test_c_host import CFLAGS, LIBDIR
    llsm.load()
    exe = str(tmp_path / "pitch_batch_host")
    subprocess.check_call(CFLAGS + ["-o", exe, os.path.join(HERE, "c_host", "pitch_batch_host.c"),
                                    "-L" + LIBDIR, "-l:libllsm2_amd.so", "-Wl,-rpath," + LIBDIR, "-lm"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "pitch_batch ok" in out.stdout, out.stdout + out.stderr
