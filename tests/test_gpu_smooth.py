"""-m gpu: smoothing of parameter tracks around joins (llsm_gpu_batch_smooth) against the numpy restatement of rules
S1 - S9 of llsm_gpu.h in tests/smooth_reference.py.  Every comparison is bit for bit.  That bound is derived, not measured:
the products w x are exact in float64 (an integer below 2^6 times a float32), the order of the additions is part of the
rule, the division and the rounding to float32 are correctly rounded on both sides, and the library is built with
-ffp-contract=off -fno-fast-math.  A differing bit means the kernel adds in another order.
The kernel works in tiles of 16 listed frames (kSmoothTile of csrc/kernels.h); the shapes here straddle that."""
import os
import subprocess

import numpy as np
import pytest

import libllsm2_amd as llsm
import smooth_reference as ref
from conftest import FS
from test_gpu_retime import ROWS, analysed, beq, bits, rows_of, synthetic_src

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
A = llsm
TILE = 16
NFRM = np.array([1, 2, 3, 40, 7, 70], np.int32)           # 123 frames: a multiple neither of four nor of the tile
OFF = np.concatenate([[0], np.cumsum(NFRM)])
FTOT = int(OFF[-1])
SINGLE = (llsm.SMOOTH_F0, llsm.SMOOTH_RD, llsm.SMOOTH_VTMAGN, llsm.SMOOTH_PSD, llsm.SMOOTH_EDC)


@pytest.fixture(scope="module")
def ctx():
    c = llsm.Context(0)
    yield c
    c.close()


def make_batch(ctx, npsd=256, nfrm=NFRM, rows=None, seed=5):
    """synthetic_src's batch; utterance 3 all voiced and utterance 5 two long voiced runs around an unvoiced one, so that
    windows of radius 32 are cut by the utterance and by a voicing change as well as by the short runs of the other
    utterances; or the given rows"""
    ao = llsm.make_aoptions(f0_refine=0, npsd=npsd)
    b, r = synthetic_src(ctx, ao, nfrm, seed)
    if rows is None and len(nfrm) == len(NFRM):
        f0 = r[A.A_F0]
        rng = np.random.default_rng(seed + 1)
        f0[OFF[3]:OFF[4]] = rng.uniform(80, 300, 40)
        f0[OFF[5]:OFF[6]] = rng.uniform(80, 300, 70)
        f0[OFF[5] + 30:OFF[5] + 38] = 0
        b.upload(A.A_F0, f0)
    if rows is not None:
        for aid in ROWS:
            b.upload(aid, rows[aid])
        r = rows
    return b, {aid: np.array(v, copy=True) for aid, v in r.items()}, ao


def radii_under_test():
    """radii from {0 x many, 1, 2, 5, 32} with the cases the kernel can get wrong"""
    rng = np.random.default_rng(11)
    r = rng.choice([0, 0, 0, 0, 0, 0, 1, 2, 5, 32], FTOT).astype(np.int32)
    r[OFF[5] + 8:OFF[5] + 8 + 2 * TILE + 5] = rng.choice([1, 2, 5, 32], 2 * TILE + 5)   # a run longer than two tiles
    r[OFF[0]] = 5; r[OFF[1]:OFF[2]] = [32, 5]; r[OFF[2]:OFF[3]] = [2, 32, 5]            # radii larger than the utterance
    for u in (3, 4, 5):                                                                 # both sides of utterance bounds
        r[OFF[u] - 1] = 5; r[OFF[u]] = 32
    r[OFF[3] + 20] = 32                                                                 # clipped by both ends of 40 frames
    r[OFF[6] - 1] = 32                                                                  # the batch's last frame
    r[OFF[3] + 5:OFF[3] + 9] = 0                                                        # a gap inside a run
    return r


_REF = {}


def reference(s, radius, flags, key):
    """the expected rows, computed once per (shape, flags) and handed out as copies"""
    if key not in _REF:
        _REF[key] = ref.smooth(s, NFRM, radius, flags)
    want, hit = _REF[key]
    return {aid: v.copy() for aid, v in want.items()}, hit.copy()


def assert_rows(got, want, where):
    for aid in ROWS:
        bad = np.flatnonzero((bits(got[aid]) != bits(want[aid])).reshape(len(got[aid]), -1).any(1))
        assert bad.size == 0, (where, aid, bad[:8])


# ------------------------------------------------------------------ 1: the rules, bit for bit
@pytest.mark.parametrize("npsd", [256, 129])
@pytest.mark.parametrize("flags", (llsm.SMOOTH_ALL,) + SINGLE)
def test_rows_match_the_rules_bit_for_bit(ctx, npsd, flags):
    b, s, _ = make_batch(ctx, npsd)
    radius = radii_under_test()
    b.smooth(radius, flags)
    ctx.sync()
    got = rows_of(b)
    b.close()
    want, hit = reference(s, radius, flags, (npsd, flags))
    assert_rows(got, want, (npsd, flags))
    for aid in ref.NEVER:                                     # rule S7 (and AMPL / PHSE of rule S5)
        assert beq(got[aid], s[aid]), aid
    # the cases were there, and the edit did move the rows
    voiced = s[A.A_F0] != 0
    assert (hit & voiced).sum() > 20 and (hit & ~voiced).sum() > 2 and ((radius > 0) & ~hit).sum() >= 1
    assert hit[OFF[3] - 1] or hit[OFF[3]] or hit[OFF[4] - 1] or hit[OFF[5]]
    for bit, aid in ref.TRACKS:
        assert beq(got[aid], s[aid]) == (not flags & bit), (flags, aid)
    edited = hit & voiced if flags & 7 else np.zeros(FTOT, bool)
    assert np.all(got[A.A_NHAR][edited] == 0) and np.all(got[A.A_HAS_HM][edited] == 0)
    assert beq(got[A.A_NHAR][~edited], s[A.A_NHAR][~edited]) and beq(got[A.A_HAS_HM][~edited], s[A.A_HAS_HM][~edited])


# ------------------------------------------------------------------ 2: identities that need no reference
def runs_of(f0, nfrm):
    """(first, last + 1) flat frames of every voicing run"""
    out, o = [], 0
    for n in nfrm:
        i = 0
        while i < n:
            j = i
            while j + 1 < n and (f0[o + j + 1] != 0) == (f0[o + i] != 0):
                j += 1
            out.append((o + i, o + j + 1))
            i = j + 1
        o += int(n)
    return out


def test_rows_constant_along_each_voicing_run_come_back_unchanged(ctx):
    b, s, _ = make_batch(ctx)
    for aid in (A.A_F0, A.A_RD, A.A_VTMAGN, A.A_PSD, A.A_EDC):
        for a, e in runs_of(s[A.A_F0], NFRM):
            s[aid][a:e] = s[aid][a]                           # (F0: the run's first value; zero stays zero)
        b.upload(aid, s[aid])
    radius = np.random.default_rng(3).choice([1, 2, 5, 32], FTOT).astype(np.int32)
    b.smooth(radius)
    ctx.sync()
    got = rows_of(b)
    b.close()
    # every partial sum is an exact integer multiple of the run's value, and so is the quotient
    for aid in ROWS:
        if aid not in (A.A_NHAR, A.A_HAS_HM):
            assert beq(got[aid], s[aid]), aid
    _, hit = ref.smooth(s, NFRM, radius)
    edited = hit & (s[A.A_F0] != 0)
    assert edited.sum() > 40 and np.all(got[A.A_NHAR][edited] == 0) and np.all(got[A.A_HAS_HM][edited] == 0)
    assert beq(got[A.A_NHAR][~edited], s[A.A_NHAR][~edited]) and beq(got[A.A_HAS_HM][~edited], s[A.A_HAS_HM][~edited])


def test_an_integer_ramp_comes_back_unchanged_where_the_window_is_whole(ctx):
    b, s, _ = make_batch(ctx)
    j = np.arange(FTOT, dtype=np.int64)

    def ramp(shape_tail, base):
        k = np.arange(int(np.prod(shape_tail)) or 1, dtype=np.int64).reshape(shape_tail or ())
        return (base + k % 7 + (k % 5 - 2) * j.reshape((-1,) + (1,) * len(shape_tail))).astype(np.float32)
    for aid, base in ((A.A_F0, 300), (A.A_RD, 3), (A.A_VTMAGN, -40), (A.A_PSD, -60), (A.A_EDC, 9)):
        s[aid] = ramp(s[aid].shape[1:], base)
        b.upload(aid, s[aid])
    assert np.all(s[A.A_F0] > 0)                              # F0 = 300 - 2 j: every frame voiced, one run per utterance
    radius = np.random.default_rng(4).choice([1, 2, 5, 32], FTOT).astype(np.int32)
    b.smooth(radius)
    ctx.sync()
    got = rows_of(b)
    b.close()
    whole = np.zeros(FTOT, bool)
    for u, n in enumerate(NFRM):
        i = np.arange(n)
        whole[OFF[u]:OFF[u + 1]] = (i - radius[OFF[u]:OFF[u + 1]] >= 0) & (i + radius[OFF[u]:OFF[u + 1]] <= n - 1)
    assert whole.sum() > 20 and (~whole).sum() > 10
    for aid in (A.A_F0, A.A_RD, A.A_VTMAGN, A.A_PSD, A.A_EDC):
        assert beq(got[aid][whole], s[aid][whole]), aid
    assert not beq(got[A.A_VTMAGN][~whole], s[A.A_VTMAGN][~whole])      # a clipped window does move a ramp
    want, _ = ref.smooth(s, NFRM, radius)
    assert_rows(got, want, "ramp")


# ------------------------------------------------------------------ 3: untouched means untouched
def test_untouched_means_untouched(ctx):
    b, s, _ = make_batch(ctx)
    ctx.set_profiling(True); ctx.reset_profile()
    try:
        b.smooth(np.zeros(FTOT, np.int32)); b.smooth(0); b.smooth(5, 0)
        ctx.sync()
        assert not any(k.startswith("k_smooth") for k in ctx.profile()), ctx.profile()
        got = rows_of(b)
        for aid in ROWS:
            assert beq(got[aid], s[aid]), aid
        # rule S3: a voiced frame between two unvoiced ones, and an unvoiced one between two voiced
        f0 = s[A.A_F0].copy()
        o = int(OFF[3])
        f0[o + 10:o + 17] = [0, 0, 150, 0, 170, 180, 0]
        b.upload(A.A_F0, f0); s[A.A_F0] = f0
        radius = np.zeros(FTOT, np.int32); radius[[o + 12, o + 13]] = 5
        b.smooth(radius)
        ctx.sync()
        prof = ctx.profile()
        assert prof["k_smooth_rows"][1] == 1 and prof["k_smooth_store"][1] == 1, prof
        got = rows_of(b)
        for aid in ROWS:
            assert beq(got[aid], s[aid]), aid
        radius[o + 14] = 5                                    # the same call does edit a frame with a neighbour
        b.smooth(radius)
        ctx.sync()
        got = rows_of(b)
        want, hit = ref.smooth(s, NFRM, radius)
        assert list(np.flatnonzero(hit)) == [o + 14]
        assert_rows(got, want, "S3")
    finally:
        ctx.set_profiling(False)
        b.close()


# ------------------------------------------------------------------ 4: a snapshot, not a sequential edit
def test_the_call_reads_a_snapshot(ctx):
    b, s, _ = make_batch(ctx)
    b.smooth(3)
    ctx.sync()
    got = rows_of(b)
    b.close()
    want, _ = ref.smooth(s, NFRM, np.full(FTOT, 3))
    seq, _ = ref.smooth(s, NFRM, np.full(FTOT, 3), in_place=True)
    assert_rows(got, want, "snapshot")
    assert not beq(seq[A.A_VTMAGN], want[A.A_VTMAGN]) and not beq(seq[A.A_F0], want[A.A_F0])


# ------------------------------------------------------------------ 5: batch invariance
def test_an_utterance_does_not_depend_on_the_rest(ctx):
    b, s, _ = make_batch(ctx, 129)
    radius = radii_under_test()
    b.smooth(radius)
    one, _, _ = make_batch(ctx, 129, NFRM[3:4], {aid: s[aid][OFF[3]:OFF[4]] for aid in ROWS})
    one.smooth(radius[OFF[3]:OFF[4]])
    ctx.sync()
    whole, alone = rows_of(b), rows_of(one)
    b.close(); one.close()
    for aid in ROWS:
        assert beq(alone[aid], whole[aid][OFF[3]:OFF[4]]), aid
    assert not beq(alone[A.A_VTMAGN], s[A.A_VTMAGN][OFF[3]:OFF[4]])


# ------------------------------------------------------------------ 6: refusals
def test_refusals_leave_the_batch_untouched(ctx):
    L = llsm.load()
    b, s, ao = make_batch(ctx)
    no_l1 = llsm.Batch(ctx, ao, FS, [0] * len(NFRM), NFRM)
    before0 = rows_of(no_l1, l1=False)

    def call(h, radius, flags):
        r = np.ascontiguousarray(radius, np.int32)
        rc = L.llsm_gpu_batch_smooth(h, r.ctypes.data_as(llsm.P_int), flags)
        return rc, L.llsm_gpu_last_error().decode()

    ok = np.full(FTOT, 2, np.int32)
    bad = lambda i, v: np.where(np.arange(FTOT) == i, v, 2).astype(np.int32)
    cases = {"radius -1": ((b.h, bad(7, -1), 31), "frame 7"), "radius 33": ((b.h, bad(122, 33), 31), "frame 122"),
             "radius 33 at 0": ((b.h, bad(0, 33), 1), "frame 0"),
             "flag 32": ((b.h, ok, 32), "flag"), "flag -1": ((b.h, ok, -1), "flag"), "flag 63": ((b.h, ok, 63), "flag"),
             "no layer 1": ((no_l1.h, ok, 31), "layer 1")}
    for name, (args, needle) in cases.items():
        rc, msg = call(*args)
        assert rc == -1 and msg.startswith("llsm_gpu_batch_smooth:") and needle in msg, (name, rc, msg)
    with pytest.raises(llsm.LlsmError):
        b.smooth(33)
    ctx.sync()
    after, after0 = rows_of(b), rows_of(no_l1, l1=False)
    for aid in ROWS:
        assert beq(after[aid], s[aid]), aid
    for aid in before0:
        assert beq(after0[aid], before0[aid]), aid
    # both ends of the range are accepted
    edge = np.where(np.arange(FTOT) % 2 == 0, 32, 0).astype(np.int32)
    rc, msg = call(b.h, edge, 31)
    assert rc == 0, msg
    ctx.sync()
    want, _ = ref.smooth(s, NFRM, edge)
    assert_rows(rows_of(b), want, "edges")
    b.close(); no_l1.close()


# ------------------------------------------------------------------ 7: end to end
def test_a_join_is_smoothed_end_to_end(ctx):
    src, ao = analysed(ctx)                                  # four utterances of 30 000 samples, layer 1
    so = llsm.make_soptions(FS)
    n, h = 80, 40                                             # first half: utterance 0 from frame 10, second: utterance 1 from 80
    pos = np.concatenate([10 + np.arange(h), 80 + np.arange(n - h)]).astype(np.float32)
    utt = np.repeat([0, 1], [h, n - h]).astype(np.int32)
    dst = llsm.Batch(ctx, ao, FS, [0], [n])
    dst.splice(src, pos, utt)
    ctx.sync()
    s = rows_of(dst)
    radius, joins = llsm.join_radii([n], pos, utt, reach=8)
    assert joins == 1 and radius[h - 1] == radius[h] == 8 and radius[h - 9] == radius[h + 8] == 0
    dst.smooth(radius)
    ctx.sync()
    got = rows_of(dst)
    want, hit = ref.smooth(s, [n], radius)
    assert_rows(got, want, "join")
    far = radius == 0
    assert far.sum() == n - 16
    for aid in ROWS:
        assert beq(got[aid][far], s[aid][far]), aid
    f0a, f0b = s[A.A_F0], got[A.A_F0]
    assert f0a[h - 1] > 0 and f0a[h] > 0 and hit[h - 1] and hit[h]
    before, after = abs(float(f0a[h]) - float(f0a[h - 1])), abs(float(f0b[h]) - float(f0b[h - 1]))
    print("F0 step across the join: %.3f Hz before, %.3f Hz after" % (before, after))
    assert after < before
    dst.tolayer0(True); dst.synthesize(so, seed=5)
    y = dst.download(A.A_Y).astype(np.float64)
    ctx.sync()
    hm, nv = dst.download(A.A_HAS_HM), dst.download(A.A_NVSPHSE)
    dst.close(); src.close()
    assert np.all(hm[(f0b > 0) & (nv > 0)] == 1)                         # tolayer0 rebuilt the harmonics the edit dropped
    assert y.size > 0 and np.all(np.isfinite(y)) and float(np.sqrt(np.mean(y ** 2))) > 1e-3


# ------------------------------------------------------------------ 8: the C host
def test_c_host_smooths_a_join_through_the_batch_api(tmp_path):
    """tests/c_host/smooth_batch_host.c: select's lists -> splice -> join_radii -> smooth -> tolayer0 -> synthesize through
    llsm_gpu.h alone, built with the flags of the other C-host tests"""
    from test_c_host import CFLAGS, LIBDIR
    llsm.load()
    exe = str(tmp_path / "smooth_batch_host")
    subprocess.check_call(CFLAGS + ["-o", exe, os.path.join(HERE, "c_host", "smooth_batch_host.c"),
                                    "-L" + LIBDIR, "-l:libllsm2_amd.so", "-Wl,-rpath," + LIBDIR, "-lm"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "smooth_batch ok" in out.stdout, out.stdout + out.stderr
    step = [ln for ln in out.stdout.splitlines() if ln.startswith("smooth_batch: F0 step")]
    assert len(step) == 1
    before, after = [float(v) for v in step[0].split(":")[2].replace("Hz", "").split("->")]
    assert after < before, step
