"""What the alignment test modules share (tests/test_align*_host.py, tests/test_gpu_align*.py): the caps and the generated
cases that a host module and its GPU twin both check, and the helpers of the GPU modules -- tiny batches with synthetic
LLSM_GPU_CODE, bit comparisons, and the cutter of the planes 6, 9, 12 and 13 of llsm_gpu_batch_debug_plane.

Batches are tiny: layer 1 at nfft 128 and the coder at orders 64 + 5 (72 columns) enabled on batches without samples, and
synthetic LLSM_GPU_CODE rows uploaded."""
import numpy as np

import libllsm2_amd as llsm
import align_reference as aref
import align_slope_reference as sref
import align_band_slope_reference as kref

# ---------------------------------------------------------------- caps and generated cases
DIFFER_CAP = 0.005              # share of all frames on which float32 may leave the float64 chain
COST_REL = 1e-5
SEEDS = range(12)
FULL_SIZES = [(200, 170), (64, 65), (129, 63), (300, 410)]          # tests/test_align_host.py and its GPU twin
BAND_SIZES = [(120, 150), (200, 200), (150, 97), (257, 300)]        # tests/test_align_band_host.py and its GPU twin
SLOPE_SIZES = [(200, 170), (64, 65), (129, 90), (300, 410)]         # tests/test_align_slope_host.py and its GPU twin

_full_cases = {}
_slope_cases = {}


def full_case(size, seed):
    """(float32 chain, float64 chain, truth) of one generated pair, each (pos, cost); computed once"""
    key = (size, seed)
    if key not in _full_cases:
        A, B, truth = aref.make(seed, size[0], size[1], 24, 0.3)
        A = A.astype(np.float32); B = B.astype(np.float32)
        _full_cases[key] = (aref.align(A, B, 0, 24, step_cost=1.0), aref.align(A, B, 0, 24, step_cost=1.0, dtype=np.float64), truth)
    return _full_cases[key]


def slope_case(size, seed):
    """(float32 chain, float64 chain, truth, float32 chain of rules D1 - D3) of one generated pair, each (pos, cost)"""
    key = (size, seed)
    if key not in _slope_cases:
        A, B, truth = aref.make(seed, size[0], size[1], 24, 0.3)
        A = A.astype(np.float32); B = B.astype(np.float32)
        _slope_cases[key] = (sref.align(A, B, 0, 24, step_cost=1.0), sref.align(A, B, 0, 24, step_cost=1.0, dtype=np.float64), truth,
                             aref.align(A, B, 0, 24, step_cost=1.0))
    return _slope_cases[key]


def slope_properties(pos, na, nb):
    """what follows from L4 for the positions of any plane"""
    lo, hi = sref.rows(na, nb)
    assert not np.any(np.isnan(pos)) and pos[0] == 0 and pos[-1] >= nb - 1.5 and pos[-1] <= nb - 1
    d1 = np.diff(pos)
    assert np.all(d1 >= 0) and np.all(d1 <= 2), (na, nb, pos)
    assert np.all(pos[2:] - pos[:-2] >= 1), (na, nb, pos)
    assert np.all((pos * 2) % 1 == 0)                               # a row spans one column or two
    assert np.all(pos >= lo - 1) and np.all(pos <= hi + 1)            # (a cell between the ends of a move may lie one outside)


def band_slope_properties(pos, na, nb, band):
    """what follows from K4 as from L4, and the band"""
    assert not np.any(np.isnan(pos)) and pos[0] == 0 and pos[-1] >= nb - 1.5 and pos[-1] <= nb - 1
    d1 = np.diff(pos)
    assert np.all(d1 >= 0) and np.all(d1 <= 2), (na, nb, pos)
    assert np.all(pos[2:] - pos[:-2] >= 1), (na, nb, pos)
    assert np.all((pos * 2) % 1 == 0)                               # a row spans one column or two
    p, q = kref.band_rows(na, nb, band)
    assert np.all(pos >= np.array(p)) and np.all(pos <= np.array(q))


# ---------------------------------------------------------------- the GPU modules' batches and comparisons
FS = 44100.0
NFFT, OSP, OBAP, DIM = 128, 64, 5, 72


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def beq(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(bits(a), bits(b))


def same(x, y):
    """bit for bit, or both NaN"""
    x = np.asarray(x, np.float32); y = np.asarray(y, np.float32)
    return x.shape == y.shape and bool(np.all((bits(x) == bits(y)) | (np.isnan(x) & np.isnan(y))))


def slices(code, n):
    off = np.concatenate([[0], np.cumsum(n)])
    return [code[off[k]:off[k + 1]] for k in range(len(n))]


def coded(ctx, nfrm, code=None, coder=(OSP, OBAP)):
    """a batch without samples whose utterances have nfrm frames, layer 1 and the coder enabled, CODE uploaded"""
    b = llsm.Batch(ctx, llsm.make_aoptions(f0_refine=0), FS, [0] * len(nfrm), nfrm)
    b.enable_layer1(NFFT)
    if coder:
        b.enable_coder(*coder)
        if code is not None:
            b.upload(llsm.A_CODE, code)
    return b


def random_code(seed, n, integer=False):
    """n coder vectors: normal features (small integers with `integer`, so that accumulated costs tie often), the voicing
    column mixed from 0, 1 and values next to the threshold"""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((n, DIM)) * 3
    if integer:
        c = np.round(c / 3)
    c = c.astype(np.float32)
    c[:, 0] = rng.choice(np.array([0, 1, 1, 0.5, 0.50000006], np.float32), n)
    return c


def rows_of(b, code):
    return [code[int(b.frm_off[u]):int(b.frm_off[u + 1])] for u in range(b.layout.n_utt)]


def planes_of(b, which, rows, widths):
    """plane `which` (6, 9, 12 or 13) of batch b cut into the planes [rows[p]][widths[p]] of the pairs of the last call: a
    width is nb of a whole matrix, 2 band + 1 of a band plane"""
    flat = b.debug_plane(which)
    assert flat.shape == (sum(n * m for n, m in zip(rows, widths)),)
    out, at = [], 0
    for n, m in zip(rows, widths):
        out.append(flat[at:at + n * m].reshape(n, m)); at += n * m
    return out


def band_widths(bands):
    return [2 * w + 1 for w in bands]


def all_arrays(b):
    ids = [a for a in range(llsm.A_NARRAYS) if b.L.llsm_gpu_batch_array_bytes(b.h, a) > 0]
    return {a: b.download(a) for a in ids}
