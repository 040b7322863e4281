"""Rule P1 of llsm_gpu_batch_pool_code and rules Y1 - Y5 of llsm_gpu_batch_align_pyramid (llsm_gpu.h) restated in numpy: the
reference of tests/test_align_pyramid_host.py and tests/test_gpu_align_pyramid.py.  P1 is an explicit ascending loop of
float32 additions and one float32 division, not np.mean (which sums pairwise); the chain stands on the references of the
calls it is made of -- align_reference (D1 - D3), align_slope_reference (L1 - L4) and align_around_reference (the centre line
and A1 - A3) -- and adds only the order of the steps and the band of Y4."""
import numpy as np

import align_reference as aref
import align_slope_reference as sref
import align_around_reference as rref


def pool_frames(n, factor):
    return (n + factor - 1) // factor


def pool(code, factor):
    """P1: [ceil(n / factor)][dim] float32 from the rows [n][dim] of one utterance"""
    code = np.asarray(code, np.float32)
    n = len(code)
    out = np.zeros((pool_frames(n, factor),) + code.shape[1:], np.float32)
    with np.errstate(all="ignore"):
        for k in range(len(out)):
            lo, hi = k * factor, min(n, (k + 1) * factor)
            s = np.zeros(code.shape[1:], np.float32)
            for j in range(lo, hi):
                s = s + code[j]
            out[k] = s / np.float32(hi - lo)
    assert out.dtype == np.float32
    return out


def coarse(fa, fb, factor, slope, first, count, step_cost=0.0, voicing_cost=0.0):
    """Y1 - Y2: (pos_c, the pooled rows of a, those of b)"""
    pa, pb = pool(fa, factor), pool(fb, factor)
    run = sref.align if slope else aref.align
    return run(pa, pb, first, count, step_cost=step_cost, voicing_cost=voicing_cost)[0], pa, pb


def band_min(center, nb, slope):
    """llsm_gpu_align_around_min: the closed form of A1 without the slope pattern, else the bands tried in turn"""
    return rref.band_min(center, nb, 1) if slope else rref.band_min_plain(center, nb)


def line_and_band(pos_c, ncb, na, nb, factor, margin, slope):
    """Y3 - Y4: (center int64 [na], band)"""
    center = rref.center_line(pos_c, ncb, na, nb)
    return center, max(min(margin * factor, nb - 1), band_min(center, nb, slope))


def align(fa, fb, factor, margin, slope, first, count, step_cost=0.0, voicing_cost=0.0):
    """Y1 - Y5: (pos, cost, center, band)"""
    na, nb = len(fa), len(fb)
    pos_c, _, pb = coarse(fa, fb, factor, slope, first, count, step_cost, voicing_cost)
    center, band = line_and_band(pos_c, len(pb), na, nb, factor, margin, slope)
    pos, cost, _ = rref.align(fa, fb, center, band, slope, first, count, step_cost, voicing_cost)
    return pos, cost, center, band
