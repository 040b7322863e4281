"""The metric of tests/noise_filter_reference.py on the CPU: the yardstick of every utterance of every configuration the GPU
module runs (float32 build of the oracle against the float64 build, the float64 oracle's own excitation rounded to float32 as
stand-in for plane 15), the two conditions on the inputs, the value of KAPPA, the route every configuration is meant to
reach, and that the checker flags wrong candidates -- built with the same oracle on altered inputs."""
import math

import numpy as np
import pytest

import libllsm2_amd as llsm
import noise_filter_reference as R
from gpu_common import CONVENTION_NAMES

SEED = 3


def product_route(fused, npsd, thop, fs):
    return llsm.load().llsm_gpu_plan_index(17, int(fused), int(npsd), 0.0, thop, fs, 0.0)


@pytest.fixture(scope="module")
def table(o64, o32):
    """{config name: (config, [(utterance name, params, has, x, Ref)])}, computed once"""
    R.follow_product_conventions((o64, o32), CONVENTION_NAMES)   # every convention set: nothing is left to an earlier test
    out = {}
    for cfg in R.configurations(product_route).values():
        rows = []
        for name, p, has in R.make_utterances(cfg["fs"], cfg["thop"], cfg["npsd"], cfg["N"], cfg["nlong"], cfg["fnyq"]):
            x = R.excitation_stand_in(o64, p, cfg["fs"], SEED)
            rows.append((name, p, has, x, R.Ref(o64, o32, p, has, cfg["fs"], x)))
        out[cfg["name"]] = (cfg, rows)
    return out


def test_yardstick_table_and_input_conditions(table):
    bad = []
    print("\nconfiguration: worst Y_u, worst per-hop ratio, largest bound (utterance)")
    for cname, (cfg, rows) in table.items():
        assert all(ref.N == cfg["N"] for *_, ref in rows), cname
        wy = max(rows, key=lambda r: r[4].Y); wh = max(rows, key=lambda r: r[4].hop32); wb = max(rows, key=lambda r: r[4].bound)
        print("%-24s Y %6.1f (%s)  hop %5.1f (%s)  bound %6.1f (%s)" %
              (cname, wy[4].Y, wy[0], wh[4].hop32, wh[0], wb[4].bound, wb[0]))
        for name, p, has, x, ref in rows:
            bad += [(cname, name) + c for c in ref.conditions()]
            # the float32 oracle is inside its own bound by construction; the float64 oracle is at 0
            assert not R.judge(ref.y32.astype(np.float32), ref)["failed"] or ref.Y == 0, (cname, name)
            assert R.judge(ref.y64, ref)["a_units"] == 0
    assert not bad, bad


def test_inputs_hold_what_they_are_for(table):
    """dead partners of both kinds, uncovered samples inside an utterance, an all-dead and a frameless utterance"""
    for cname, (cfg, rows) in table.items():
        by = {name: (p, ref) for name, p, has, x, ref in rows}
        p, ref = by["dead"]
        assert ref.frame_rms[2] == 0 and ref.frame_rms[5] == 0 and ref.frame_rms[3] > 0 and ref.frame_rms[4] > 0
        zero = np.flatnonzero(ref.T == 0)
        inner = zero[(zero > ref.c[7]) & (zero < ref.c[-3])]
        assert inner.size, cname
        assert np.all(ref.y64[zero] == 0)
        assert not by["all_dead"][1].T.any() and by["frameless"][1].ny > 0 and not by["frameless"][1].T.any()
        assert np.all(by["steps"][1].frame_rms > 0)
        q, lo = by["quiet"][1], by["loud_before"][1]
        assert 500 < np.median(lo.frame_rms) / np.median(q.frame_rms) < 2000, cname


def test_kappa_is_four_times_the_float32_oracle(table):
    worst = max(ref.hop32 for cfg, rows in table.values() for *_, ref in rows)
    kappa = float(math.ceil(4.0 * worst))
    print("\nlargest per-hop ratio of the float32 oracle %.2f EPS -> KAPPA %g" % (worst, kappa))
    assert R.KAPPA == kappa, (worst, kappa)


def test_routes_of_the_configurations():
    """the kernel each configuration is meant to reach, fused wanted and not (llsm_gpu_plan_index case 17)"""
    seen = set()
    for cfg in R.configurations(product_route).values():
        got = product_route(1, cfg["npsd"], cfg["thop"], cfg["fs"])
        assert got == cfg["route"], (cfg["name"], got, cfg["route"])
        off = product_route(0, cfg["npsd"], cfg["thop"], cfg["fs"])
        assert off == (R.ROUTE_WF if cfg["N"] in R.FUSED_SIZES else cfg["route"]), (cfg["name"], off)
        seen.add(got)
    assert seen == {R.ROUTE_LDS, R.ROUTE_SCRATCH, R.ROUTE_FUSED + 1, R.ROUTE_FUSED + 12, R.ROUTE_FUSED + 14}, seen


# ---- wrong candidates: the same oracle on altered inputs ----

def _shift(x, k=1):
    y = np.zeros_like(x); y[k:] = x[:-k]
    return y


def wrong_candidates(o64, cfg, p, has, x, ref):
    fs = cfg["fs"]
    x64 = x.astype(np.float64)
    live = np.flatnonzero(ref.frame_rms > 0)
    k = int(live[len(live) // 2])
    f = lambda q=p, h=has, xx=x64: o64.filter_noise(q, fs, xx, h)[0]
    yield "excitation one sample late", f(xx=_shift(x64))
    prev = o64.lib.o_conv_mavg_half()
    assert prev == 3
    o64.set_convention("moving_avg_half", 2)
    try:
        yield "moving_avg_half 2 for 3", f()
    finally:
        o64.set_convention("moving_avg_half", prev)
    h2 = has.copy(); h2[k] ^= 1
    yield "PSDRES flag of frame %d flipped" % k, f(h=h2)
    q = p.copy(); h2 = has.copy()
    for a in (q.psd, q.psdres, h2):
        a[[2, 3]] = a[[3, 2]]
    yield "rows of the pair (2, 3) swapped", f(q=q, h=h2)
    q = p.copy(); q.fnyq = p.fnyq * p.npsd / (p.npsd - 1.0)
    yield "fnyq stretched by npsd / (npsd - 1)", f(q=q)
    q = p.copy(); q.psd[k] = -120.0
    yield "live frame %d dropped" % k, f(q=q)
    y = ref.y64.copy(); y[ref.edges[-2]:] = 0.0
    yield "last hop zeroed", y
    q = p.copy(); q.psd[np.arange(p.nfrm) != k] = -120.0
    yk = f(q=q)
    yield "span of frame %d one sample late" % k, ref.y64 - yk + _shift(yk)


def test_checker_flags_wrong_candidates(table, o64):
    """on the long utterance of every configuration each wrong candidate fails (a) or (b)"""
    missed = []
    for cname, (cfg, rows) in table.items():
        name, p, has, x, ref = rows[0]
        assert name == "steps"
        n = 0
        for what, y in wrong_candidates(o64, cfg, p, has, x, ref):
            m = R.judge(y, ref)
            n += 1
            if not ({"a", "b"} & set(m["failed"])):
                missed.append((cname, what, m["a_ratio"], m["b_ratio"]))
        assert n == 8
    assert not missed, missed


def test_checker_flags_values_where_nothing_may_be():
    """a value, a negative zero or a NaN where T is 0"""
    class Fake:
        ny = 6; y64 = np.zeros(6); T = np.array([0.0, 0, 1, 1, 0, 0]); edges = np.array([0, 3, 6]); bound = 10.0
    y = np.zeros(6, np.float32)
    assert not R.judge(y, Fake)["failed"]
    for v in (1e-30, -0.0, np.nan):
        z = y.copy(); z[4] = v
        assert R.judge(z, Fake)["failed"], v
    z = y.copy(); z[2] = 11 * R.EPS
    assert "a" in R.judge(z, Fake)["failed"]
