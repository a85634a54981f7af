"""tests/gaugefix_ref.py, the numpy restatement of src/gauge/gaugefix.nim, checks itself (no GPU): the gradient against a per-site
loop, gauge invariance of the plaquettes, gfMetric against the link trace of the transformed field, the parity structure of a
relax sweep -- and measures the yardstick and the iteration counts the GPU tests (tests/test_gpu_gaugefix.py) rely on."""
import numpy as np
import pytest

import gaugefix_ref as R
from qex_amd.layout import Layout


@pytest.fixture(scope="module")
def small():
    lo = Layout([4, 4, 4, 4])
    rng = np.random.default_rng(5)
    G = [R.random_su3(lo, 20 + mu) for mu in range(4)]
    t = R.random_su3(lo, 30) + 0.1 * (rng.standard_normal((lo.vol, 3, 3)) + 1j * rng.standard_normal((lo.vol, 3, 3)))   # not unitary
    return lo, G, t


@pytest.mark.parametrize("dirs", [R.COULOMB, R.LANDAU, (3, 1)])
def test_gradient_against_a_per_site_loop(small, dirs):
    lo, G, t = small
    gd = R.gradient(lo, G, t, dirs)
    want = np.zeros_like(gd)
    for s in range(lo.vol):
        x = lo.coord(s)
        for mu in dirs:
            xf, xb = list(x), list(x)
            xf[mu] += 1
            xb[mu] -= 1
            f, b = lo.index(xf), lo.index(xb)
            want[s] += G[mu][s] @ t[f].conj().T + (t[b] @ G[mu][b]).conj().T
    assert np.abs(gd - want).max() < 1e-13


def test_plaquettes_are_invariant_and_gfmetric_is_the_link_trace_of_the_transformed_field(small):
    lo, G, _ = small
    t = R.random_su3(lo, 31)
    Gt = R.gauge_transform(lo, G, t)
    assert np.abs(R.plaq(lo, Gt) - R.plaq(lo, G)).max() < 1e-13
    for dirs in (R.COULOMB, R.LANDAU):
        assert abs(R.gf_metric(lo, G, t, dirs) - R.link_trace(lo, Gt, dirs)) < 1e-13


def test_a_relaxE_sweep_leaves_the_odd_sites_bit_unchanged(small):
    lo, G, _ = small
    t = R.random_su3(lo, 32)
    t1 = t.copy()
    R.relax(lo, t1, R.gradient(lo, G, t, R.LANDAU), 0, 1.8)
    h = lo.vol // 2
    assert np.array_equal(t1[h:], t[h:]) and not np.array_equal(t1[:h], t[:h])
    assert np.abs(R.mul(t1, R.adj(t1)) - np.eye(3)).max() < 1e-13          # the SU(2) steps keep t unitary
    g = np.stack([R.rmat(m) for m in G], axis=1)
    _, info = R.get_gauge_fix_transform(lo, g, R.LANDAU, gstop=0, maxits=3)
    assert info["kinds"] == [1, 0, 1] and np.all(np.diff(R.full_history(info)[:, 0]) > 0)     # relaxO first; the trace grows


@pytest.mark.parametrize("dirs", [R.COULOMB, R.LANDAU])
@pytest.mark.parametrize("orf", [1.8, 1.0])
def test_yardstick_fp64_against_longdouble_over_40_relax_iterations(oracle, dirs, orf):
    """The recorded YARDSTICK rows of 4x6x10x6 are what this machine measures (they are a few 1e-15: the bound of the GPU tests,
    max(1e-12, 3 x yardstick), is 1e-12)."""
    lat = (4, 6, 10, 6)
    lo, g = R.warm_rotated(oracle, lat)
    t, i = R.get_gauge_fix_transform(lo, g, dirs, gstop=0, orf=orf, maxits=40)
    tl, il = R.get_gauge_fix_transform(lo, g, dirs, gstop=0, orf=orf, maxits=40, dtype=np.longdouble)
    dh = float(np.max(np.abs(R.full_history(i) / R.full_history(il) - 1)))
    dt = float(np.max(np.abs(t - tl)))
    print("yardstick %s %s orf %g: history %.3e, t %.3e" % (lat, dirs, orf, dh, dt))
    yh, yt = R.YARDSTICK[(lat, tuple(dirs), orf)]
    assert i["iters"] == il["iters"] == 40
    assert dh <= 2 * yh and dt <= 2 * yt and R.bound(dh) == R.bound(dt) == 1e-12


@pytest.mark.parametrize("dirs", [R.COULOMB, R.LANDAU])
def test_recorded_iteration_counts(oracle, dirs):
    """gstop = 1e-5 on 4x6x10x6: the count the GPU test compares with; the last 11 evaluations stay at gdsq <= gstop"""
    lat = (4, 6, 10, 6)
    lo, g = R.warm_rotated(oracle, lat)
    t, info = R.get_gauge_fix_transform(lo, g, dirs, gstop=1e-5, orf=1.8, maxits=5000)
    print("iterations %s %s: %d, gdsq %.3e" % (lat, dirs, info["iters"], info["gdsq"]))
    assert info["iters"] == R.REF_ITERS[(lat, tuple(dirs), 1e-5)] and info["gdsq"] <= 1e-5
    assert info["kinds"][-10:] == [2] * 10 and np.abs(R.mul(t, R.adj(t)) - np.eye(3)).max() < 1e-12


@pytest.mark.slow
def test_all_recorded_constants(oracle):
    """Every row of REF_ITERS, the 8^4 rows of YARDSTICK and GRANDOM_ITERS, re-measured (minutes: run with -m slow)."""
    for (lat, dirs, gstop), want in R.REF_ITERS.items():
        lo, g = R.warm_rotated(oracle, lat)
        _, info = R.get_gauge_fix_transform(lo, g, dirs, gstop=gstop, orf=1.8, maxits=5000)
        print("iterations %s %s %g: %d" % (lat, dirs, gstop, info["iters"]))
        assert info["iters"] == want and info["gdsq"] <= gstop
    for (lat, dirs, orf), (yh, yt) in R.YARDSTICK.items():
        if lat != (8, 8, 8, 8):
            continue
        lo, g = R.warm_rotated(oracle, lat)
        t, i = R.get_gauge_fix_transform(lo, g, dirs, gstop=0, orf=orf, maxits=40)
        tl, il = R.get_gauge_fix_transform(lo, g, dirs, gstop=0, orf=orf, maxits=40, dtype=np.longdouble)
        dh = float(np.max(np.abs(R.full_history(i) / R.full_history(il) - 1)))
        dt = float(np.max(np.abs(t - tl)))
        print("yardstick %s %s orf %g: history %.3e, t %.3e" % (lat, dirs, orf, dh, dt))
        assert dh <= 2 * yh and dt <= 2 * yt
    lo, g = R.grandom_rotated(oracle, (8, 8, 8, 8))
    for dirs, want in R.GRANDOM_ITERS.items():
        _, info = R.get_gauge_fix_transform(lo, g, dirs, gstop=1e-5, orf=1.8, maxits=5000)
        print("g.random 8^4 %s: %d iterations, met %.6f" % (dirs, info["iters"], info["met"]))
        assert info["iters"] == want
