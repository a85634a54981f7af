"""Coulomb / Landau gauge fixing on the device (qexhip_gauge_fix, qexhip_gauge_transform, qexhip_gauge_link_trace) against
tests/gaugefix_ref.py, the numpy restatement of src/gauge/gaugefix.nim.

Inputs: the oracle's gauge_warm(0.3) transformed by a random SU(3) field (gaugefix_ref.warm_rotated) on 8^4 and on 4x6x10x6
(unequal extents, a partial last tile).  Iteration counts of the reference and the yardstick of the 40-iteration comparison were
measured on the CPU and are recorded in gaugefix_ref.REF_ITERS / YARDSTICK.  Observed values are printed (pytest -s)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import gaugefix_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_INPUT, _REF40 = {}, {}


def _input(o, lat):
    if lat not in _INPUT:
        _INPUT[lat] = R.warm_rotated(o, lat)
    return _INPUT[lat]


def _ref40(o, lat, dirs, orf):
    key = (lat, dirs, orf)
    if key not in _REF40:
        lo, g = _input(o, lat)
        _REF40[key] = R.get_gauge_fix_transform(lo, g, dirs, gstop=0, orf=orf, maxits=40, keep=(39,))
    return _REF40[key]


def _ctx(lat, g, halo=False, emu_us=0):
    import qex_amd as q

    ctx = q.Context(list(lat))
    if halo:
        ctx.force_halo(True)
        ctx.set_option("emu_exchange_us", emu_us)
    q.gaugeSet(ctx, g)
    return ctx


@pytest.mark.parametrize("lat", R.LATS)
@pytest.mark.parametrize("dirs", [R.COULOMB, R.LANDAU])
@pytest.mark.parametrize("orf", [1.8, 1.0])
def test_fixed_relax_count_against_the_reference(oracle, lat, dirs, orf):
    """gstop = 0, maxits = 40: pure relax sweeps.  The 41 evaluations (met, gre, gro) agree with the reference to
    max(1e-12 relative, 3 x yardstick) and t to the same bound (absolute, elements are O(1)).  The yardstick -- fp64 against
    np.longdouble of the reference itself over these 40 iterations, measured on the CPU -- is at most 6.6e-15 (history) and 2.5e-15 (t)
    over the eight cases (gaugefix_ref.YARDSTICK), so the bound is 1e-12: a margin of ~150 x the yardstick.  The last sweep is
    relaxE: the odd sites are bit for bit those of the state after 39 iterations."""
    import qex_amd as q

    lo, g = _input(oracle, lat)
    tr, ir = _ref40(oracle, lat, dirs, orf)
    ctx = _ctx(lat, g)
    t39, i39 = q.getGaugeFixTransform(ctx, dirs, gstop=0.0, orf=orf, maxits=39)
    t, info = q.getGaugeFixTransform(ctx, dirs, gstop=0.0, orf=orf, maxits=40)
    assert info["iters"] == 40 and i39["iters"] == 39 and info["hist"].shape == (40, 3)
    yh, yt = R.YARDSTICK[(lat, dirs, orf)]
    h = np.vstack([info["hist"], [[info["met"], info["gre"], info["gro"]]]])
    dh = float(np.max(np.abs(h / R.full_history(ir) - 1)))
    dt = float(np.max(np.abs(R.cmat(t) - tr)))
    print("%s %s orf %g: history dev %.3e (bound %.1e), t dev %.3e (bound %.1e)" % (lat, dirs, orf, dh, R.bound(yh), dt, R.bound(yt)))
    assert dh <= R.bound(yh) and dt <= R.bound(yt)
    assert np.array_equal(info["hist"][:39], i39["hist"])
    half = lo.vol // 2
    assert np.array_equal(t[half:], t39[half:]) and not np.array_equal(t[:half], t39[:half])
    assert float(np.max(np.abs(R.cmat(t39) - ir["states"][39]))) <= R.bound(yt)


@pytest.mark.parametrize("lat", R.LATS)
@pytest.mark.parametrize("dirs", [R.COULOMB, R.LANDAU])
@pytest.mark.parametrize("gstop", [1e-5, 1e-10])
def test_convergence(oracle, lat, dirs, gstop):
    """gdsq recomputed in numpy from the downloaded t is <= gstop; t is in SU(3) to 1e-12; the iteration count is within 2 % (at
    least 2) of the reference's, measured on the CPU (gaugefix_ref.REF_ITERS); a too small maxits is returned as iters, rc 0."""
    import qex_amd as q

    lo, g = _input(oracle, lat)
    ctx = _ctx(lat, g)
    t, info = q.getGaugeFixTransform(ctx, dirs, gstop=gstop, orf=1.8, maxits=5000)
    G, tc = R.links(g), R.cmat(t)
    met, gre, gro = R.metrics(lo, R.gradient(lo, G, tc, dirs), tc, len(dirs))
    want = R.REF_ITERS[(lat, dirs, gstop)]
    print("%s %s gstop %g: %d iterations (reference %d), gdsq %.3e (numpy %.3e), met %.12f" %
          (lat, dirs, gstop, info["iters"], want, info["gdsq"], gre + gro, info["met"]))
    assert gre + gro <= gstop and info["gdsq"] <= gstop
    assert abs(met - info["met"]) < 1e-13
    assert np.abs(R.mul(tc, R.adj(tc)) - np.eye(3)).max() < 1e-12 and np.abs(np.linalg.det(tc) - 1).max() < 1e-12
    assert abs(info["iters"] - want) <= max(2, 0.02 * want)
    _, few = q.getGaugeFixTransform(ctx, dirs, gstop=gstop, orf=1.8, maxits=10)
    assert few["iters"] == 10 and few["hist"].shape == (10, 3)


@pytest.mark.parametrize("lat", R.LATS)
@pytest.mark.parametrize("dirs", [R.COULOMB, R.LANDAU])
def test_transform_of_the_resident_links(oracle, lat, dirs):
    """after qexhip_gauge_transform: plaquettes and Polyakov loops unchanged to 1e-13, the link trace is the final met to 1e-13,
    and a second fix from the identity stops within the first 12 iterations"""
    import qex_amd as q

    lo, g = _input(oracle, lat)
    ctx = _ctx(lat, g)
    pl0, lp0 = q.plaq(ctx), np.array(q.ploops(ctx))
    assert abs(q.linkTrace(ctx, dirs) - R.link_trace(lo, R.links(g), dirs)) < 1e-13
    t, info = q.getGaugeFixTransform(ctx, dirs, gstop=1e-10, orf=1.8, maxits=5000)
    q.gaugeTransform(ctx)
    pl1, lp1 = q.plaq(ctx), np.array(q.ploops(ctx))
    lt = q.linkTrace(ctx, dirs)
    print("%s %s: plaq dev %.2e, loops dev %.2e, link trace %.15f, met %.15f" % (lat, dirs, np.abs(pl1 - pl0).max(), np.abs(lp1 - lp0).max(), lt, info["met"]))
    assert np.abs(pl1 - pl0).max() < 1e-13 and np.abs(lp1 - lp0).max() < 1e-13
    assert abs(lt - info["met"]) < 1e-13
    want = R.gauge_transform(lo, R.links(g), R.cmat(t))
    got = np.zeros_like(g)
    q._lib.check(q.lib().qexhip_gauge_get(ctx._h, got.ctypes.data))
    assert max(np.abs(R.cmat(got[:, mu]) - want[mu]).max() for mu in range(4)) < 1e-13
    _, again = q.getGaugeFixTransform(ctx, dirs, gstop=1e-10, orf=1.8, maxits=5000)
    print("second fix: %d iterations, gdsq %.3e" % (again["iters"], again["gdsq"]))
    assert again["iters"] <= 12 and again["gdsq"] <= 1e-10


def test_a_small_transform_of_the_unit_gauge_is_undone(oracle):
    """the unit gauge transformed by exp(0.1 TAH(random)), Landau-fixed: link trace >= 1 - 1e-6"""
    import qex_amd as q

    lat = (4, 6, 10, 6)
    lo = q.Layout(list(lat))
    rng = np.random.default_rng(3)
    a = R.tah(rng.standard_normal((lo.vol, 3, 3)) + 1j * rng.standard_normal((lo.vol, 3, 3)))
    unit = [np.tile(np.eye(3, dtype=complex), (lo.vol, 1, 1)) for _ in range(4)]
    g = np.ascontiguousarray(np.stack([R.rmat(m) for m in R.gauge_transform(lo, unit, R.expm(0.1 * a))], axis=1))
    ctx = _ctx(lat, g)
    before = q.linkTrace(ctx, R.LANDAU)
    _, info = q.getGaugeFixTransform(ctx, R.LANDAU, gstop=1e-12, orf=1.8, maxits=5000)
    q.gaugeTransform(ctx)
    after = q.linkTrace(ctx, R.LANDAU)
    print("link trace %.9f -> %.12f in %d iterations (gdsq %.2e)" % (before, after, info["iters"], info["gdsq"]))
    assert before < 0.999 and after >= 1 - 1e-6


def test_result_does_not_depend_on_the_chunk_size(oracle):
    """option gfix_check 1, 7, 16: bit-identical t, iters and history (relax phase, the hand-over to the line minimisation, polish)"""
    import qex_amd as q

    lat = (4, 6, 10, 6)
    lo, g = _input(oracle, lat)
    ctx = _ctx(lat, g)
    res = []
    for chunk in (1, 7, 16):
        ctx.set_option("gfix_check", chunk)
        res.append(q.getGaugeFixTransform(ctx, R.COULOMB, gstop=1e-5, orf=1.8, maxits=5000))
    for t, info in res[1:]:
        assert info["iters"] == res[0][1]["iters"] and np.array_equal(info["hist"], res[0][1]["hist"]) and np.array_equal(t, res[0][0])
        assert (info["met"], info["gre"], info["gro"]) == (res[0][1]["met"], res[0][1]["gre"], res[0][1]["gro"])
    with pytest.raises(q.QexHipError):
        ctx.set_option("gfix_check", 0)


@pytest.mark.parametrize("dirs", [R.COULOMB, R.LANDAU])
def test_one_rank_halo_path_is_bit_identical_under_delayed_exchanges(oracle, dirs):
    """One rank with ghost zones (force_halo) and every exchange delayed by 40 us: t after 40 relax iterations, and the history, are
    the bits of the context without a halo; so are the transformed links."""
    import qex_amd as q

    lat = (8, 8, 8, 8)
    lo, g = _input(oracle, lat)
    c0, c1 = _ctx(lat, g), _ctx(lat, g, halo=True, emu_us=40)
    assert c1.sweep_info()["halo"] and not c0.sweep_info()["halo"]
    t0, i0 = q.getGaugeFixTransform(c0, dirs, gstop=0.0, orf=1.8, maxits=40)
    t1, i1 = q.getGaugeFixTransform(c1, dirs, gstop=0.0, orf=1.8, maxits=40)
    assert np.array_equal(t1, t0) and np.array_equal(i1["hist"], i0["hist"]) and i1["met"] == i0["met"]
    out = []
    for c in (c0, c1):
        q.gaugeTransform(c)
        gg = np.zeros_like(g)
        q._lib.check(q.lib().qexhip_gauge_get(c._h, gg.ctypes.data))
        out.append((gg, q.plaq(c), q.linkTrace(c, dirs)))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]


def test_refusals(oracle):
    """Through the raw C ABI: QEXHIP_ERR_ARG and a message for bad dirs, orf outside (0, 2], maxits < 0, no resident gauge field, no
    resident transform -- with nothing written: outputs keep their sentinels, t keeps its bits."""
    import qex_amd as q

    L = q.lib()
    lat = (4, 6, 10, 6)
    lo, g = _input(oracle, lat)
    i4 = C.c_int * 4
    its, met, hist, out = C.c_int(-7), (C.c_double * 4)(-7, -7, -7, -7), (C.c_double * 6)(*([-7.0] * 6)), C.c_double(-7)

    def fix(ctx, dirs, n, gstop=1e-5, orf=1.8, maxits=10):
        return L.qexhip_gauge_fix(ctx._h, dirs, n, gstop, orf, maxits, C.byref(its), met, hist, 2)

    def refused(rc, word):
        msg = L.qexhip_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)
        assert its.value == -7 and list(met) == [-7.0] * 4 and list(hist) == [-7.0] * 6 and out.value == -7.0

    bare = q.Context(list(lat))
    refused(fix(bare, i4(0, 1, 2, 3), 3), "no resident gauge field")
    refused(L.qexhip_gauge_link_trace(bare._h, i4(0, 1, 2, 3), 3, C.byref(out)), "no resident gauge field")
    refused(L.qexhip_gauge_transform(bare._h), "no resident gauge field")
    ctx = _ctx(lat, g)
    refused(fix(ctx, i4(0, 1, 2, 3), 3), "no resident transform")
    refused(L.qexhip_gauge_transform(ctx._h), "no resident transform")
    tbuf = np.full((lo.vol, 3, 3, 2), -7.0)
    refused(L.qexhip_gfix_get_transform(ctx._h, tbuf.ctypes.data), "no resident transform")
    assert np.all(tbuf == -7.0)
    t_in = R.rmat(R.random_su3(lo, 77))
    q._lib.check(L.qexhip_gfix_set_transform(ctx._h, t_in.ctypes.data))
    for dirs, n, word in ((i4(0, 1, 1, 3), 3, "repeated"), (i4(0, 4, 1, 3), 2, "not a direction"), (i4(0, -1, 1, 3), 2, "not a direction"),
                          (i4(0, 1, 2, 3), 0, "1..4 directions"), (i4(0, 1, 2, 3), 5, "1..4 directions"), (None, 3, "1..4 directions")):
        refused(fix(ctx, dirs, n), word)
        refused(L.qexhip_gauge_link_trace(ctx._h, dirs, n, C.byref(out)), word)
    for orf in (0.0, -1.0, 2.5, float("nan")):
        refused(fix(ctx, i4(0, 1, 2, 3), 3, orf=orf), "over-relaxation")
    refused(fix(ctx, i4(0, 1, 2, 3), 3, maxits=-1), "maxits")
    t_out, g_out = np.zeros_like(t_in), np.zeros_like(g)
    q._lib.check(L.qexhip_gfix_get_transform(ctx._h, t_out.ctypes.data))
    q._lib.check(L.qexhip_gauge_get(ctx._h, g_out.ctypes.data))
    assert np.array_equal(t_out, t_in) and np.array_equal(g_out, g)
    assert fix(ctx, i4(0, 1, 2, 3), 3, maxits=0) == 0 and its.value == 0 and met[3] == met[1] + met[2] and hist[0] == -7.0
    ctx.release_workspace()
    its.value = -7
    for k in range(4):
        met[k] = -7.0
    refused(fix(ctx, i4(0, 1, 2, 3), 3), "no resident transform")


def test_example_prints_the_api_link_trace(oracle):
    """examples/gauge_fix.py -lat 8 8 8 8 (Coulomb) prints the link trace the API returns for the same steps; -wall 0 runs too"""
    import qex_amd as q

    lat = [8, 8, 8, 8]
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "gauge_fix.py"), "-lat"] + [str(v) for v in lat] + ["-wall", "0"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    m = re.search(r"^post-fix link trace: (\S+)$", p.stdout, re.M)
    assert m and "corner: 7" in p.stdout and "gauge fixing:" in p.stdout, p.stdout[-2000:]
    rf = q.RngField(lat, q.RngMilc6, 987654321)
    g = rf.warm(0.3)
    rot = np.ascontiguousarray(rf.random()[:, 0])
    ctx = _ctx(lat, g)
    q._lib.check(q.lib().qexhip_gfix_set_transform(ctx._h, rot.ctypes.data))
    q.gaugeTransform(ctx)
    _, info = q.getGaugeFixTransform(ctx, [0, 1, 2], gstop=1e-6, orf=1.5)
    q.gaugeTransform(ctx)
    lt = q.linkTrace(ctx, [0, 1, 2])
    print("example: %s, API: %.16g (met %.16g, %d iterations)" % (m.group(1), lt, info["met"], info["iters"]))
    assert abs(float(m.group(1)) - lt) < 1e-13 and abs(lt - info["met"]) < 1e-13
