"""Stout smearing on the device (qexhip_stout_*; qex_amd/stout.py) against tests/stout_ref.py, the numpy restatement of
src/gauge/stoutsmear.nim that tests/test_stout_ref.py proves on the CPU.

Shapes: 8^4 (paired-parity tiles), 4x6x10x6 (the awkward shape) and 6x6x6x8 (a partial tile, the unpaired kernel path).
Configuration per shape: g.random followed by ten in-place stout steps (tstoutderiv.nim:19-23).  Tolerances are the project's own
for the nHYP counterparts (tests/test_smear.py:110,198): forward ||x - ref|| / ||ref|| < 1e-12, chain < 1e-11.  Observed values
are printed (pytest -s) and recorded in DESIGN.md."""
import ctypes as C

import numpy as np
import pytest

import stout_ref as R

pytestmark = pytest.mark.gpu
LATS = [(8, 8, 8, 8), (4, 6, 10, 6), (6, 6, 6, 8)]
_CFG, _REF = {}, {}


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def cfg(o, lat, alpha=0.1):
    key = (lat, alpha)
    if key not in _CFG:
        lo = o.Layout(list(lat))
        _CFG[key] = (lo, R.reference_config(lo, alpha))
    return _CFG[key]


def chain_field(o, lo):
    rf = o.RngField(lo, o.RNG_MILC6, 21)
    return o.gauge_random_tah(lo, rf) + 0.3 * o.gauge_random(lo, rf)      # generic, non-algebra (test_gpu_nhyp_force_chain)


def ref_chain(o, lat, alphas):
    key = (lat, alphas)
    if key not in _REF:
        lo, g = cfg(o, lat)
        _REF[key] = R.chain_deriv(lo, alphas, g, chain_field(o, lo))
    return _REF[key]


def ctx_of(lat, halo=False, **opts):
    import qex_amd as q

    ctx = q.Context(list(lat))
    if halo:
        ctx.force_halo(True)
    for k, v in opts.items():
        ctx.set_option(k, v)
    return ctx


@pytest.mark.parametrize("lat", LATS)
@pytest.mark.parametrize("alpha", [0.02, 0.1])
@pytest.mark.parametrize("flow_exp", [1, 0])
def test_smear_against_the_reference(oracle, lat, alpha, flow_exp):
    import qex_amd as q

    lo, g = cfg(oracle, lat)
    ref = R.StoutSmear(lo, alpha).smear(g)
    ctx = ctx_of(lat, flow_exp=flow_exp)
    fl = np.zeros_like(g)
    q.stoutSmear(ctx, g, alpha, fl)
    d = rel(fl, ref)
    print("%s alpha %g flow_exp %d: smear dev %.3e" % (lat, alpha, flow_exp, d))
    assert d < 1e-12
    gi = g.copy()
    q.stoutSmear(ctx, gi, alpha, gi)                       # in place
    assert np.array_equal(gi, fl)
    ss = q.newStoutSmear(ctx, alpha)                       # the level object, in place and out of place
    g2, f2 = g.copy(), np.zeros_like(g)
    ss.smear(g2, f2)
    ss.smear(g2, g2)
    assert np.array_equal(f2, fl) and np.array_equal(g2, fl)
    q.gaugeSet(ctx, g)                                     # the resident form
    p0 = q.plaq(ctx).sum()
    fr = np.zeros_like(g)
    q.stoutSmear(ctx, None, alpha, fr)
    assert np.array_equal(fr, fl)
    assert q.plaq(ctx).sum() == p0                         # fl given: the resident links stay
    q.stoutSmear(ctx, None, alpha, None)                   # ... fl = NULL: they are replaced
    check = np.zeros_like(g)
    q.lib().qexhip_gauge_get(ctx._h, check.ctypes.data_as(C.c_void_p))
    assert np.array_equal(check, fl)
    p1 = q.plaq(ctx).sum()
    print("   plaquette sum %.12g -> %.12g" % (p0, p1))
    assert p1 > p0


def test_smear_with_alpha_zero_is_the_identity(oracle):
    import qex_amd as q

    lat = LATS[1]
    lo, g = cfg(oracle, lat)
    for fe in (1, 0):
        ctx = ctx_of(lat, flow_exp=fe)
        fl = np.zeros_like(g)
        sf = q.stoutSmearGetForce(ctx, g, fl, [0.0])
        assert np.array_equal(fl, g)
        chain = chain_field(oracle, lo)
        f = np.zeros_like(g)
        sf(f, chain)
        assert rel(f, chain) < 1e-15


@pytest.mark.parametrize("lat", LATS)
@pytest.mark.parametrize("alphas", [(0.1,), (0.1, 0.09), (0.1, 0.09, 0.12)], ids=["1level", "2levels", "3levels"])
def test_force_chain_against_the_reference(oracle, lat, alphas):
    import qex_amd as q

    lo, g = cfg(oracle, lat)
    chain = chain_field(oracle, lo)
    rfl, rf = ref_chain(oracle, lat, alphas)
    ctx = ctx_of(lat, flow_exp=0)
    fl = np.zeros_like(g)
    sf = q.stoutSmearGetForce(ctx, g, fl, alphas)
    f = np.zeros_like(g)
    sf(f, chain)
    dl, df = rel(fl, rfl), rel(f, rf)
    print("%s %d levels: links dev %.3e, chain dev %.3e" % (lat, len(alphas), dl, df))
    assert dl < 1e-12 and df < 1e-11
    f2 = chain.copy()
    sf(f2, f2)                                             # f aliasing chain
    assert np.array_equal(f2, f)
    # n single-level objects chained through the host (tstoutderiv.nim:149-193)
    ss = [q.newStoutSmear(ctx, a) for a in alphas]
    cur = g
    for s in ss:
        nxt = np.zeros_like(g)
        s.smear(cur, nxt)
        cur = nxt
    assert np.array_equal(cur, fl)
    fo = chain
    for s in reversed(ss):
        d = np.zeros_like(g)
        s.smearDeriv(d, fo)
        fo = d
    assert np.array_equal(fo, f)
    # the closed-form exp of the default setting: the same function, another algorithm
    ctx1 = ctx_of(lat)
    sf1 = q.stoutSmearGetForce(ctx1, g, None, alphas)
    f1 = np.zeros_like(g)
    sf1(f1, chain)
    d1 = rel(f1, rf)
    print("   flow_exp 1: chain dev %.3e" % d1)
    assert d1 < 1e-11


def test_force_refusals_and_halo_path(oracle):
    import qex_amd as q

    lat = LATS[0]
    lo, g = cfg(oracle, lat)
    chain = chain_field(oracle, lo)
    alphas = (0.1, 0.09)
    ctx = ctx_of(lat)
    f = np.zeros_like(g)
    with pytest.raises(q.QexHipError):                     # nothing prepared
        q._lib.check(q.lib().qexhip_stout_force(ctx._h, f.ctypes.data_as(C.c_void_p), chain.ctypes.data_as(C.c_void_p)))
    sf = q.stoutSmearGetForce(ctx, g, None, alphas)
    sf(f, chain)
    fg = np.zeros_like(g)
    sf.gaugeForce(fg, 6.0)
    sf.release()
    with pytest.raises(q.QexHipError):
        sf(f, chain)
    with pytest.raises(q.QexHipError):
        sf.gaugeForce(fg, 6.0)
    gi = g.copy()
    sfi = q.stoutSmearGetForce(ctx, gi, gi, alphas)        # level 0 in place
    with pytest.raises(q.QexHipError):
        sfi(f, chain)
    ss = q.newStoutSmear(ctx, 0.1)
    gi = g.copy()
    ss.smear(gi, gi)
    with pytest.raises(q.QexHipError):
        ss.smearDeriv(f, chain)
    so, fo, d0, d1 = q.newStoutSmear(ctx, 0.1), np.zeros_like(g), np.zeros_like(g), np.zeros_like(g)
    so.smear(g, fo)
    so.smearDeriv(d0, chain)
    ctx.release_workspace()                                # the object smears its kept input again
    so.smearDeriv(d1, chain)
    assert np.array_equal(d0, d1)
    sf = q.stoutSmearGetForce(ctx, g, None, alphas)
    ctx.release_workspace()                                # drops the chain
    with pytest.raises(q.QexHipError):
        sf(f, chain)
    # the ghost-slice form of every kernel (t "sharded" over one rank): the same arithmetic per link, the same bits
    ctxh = ctx_of(lat, halo=True)
    flh, fl0 = np.zeros_like(g), np.zeros_like(g)
    sfh = q.stoutSmearGetForce(ctxh, g, flh, alphas)
    q.stoutSmearGetForce(ctx, g, fl0, alphas)
    fh, fgh = np.zeros_like(g), np.zeros_like(g)
    sfh(fh, chain)
    sfh.gaugeForce(fgh, 6.0)
    assert np.array_equal(flh, fl0) and np.array_equal(fh, f) and np.array_equal(fgh, fg)


@pytest.mark.parametrize("alphas", [(0.1,), (0.1, 0.09), (0.1, 0.09, 0.12)], ids=["1level", "2levels", "3levels"])
def test_tstoutderiv_on_the_device(oracle, alphas):
    """tests/base/tstoutderiv.nim with the closure's gaugeForce (cplaq = 6) and qexhip_gauge_action on the device-smeared links:
    the reference's five directions and three criteria"""
    import qex_amd as q

    o = oracle
    lat = LATS[0]
    lo, g = cfg(o, lat)
    rfd = o.RngField(lo, o.RNG_MRG32K3A, 4321)
    directions = [o.gauge_random_tah(lo, rfd) for _ in range(5)]
    ctx = ctx_of(lat)
    sf = q.stoutSmearGetForce(ctx, g, None, alphas)
    f = np.zeros_like(g)
    sf.gaugeForce(f, 6.0)

    def action(gg):
        q.gaugeSet(ctx, gg)
        for a in alphas:
            q.stoutSmear(ctx, None, a, None)
        return q.gaugeAction(ctx, None, plaq=6.0)

    fails = []
    for n, p in enumerate(directions):
        d, e = R.ndiff(lambda x: action(R.addnoise(lo, x, p, g)), 0.0, 1.0)
        pf = R.redot(p, f)
        err = abs(pf - d)
        print("%d levels test %d: p.f %.12g ndiff %.12g delta %.3g err(ndiff) %.3g" % (len(alphas), n, pf, d, pf - d, e))
        if not (err < max(2e-8, 32 * e) and err < 1e-5 and abs(err / pf) < 1e-7):
            fails.append((n, pf, d, e))
    assert not fails, fails


def test_tstoutinverse_on_the_device(oracle):
    """tests/base/tstoutinverse.nim: alpha = 0.02, del2 <= 1e-24; the iteration count within +-1 of the restatement's (the sums run
    in another order, so the crossing of rdf2req may move by one)"""
    import qex_amd as q

    lat = LATS[0]
    lo, g = cfg(oracle, lat, 0.02)
    ctx = ctx_of(lat)
    ss = q.newStoutSmear(ctx, 0.02)
    f, u = np.zeros_like(g), np.zeros_like(g)
    ss.smear(g, f)
    it, r2 = ss.inverse(u, f)
    d2 = R.del2(lo, u, g)
    way = "the same" if it == R.INVERSE_ITERS else ("one later" if it > R.INVERSE_ITERS else "one earlier")
    print("inverse: %d iterations (restatement %d: %s), rdf2 %.3e, del2 %.3e, diverging %s" % (it, R.INVERSE_ITERS, way, r2, d2, ss.diverging))
    assert d2 <= 1e-24
    assert abs(it - R.INVERSE_ITERS) <= 1 and r2 < 1e-24
    ctx1 = ctx_of(lat, stout_check=1)                      # read back after every iteration: the same bits and count
    u1 = np.zeros_like(g)
    it1, r21 = q.newStoutSmear(ctx1, 0.02).inverse(u1, f)
    assert (it1, r21) == (it, r2) and np.array_equal(u1, u)
    ctxh = ctx_of(lat, halo=True, stout_check=3)           # ghost-slice form of the kernel
    uh = np.zeros_like(g)
    ith, r2h = q.newStoutSmear(ctxh, 0.02).inverse(uh, f)
    assert (ith, r2h) == (it, r2) and np.array_equal(uh, u)
    # maxits = 3: three iterations and the rdf2 of the returned field
    u3 = np.zeros_like(g)
    it3, r23 = ss.inverse(u3, f, maxIter=3)
    ur, itr, r2r, _ = R.StoutSmear(lo, 0.02).inverse(f, max_iter=3)
    print("maxits 3: rdf2 %.6e (restatement %.6e), field dev %.3e" % (r23, r2r, rel(u3, ur)))
    assert it3 == 3 and itr == 3 and abs(r23 / r2r - 1) < 1e-9 and rel(u3, ur) < 1e-12
    u0 = np.zeros_like(g)
    it0, _ = ss.inverse(u0, f, maxIter=0)
    assert it0 == 0 and np.array_equal(u0, f)


@pytest.mark.parametrize("lat", LATS[1:])
def test_inverse_on_the_other_shapes(oracle, lat):
    import qex_amd as q

    lo, g = cfg(oracle, lat, 0.02)
    ctx = ctx_of(lat)
    ss = q.newStoutSmear(ctx, 0.02)
    f, u = np.zeros_like(g), np.zeros_like(g)
    ss.smear(g, f)
    it, r2 = ss.inverse(u, f)
    _, itr, r2r, _ = R.StoutSmear(lo, 0.02).inverse(f)
    d2 = R.del2(lo, u, g)
    print("%s inverse: %d iterations (restatement %d), rdf2 %.3e, del2 %.3e" % (lat, it, itr, r2, d2))
    assert d2 <= 1e-24 and abs(it - itr) <= 1


def test_inverse_reports_divergence(oracle):
    import qex_amd as q

    lat = LATS[0]
    lo, g = cfg(oracle, lat, 0.02)
    ctx = ctx_of(lat)
    ss = q.newStoutSmear(ctx, R.DIVERGING_ALPHA)
    f, u = np.zeros_like(g), np.zeros_like(g)
    ss.smear(g, f)
    it, r2 = ss.inverse(u, f, maxIter=5)
    print("alpha %g: %d iterations, rdf2 %.3e, diverging %s" % (R.DIVERGING_ALPHA, it, r2, ss.diverging))
    assert it == 5 and ss.diverging
    ss2 = q.newStoutSmear(ctx, 0.02)
    ss2.inverse(u, f, maxIter=5)
    assert not ss2.diverging


def test_argument_errors_leave_everything_untouched(oracle):
    import qex_amd as q

    lat = LATS[1]
    lo, g = cfg(oracle, lat)
    ctx = ctx_of(lat)
    q.gaugeSet(ctx, g)
    L = q.lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    fl = np.full_like(g, 7.0)
    out = fl.copy()
    its, r2, dv = C.c_int(-5), C.c_double(-5.0), C.c_int(-5)
    one = (C.c_double * 1)(0.1)
    nine = (C.c_double * 9)(*([0.1] * 9))
    cases = []
    for bad in (float("nan"), float("inf"), -float("inf")):
        cases.append(L.qexhip_stout_smear(ctx._h, vp(g), bad, vp(out)))
        cases.append(L.qexhip_stout_smear(ctx._h, None, bad, None))
        cases.append(L.qexhip_stout_prepare(ctx._h, vp(g), (C.c_double * 1)(bad), 1, vp(out)))
        cases.append(L.qexhip_stout_inverse(ctx._h, vp(g), bad, 1e-24, 10, vp(out), C.byref(its), C.byref(r2), C.byref(dv)))
    cases.append(L.qexhip_stout_prepare(ctx._h, vp(g), one, 0, vp(out)))
    cases.append(L.qexhip_stout_prepare(ctx._h, vp(g), nine, 9, vp(out)))
    cases.append(L.qexhip_stout_prepare(ctx._h, None, one, -1, None))
    cases.append(L.qexhip_stout_inverse(ctx._h, vp(g), 0.02, 1e-24, -1, vp(out), C.byref(its), C.byref(r2), C.byref(dv)))
    cases.append(L.qexhip_stout_inverse(ctx._h, vp(out), 0.02, 1e-24, 10, vp(out), C.byref(its), C.byref(r2), C.byref(dv)))
    assert cases and all(rc == -1 for rc in cases), cases     # QEXHIP_ERR_ARG
    assert np.array_equal(out, fl) and (its.value, r2.value, dv.value) == (-5, -5.0, -5)
    res = np.zeros_like(g)
    L.qexhip_gauge_get(ctx._h, vp(res))
    assert np.array_equal(res, g)                             # the resident links, bit for bit
