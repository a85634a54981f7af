"""SloppyHalf on 16-bit storage (option "half" = 1): the 16-bit operator against the fp64 one and against a numpy model of the
format built on the oracle's sweeps, the reliable-update solveXX / solve against the fp64 CG, the stall guard's hand-over to fp32,
the switch leaving every other path alone, maxits, and staleness of the 16-bit link copy.  Observed values are printed (pytest -s)
and recorded in DESIGN.md.

Measured on MI355X (8^4 and 4.6.10.6, m = 0.1): see the table in DESIGN.md section 4 ("16-bit storage")."""
import ctypes as C
import functools

import numpy as np
import pytest

from half_ref import Model as _Model              # the 16-bit formats and operator in numpy

pytestmark = pytest.mark.gpu

SEED = 987654321
KINDS = [("random", False, 1), ("warm", False, 1), ("random", True, 1), ("warm", True, 1), ("scaled", False, 0), ("scaled", True, 0),
         ("hisq", True, 0)]


@functools.lru_cache(maxsize=None)
def _inputs(lat, kind, naik):
    """host inputs as tests/test_gpu_sloppy.py builds them, once per (lattice, kind)"""
    from oracle import oracle as o

    o.build()
    lo = o.Layout(list(lat))
    rf = o.RngField(lo, o.RNG_MILC6, SEED)
    if kind == "scaled":                               # rows not unitary: 18 reals
        fat = 1.01 * o.gauge_warm(lo, 0.5, rf)
        o.rephase(lo, fat)
        lng = 0.3 * fat if naik else None
    elif kind == "hisq":
        g = o.gauge_warm(lo, 0.5, rf)
        fat, lng = o.hisq_smear(lo, g)
        o.rephase(lo, fat)
        o.rephase(lo, lng)
    else:
        gen = (lambda: o.gauge_warm(lo, 0.5, rf)) if kind == "warm" else (lambda: o.gauge_random(lo, rf))
        fat = gen()
        o.rephase(lo, fat)
        lng = None
        if naik:
            lng = gen()
            o.rephase(lo, lng)
    b = o.vector_gaussian(lo, rf)
    for a in (fat, lng, b):
        if a is not None:
            a.setflags(write=False)
    return lo, fat, lng, b


def _setup(lat, kind, naik=False, half=1):
    import qex_amd as q

    lo, fat, lng, b = _inputs(tuple(lat), kind, naik)
    ctx = q.Context(list(lat))
    s = q.newStag3(ctx, fat, lng) if lng is not None else q.newStag(ctx, fat)
    ctx.set_option("half", half)
    return lo, ctx, s, fat, lng, b


def _half(lo, par_even):
    h = lo.vol // 2
    return slice(0, h) if par_even else slice(h, lo.vol)


def _maxrel(a, ref):
    return float(np.abs(a - ref).max() / np.abs(ref).max())


def _true_r2(ctx, xh, bh, mass, par_even):
    """|b - A x|^2 on the parity, with the fp64 operator (dev_op_xx)"""
    fx, fr = ctx.field_new(xh), ctx.field_new()
    try:
        ctx.dev_op_xx(fr, fx, mass * mass, par_even)
        ax = ctx.field_download(fr)
    finally:
        ctx.field_free(fx)
        ctx.field_free(fr)
    sl = slice(0, len(xh) // 2) if par_even else slice(len(xh) // 2, len(xh))
    return float(np.sum((bh[sl] - ax[sl]) ** 2))


# ---- 1. the 16-bit operator ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lat", [[8, 8, 8, 8], [4, 6, 10, 6]])
@pytest.mark.parametrize("kind,naik,fmt", KINDS)
def test_op_xx_half_vs_fp64_and_model(oracle, lat, kind, naik, fmt):
    o = oracle
    lo, ctx, s, fat, lng, b = _setup(lat, kind, naik)
    f, s_fat, s_long, dev = ctx.links_info_half()
    assert f == fmt and f == ctx.links_info_f32()[0], (f, dev)
    assert s_fat == float(np.abs(fat).max())
    assert s_long == (float(np.abs(lng).max()) if lng is not None else 0.0)
    model = _Model(o, lo, fat, lng, fmt)
    for par_even, m2 in ((True, 0.01), (False, 0.04)):
        sl = _half(lo, par_even)
        fx, fh, f64 = ctx.field_new(b), ctx.field_new(), ctx.field_new()
        ctx.dev_op_xx_half(fh, fx, m2, par_even)
        ctx.dev_op_xx(f64, fx, m2, par_even)
        rh, r64 = ctx.field_download(fh), ctx.field_download(f64)
        for fid in (fx, fh, f64):
            ctx.field_free(fid)
        ref = o.stagD2xx(lo, fat, lng, b, m2, par_even)
        assert _maxrel(r64[sl], ref[sl]) <= 1e-12
        rm = model.op_xx(b, m2, par_even)
        e_model = _maxrel(rm[sl], ref[sl])               # the error of the format alone, from the reference on the CPU
        e_hip, e_hm = _maxrel(rh[sl], r64[sl]), _maxrel(rh[sl], rm[sl])
        print(f"op_xx_half {lat} {kind} naik={naik} fmt={f} par_even={par_even}: max rel err vs fp64 {e_hip:.2e}, model vs fp64 "
              f"{e_model:.2e}, HIP vs model {e_hm:.2e}")
        # fp32 arithmetic may flip roundings by one step per stored value: a factor 2
        assert e_hip <= 2 * e_model
        assert not rh[_half(lo, not par_even)].any()        # the other parity is not written


# ---- 2. solveXX on 16-bit storage -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("par_even", [True, False])
@pytest.mark.parametrize("r2req", [1e-8, 1e-14, 1e-20])
@pytest.mark.parametrize("kind,naik", [("random", False), ("warm", False), ("random", True), ("scaled", False), ("hisq", True)])
def test_solveXX_half(oracle, kind, naik, par_even, r2req):
    import qex_amd as q

    lo, ctx, s, fat, lng, b = _setup([8, 8, 8, 8], kind, naik)
    mass = 0.1
    sl = _half(lo, par_even)
    sp64 = q.SolverParams(r2req=r2req, maxits=5000, verbosity=0)
    x64 = np.zeros_like(b)
    s.solveXX(x64, b, mass, sp64, par_even)
    sp = q.SolverParams(r2req=r2req, maxits=5000, verbosity=0, sloppySolve=q.SloppyHalf)
    x = np.zeros_like(b)
    s.solveXX(x, b, mass, sp, par_even)
    last = ctx.sloppy_last()
    b2 = float(np.sum(b[sl] ** 2))
    r2 = _true_r2(ctx, x, b, mass, par_even)
    ratio = sp.iterations / sp64.iterations
    xerr = np.linalg.norm(x[sl] - x64[sl]) / np.linalg.norm(x64[sl])
    print(f"solveXX_half {kind} naik={naik} par_even={par_even} r2req={r2req:g}: its {sp.iterations} vs fp64 {sp64.iterations} "
          f"(ratio {ratio:.3f}), updates {sp.reliableUpdates}, true r2/b2 {r2 / b2:.3e} (reported {sp.r2:.3e}), x rel diff {xerr:.2e}, "
          f"last {last}")
    assert last["precision"] == 2 and last["fell_back"] == 0 and last["half_iters"] == sp.iterations and last["f32_iters"] == 0
    assert r2 <= r2req * b2
    assert abs(sp.r2 - r2 / b2) <= 1e-6 * r2 / b2 + 1e-300
    # |x - x64| <= |A^-1| (|r| + |r64|) and |A^-1| <= 1/(4 m^2): both residuals are below sqrt(r2req) |b|
    assert xerr <= 2 * np.sqrt(r2req) * np.sqrt(b2) / (4 * mass * mass) / np.linalg.norm(x64[sl]) * 1.01
    # beyond 2x the 16-bit sweep, at best 1.9x cheaper in bytes, cannot pay for itself
    assert sp.iterations <= 2 * sp64.iterations
    assert sp.reliableUpdates >= 1
    assert not x[_half(lo, not par_even)].any()


# ---- 3. full solve --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r2req", [1e-8, 1e-14, 1e-20])
@pytest.mark.parametrize("kind,naik", [("random", False), ("hisq", True)])
def test_solve_half_full(oracle, kind, naik, r2req):
    import qex_amd as q

    o = oracle
    lo, ctx, s, fat, lng, b = _setup([8, 8, 8, 8], kind, naik)
    m = 0.1
    sp64 = q.SolverParams(r2req=r2req, maxits=5000, verbosity=0)
    x64 = np.zeros_like(b)
    s.solve(x64, b, m, sp64)
    sp = q.SolverParams(r2req=r2req, maxits=5000, verbosity=0, sloppySolve=q.SloppyHalf)
    x = np.zeros_like(b)
    s.solve(x, b, m, sp)
    last = ctx.sloppy_last()
    res = b - o.D(lo, fat, lng, x, m)
    rel = float(np.sum(res ** 2) / np.sum(b ** 2))
    print(f"solve_half {kind} r2req={r2req:g}: its {sp.iterations} vs fp64 {sp64.iterations} (ratio {sp.iterations / sp64.iterations:.3f}), "
          f"updates {sp.reliableUpdates}, |b-Dx|^2/|b|^2 {rel:.3e} (reported {sp.r2:.3e}), last {last}")
    assert rel <= r2req and sp.r2 <= r2req and sp.reliableUpdates >= 1
    assert abs(sp.r2 - rel) <= 1e-6 * rel
    assert last["precision"] == 2 and last["fell_back"] == 0 and last["half_iters"] + last["f32_iters"] == sp.iterations
    assert sp.iterations <= 2 * sp64.iterations


# ---- 4. the stall guard -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("par_even", [True, False])
def test_fallback_finishes_in_fp32(oracle, par_even):
    import qex_amd as q

    lo, ctx, s, fat, lng, b = _setup([8, 8, 8, 8], "random")
    mass, r2req = 0.1, 1e-14
    sl = _half(lo, par_even)
    b2 = float(np.sum(b[sl] ** 2))
    ctx.set_option("half_stall", 0)                      # hand over at the first reliable update
    sp = q.SolverParams(r2req=r2req, maxits=5000, verbosity=0, sloppySolve=q.SloppyHalf)
    x = np.zeros_like(b)
    s.solveXX(x, b, mass, sp, par_even)
    last = ctx.sloppy_last()
    r2 = _true_r2(ctx, x, b, mass, par_even)
    print(f"fallback par_even={par_even}: its {sp.iterations}, updates {sp.reliableUpdates}, true r2/b2 {r2 / b2:.3e}, last {last}")
    assert r2 <= r2req * b2 and abs(sp.r2 - r2 / b2) <= 1e-6 * r2 / b2
    assert last["precision"] == 2 and last["fell_back"] == 1
    assert last["half_iters"] > 0 and last["f32_iters"] > 0 and last["half_iters"] + last["f32_iters"] == sp.iterations
    # the full solve sums over its inner solves
    spf = q.SolverParams(r2req=1e-12, maxits=5000, verbosity=0, sloppySolve=q.SloppyHalf)
    xf = np.zeros_like(b)
    s.solve(xf, b, mass, spf)
    last = ctx.sloppy_last()
    assert spf.r2 <= 1e-12 and last["fell_back"] == 1 and last["half_iters"] + last["f32_iters"] == spf.iterations
    # the default guard does not fire at m = 0.1
    ctx.set_option("half_stall", 2)
    sp2 = q.SolverParams(r2req=r2req, maxits=5000, verbosity=0, sloppySolve=q.SloppyHalf)
    s.solveXX(x, b, mass, sp2, par_even)
    last = ctx.sloppy_last()
    assert last["fell_back"] == 0 and last["f32_iters"] == 0 and last["half_iters"] == sp2.iterations
    # a single-precision solve reports itself
    sp1 = q.SolverParams(r2req=r2req, maxits=5000, verbosity=0, sloppySolve=q.SloppySingle)
    s.solveXX(x, b, mass, sp1, par_even)
    assert ctx.sloppy_last() == dict(precision=1, half_iters=0, f32_iters=sp1.iterations, fell_back=0)


# ---- 5. the switch leaves every other path alone ------------------------------------------------------------------------------
def test_switch_leaves_other_paths_alone(oracle):
    import qex_amd as q

    lo, ctx, s, fat, lng, b = _setup([8, 8, 8, 8], "random", half=0)
    o = oracle
    rf = o.RngField(lo, o.RNG_MILC6, 4711)
    b2v = o.vector_gaussian(lo, rf)

    def run():
        out = {}
        for name, sl in (("single", q.SloppySingle), ("fp64", q.SloppyNone), ("half", q.SloppyHalf)):
            sp = q.SolverParams(r2req=1e-14, maxits=5000, verbosity=0, sloppySolve=sl)
            x = np.zeros_like(b)
            s.solveEE(x, b, 0.1, sp)
            y = np.zeros_like(b)
            sp2 = q.SolverParams(r2req=1e-12, maxits=5000, verbosity=0, sloppySolve=sl)
            s.solve(y, b, 0.1, sp2)
            out[name] = (x, sp.iterations, sp.r2, y, sp2.iterations, sp2.r2)
        for sl in (1, 2):
            xs = [np.zeros_like(b), np.zeros_like(b)]
            its, fin, nup = s.solveXX_batch(xs, [b, b2v], [0.1, 0.2], 1e-14, 5000, True, sloppy=sl)
            out["batch%d" % sl] = (xs[0], xs[1], tuple(its), tuple(fin), tuple(nup))
            ms = [np.zeros_like(b), np.zeros_like(b)]
            sp = q.SolverParams(r2req=1e-14, maxits=5000, verbosity=0)
            fin = s.solveXX_multi(ms, b, [0.1, 0.05], sp, True, sloppy=sl)
            out["multi%d" % sl] = (ms[0], ms[1], sp.iterations, tuple(fin))
        return out

    def same(a, b_):
        return all(np.array_equal(u, v) if isinstance(u, np.ndarray) else u == v for u, v in zip(a, b_))

    off = run()
    assert same(off["half"], off["single"])               # option 0: SloppyHalf runs single, bit for bit
    ctx.set_option("half", 1)
    on = run()
    assert same(on["single"], off["single"]) and same(on["fp64"], off["fp64"])
    for k in ("batch", "multi"):
        assert same(on[k + "2"], on[k + "1"]) and same(on[k + "1"], off[k + "1"])
    assert not same(on["half"][:1], off["half"][:1])      # and the 16-bit path is another computation
    assert ctx.sloppy_last()["precision"] == 2


# ---- 6. bad values, mass 0, maxits ------------------------------------------------------------------------------------------
def test_bad_option_mass_zero_and_maxits(oracle):
    import qex_amd as q
    from qex_amd._lib import lib

    lo, ctx, s, fat, lng, b = _setup([8, 8, 8, 8], "random")
    L = lib()
    for bad in (2, -1):
        assert L.qexhip_set_option(ctx._h, b"half", bad) == -1 and b"half" in L.qexhip_last_error()
    assert L.qexhip_set_option(ctx._h, b"half_stall", -1) == -1
    x = np.zeros_like(b)
    pv = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert L.qexhip_stag_solve_xx_sloppy(ctx._h, pv(x), pv(b), 0.0, 1e-14, 100, 1, 2, None, None, None) == -1
    assert b"mass 0" in L.qexhip_last_error()
    fb, fx = ctx.field_new(b), ctx.field_new()
    assert L.qexhip_dev_solve_xx_sloppy(ctx._h, fx, fb, 0.0, 1e-14, 100, 1, 2, None, None, None) == -1
    # maxits: not an error, and the reported residual is the true one of the returned x
    its, fin, nup = ctx.dev_solve_xx_sloppy(fx, fb, 0.1, 1e-14, 10, True, q.SloppyHalf)
    x3 = ctx.field_download(fx)
    b2 = float(np.sum(b[: lo.vol // 2] ** 2))
    assert its == 10 and nup >= 1 and fin > 1e-14
    assert abs(fin - _true_r2(ctx, x3, b, 0.1, True) / b2) <= 1e-6 * fin
    assert ctx.sloppy_last() == dict(precision=2, half_iters=10, f32_iters=0, fell_back=0)
    ctx.field_free(fb)
    ctx.field_free(fx)


# ---- 7. the 16-bit links follow every change of the operator ----------------------------------------------------------------
def test_stale_half_links_are_rebuilt(oracle):
    import qex_amd as q

    o = oracle
    lo, ctx, s, fatA, lng, b = _setup([8, 8, 8, 8], "random")
    spA = q.SolverParams(r2req=1e-14, maxits=5000, verbosity=0, sloppySolve=q.SloppyHalf)
    x = np.zeros_like(b)
    s.solveEE(x, b, 0.1, spA)
    itsA = spA.iterations
    rf = o.RngField(lo, o.RNG_MILC6, 12345)
    fatB = o.gauge_random(lo, rf)
    o.rephase(lo, fatB)
    st = q.newStag(ctx, fatB)
    sp = q.SolverParams(r2req=1e-14, maxits=5000, verbosity=0, sloppySolve=q.SloppyHalf)
    sp64 = q.SolverParams(r2req=1e-14, maxits=5000, verbosity=0)
    xs, x64 = np.zeros_like(b), np.zeros_like(b)
    st.solveEE(xs, b, 0.1, sp)
    st.solveEE(x64, b, 0.1, sp64)
    h = lo.vol // 2
    b2 = float(np.sum(b[:h] ** 2))
    assert _true_r2(ctx, xs, b, 0.1, True) <= 1e-14 * b2
    # with A's 16-bit links the iteration would chase another operator's residual: the count stays that of a 16-bit solve
    print(f"stale links: its on A {itsA}, on B {sp.iterations} (fp64 {sp64.iterations})")
    assert sp.iterations <= 2 * sp64.iterations and ctx.sloppy_last()["fell_back"] == 0
    # and the 16-bit operator is B's
    fx, fh = ctx.field_new(b), ctx.field_new()
    ctx.dev_op_xx_half(fh, fx, 0.01, True)
    rh = ctx.field_download(fh)
    ctx.field_free(fx)
    ctx.field_free(fh)
    ref = o.stagD2xx(lo, fatB, None, b, 0.01, True)
    e_model = _maxrel(_Model(o, lo, fatB, None, 1).op_xx(b, 0.01, True)[:h], ref[:h])
    assert _maxrel(rh[:h], ref[:h]) <= 2 * e_model


# ---- 8. the deflated single-system solve takes the same inner solve ---------------------------------------------------------
def test_deflated_solve_runs_half(oracle):
    import qex_amd as q
    import eig_ref as R

    lat = (4, 4, 8, 8)
    lo, g, _, b = R.inputs(lat)
    ctx = q.Context(list(lat), device=0)
    s = q.newStag(ctx, g)
    B = s.eigs(16, nvecs=40, relerr=0.0, abserr=1e-9, cheb_degree=8, cheb_lo=0.3, cheb_hi=0.0, max_restarts=40)
    try:
        ctx.set_option("half", 1)
        b = np.ascontiguousarray(b)
        sp = q.SolverParams(r2req=1e-14, maxits=5000, verbosity=0, sloppySolve=q.SloppyHalf)
        x = np.zeros_like(b)
        s.solveEE(x, b, 0.1, sp, deflate=B)
        h = lo.vol // 2
        b2 = float(np.sum(b[:h] ** 2))
        r2 = _true_r2(ctx, x, b, 0.1, True)
        last = ctx.sloppy_last()
        print(f"deflated half solveEE: its {sp.iterations}, true r2/b2 {r2 / b2:.3e}, last {last}")
        assert r2 <= 1e-14 * b2 and abs(sp.r2 - r2 / b2) <= 1e-6 * r2 / b2
        assert last["precision"] == 2 and last["half_iters"] == sp.iterations
    finally:
        B.free()
        ctx.close()
