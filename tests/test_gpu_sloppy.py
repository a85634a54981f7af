"""Mixed-precision staggered CG (SolverParams.sloppySolve): the fp32 operator against the fp64 one and the oracle, the
reliable-update solveXX / solve against the fp64 CG, staleness of the fp32 link copy, and sloppy = 0 being the fp64 solve bit for
bit.  Observed values are printed (pytest -s) and recorded in DESIGN.md."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 987654321


def _setup(o, lat, kind, naik=False):
    import qex_amd as q

    lo = o.Layout(lat)
    rf = o.RngField(lo, o.RNG_MILC6, SEED)
    if kind == "scaled":                               # rows not unitary: the sign format does not apply, fp32 keeps 18 reals
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
    ctx = q.Context(lat)
    s = q.newStag3(ctx, fat, lng) if lng is not None else q.newStag(ctx, fat)
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


# ---- 1. the fp32 operator -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lat", [[8, 8, 8, 8], [4, 6, 10, 6]])
# QEX's g.random is unitary to ~1e-11 (18 reals in fp64, whose bound is 5e-14): well inside the fp32 sign format's 1e-6
@pytest.mark.parametrize("kind,naik,fmt", [("random", False, 1), ("warm", False, 1), ("random", True, 1), ("warm", True, 1),
                                           ("scaled", False, 0), ("scaled", True, 0), ("hisq", True, 0)])
def test_op_xx_sloppy_vs_fp64_and_oracle(oracle, lat, kind, naik, fmt):
    o = oracle
    lo, ctx, s, fat, lng, b = _setup(o, lat, kind, naik)
    f, dev = ctx.links_info_f32()
    assert f == fmt, (f, dev)
    for par_even, m2 in ((True, 0.01), (False, 0.04)):
        sl = _half(lo, par_even)
        fx, f32, f64 = ctx.field_new(b), ctx.field_new(), ctx.field_new()
        ctx.dev_op_xx_sloppy(f32, fx, m2, par_even)
        ctx.dev_op_xx(f64, fx, m2, par_even)
        r32, r64 = ctx.field_download(f32), ctx.field_download(f64)
        for fid in (fx, f32, f64):
            ctx.field_free(fid)
        ref = o.stagD2xx(lo, fat, lng, b, m2, par_even)
        e64, eor = _maxrel(r32[sl], r64[sl]), _maxrel(r32[sl], ref[sl])
        print(f"op_xx_sloppy {lat} {kind} naik={naik} fmt={f} dev={dev:.1e} par_even={par_even}: max rel err vs fp64 {e64:.2e}, "
              f"vs oracle {eor:.2e}")
        assert e64 <= 1e-5 and eor <= 1e-5
        assert not r32[_half(lo, not par_even)].any()        # the other parity is not written


def test_recon_cap_keeps_18_reals(oracle):
    o = oracle
    lo, ctx, s, fat, lng, b = _setup(o, [8, 8, 8, 8], "warm")
    assert ctx.links_info_f32()[0] == 1
    ctx.set_option("recon", 0)
    import qex_amd as q

    q.newStag(ctx, fat)
    assert ctx.links_info_f32()[0] == 0


# ---- 2. sloppy solveXX ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("par_even", [True, False])
@pytest.mark.parametrize("r2req", [1e-8, 1e-14, 1e-20])
@pytest.mark.parametrize("kind", ["random", "warm"])
def test_solveXX_sloppy(oracle, kind, par_even, r2req):
    import qex_amd as q

    o = oracle
    lo, ctx, s, fat, lng, b = _setup(o, [8, 8, 8, 8], kind)
    mass = 0.1
    sl = _half(lo, par_even)
    sp64 = q.SolverParams(r2req=r2req, maxits=5000, verbosity=0)
    x64 = np.zeros_like(b)
    s.solveXX(x64, b, mass, sp64, par_even)
    sp = q.SolverParams(r2req=r2req, maxits=5000, verbosity=0, sloppySolve=q.SloppySingle)
    x = np.zeros_like(b)
    s.solveXX(x, b, mass, sp, par_even)
    b2 = float(np.sum(b[sl] ** 2))
    r2 = _true_r2(ctx, x, b, mass, par_even)
    ratio = sp.iterations / sp64.iterations
    xerr = np.linalg.norm(x[sl] - x64[sl]) / np.linalg.norm(x64[sl])
    print(f"solveXX_sloppy {kind} par_even={par_even} r2req={r2req:g}: its {sp.iterations} vs fp64 {sp64.iterations} "
          f"(ratio {ratio:.3f}), updates {sp.reliableUpdates}, true r2/b2 {r2 / b2:.3e} (reported {sp.r2:.3e}), x rel diff {xerr:.2e}")
    assert r2 <= r2req * b2
    assert abs(sp.r2 - r2 / b2) <= 1e-6 * r2 / b2 + 1e-300
    # |x - x64| <= |A^-1| (|r| + |r64|) and |A^-1| <= 1/(4 m^2): both residuals are below sqrt(r2req) |b|
    assert xerr <= 2 * np.sqrt(r2req) * np.sqrt(b2) / (4 * mass * mass) / np.linalg.norm(x64[sl]) * 1.01
    assert sp.iterations <= 1.5 * sp64.iterations
    if r2req <= 1e-14:
        assert sp.reliableUpdates >= 1
    assert not x[_half(lo, not par_even)].any()


def test_solveXX_sloppy_resident_and_half(oracle):
    """dev_solve_xx_sloppy on resident fields; SloppyHalf runs single: the same iterations and bits"""
    import qex_amd as q

    o = oracle
    lo, ctx, s, fat, lng, b = _setup(o, [8, 8, 8, 8], "random")
    fb, fx = ctx.field_new(b), ctx.field_new()
    its, fin, nup = ctx.dev_solve_xx_sloppy(fx, fb, 0.1, 1e-14, 5000, True, q.SloppySingle)
    x1 = ctx.field_download(fx)
    its2, fin2, nup2 = ctx.dev_solve_xx_sloppy(fx, fb, 0.1, 1e-14, 5000, True, q.SloppyHalf)
    x2 = ctx.field_download(fx)
    assert (its, fin, nup) == (its2, fin2, nup2) and np.array_equal(x1, x2)
    assert fin <= 1e-14 and nup >= 1
    # maxits: not an error, and the reported residual is the true one of the returned x
    its3, fin3, nup3 = ctx.dev_solve_xx_sloppy(fx, fb, 0.1, 1e-14, 10, True, q.SloppySingle)
    x3 = ctx.field_download(fx)
    b2 = float(np.sum(b[: lo.vol // 2] ** 2))
    assert its3 == 10 and nup3 >= 1 and fin3 > 1e-14
    assert abs(fin3 - _true_r2(ctx, x3, b, 0.1, True) / b2) <= 1e-6 * fin3
    ctx.field_free(fb)
    ctx.field_free(fx)


# ---- 3. full solve ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("branch", ["reconL", "reconR"])
@pytest.mark.parametrize("source", ["point", "random"])
def test_solve_sloppy_full(oracle, branch, source):
    import qex_amd as q

    o = oracle
    lo, ctx, s, fat, lng, b = _setup(o, [8, 8, 8, 8], "random")
    if source == "point":
        b = np.zeros_like(b)
        b[0, 0, 0] = 1.0                               # even site: b.odd = 0 takes solveReconR, the other parity reconL
    if branch == "reconR":
        b[lo.vol // 2:] = 0.0
    elif source == "point":
        b[lo.vol // 2 + 3, 1, 0] = 1.0                 # both parities: solveReconL
    m, r2req = 0.1, 1e-12
    sp = q.SolverParams(r2req=r2req, maxits=5000, verbosity=0, sloppySolve=q.SloppySingle)
    x = np.zeros_like(b)
    s.solve(x, b, m, sp)
    res = b - o.D(lo, fat, None, x, m)
    rel = float(np.sum(res ** 2) / np.sum(b ** 2))
    print(f"solve_sloppy {branch} {source}: its {sp.iterations} updates {sp.reliableUpdates} |b-Dx|^2/|b|^2 {rel:.3e} (reported {sp.r2:.3e})")
    assert rel <= r2req and sp.r2 <= r2req and sp.reliableUpdates >= 1
    # usePrevSoln: restart from the solution with a tighter tolerance
    sp2 = q.SolverParams(r2req=1e-18, maxits=5000, verbosity=0, usePrevSoln=True, sloppySolve=q.SloppySingle)
    s.solve(x, b, m, sp2)
    res = b - o.D(lo, fat, None, x, m)
    rel2 = float(np.sum(res ** 2) / np.sum(b ** 2))
    print(f"  usePrevSoln r2req 1e-18: its {sp2.iterations} |b-Dx|^2/|b|^2 {rel2:.3e}")
    assert rel2 <= 1e-18 and sp2.r2 <= 1e-18


# ---- 4. the fp32 links follow every change of the operator ----------------------------------------------------------
def test_stale_links_are_rebuilt(oracle):
    import qex_amd as q

    o = oracle
    lat = [8, 8, 8, 8]
    lo, ctx, s, fatA, lng, b = _setup(o, lat, "random")
    rf = o.RngField(lo, o.RNG_MILC6, 12345)
    fatB = o.gauge_random(lo, rf)
    o.rephase(lo, fatB)
    spA = q.SolverParams(r2req=1e-14, maxits=5000, verbosity=0, sloppySolve=q.SloppySingle)
    x = np.zeros_like(b)
    s.solveEE(x, b, 0.1, spA)

    def check_on(fat):
        sp = q.SolverParams(r2req=1e-14, maxits=5000, verbosity=0, sloppySolve=q.SloppySingle)
        sp64 = q.SolverParams(r2req=1e-14, maxits=5000, verbosity=0)
        xs, x64 = np.zeros_like(b), np.zeros_like(b)
        st = q.newStag(ctx, fat)
        st.solveEE(xs, b, 0.1, sp)
        st.solveEE(x64, b, 0.1, sp64)
        h = lo.vol // 2
        # the fp32 operator is B's, not A's
        fx, f32 = ctx.field_new(b), ctx.field_new()
        ctx.dev_op_xx_sloppy(f32, fx, 0.01, True)
        r32 = ctx.field_download(f32)
        ctx.field_free(fx)
        ctx.field_free(f32)
        ref = o.stagD2xx(lo, fat, None, b, 0.01, True)
        assert _maxrel(r32[:h], ref[:h]) <= 1e-5
        xerr = np.linalg.norm(xs[:h] - x64[:h]) / np.linalg.norm(x64[:h])
        assert xerr <= 1e-5 and sp.iterations <= 1.5 * sp64.iterations, (xerr, sp.iterations, sp64.iterations)
        return sp.iterations, sp64.iterations

    print("links B:", check_on(fatB))
    # an MD link update (exp(t p) g on the device), then the operator rebuilt from the updated links
    p = o.gauge_random_tah(lo, rf)
    gC = fatA.copy()
    q.gaugeUpdate(ctx, gC, p, 0.05)
    assert not np.array_equal(gC, fatA)
    print("links after MD update:", check_on(gC))


# ---- 5. sloppy = 0 is the fp64 solve, bad values are refused -------------------------------------------------------
def test_sloppy_zero_is_bit_identical_and_bad_values_refused(oracle):
    import qex_amd as q
    from qex_amd._lib import lib

    o = oracle
    lo, ctx, s, fat, lng, b = _setup(o, [8, 8, 8, 8], "random")
    L = lib()
    for maxits in (5000, 17):
        x0, x1 = np.zeros_like(b), np.zeros_like(b)
        its0, fin0 = C.c_int(0), C.c_double(0)
        its1, fin1, nup = C.c_int(0), C.c_double(0), C.c_int(-5)
        hist = np.zeros(1)
        pv = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        assert L.qexhip_stag_solve_xx(ctx._h, pv(x0), pv(b), 0.1, 1e-14, maxits, 1, C.byref(its0), C.byref(fin0), pv(hist), 0) == 0
        assert L.qexhip_stag_solve_xx_sloppy(ctx._h, pv(x1), pv(b), 0.1, 1e-14, maxits, 1, 0, C.byref(its1), C.byref(fin1),
                                             C.byref(nup)) == 0
        assert its0.value == its1.value and fin0.value == fin1.value and np.array_equal(x0, x1) and nup.value == 0
        if maxits == 17:
            assert its1.value == 17
        y0, y1 = np.zeros_like(b), np.zeros_like(b)
        assert L.qexhip_stag_solve_prev(ctx._h, pv(y0), pv(b), 0.1, 1e-14, maxits, 0, C.byref(its0), C.byref(fin0)) == 0
        assert L.qexhip_stag_solve_sloppy(ctx._h, pv(y1), pv(b), 0.1, 1e-14, maxits, 0, 0, C.byref(its1), C.byref(fin1),
                                          C.byref(nup)) == 0
        assert its0.value == its1.value and fin0.value == fin1.value and np.array_equal(y0, y1)
    # the Python layer with sloppySolve = 0 takes the fp64 entries
    sp, spn = q.SolverParams(r2req=1e-14, verbosity=0), q.SolverParams(r2req=1e-14, verbosity=0, sloppySolve=q.SloppyNone)
    xa, xb = np.zeros_like(b), np.zeros_like(b)
    s.solveEE(xa, b, 0.1, sp)
    s.solveEE(xb, b, 0.1, spn)
    assert np.array_equal(xa, xb) and sp.iterations == spn.iterations
    for bad in (-1, 3, 7):
        x = np.zeros_like(b)
        rc = L.qexhip_stag_solve_xx_sloppy(ctx._h, x.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), 0.1, 1e-14, 100, 1,
                                           bad, None, None, None)
        assert rc == -1 and b"sloppy" in L.qexhip_last_error()
        rc = L.qexhip_stag_solve_sloppy(ctx._h, x.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), 0.1, 1e-14, 100, 0, bad,
                                        None, None, None)
        assert rc == -1
        rc = L.qexhip_dev_solve_xx_sloppy(ctx._h, 1, 2, 0.1, 1e-14, 100, 1, bad, None, None, None)
        assert rc == -1
    with pytest.raises(ValueError):
        s.solve([np.zeros_like(b)] * 2, b, [0.1, 0.2], q.SolverParams(sloppySolve=q.SloppySingle))


# ---- 6. the bench workload ------------------------------------------------------------------------------------------
def test_sloppy_32_4_bench_workload(oracle):
    import time
    import qex_amd as q

    o = oracle
    lo, ctx, s, fat, lng, b = _setup(o, [32, 32, 32, 32], "random")
    assert ctx.links_info_f32()[0] == 1
    r2req, mass = 1e-14, 0.1
    x64, x = np.zeros_like(b), np.zeros_like(b)
    sp64 = q.SolverParams(r2req=r2req, maxits=10000, verbosity=0)
    sp = q.SolverParams(r2req=r2req, maxits=10000, verbosity=0, sloppySolve=q.SloppySingle)
    s.solveEE(x, b, mass, sp)                      # warm-up: the fp32 link copy is built here
    s.solveEE(x64, b, mass, sp64)
    sp.resetStats()
    sp64.resetStats()
    t0 = time.perf_counter()
    s.solveEE(x64, b, mass, sp64)
    t64 = time.perf_counter() - t0
    t0 = time.perf_counter()
    s.solveEE(x, b, mass, sp)
    t32 = time.perf_counter() - t0
    h = lo.vol // 2
    b2 = float(np.sum(b[:h] ** 2))
    r2 = _true_r2(ctx, x, b, mass, True)
    print(f"32^4 solveEE r2req 1e-14: fp64 {sp64.iterations} its {t64 * 1e3:.1f} ms ({t64 / sp64.iterations * 1e6:.1f} us/it); "
          f"sloppy {sp.iterations} its {t32 * 1e3:.1f} ms ({t32 / sp.iterations * 1e6:.1f} us/it), {sp.reliableUpdates} updates, "
          f"true r2/b2 {r2 / b2:.3e}; speedup {t64 / t32:.2f}x")
    assert r2 <= r2req * b2 and sp.reliableUpdates >= 1
