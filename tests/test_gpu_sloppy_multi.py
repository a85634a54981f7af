"""Mixed-precision multi-shift CG (qexhip_stag_solve_xx_multi_sloppy / dev_solve_xx_multi_sloppy / stag_solve_multi_sloppy): every
shift's TRUE residual recomputed by the fp64 oracle, agreement with the fp64 multi-shift solve inside the bound the two residuals
allow, the refinement phase, sloppy = 0 being the fp64 solve, the full solve, the refusals of the C ABI, ghost zones on one rank,
and the 32^4 Naik 10-shift workload.  Observed values are printed (pytest -s).

Normalisation: the base operator is A_0 = 4 m0^2 - (2D)(2D) on one parity (oracle: stagD2xx(x, m0^2)), shift k is A_k = A_0 + sg_k
= stagD2xx(x, m0^2 + sg_k / 4); D is anti-Hermitian, so lambda_min(A_k) >= c_k = 4 m0^2 + sg_k."""
import ctypes as C
import os
import re
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 987654321
LATS = [[8, 8, 8, 8], [4, 6, 10, 6]]
LINKS = [("random", False), ("warm", False), ("random", True), ("warm", True)]
MASSES = [0.05, 0.1, 0.2, 0.4]
MAXITS = 5000


def shifts_of(masses):
    return [masses[0]] + [4.0 * (m * m - masses[0] ** 2) for m in masses[1:]]      # stagSolve.nim:391-394


class Case:
    """links, source and contexts of one (lattice, links) pair -- as tests/test_gpu_sloppy_batch.py::_setup builds them"""

    def __init__(self, o, lat, kind, naik):
        self.o, self.lat = o, list(lat)
        self.lo = lo = o.Layout(lat)
        rf = o.RngField(lo, o.RNG_MILC6, SEED)
        gen = (lambda: o.gauge_warm(lo, 0.5, rf)) if kind == "warm" else (lambda: o.gauge_random(lo, rf))
        self.fat = gen()
        o.rephase(lo, self.fat)
        self.lng = None
        if naik:
            self.lng = gen()
            o.rephase(lo, self.lng)
        self.b = o.vector_gaussian(lo, rf)
        self.h = lo.vol // 2

    def op(self, halo=False, overlap=None):
        import qex_amd as q

        ctx = q.Context(self.lat)
        if halo:
            ctx.force_halo(True)
            ctx.set_option("emu_exchange_us", 40)
            ctx.set_option("overlap", overlap)
        s = q.newStag3(ctx, self.fat, self.lng) if self.lng is not None else q.newStag(ctx, self.fat)
        return ctx, s

    def half(self, par_even):
        return slice(0, self.h) if par_even else slice(self.h, 2 * self.h)

    def resid(self, x, sh, k, par_even):
        """oracle: (|b - A_k x|, |A_k x|) on the parity"""
        m2 = sh[0] ** 2 + (0.25 * sh[k] if k else 0.0)
        ax = self.o.stagD2xx(self.lo, self.fat, self.lng, x, m2, par_even)
        sl = self.half(par_even)
        return float(np.linalg.norm(self.b[sl] - ax[sl])), float(np.linalg.norm(ax[sl]))


_cases = {}


def case(o, lat, kind, naik):
    key = (tuple(lat), kind, naik)
    if key not in _cases:
        _cases[key] = Case(o, lat, kind, naik)
    return _cases[key]


def run_sloppy(s, K, sh, r2req, par_even, sloppy=1, maxits=MAXITS):
    import qex_amd as q

    xs = [np.zeros_like(K.b) for _ in sh]
    sp = q.SolverParams(r2req=r2req, maxits=maxits, verbosity=0)
    fin = s.solveXX_multi(xs, K.b, sh, sp, parEven=par_even, sloppy=sloppy)
    return xs, sp, fin


def run_fp64(s, K, sh, r2req, par_even, maxits=MAXITS):
    import qex_amd as q

    xs = [np.zeros_like(K.b) for _ in sh]
    sp = q.SolverParams(r2req=r2req, maxits=maxits, verbosity=0)
    s.solveXX_multi(xs, K.b, sh, sp, parEven=par_even)
    return xs, sp


def check_true_residuals(K, sh, xs, fin, r2req, par_even, margin=None, tag=""):
    """item 1: the oracle's |b - A_k x_k|^2/|b|^2 <= r2req (1 + margin), and the returned value agrees with it to the same margin.
    margin None: 1e-4 (the library's and the oracle's fp64 operator differ by <= 1e-13 |A x|; at the tightest case |r| = 1e-7 |b|
    that is 1e-6 relative on |r|).  Else computed per shift from the oracle's |A x|: (1 + 1e-13 |A x| / |r|)^2 - 1."""
    sl = K.half(par_even)
    b2 = float(np.sum(K.b[sl] ** 2))
    out = []
    for k in range(len(sh)):
        r, ax = K.resid(xs[k], sh, k, par_even)
        mg = 1e-4 if margin is None else (1.0 + 1e-13 * ax / max(r, 1e-300)) ** 2 - 1.0
        rel = r * r / b2
        print(f"   {tag} shift {k}: oracle r2/b2 {rel:.4e} returned {fin[k]:.4e} (r2req {r2req:g}, margin {mg:.2e})")
        assert rel <= r2req * (1.0 + mg), (tag, k, rel, r2req)
        assert abs(fin[k] - rel) <= mg * rel + 1e-300, (tag, k, fin[k], rel)
        assert not xs[k][K.half(not par_even)].any()
        out.append(r)
    return out


def check_against_fp64(K, sh, xs, x64, par_even, tag=""):
    """item 2: |x_k - x_k^64| <= (|r_k| + |r_k^64|) / c_k, both residuals by the oracle -- a derived bound (lambda_min(A_k) >= c_k)"""
    sl = K.half(par_even)
    for k in range(len(sh)):
        ck = 4.0 * sh[0] ** 2 + (sh[k] if k else 0.0)
        r = K.resid(xs[k], sh, k, par_even)[0]
        r64 = K.resid(x64[k], sh, k, par_even)[0]
        dx = float(np.linalg.norm(xs[k][sl] - x64[k][sl]))
        print(f"   {tag} shift {k}: |x - x64| {dx:.3e} bound {(r + r64) / ck:.3e} (|r| {r:.3e} |r64| {r64:.3e})")
        assert dx <= (r + r64) / ck, (tag, k, dx, r, r64, ck)


# ---- 1 + 2. the true residual of every shift; agreement with the fp64 multi-shift solve --------------------------------
@pytest.mark.parametrize("kind,naik", LINKS)
@pytest.mark.parametrize("lat", LATS)
def test_true_residual_and_fp64_agreement(oracle, lat, kind, naik):
    K = case(oracle, lat, kind, naik)
    ctx, s = K.op()
    sh = shifts_of(MASSES)
    for par_even in (True, False):
        for r2req in (1e-8, 1e-14):
            xs, sp, fin = run_sloppy(s, K, sh, r2req, par_even)
            x64, sp64 = run_fp64(s, K, sh, r2req, par_even)
            tag = f"{lat} {kind} naik={naik} par_even={par_even} r2req={r2req:g}"
            print(f"{tag}: fp32 its {sp.iterations} updates {sp.reliableUpdates} refine {sp.refineIterations} | fp64 its {sp64.iterations} "
                  f"(ratio {sp.iterations / max(sp64.iterations, 1):.3f})")
            assert sp.iterations < MAXITS and sp.reliableUpdates >= 1
            assert sp.r2 == max(fin) and len(sp.refineIterations) == len(sh) and sp.refineIterations[0] == 0
            check_true_residuals(K, sh, xs, fin, r2req, par_even, tag=tag)
            check_against_fp64(K, sh, xs, x64, par_even, tag=tag)
    ctx.close()


# ---- 3. the refinement path -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("naik,nmass", [(False, 4), (True, 4), (False, 10), (True, 1)])
def test_refinement_is_exercised(oracle, naik, nmass):
    K = case(oracle, [8, 8, 8, 8], "random", naik)
    ctx, s = K.op()
    masses = MASSES if nmass == 4 else [0.05 * 1.4 ** k for k in range(nmass)]       # (10: batches of 4 + 4 + 1 shifts)
    sh = shifts_of(masses)
    r2req = 1e-20
    for par_even in (True, False):
        xs, sp, fin = run_sloppy(s, K, sh, r2req, par_even)
        tag = f"refine naik={naik} nmass={nmass} par_even={par_even}"
        print(f"{tag}: fp32 its {sp.iterations} updates {sp.reliableUpdates} refine {sp.refineIterations}")
        assert sp.iterations < MAXITS and len(sp.refineIterations) == nmass
        check_true_residuals(K, sh, xs, fin, r2req, par_even, margin="oracle", tag=tag)
        if nmass > 1:
            # a true residual of 1e-10 |b| cannot come out of fp32 search directions for the shifted systems, where nothing replaces
            # the residual
            assert sum(sp.refineIterations) > 0 and sp.refineIterations[0] == 0
        else:
            assert sp.refineIterations == [0]
    ctx.close()


# ---- 4. sloppy = 0 is the fp64 solve; SloppyHalf runs single ----------------------------------------------------------
def test_sloppy_zero_is_the_fp64_solve_and_half_is_single(oracle):
    import qex_amd as q

    K = case(oracle, [8, 8, 8, 8], "random", False)
    ctx, s = K.op()
    sh = shifts_of(MASSES)
    for maxits in (MAXITS, 9):
        xa, spa = run_fp64(s, K, sh, 1e-12, True, maxits)
        xb, spb, fin = run_sloppy(s, K, sh, 1e-12, True, sloppy=0, maxits=maxits)
        assert spa.iterations == spb.iterations and spb.reliableUpdates == 0 and spb.refineIterations == [0] * 4
        assert all(np.array_equal(a, b) for a, b in zip(xa, xb))
        spa = q.SolverParams(r2req=1e-12, maxits=maxits, verbosity=0)
        spb = q.SolverParams(r2req=1e-12, maxits=maxits, verbosity=0, sloppySolve=q.SloppySingle)       # the keyword overrides
        ya, yb = [np.zeros_like(K.b) for _ in MASSES], [np.zeros_like(K.b) for _ in MASSES]
        s.solve(ya, K.b, MASSES, spa)
        s.solve(yb, K.b, MASSES, spb, sloppy=0)
        assert (spa.iterations, spa.r2, spb.reliableUpdates) == (spb.iterations, spb.r2, 0)
        assert all(np.array_equal(a, b) for a, b in zip(ya, yb))
    # resident fields
    fb, fx = ctx.field_new(K.b), [ctx.field_new() for _ in sh]
    i0, _ = ctx.dev_solve_xx_multi(fx, fb, sh, 1e-12, MAXITS)
    d0 = [ctx.field_download(f) for f in fx]
    i1, f1, u1, ref1 = ctx.dev_solve_xx_multi(fx, fb, sh, 1e-12, MAXITS, sloppy=0)
    assert i0 == i1 and u1 == 0 and ref1 == [0] * 4 and all(np.array_equal(a, ctx.field_download(f)) for a, f in zip(d0, fx))
    # sloppy = 2 gives the bits of sloppy = 1; the resident entry gives the host entry's
    x1, sp1, fin1 = run_sloppy(s, K, sh, 1e-14, False, sloppy=q.SloppySingle)
    x2, sp2, fin2 = run_sloppy(s, K, sh, 1e-14, False, sloppy=q.SloppyHalf)
    assert (sp1.iterations, sp1.reliableUpdates, sp1.refineIterations, fin1) == (sp2.iterations, sp2.reliableUpdates, sp2.refineIterations, fin2)
    assert all(np.array_equal(a, b) for a, b in zip(x1, x2))
    i3, f3, u3, ref3 = ctx.dev_solve_xx_multi(fx, fb, sh, 1e-14, MAXITS, par_even=False, sloppy=1)
    assert (i3, f3, u3, ref3) == (sp1.iterations, fin1, sp1.reliableUpdates, sp1.refineIterations)
    assert all(np.array_equal(a, ctx.field_download(f)) for a, f in zip(x1, fx))
    # the workspace can be handed back, and the next solve gives the same bits
    from qex_amd._lib import check, lib
    check(lib().qexhip_release_workspace(ctx._h))
    x4, sp4, fin4 = run_sloppy(s, K, sh, 1e-14, False)
    assert fin4 == fin1 and all(np.array_equal(a, b) for a, b in zip(x1, x4))
    ctx.close()


# ---- 5. the full solve ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lat,kind,naik", [([8, 8, 8, 8], "random", False), ([4, 6, 10, 6], "warm", True)])
def test_full_solve(oracle, lat, kind, naik):
    import qex_amd as q

    o = oracle
    K = case(o, lat, kind, naik)
    ctx, s = K.op()
    b2 = float(np.sum(K.b ** 2))
    for r2req in (1e-8, 1e-14):
        sp = q.SolverParams(r2req=r2req, maxits=20000, verbosity=0)
        xs = [np.zeros_like(K.b) for _ in MASSES]
        s.solve(xs, K.b, MASSES, sp, sloppy=1)
        sp64 = q.SolverParams(r2req=r2req, maxits=20000, verbosity=0)
        x64 = [np.zeros_like(K.b) for _ in MASSES]
        s.solve(x64, K.b, MASSES, sp64)
        print(f"solve {lat} {kind} naik={naik} r2req={r2req:g}: fp32 its {sp.iterations} updates {sp.reliableUpdates} r2 {sp.r2:.3e} | "
              f"fp64 its {sp64.iterations} r2 {sp64.r2:.3e}")
        assert sp.calls == 1 and sp.reliableUpdates >= 1 and sp.iterations < 20000
        for k, m in enumerate(MASSES):
            r = float(np.linalg.norm(K.b - o.D(K.lo, K.fat, K.lng, xs[k], m)))
            r64 = float(np.linalg.norm(K.b - o.D(K.lo, K.fat, K.lng, x64[k], m)))
            dx = float(np.linalg.norm(xs[k] - x64[k]))
            print(f"   mass {m}: |b - D x|^2/b2 {r * r / b2:.3e} (fp64 {r64 * r64 / b2:.3e}) |x - x64| {dx:.3e} bound {(r + r64) / m:.3e}")
            if k == 0:
                assert r * r / b2 <= r2req * (1.0 + 1e-4)
            assert dx <= (r + r64) / m          # |D(m) v| >= m |v|: D is anti-Hermitian
    ctx.close()


# ---- 6. refusals through the raw C ABI --------------------------------------------------------------------------------
def test_refusals(oracle):
    from qex_amd._lib import lib

    L = lib()
    K = case(oracle, [8, 8, 8, 8], "random", False)
    ctx, s = K.op()
    ERR_ARG = -1
    n = 33
    xs = [np.full_like(K.b, 3.0) for _ in range(n)]
    ids = [ctx.field_new() for _ in range(4)]
    fb = ctx.field_new(K.b)

    def raw(which, nmass, vals, sloppy):
        xp = (C.c_void_p * n)(*[a.ctypes.data for a in xs])
        v = (C.c_double * max(len(vals), 1))(*vals)
        its, nup = C.c_int(0), C.c_int(0)
        fin, ref = (C.c_double * n)(), (C.c_int * n)()
        if which == "xx":
            return L.qexhip_stag_solve_xx_multi_sloppy(ctx._h, xp, K.b.ctypes.data, v, nmass, 1e-10, 100, 1, sloppy, C.byref(its), fin,
                                                       C.byref(nup), ref)
        if which == "full":
            f1 = C.c_double(0)
            return L.qexhip_stag_solve_multi_sloppy(ctx._h, xp, K.b.ctypes.data, v, nmass, 1e-10, 100, sloppy, C.byref(its), C.byref(f1),
                                                    C.byref(nup))
        xi = (C.c_int * n)(*(ids + [ids[0]] * (n - 4)))
        return L.qexhip_dev_solve_xx_multi_sloppy(ctx._h, xi, fb, v, nmass, 1e-10, 100, 1, sloppy, C.byref(its), fin, None, None)

    good = {"xx": shifts_of(MASSES), "dev": shifts_of(MASSES), "full": MASSES}
    for which in ("xx", "full", "dev"):
        for bad in (3, -1):
            assert raw(which, 4, good[which], bad) == ERR_ARG and b"sloppy" in L.qexhip_last_error(), which
        assert raw(which, 4, [0.0] + list(good[which][1:]), 1) == ERR_ARG and b"mass 0" in L.qexhip_last_error(), which
        for nm in (33, 0):
            assert raw(which, nm, [0.1] * 33, 1) == ERR_ARG and b"nmass" in L.qexhip_last_error(), (which, nm)
        assert all((x == 3.0).all() for x in xs)                  # nothing was solved
        assert raw(which, 4, good[which], 1) == 0                 # and a valid call on the same context succeeds
        if which != "dev":
            assert not (xs[0] == 3.0).all()
            for x in xs[:4]:
                x[:] = 3.0
    ctx.close()


# ---- 7. one rank with ghost zones -------------------------------------------------------------------------------------
@pytest.mark.parametrize("naik", [False, True])
def test_ghost_zones_on_one_rank(oracle, naik):
    K = case(oracle, [8, 8, 8, 8], "random", naik)
    sh = shifts_of(MASSES)
    ctx, s = K.op()
    ref = {(pe, rq): run_sloppy(s, K, sh, rq, pe) for pe in (True, False) for rq in (1e-14, 1e-20)}
    ctx.close()
    # overlap = 0: bit for bit the no-halo context's solve (batched refinement there, one shift at a time here)
    ctx, s = K.op(halo=True, overlap=0)
    assert "halo=1" in ctx.info()
    for (pe, rq), (x0, sp0, fin0) in ref.items():
        xs, sp, fin = run_sloppy(s, K, sh, rq, pe)
        print(f"halo overlap=0 naik={naik} par_even={pe} r2req={rq:g}: its {sp.iterations} updates {sp.reliableUpdates} refine {sp.refineIterations}")
        assert (sp.iterations, sp.reliableUpdates, sp.refineIterations) == (sp0.iterations, sp0.reliableUpdates, sp0.refineIterations)
        assert fin == fin0
        assert all(np.array_equal(a, b) for a, b in zip(xs, x0))
    ctx.close()
    ctx, s = K.op(halo=True, overlap=1)
    for pe in (True, False):
        for rq in (1e-8, 1e-14):
            xs, sp, fin = run_sloppy(s, K, sh, rq, pe)
            x64, sp64 = run_fp64(s, K, sh, rq, pe)
            tag = f"halo overlap=1 naik={naik} par_even={pe} r2req={rq:g}"
            print(f"{tag}: fp32 its {sp.iterations} updates {sp.reliableUpdates} refine {sp.refineIterations} | fp64 its {sp64.iterations}")
            assert sp.iterations < MAXITS
            check_true_residuals(K, sh, xs, fin, rq, pe, tag=tag)
            check_against_fp64(K, sh, xs, x64, pe, tag=tag)
    ctx.close()


# ---- 8. the measurement workload --------------------------------------------------------------------------------------
def _bench_masses_and_shifts():
    """the multi-shift leg's masses and shifts, read from bench.py's text (not imported)"""
    src = open(os.path.join(ROOT, "bench.py")).read()
    leg = src[src.index("def leg_naik_multishift"):]
    ms = re.search(r"^\s*masses = (\[.*\])\s*$", leg, re.M)
    sh = re.search(r"^\s*shifts = (\[.*?\])\s*(#.*)?$", leg, re.M)
    assert ms is not None, "bench.py: no `masses = [...]` line in leg_naik_multishift any more"
    assert sh is not None, "bench.py: no `shifts = [...]` line in leg_naik_multishift any more"
    ms, sh = ms.group(1), sh.group(1)
    assert "HisqCoefs" in leg[:400]
    env = {"np": np, "float": float, "range": range}
    env["masses"] = eval(ms, env)                      # noqa: S307 -- an expression of this repository's own benchmark
    return env["masses"], eval(sh, env)                # noqa: S307


def test_sloppy_multi_32_4_naik_10_shifts(oracle):
    import qex_amd as q

    o = oracle
    lat = [32, 32, 32, 32]
    masses, sh = _bench_masses_and_shifts()
    assert len(sh) == 10 and sh[0] == masses[0]
    lo = q.Layout(lat)
    rf = q.RngField(lat, q.RngMilc6, SEED)
    g = rf.random()
    b = rf.gaussian_vector()
    q.rephase(lo, g)
    ctx = q.Context(lat)
    s = q.Staggered(ctx, g, smear=q.HisqCoefs())
    assert s.links_info()[0] == 16
    r2req = 1e-14

    def solve(sloppy):
        xs = [np.zeros_like(b) for _ in sh]
        sp = q.SolverParams(r2req=r2req, maxits=MAXITS, verbosity=0)
        t0 = time.perf_counter()
        fin = s.solveXX_multi(xs, b, sh, sp, sloppy=sloppy)
        return time.perf_counter() - t0, xs, sp, fin

    solve(1), solve(None)                                                  # warm-up: fp32 links, pools
    t32, xs, sp, fin = min((solve(1) for _ in range(3)), key=lambda r: r[0])
    t64, x64, sp64, _ = min((solve(None) for _ in range(3)), key=lambda r: r[0])
    print(f"32^4 HISQ Naik 10 shifts r2req {r2req:g} (host arrays): sloppy {t32 * 1e3:.1f} ms its {sp.iterations} updates {sp.reliableUpdates} "
          f"refine {sp.refineIterations} | fp64 {t64 * 1e3:.1f} ms its {sp64.iterations}")
    assert sp.iterations < MAXITS
    # item 1 with the oracle on the links the operator holds (the device's HISQ smearing of the same start)
    fl, ll = np.zeros_like(g), np.zeros_like(g)
    q.HisqCoefs().init().smear(ctx, g, fl, ll)
    ctx.close()
    K = Case.__new__(Case)
    K.o, K.lat, K.lo, K.fat, K.lng, K.b, K.h = o, lat, o.Layout(lat), fl, ll, b, lo.vol // 2
    check_true_residuals(K, sh, xs, fin, r2req, True, tag="32^4")
