"""The 16-bit lock-step batch (option "half_batch" = 1, sloppy = 2 on the batched entries): the multi-right-hand-side 16-bit sweep
against the single-system 16-bit operator and every system of a batched solve against its own single-system SloppyHalf solve, BIT
FOR BIT -- solution, iterations (16-bit plus fp32), true residual, reliable updates, fall-back -- on 8^4 and 4.6.10.6 (Vh = 720: the
last 64-site tile and the last 256-lane workgroup are partial, every extent differs).  The single operator and solve are pinned to
the fp64 ones and to the numpy model of the format by tests/test_gpu_half.py, so no tolerance appears here except where a fp64 result
is compared.  Observed values are printed (pytest -s)."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 987654321
LATS = [[8, 8, 8, 8], [4, 6, 10, 6]]
LINKS = [("random", False, 1), ("random", True, 1), ("scaled", False, 0), ("hisq", True, 0)]
MS = [0.1, 0.2, 0.15, 0.3]
R2 = [1e-8, 1e-14, 1e-20, 1e-14]
M2 = [0.01, 0.04, 0.0225, 0.09]


@functools.lru_cache(maxsize=None)
def _inputs(lat, kind, naik):
    """links as tests/test_gpu_half.py builds them and four distinct gaussian sources, once per (lattice, kind)"""
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
        fat = o.gauge_random(lo, rf)
        o.rephase(lo, fat)
        lng = None
        if naik:
            lng = o.gauge_random(lo, rf)
            o.rephase(lo, lng)
    bs = tuple(o.vector_gaussian(lo, rf) for _ in range(4))
    for a in (fat, lng) + bs:
        if a is not None:
            a.setflags(write=False)
    return lo, fat, lng, bs


def _setup(lat, kind, naik=False, half=1, half_batch=1, halo=False):
    import qex_amd as q

    lo, fat, lng, bs = _inputs(tuple(lat), kind, naik)
    ctx = q.Context(list(lat))
    if halo:
        ctx.force_halo(True)
    s = q.newStag3(ctx, fat, lng) if lng is not None else q.newStag(ctx, fat)
    ctx.set_option("half", half)
    ctx.set_option("half_batch", half_batch)
    return lo, ctx, s, fat, lng, list(bs)


def _half(lo, par_even):
    h = lo.vol // 2
    return slice(0, h) if par_even else slice(h, lo.vol)


def _single_xx(ctx, b, m, r2req, maxits, par_even, sloppy=2):
    """qexhip_dev_solve_xx_sloppy for one system: (x, iterations, true r2/b2, updates, sloppy_last)"""
    fb, fx = ctx.field_new(b), ctx.field_new()
    try:
        its, fin, nup = ctx.dev_solve_xx_sloppy(fx, fb, m, r2req, maxits, par_even, sloppy)
        return ctx.field_download(fx), its, fin, nup, ctx.sloppy_last()
    finally:
        ctx.field_free(fb)
        ctx.field_free(fx)


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


def _batch_vs_single(tag, ctx, s, lo, bs, ms, r2, maxits, par_even):
    """one batched solveXX against the single solves of its systems; returns the batch's (its, fin, nup, last)"""
    n = len(bs)
    xs = [np.zeros_like(b) for b in bs]
    its, fin, nup = s.solveXX_batch(xs, bs, ms, r2, maxits, par_even, sloppy=2)
    last = ctx.sloppy_last_batch()
    assert len(last) == n, (tag, last)
    for j in range(n):
        x1, its1, fin1, nup1, last1 = _single_xx(ctx, bs[j], ms[j], r2[j], maxits, par_even)
        t = (tag, n, j)
        assert (its[j], nup[j]) == (its1, nup1), (t, its[j], its1, nup[j], nup1)
        assert fin[j] == fin1, (t, fin[j], fin1)
        assert np.array_equal(xs[j], x1), (t, float(np.abs(xs[j] - x1).max()))
        assert last[j] == last1, (t, last[j], last1)
        assert not xs[j][_half(lo, not par_even)].any()
    return xs, its, fin, nup, last


# ---- 1. the sweep ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lat", LATS)
@pytest.mark.parametrize("kind,naik,fmt", LINKS)
def test_sweep_equals_the_single_operator(oracle, lat, kind, naik, fmt):
    lo, ctx, s, fat, lng, bs = _setup(lat, kind, naik, half=0, half_batch=0)      # the probes need neither option
    assert ctx.links_info_half()[0] == fmt
    fx = [ctx.field_new(b) for b in bs]
    for par_even in (True, False):
        single = []
        for j in range(4):
            fh = ctx.field_new()
            ctx.dev_op_xx_half(fh, fx[j], M2[j], par_even)
            single.append(ctx.field_download(fh))
            ctx.field_free(fh)
            assert single[j][_half(lo, par_even)].any()
        for n in (1, 2, 3, 4):
            fr = [ctx.field_new() for _ in range(n)]
            ctx.dev_op_xx_half_batch(fr, fx[:n], M2[:n], par_even)
            for j in range(n):
                r = ctx.field_download(fr[j])
                assert np.array_equal(r, single[j]), (lat, kind, par_even, n, j, float(np.abs(r - single[j]).max()))
                assert not r[_half(lo, not par_even)].any()
            for f in fr:
                ctx.field_free(f)
    ctx.close()


# ---- 2. solveXX -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("par_even", [True, False])
@pytest.mark.parametrize("lat", LATS)
@pytest.mark.parametrize("kind,naik,fmt", LINKS)
def test_solveXX_batch_equals_single_half(oracle, lat, kind, naik, fmt, par_even):
    lo, ctx, s, fat, lng, bs = _setup(lat, kind, naik)
    sl = _half(lo, par_even)
    for n in (4, 3, 2, 1):
        xs, its, fin, nup, last = _batch_vs_single((lat, kind, par_even), ctx, s, lo, bs[:n], MS[:n], R2[:n], 5000, par_even)
        print(f"half batch {lat} {kind} naik={naik} par_even={par_even} n={n}: its {its} updates {nup} r2/b2 {fin} last {last}")
        for j in range(n):
            b2 = float(np.sum(bs[j][sl] ** 2))
            assert last[j]["precision"] == 2 and last[j]["half_iters"] + last[j]["f32_iters"] == its[j]
            assert _true_r2(ctx, xs[j], bs[j], MS[j], par_even) <= R2[j] * b2
    # shared maxits: not an error, and the reported residual is the true one of the returned x
    xs, its, fin, nup, last = _batch_vs_single((lat, kind, par_even, "maxits"), ctx, s, lo, bs, MS, R2, 10, par_even)
    for j in range(4):
        b2 = float(np.sum(bs[j][sl] ** 2))
        assert its[j] == 10 and nup[j] >= 1
        assert abs(fin[j] - _true_r2(ctx, xs[j], bs[j], MS[j], par_even) / b2) <= 1e-6 * fin[j]
    ctx.close()


# ---- 3. full solve --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,naik", [("random", False), ("hisq", True)])
def test_full_solve_batch_equals_single_solves(oracle, kind, naik):
    import qex_amd as q

    lo, ctx, s, fat, lng, bs = _setup([8, 8, 8, 8], kind, naik)
    r2 = [1e-8, 1e-14, 1e-18, 1e-12]
    sps = [q.SolverParams(r2req=r, maxits=5000, verbosity=0) for r in r2]
    xs = [np.zeros_like(b) for b in bs]
    s.solve_batch(xs, bs, MS, sps, sloppy=2)
    last = ctx.sloppy_last_batch()
    fb, fx = [ctx.field_new(b) for b in bs], [ctx.field_new() for _ in bs]
    dits, dfin, dnup = ctx.dev_solve_batch(fx, fb, MS, r2, 5000, sloppy=2)
    for j in range(4):
        sp = q.SolverParams(r2req=r2[j], maxits=5000, verbosity=0, sloppySolve=q.SloppyHalf)
        x1 = np.zeros_like(bs[j])
        s.solve(x1, bs[j], MS[j], sp)
        l1 = ctx.sloppy_last()
        print(f"full half batch {kind} system {j}: its {sps[j].iterations} updates {sps[j].reliableUpdates} r2 {sps[j].r2:.3e} last {last[j]}")
        assert np.array_equal(xs[j], x1), (j, float(np.abs(xs[j] - x1).max()))
        assert (sps[j].iterations, sps[j].r2, sps[j].reliableUpdates) == (sp.iterations, sp.r2, sp.reliableUpdates), j
        assert last[j] == l1 and l1["precision"] == 2, (j, last[j], l1)
        assert sp.r2 <= r2[j]
        assert np.array_equal(ctx.field_download(fx[j]), xs[j])
        assert (dits[j], dfin[j], dnup[j]) == (sp.iterations, sp.r2, sp.reliableUpdates), j
    ctx.close()


# ---- 4. the stall guard, per system -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("par_even", [True, False])
def test_stall_guard_per_system(oracle, par_even):
    lo, ctx, s, fat, lng, bs = _setup([8, 8, 8, 8], "random")
    ctx.set_option("half_stall", 0)                      # every system hands over to fp32 at its first reliable update
    r2 = [1e-14, 1e-14, 1e-20, 1e-14]                    # (1e-8 may be met by the first update, which is no hand-over)
    xs, its, fin, nup, last = _batch_vs_single(("stall0", par_even), ctx, s, lo, bs, MS, r2, 5000, par_even)
    print(f"stall guard 0 par_even={par_even}: its {its} updates {nup} last {last}")
    sl = _half(lo, par_even)
    for j in range(4):
        assert last[j]["fell_back"] == 1 and last[j]["half_iters"] > 0 and last[j]["f32_iters"] > 0
        assert last[j]["half_iters"] + last[j]["f32_iters"] == its[j]
        assert _true_r2(ctx, xs[j], bs[j], MS[j], par_even) <= r2[j] * float(np.sum(bs[j][sl] ** 2))
    ctx.set_option("half_stall", 2)
    xs, its, fin, nup, last = _batch_vs_single(("stall2", par_even), ctx, s, lo, bs, MS, r2, 5000, par_even)
    for j in range(4):
        assert last[j] == dict(precision=2, half_iters=its[j], f32_iters=0, fell_back=0)
    ctx.close()


# ---- 5. the switch ------------------------------------------------------------------------------------------------------------
def test_switch_leaves_other_paths_alone(oracle):
    import qex_amd as q

    lo, ctx, s, fat, lng, bs = _setup([8, 8, 8, 8], "random", half=0, half_batch=0)
    b, b2v = bs[0], bs[1]

    def run():
        out = {}
        for name, sl in (("single", q.SloppySingle), ("fp64", q.SloppyNone), ("half", q.SloppyHalf)):
            sp = q.SolverParams(r2req=1e-14, maxits=5000, verbosity=0, sloppySolve=sl)
            x = np.zeros_like(b)
            s.solveEE(x, b, 0.1, sp)
            out[name] = (x, sp.iterations, sp.r2, sp.reliableUpdates)
        for sl in (0, 1, 2):
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
    assert same(off["batch2"], off["batch1"]) and same(off["half"], off["single"])
    ctx.set_option("half_batch", 1)                       # "half" stays 0: the option does not depend on it
    on = run()
    for k in ("single", "fp64", "half", "batch0", "batch1", "multi0", "multi1", "multi2"):
        assert same(on[k], off[k]), k
    assert not same(on["batch2"][:2], on["batch1"][:2])   # the 16-bit batch is another computation
    assert [d["precision"] for d in ctx.sloppy_last_batch()] == [2, 2]      # (the multi-shift solve is no batched entry)
    ctx.set_option("half_batch", 0)
    back = run()
    assert same(back["batch2"], off["batch1"]) and same(back["batch1"], off["batch1"])
    ctx.close()


# ---- 6. refusals, before any launch -------------------------------------------------------------------------------------------
def _raw(L, ctx, which, n, xs, bs, ms, r2, maxits, sloppy, ids=None):
    xp = (C.c_void_p * len(xs))(*[a.ctypes.data for a in xs])
    bp = (C.c_void_p * len(bs))(*[a.ctypes.data for a in bs])
    mv, rv = (C.c_double * len(ms))(*ms), (C.c_double * len(r2))(*r2)
    k = max(n, 1)
    its, fin, nup = (C.c_int * k)(), (C.c_double * k)(), (C.c_int * k)()
    if which == "xx":
        return L.qexhip_stag_solve_xx_batch_sloppy(ctx._h, n, xp, bp, mv, rv, maxits, 1, sloppy, its, fin, nup)
    if which == "full":
        return L.qexhip_stag_solve_batch_sloppy(ctx._h, n, xp, bp, mv, rv, maxits, sloppy, its, fin, nup)
    xi, bi = (C.c_int * len(ids[0]))(*ids[0]), (C.c_int * len(ids[1]))(*ids[1])
    return L.qexhip_dev_solve_batch_sloppy(ctx._h, n, xi, bi, mv, rv, maxits, sloppy, its, fin, nup)


def test_refusals(oracle):
    from qex_amd._lib import lib

    L = lib()
    lo, ctx, s, fat, lng, bs4 = _setup([8, 8, 8, 8], "random")
    bs = bs4 + [bs4[0]]
    for bad in (2, -1):
        assert L.qexhip_set_option(ctx._h, b"half_batch", bad) == -1 and b"half_batch" in L.qexhip_last_error()
    ids = ([ctx.field_new() for _ in range(5)], [ctx.field_new(b) for b in bs])
    for which in ("xx", "full", "dev"):
        xs = [np.full_like(b, 3.0) for b in bs]
        two = (ids[0][:2], ids[1][:2])
        assert _raw(L, ctx, which, 2, xs[:2], bs[:2], [0.1, 0.0], [1e-10, 1e-10], 100, 2, two) == -1        # mass 0
        assert b"mass" in L.qexhip_last_error()
        assert _raw(L, ctx, which, 5, xs, bs, [0.1] * 5, [1e-10] * 5, 100, 2, ids) == -1                     # n = 5
        assert all((x == 3.0).all() for x in xs)                 # nothing was solved
        assert _raw(L, ctx, which, 2, xs[:2], bs[:2], [0.1, 0.2], [1e-10, 1e-10], 100, 2, two) == 0          # and the good call runs
        assert [d["precision"] for d in ctx.sloppy_last_batch()] == [2, 2]
    assert L.qexhip_dev_op_xx_half_batch(ctx._h, 5, (C.c_int * 5)(*ids[0]), (C.c_int * 5)(*ids[1]), (C.c_double * 5)(*[0.01] * 5), 1) == -1
    ctx.close()
    # a context with ghost zones in t: the sloppy batch's existing error, whatever the option says
    lo, ctx, s, fat, lng, bs = _setup([8, 8, 8, 8], "random", halo=True)
    ids = ([ctx.field_new() for _ in range(2)], [ctx.field_new(b) for b in bs[:2]])
    xs = [np.full_like(b, 3.0) for b in bs[:2]]
    for which in ("xx", "full", "dev"):
        rc = _raw(L, ctx, which, 2, xs, bs[:2], [0.1, 0.2], [1e-10, 1e-10], 100, 2, ids)
        msg = L.qexhip_last_error().decode()
        assert rc == -1 and "shard" in msg, (which, rc, msg)
        assert all((x == 3.0).all() for x in xs)
    ctx.close()


# ---- 7. the 16-bit links follow a change of the operator ------------------------------------------------------------------
def test_stale_links_are_rebuilt(oracle):
    import qex_amd as q

    o = oracle
    lo, ctx, s, fatA, lng, bs = _setup([8, 8, 8, 8], "random")
    xsA = [np.zeros_like(b) for b in bs]
    s.solveXX_batch(xsA, bs, MS, R2, 5000, True, sloppy=2)
    rf = o.RngField(lo, o.RNG_MILC6, 12345)
    fatB = o.gauge_random(lo, rf)
    o.rephase(lo, fatB)
    st = q.newStag(ctx, fatB)
    xs, its, fin, nup, last = _batch_vs_single("stale", ctx, st, lo, bs, MS, R2, 5000, True)
    h = lo.vol // 2
    for j in range(4):
        assert not np.array_equal(xs[j], xsA[j])
        assert _true_r2(ctx, xs[j], bs[j], MS[j], True) <= R2[j] * float(np.sum(bs[j][:h] ** 2))      # (the fp64 operator is B's)
        assert last[j]["fell_back"] == 0
    ctx.close()


# ---- 8. the deflated batch ----------------------------------------------------------------------------------------------------
def test_deflated_batch_runs_half(oracle):
    import qex_amd as q
    import eig_ref as R

    o = oracle
    lat = (4, 4, 8, 8)
    lo, g, _, b0 = R.inputs(lat)
    rf = o.RngField(lo, o.RNG_MILC6, 4711)
    bs = [np.ascontiguousarray(b0)] + [o.vector_gaussian(lo, rf) for _ in range(3)]
    ctx = q.Context(list(lat), device=0)
    s = q.newStag(ctx, g)
    B = s.eigs(16, nvecs=40, relerr=0.0, abserr=1e-9, cheb_degree=8, cheb_lo=0.3, cheb_hi=0.0, max_restarts=40)
    try:
        ctx.set_option("half_batch", 1)
        ms, r2 = [0.1, 0.05, 0.15, 0.1], [1e-14, 1e-12, 1e-16, 1e-10]
        for par_even in (True, False):
            sl = _half(lo, par_even)
            xu = [np.zeros_like(b) for b in bs]
            its_u, fin_u, nup_u = s.solveXX_batch(xu, bs, ms, r2, 5000, par_even, sloppy=2)
            xd = [np.zeros_like(b) for b in bs]
            its_d, fin_d, nup_d = s.solveXX_batch(xd, bs, ms, r2, 5000, par_even, sloppy=2, deflate=B)
            last = ctx.sloppy_last_batch()
            print(f"deflated half batch par_even={par_even}: its {its_d} (undeflated {its_u}) updates {nup_d} r2/b2 {fin_d} last {last}")
            for j in range(4):
                b2 = float(np.sum(bs[j][sl] ** 2))
                assert last[j]["precision"] == 2 and last[j]["half_iters"] + last[j]["f32_iters"] == its_d[j]
                assert _true_r2(ctx, xd[j], bs[j], ms[j], par_even) <= r2[j] * b2
                assert its_d[j] <= its_u[j], (j, its_d[j], its_u[j])
    finally:
        B.free()
        ctx.close()


# ---- 9. scalar trace ------------------------------------------------------------------------------------------------------------
def test_scalar_trace_does_not_depend_on_the_batch(oracle):
    import qex_amd as q

    lat = [8, 8, 8, 8]
    lo, ctx, s, fat, lng, _ = _setup(lat, "hisq", True)
    qlo = q.Layout(lat)
    mass, r2req = 0.1, 1e-12

    def trace(**kw):
        lines = []
        tr, est, st = q.scalarTrace(s, qlo, q.RngField(lat, q.RngMilc6, SEED), mass, r2req, source_type="Z4", dilute_type="EO",
                                    improved_trace=False, out=lines.append, **kw)
        return tr[0], st, [float(ln.split(":")[1]) for ln in lines if ln.startswith("src norm2")]

    t4, st4, src4 = trace(sloppy=2, batch=4)
    assert all(d["precision"] == 2 for d in ctx.sloppy_last_batch())
    t1, st1, src1 = trace(sloppy=2, batch=1)
    assert np.array_equal(t4, t1) and st4["iterations"] == st1["iterations"] and st4["updates"] == st1["updates"]
    t64, st64, src64 = trace(sloppy=0, batch=4)
    assert src4 == src64 and len(src64) == 2 * lat[3]
    # per solve |x - x64| <= 2 sqrt(r2req) |b| / m (||(D+m)^-1|| <= 1/m), so its contribution sum_x |b(x)^+ (x - x64)(x)| to the trace is at
    # most |b| 2 sqrt(r2req) |b| / m; the trace carries 1/nc
    bound = sum(2.0 * np.sqrt(r2req) * b2 / mass for b2 in src64) / 3.0
    diff = float(np.abs((t4[:, 0] - t64[:, 0]) + 1j * (t4[:, 1] - t64[:, 1])).sum())
    print(f"scalar trace 16-bit vs fp64: sum |diff| {diff:.3e}, bound {bound:.3e}; iterations {st4['iterations'][0]} vs {st64['iterations'][0]}")
    assert 0 < diff <= bound
    ctx.close()
