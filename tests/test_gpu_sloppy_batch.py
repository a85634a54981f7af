"""Mixed-precision lock-step batched CG (qexhip_stag_solve_xx_batch_sloppy / solve_batch_sloppy / dev_solve_batch_sloppy): every
system of a batch against the single-system sloppy solve of that system BIT FOR BIT (solution, fp32 iterations, true residual,
reliable updates), the true residual recomputed with the fp64 operator, sloppy = 0 being the fp64 batch, the refusals, the staleness
of the fp32 link copy, the meson tables, and the 32^4 workload.  Observed values are printed (pytest -s)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 987654321
LATS = [[8, 8, 8, 8], [4, 6, 10, 6]]
LINKS = [("random", False), ("warm", False), ("random", True), ("warm", True)]
MS = [0.1, 0.2, 0.4, 0.05]
R2 = [1e-14, 1e-12, 1e-16, 1e-12]


def _setup(o, lat, kind, naik=False, halo=False):
    import qex_amd as q

    lo = o.Layout(lat)
    rf = o.RngField(lo, o.RNG_MILC6, SEED)
    gen = (lambda: o.gauge_warm(lo, 0.5, rf)) if kind == "warm" else (lambda: o.gauge_random(lo, rf))
    fat = gen()
    o.rephase(lo, fat)
    lng = None
    if naik:
        lng = gen()
        o.rephase(lo, lng)
    ctx = q.Context(lat)
    if halo:
        ctx.force_halo(True)
    s = q.newStag3(ctx, fat, lng) if lng is not None else q.newStag(ctx, fat)
    return lo, rf, ctx, s, fat, lng


def _half(lo, par_even):
    h = lo.vol // 2
    return slice(0, h) if par_even else slice(h, lo.vol)


def _single_xx(ctx, b, m, r2req, maxits, par_even, sloppy=1):
    """qexhip_dev_solve_xx_sloppy for one system: (x, fp32 iterations, true r2/b2, updates)"""
    fb, fx = ctx.field_new(b), ctx.field_new()
    try:
        its, fin, nup = ctx.dev_solve_xx_sloppy(fx, fb, m, r2req, maxits, par_even, sloppy)
        return ctx.field_download(fx), its, fin, nup
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


def _assert_same(tag, got, ref):
    (x, its, fin, nup), (x1, its1, fin1, nup1) = got, ref
    assert (its, nup) == (its1, nup1), (tag, its, its1, nup, nup1)
    assert fin == fin1, (tag, fin, fin1)
    assert np.array_equal(x, x1), (tag, float(np.abs(x - x1).max()))


# ---- 1. batch equals single, bit for bit ----------------------------------------------------------------------------
@pytest.mark.parametrize("par_even", [True, False])
@pytest.mark.parametrize("kind,naik", LINKS)
@pytest.mark.parametrize("lat", LATS)
def test_solveXX_batch_sloppy_equals_single(oracle, lat, kind, naik, par_even):
    o = oracle
    lo, rf, ctx, s, fat, lng = _setup(o, lat, kind, naik)
    assert ctx.links_info_f32()[0] == 1
    bs = [o.vector_gaussian(lo, rf) for _ in MS]
    ref = [_single_xx(ctx, bs[j], MS[j], R2[j], 5000, par_even) for j in range(4)]
    for n in (4, 3, 2, 1):
        xs = [np.zeros_like(b) for b in bs[:n]]
        its, fin, nup = s.solveXX_batch(xs, bs[:n], MS[:n], R2[:n], 5000, par_even, sloppy=1)
        print(f"solveXX_batch sloppy {lat} {kind} naik={naik} par_even={par_even} n={n}: its {its} updates {nup} r2/b2 {fin}")
        for j in range(n):
            _assert_same((n, j), (xs[j], its[j], fin[j], nup[j]), ref[j])
            assert not xs[j][_half(lo, not par_even)].any()
            assert nup[j] >= 1 and its[j] < 5000
    # r2req = 0 with a small shared maxits: every system stops there, behind at least one reliable update; a zero source is done at once
    bz = [bs[0], np.zeros_like(bs[1]), bs[2], bs[3]]
    xs = [np.ones_like(b) for b in bz]
    its, fin, nup = s.solveXX_batch(xs, bz, MS, 0.0, 7, par_even, sloppy=1)
    assert its == [7, 0, 7, 7] and nup[1] == 0 and fin[1] == 0.0 and not xs[1].any(), (its, nup, fin)
    for j in (0, 2, 3):
        assert nup[j] >= 1
        _assert_same(("maxits", j), (xs[j], its[j], fin[j], nup[j]), _single_xx(ctx, bz[j], MS[j], 0.0, 7, par_even))
    ctx.close()


@pytest.mark.parametrize("kind,naik", LINKS)
@pytest.mark.parametrize("lat", LATS)
def test_solve_batch_sloppy_equals_single(oracle, lat, kind, naik):
    """the full solve: reconstruct-right for one-parity sources (either parity), reconstruct-left otherwise, against
    qexhip_stag_solve_sloppy (Staggered.solve with sp.sloppySolve)"""
    import qex_amd as q

    o = oracle
    lo, rf, ctx, s, fat, lng = _setup(o, lat, kind, naik)
    bs = [o.vector_gaussian(lo, rf) for _ in MS]
    bs[0][lo.vol // 2:] = 0                                  # phi.odd := 0: ReconR, even inner solve
    bs[1][:lo.vol // 2] = 0                                  # odd-only source: ReconR, odd inner solve
    r2 = [1e-12, 1e-16, 1e-20, 1e-14]                        # (2, 3: both parities, ReconL)
    ref = []
    for j in range(4):
        sp = q.SolverParams(r2req=r2[j], maxits=10000, verbosity=0, sloppySolve=q.SloppySingle)
        x1 = np.zeros_like(bs[j])
        s.solve(x1, bs[j], MS[j], sp)
        ref.append((x1, sp.iterations, sp.r2, sp.reliableUpdates))
    for n in (4, 3, 2, 1):
        sps = [q.SolverParams(r2req=r2[j], maxits=10000, verbosity=0) for j in range(n)]
        xs = [np.zeros_like(b) for b in bs[:n]]
        its = s.solve_batch(xs, bs[:n], MS[:n], sps, sloppy=1)
        print(f"solve_batch sloppy {lat} {kind} naik={naik} n={n}: its {its} updates {[sp.reliableUpdates for sp in sps]} "
              f"r2 {[sp.r2 for sp in sps]}")
        for j in range(n):
            assert its[j] == sps[j].iterations and sps[j].calls == 1
            _assert_same((n, j), (xs[j], its[j], sps[j].r2, sps[j].reliableUpdates), ref[j])
            assert sps[j].reliableUpdates >= 1
            r = np.zeros_like(xs[j])
            s.D(r, xs[j], MS[j])
            assert ((r - bs[j]) ** 2).sum() / (bs[j] ** 2).sum() <= r2[j]
    ctx.close()


# ---- 2. the true residual, and the iteration count against the fp64 batch --------------------------------------------
@pytest.mark.parametrize("kind,naik", LINKS)
@pytest.mark.parametrize("lat", LATS)
def test_true_residual_and_iterations(oracle, lat, kind, naik):
    o = oracle
    lo, rf, ctx, s, fat, lng = _setup(o, lat, kind, naik)
    bs = [o.vector_gaussian(lo, rf) for _ in MS]
    for par_even in (True, False):
        sl = _half(lo, par_even)
        x64 = [np.zeros_like(b) for b in bs]
        its64, _ = s.solveXX_batch(x64, bs, MS, R2, 5000, par_even)
        xs = [np.zeros_like(b) for b in bs]
        its, fin, nup = s.solveXX_batch(xs, bs, MS, R2, 5000, par_even, sloppy=1)
        for j in range(4):
            b2 = float(np.sum(bs[j][sl] ** 2))
            r2 = _true_r2(ctx, xs[j], bs[j], MS[j], par_even)
            print(f"  {lat} {kind} naik={naik} par_even={par_even} system {j}: its {its[j]} vs fp64 batch {its64[j]} "
                  f"(ratio {its[j] / its64[j]:.3f}), updates {nup[j]}, true r2/b2 {r2 / b2:.3e} (reported {fin[j]:.3e})")
            assert r2 <= R2[j] * b2
            assert abs(fin[j] - r2 / b2) <= 1e-6 * r2 / b2 + 1e-300
            assert its[j] <= 1.5 * its64[j]
    ctx.close()


# ---- 3. sloppy = 0 is the fp64 batch; SloppyHalf runs single ---------------------------------------------------------
def test_sloppy_zero_is_the_fp64_batch_and_half_is_single(oracle):
    import qex_amd as q

    o = oracle
    lo, rf, ctx, s, fat, lng = _setup(o, [8, 8, 8, 8], "random")
    bs = [o.vector_gaussian(lo, rf) for _ in MS]
    for maxits in (5000, 9):
        xa, xb = [np.zeros_like(b) for b in bs], [np.zeros_like(b) for b in bs]
        ia, fa = s.solveXX_batch(xa, bs, MS, R2, maxits, True)
        ib, fb, ub = s.solveXX_batch(xb, bs, MS, R2, maxits, True, sloppy=0)
        assert ia == ib and fa == fb and ub == [0] * 4 and all(np.array_equal(a, b) for a, b in zip(xa, xb))
        spa = [q.SolverParams(r2req=r, maxits=maxits, verbosity=0) for r in R2]
        spb = [q.SolverParams(r2req=r, maxits=maxits, verbosity=0, sloppySolve=q.SloppySingle) for r in R2]   # the keyword overrides
        ya, yb = [np.zeros_like(b) for b in bs], [np.zeros_like(b) for b in bs]
        ja = s.solve_batch(ya, bs, MS, spa)
        jb = s.solve_batch(yb, bs, MS, spb, sloppy=0)
        assert ja == jb and [p.r2 for p in spa] == [p.r2 for p in spb] and all(p.reliableUpdates == 0 for p in spb)
        assert all(np.array_equal(a, b) for a, b in zip(ya, yb))
    x1, x2 = [np.zeros_like(b) for b in bs], [np.zeros_like(b) for b in bs]
    r1 = s.solveXX_batch(x1, bs, MS, R2, 5000, False, sloppy=q.SloppySingle)
    r2 = s.solveXX_batch(x2, bs, MS, R2, 5000, False, sloppy=q.SloppyHalf)
    assert r1 == r2 and all(np.array_equal(a, b) for a, b in zip(x1, x2))
    # resident fields: dev_solve_batch(sloppy=0) is dev_solve_batch, (sloppy=1) the host entry's bits
    fb_, fx_ = [ctx.field_new(b) for b in bs], [ctx.field_new() for _ in bs]
    i0, f0 = ctx.dev_solve_batch(fx_, fb_, MS, R2, 5000)
    d0 = [ctx.field_download(f) for f in fx_]
    i1, f1, u1 = ctx.dev_solve_batch(fx_, fb_, MS, R2, 5000, sloppy=0)
    assert (i0, f0) == (i1, f1) and u1 == [0] * 4 and all(np.array_equal(a, ctx.field_download(f)) for a, f in zip(d0, fx_))
    i2, f2, u2 = ctx.dev_solve_batch(fx_, fb_, MS, R2, 5000, sloppy=1)
    sps = [q.SolverParams(r2req=r, maxits=5000, verbosity=0) for r in R2]
    ys = [np.zeros_like(b) for b in bs]
    s.solve_batch(ys, bs, MS, sps, sloppy=1)
    assert i2 == [p.iterations for p in sps] and f2 == [p.r2 for p in sps] and u2 == [p.reliableUpdates for p in sps]
    assert all(np.array_equal(y, ctx.field_download(f)) for y, f in zip(ys, fx_))
    ctx.close()


# ---- 4. systems finish independently ---------------------------------------------------------------------------------
@pytest.mark.parametrize("par_even", [True, False])
def test_systems_finish_independently(oracle, par_even):
    o = oracle
    lo, rf, ctx, s, fat, lng = _setup(o, [8, 8, 8, 8], "warm")
    bs = [o.vector_gaussian(lo, rf) for _ in range(4)]
    ms, r2 = [0.1, 0.1, 0.3, 0.05], [1e-8, 1e-20, 1e-8, 1e-20]
    xs = [np.zeros_like(b) for b in bs]
    its, fin, nup = s.solveXX_batch(xs, bs, ms, r2, 5000, par_even, sloppy=1)
    print(f"independent stops par_even={par_even}: its {its} updates {nup} r2/b2 {fin}")
    assert its[0] < its[1] and its[2] < its[3]
    for j in range(4):
        # the early systems are what they were when they stopped (their own solve's bits), the late ones their own solve's too
        _assert_same(j, (xs[j], its[j], fin[j], nup[j]), _single_xx(ctx, bs[j], ms[j], r2[j], 5000, par_even))
        assert fin[j] <= r2[j]
    ctx.close()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------
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

    o = oracle
    L = lib()
    # a context with ghost zones in t (what each rank of a t-sharded job holds): refused, and the text says why
    lo, rf, ctx, s, fat, lng = _setup(o, [8, 8, 8, 8], "random", halo=True)
    bs = [o.vector_gaussian(lo, rf) for _ in range(5)]
    xs = [np.full_like(b, 3.0) for b in bs]
    ids = ([ctx.field_new() for _ in range(5)], [ctx.field_new(b) for b in bs])
    for which in ("xx", "full", "dev"):
        rc = _raw(L, ctx, which, 2, xs[:2], bs[:2], [0.1, 0.2], [1e-10, 1e-10], 100, 1, (ids[0][:2], ids[1][:2]))
        msg = L.qexhip_last_error().decode()
        assert rc == -1 and "shard" in msg, (which, rc, msg)
        assert all((x == 3.0).all() for x in xs)                 # nothing was solved
    # sloppy = 0 there is the fp64 batch, which runs on such a context
    assert _raw(L, ctx, "xx", 2, xs[:2], bs[:2], [0.1, 0.2], [1e-10, 1e-10], 100, 0) == 0
    ctx.close()
    lo, rf, ctx, s, fat, lng = _setup(o, [8, 8, 8, 8], "random")
    ids = ([ctx.field_new() for _ in range(5)], [ctx.field_new(b) for b in bs])
    for which in ("xx", "full", "dev"):
        xs = [np.full_like(b, 3.0) for b in bs]
        two = (ids[0][:2], ids[1][:2])
        assert _raw(L, ctx, which, 2, xs[:2], bs[:2], [0.1, 0.0], [1e-10, 1e-10], 100, 1, two) == -1        # mass 0
        assert b"mass" in L.qexhip_last_error()
        for bad in (3, -1):
            assert _raw(L, ctx, which, 2, xs[:2], bs[:2], [0.1, 0.2], [1e-10, 1e-10], 100, bad, two) == -1   # sloppy outside 0..2
            assert b"sloppy" in L.qexhip_last_error()
        for n in (5, 0):
            assert _raw(L, ctx, which, n, xs, bs, [0.1] * 5, [1e-10] * 5, 100, 1, ids) == -1                 # n outside 1..4
        assert all((x == 3.0).all() for x in xs)
        assert _raw(L, ctx, which, 2, xs[:2], bs[:2], [0.1, 0.2], [1e-10, 1e-10], 100, 1, two) == 0          # and the good call runs
    # aliased resident fields are refused as by dev_solve_batch
    assert _raw(L, ctx, "dev", 2, [], [], [0.1, 0.2], [1e-10] * 2, 100, 1, ([ids[0][0], ids[0][0]], ids[1][:2])) == -1
    ctx.close()


# ---- 6. the fp32 links follow a change of the operator ---------------------------------------------------------------
def test_stale_links_are_rebuilt_for_the_batch(oracle):
    import qex_amd as q

    o = oracle
    lo, rf, ctx, s, fatA, lng = _setup(o, [8, 8, 8, 8], "random")
    bs = [o.vector_gaussian(lo, rf) for _ in range(3)]
    ms, r2 = [0.1, 0.2, 0.05], [1e-14] * 3
    xa = [np.zeros_like(b) for b in bs]
    ita, _, _ = s.solveXX_batch(xa, bs, ms, r2, 5000, True, sloppy=1)          # the fp32 copy of A's links now exists
    rfb = o.RngField(lo, o.RNG_MILC6, 12345)
    fatB = o.gauge_random(lo, rfb)
    o.rephase(lo, fatB)
    sB = q.newStag(ctx, fatB)
    xb = [np.zeros_like(b) for b in bs]
    itb, finb, nupb = sB.solveXX_batch(xb, bs, ms, r2, 5000, True, sloppy=1)   # FIRST sloppy call on B: the batch itself must rebuild
    x64 = [np.zeros_like(b) for b in bs]
    it64, _ = sB.solveXX_batch(x64, bs, ms, r2, 5000, True)
    h = lo.vol // 2
    for j in range(3):
        _assert_same(j, (xb[j], itb[j], finb[j], nupb[j]), _single_xx(ctx, bs[j], ms[j], r2[j], 5000, True))
        xerr = np.linalg.norm(xb[j][:h] - x64[j][:h]) / np.linalg.norm(x64[j][:h])
        assert xerr <= 1e-5 and itb[j] <= 1.5 * it64[j], (j, xerr, itb[j], it64[j])     # (stale fp32 links stall the fp32 iteration)
        assert not np.array_equal(xa[j], xb[j])
        b2 = float(np.sum(bs[j][:h] ** 2))
        assert _true_r2(ctx, xb[j], bs[j], ms[j], True) <= r2[j] * b2
    # an MD link update on the device, then the operator rebuilt from the updated links
    p = o.gauge_random_tah(lo, rfb)
    gC = fatA.copy()
    q.gaugeUpdate(ctx, gC, p, 0.05)
    sC = q.newStag(ctx, gC)
    xc = [np.zeros_like(b) for b in bs]
    itc, finc, nupc = sC.solveXX_batch(xc, bs, ms, r2, 5000, True, sloppy=1)
    it64, _ = sC.solveXX_batch(x64, bs, ms, r2, 5000, True)
    for j in range(3):
        _assert_same(("md", j), (xc[j], itc[j], finc[j], nupc[j]), _single_xx(ctx, bs[j], ms[j], r2[j], 5000, True))
        assert itc[j] <= 1.5 * it64[j]
    ctx.close()


# ---- 7. meson tables --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lat", [[8, 8, 8, 8], [4, 6, 10, 6]])
def test_meson_tables_sloppy_against_fp64(oracle, lat):
    import qex_amd as q

    o = oracle
    lo, rf, ctx, s, fat, lng = _setup(o, lat, "random")
    qlo = q.Layout(lat)
    cl0, cs0, st0 = q.localMesonTables(s, qlo, 0.1, 2, 1e-20, maxits=20000)
    cl1, cs1, st1 = q.localMesonTables(s, qlo, 0.1, 2, 1e-20, maxits=20000, sloppy=1)
    assert st0["updates"] == [[0] * 4] * 3
    assert all(min(u) >= 1 for u in st1["updates"]) and all(max(i) < 20000 for i in st1["iterations"])
    for k, (a, b) in enumerate(zip([cl1] + cs1, [cl0] + cs0)):
        rel = float(np.abs(a - b).max() / np.abs(b).max())
        print(f"meson table {k} {lat}: sloppy vs fp64 max rel diff {rel:.2e}; its {st1['iterations']} vs {st0['iterations']}, "
              f"updates {st1['updates']}")
        assert rel < 1e-8, (k, rel)
    ctx.close()


def test_example_with_sloppy_batches():
    ex = os.path.join(ROOT, "examples", "stag_mesons.py")
    run = lambda extra: subprocess.run([sys.executable, ex, "-lat", "8", "8", "8", "8"] + extra, stdout=subprocess.PIPE,   # noqa: E731
                                       stderr=subprocess.PIPE, text=True, timeout=300, cwd=ROOT)
    p1 = run(["-sloppy", "1"])
    assert p1.returncode == 0, p1.stderr[-4000:]
    assert "mixed-precision batches: fp32 link format" in p1.stdout and "reliable updates per colour" in p1.stdout
    p0 = run([])
    assert p0.returncode == 0, p0.stderr[-4000:]
    assert "reliable updates" not in p0.stdout and "mixed-precision" not in p0.stdout

    def tables(out):
        return np.array([float(ln.split()[1]) for ln in out.splitlines() if len(ln.split()) == 2 and ln.split()[0].isdigit()])

    a, b = tables(p1.stdout), tables(p0.stdout)
    assert a.shape == b.shape == (4 * 8 * 8,)
    # both runs stop at |r| <= 1e-8 |b| (the example's default r2req = 1e-16): each propagator is off by at most cond(D) 1e-8 with
    # cond(D) <= (m + 4) / m = 41 at m = 0.1, the two runs differ by twice that, and the tables are quadratic in the propagators:
    # 2 * 2 * 41e-8 = 1.64e-6
    assert np.abs(a - b).max() <= 2e-6 * np.abs(b).max()
    # more than one rank is refused with a clear message before anything is set up
    p2 = subprocess.run([sys.executable, ex, "-sloppy", "1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120,
                        cwd=ROOT, env=dict(os.environ, WORLD_SIZE="2", RANK="0"))
    assert p2.returncode != 0 and "single rank" in p2.stderr


# ---- 8. the measurement workload ---------------------------------------------------------------------------------------
def test_sloppy_batch_32_4_workload(oracle):
    """four point-source-like systems (the point source of fpvaMeas.nim and its three symmetric shifts) on 32^4 g.random links"""
    import time
    import qex_amd as q

    o = oracle
    lat = [32, 32, 32, 32]
    lo, rf, ctx, s, fat, lng = _setup(o, lat, "random")
    assert ctx.links_info_f32()[0] == 1
    qlo = q.Layout(lat)
    src = q.pointSource(qlo, [0, 0, 0, 2], 0)
    bs = [src]
    for mu in range(3):
        h = np.zeros_like(src)
        s.symShift(h, src, mu)
        bs.append(h)
    m, r2req = 0.1, 1e-14
    sp1 = q.SolverParams(r2req=r2req, maxits=10000, verbosity=0, sloppySolve=q.SloppySingle)
    x1 = np.zeros_like(bs[1])
    s.solve(x1, bs[1], m, sp1)                       # one single solve (also the warm-up: the fp32 links are built here)
    sps = [q.SolverParams(r2req=r2req, maxits=10000, verbosity=0) for _ in bs]
    xs = [np.zeros_like(b) for b in bs]
    t0 = time.perf_counter()
    its = s.solve_batch(xs, bs, [m] * 4, sps, sloppy=1)
    t32 = time.perf_counter() - t0
    sp64 = [q.SolverParams(r2req=r2req, maxits=10000, verbosity=0) for _ in bs]
    x64 = [np.zeros_like(b) for b in bs]
    t0 = time.perf_counter()
    its64 = s.solve_batch(x64, bs, [m] * 4, sp64)
    t64 = time.perf_counter() - t0
    print(f"32^4 solve_batch of 4 point-like sources r2req {r2req:g}: sloppy its {its} updates {[p.reliableUpdates for p in sps]} "
          f"{t32 * 1e3:.1f} ms (host arrays); fp64 batch its {its64} {t64 * 1e3:.1f} ms")
    _assert_same("32^4 system 1", (xs[1], its[1], sps[1].r2, sps[1].reliableUpdates), (x1, sp1.iterations, sp1.r2, sp1.reliableUpdates))
    for j in range(4):
        r = np.zeros_like(xs[j])
        s.D(r, xs[j], m)
        rel = float(((r - bs[j]) ** 2).sum() / (bs[j] ** 2).sum())
        print(f"  system {j}: |b - D x|^2/|b|^2 {rel:.3e} (reported {sps[j].r2:.3e})")
        assert rel <= r2req and sps[j].r2 <= r2req and sps[j].reliableUpdates >= 1
        assert its[j] <= 1.5 * its64[j]
    ctx.close()
