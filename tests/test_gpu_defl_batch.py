"""Deflated lock-step batches on both parities from the even basis: the two multi-right-hand-side block kernels against the single
ones (bit for bit) and numpy, the deflated batch against the single deflated solve, the odd-parity projection
    x0.odd = D_oe V diag(1 / (4 lambda (lambda + m^2))) V^+ (-D_eo b.odd)
against a numpy CG on the dense odd-odd operator, the full solves of time / even-odd diluted sources, and the two measurement
drivers with deflate=.  tests/eig_ref.py builds the inputs and the dense even-even reference once per lattice; the dense D_oe is built
here the same way.  Observed values are printed (pytest -s)."""
import ctypes as C
import functools

import numpy as np
import pytest

import eig_ref as R

pytestmark = pytest.mark.gpu

# the options of test_gpu_eig.py that converge nev = 16 / nvecs = 40 to abserr = 1e-9 on these inputs
CHEB = dict(cheb_degree=8, cheb_lo=0.3, cheb_hi=0.0, max_restarts=40)


def ovec(field, vh):
    """odd half of a host field (vol, 3, 2) as a complex vector of 3 vh entries"""
    e = np.asarray(field)[vh:]
    return (e[..., 0] + 1j * e[..., 1]).reshape(-1)


def relerr(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


# ---------------------------------------------------------------- the two kernels
HOOK_LAT = (4, 6, 4, 6)


@pytest.fixture(scope="module")
def hook():
    """a context on 4.6.4.6 (288 even sites = 4.5 tiles) with a 40-vector basis of Gaussian vectors and four Gaussian w_k"""
    import qex_amd as q

    vol = int(np.prod(HOOK_LAT))
    vh = vol // 2
    rng = np.random.default_rng(R.SEED)
    vecs = [rng.standard_normal((vol, 3, 2)) for _ in range(22)]
    ws = [rng.standard_normal((vol, 3, 2)) for _ in range(4)]
    ctx = q.Context(list(HOOK_LAT), device=0)
    basis = q.EigBasis(ctx, 40)
    for i, v in enumerate(vecs):
        basis.set_vector(i, v)
    V = np.stack([R.cvec(v, vh) for v in vecs], axis=1)
    yield dict(ctx=ctx, basis=basis, ws=ws, V=V, vh=vh, vol=vol)
    basis.free()
    ctx.close()


def _dot_checks(ctx, B, V, ws, vh, i0, n, nrhs):
    ids = [ctx.field_new(w) for w in ws[:nrhs]]
    try:
        m1 = B.block_dot_multi(i0, n, ids)
        m2 = B.block_dot_multi(i0, n, ids)
        assert m1.shape == (nrhs, n)
        assert np.array_equal(m1, m2), "the multi-right-hand-side block dot is not bit-identical run to run"
        worst = 0.0
        for k in range(nrhs):
            single = B.block_dot(i0, n, ids[k])
            assert np.array_equal(m1[k], single), (k, "row differs from block_dot of that w alone")
            ref = V[:, i0:i0 + n].conj().T @ R.cvec(ws[k], vh)
            worst = max(worst, (np.abs(m1[k] - ref) / np.abs(ref)).max())
        return worst
    finally:
        for fid in ids:
            ctx.field_free(fid)


@pytest.mark.parametrize("i0", [0, 5])
@pytest.mark.parametrize("n", [1, 3, 8, 17])
@pytest.mark.parametrize("nrhs", [1, 2, 3, 4])
def test_block_dot_multi_is_block_dot_bit_for_bit(hook, nrhs, n, i0):
    worst = _dot_checks(hook["ctx"], hook["basis"], hook["V"], hook["ws"], hook["vh"], i0, n, nrhs)
    print("block dot multi nrhs = %d n = %d i0 = %d: max relative deviation from numpy %.2e" % (nrhs, n, i0, worst))
    assert worst <= 1e-13


def test_block_kernels_across_the_chunk_boundary(hook):
    """130 vectors, n = 130, nrhs = 4: two launches of the dot (128 + 2 vectors)"""
    import qex_amd as q

    ctx, ws, vh, vol = hook["ctx"], hook["ws"], hook["vh"], hook["vol"]
    rng = np.random.default_rng(130)
    vecs = [rng.standard_normal((vol, 3, 2)) for _ in range(130)]
    B = q.EigBasis(ctx, 130)
    try:
        for i, v in enumerate(vecs):
            B.set_vector(i, v)
        V = np.stack([R.cvec(v, vh) for v in vecs], axis=1)
        worst = _dot_checks(ctx, B, V, ws, vh, 0, 130, 4)
        print("block dot multi across the chunk boundary: max relative deviation from numpy %.2e" % worst)
        assert worst <= 1e-13
        _axpy_checks(ctx, B, ws, vh, 0, 130, 4)
    finally:
        B.free()


def _axpy_checks(ctx, B, ws, vh, i0, n, nrhs):
    coef = np.stack([(np.arange(1, n + 1) * 0.37 - 1.0 - 0.2 * k) + 1j * (0.5 + 0.3 * k - 0.11 * np.arange(n)) for k in range(nrhs)])
    ids = [ctx.field_new(w) for w in ws[:nrhs]]
    one = ctx.field_new()
    try:
        B.block_axpy_multi(i0, coef, ids)
        for k in range(nrhs):
            ctx.field_upload(one, ws[k])
            B.block_axpy(i0, coef[k], one)
            got, want = ctx.field_download(ids[k]), ctx.field_download(one)
            assert np.array_equal(got, want), (k, "differs from block_axpy with that system's coefficients")
            assert np.array_equal(got[vh:], ws[k][vh:]), "the odd half was touched"
            assert not np.array_equal(got[:vh], ws[k][:vh])
    finally:
        for fid in ids + [one]:
            ctx.field_free(fid)


@pytest.mark.parametrize("i0", [0, 5])
@pytest.mark.parametrize("n", [1, 3, 8, 17])
@pytest.mark.parametrize("nrhs", [1, 2, 3, 4])
def test_block_axpy_multi_is_block_axpy_bit_for_bit(hook, nrhs, n, i0):
    _axpy_checks(hook["ctx"], hook["basis"], hook["ws"], hook["vh"], i0, n, nrhs)


def test_all_ones_count_exactly(hook):
    """all-ones vectors and w_k = (k + 1) on every site: <v_j, w_k> = 3 x 288 x (k + 1) exactly -- the 32 spare lanes of the ragged
    last tile add nothing for any right-hand side"""
    import qex_amd as q

    ctx, vh, vol = hook["ctx"], hook["vh"], hook["vol"]
    ones = np.zeros((vol, 3, 2))
    ones[..., 0] = 1.0
    B = q.EigBasis(ctx, 3)
    ids = [ctx.field_new(ones * (k + 1)) for k in range(4)]
    try:
        for i in range(3):
            B.set_vector(i, ones)
        c = B.block_dot_multi(0, 3, ids)
        print("all-ones block dot multi:", c.real.tolist())
        assert 3 * vh == 864
        for k in range(4):
            assert np.all(c[k] == 864.0 * (k + 1))
    finally:
        for fid in ids:
            ctx.field_free(fid)
        B.free()


def test_multi_hooks_refuse_bad_arguments(hook):
    import qex_amd as q

    ctx, B = hook["ctx"], hook["basis"]
    ids = [ctx.field_new(w) for w in hook["ws"]]
    before = [ctx.field_download(f) for f in ids]
    out = np.zeros(4 * 41 * 2 + 16)
    L = q.lib()
    i4 = (C.c_int * 5)(*(ids + [ids[0]]))
    rep = (C.c_int * 4)(ids[0], ids[1], ids[0], ids[2])
    assert L.qexhip_eig_block_dot_multi(ctx._h, B.id, 30, 11, 2, i4, out.ctypes.data) == -1
    assert L.qexhip_eig_block_dot_multi(ctx._h, B.id, -1, 2, 2, i4, out.ctypes.data) == -1
    assert L.qexhip_eig_block_dot_multi(ctx._h, B.id, 0, 0, 2, i4, out.ctypes.data) == -1
    assert L.qexhip_eig_block_dot_multi(ctx._h, B.id, 0, 4, 0, i4, out.ctypes.data) == -1
    assert L.qexhip_eig_block_dot_multi(ctx._h, B.id, 0, 4, 5, i4, out.ctypes.data) == -1
    assert L.qexhip_eig_block_axpy_multi(ctx._h, B.id, 0, 41, 2, out.ctypes.data, i4) == -1
    assert L.qexhip_eig_block_axpy_multi(ctx._h, B.id, 38, 3, 2, out.ctypes.data, i4) == -1
    assert L.qexhip_eig_block_axpy_multi(ctx._h, B.id, 0, 4, 0, out.ctypes.data, i4) == -1
    assert L.qexhip_eig_block_axpy_multi(ctx._h, B.id, 0, 4, 5, out.ctypes.data, i4) == -1
    assert L.qexhip_eig_block_axpy_multi(ctx._h, B.id, 0, 4, 4, out.ctypes.data, rep) == -1
    assert L.qexhip_eig_block_dot_multi(ctx._h, B.id, 0, 4, 4, rep, out.ctypes.data) == 0      # a repeated w is fine
    for f, b in zip(ids, before):
        assert np.array_equal(ctx.field_download(f), b), "a refused call wrote to a field"
        ctx.field_free(f)


# ---------------------------------------------------------------- solves
DLAT, MASS, R2REQ = (4, 4, 8, 8), 0.01, 1e-20


@functools.lru_cache(maxsize=None)
def dense_odd():
    """(D_oe as a complex (3 Vh, 3 Vh) matrix from oracle.D(m = 0) on the even unit vectors, H_o = D_oe D_oe^+)"""
    from oracle import oracle as o

    lo, g, _, _ = R.inputs(DLAT)
    H, _, _ = R.dense(DLAT)
    vh = lo.vol // 2
    n = 3 * vh
    Doe = np.zeros((n, n), dtype=np.complex128)
    x = lo.new_vector()
    for k in range(n):
        x[k // 3, k % 3, 0] = 1.0
        Doe[:, k] = ovec(o.D(lo, g, None, x, 0.0), vh)
        x[k // 3, k % 3, 0] = 0.0
    dev = np.abs(H - Doe.conj().T @ Doe).max()
    print("|H - D_oe^+ D_oe|_max = %.2e" % dev)
    assert dev < 1e-13
    return Doe, Doe @ Doe.conj().T


@pytest.fixture(scope="module")
def sol():
    import qex_amd as q
    from oracle import oracle as o

    lo, g, _, b = R.inputs(DLAT)
    rf = o.RngField(lo, o.RNG_MILC6, 4242)
    bs = [np.ascontiguousarray(b)] + [o.vector_gaussian(lo, rf) for _ in range(3)]
    ctx = q.Context(list(DLAT), device=0)
    s = q.newStag(ctx, g)
    B = s.eigs(16, nvecs=40, relerr=0.0, abserr=1e-9, **CHEB)
    assert B.nconv == 16
    bid = [ctx.field_new(v) for v in bs]
    xid = [ctx.field_new() for _ in bs]
    yield dict(ctx=ctx, s=s, B=B, bs=bs, bid=bid, xid=xid, lo=lo, g=g, vh=lo.vol // 2, q=q)
    B.free()
    ctx.close()


def test_even_batch_against_the_single_deflated_solve(sol):
    ctx, B, bid, xid = sol["ctx"], sol["B"], sol["bid"], sol["xid"]
    ms = [0.01, 0.01, 0.02, 0.05]
    its, r2, nup = ctx.dev_solve_xx_batch_deflated(B, 16, xid, bid, ms, R2REQ, 5000)
    xs = [ctx.field_download(f) for f in xid]
    one = ctx.field_new()
    for k in range(4):
        i1, r1 = ctx.dev_solve_xx_deflated(B, 16, one, bid[k], ms[k], R2REQ, 5000)
        x1 = ctx.field_download(one)
        eq = np.array_equal(xs[k], x1)
        print("system %d (m = %g): batch %d its r2/b2 %.4e, single %d its r2/b2 %.4e, x %s" %
              (k, ms[k], its[k], r2[k], i1, r1, "bit-identical" if eq else "relerr %.2e" % relerr(xs[k], x1)))
        assert eq or relerr(xs[k], x1) < 1e-13
        assert abs(its[k] - i1) <= 1
        assert r2[k] <= R2REQ * (1 + 1e-3)
    assert nup == [0, 0, 0, 0]
    ctx.field_free(one)


def test_odd_batch_from_the_even_basis(sol):
    from oracle import oracle as o

    ctx, s, B, vh, lo, g = sol["ctx"], sol["s"], sol["B"], sol["vh"], sol["lo"], sol["g"]
    Doe, Ho = dense_odd()
    _, w, v = R.dense(DLAT)
    A = 4.0 * (MASS * MASS * np.eye(Ho.shape[0]) + Ho)
    U = Doe @ v[:, :16] / np.sqrt(w[:16])                       # the odd pairs of the 16 lowest even pairs
    bo = []
    for b in sol["bs"]:
        b = b.copy()
        b[:vh] = 0.0
        bo.append(b)
    ids = [ctx.field_new(b) for b in bo]
    its, r2, _ = ctx.dev_solve_xx_batch_deflated(B, 16, sol["xid"], ids, [MASS] * 4, R2REQ, 5000, par_even=False)
    xs0 = [np.zeros_like(b) for b in bo]
    its0, _ = s.solveXX_batch(xs0, bo, [MASS] * 4, R2REQ, 5000, parEven=False)
    for k in range(4):
        xf = ctx.field_download(sol["xid"][k])
        bc = ovec(bo[k], vh)
        b2 = np.vdot(bc, bc).real
        rr = bc - ovec(o.stagD2xx(lo, g, None, xf, MASS * MASS, False), vh)
        r2o = np.vdot(rr, rr).real / b2
        xsol = np.linalg.solve(A, bc)
        xerr = relerr(ovec(xf, vh), xsol)
        _, it_plain = R.cg(A, bc, np.zeros_like(bc), R2REQ)
        _, it_defl = R.cg(A, bc, U @ ((U.conj().T @ bc) / (4.0 * (w[:16] + MASS * MASS))), R2REQ)
        print("odd system %d: deflated %d its (numpy %d), undeflated %d (numpy %d), ratio %.3f; r2/b2 %.6e (oracle %.6e); |x - solve| %.2e"
              % (k, its[k], it_defl, its0[k], it_plain, its[k] / its0[k], r2[k], r2o, xerr))
        assert not xf[:vh].any(), "the even half of an odd solution is not zero"
        assert r2[k] <= R2REQ * (1 + 1e-3)
        assert abs(r2o / r2[k] - 1) <= 1e-6
        assert xerr <= 1e-9
        assert its[k] <= 0.75 * its0[k]
        assert abs(its[k] - it_defl) <= max(2, 0.02 * it_defl)
    for f in ids:
        ctx.field_free(f)


@pytest.mark.parametrize("par_even", [True, False])
def test_no_modes_is_the_undeflated_batch(sol, par_even):
    ctx, s, B, bs = sol["ctx"], sol["s"], sol["B"], sol["bs"]
    ms = [0.01, 0.01, 0.02, 0.05]
    x0 = [np.zeros_like(b) for b in bs]
    x1 = [np.zeros_like(b) for b in bs]
    its0, r0 = s.solveXX_batch(x0, bs, ms, R2REQ, 5000, parEven=par_even)
    its1, r1 = s.solveXX_batch(x1, bs, ms, R2REQ, 5000, parEven=par_even, deflate=B, nev=0)
    assert its1 == its0 and r1 == r0
    for a, b in zip(x0, x1):
        assert np.array_equal(a, b)
    its2, r2, _ = ctx.dev_solve_xx_batch_deflated(B, 0, sol["xid"], sol["bid"], ms, R2REQ, 5000, par_even=par_even)
    assert its2 == its0 and r2 == r0
    for a, f in zip(x0, sol["xid"]):
        assert np.array_equal(a, ctx.field_download(f))


@pytest.mark.parametrize("par_even", [True, False])
def test_sloppy_deflated_batch(sol, par_even):
    s, B, bs = sol["s"], sol["B"], sol["bs"]
    x0 = [np.zeros_like(b) for b in bs]
    x1 = [np.zeros_like(b) for b in bs]
    its0, r0, nup0 = s.solveXX_batch(x0, bs, [MASS] * 4, R2REQ, 20000, parEven=par_even, sloppy=1)
    its1, r1, nup1 = s.solveXX_batch(x1, bs, [MASS] * 4, R2REQ, 20000, parEven=par_even, sloppy=1, deflate=B)
    print("sloppy %s batch: undeflated %s its (%s updates), deflated %s its (%s updates), r2/b2 %s" %
          ("even" if par_even else "odd", its0, nup0, its1, nup1, ["%.3e" % v for v in r1]))
    for k in range(4):
        assert r1[k] <= R2REQ * (1 + 1e-3)
        assert its1[k] <= 0.75 * its0[k]


def _z4_patterns(sol):
    """four time / even-odd diluted Z4 sources: t in {0, 3} x both parities, as resident fields"""
    q, ctx = sol["q"], sol["ctx"]
    eta = ctx.field_new()
    q.RngField(list(DLAT), q.RngMilc6, R.SEED).dev_z4_vector(ctx, eta)
    src = [ctx.field_new() for _ in range(4)]
    pats = [(0, 0), (0, 1), (3, 0), (3, 1)]                  # (t, parity pattern)
    ctx.dev_dilute(src, eta, 0, [p for _, p in pats], [t for t, _ in pats], 1.0)
    ctx.field_free(eta)
    return src, pats


def test_full_solves_of_diluted_sources(sol):
    from oracle import oracle as o

    ctx, B, lo, g, vh = sol["ctx"], sol["B"], sol["lo"], sol["g"], sol["vh"]
    src, pats = _z4_patterns(sol)
    its0, r0 = ctx.dev_solve_batch(sol["xid"], src, [MASS] * 4, R2REQ, 20000)
    its1, r1 = ctx.dev_solve_batch(sol["xid"], src, [MASS] * 4, R2REQ, 20000, deflate=B)
    for k, (t, p) in enumerate(pats):
        b, x = ctx.field_download(src[k]), ctx.field_download(sol["xid"][k])
        assert b[vh:].any() != b[:vh].any()                  # one parity only
        r = b - o.D(lo, g, None, x, MASS)
        r2o = np.vdot(r, r).real / np.vdot(b, b).real
        print("t = %d %s source: %d its undeflated, %d deflated (ratio %.3f); r2 %.4e, with the oracle's D %.4e" %
              (t, "odd" if b[vh:].any() else "even", its0[k], its1[k], its1[k] / its0[k], r1[k], r2o))
        assert r1[k] <= R2REQ and r2o <= R2REQ * (1 + 1e-3)
        assert its1[k] <= 0.75 * its0[k]
    for f in src:
        ctx.field_free(f)


# Both runs stop every full solve at |D phi - b| <= 1e-10 |b| (r2req = 1e-20), so each phi is within |r| / sigma_min(D + m) of the exact
# one, sigma_min^2 = lambda_0 + m^2 >= 0.0157 on these links (test_gpu_eig.py): |d phi| <= 8e-10 |b| per run, 1.6e-9 |b| between the two.
# |phi| >= |b| / |D + m| with |D + m|^2 = lambda_max + m^2 <= 5.3, so |d phi| / |phi| <= 3.7e-9; the trace and the meson tables are
# bilinear in phi: 7.4e-9 of their scale.
TOL_DEFL = 1e-8


def test_scalar_trace_and_meson_tables_with_deflation(sol):
    q, s, B, lo = sol["q"], sol["s"], sol["B"], sol["lo"]
    qlo = q.Layout(list(DLAT))
    run = lambda **kw: q.scalarTrace(s, qlo, q.RngField(list(DLAT), q.RngMilc6, R.SEED), MASS, R2REQ, out=None, **kw)
    tr0, est0, st0 = run()
    tr1, est1, st1 = run(deflate=B)
    scale = np.abs(tr0[0]).max()
    dt, de = np.abs(tr1[0] - tr0[0]).max() / scale, np.abs(est1[0] - est0[0]).max() / scale
    n0, n1 = sum(st0["iterations"][0]), sum(st1["iterations"][0])
    print("scalarTrace EO: deviation of the trace %.3e, of est %.3e (of max|trace| = %.4g); iterations %d -> %d (ratio %.3f)" %
          (dt, de, scale, n0, n1, n1 / n0))
    assert len(st1["iterations"][0]) == 16
    assert dt < TOL_DEFL and de < TOL_DEFL
    assert n1 <= 0.75 * n0
    cl0, cs0, m0 = q.localMesonTables(s, qlo, MASS, 1, R2REQ)
    cl1, cs1, m1 = q.localMesonTables(s, qlo, MASS, 1, R2REQ, deflate=B)
    k0, k1 = int(np.sum(m0["iterations"])), int(np.sum(m1["iterations"]))
    dev = max(np.abs(a - b).max() / np.abs(b).max() for a, b in zip([cl1] + cs1, [cl0] + cs0))
    print("localMesonTables: max deviation %.3e of a table's scale; iterations %d -> %d (ratio %.3f)" % (dev, k0, k1, k1 / k0))
    assert dev < TOL_DEFL
    assert k1 < k0


def test_refusals(sol):
    """last test of the module: it changes the operator's links"""
    from oracle import oracle as o

    q, ctx, B, bid, xid, lo = sol["q"], sol["ctx"], sol["B"], sol["bid"], sol["xid"], sol["lo"]
    L = q.lib()
    i4, d4 = C.c_int * 4, C.c_double * 4
    its, fin, nup = (C.c_int * 8)(), (C.c_double * 8)(), (C.c_int * 8)()
    ms, rq = (C.c_double * 8)(*([MASS] * 8)), (C.c_double * 8)(*([R2REQ] * 8))
    x, b = (C.c_int * 8)(*(xid + xid)), (C.c_int * 8)(*(bid + bid))

    def xx(nev, n, xs, bs, sloppy=0):
        return L.qexhip_dev_solve_xx_batch_deflated(ctx._h, B.id, nev, n, xs, bs, ms, rq, 100, 1, sloppy, its, fin, nup)

    def full(nev, n, xs, bs):
        return L.qexhip_dev_solve_batch_deflated(ctx._h, B.id, nev, n, xs, bs, ms, rq, 100, 0, its, fin, nup)

    alias = i4(xid[0], bid[1], xid[2], xid[3])           # x_1 is b_1
    twice = i4(xid[0], xid[0], xid[2], xid[3])
    for fn in (xx, full):
        assert fn(16, 4, alias, b) == -1
        assert fn(16, 4, twice, b) == -1
        assert fn(16, 5, x, b) == -1
        assert fn(16, 0, x, b) == -1
        assert fn(41, 4, x, b) == -1
        assert fn(-1, 4, x, b) == -1
    assert xx(16, 4, x, b, sloppy=3) == -1
    g2 = o.gauge_warm(lo, 0.2, o.RngField(lo, o.RNG_MILC6, 4711))
    o.rephase(lo, g2)
    q.newStag(ctx, g2)
    for fn in (xx, full):
        assert fn(16, 4, x, b) == -3          # QEXHIP_ERR_STATE
        assert fn(0, 4, x, b) == -3
