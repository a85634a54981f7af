"""Low modes of the even/odd staggered operator and deflated CG on the device: the three block kernels against numpy, the
eigenpairs of Staggered.eigs against the dense spectrum of the oracle's operator, and the deflated solve against a numpy CG on the
dense matrix.  tests/eig_ref.py builds the inputs and the dense references once per lattice.

Lattices: 4.4.4.6 (576 dimensions on the even sites, exactly 3 wavefront tiles), 4.6.4.6 (864 dimensions, 4.5 tiles: a ragged last
tile), 4.4.8.8 (1536 dimensions).  Observed values are printed (pytest -s).

Sizes.  The block-kernel tests of this module stop at n = 17 vectors per call and rotations of m <= 40; the sizes the eigensolver
and the deflated solves use them at -- more than 128 vectors (the 128-vector chunks of the block dot), m in 64 .. 512 (all three
instantiations of k_rotate, with and without the large-LDS opt-in) and every grid-stride loop wrapped (30.30.30.22, 14.14.14.34)
-- are held to numpy in test_gpu_eig_blocks.py: integer data exactly, Gaussian data within the bound of the kernel's own
summation (observed worst ratios to the bound: rotation 0.016, block axpy 0.007, block dot 0.009).  Here one eigensolve with
nev = 48 of nvecs = 210 on 4.6.4.6 (k_rotate<32> from 210 to 129 vectors, orthogonalisation in two chunks) and the deflated solves
with the 129 vectors it leaves (144 -> 47 iterations) run those paths inside the solvers."""
import ctypes as C

import numpy as np
import pytest

import eig_ref as R

pytestmark = pytest.mark.gpu

# Options that converge nev = 16 / nvecs = 40 to abserr = 1e-9 on these inputs.  A numpy model of the same algorithm on the dense
# operators needs 3-6 restarts with T_8 on [0.3, 1.1 lambda_max] (the 17th eigenvalue is 0.08, the 40th 0.21; lambda_max 5.2) and
# 32-56 restarts with plain Lanczos; max_restarts leaves a factor of five.
CHEB = dict(cheb_degree=8, cheb_lo=0.3, cheb_hi=0.0, max_restarts=40)
PLAIN = dict(cheb_degree=0, max_restarts=300)


# ---------------------------------------------------------------- block kernels
HOOK_LAT = (4, 6, 4, 6)


@pytest.fixture(scope="module")
def hook():
    """a context on 4.6.4.6 with a 40-vector basis, 40 Gaussian host vectors and w (oracle's vector_gaussian)"""
    import qex_amd as q
    from oracle import oracle as o

    o.build()
    lo = o.Layout(list(HOOK_LAT))
    rf = o.RngField(lo, o.RNG_MILC6, R.SEED)
    vecs = [o.vector_gaussian(lo, rf) for _ in range(40)]
    w = o.vector_gaussian(lo, rf)
    ctx = q.Context(list(HOOK_LAT), device=0)
    basis = q.EigBasis(ctx, 40)
    vh = lo.vol // 2
    V = np.stack([R.cvec(v, vh) for v in vecs], axis=1)

    def fill(n=40):
        for i in range(n):
            basis.set_vector(i, vecs[i])

    yield dict(ctx=ctx, basis=basis, vecs=vecs, w=w, V=V, vh=vh, vol=lo.vol, fill=fill)
    basis.free()
    ctx.close()


@pytest.mark.parametrize("i0", [0, 5])
@pytest.mark.parametrize("n", [1, 3, 8, 17])
def test_block_dot_and_block_axpy_against_numpy(hook, n, i0):
    ctx, B, V, vh = hook["ctx"], hook["basis"], hook["V"], hook["vh"]
    hook["fill"](22)
    wid = ctx.field_new(hook["w"])
    w = R.cvec(hook["w"], vh)
    c1 = B.block_dot(i0, n, wid)
    c2 = B.block_dot(i0, n, wid)
    ref = V[:, i0:i0 + n].conj().T @ w
    rel = np.abs(c1 - ref) / np.abs(ref)
    print("block dot n = %d i0 = %d: max relative deviation %.2e, smallest |c| %.3g" % (n, i0, rel.max(), np.abs(ref).min()))
    assert np.array_equal(c1, c2), "block dot is not bit-identical run to run"
    assert rel.max() <= 1e-13
    coef = (np.arange(1, n + 1) * 0.37 - 1.0) + 1j * (0.5 - 0.11 * np.arange(n))
    B.block_axpy(i0, coef, wid)
    y = R.cvec(ctx.field_download(wid), vh)
    yref = w + V[:, i0:i0 + n] @ coef
    full = ctx.field_download(wid)
    dev = np.abs(y - yref).max()
    print("block axpy n = %d i0 = %d: max deviation %.2e" % (n, i0, dev))
    assert dev <= 1e-13
    assert np.array_equal(full[vh:], hook["w"][vh:]), "block axpy touched the odd half"
    ctx.field_free(wid)


def test_block_dot_leaves_out_the_spare_lanes_of_the_ragged_tile(hook):
    """Basis vectors and w are 1 on every site: <v, w> is the number of colour components on the even sites, exactly.  On 4.6.4.6
    that is 3 x 288 = 864 (4.5 tiles: 32 spare lanes in the last one, each of which would add 3).  (The issue quotes 1296 = 3 x 432,
    the figure of 4.6.6.6; the lattice it names, and this test uses, has 288 even sites.)"""
    ctx, B, vh, vol = hook["ctx"], hook["basis"], hook["vh"], hook["vol"]
    ones = np.zeros((vol, 3, 2))
    ones[..., 0] = 1.0
    for i in range(3):
        B.set_vector(i, ones)
    wid = ctx.field_new(ones)
    c = B.block_dot(0, 3, wid)
    ctx.field_free(wid)
    print("all-ones block dot:", c)
    assert 3 * vh == 864 and np.all(c == 864.0)


@pytest.mark.parametrize("m", [2, 17, 40])
def test_rotation_in_place_against_numpy(hook, m):
    B, V, vh = hook["basis"], hook["V"], hook["vh"]
    rng = np.random.default_rng(m)
    for k in sorted({1, m // 2, m}):
        hook["fill"](m)
        Q = rng.uniform(-1, 1, (m, k))
        B.rotate(Q)
        got = np.stack([R.cvec(B.vector(i), vh) for i in range(k)], axis=1)
        dev = np.abs(got - V[:, :m] @ Q).max()
        print("rotate m = %d k = %d: max deviation %.2e" % (m, k, dev))
        assert dev <= 1e-13
        if k < m:     # the header's promise: vectors k .. m-1 are left as they were
            assert np.array_equal(R.cvec(B.vector(m - 1), vh), V[:, m - 1])


def test_block_hooks_refuse_bad_ranges(hook):
    import qex_amd as q

    ctx, B = hook["ctx"], hook["basis"]
    wid = ctx.field_new(hook["w"])
    out = np.zeros(100)
    L = q.lib()
    assert L.qexhip_eig_block_dot(ctx._h, B.id, 30, 11, wid, out.ctypes.data) == -1
    assert L.qexhip_eig_block_dot(ctx._h, B.id, -1, 2, wid, out.ctypes.data) == -1
    assert L.qexhip_eig_block_axpy(ctx._h, B.id, 0, 41, out.ctypes.data, wid) == -1
    Q = np.zeros((41, 41))
    assert L.qexhip_eig_rotate(ctx._h, B.id, 41, 2, Q.ctypes.data) == -1
    assert L.qexhip_eig_rotate(ctx._h, B.id, 3, 4, Q.ctypes.data) == -1
    assert L.qexhip_eig_get_vector(ctx._h, B.id, 40, wid) == -1
    ctx.field_free(wid)


# ---------------------------------------------------------------- eigenpairs
def _check_pairs(lat, hisq, B, nev):
    H, w, _ = R.dense(lat, hisq)
    vh = H.shape[0] // 3
    print("%s hisq=%s: nconv %d, stats %s" % (lat, hisq, B.nconv, B.stats))
    assert B.nconv == nev
    assert np.all(np.diff(B.evals) > 0)
    V = np.stack([R.cvec(B.vector(i), vh) for i in range(nev)], axis=1)
    orth = np.abs(V.conj().T @ V - np.eye(nev)).max()
    worst = 0.0
    for i in range(nev):
        ro = np.linalg.norm(R.oracle_H(lat, hisq, V[:, i]) - B.evals[i] * V[:, i])
        worst = max(worst, ro - B.resid[i])
        assert B.resid[i] <= 1e-9, (i, B.resid[i])
        assert ro <= B.resid[i] + 1e-12, (i, ro, B.resid[i])
        assert abs(B.evals[i] - w[i]) <= B.resid[i] + 1e-12 * w[-1], (i, B.evals[i], w[i], B.resid[i])
    print("   max resid %.2e, oracle resid - resid <= %.2e, |V^+ V - 1| %.2e, max |lambda - dense| %.2e"
          % (B.resid.max(), worst, orth, np.abs(B.evals - w[:nev]).max()))
    assert orth <= 1e-12


@pytest.mark.parametrize("mode", ["cheb", "plain"])
@pytest.mark.parametrize("lat", [(4, 4, 4, 6), (4, 6, 4, 6)])
def test_eigenpairs_against_the_dense_spectrum(lat, mode):
    import qex_amd as q

    _, g, _, _ = R.inputs(lat)
    ctx = q.Context(list(lat), device=0)
    s = q.newStag(ctx, g)
    B = s.eigs(16, nvecs=40, relerr=0.0, abserr=1e-9, **(CHEB if mode == "cheb" else PLAIN))
    try:
        _check_pairs(lat, False, B, 16)
    finally:
        B.free()
        ctx.close()


def test_eigenpairs_of_a_hisq_operator():
    """HISQ fat + Naik links (smeared on the device; the dense reference from the oracle's hisq_smear + newStag3 operator)"""
    import qex_amd as q

    lat = (4, 6, 4, 6)
    _, g, _, _ = R.inputs(lat)
    _, w, _ = R.dense(lat, True)
    gaps = np.diff(w[:10])
    print("HISQ dense spectrum, lowest 10:", w[:10], "gaps:", gaps)
    assert gaps.min() > 1e-6, "the input's low spectrum is degenerate: not a fair input"
    ctx = q.Context(list(lat), device=0)
    s = q.Staggered(ctx, g, smear=q.HisqCoefs())
    B = s.eigs(8, nvecs=24, relerr=0.0, abserr=1e-9, **CHEB)
    try:
        _check_pairs(lat, True, B, 8)
    finally:
        B.free()
        ctx.close()


# ---------------------------------------------------------------- more than 128 vectors
# nev = 48 of nvecs = 210 on 4.6.4.6: every restart rotates m = 210 vectors down to k = 48 + (210 - 48) / 2 = 129 with k_rotate<32>
# (five passes of its column loop), and the orthogonalisation of steps 128 .. 209 runs the block dot in two chunks.  The 48th
# eigenvalue is 0.199 < cheb_lo.  The 129 Ritz vectors the last restart keeps are orthonormal (48 converged pairs, 81 further Ritz
# vectors of the same Lanczos space), which is all the projection x0 = sum_i v_i <v_i, b> / (4 (rho_i + m^2)) with their Rayleigh
# quotients rho_i needs: the deflated solves below take nev = 129 of them.
WLAT, WNEV, WNVECS, WDEFL = (4, 6, 4, 6), 48, 210, 129


@pytest.fixture(scope="module")
def wide():
    import time

    import qex_amd as q
    from oracle import oracle as o

    lo, g, _, b = R.inputs(WLAT)
    ctx = q.Context(list(WLAT), device=0)
    s = q.newStag(ctx, g)
    t0 = time.time()
    B = s.eigs(WNEV, nvecs=WNVECS, relerr=0.0, abserr=1e-9, **CHEB)
    print("eigs nev = %d nvecs = %d on %s: %.2f s" % (WNEV, WNVECS, WLAT, time.time() - t0))
    rf = o.RngField(lo, o.RNG_MILC6, 4242)
    bs = [np.ascontiguousarray(b)] + [o.vector_gaussian(lo, rf) for _ in range(3)]
    yield dict(ctx=ctx, s=s, B=B, bs=bs, lo=lo, g=g, vh=lo.vol // 2)
    B.free()
    ctx.close()


def test_eigenpairs_with_more_than_128_vectors(wide):
    assert WNVECS > 128 and WNEV + (WNVECS - WNEV) // 2 == WDEFL > 128
    _check_pairs(WLAT, False, wide["B"], WNEV)


def test_deflated_solves_with_more_than_128_vectors(wide):
    """what test_deflated_solve_against_numpy_cg and test_even_batch_against_the_single_deflated_solve (test_gpu_defl_batch.py)
    assert at nev = 16, at nev = 129: block dot and block axpy in two chunks, single and for four right-hand sides"""
    from oracle import oracle as o

    ctx, B, bs, vh = wide["ctx"], wide["B"], wide["bs"], wide["vh"]
    V = np.stack([R.cvec(B.vector(i), vh) for i in range(WDEFL)], axis=1)
    orth = np.abs(V.conj().T @ V - np.eye(WDEFL)).max()
    print("the %d leading vectors: |V^+ V - 1| %.2e" % (WDEFL, orth))
    assert orth <= 1e-12
    bid, xid = [ctx.field_new(v) for v in bs], [ctx.field_new() for _ in bs]
    one = ctx.field_new()
    its0, _, _ = ctx.dev_solve_xx(one, bid[0], MASS, R2REQ, 5000)
    its1, r1 = ctx.dev_solve_xx_deflated(B, WDEFL, one, bid[0], MASS, R2REQ, 5000)
    xf = ctx.field_download(one)
    rr = R.cvec(bs[0], vh) - R.cvec(o.stagD2xx(wide["lo"], wide["g"], None, xf, MASS * MASS, True), vh)
    r2o = np.vdot(rr, rr).real / np.vdot(R.cvec(bs[0], vh), R.cvec(bs[0], vh)).real
    print("plain %d its, deflated with %d vectors %d its, ratio %.3f; r2/b2 %.6e (oracle %.6e)" % (its0, WDEFL, its1, its1 / its0, r1, r2o))
    assert its1 <= 0.75 * its0
    assert r1 <= R2REQ * (1 + 1e-3)
    assert abs(r2o / r1 - 1) <= 1e-6
    ms = [0.01, 0.01, 0.02, 0.05]
    its, r2, nup = ctx.dev_solve_xx_batch_deflated(B, WDEFL, xid, bid, ms, R2REQ, 5000)
    for k in range(4):
        xk = ctx.field_download(xid[k])
        i1, rk = ctx.dev_solve_xx_deflated(B, WDEFL, one, bid[k], ms[k], R2REQ, 5000)
        x1 = ctx.field_download(one)
        eq = np.array_equal(xk, x1)
        rel = np.linalg.norm(xk - x1) / np.linalg.norm(x1)
        print("system %d (m = %g): batch %d its r2/b2 %.4e, single %d its r2/b2 %.4e, x %s" %
              (k, ms[k], its[k], r2[k], i1, rk, "bit-identical" if eq else "relerr %.2e" % rel))
        assert eq or rel < 1e-13
        assert abs(its[k] - i1) <= 1
        assert r2[k] <= R2REQ * (1 + 1e-3)
    assert nup == [0, 0, 0, 0]
    for f in bid + xid + [one]:
        ctx.field_free(f)


# ---------------------------------------------------------------- deflated solve
DLAT, MASS, R2REQ = (4, 4, 8, 8), 0.01, 1e-20


@pytest.fixture(scope="module")
def defl():
    import qex_amd as q

    lo, g, _, b = R.inputs(DLAT)
    H, w, v = R.dense(DLAT)
    A = 4.0 * (MASS * MASS * np.eye(H.shape[0]) + H)
    vh = lo.vol // 2
    bc = R.cvec(b, vh)
    _, its_plain = R.cg(A, bc, np.zeros_like(bc), R2REQ)
    x0 = v[:, :16] @ ((v[:, :16].conj().T @ bc) / (4.0 * (w[:16] + MASS * MASS)))
    _, its_defl = R.cg(A, bc, x0, R2REQ)
    ctx = q.Context(list(DLAT), device=0)
    s = q.newStag(ctx, g)
    B = s.eigs(16, nvecs=40, relerr=0.0, abserr=1e-9, **CHEB)
    assert B.nconv == 16
    bid, xid = ctx.field_new(np.ascontiguousarray(b)), ctx.field_new()
    print("numpy CG on the dense A: %d iterations from 0, %d from the exact 16-mode guess" % (its_plain, its_defl))
    yield dict(ctx=ctx, s=s, B=B, bid=bid, xid=xid, A=A, bc=bc, b=b, lo=lo, g=g, vh=vh, its_plain=its_plain, its_defl=its_defl)
    B.free()
    ctx.close()


def _close(a, ref):
    return abs(a - ref) <= max(2, 0.02 * ref)


def test_deflated_solve_against_numpy_cg(defl):
    from oracle import oracle as o

    ctx, B, bid, xid, vh = defl["ctx"], defl["B"], defl["bid"], defl["xid"], defl["vh"]
    its0, r0, _ = ctx.dev_solve_xx(xid, bid, MASS, R2REQ, 5000)
    its1, r1 = ctx.dev_solve_xx_deflated(B, 16, xid, bid, MASS, R2REQ, 5000)
    xf = ctx.field_download(xid)
    x = R.cvec(xf, vh)
    xs = np.linalg.solve(defl["A"], defl["bc"])
    xerr = np.linalg.norm(x - xs) / np.linalg.norm(xs)
    rr = R.cvec(defl["b"], vh) - R.cvec(o.stagD2xx(defl["lo"], defl["g"], None, xf, MASS * MASS, True), vh)
    r2o = np.vdot(rr, rr).real / np.vdot(defl["bc"], defl["bc"]).real
    print("plain %d its (numpy %d), deflated %d its (numpy %d), ratio %.3f; r2/b2 %.6e (oracle %.6e, rel dev %.2e); |x - solve| %.2e"
          % (its0, defl["its_plain"], its1, defl["its_defl"], its1 / its0, r1, r2o, abs(r2o / r1 - 1), xerr))
    assert _close(its0, defl["its_plain"])
    assert _close(its1, defl["its_defl"])
    assert its1 <= 0.75 * its0
    assert r1 <= R2REQ * (1 + 1e-3)
    assert abs(r2o / r1 - 1) <= 1e-6
    assert xerr <= 1e-9


def test_deflating_with_no_modes_is_the_undeflated_solver(defl):
    ctx, B, bid, xid = defl["ctx"], defl["B"], defl["bid"], defl["xid"]
    its0, r0, _ = ctx.dev_solve_xx(xid, bid, MASS, R2REQ, 5000)
    x0 = ctx.field_download(xid)
    its1, r1 = ctx.dev_solve_xx_deflated(B, 0, xid, bid, MASS, R2REQ, 5000)
    x1 = ctx.field_download(xid)
    assert its1 == its0 and r1 == r0 and np.array_equal(x0, x1)


def test_deflated_sloppy_solve(defl):
    ctx, B, bid, xid = defl["ctx"], defl["B"], defl["bid"], defl["xid"]
    its0, r0, nup = ctx.dev_solve_xx_sloppy(xid, bid, MASS, R2REQ, 20000)
    its1, r1 = ctx.dev_solve_xx_deflated(B, 16, xid, bid, MASS, R2REQ, 20000, sloppy=1)
    print("sloppy: undeflated %d its (r2/b2 %.3e, %d updates), deflated %d its (r2/b2 %.3e), ratio %.3f" % (its0, r0, nup, its1, r1, its1 / its0))
    assert r1 <= R2REQ * (1 + 1e-3)
    assert its1 <= 0.75 * its0


def test_host_pointer_twins_and_the_full_solve(defl):
    """qexhip_stag_solve_xx_deflated gives the resident entry's bits; Staggered.solve(deflate=) reaches the full solve's residual in
    fewer iterations than the undeflated one"""
    import qex_amd as q

    ctx, s, B, bid, xid, b = defl["ctx"], defl["s"], defl["B"], defl["bid"], defl["xid"], defl["b"]
    its1, r1 = ctx.dev_solve_xx_deflated(B, 16, xid, bid, MASS, R2REQ, 5000)
    xd = ctx.field_download(xid)
    sp = q.SolverParams(r2req=R2REQ, maxits=5000, verbosity=0)
    xh = np.zeros_like(b)
    s.solveEE(xh, np.ascontiguousarray(b), MASS, sp, deflate=B)
    assert sp.iterations == its1 and sp.r2 == r1 and np.array_equal(xh, xd)
    sp0, sp1 = q.SolverParams(r2req=1e-16, maxits=5000, verbosity=0), q.SolverParams(r2req=1e-16, maxits=5000, verbosity=0)
    x0, x1 = np.zeros_like(b), np.zeros_like(b)
    s.solve(x0, np.ascontiguousarray(b), MASS, sp0)
    s.solve(x1, np.ascontiguousarray(b), MASS, sp1, deflate=B)
    dx = np.linalg.norm(x1 - x0) / np.linalg.norm(x0)
    print("full solve: %d its undeflated, %d deflated; r2 %.2e / %.2e; |dx|/|x| %.2e" % (sp0.iterations, sp1.iterations, sp0.r2, sp1.r2, dx))
    assert sp1.r2 <= 1e-16 and sp1.iterations < sp0.iterations
    # both solutions have |D x - b| <= 1e-8 |b|: they differ by at most 2e-8 |b| / sigma_min(D), sigma_min^2 = lambda_0 + m^2 >= 0.0157
    assert dx <= 2e-8 / np.sqrt(0.0157) * np.linalg.norm(b) / np.linalg.norm(x0)


def test_a_basis_of_other_links_is_refused(defl):
    """last test of the module: it changes the operator's links"""
    import qex_amd as q
    from oracle import oracle as o

    ctx, B, bid, xid, lo = defl["ctx"], defl["B"], defl["bid"], defl["xid"], defl["lo"]
    g2 = o.gauge_warm(lo, 0.2, o.RngField(lo, o.RNG_MILC6, 4711))
    o.rephase(lo, g2)
    q.newStag(ctx, g2)
    its, fin = C.c_int(0), C.c_double(0)
    rc = q.lib().qexhip_dev_solve_xx_deflated(ctx._h, B.id, 16, xid, bid, MASS, R2REQ, 100, 0, C.byref(its), C.byref(fin))
    assert rc == -3, rc      # QEXHIP_ERR_STATE
    rc = q.lib().qexhip_dev_solve_xx_deflated(ctx._h, B.id, 0, xid, bid, MASS, R2REQ, 100, 0, C.byref(its), C.byref(fin))
    assert rc == -3, rc
