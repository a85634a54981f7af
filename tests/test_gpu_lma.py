"""Low-mode averaging of the scalar trace on the GPU: k_block_norm2_accum (csrc/eig.hip), qexhip_eig_lowmode_diag,
qexhip_eig_project_out, qexhip_cfield_axpy and scalarTrace(lma=True), against tests/lma_ref.py (numpy over the oracle's D) and the
dense algebra of 4^4.

Inputs are those of tests/eig_ref.py (gauge_warm(0.3), seed 987654321, one-hop links); the eigenvectors are the dense ones, loaded
with set_vector, so nothing here depends on the eigensolver's convergence (the 4.6.10.6 basis of project_out comes from
Staggered.eigs and is compared with the reference built on the DOWNLOADED vectors).  Measured deviations are printed (pytest -s)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import eig_ref as E  # noqa: E402
import lma_ref as LR  # noqa: E402
import scalar_trace_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = E.SEED
LAT, RAGGED, TINY = (4, 4, 4, 8), (4, 6, 10, 6), (4, 4, 4, 4)      # 4.6.10.6: 720 sites per parity, a ragged last tile
R2REQ = 1e-24
TOL5 = 1e-9          # the bar and the reasoning of tests/test_gpu_scalar_trace.py


def _int_field(vol, salt):
    return E.int_pattern(vol, [0], salt)[..., 0].astype(np.float64)


# ---------------------------------------------------------------- the kernel
@pytest.fixture(scope="module", params=[LAT, RAGGED], ids=lambda p: ".".join(map(str, p)))
def rig(request):
    """a context without links, a 133-vector basis of integer vectors, two integer fields that pre-load a cfield"""
    import qex_amd as q

    lat = request.param
    ctx = q.Context(list(lat), device=0)
    vol = int(np.prod(lat))
    vh = vol // 2
    nb = 133
    B = q.EigBasis(ctx, nb)
    V = E.int_pattern(vh, range(nb)).astype(np.float64)             # (vh, 3, 2, nb)
    up = ctx.field_new()
    buf = np.zeros((vol, 3, 2))
    for i in range(nb):
        buf[:vh] = V[..., i]
        ctx.field_upload(up, buf)
        B.set_vector(i, up)
    fa, fb = _int_field(vol, 3), _int_field(vol, 4)
    r = dict(q=q, ctx=ctx, B=B, V=V, vol=vol, vh=vh, up=up, fa=fa, fb=fb, ia=ctx.field_new(fa), ib=ctx.field_new(fb),
             pre=R.site_dot(fa, fb))
    assert r["pre"][:, 0].any() and r["pre"][:, 1].any()
    yield r
    B.free()
    ctx.close()


def test_block_norm2_accum_exact(rig):
    """integer vectors and weights: every product and sum is exact, so the even real parts equal the integer reference and the odd
    sites and the imaginary parts are exactly the pre-loaded values"""
    ctx, B, V, vh = rig["ctx"], rig["B"], rig["V"], rig["vh"]
    n2 = (V.astype(np.int64) ** 2).sum(axis=(1, 2))                  # (vh, nb)
    cf = ctx.cfield_new()
    for n in (1, 5, 128, 130):
        for i0 in (0, 3):
            w = E.int_matrix(n, 1, salt=n + i0)[:, 0]
            ctx.cfield_zero(cf)
            ctx.dev_trace_accum(cf, [rig["ia"]], [rig["ib"]], 1.0)
            assert np.array_equal(ctx.cfield_download(cf), rig["pre"])
            B.block_norm2_accum(i0, w, cf)
            want = rig["pre"].copy()
            want[:vh, 0] += n2[:, i0:i0 + n] @ w.astype(np.int64)
            assert np.abs(want).max() < 2 ** 53
            got = ctx.cfield_download(cf)
            assert np.array_equal(got, want), (n, i0, np.abs(got - want).max())
    ctx.cfield_free(cf)


def test_block_norm2_accum_is_the_accumulate_chain(rig):
    """Gaussian vectors, non-integer weights: bit for bit get_vector + dev_trace_accum, vector after vector"""
    q, ctx, vol, vh = rig["q"], rig["ctx"], rig["vol"], rig["vh"]
    rng = np.random.default_rng(vol)
    nb, i0, n = 21, 2, 19                                            # two unrolled groups of eight and a remainder
    B = q.EigBasis(ctx, nb)
    buf = np.zeros((vol, 3, 2))
    for i in range(nb):
        buf[:vh] = rng.standard_normal((vh, 3, 2))
        ctx.field_upload(rig["up"], buf)
        B.set_vector(i, rig["up"])
    w = rng.standard_normal(n) * np.exp(rng.standard_normal(n))
    c1, c2, f = ctx.cfield_new(), ctx.cfield_new(), ctx.field_new()
    for c in (c1, c2):
        ctx.dev_trace_accum(c, [rig["ia"]], [rig["ib"]], 0.37)
    B.block_norm2_accum(i0, w, c1)
    for j in range(n):
        B.get_vector(i0 + j, f)
        ctx.dev_trace_accum(c2, [f], [f], w[j])
    g1, g2 = ctx.cfield_download(c1), ctx.cfield_download(c2)
    assert np.array_equal(g1, g2)
    assert np.array_equal(g1[vh:], 0.37 * rig["pre"][vh:]) and np.array_equal(g1[:, 1], 0.37 * rig["pre"][:, 1])
    assert not np.array_equal(g1[:vh, 0], 0.37 * rig["pre"][:vh, 0])
    B.free()


# ---------------------------------------------------------------- 4.4.4.8 with 16 dense modes
class _Setup:
    def __init__(self, lat, nev):
        import qex_amd as q
        from oracle import oracle as o

        self.q, self.o, self.lat, self.nev = q, o, lat, nev
        self.olo, self.g, _, _ = E.inputs(lat)
        _, self.w, v = E.dense(lat)
        self.V = np.ascontiguousarray(v[:, :nev])
        self.lo = q.Layout(list(lat))
        self.vol, self.vh = self.lo.vol, self.lo.vol // 2
        self.ctx = q.Context(list(lat), device=0)
        self.stag = q.newStag(self.ctx, self.g)
        self.B = q.EigBasis(self.ctx, nev)
        for i in range(nev):
            self.B.set_vector(i, E.field_of(self.V[:, i], self.vol))
        self.lam = self.B.rayleigh(nev)
        assert np.abs(self.lam - self.w[:nev]).max() < 1e-12
        self.proj = LR.Projector(self.V, self.lam, LR.oracle_D(lat))
        self.eta = q.RngField(list(lat), q.RngMilc6, SEED).z4_vector()
        self._runs, self._refs = {}, {}

    def run(self, seed=SEED, **kw):
        key = (seed,) + tuple(sorted(kw.items()))
        if key not in self._runs:
            kw = dict(kw)
            mass, r2req = kw.pop("mass", 0.1), kw.pop("r2req", R2REQ)
            kw.setdefault("nev", self.nev)
            tr, est, st = self.q.scalarTrace(self.stag, self.lo, self.q.RngField(list(self.lat), self.q.RngMilc6, seed), mass, r2req,
                                             out=None, deflate=self.B, **kw)
            self._runs[key] = (tr[0], est[0], st)
        return self._runs[key]

    def ref_pairs(self, kind, mass):
        """the oracle's solves of every diluted source, once: [(b, phi)] in pattern order"""
        if (kind, mass) not in self._refs:
            solve = lambda b: self.o.solve(self.olo, self.g, None, b, mass, R2REQ, 100000)[0]
            self._refs[(kind, mass)] = R.scalar_trace(solve, self.eta, self.lo.coords, self.lat[3], mass, kind, True)[2]
        return self._refs[(kind, mass)]

    def close(self):
        self.B.free()
        self.ctx.close()


@pytest.fixture(scope="module")
def S():
    s = _Setup(LAT, 16)
    yield s
    s.close()


def test_lowmode_diag_against_the_oracle(S):
    ctx, B = S.ctx, S.B
    c1, c2 = ctx.cfield_new(), ctx.cfield_new()
    for m in (0.1, 0.5):
        ctx.cfield_zero(c1)
        ctx.cfield_zero(c2)
        B.lowmode_diag(16, m, c1)
        wgt = m / (m * m + S.lam)
        B.block_norm2_accum(0, wgt, c2)
        got, hook = ctx.cfield_download(c1), ctx.cfield_download(c2)
        L = S.proj.diag(m)
        scale = L.max()
        assert np.array_equal(got[:S.vh], hook[:S.vh]) and not got[:, 1].any()
        de, do = np.abs(got[:S.vh, 0] - L[:S.vh]).max() / scale, np.abs(got[S.vh:, 0] - L[S.vh:]).max() / scale
        want = wgt.sum()
        se, so = abs(got[:S.vh, 0].sum() - want) / want, abs(got[S.vh:, 0].sum() - want) / want
        print("m = %g: L even %.3e odd %.3e of max L = %.6g; sum rules even %.3e odd %.3e of %.6g" % (m, de, do, scale, se, so, want))
        assert de < 1e-12 and do < 1e-12 and se < 1e-12 and so < 1e-12
        B.lowmode_diag(16, m, c1)                                    # it accumulates
        assert np.abs(ctx.cfield_download(c1)[:, 0] - 2 * L).max() < 1e-12 * scale
    # cfield_axpy: dst += a src on both components
    ctx.cfield_zero(c2)
    fa, fb = ctx.field_new(_int_field(S.vol, 3)), ctx.field_new(_int_field(S.vol, 4))
    ctx.dev_trace_accum(c2, [fa], [fb], 1.0)
    before, src = ctx.cfield_download(c1), ctx.cfield_download(c2)
    ctx.cfield_axpy(c1, -0.75, c2)
    assert np.array_equal(ctx.cfield_download(c1), before + (-0.75) * src) and np.array_equal(ctx.cfield_download(c2), src)
    for f in (fa, fb):
        ctx.field_free(f)
    for c in (c1, c2):
        ctx.cfield_free(c)


def _project_checks(q, ctx, B, nev, lat, label):
    vol = int(np.prod(lat))
    vh = vol // 2
    V = np.stack([E.cvec(B.vector(i), vh) for i in range(nev)], axis=1)
    lam = B.rayleigh(nev)
    proj = LR.Projector(V, lam, LR.oracle_D(lat))
    rng = np.random.default_rng(vol + nev)
    phis = [rng.standard_normal((vol, 3, 2)) for _ in range(4)]
    want = proj.Q(np.stack([LR.cfull(p) for p in phis], axis=1))
    ids = [ctx.field_new() for _ in range(4)]
    alone = []
    for k in range(4):                                                # each system alone
        ctx.field_upload(ids[0], phis[k])
        B.project_out(nev, [ids[0]])
        alone.append(ctx.field_download(ids[0]))
    for n in (1, 2, 3, 4):
        for k in range(n):
            ctx.field_upload(ids[k], phis[k])
        B.project_out(nev, ids[:n])
        for k in range(n):
            got = ctx.field_download(ids[k])
            scale = np.abs(LR.cfull(phis[k])).max()
            dev = np.abs(LR.cfull(got) - want[:, k]).max() / scale
            print("%s n = %d system %d: |Q phi - numpy| %.3e of max|phi|" % (label, n, k, dev))
            assert dev < 1e-12
            assert np.array_equal(got, alone[k]), (n, k)              # each system of a group is itself projected alone
    # the group of four is resident
    for k in range(4):
        d = np.abs(B.block_dot(0, nev, ids[k])).max()
        nrm = np.linalg.norm(phis[k])
        print("%s system %d: max |<v_i, Q phi>| = %.3e |phi|" % (label, k, d / nrm))
        assert d < 1e-13 * nrm
    B.project_out(nev, ids)
    for k in range(4):
        ch = np.abs(ctx.field_download(ids[k]) - alone[k]).max() / np.abs(phis[k]).max()
        print("%s system %d: a second projection changes the field by %.3e of max|phi|" % (label, k, ch))
        assert ch < 1e-12
    for f in ids:
        ctx.field_free(f)


def test_project_out_against_numpy(S):
    _project_checks(S.q, S.ctx, S.B, 16, LAT, "4.4.4.8 / 16 dense modes")
    import qex_amd as q

    _, g, _, _ = E.inputs(RAGGED)
    ctx = q.Context(list(RAGGED), device=0)
    s = q.newStag(ctx, g)
    B = s.eigs(5, nvecs=24, relerr=0.0, abserr=1e-9, cheb_degree=8, cheb_lo=0.3, cheb_hi=0.0, max_restarts=60)
    try:
        print("4.6.10.6: %d of 5 pairs converged, evals %s" % (B.nconv, B.evals))
        _project_checks(q, ctx, B, 5, RAGGED, "4.6.10.6 / 5 modes of Staggered.eigs")
    finally:
        B.free()
        ctx.close()


def test_complete_basis_makes_the_trace_exact():
    """all 384 modes of 4^4: Q = 0, the noise is gone, and every run returns the dense diagonal of m (m^2 - D^2)^-1"""
    m = 0.1
    s = _Setup(TINY, 384)
    try:
        D = LR.dense_D(TINY)
        want = (m * np.linalg.inv(m * m * np.eye(D.shape[0]) - D @ D)).diagonal().real.reshape(-1, 3).sum(axis=1) / 3.0
        scale = want.max()
        runs = {}
        for seed in (SEED, 4242):
            for improved in (True, False):
                tr, est, st = s.run(seed=seed, mass=m, improved_trace=improved, lma=True)
                low = st["low_trace"]
                dl = np.abs(low[:, 0] - want).max() / scale
                dt = max(np.abs(tr[:, 0] - want).max(), np.abs(tr[:, 1]).max()) / scale
                print("seed %d improved=%s: |low_trace - dense| %.3e, |trace - dense| %.3e of max = %.6g; iterations %s" %
                      (seed, improved, dl, dt, scale, st["iterations"][0]))
                assert low.shape == (s.vol, 2) and not low[:, 1].any() and dl < 1e-11 and dt < TOL5
                assert np.abs(st["low_est"] - R.slice_sums(low, s.lo.coords, TINY[3])[:, 0] / 64.0).max() < 1e-12 * scale
                assert np.abs(est - st["low_est"]).max() < TOL5 * scale
                runs[(seed, improved)] = tr
        assert np.abs(runs[(SEED, True)] - runs[(4242, True)]).max() < 2 * TOL5 * scale
        # without LMA the two seeds differ at O(1): the check above is not vacuous
        p1 = s.run(seed=SEED, mass=m, improved_trace=True, lma=False)[0]
        p2 = s.run(seed=4242, mass=m, improved_trace=True, lma=False)[0]
        assert np.abs(p1 - p2).max() > 0.1 * scale
    finally:
        s.close()


@pytest.mark.parametrize("kind,mass,improved", [(R.EO, 0.1, True), (R.EO, 0.1, False), (R.CORNER, 0.5, True)])
def test_lma_trace_against_the_oracle(S, kind, mass, improved):
    tr, est, st = S.run(mass=mass, improved_trace=improved, dilute_type="EO" if kind == R.EO else "CORNER", lma=True)
    rt, re, rl = LR.lma_trace(S.proj, S.ref_pairs(kind, mass), S.lo.coords, LAT[3], mass, improved)
    scale = np.abs(R.cplx(rt)).max()
    dt, de, dl = np.abs(tr - rt).max() / scale, np.abs(est - re).max() / scale, np.abs(st["low_trace"][:, 0] - rl).max() / scale
    print("kind %d m = %g improved=%s: trace %.3e est %.3e low %.3e of max|trace| = %.4g; low part of the site sum %.3f" %
          (kind, mass, improved, dt, de, dl, scale, rl.sum() / rt[:, 0].sum()))
    assert dt < TOL5 and de < TOL5 and dl < 1e-12
    assert set(st) >= {"lowmode_s", "project_s", "low_trace", "low_est", "solve_s", "contract_s", "iterations", "updates"}


def test_lma_leaves_the_solves_alone(S):
    tl, el, sl = S.run(improved_trace=True, lma=True)
    tp, ep, sp = S.run(improved_trace=True)
    assert sl["iterations"] == sp["iterations"] and sl["updates"] == sp["updates"]
    assert "low_trace" not in sp and "project_s" not in sp
    assert not np.array_equal(tl, tp)
    t0, e0, _ = S.run(improved_trace=True, lma=True, nev=0)
    tq, eq, _ = S.run(improved_trace=True, nev=0)
    assert np.array_equal(t0, tq) and np.array_equal(e0, eq)
    for batch in (1, 3):
        tb, eb, _ = S.run(improved_trace=True, lma=True, batch=batch)
        assert np.array_equal(tb, tl) and np.array_equal(eb, el), batch
    for batch in (1, 3):
        assert np.array_equal(S.run(improved_trace=False, lma=True, batch=batch)[0], S.run(improved_trace=False, lma=True)[0]), batch
    ts, es, ss = S.run(improved_trace=True, lma=True, sloppy=1, r2req=1e-18)
    scale = np.abs(tl).max()
    dt, de = np.abs(ts - tl).max() / scale, np.abs(es - el).max() / scale
    print("sloppy=1 with lma: trace deviation %.3e, est deviation %.3e; iterations %s updates %s" %
          (dt, de, ss["iterations"][0], ss["updates"][0]))
    assert dt < TOL5 * 1e3 and de < TOL5 * 1e3
    assert ss["iterations"] == S.run(improved_trace=True, sloppy=1, r2req=1e-18)[2]["iterations"]


def test_refusals(S):
    q, ctx, B = S.q, S.ctx, S.B
    E_ = q.QexHipError
    cf = ctx.cfield_new()
    a, b = ctx.field_new(), ctx.field_new()
    rf = lambda: q.RngField(list(LAT), q.RngMilc6, SEED)
    with pytest.raises(ValueError, match="deflate"):
        q.scalarTrace(S.stag, S.lo, rf(), 0.1, 1e-12, out=None, lma=True)
    with pytest.raises(E_, match="same"):
        B.project_out(16, [a, b, a])
    with pytest.raises(E_, match="n = 5"):
        B.project_out(16, [a, b, a, b, a])
    with pytest.raises(E_, match="n = 0"):
        B.project_out(16, [])
    with pytest.raises(E_, match="unknown field"):
        B.project_out(16, [a, 999])
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(E_, match="mass"):
            B.lowmode_diag(16, bad, cf)
    with pytest.raises(E_, match="nev = 17"):
        B.lowmode_diag(17, 0.1, cf)
    with pytest.raises(E_, match="nev = -1"):
        B.project_out(-1, [a])
    with pytest.raises(E_, match="nev = 17"):
        B.project_out(17, [a])
    with pytest.raises(E_, match="unknown cfield"):
        B.lowmode_diag(16, 0.1, cf + 50)
    with pytest.raises(E_, match="unknown cfield"):
        B.block_norm2_accum(0, [1.0], cf + 50)
    with pytest.raises(E_, match=r"vectors 10\.\.16"):
        B.block_norm2_accum(10, [1.0] * 7, cf)
    with pytest.raises(E_, match="same cfield"):
        ctx.cfield_axpy(cf, 1.0, cf)
    with pytest.raises(E_, match="unknown cfield"):
        ctx.cfield_axpy(cf, 1.0, cf + 50)
    assert not ctx.cfield_download(cf).any()                          # nothing was launched
    # a basis of other links: refused by both entries and by the driver, nothing written
    ctx.field_upload(a, S.eta)
    q.newStag(ctx, S.g)
    try:
        with pytest.raises(E_, match="other links"):
            B.lowmode_diag(16, 0.1, cf)
        with pytest.raises(E_, match="other links"):
            B.project_out(16, [a])
        with pytest.raises(E_, match="other links"):
            q.scalarTrace(S.stag, S.lo, rf(), 0.1, 1e-12, out=None, deflate=B, nev=16, lma=True)
        assert not ctx.cfield_download(cf).any() and np.array_equal(ctx.field_download(a), S.eta)
    finally:
        for i in range(16):                                           # the basis is that of the present links again
            B.set_vector(i, E.field_of(S.V[:, i], S.vol))
    B.lowmode_diag(16, 0.1, cf)
    assert ctx.cfield_download(cf).any()
    ctx.cfield_free(cf)
    for f in (a, b):
        ctx.field_free(f)
