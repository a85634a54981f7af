"""The stochastic scalar trace on the GPU (csrc/trace.hip, the Z4 / Z2 cases of csrc/rng.hip, qex_amd/scalar_trace.py;
src/observables/scalarTrace.nim, src/algorithms/dilution.nim).

The kernels are pinned against the numpy restatement tests/scalar_trace_ref.py on identical uploaded fields (bit for bit where the
values are exact), the whole measurement against the oracle's CG, and by the identity Re sum <b, phi> = m sum <phi, phi>.
Measured deviations are printed (pytest -s)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import qex_amd as q  # noqa: E402
import scalar_trace_ref as R  # noqa: E402
from oracle import oracle as o  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 987654321
EPS = np.finfo(np.float64).eps
LATS = [[4, 4, 4, 8], [4, 6, 10, 6]]      # 4.6.10.6: 720 sites per parity (partial tile), 60-site slices (partial 256-site chunk)


@pytest.mark.parametrize("lat", LATS)
def test_device_noise_is_the_host_noise(lat):
    ctx = q.Context(lat)
    host, dev = q.RngField(lat, q.RngMilc6, SEED), q.RngField(lat, q.RngMilc6, SEED)
    f = ctx.field_new()
    draws = []
    for name in ("z4", "z2", "z4", "z4"):           # the later draws continue the stream
        want = getattr(host, name + "_vector")()
        getattr(dev, "dev_" + name + "_vector")(ctx, f)
        got = ctx.field_download(f)
        assert np.array_equal(got, want), name
        assert np.array_equal(dev.state(), host.state()), name
        draws.append(got)
    assert not np.array_equal(draws[2], draws[3]) and not np.array_equal(draws[0], draws[2])
    assert set(np.unique(R.cplx(draws[0]))) == {1, -1, 1j, -1j} and set(np.unique(R.cplx(draws[1]))) == {1, -1}
    with pytest.raises(q.QexHipError, match="RngMilc6"):
        q.RngField(lat, q.MRG32k3a, 5).dev_z4_vector(ctx, f)
    ctx.close()


@pytest.mark.parametrize("lat", LATS)
@pytest.mark.parametrize("kind", [R.EO, R.CORNER])
def test_dilute_is_the_numpy_mask(lat, kind):
    lo = q.Layout(lat)
    ctx = q.Context(lat)
    src = np.random.default_rng(sum(lat) + kind).standard_normal((lo.vol, 3, 2))
    fs = ctx.field_new(src)
    dst = [ctx.field_new(src) for _ in range(4)]           # not zero beforehand: every site must be written
    pats = R.patterns(kind, lat[3])
    for scale in (1.0, 1.0 / np.sqrt(2.0)):
        total = np.zeros_like(src)
        k0, n, sizes, mixed = 0, 1, set(), False
        while k0 < len(pats):
            grp = pats[k0:k0 + n]
            ctx.dev_dilute(dst[:len(grp)], fs, kind, [i for _, i in grp], [t for t, _ in grp], scale)
            for d, (t, idx) in zip(dst, grp):
                got = ctx.field_download(d)
                assert np.array_equal(got, R.dilute(src, lo.coords, kind, idx, t, scale)), (scale, t, idx)
                assert not np.signbit(got[~R.mask(lo.coords, kind, idx, t)]).any()           # +0.0 outside the pattern
                total += got
            sizes.add(len(grp))
            mixed = mixed or len({t for t, _ in grp}) > 1
            k0 += len(grp)
            n = n % 4 + 1
        assert sizes == {1, 2, 3, 4} and mixed
        if scale == 1.0:
            assert np.array_equal(total, src)              # the patterns of all t partition the lattice
    # the same pattern twice in one launch, out of order t
    ctx.dev_dilute(dst[:3], fs, kind, [1, 1, 0], [lat[3] - 1, lat[3] - 1, 0], 1.0)
    assert np.array_equal(ctx.field_download(dst[0]), ctx.field_download(dst[1]))
    assert np.array_equal(ctx.field_download(dst[2]), R.dilute(src, lo.coords, kind, 0, 0))
    ctx.close()


def test_bad_arguments_raise():
    lat = [4, 4, 4, 4]
    ctx = q.Context(lat)
    a, b, c = ctx.field_new(), ctx.field_new(), ctx.field_new()
    tr = ctx.cfield_new()
    with pytest.raises(q.QexHipError, match="n = 5"):
        ctx.dev_dilute([a] * 5, b, 0, [0] * 5, [0] * 5)
    with pytest.raises(q.QexHipError, match="n = 0"):
        ctx.dev_dilute([], b, 0, [], [])
    with pytest.raises(q.QexHipError, match="kind = 2"):
        ctx.dev_dilute([a], b, 2, [0], [0])
    with pytest.raises(q.QexHipError, match="idx"):
        ctx.dev_dilute([a], b, 0, [2], [0])
    with pytest.raises(q.QexHipError, match="idx"):
        ctx.dev_dilute([a], b, 1, [8], [0])
    with pytest.raises(q.QexHipError, match="idx"):
        ctx.dev_dilute([a], b, 1, [-1], [0])
    with pytest.raises(q.QexHipError, match=r"t\[1\] = 4"):
        ctx.dev_dilute([a, c], b, 0, [0, 1], [3, 4])
    with pytest.raises(q.QexHipError, match=r"t\[0\] = -1"):
        ctx.dev_dilute([a], b, 0, [0], [-1])
    with pytest.raises(q.QexHipError, match="source"):
        ctx.dev_dilute([a, b], b, 0, [0, 1], [0, 0])
    with pytest.raises(q.QexHipError, match="same field"):
        ctx.dev_dilute([a, c, a], b, 0, [0, 1, 0], [0, 0, 1])
    with pytest.raises(q.QexHipError, match="unknown field"):
        ctx.dev_dilute([a, 999], b, 0, [0, 1], [0, 0])
    with pytest.raises(q.QexHipError, match="unknown field"):
        ctx.dev_dilute([a], 999, 0, [0], [0])
    with pytest.raises(q.QexHipError, match="n = 5"):
        ctx.dev_trace_accum(tr, [a] * 5, [b] * 5)
    with pytest.raises(q.QexHipError, match="n = 0"):
        ctx.dev_trace_accum(tr, [], [])
    with pytest.raises(q.QexHipError, match="unknown field"):
        ctx.dev_trace_accum(tr, [a, 999], [b, b])
    with pytest.raises(q.QexHipError, match="unknown cfield"):
        ctx.dev_trace_accum(tr + 7, [a], [b])
    with pytest.raises(q.QexHipError, match="unknown cfield"):
        ctx.dev_cfield_slices(0)
    with pytest.raises(q.QexHipError, match="unknown cfield"):
        ctx.cfield_download(a + 100)
    ctx.cfield_free(tr)
    with pytest.raises(q.QexHipError, match="unknown cfield"):
        ctx.cfield_zero(tr)
    ctx.close()                                     # frees the colour vectors that are left


@pytest.mark.parametrize("lat", LATS)
def test_accumulate_and_slices_against_numpy(lat):
    lo = q.Layout(lat)
    ctx = q.Context(lat)
    rng = np.random.default_rng(sum(lat))
    A = [rng.standard_normal((lo.vol, 3, 2)) for _ in range(4)]
    B = [rng.standard_normal((lo.vol, 3, 2)) for _ in range(4)]
    ia, ib = [ctx.field_new(f) for f in A], [ctx.field_new(f) for f in B]
    tr, tr1 = ctx.cfield_new(), ctx.cfield_new()
    assert not ctx.cfield_download(tr).any()                      # created zeroed

    def mag(xs, ys, coef):       # sum_k sum_col |a||b| per site
        return abs(coef) * sum((np.abs(R.cplx(x)) * np.abs(R.cplx(y))).sum(axis=1) for x, y in zip(xs, ys))

    # unimproved form, n = 1..4, on top of what is there
    ref, bound = np.zeros((lo.vol, 2)), np.zeros(lo.vol)
    for n, coef in ((1, 1.0), (2, -0.75), (3, 1.0), (4, 0.3)):
        ctx.dev_trace_accum(tr, ia[:n], ib[:n], coef)
        for x, y in zip(A[:n], B[:n]):
            R.accumulate(ref, x, y, coef)
        bound += mag(A[:n], B[:n], coef)
        got = ctx.cfield_download(tr)
        dev = np.abs(R.cplx(got) - R.cplx(ref))
        print("lat %s unimproved n=%d: max deviation / bound %.3f" % (lat, n, (dev / (32 * EPS * bound)).max()))
        assert (dev <= 32 * EPS * bound).all()
    # four pairs in one launch = four launches with one pair each, bit for bit, from the same starting field
    ctx.dev_trace_accum(tr1, ia[:1], ib[:1], 1.0)
    ctx.dev_trace_accum(tr1, ia[:2], ib[:2], -0.75)
    ctx.dev_trace_accum(tr1, ia[:3], ib[:3], 1.0)
    for k in range(4):
        ctx.dev_trace_accum(tr1, [ia[k]], [ib[k]], 0.3)
    assert np.array_equal(ctx.cfield_download(tr1), got)
    # improved form: a is b, the imaginary part is exactly 0; mixed with an unimproved pair in one launch it stays that pair's
    ctx.cfield_zero(tr1)
    assert not ctx.cfield_download(tr1).any()
    ctx.dev_trace_accum(tr1, ia, ia, 0.1)
    g1 = ctx.cfield_download(tr1)
    ref1 = np.zeros((lo.vol, 2))
    for x in A:
        R.accumulate(ref1, x, x, 0.1)
    assert not g1[:, 1].any() and (np.abs(g1[:, 0] - ref1[:, 0]) <= 32 * EPS * mag(A, A, 0.1)).all()
    ctx.cfield_zero(tr1)
    for x in ia:
        ctx.dev_trace_accum(tr1, [x], [x], 0.1)
    assert np.array_equal(ctx.cfield_download(tr1), g1)
    # scale is one exact multiplication per component
    ctx.cfield_scale(tr, 1.0 / 3.0)
    gs = ctx.cfield_download(tr)
    assert np.array_equal(gs, got * (1.0 / 3.0))

    # slice sums
    nt, per = lat[3], lo.vol // lat[3]
    sl = ctx.dev_cfield_slices(tr)
    want = R.slice_sums(gs, lo.coords, nt)
    tol = np.zeros((nt, 2))
    np.add.at(tol, lo.coords[:, 3], np.abs(gs))
    tol *= EPS * per
    print("lat %s slices: max deviation / bound %.3g" % (lat, (np.abs(sl - want) / tol).max()))
    assert sl.shape == (nt, 2) and (np.abs(sl - want) <= tol).all()
    assert np.array_equal(ctx.dev_cfield_slices(tr), sl)                      # fixed reduction order: the same bits again
    assert (np.abs(sl.sum(axis=0) - gs.sum(axis=0)) <= tol.sum(axis=0)).all()
    ctx.close()


# ---- the whole measurement on 4.4.4.8 ----
LAT = [4, 4, 4, 8]
R2REQ = 1e-24
TOL5 = 1e-9          # relative to max|trace|: both sides stop at |r| = 1e-12 |b|, |d phi| <= |r| / m = 1e-11 |b|, the trace is bilinear in
                     # phi with |D + m| = O(10): a few 1e-10


class _Setup:
    def __init__(self):
        self.lo, self.olo = q.Layout(LAT), o.Layout(LAT)
        self.g = o.gauge_warm(self.olo, 0.5, o.RngField(self.olo, o.RNG_MILC6, SEED))
        o.rephase(self.olo, self.g)
        self.ctx = q.Context(LAT)
        self.stag = q.newStag(self.ctx, self.g)
        self.eta = q.RngField(LAT, q.RngMilc6, SEED).z4_vector()
        self._runs, self._refs = {}, {}

    def run(self, **kw):
        """scalarTrace on a fresh same-seed generator; results kept per argument set"""
        key = tuple(sorted(kw.items()))
        if key not in self._runs:
            kw = dict(kw)
            mass, r2req = kw.pop("mass", 0.1), kw.pop("r2req", R2REQ)
            lines = []
            tr, est, st = q.scalarTrace(self.stag, self.lo, q.RngField(LAT, q.RngMilc6, SEED), mass, r2req, out=lines.append, **kw)
            self._runs[key] = (tr[0], est[0], st, lines)
        return self._runs[key]

    def ref(self, kind, mass):
        """the oracle's solves of every diluted source, once: [(b, phi)] in pattern order"""
        if (kind, mass) not in self._refs:
            its = []

            def solve(b):
                x, it, _ = o.solve(self.olo, self.g, None, b, mass, R2REQ, 100000)
                its.append(it)
                return x

            self._refs[(kind, mass)] = R.scalar_trace(solve, self.eta, self.lo.coords, LAT[3], mass, kind, True)[2]
            print("oracle: %d solves at mass %g, iterations %d..%d" % (len(its), mass, min(its), max(its)))
        return self._refs[(kind, mass)]

    def ref_trace(self, kind, mass, improved):
        pairs = iter(self.ref(kind, mass))
        return R.scalar_trace(lambda b: next(pairs)[1], self.eta, self.lo.coords, LAT[3], mass, kind, improved)[:2]


@pytest.fixture(scope="module")
def S():
    s = _Setup()
    yield s
    s.ctx.close()


@pytest.mark.parametrize("improved", [True, False])
def test_scalar_trace_against_the_oracle_eo(S, improved):
    tr, est, st, _ = S.run(improved_trace=improved)
    rt, re = S.ref_trace(R.EO, 0.1, improved)
    scale = np.abs(R.cplx(rt)).max()
    dt, de = np.abs(tr - rt).max() / scale, np.abs(est - re).max() / scale
    print("EO improved=%s: trace deviation %.3e, est deviation %.3e (of max|trace| = %.4g); iterations %s" %
          (improved, dt, de, scale, st["iterations"][0]))
    assert tr.shape == (S.lo.vol, 2) and est.shape == (LAT[3],) and len(st["iterations"][0]) == 16
    assert dt < TOL5 and de < TOL5
    if improved:
        assert not tr[:, 1].any()


def test_scalar_trace_against_the_oracle_corner(S):
    tr, est, st, _ = S.run(improved_trace=True, dilute_type="CORNER", mass=0.5)
    rt, re = S.ref_trace(R.CORNER, 0.5, True)
    scale = np.abs(R.cplx(rt)).max()
    dt, de = np.abs(tr - rt).max() / scale, np.abs(est - re).max() / scale
    print("CORNER improved: trace deviation %.3e, est deviation %.3e (of max|trace| = %.4g)" % (dt, de, scale))
    assert len(st["iterations"][0]) == 64 and dt < TOL5 and de < TOL5


def test_improved_and_unimproved_site_sums_agree(S):
    """D is anti-Hermitian: Re sum_x <b, phi> = m sum_x <phi, phi> for every diluted source, so the two traces have the same site
    sum up to the solver's residual"""
    t1, e1, _, _ = S.run(improved_trace=True)
    t0, e0, _, _ = S.run(improved_trace=False)
    s1, s0 = t1[:, 0].sum(), t0[:, 0].sum()
    print("site sums: improved %.15g unimproved %.15g relative difference %.3e" % (s1, s0, abs(s1 - s0) / abs(s1)))
    assert abs(s1 - s0) <= 1e-10 * abs(s1)


def test_grouping_invariance(S):
    """the fp64 lock-step batch is its single solves bit for bit, and the accumulation adds pattern after pattern: batch = 1, 2, 3
    and 4 give the same trace bits"""
    ctx, lo = S.ctx, S.lo
    eta = ctx.field_new(S.eta)
    b, x, y = ([ctx.field_new() for _ in range(4)] for _ in range(3))
    ctx.dev_dilute(b, eta, R.EO, [0, 1, 0, 1], [0, 0, 1, 1])
    i4, _ = ctx.dev_solve_batch(x, b, [0.1] * 4, R2REQ, 100000)
    i1 = [ctx.dev_solve_batch([y[k]], [b[k]], [0.1], R2REQ, 100000)[0][0] for k in range(4)]
    same = [np.array_equal(ctx.field_download(x[k]), ctx.field_download(y[k])) for k in range(4)]
    print("batch of four vs single solves: iterations %s / %s, bit-equal %s" % (i4, i1, same))
    for f in [eta] + b + x + y:
        ctx.field_free(f)
    assert all(same) and i4 == i1
    t4 = S.run(improved_trace=True)[0]
    for batch in (1, 3):
        tb, eb, _, _ = S.run(improved_trace=True, batch=batch)
        assert np.array_equal(tb, t4) and np.array_equal(eb, S.run(improved_trace=True)[1]), batch
    assert np.array_equal(S.run(improved_trace=False, batch=1)[0], S.run(improved_trace=False)[0])


def test_driver_log_lines_and_gaussian_norm(S):
    tr, est, st, lines = S.run(improved_trace=True)
    assert lines[0] == "Generating a Z4 noise source." and lines[1] == "noise norm2: %r" % (3.0 * S.lo.vol,)
    body = lines[2:2 + 3 * 16]
    assert all(ln.startswith("src norm2: ") for ln in body[0::3]) and all(ln.startswith("dest norm2: ") for ln in body[1::3])
    assert set(body[2::3]) == {"Computing the improved trace."}
    assert [float(ln.split()[-1]) for ln in body[0::3]] == [3.0 * S.lo.vol / 16] * 16         # Z4: |eta(x)|^2 = 3 on a 16th of the sites
    tail = lines[2 + 3 * 16:]
    assert tail == ["initsrc 0 timeslice %d pbp %r" % (t, float(est[t])) for t in range(LAT[3])]
    assert "Computing the unimproved trace." in S.run(improved_trace=False)[3]
    # Gauss: the source carries 1/sqrt(2) (scalarTrace.nim:157-160)
    gv = q.RngField(LAT, q.RngMilc6, SEED).gaussian_vector()
    lg = S.run(improved_trace=False, source_type="Gauss", r2req=1e-12)[3]
    assert lg[0] == "Generating a Gauss noise source."
    n2 = float(lg[1].split()[-1])
    assert abs(n2 - 0.5 * (gv ** 2).sum()) < 1e-12 * n2
    srcs = [float(ln.split()[-1]) for ln in lg if ln.startswith("src norm2: ")]
    assert len(srcs) == 16 and abs(sum(srcs) - n2) < 1e-12 * n2
    # two sources: the second continues the stream
    trs, ests, st2 = q.scalarTrace(S.stag, S.lo, q.RngField(LAT, q.RngMilc6, SEED), 0.1, 1e-16, num_stoch=2, out=None)
    assert len(trs) == 2 and len(ests) == 2 and len(st2["iterations"]) == 2 and not np.array_equal(trs[0], trs[1])
    assert np.abs(trs[0] - tr).max() < 1e-5 * np.abs(tr).max()
    for bad in (dict(source_type="Z3"), dict(dilute_type="WALL"), dict(batch=5), dict(t_offset=2)):
        with pytest.raises(ValueError):
            q.scalarTrace(S.stag, S.lo, q.RngField(LAT, q.RngMilc6, SEED), 0.1, 1e-12, out=None, **bad)


def test_sloppy_driver_against_fp64(S):
    """mixed-precision batches at r2req = 1e-18: against the fp64 result at r2req = 1e-24 the bound of the oracle comparison,
    loosened by the ratio of the requested residuals sqrt(1e-18 / 1e-24) = 1e3"""
    tr, est, _, _ = S.run(improved_trace=True)
    ts, es, st, _ = S.run(improved_trace=True, sloppy=1, r2req=1e-18)
    scale = np.abs(tr).max()
    dt, de = np.abs(ts - tr).max() / scale, np.abs(es - est).max() / scale
    print("sloppy=1: trace deviation %.3e, est deviation %.3e; iterations %s updates %s" % (dt, de, st["iterations"][0], st["updates"][0]))
    assert dt < TOL5 * 1e3 and de < TOL5 * 1e3 and len(st["updates"][0]) == 16
