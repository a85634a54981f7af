"""The connected scalar correlator on the GPU (csrc/conn.hip, qex_amd/conn4d.py; src/observables/conn4d.nim).

The kernels are pinned against the numpy restatement tests/conn4d_ref.py on identical uploaded fields (bit for bit where the values
are exact), the whole measurement against the oracle's CG within a bound derived from the requested residual.  Measured deviations
are printed (pytest -s)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import conn4d_ref as R  # noqa: E402
import qex_amd as q  # noqa: E402
from oracle import oracle as o  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 987654321
EPS = np.finfo(np.float64).eps
LATS = [[4, 4, 4, 8], [4, 6, 10, 6]]      # 4.6.10.6: 720 sites per parity (partial tile), 60-site slices (partial 256-site chunk)


def _points(lat):
    """zero, even, odd-sum (parity flip), and a wrap in each of the four directions"""
    far = [v - 1 for v in lat]
    return [[0, 0, 0, 0], [2, 0, 2, 4], [1, 2, 0, 2], [far[0], 0, 0, 0], [0, far[1], 0, 0], [0, 0, far[2], 0], [0, 0, 0, far[3]], far]


@pytest.mark.parametrize("lat", LATS)
def test_point_sources_are_the_numpy_ones(lat):
    lo = q.Layout(lat)
    ctx = q.Context(lat)
    noise = np.random.default_rng(sum(lat)).standard_normal((lo.vol, 3, 2))
    ids = [ctx.field_new(noise) for _ in range(4)]           # not zero beforehand: every site must be written
    far = [v - 1 for v in lat]
    odd = [1, 2, 0, 2]
    pts, ic = [[0, 0, 0, 0], far, odd, odd], [0, 2, 1, 2]
    ctx.dev_point_source(ids, pts, ic)
    for k in range(4):
        got = ctx.field_download(ids[k])
        assert np.array_equal(got, R.point_source(lo.coords, pts[k], ic[k])), k
        assert not np.signbit(got).any() and got.sum() == 1.0
    # one and three in a call, other fields untouched
    ctx.dev_point_source(ids[1:2], [odd], [0])
    assert np.array_equal(ctx.field_download(ids[1]), R.point_source(lo.coords, odd, 0))
    assert np.array_equal(ctx.field_download(ids[0]), R.point_source(lo.coords, pts[0], 0))
    ctx.dev_point_source(ids[1:], [far, far, [0, 0, 0, 0]], [0, 1, 2])
    for k, (p, c) in enumerate(((far, 0), (far, 1), ([0, 0, 0, 0], 2))):
        assert np.array_equal(ctx.field_download(ids[1 + k]), R.point_source(lo.coords, p, c))
    ctx.close()


@pytest.mark.parametrize("lat", LATS)
def test_accumulate_exact_values(lat):
    """components that are multiples of 1/8 in [-2, 2] and scal = 1/16: every product and sum is exact, so the device equals numpy
    bit for bit whatever the order"""
    lo = q.Layout(lat)
    ctx = q.Context(lat)
    rng = np.random.default_rng(sum(lat) + 1)
    pts = _points(lat)
    F = [rng.integers(-16, 17, size=(lo.vol, 3, 2)) / 8.0 for _ in pts]
    ids = [ctx.field_new(f) for f in F]
    pre = rng.integers(-16, 17, size=(lo.vol, 2)) / 8.0
    # a cfield holding `pre` in both components (there is no cfield upload): <a, b> with a = (1, 0, 0) and b = (pre, 0, 0), exactly
    a = np.zeros((lo.vol, 3, 2))
    b = np.zeros((lo.vol, 3, 2))
    a[:, 0, 0] = 1.0
    b[:, 0, :] = pre
    ia, ib = ctx.field_new(a), ctx.field_new(b)
    sizes = set()
    for groups in ([1, 2, 3, 2], [4, 4], [3, 1, 4]):
        tr = ctx.cfield_new()
        ctx.dev_trace_accum(tr, [ia], [ib], 1.0)
        assert np.array_equal(ctx.cfield_download(tr), pre)
        ref = pre[:, 0].copy()
        k0 = 0
        for n in groups:
            ctx.dev_conn_accum(tr, ids[k0:k0 + n], pts[k0:k0 + n], 1.0 / 16.0)
            for k in range(k0, k0 + n):
                R.conn_accum(ref, F[k], lo.coords, lat, pts[k], 1.0 / 16.0)
            got = ctx.cfield_download(tr)
            assert np.array_equal(got[:, 0], ref), (groups, k0, n)
            assert np.array_equal(got[:, 1], pre[:, 1]), (groups, k0, n)          # the imaginary part is not touched
            sizes.add(n)
            k0 += n
        ctx.cfield_free(tr)
    assert sizes == {1, 2, 3, 4}
    # every point on its own, so a wrong wrap in one direction cannot hide behind another
    for k, pt in enumerate(pts):
        tr = ctx.cfield_new()
        ctx.dev_conn_accum(tr, [ids[k]], [pt], 1.0 / 16.0)
        got = ctx.cfield_download(tr)
        assert np.array_equal(got[:, 0], R.translate(R.site_norm2(F[k]) / 16.0, lo.coords, lat, pt)), pt
        assert not got[:, 1].any()
        ctx.cfield_free(tr)
    ctx.close()


@pytest.mark.parametrize("lat", LATS)
def test_accumulate_random_values(lat):
    """deviation from numpy at most 8 eps sum_k scal |phi_k|^2 per site: gamma_6 of the six-term sum of squares, the product and
    the add; four systems in one call are four calls bit for bit"""
    lo = q.Layout(lat)
    ctx = q.Context(lat)
    rng = np.random.default_rng(sum(lat) + 2)
    pts = _points(lat)[1:5]
    F = [rng.standard_normal((lo.vol, 3, 2)) for _ in pts]
    ids = [ctx.field_new(f) for f in F]
    scal = 1.0 / 3.0
    tr, tr1 = ctx.cfield_new(), ctx.cfield_new()
    ref, bound = np.zeros(lo.vol), np.zeros(lo.vol)
    for n in (4, 3, 1):                      # on top of what is there
        ctx.dev_conn_accum(tr, ids[:n], pts[:n], scal)
        for k in range(n):
            R.conn_accum(ref, F[k], lo.coords, lat, pts[k], scal)
            bound += R.translate(scal * R.site_norm2(F[k]), lo.coords, lat, pts[k])
        got = ctx.cfield_download(tr)
        dev = np.abs(got[:, 0] - ref)
        print("lat %s n=%d: max deviation / bound %.3f" % (lat, n, (dev / (8 * EPS * bound)).max()))
        assert (dev <= 8 * EPS * bound).all() and not got[:, 1].any()
    for n in (4, 3, 1):
        for k in range(n):
            ctx.dev_conn_accum(tr1, [ids[k]], [pts[k]], scal)
    assert np.array_equal(ctx.cfield_download(tr1), got)
    ctx.cfield_zero(tr1)
    ctx.dev_conn_accum(tr1, ids[:2], pts[:2], scal)
    ctx.dev_conn_accum(tr1, ids[2:], pts[2:], scal)
    ctx.cfield_zero(tr)
    ctx.dev_conn_accum(tr, ids, pts, scal)
    assert np.array_equal(ctx.cfield_download(tr1), ctx.cfield_download(tr))
    ctx.close()


@pytest.mark.parametrize("lat", LATS)
def test_sign_and_slices(lat):
    lo = q.Layout(lat)
    ctx = q.Context(lat)
    rng = np.random.default_rng(sum(lat) + 3)
    A, B = rng.standard_normal((lo.vol, 3, 2)), rng.standard_normal((lo.vol, 3, 2))
    tr = ctx.cfield_new()
    ctx.dev_trace_accum(tr, [ctx.field_new(A)], [ctx.field_new(B)], 1.0)
    before = ctx.cfield_download(tr)
    assert before[:, 1].any()
    ctx.cfield_stag_sign(tr)
    signed = ctx.cfield_download(tr)
    assert np.array_equal(signed, R.stag_sign(before, lo.coords)) and not np.array_equal(signed, before)
    nt, per = lat[3], lo.vol // lat[3]
    sl = ctx.dev_cfield_slices(tr)
    want = R.slice_sums(signed[:, 0], lo.coords, nt)
    tol = np.zeros(nt)
    np.add.at(tol, lo.coords[:, 3], np.abs(signed[:, 0]))
    tol *= EPS * per                                    # the summation bound of the scalar-trace test's slice sums
    print("lat %s slices of the signed field: max deviation / bound %.3g" % (lat, (np.abs(sl[:, 0] - want) / tol).max()))
    assert (np.abs(sl[:, 0] - want) <= tol).all()
    ctx.cfield_stag_sign(tr)
    assert np.array_equal(ctx.cfield_download(tr), before)                 # twice: the identity
    ctx.close()


def test_one_rank_with_ghost_zones_is_one_rank_without():
    """ghost zones forced on one rank: the fields carry ghost tiles, the kernels take the same path and give the same bits"""
    lat = [8, 8, 6, 8]
    lo = q.Layout(lat)
    rng = np.random.default_rng(11)
    pts = [[0, 0, 0, 0], [7, 7, 5, 7], [1, 2, 3, 3], [2, 4, 0, 4]]
    F = [rng.standard_normal((lo.vol, 3, 2)) for _ in pts]
    out = []
    for halo in (False, True):
        ctx = q.Context(lat)
        if halo:
            ctx.force_halo()
        ids = [ctx.field_new(f) for f in F]
        src = [ctx.field_new(F[0]) for _ in pts]
        tr = ctx.cfield_new()
        ctx.dev_conn_accum(tr, ids, pts, 0.25)
        ctx.cfield_stag_sign(tr)
        ctx.dev_point_source(src, pts, [0, 1, 2, 0])
        out.append((ctx.cfield_download(tr), [ctx.field_download(s) for s in src]))
        ctx.close()
    assert np.array_equal(out[0][0], out[1][0])
    want = np.zeros(lo.vol)
    for f, p in zip(F, pts):
        R.conn_accum(want, f, lo.coords, lat, p, 0.25)
    assert np.abs(out[0][0][:, 0] - R.stag_sign(want, lo.coords)).max() <= 8 * EPS * np.abs(want).max()
    for k, (a, b) in enumerate(zip(out[0][1], out[1][1])):
        assert np.array_equal(a, b) and np.array_equal(a, R.point_source(lo.coords, pts[k], [0, 1, 2, 0][k]))


def test_refusals_leave_the_fields_alone():
    lat = [4, 4, 4, 8]
    lo = q.Layout(lat)
    ctx = q.Context(lat)
    rng = np.random.default_rng(7)
    A, B = rng.standard_normal((lo.vol, 3, 2)), rng.standard_normal((lo.vol, 3, 2))
    a, b = ctx.field_new(A), ctx.field_new(B)
    tr = ctx.cfield_new()
    ctx.dev_trace_accum(tr, [a], [b], 1.0)
    t0 = ctx.cfield_download(tr)
    z = [0, 0, 0, 0]
    E = q.QexHipError
    with pytest.raises(E, match="n = 5"):
        ctx.dev_point_source([a] * 5, [z] * 5, [0] * 5)
    with pytest.raises(E, match="n = 0"):
        ctx.dev_point_source([], [], [])
    with pytest.raises(E, match="unknown field"):
        ctx.dev_point_source([a, 999], [z, z], [0, 0])
    with pytest.raises(E, match="same field"):
        ctx.dev_point_source([a, b, a], [z, z, z], [0, 1, 2])
    with pytest.raises(E, match=r"pts\[1\]\[3\] = 8"):
        ctx.dev_point_source([a, b], [z, [0, 0, 0, 8]], [0, 0])
    with pytest.raises(E, match=r"pts\[0\]\[0\] = -1"):
        ctx.dev_point_source([a], [[-1, 0, 0, 0]], [0])
    with pytest.raises(E, match=r"pts\[0\]\[1\] = 4"):
        ctx.dev_point_source([a], [[0, 4, 0, 0]], [0])
    with pytest.raises(E, match=r"ic\[0\] = 3"):
        ctx.dev_point_source([a], [z], [3])
    with pytest.raises(E, match=r"ic\[1\] = -1"):
        ctx.dev_point_source([a, b], [z, z], [0, -1])
    with pytest.raises(E, match="n = 5"):
        ctx.dev_conn_accum(tr, [a] * 5, [z] * 5, 1.0)
    with pytest.raises(E, match="n = 0"):
        ctx.dev_conn_accum(tr, [], [], 1.0)
    with pytest.raises(E, match="unknown field"):
        ctx.dev_conn_accum(tr, [a, 999], [z, z], 1.0)
    with pytest.raises(E, match="unknown cfield"):
        ctx.dev_conn_accum(tr + 7, [a], [z], 1.0)
    with pytest.raises(E, match=r"pts\[1\]\[3\] = 8"):
        ctx.dev_conn_accum(tr, [a, b], [z, [0, 0, 0, 8]], 1.0)
    with pytest.raises(E, match=r"pts\[0\]\[2\] = 4"):
        ctx.dev_conn_accum(tr, [a], [[0, 0, 4, 0]], 1.0)
    with pytest.raises(E, match="unknown cfield"):
        ctx.cfield_stag_sign(tr + 7)
    with pytest.raises(E, match="unknown cfield"):
        ctx.cfield_stag_sign(0)
    with pytest.raises(ValueError):
        ctx.dev_point_source([a], [z, z], [0])
    with pytest.raises(ValueError):
        ctx.dev_conn_accum(tr, [a], [[0, 0, 0]], 1.0)
    assert np.array_equal(ctx.field_download(a), A) and np.array_equal(ctx.field_download(b), B)
    assert np.array_equal(ctx.cfield_download(tr), t0)
    ctx.close()


# ---- the whole measurement on 4.4.4.8 ----
LAT = [4, 4, 4, 8]
MASS, R2REQ = 0.1, 1e-20
PTS = [[0, 0, 0, 0], [2, 0, 2, 6], [1, 2, 0, 4]]       # the origin, one that wraps in t, one with an odd coordinate


class _Setup:
    def __init__(self):
        self.lo, self.olo = q.Layout(LAT), o.Layout(LAT)
        self.g = o.gauge_warm(self.olo, 0.5, o.RngField(self.olo, o.RNG_MILC6, SEED))
        o.rephase(self.olo, self.g)
        self.ctx = q.Context(LAT)
        self.stag = q.newStag(self.ctx, self.g)
        its = []

        def solve(b):
            x, it, _ = o.solve(self.olo, self.g, None, b, MASS, R2REQ, 100000)
            its.append(it)
            return x

        self.locmes, self.est, phis = R.conn_meson(solve, self.lo.coords, LAT, PTS)
        print("oracle: %d solves, iterations %d..%d" % (len(its), min(its), max(its)))
        # two solutions with |b - (D+m)x|^2 <= r2req |b|^2, |b| = 1, differ by at most eps = 2 sqrt(r2req) / m in norm (|(D+m)^-1| <= 1/m),
        # so per site |d locmes| <= sum_systems scal (2 max|phi| eps + eps^2), |phi| the norm of the colour vector of a site
        eps = 2.0 * np.sqrt(R2REQ) / MASS
        self.bound = sum((1.0 / len(PTS)) * (2.0 * np.sqrt(R.site_norm2(p).max()) * eps + eps * eps) for p in phis)
        self._runs = {}

    def run(self, **kw):
        key = tuple(sorted(kw.items()))
        if key not in self._runs:
            lines = []
            self._runs[key] = q.connMeson(self.stag, self.lo, PTS, MASS, R2REQ, out=lines.append, **kw) + (lines,)
        return self._runs[key]


@pytest.fixture(scope="module")
def S():
    s = _Setup()
    yield s
    s.ctx.close()


def test_conn_meson_against_the_oracle(S):
    loc, est, st, lines = S.run()
    dl = np.abs(loc - S.locmes).max()
    de = np.abs(est - S.est).max()
    per = S.lo.vol // LAT[3]
    print("fp64 batch=4: locmes deviation %.3e (bound %.3e, max|locmes| %.3e), est deviation %.3e; iterations %s" %
          (dl, S.bound, np.abs(S.locmes).max(), de, st["iterations"]))
    assert loc.shape == (S.lo.vol,) and est.shape == (LAT[3],) and len(st["iterations"]) == 9 and st["updates"] == [0] * 9
    assert dl <= S.bound and de <= per * S.bound
    assert [ln for ln in lines if ln.startswith("Color")] == ["Color %d" % c for _ in PTS for c in range(3)]
    assert len([ln for ln in lines if ln.startswith("norm2: ")]) == 9
    # the sign is on: sites with odd x0+x1+x2 are <= 0, the others >= 0, and est is the slice sum of the signed field
    odd = ((S.lo.coords[:, 0] + S.lo.coords[:, 1] + S.lo.coords[:, 2]) & 1).astype(bool)
    assert (loc[odd] <= 0).all() and (loc[~odd] >= 0).all() and (loc[odd] < 0).any()
    assert np.abs(est - R.slice_sums(loc, S.lo.coords, LAT[3])).max() <= EPS * per * np.abs(loc).sum()


def test_conn_meson_does_not_depend_on_the_batch(S):
    """the fp64 lock-step batch is its single solves bit for bit, and the accumulation adds system after system"""
    l4, e4, s4, _ = S.run()
    for batch in (1, 3):
        lb, eb, sb, _ = S.run(batch=batch)
        print("batch=%d iterations %s (batch=4: %s)" % (batch, sb["iterations"], s4["iterations"]))
        assert sb["iterations"] == s4["iterations"]
        assert np.array_equal(lb, l4) and np.array_equal(eb, e4), batch


@pytest.mark.parametrize("sloppy", [1, 2])
def test_conn_meson_sloppy(S, sloppy):
    if sloppy == 2:
        S.ctx.set_option("half_batch", 1)
    try:
        loc, est, st, _ = S.run(sloppy=sloppy)
        last = S.ctx.sloppy_last_batch()
    finally:
        if sloppy == 2:
            S.ctx.set_option("half_batch", 0)
    dl, de = np.abs(loc - S.locmes).max(), np.abs(est - S.est).max()
    print("sloppy=%d: locmes deviation %.3e (bound %.3e), est deviation %.3e; iterations %s updates %s; last batch %s" %
          (sloppy, dl, S.bound, de, st["iterations"], st["updates"], last))
    if sloppy == 2:
        assert last and all(r["precision"] == 2 and r["half_iters"] > 0 for r in last)           # the 16-bit path ran
    assert len(st["updates"]) == 9 and min(st["updates"]) > 0
    assert dl <= S.bound and de <= (S.lo.vol // LAT[3]) * S.bound


def test_example_program(S, tmp_path):
    """examples/conn4d.py end to end on the unit gauge: its table is the slice sums of the field it wrote, the record carries the
    reference's metadata, explicit -sources reproduce a connMeson call, and the random points are the seed's"""
    import subprocess

    fn = str(tmp_path / "scprop.out")
    cmd = [sys.executable, os.path.join(ROOT, "examples", "conn4d.py"), "-lat", "4", "4", "4", "8", "-outfn", fn, "-cg_prec", "1e-10",
           "-sloppy", "0", "-seed", "11", "-num_source", "2"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.splitlines()
    want = []
    Rg = q.GlobalRng(11)
    for _ in range(2):
        q.randomPoint(Rg, LAT, want, q.defaultSqMinDistance(LAT, 2))
    assert [ln for ln in lines if ln.startswith("point source")] == ["point source %d, living at %s." % (i, pt) for i, pt in enumerate(want)]
    assert any(ln.startswith("unitary deviation avg: ") for ln in lines) and any(ln.startswith("new unitary deviation avg: ") for ln in lines)
    assert sum(ln.startswith("plaq ss: ") for ln in lines) == 2 and lines.count("Color 2") == 2
    table = [ln.split() for ln in lines if len(ln.split()) == 2 and ln.split()[0].isdigit()][-LAT[3]:]
    est = np.array([float(v) for _, v in table])
    assert [int(t) for t, _ in table] == list(range(LAT[3]))
    f, _ = q.readField(fn, LAT, ())
    assert q.fileMetadata(fn)[1] == "l4.t8.m0.1"
    per = S.lo.vol // LAT[3]
    print("example: est %s" % est)
    assert np.abs(est - R.slice_sums(f, S.lo.coords, LAT[3])).max() <= EPS * per * np.abs(f).sum() and np.abs(est).max() > 0
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "conn4d.py"), "-sources", "1", "2", "3"], capture_output=True, text=True)
    assert p.returncode != 0 and "sources should be an integer array" in p.stderr


def test_conn_meson_arguments(S):
    for bad in (dict(batch=5), dict(batch=0), dict(t_offset=2)):
        with pytest.raises(ValueError):
            q.connMeson(S.stag, S.lo, PTS, MASS, 1e-12, out=None, **bad)
    with pytest.raises(ValueError):
        q.connMeson(S.stag, q.Layout([4, 4, 4, 4]), PTS, MASS, 1e-12, out=None)
    with pytest.raises(ValueError):
        q.connMeson(S.stag, S.lo, [], MASS, 1e-12, out=None)
    with pytest.raises(q.QexHipError, match=r"pts\[0\]\[3\] = 8"):
        q.connMeson(S.stag, S.lo, [[0, 0, 0, 8]], MASS, 1e-12, out=None)
    loc, est, st = q.connMeson(S.stag, S.lo, PTS[:1], MASS, 1e-12, out=None, batch=2)
    assert len(st["iterations"]) == 3
