"""Rooted HISQ on the device: the accumulating multi-shift solve (qexhip_dev_rational_xx / qexhip_stag_rational_xx), the rational
force (qexhip_md_hisq_fforce_rational) and examples/hisq_rhmc.py.

    r(x) = f0 + sum_k alpha_k / (x + beta_k) of M^+M = m^2 - D_eo D_oe = A(m) / 4 on one parity.

Yardsticks: the existing multi-shift solve with the mapped shifts (history bit for bit; the sum f0 b + sum 4 alpha_k x_k formed in
numpy), tests/rational_ref.py (binary128 solves on the oracle), the lock-step batch force, and the action differentiated
numerically.  Shapes: [4,4,4,6] warm HISQ Naik (six tiles per parity) and [4,6,10,6] random one-hop links (11.25 tiles: ragged
last tile), both parities.  Observed figures are printed (pytest -s).

The terms are the first nterm of one shuffled list of 32 (so that the sort is exercised and rationals share reference solves);
beta spans [0.003, 60], alpha has both signs, m = 0.3."""
import ctypes as C
import functools

import numpy as np
import pytest

import hisq_replay as R
import rational_ref as RR

pytestmark = pytest.mark.gpu
SEED = 987654321
MASS = 0.3
MAXITS = 5000
SHAPES = {"hisq": [4, 4, 4, 6], "random": [4, 6, 10, 6]}
NTERMS = [1, 2, 5, 32]
F0 = 0.37
_perm = np.random.default_rng(5).permutation(32)
BETA = np.geomspace(0.003, 60.0, 32)[_perm]
ALPHA = (np.linspace(0.2, 1.7, 32) * np.where(np.arange(32) % 7 == 3, -1.0, 1.0))[_perm]
ERR_ARG = -1


class Case:
    def __init__(self, kind):
        import qex_amd as q
        from oracle import oracle as o

        o.build()
        self.o, self.kind, self.lat = o, kind, SHAPES[kind]
        self.lo = lo = o.Layout(self.lat)
        rf = o.RngField(lo, o.RNG_MILC6, SEED)
        if kind == "hisq":
            g = o.gauge_warm(lo, 0.3, rf)
            o.rephase(lo, g)
            self.fat, self.lng = o.hisq_smear(lo, g)
        else:
            self.fat, self.lng = o.gauge_random(lo, rf), None
            o.rephase(lo, self.fat)
        self.b = o.vector_gaussian(lo, rf)
        for a in (self.fat, self.lng, self.b):
            if a is not None:
                a.setflags(write=False)
        self.h = lo.vol // 2
        self.ctx = q.Context(self.lat)
        self.s = q.newStag3(self.ctx, self.fat, self.lng) if self.lng is not None else q.newStag(self.ctx, self.fat)
        self.bid = self.ctx.field_new(np.ascontiguousarray(self.b))
        self.out = self.ctx.field_new()
        self.xs = [self.ctx.field_new() for _ in range(32)]

    def half(self, par_even):
        return slice(0, self.h) if par_even else slice(self.h, 2 * self.h)


@functools.lru_cache(maxsize=None)
def case(kind):
    return Case(kind)


def existing_path(K, bid, b, f0, alpha, beta, r2req, maxits, par_even, histcap=0):
    """f0 b + sum_k 4 alpha_k x_k with x_k from dev_solve_xx_multi at the mapped shifts, summed in numpy in the caller's order"""
    order, sh = RR.mapped_shifts(MASS, alpha, beta)
    n = len(alpha)
    its, hist = K.ctx.dev_solve_xx_multi(K.xs[:n], bid, sh, r2req, maxits, par_even, histcap=histcap)
    sl = K.half(par_even)
    S = np.zeros_like(b)
    S[sl] = f0 * b[sl]
    for j, k in enumerate(order):
        S[sl] += 4.0 * alpha[k] * K.ctx.field_download(K.xs[j])[sl]
    return S, its, hist


@functools.lru_cache(maxsize=None)
def both(kind, par_even, nterm, r2req, maxits=MAXITS):
    """(new sum, iterations, history) and the same of the existing path; computed once, never written"""
    K = case(kind)
    al, be = ALPHA[:nterm], BETA[:nterm]
    K.ctx.field_upload(K.out, np.full_like(K.b, 7.0))           # the other parity has to be zeroed by the call
    its, hist = K.ctx.dev_rational_xx(K.out, K.bid, MASS, F0, al, be, r2req, maxits, par_even, histcap=maxits + 1)
    new = K.ctx.field_download(K.out)
    old, its0, hist0 = existing_path(K, K.bid, K.b, F0, al, be, r2req, maxits, par_even, histcap=maxits + 1)
    for a in (new, old, hist, hist0):
        a.setflags(write=False)
    return dict(new=new, its=its, hist=hist, old=old, its0=its0, hist0=hist0)


@functools.lru_cache(maxsize=None)
def reference(kind, par_even, nterm):
    K = case(kind)
    ref = RR.rational_ref(K.o, K.lo, K.fat, K.lng, K.b, MASS, F0, ALPHA[:nterm], BETA[:nterm], par_even)
    ref.setflags(write=False)
    return ref


def truncated_reference(K, b, f0, alpha, beta, maxits, par_even):
    """the oracle's fp64 multi-shift CG stopped at the same count, summed in long double: what a truncated solve is compared with
    (a converged reference is O(1) away from both paths there and would show nothing)"""
    order, sh = RR.mapped_shifts(MASS, alpha, beta)
    xs, its, _ = K.o.solveXX_multi(K.lo, K.fat, K.lng, b, sh, 0.0, maxits, par_even)
    sl = K.half(par_even)
    acc = np.zeros(b.shape, dtype=np.longdouble)
    acc[sl] = np.longdouble(f0) * b[sl]
    for j, k in enumerate(order):
        acc[sl] += np.longdouble(4.0 * alpha[k]) * xs[j][sl]
    return np.asarray(acc, dtype=np.float64), its


def relation(tag, new, old, ref):
    """the new sum is never further from the reference than 4 x the existing path's, plus 1e-15 relative: both are fp64 sums of the
    same terms in a different order"""
    nr = np.linalg.norm(ref)
    dn, do = np.linalg.norm(new - ref), np.linalg.norm(old - ref)
    print("%s: |new - ref| %.3e, |existing - ref| %.3e, |new - existing| %.3e, all / |ref|" % (tag, dn / nr, do / nr, np.linalg.norm(new - old) / nr))
    assert dn <= 4.0 * do + 1e-15 * nr, (tag, dn / nr, do / nr)


PARAMS = [(k, p, n) for k in SHAPES for p in (True, False) for n in NTERMS]
IDS = ["%s-%s-%d" % (k, "even" if p else "odd", n) for k, p, n in PARAMS]


@pytest.mark.parametrize("kind,par_even,nterm", PARAMS, ids=IDS)
def test_history_is_the_multishift_history_bit_for_bit(kind, par_even, nterm):
    for r2req in (1e-12, 1e-24):
        r = both(kind, par_even, nterm, r2req)
        print("%s %s nterm %d r2req %g: %d iterations (existing %d)" % (kind, par_even, nterm, r2req, r["its"], r["its0"]))
        assert r["its"] == r["its0"] and r["its"] > 0
        assert r["hist"].size == r["its"] + 1 and np.array_equal(r["hist"], r["hist0"])


@pytest.mark.parametrize("kind,par_even,nterm", PARAMS, ids=IDS)
def test_sum_against_the_binary128_reference(kind, par_even, nterm):
    """r2req 1e-12: within 1e-6 of the reference (the figure of test_multishift); r2req 1e-24: the relation to the existing path.
    Observed (one MI355X): r2req 1e-12: 7.5e-09 .. 5.2e-07; r2req 1e-24: new and existing path both 1.1e-14 .. 6.1e-13 from the
    reference (equal to three digits in every case) and 5.1e-17 .. 2.0e-15 from each other."""
    K = case(kind)
    ref = reference(kind, par_even, nterm)
    sl, other = K.half(par_even), K.half(not par_even)
    r = both(kind, par_even, nterm, 1e-12)
    dev = np.linalg.norm(r["new"][sl] - ref[sl]) / np.linalg.norm(ref[sl])
    print("%s %s nterm %d r2req 1e-12: |S - ref| / |ref| = %.3e" % (kind, par_even, nterm, dev))
    assert dev < 1e-6
    assert not r["new"][other].any()
    r = both(kind, par_even, nterm, 1e-24)
    assert not r["new"][other].any()
    relation("%s %s nterm %d r2req 1e-24" % (kind, par_even, nterm), r["new"], r["old"], ref)


@pytest.mark.parametrize("kind,par_even", [(k, p) for k in SHAPES for p in (True, False)])
def test_stopped_at_three_iterations(kind, par_even):
    """maxits = 3: the loop condition turns false with an update pending, which has to run once more.  Against the converged
    binary128 reference both paths are 0.24 .. 0.56 away (it shows nothing but is the relation as stated); against the oracle's fp64
    multi-shift CG stopped at 3 they are <= 4.8e-16 away and 6.2e-17 .. 1.5e-16 from each other (observed, one MI355X)."""
    K = case(kind)
    for nterm in (2, 5):
        r = both(kind, par_even, nterm, 1e-24, 3)
        assert r["its"] == 3 == r["its0"] and np.array_equal(r["hist"], r["hist0"])
        assert not r["new"][K.half(not par_even)].any()
        tag = "%s %s nterm %d maxits 3" % (kind, par_even, nterm)
        relation(tag + " (binary128, converged)", r["new"], r["old"], reference(kind, par_even, nterm))
        tref, tits = truncated_reference(K, K.b, F0, ALPHA[:nterm], BETA[:nterm], 3, par_even)
        assert tits == 3
        relation(tag + " (oracle stopped at 3)", r["new"], r["old"], tref)
        # and it did take the third update: stopped at 2 it is a different vector
        r2 = both(kind, par_even, nterm, 1e-24, 2)
        assert np.linalg.norm(r["new"] - r2["new"]) > 1e-3 * np.linalg.norm(r["new"])


@pytest.mark.parametrize("kind,par_even", [(k, p) for k in SHAPES for p in (True, False)])
def test_no_iteration_and_zero_source(kind, par_even):
    K = case(kind)
    ctx, sl = K.ctx, K.half(par_even)
    want = np.zeros_like(K.b)
    want[sl] = F0 * K.b[sl]
    for nterm in (1, 5):
        ctx.field_upload(K.out, np.full_like(K.b, 7.0))
        its, hist = ctx.dev_rational_xx(K.out, K.bid, MASS, F0, ALPHA[:nterm], BETA[:nterm], 1.0, MAXITS, par_even, histcap=4)
        assert its == 0 and np.array_equal(hist, [1.0])
        assert np.array_equal(ctx.field_download(K.out), want)
        zid = ctx.field_new()
        ctx.field_upload(K.out, np.full_like(K.b, 7.0))
        its, _ = ctx.dev_rational_xx(K.out, zid, MASS, F0, ALPHA[:nterm], BETA[:nterm], 1e-12, MAXITS, par_even)
        assert its == 0 and not ctx.field_download(K.out).any()
        ctx.field_free(zid)


def test_zero_and_repeated_poles_and_the_host_entry():
    """beta = 0 and a repeated beta are legal (the repeated pole is a second copy of the base system); the host-pointer twin
    returns the bits of the resident entry"""
    import qex_amd as q

    K = case("hisq")
    al, be = [0.5, 0.25, 0.8, 0.25], [0.4, 0.0, 0.4, 0.0]
    K.ctx.dev_rational_xx(K.out, K.bid, MASS, F0, al, be, 1e-24, MAXITS, True)
    new = K.ctx.field_download(K.out)
    merged = RR.rational_ref(K.o, K.lo, K.fat, K.lng, K.b, MASS, F0, [1.3, 0.5], [0.4, 0.0], True)
    old, _, _ = existing_path(K, K.bid, K.b, F0, np.array(al), np.array(be), 1e-24, MAXITS, True)
    relation("repeated and zero poles", new, old, merged)
    out = np.full_like(K.b, 7.0)
    sp = q.SolverParams(r2req=1e-24, maxits=MAXITS, verbosity=0)
    K.s.rationalXX(out, K.b, MASS, (F0, al, be), sp, parEven=True, histcap=MAXITS)
    assert np.array_equal(out, new) and sp.iterations > 10 and sp.r2hist.size == sp.iterations + 1


def test_grid_stride_second_trip():
    """[24,24,24,28], unit links: 193,536 sites per parity = 580,608 double2, more than the 2048 x 256 a pass of the grid covers.
    nterm 3, maxits 4, against the oracle's fp64 multi-shift CG stopped at 4 (binary128 is out of reach at this size).
    Observed: new 1.2e-16 / 1.4e-16 (even / odd), existing path 1.2e-16 / 1.4e-16, 1.2e-16 from each other."""
    import qex_amd as q
    from oracle import oracle as o

    class Big:
        pass

    K = Big()
    K.o, K.lat = o, [24, 24, 24, 28]
    K.lo = lo = o.Layout(K.lat)
    K.fat, K.lng = o.gauge_unit(lo), None
    o.rephase(lo, K.fat)
    K.b = o.vector_gaussian(lo, o.RngField(lo, o.RNG_MILC6, SEED))
    K.h = lo.vol // 2
    K.half = lambda pe: slice(0, K.h) if pe else slice(K.h, 2 * K.h)
    assert K.h * 3 > 2048 * 256
    K.ctx = q.Context(K.lat)
    q.newStag(K.ctx, K.fat)
    bid, out = K.ctx.field_new(np.ascontiguousarray(K.b)), K.ctx.field_new()
    K.xs = [K.ctx.field_new() for _ in range(3)]
    al, be = ALPHA[:3], BETA[:3]
    for par_even in (True, False):
        K.ctx.field_upload(out, np.full_like(K.b, 7.0))
        its, hist = K.ctx.dev_rational_xx(out, bid, MASS, F0, al, be, 1e-30, 4, par_even, histcap=8)
        new = K.ctx.field_download(out)
        old, its0, hist0 = existing_path(K, bid, K.b, F0, al, be, 1e-30, 4, par_even, histcap=8)
        assert its == 4 == its0 and np.array_equal(hist, hist0)
        assert not new[K.half(not par_even)].any()
        tref, tits = truncated_reference(K, K.b, F0, al, be, 4, par_even)
        assert tits == 4
        relation("24^3 x 28 %s" % ("even" if par_even else "odd"), new, old, tref)
    K.ctx.close()


def test_argument_errors_leave_the_output_alone():
    import qex_amd as q

    K = case("hisq")
    L, h = q.lib(), K.ctx._h
    mark = np.full_like(K.b, 3.0)
    K.ctx.field_upload(K.out, mark)
    d = lambda v: (C.c_double * len(v))(*v)
    its = C.c_int(-5)

    def call(out_id, b_id, mass, f0, nterm, alpha, beta):
        return L.qexhip_dev_rational_xx(h, out_id, b_id, mass, f0, nterm, alpha, beta, 1e-12, 100, 1, C.byref(its), None, 0)

    a2, b2 = d([0.5, 0.7]), d([0.1, 0.2])
    big = d([1.0] * 40)
    bad = [("nterm 0", call(K.out, K.bid, MASS, F0, 0, a2, b2)),
           ("nterm 33", call(K.out, K.bid, MASS, F0, 33, big, big)),
           ("m^2 + beta_min = 0", call(K.out, K.bid, MASS, F0, 2, a2, d([-MASS * MASS, 0.2]))),
           ("m^2 + beta_min < 0", call(K.out, K.bid, MASS, F0, 2, a2, d([0.2, -1.0]))),
           ("alpha nan", call(K.out, K.bid, MASS, F0, 2, d([0.5, float("nan")]), b2)),
           ("beta inf", call(K.out, K.bid, MASS, F0, 2, a2, d([0.1, float("inf")]))),
           ("f0 inf", call(K.out, K.bid, MASS, float("inf"), 2, a2, b2)),
           ("mass nan", call(K.out, K.bid, float("nan"), F0, 2, a2, b2)),
           ("out is b", call(K.bid, K.bid, MASS, F0, 2, a2, b2)),
           ("unknown out", call(987654, K.bid, MASS, F0, 2, a2, b2)),
           ("unknown b", call(K.out, 987654, MASS, F0, 2, a2, b2)),
           ("alpha NULL", call(K.out, K.bid, MASS, F0, 2, None, b2)),
           ("beta NULL", call(K.out, K.bid, MASS, F0, 2, a2, None))]
    for name, rc in bad:
        assert rc == ERR_ARG, (name, rc)
    assert its.value == -5
    assert np.array_equal(K.ctx.field_download(K.out), mark)
    assert np.array_equal(K.ctx.field_download(K.bid), K.b)
    # the host twin refuses the same before it stages anything
    out = mark.copy()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.qexhip_stag_rational_xx(h, p(out), p(K.b), MASS, F0, 0, a2, b2, 1e-12, 100, 1, None, None, 0) == ERR_ARG
    assert L.qexhip_stag_rational_xx(h, p(out), p(K.b), MASS, F0, 2, a2, d([0.2, -1.0]), 1e-12, 100, 1, None, None, 0) == ERR_ARG
    assert np.array_equal(out, mark)
    with pytest.raises(q.QexHipError):
        K.ctx.dev_rational_xx(K.out, K.bid, MASS, F0, [1.0], [-1.0], 1e-12, 100)


# ---- the force ----
FORCE_SHAPES = [([4, 4, 4, 6], "warm"), ([4, 6, 10, 6], "random")]
T = -0.37
FORCE_R2 = 1e-28
RTOL = 2e-11          # tests/test_gpu_hisq_md.py: two paths of one trajectory


@functools.lru_cache(maxsize=None)
def md_fields(lat, start):
    import qex_amd as q

    rng = q.RngField(list(lat), q.RngMilc6, 4711)
    g = rng.warm(0.3) if start == "warm" else rng.random()
    p = rng.randomTAH()
    phi = rng.gaussian_vector()
    phi[phi.shape[0] // 2:] = 0
    for a in (g, p, phi):
        a.setflags(write=False)
    return g, p, phi


def relnorm(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("lat,start", FORCE_SHAPES)
def test_rational_force_is_the_batch_force(lat, start):
    """one multi-shift solve + reconstruction against nterm full solves of hisq_fforce_solve at the masses m_k, weights alpha_k / m_k:
    force and kicked momenta at 2e-11; one pole at beta = 0: m f is the force of hisq_fforce_solve([phi], [m], [1]).
    Observed: force 9.7e-16 .. 1.3e-14, momenta 6.0e-17 .. 1.2e-14, one pole 1.0e-15 / 1.1e-14; sloppy = 1 at 1e-20: 5.6e-11 / 8.2e-11."""
    import qex_amd as q

    g, p, phi = md_fields(tuple(lat), start)
    ctx = q.Context(list(lat))
    md = q.ResidentMD(ctx)
    md.begin(g.copy(), p.copy())
    md.hisq_prepare(set_links=True)
    phis = [ctx.field_new(np.ascontiguousarray(phi)) for _ in range(5)]
    al_all, be_all = [0.3, -0.5, 0.9, 1.7, 0.6], [0.15, 0.02, 4.0, 0.9, 0.0]

    def run(rational, al, be):
        md.begin(None, p.copy())
        mk = [float(np.sqrt(MASS * MASS + b)) for b in be]
        if rational:
            its = md.hisq_fforce_rational(phis[0], MASS, al, be, FORCE_R2, MAXITS, T)
        else:
            its = md.hisq_fforce_solve(phis[:len(al)], mk, [a / m for a, m in zip(al, mk)], FORCE_R2, MAXITS, T)
        p1 = np.zeros_like(p)
        md.end(None, p1)
        return md.hisq_force(), p1, its

    for n in (1, 3, 5):
        f1, p1, i1 = run(True, al_all[:n], be_all[:n])
        f0, p0, i0 = run(False, al_all[:n], be_all[:n])
        print("%s %s nterm %d: force %.2e momenta %.2e (iterations %r, batch %r)" % (lat, start, n, relnorm(f1, f0), relnorm(p1, p0), i1, i0))
        assert relnorm(f1, f0) <= RTOL and relnorm(p1, p0) <= RTOL
        assert not np.array_equal(p0, p) and np.abs(f0).max() > 1e-3
    f1, p1, _ = run(True, [1.0], [0.0])
    md.begin(None, p.copy())
    md.hisq_fforce_solve(phis[:1], [MASS], [1.0], FORCE_R2, MAXITS, T)
    f0 = md.hisq_force()
    print("%s %s one pole at 0: m f against the plain force %.2e" % (lat, start, relnorm(MASS * f1, f0)))
    assert relnorm(MASS * f1, f0) <= RTOL
    # sloppy = 1 goes through the mixed-precision multi-shift solve: the same force at that solve's tolerance.  Every shift's true
    # residual is <= 1e-10 |b| there, a solution error of at most 1e-10 x cond(A(m_0)) ~ 1e-10 x 60 relative; the force is bilinear in
    # the solutions: 2 x 6e-9, held to 1e-8
    md.begin(None, p.copy())
    md.hisq_fforce_rational(phis[0], MASS, al_all[:3], be_all[:3], 1e-20, MAXITS, T, sloppy=1)
    fs = md.hisq_force()
    f3 = run(True, al_all[:3], be_all[:3])[0]
    print("%s %s sloppy = 1: %.2e" % (lat, start, relnorm(fs, f3)))
    assert relnorm(fs, f3) <= 1e-8
    # refusals before any launch: the momenta stay
    md.begin(None, p.copy())
    L = q.lib()
    d = lambda v: (C.c_double * len(v))(*v)
    assert L.qexhip_md_hisq_fforce_rational(ctx._h, phis[0], MASS, 0, d([1.0]), d([0.1]), 1e-12, 100, 0, T, None) == ERR_ARG
    assert L.qexhip_md_hisq_fforce_rational(ctx._h, phis[0], MASS, 1, d([1.0]), d([-1.0]), 1e-12, 100, 0, T, None) == ERR_ARG
    assert L.qexhip_md_hisq_fforce_rational(ctx._h, 987654, MASS, 1, d([1.0]), d([0.1]), 1e-12, 100, 0, T, None) == ERR_ARG
    assert L.qexhip_md_hisq_fforce_rational(ctx._h, phis[0], MASS, 1, d([1.0]), d([0.1]), 1e-12, 100, 3, T, None) == ERR_ARG
    p2 = np.zeros_like(p)
    md.end(None, p2)
    assert np.array_equal(p2, p)
    ctx.close()


def test_state_errors_of_the_force():
    import qex_amd as q

    ctx = q.Context([4, 4, 4, 6])
    phi = ctx.field_new()
    d = lambda v: (C.c_double * len(v))(*v)
    rc = q.lib().qexhip_md_hisq_fforce_rational(ctx._h, phi, MASS, 1, d([1.0]), d([0.1]), 1e-12, 100, 0, T, None)
    assert rc == -3, rc
    ctx.close()


def test_rational_force_is_the_gradient_of_the_rational_action():
    """S_f(U) = 1/2 Re<phi, r(M^+M) phi>_even from dev_rational_xx + dev_redot on the links exp(+-eps X) U against -1/2 sum X o f
    with f from hisq_fforce_rational: field, phi, directions, step sizes and criteria of
    tests/test_gpu_hisq_hmc.py::test_product_force_is_the_gradient_of_the_product_action.
    Observed: t link 6.59e-07 -> 1.65e-07 (ratio 0.250); global direction 4.47e-10; the force solve takes 63 iterations."""
    from test_gpu_hisq_hmc import VOL, exp_update, new_driver, random_tah
    import qex_amd as q

    f0, al, be = 0.2, [0.3, 0.5, 0.9, 1.7], [0.02, 0.15, 0.9, 4.0]
    h = new_driver(False, 3, 2)
    h.prepare()
    ctx, md, m = h.ctx, h.md, R.MASS
    lo = q.Layout(R.LAT)
    g = h.links()
    its = md.hisq_fforce_rational(h.phi, m, al, be, 1e-26, R.MAXITS, 0.0)
    F = -0.5 * md.hisq_force()
    chi = ctx.field_new()

    def S(eps, X):
        md.begin(exp_update(g, X, eps), None)
        md.hisq_prepare(set_links=True)
        ctx.dev_rational_xx(chi, h.phi, m, f0, al, be, 1e-26, R.MAXITS, True)
        return 0.5 * ctx.dev_redot(h.phi, chi, "even")

    X = random_tah(np.random.default_rng(7), (VOL, 4))
    last = [i for i in range(VOL // 2) if lo.coord(i)[3] == R.LAT[3] - 1]
    Xd = R.single_link(X, last[5], 3)
    d1, d2 = R.gradient_deviation(S, F, Xd, 1.6e-3), R.gradient_deviation(S, F, Xd, 8e-4)
    dg = R.gradient_deviation(S, F, X, 1e-5)
    print("force solve %r iterations; t link at %s: eps 1.6e-3: %.2e -> %.2e (ratio %.3f); global direction, eps 1e-5: %.2e" % (
        its, lo.coord(last[5]), d1, d2, d2 / d1, dg))
    assert d2 < 1e-6 and d2 < 0.35 * d1, (d1, d2)
    assert dg < 1e-8, dg
    ctx.close()


# ---- the example ----
STEP_PAIRS = [(3, 2), (6, 4), (12, 8)]


@functools.lru_cache(maxsize=None)
def rhmc_example():
    import importlib.util
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("hisq_rhmc_example", os.path.join(root, "examples", "hisq_rhmc.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.FORCE_TOL = R.FORCE_R2
    return mod


@functools.lru_cache(maxsize=None)
def rhmc_rationals():
    lo, hi = R.MASS ** 2, R.MASS ** 2 + 6.0
    return rhmc_example().fit_rationals(2, lo, hi, 12, 8), lo, hi


def new_rhmc(gsteps, fsteps):
    rats, lo, hi = rhmc_rationals()
    return rhmc_example().HisqRHMC(R.LAT, rats, lo, hi, nf=2, beta=R.BETA, mass=R.MASS, tau=R.TAU, gsteps=gsteps, fsteps=fsteps,
                                   seed=R.SEED, warm=R.WARM)


def test_example_dH_is_second_order_and_a_rejection_restores_the_links():
    """-lat 4 4 4 6 -warm 0.3 -nf 2 (beta 12, m 0.1, tau 0.1, seed 123456789) at (gauge, fermion) steps (3,2), (6,4), (12,8): |dH| of
    the coarsest above 1e-4, both ratios in [3.6, 4.5]; a rejected trajectory puts the saved links back bit for bit.
    Observed: dH -0.135002892914, -0.033217716096, -0.008281610584; ratios 4.0642 and 4.0110."""
    dH = []
    for sp in STEP_PAIRS:
        h = new_rhmc(*sp)
        h.prepare()
        g0 = h.links()
        h.evolve()
        g1 = h.links()
        if sp == STEP_PAIRS[0]:
            h.srng.uniform = lambda: 2.0
        accepted, d, _, rnd = h.finish()
        dH.append(d)
        if sp == STEP_PAIRS[0]:
            assert not accepted and rnd == 2.0
            assert np.array_equal(h.links(), g0) and not np.array_equal(g1, g0)
        print("steps %r: H_i terms -> dH %r, iterations %r" % (sp, d, h.iters))
        h.ctx.close()
    r1, r2 = dH[0] / dH[1], dH[1] / dH[2]
    print("dH %r, ratios %.4f %.4f" % (dH, r1, r2))
    assert abs(dH[0]) > 1e-4
    assert 3.6 <= r1 <= 4.5 and 3.6 <= r2 <= 4.5, (dH, r1, r2)
