"""examples/hisqhmc.py and the qexhip_md_hisq_* entries under it against an outside yardstick: the oracle replay of
src/examples/hisqhmc.nim (tests/hisq_replay.py, pinned on the CPU by tests/test_hisq_hmc_ref.py), and, without the oracle, the
product's own fermion action differentiated numerically.  tests/test_gpu_hisq_md.py compares the library with itself (resident
against host pointers, fused against unfused); here a wrong sign or factor that both paths share shows.

The driver is imported in-process and run at [4,4,4,6] (384 sites, six tiles per parity, launch-bound), beta 12, m 0.1, warm(0.3),
seed 123456789, tau 0.1, with its force tolerance set to 1e-24 (RSQ of tests/hmc_replay.py): the reference's ForceCGTol = 1e-12 moves
dH by 2.6e-7 and the momenta by 1e-7 on the replay itself, far above the bounds below.  Observed figures are printed (pytest -s)."""
import functools

import numpy as np
import pytest

import hisq_replay as R

pytestmark = pytest.mark.gpu
STEP_PAIRS = [(3, 2), (6, 4), (12, 8)]
RATIO_BAND = (3.9, 4.2)
VOL = int(np.prod(R.LAT))


@functools.lru_cache(maxsize=None)
def example():
    ex = R.load_example()
    ex.FORCE_TOL = R.FORCE_R2
    return ex


def new_driver(host, gsteps, fsteps):
    return example().HisqHMC(R.LAT, beta=R.BETA, mass=R.MASS, tau=R.TAU, gsteps=gsteps, fsteps=fsteps, seed=R.SEED, warm=R.WARM, host=host)


@functools.lru_cache(maxsize=None)
def driven(host, gsteps, fsteps):
    """one trajectory of the example, computed once per session, never written"""
    h = new_driver(host, gsteps, fsteps)
    h.prepare()
    r = dict(hi=h.terms, g_start=h.links(), p_start=h.momenta())
    assert sum(h.terms) == h.hi
    h.evolve()
    r.update(g_evolved=h.links(), p_evolved=h.momenta())
    accepted, dH, _, rnd = h.finish()
    assert sum(h.terms) == h.hf
    r.update(hf=h.terms, dH=dH, rnd=rnd, accepted=accepted, iters=dict(h.iters))
    h.ctx.close()
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def relnorm(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("steps", [(3, 2), (12, 8)])
@pytest.mark.parametrize("host", [False, True], ids=["resident", "host"])
def test_trajectory_against_the_oracle_replay(oracle, host, steps):
    """H_i and H_f term by term at RTOL = 2e-11 of their scale (T, S_g: max(|x|, 16 V); S_f: itself), dH at 1e-6 absolute, links
    at 1e-12 and momenta at 1e-11 in relative norm after evolve, the deviate exactly, the verdict.
    Observed (one MI355X), resident and host alike, (3,2) and (12,8): start links 2.1e-16 of the oracle's warm start, momenta
    identical; energy terms <= 4.7e-16 of their scale; dH off the replay's by 5.5e-12 and 7.3e-12; links after evolve 3.6e-16 and
    5.9e-16, momenta 2.8e-16 and 3.6e-16; deviate 0.3787543773651123, ACC.  (101 action and 243 / 973 force iterations.)"""
    ref, got = R.trajectory(*steps), driven(host, *steps)
    name = "%s %s" % ("host" if host else "resident", steps)
    print("%s: start links %.2e momenta %.2e; solver iterations %r" % (name, relnorm(got["g_start"], ref["g_start"]),
                                                                      relnorm(got["p_start"], ref["p_start"]), got["iters"]))
    worst = 0.0
    for k in ("hi", "hf"):
        devs = [abs(x - y) / sc for x, y, sc in zip(got[k], ref[k], R.energy_scales(ref[k], VOL))]
        print("%s: %s %r  (T, S_g, S_f relative deviations %s)" % (name, k, got[k], " ".join("%.2e" % d for d in devs)))
        worst = max(worst, max(devs))
    dl, dp = relnorm(got["g_evolved"], ref["g_evolved"]), relnorm(got["p_evolved"], ref["p_evolved"])
    print("%s: dH %r (replay %r, deviation %.2e); links %.2e momenta %.2e; deviate %r %s" % (
        name, got["dH"], ref["dH"], abs(got["dH"] - ref["dH"]), dl, dp, got["rnd"], "ACC" if got["accepted"] else "REJ"))
    assert worst <= R.RTOL
    assert abs(got["dH"] - ref["dH"]) <= R.DH_TOL
    assert dl <= R.LINK_TOL and dp <= R.MOM_TOL
    assert got["rnd"] == ref["rnd"] and got["accepted"] == ref["accepted"]
    assert np.abs(ref["g_evolved"] - ref["g_start"]).max() > 1e-3            # it did move


def test_dH_is_second_order_on_the_device(oracle):
    """resident path, (gauge, fermion) steps (3,2), (6,4), (12,8): each dH within 1e-6 of the replay's, both ratios inside
    [3.9, 4.2] (the replay: 4.071, 4.018).
    Observed: dH -0.143370505999, -0.035220534010, -0.008765706285 (the replay's to 7.3e-12), ratios 4.0707 and 4.0180."""
    dH = [driven(False, *sp)["dH"] for sp in STEP_PAIRS]
    ref = [R.trajectory(*sp)["dH"] for sp in STEP_PAIRS]
    r1, r2 = dH[0] / dH[1], dH[1] / dH[2]
    print("dH %r, replay %r, ratios %.4f %.4f" % (dH, ref, r1, r2))
    for x, y in zip(dH, ref):
        assert abs(x - y) <= R.DH_TOL
    assert abs(dH[0]) > 1e-3
    assert RATIO_BAND[0] <= r1 <= RATIO_BAND[1] and RATIO_BAND[0] <= r2 <= RATIO_BAND[1], (dH, r1, r2)


@pytest.mark.parametrize("host", [False, True], ids=["resident", "host"])
def test_finish_reunitarises_or_reverts(oracle, host):
    """finish with the verdict forced by the deviate it is handed.  REJ: the links are the backed-up ones bit for bit.  ACC: they
    are gauge_projectSU of the evolved links at 1e-14 (the figure of test_gpu_md_building_blocks for reunit), and on the resident
    path the next smear builds the operator of THOSE links: one dev_D against the oracle's D on hisq_smear of the phased
    reunitarised field at 1e-12.
    The evolved links are unitary to rounding, so ACC is run a second time with the links drifted off the group by 1e-9, where a
    missing reunit shows: 1e-14 in relative norm, and the operator must then be the one of the reunitarised, not of the drifted links.
    Observed, both paths: reunit against gauge_projectSU 1.1e-15 (max element; the projection moves the evolved links by as much);
    drifted links 4.2e-16 (moved by 1.0e-9); the operator after finish 8.3e-16 from the oracle's on the reunitarised links, which
    is 3.2e-10 from the one on the drifted links."""
    o = oracle
    lo = o.Layout(R.LAT)
    ref = R.trajectory(3, 2)
    name = "host" if host else "resident"
    for deviate, verdict in ((2.0, False), (0.0, True)):
        h = new_driver(host, 3, 2)
        h.prepare()
        g0 = h.links()
        h.evolve()
        g1, p1 = h.links(), h.momenta()
        assert relnorm(g1, ref["g_evolved"]) <= R.LINK_TOL
        h.srng.uniform = lambda d=deviate: d
        accepted, dH, _, rnd = h.finish()
        assert accepted == verdict and rnd == deviate and abs(dH - ref["dH"]) <= R.DH_TOL
        g2 = h.links()
        if not verdict:
            assert np.array_equal(g2, g0) and not np.array_equal(g1, g0)
        else:
            want = g1.copy()
            o.gauge_projectSU(lo, want)
            dev = float(np.abs(g2 - want).max())
            print("%s ACC: reunit against gauge_projectSU %.2e (it moved the links by %.2e)" % (name, dev, np.abs(g2 - g1).max()))
            assert dev < 1e-14
            # the evolved links are unitary to rounding, so the above cannot tell a reunit from none: the same end with the links
            # drifted off the group by 1e-9 (as test_gpu_md_building_blocks drifts them), same figure in the same norm
            gd = g1 * (1.0 + 1e-9)
            h.set_fields(gd, p1)
            assert h.finish()[0]
            g3, want = h.links(), gd.copy()
            o.gauge_projectSU(lo, want)
            print("%s ACC, drifted links: reunit against gauge_projectSU %.2e (it moved them by %.2e)" % (name, relnorm(g3, want), relnorm(gd, want)))
            assert relnorm(g3, want) < 1e-14 and relnorm(gd, want) > 1e-10
            if not host:
                h.smear()
                x = o.vector_gaussian(lo, o.RngField(lo, o.RNG_MILC6, 99))
                xi, ri = h.ctx.field_new(np.ascontiguousarray(x)), h.ctx.field_new()
                h.ctx.dev_D(ri, xi, 0.2)
                Dx, Dref, Dd = h.ctx.field_download(ri), hisq_D(o, lo, want, x), hisq_D(o, lo, gd, x)
                print("resident ACC: operator after finish against the oracle's on the reunitarised links %.2e (on the drifted links: %.2e)" % (
                    relnorm(Dx, Dref), relnorm(Dd, Dref)))
                assert relnorm(Dx, Dref) < 1e-12 and relnorm(Dd, Dref) > 1e-10
        h.ctx.close()


def hisq_D(o, lo, g, x, m=0.2):
    _, su, sul = R.smear_rephase(o, lo, g)
    return o.D(lo, su, sul, x, m)


def random_tah(rng, shape):
    """traceless anti-Hermitian 3 x 3 matrices as [..., 3, 3, 2]"""
    a = rng.standard_normal(shape + (3, 3)) + 1j * rng.standard_normal(shape + (3, 3))
    x = 0.5 * (a - np.conj(np.swapaxes(a, -1, -2)))
    x -= np.trace(x, axis1=-2, axis2=-1)[..., None, None] * np.eye(3) / 3.0
    return np.stack([x.real, x.imag], axis=-1)


def exp_update(g, X, eps):
    """exp(eps X) g in numpy (Taylor series: |eps X| < 0.01, twelve terms are exact in double)"""
    u, x = g[..., 0] + 1j * g[..., 1], eps * (X[..., 0] + 1j * X[..., 1])
    term, acc = u.copy(), u.copy()
    for k in range(1, 13):
        term = np.einsum("...ij,...jk->...ik", x, term) / k
        acc += term
    return np.ascontiguousarray(np.stack([acc.real, acc.imag], axis=-1))


def test_product_force_is_the_gradient_of_the_product_action():
    """The only check here that does not pass through the oracle: S_f = 1/2 |D(-m)^-1 phi|^2 from dev_solve_batch(-m) and dev_norm2
    on the links exp(+-eps X) U (numpy, uploaded with md.begin, smeared by hisq_prepare) against sum X o f (-1/2 / m) with f =
    md.hisq_force() after hisq_fforce_solve, on the driver's warm [4,4,4,6] field with the driver's phi.  It closes the case of
    oracle and product being wrong alike in the action.  Criteria and step sizes of
    test_oracle_hisq_fermion_force_is_the_gradient_of_the_fermion_action (warm field): a t link on the last t slice, deviation at
    eps / 2 = 8e-4 below 1e-6 and below 0.35 of the one at 1.6e-3; a global direction at eps = 1e-5 below 1e-8.
    Observed: t link 6.7e-07 -> 1.7e-07 (ratio 0.250); global direction 4.7e-10; the force solve takes 66 iterations."""
    import qex_amd as q

    h = new_driver(False, 3, 2)
    h.prepare()
    ctx, md, m = h.ctx, h.md, R.MASS
    lo = q.Layout(R.LAT)
    g = h.links()
    its = md.hisq_fforce_solve([h.phi], [m], [1.0], 1e-26, R.MAXITS, 0.0)
    F = (-0.5 / m) * md.hisq_force()
    psi = ctx.field_new()

    def S(eps, X):
        md.begin(exp_update(g, X, eps), None)
        md.hisq_prepare(set_links=True)
        ctx.dev_solve_batch([psi], [h.phi], [-m], 1e-26, R.MAXITS)
        return 0.5 * ctx.dev_norm2(psi)

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
