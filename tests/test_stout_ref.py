"""tests/stout_ref.py, the numpy restatement of src/gauge/stoutsmear.nim, checks itself (no GPU) by replaying the reference's two CI
tests with their own pass criteria -- tests/base/tstoutderiv.nim (the force chain against the numerical derivative of the smeared
action, one to three levels, and the smearTest0 intermediate) and tests/base/tstoutinverse.nim -- plus single-matrix checks of
expDeriv.  Configuration: g.random (RngMilc6, seed 17^7, 8^4) followed by ten in-place stout steps.  The iteration count measured
here is what tests/test_gpu_stout.py holds the device to (+-1)."""
import numpy as np
import pytest

import stout_ref as R
from oracle import oracle as o

LAT = [8, 8, 8, 8]


@pytest.fixture(scope="module")
def lo(oracle):
    return o.Layout(LAT)


@pytest.fixture(scope="module")
def gderiv(lo):
    """tstoutderiv.nim:19-23: ss = newStoutSmear(0.1), g.random, ten ss.smear(g, g)"""
    return R.reference_config(lo, 0.1)


@pytest.fixture(scope="module")
def directions(lo):
    """tstoutderiv.nim:33,63: five p.randomTAH r from newRNGField(MRG32k3a, 4321), drawn in sequence"""
    rf = o.RngField(lo, o.RNG_MRG32K3A, 4321)
    return [o.gauge_random_tah(lo, rf) for _ in range(5)]


def replay(lo, g, directions, action, force, label):
    """the `test` template (tstoutderiv.nim:53-86) with its three criteria"""
    f = force(g)
    fails = []
    for n, p in enumerate(directions):
        d, e = R.ndiff(lambda x: action(R.addnoise(lo, x, p, g)), 0.0, 1.0)
        pf = R.redot(p, f)
        err = abs(pf - d)
        etol = max(2e-8, 32 * e)
        print("%s test %d: p.f %.12g ndiff %.12g delta %.3g err(ndiff) %.3g" % (label, n, pf, d, pf - d, e))
        if not (err < etol and err < 1e-5 and abs(err / pf) < 1e-7):
            fails.append((n, pf, d, e))
    assert not fails, fails


def test_exp_is_the_oracles_exp():
    rng = np.random.default_rng(3)
    for nrm in (0.1, 1.0, 3.0):
        m = R.tah(rng.standard_normal((3, 3)) + 1j * rng.standard_normal((3, 3)))
        m *= nrm / np.sqrt((abs(m) ** 2).sum())
        assert abs(R.cm(o.su3_fn("qo_exp", R.rm(m))) - R.exp(m)).max() < 1e-14 * max(1.0, nrm)


@pytest.mark.parametrize("nrm", [0.1, 1.0, 3.0])
def test_exp_deriv_against_central_differences(nrm):
    """Re tr(expDeriv(m, w)^+ d) = d/dh Re tr(w^+ exp(m + h d)) at h = 0, for anti-Hermitian m of norm `nrm` and generic w, d:
    fourth-order central differences with h = 1e-3 (truncation ~h^4 = 1e-12, rounding ~1e-16 / h = 1e-13), held to 1e-7
    relative -- the figure test_oracle_nhyp_force_is_the_gradient uses for projectUderiv"""
    rng = np.random.default_rng(int(10 * nrm))
    rnd = lambda: rng.standard_normal((3, 3)) + 1j * rng.standard_normal((3, 3))
    m = R.tah(rnd())
    m *= nrm / np.sqrt((abs(m) ** 2).sum())
    w = rnd()
    D = R.exp_deriv(m, w)
    S = lambda mm: np.trace(R.adj(w) @ R.exp(mm)).real
    h = 1e-3
    for _ in range(6):
        d = rnd()
        num = (-S(m + 2 * h * d) + 8 * S(m + h * d) - 8 * S(m - h * d) + S(m - 2 * h * d)) / (12 * h)
        ana = np.trace(R.adj(D) @ d).real
        assert abs(num - ana) < 1e-7 * abs(num), (nrm, num, ana)


def test_alpha_zero_is_the_identity_and_its_deriv_returns_the_chain(lo, gderiv):
    ss = R.StoutSmear(lo, 0.0)
    fl = ss.smear(gderiv)
    assert np.array_equal(fl, gderiv)
    rf = o.RngField(lo, o.RNG_MILC6, 99)
    chain = o.gauge_random_tah(lo, rf) + 0.3 * o.gauge_random(lo, rf)
    d = ss.smear_deriv(chain)
    assert np.array_equal(d, chain)


def test_tstoutderiv_plain_action(lo, gderiv, directions):
    """tstoutderiv.nim:88: test(gc.gaugeAction1, gc.gaugeForce) -- the differentiator and the conventions, without smearing"""
    act = lambda g: o.gauge_action(lo, g, 6.0)
    frc = lambda g: R.contract_project_tah(lo, g, o.gauge_deriv(lo, g, 6.0))
    replay(lo, gderiv, directions, act, frc, "plain")


def test_tstoutderiv_smear_test0(lo, gderiv, directions):
    """tstoutderiv.nim:119-131: expDeriv + gaugeForceDeriv without the outer factor gf"""
    def act(g):
        return o.gauge_action(lo, R.smear_test0(lo, R.StoutSmear(lo, 0.1), g), 6.0)

    def frc(g):
        ss = R.StoutSmear(lo, 0.1)
        sg = R.smear_test0(lo, ss, g)
        return R.contract_project_tah(lo, g, R.smear_test0_deriv(lo, ss, o.gauge_deriv(lo, sg, 6.0)))

    replay(lo, gderiv, directions, act, frc, "test0")


@pytest.mark.parametrize("alphas", [(0.1,), (0.1, 0.09), (0.1, 0.09, 0.12)], ids=["1level", "2levels", "3levels"])
def test_tstoutderiv_smeared_force(lo, gderiv, directions, alphas):
    """tstoutderiv.nim:133-195"""
    replay(lo, gderiv, directions, lambda g: R.chain_action(lo, alphas, g), lambda g: R.chain_force(lo, alphas, g), "%d-level" % len(alphas))


def test_tstoutinverse(lo):
    """tstoutinverse.nim:22-58: del2 = sum |u g^+ - 1|^2 / (2 10 4 V) <= 1e-24"""
    g = R.reference_config(lo, 0.02)
    ss = R.StoutSmear(lo, 0.02)
    f = ss.smear(g)
    u, it, r2, inc = ss.inverse(f)
    d2 = R.del2(lo, u, g)
    print("inverse iter %d r2 %.3g del2 %.3g increased at %s" % (it, r2, d2, inc))
    assert d2 <= 1e-24
    assert it == R.INVERSE_ITERS and r2 < 1e-24


def test_inverse_diverges_at_a_large_step(lo):
    g = R.reference_config(lo, 0.02)
    ss = R.StoutSmear(lo, R.DIVERGING_ALPHA)
    f = ss.smear(g)
    _, it, r2, inc = ss.inverse(f, max_iter=5)
    print("alpha %g: iter %d r2 %.3g increased at %s" % (R.DIVERGING_ALPHA, it, r2, inc))
    assert it == 5 and inc
