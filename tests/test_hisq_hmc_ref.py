"""The yardstick of the HISQ HMC driver (examples/hisqhmc.py, qexhip_md_hisq_*), pinned without the product: the oracle replay of
src/examples/hisqhmc.nim (tests/hisq_replay.py).  The reference ships no golden log for this program, so the replay is held to
what a correct HMC must satisfy: its fermion force is the gradient of the fermion action it is paired with, dH falls as dt^2, the
trajectory is reversible, its energies do not depend on the solver tolerance at the level the GPU comparison works at, and the
accept/reject stream is the oracle's RngMilc6.  No GPU.  Observed figures are printed (pytest -s)."""
import numpy as np
import pytest

import hisq_replay as R

M = 0.1
GRAD_R2 = 1e-26
STEP_PAIRS = [(3, 2), (6, 4), (12, 8)]
RATIO_BAND = (3.9, 4.2)


def link_cases(lo):
    """(site, mu): a t link on the last t slice (the antiperiodic sign), a link at an odd site, a link at an even interior site"""
    last = [i for i in range(lo.vol // 2) if lo.coord(i)[3] == lo.lat[3] - 1]
    odd = lo.vol // 2 + 37
    assert sum(lo.coord(odd)) % 2 == 1 and sum(lo.coord(11)) % 2 == 0 and lo.coord(11)[3] < lo.lat[3] - 1
    return [(last[5], 3), (odd, 1), (11, 0)]


# (lattice, start, eps of the single links, eps of the global direction, global bound at eps or None for the eps^2 criterion)
GRADIENT_CASES = [([4, 4, 4, 4], "warm", 1.6e-3, 1e-5, 1e-8), ([4, 4, 4, 6], "random", 1e-4, 2e-6, None)]


@pytest.mark.parametrize("lat,start,eps1,epsg,gbound", GRADIENT_CASES)
def test_oracle_hisq_fermion_force_is_the_gradient_of_the_fermion_action(oracle, lat, start, eps1, epsg, gbound):
    """S_f(U) = 1/2 |D(-m; U)^-1 phi|^2 (fermionAction, hisqhmc.nim:431-440) against the force mdvAll pairs it with (:633-636,
    :496-545).  The pairing: the MD flow is u' = p u (updateGauge, :549-552) with K = 1/2 sum p o p over the real components of
    the anti-Hermitian p (kineticAction, :422-429).  Define F by  d/d eps S(exp(eps X) U) = sum X o F  for algebra-valued X.  Along
    the flow dS/dt = sum p o F and dK/dt = sum p o p', so H = K + S is conserved iff p' = -F.  mdvAll does  p -= dtauF f  with
    dtauF = -1/2 dt / m, i.e. p' = (1/2 / m) f: the driver conserves H iff  F = (-1/2 / m) f,  f = TAH(hisq_force(outer_1, outer_3) u^+).
    That is what is checked, by central differences of S_f itself (solves to r2req 1e-26), on a warm field and on g.random links
    (not unitary; [4,4,4,6] is the smallest shape with a t extent other than 4).

    Single links (t link on the last t slice, an odd site, an even site): the deviation at eps / 2 is below 1e-6 relative (the figure
    of test_oracle_hisq_force_is_the_gradient) and below 0.35 of the deviation at eps, so it is the eps^2 discretisation error and
    not a wrong force.  Global direction: 1e-8 at eps = 1e-5 on the warm field; on the random field the eps^2 criterion at
    eps = 2e-6.  Measured (deviation at eps -> at eps / 2):
      warm 4^4, eps 1.6e-3:        t link 2.7e-06 -> 6.8e-07,  odd 1.2e-06 -> 3.0e-07,  even 1.0e-07 -> 2.6e-08;  global 4.5e-10
      random [4,4,4,6], eps 1e-4:  t link 1.4e-06 -> 3.4e-07,  odd 2.6e-07 -> 6.6e-08,  even 1.3e-07 -> 2.8e-08
      random global, eps 2e-6:     9.6e-07 -> 2.3e-07  (at 1e-5: 2.4e-05, at 5e-6: 6.0e-06: a factor 4.00 per halving)
    On the warm field eps = 1e-4 is too small for the criterion: the discretisation error there (1e-8 .. 4e-10) has come down to
    the rounding of S_f ~ 600 (one ulp of S_f is 3e-9 of 2 eps dS on the even link) and the ratios scatter between 0.05 and 6.8.
    From 3.2e-3 down to 4e-4 every halving divides the deviation of all three links by 3.9 .. 4.1."""
    o = oracle
    lo = o.Layout(lat)
    rf = o.RngField(lo, o.RNG_MILC6, 4711)
    g = o.gauge_warm(lo, 0.3, rf) if start == "warm" else o.gauge_random(lo, rf)
    X = o.gauge_random_tah(lo, rf)
    _, su, sul = R.smear_rephase(o, lo, g)
    phi = o.D(lo, su, sul, o.vector_gaussian(lo, rf), -M)                 # the heatbath's phi, fixed under the variation
    phi[lo.vol // 2:] = 0
    F = (-0.5 / M) * R.fermion_force(o, lo, g, phi, M, GRAD_R2)

    def S(eps, Xd):
        u = g.copy()
        o.gauge_exp_update(lo, u, Xd, eps)
        return R.fermion_action(o, lo, u, phi, M, GRAD_R2)

    for i, mu in link_cases(lo):
        Xd = R.single_link(X, i, mu)
        d1, d2 = R.gradient_deviation(S, F, Xd, eps1), R.gradient_deviation(S, F, Xd, 0.5 * eps1)
        print("%s %s link (%d, %d) at %s: eps %g: %.2e -> %.2e (ratio %.3f)" % (lat, start, i, mu, lo.coord(i), eps1, d1, d2, d2 / d1))
        assert d2 < 1e-6 and d2 < 0.35 * d1, (i, mu, d1, d2)
    d1 = R.gradient_deviation(S, F, X, epsg)
    if gbound is not None:
        print("%s %s global direction: eps %g: %.2e" % (lat, start, epsg, d1))
        assert d1 < gbound, d1
    else:
        d2 = R.gradient_deviation(S, F, X, 0.5 * epsg)
        print("%s %s global direction: eps %g: %.2e -> %.2e (ratio %.3f)" % (lat, start, epsg, d1, d2, d2 / d1))
        assert d2 < 1e-6 and d2 < 0.35 * d1, (d1, d2)


def test_replay_dH_is_second_order(oracle):
    """[4,4,4,6], beta 12, m 0.1, warm(0.3), seed 123456789, tau 0.1, 2MN with (gauge, fermion) steps (3,2), (6,4), (12,8):
    dH = -0.143370506, -0.035220534, -0.008765706, ratios 4.071 and 4.018 (required: inside [3.9, 4.2]); every sector's force
    enters, so a force that is not the gradient of its action leaves a dH that does not fall with the step.  (At tau >= 0.25 these
    lattices are far outside the asymptotic regime: dH up to 1e4.)
    Reversibility (forward, p -> -p, back) at (3,2): largest link deviation measured 1.3e-15 (2.7e-15 at (12,8)); bound 1.4e-14."""
    o = oracle
    dH = [R.trajectory(*sp)["dH"] for sp in STEP_PAIRS]
    r1, r2 = dH[0] / dH[1], dH[1] / dH[2]
    print("dH %r, ratios %.4f %.4f" % (dH, r1, r2))
    assert abs(dH[0]) > 1e-3
    assert RATIO_BAND[0] <= r1 <= RATIO_BAND[1] and RATIO_BAND[0] <= r2 <= RATIO_BAND[1], (dH, r1, r2)
    a, b = R.trajectory(3, 2), R.trajectory(12, 8)
    for k in ("g_start", "p_start", "phi"):                               # the same start at every step count
        assert np.array_equal(a[k], b[k])
    assert max(abs(x - y) for x, y in zip(a["hi"], b["hi"])) <= 1e-14 * 16.0 * 384       # (the oracle's threaded sums may reorder)
    assert np.abs(a["g_evolved"] - a["g_start"]).max() > 1e-3             # it did move
    r = R.Replay(o, gsteps=3, fsteps=2)
    r.prepare()
    dev = r.reverse_check()
    print("reversibility: max link deviation %.3e" % dev)
    assert dev < 1.4e-14
    assert np.array_equal(r.g, a["g_start"]) and np.array_equal(r.p, a["p_start"])


def test_replay_follows_hisqhmc_nim(oracle):
    """what the trajectory does besides integrating: draw order (warm start, then momenta, then the pseudofermion source from ONE
    RngMilc6 field, hisqhmc.nim:469-474), phi = D(-m) psi with the odd half zeroed, the three energy terms, Metropolis with the
    first deviate of the serial stream, projectSU on ACCEPT"""
    o = oracle
    a = R.trajectory(3, 2)
    lo = o.Layout(R.LAT)
    rf = o.RngField(lo, o.RNG_MILC6, R.SEED)
    g = o.gauge_warm(lo, R.WARM, rf)
    p = o.gauge_random_tah(lo, rf)
    psi = o.vector_gaussian(lo, rf)
    assert np.array_equal(a["g_start"], g) and np.array_equal(a["p_start"], p)
    gp = g.copy()
    o.setBC(lo, gp)
    o.stagPhase(lo, gp)
    su, sul = o.hisq_smear(lo, gp)
    assert np.abs(a["phi"][lo.vol // 2:]).max() == 0
    assert np.array_equal(a["phi"][:lo.vol // 2], o.D(lo, su, sul, psi, -R.MASS)[:lo.vol // 2])
    # S_f at the start is 1/2 |psi_even|^2 up to the solve: D(-m)^-1 on the even part of D(-m) psi (hisqhmc.nim:431-440)
    x = o.solve(lo, su, sul, a["phi"], -R.MASS, 1e-28, 10000)[0]
    assert abs(a["hi"][2] - 0.5 * (x * x).sum()) < 1e-9 * a["hi"][2]
    assert abs(a["hi"][0] - (0.5 * (p * p).sum() - 16.0 * lo.vol)) < 1e-12 * 16.0 * lo.vol
    assert abs(a["hi"][1] - o.gauge_action(lo, g, 12.0, -0.6, 0)) < 1e-12 * 16.0 * lo.vol
    assert abs(a["dH"] - (sum(a["hf"]) - sum(a["hi"]))) == 0
    assert a["rnd"] == float(o.milc6_stream(R.SEED, 987654321, 1)[0][0])
    assert a["accepted"] == (a["rnd"] <= np.exp(-a["dH"])) and a["accepted"]
    gu = a["g_evolved"].copy()
    o.gauge_projectSU(lo, gu)
    assert np.array_equal(a["g_final"], gu) and np.array_equal(a["p_final"], a["p_evolved"])
    # the REJECT branch: a trajectory so coarse that exp(-dH) underflows puts the start links back
    r = R.Replay(o, gsteps=1, fsteps=1, tau=2.0)
    b = r.trajectory()
    print("tau = 2, one step each: dH %r, deviate %r" % (b["dH"], b["rnd"]))
    assert not b["accepted"] and b["dH"] > 1.0 and np.array_equal(b["g_final"], b["g_start"])


def test_serial_rng_is_the_oracles_stream(oracle):
    """SerialRng of examples/hisqhmc.py is a hand restatement of RngMilc6.seed(seed, 987654321) + uniform (hisqhmc.nim:158-161,
    341-344): bit for bit the oracle's stream"""
    ex = R.load_example()
    for seed in (123456789, 987654321987):
        s = ex.SerialRng(seed)
        got = np.array([s.uniform() for _ in range(64)])
        ref = oracle.milc6_stream(seed, 987654321, 64)[0]
        assert ref.dtype == np.float32 and len(np.unique(ref)) > 60
        assert np.array_equal(got, ref.astype(np.float64)), (seed, got[:4], ref[:4])


@pytest.mark.parametrize("steps", [(3, 2), (12, 8)])
def test_replay_does_not_move_with_tighter_solves(steps):
    """the replay at force r2req 1e-24 against 1e-28 (action solves at 1e-20 and at 1e-28): everything the GPU tests compare agrees
    ten times inside their tolerances, so those tests measure the product and not the yardstick's solver.  Measured at (3,2) and
    (12,8): energy terms <= 3.7e-12 (T, S_g; allowed 1.2e-8) and 2.3e-13 (S_f; allowed 1.2e-9), dH <= 5.5e-12 (allowed 1e-7), links
    4.4e-15 (allowed 1e-13), momenta 4.6e-14 (allowed 1e-12).  (ForceCGTol = 1e-12 of hisqhmc.nim:41 moves dH by 2.6e-7 and the
    momenta by 1e-7: the comparison runs at 1e-24.)"""
    a = R.trajectory(*steps)
    vol = 384
    for b in (R.trajectory(*steps, force_r2=1e-28), R.trajectory(*steps, force_r2=1e-28, action_r2=1e-28)):
        for k in ("hi", "hf"):
            devs = [abs(x - y) for x, y in zip(a[k], b[k])]
            print("%s %s: %r" % (steps, k, devs))
            for d, sc in zip(devs, R.energy_scales(a[k], vol)):
                assert d <= 0.1 * R.RTOL * sc, (k, devs)
        dl = np.linalg.norm(a["g_evolved"] - b["g_evolved"]) / np.linalg.norm(a["g_evolved"])
        dp = np.linalg.norm(a["p_evolved"] - b["p_evolved"]) / np.linalg.norm(a["p_evolved"])
        print("%s dH %.3e links %.3e momenta %.3e" % (steps, abs(a["dH"] - b["dH"]), dl, dp))
        assert abs(a["dH"] - b["dH"]) <= 0.1 * R.DH_TOL and dl <= 0.1 * R.LINK_TOL and dp <= 0.1 * R.MOM_TOL
        assert a["rnd"] == b["rnd"] and a["accepted"] == b["accepted"]
