"""Replay of the reference's HISQ HMC program src/examples/hisqhmc.nim on the oracle: one HISQ pseudofermion field, the
Symanzik gauge action (plaquette + rectangle, :47-50,309), two 2MN integrators on a shared time axis (:638-645).

This is TEST INFRASTRUCTURE, as tests/hmc_replay.py is for staghmc_sh: the driver below exists only to carry the oracle's
operators (hisq_smear, D / solve with Naik links, stag_outer, hisq_force, force_projTAH, the gauge action and force, the RngMilc6
field and serial stream) along the trajectory of hisqhmc.nim:613-659, so that examples/hisqhmc.py and the qexhip_md_hisq_* entries
have a yardstick that is not the library.  The reference ships no golden log for this program; what pins the replay itself is in
tests/test_hisq_hmc_ref.py (the fermion force is the gradient of the fermion action it is paired with, dH ~ dt^2, reversibility).
It is written from hisqhmc.nim (file:line below) and the oracle's Python entry points, not from examples/hisqhmc.py.

The integrator comes from the Nim package `mdevolve` (qex.nimble:29), which is not vendored in the reference tree, so its
schedule is restated here (`schedule`): Omelyan's second-order minimum-norm scheme with mdevolve's default lambda,
      T(lambda dt)  V(dt / 2)  T((1 - 2 lambda) dt)  V(dt / 2)  T(lambda dt)          per step of length dt = tau / steps,
and newParallelEvolution (:642-645) orders the V updates of its members on the common time axis, advancing the shared T up to each;
V updates of different members that fall on the same time (nonZeroStep 1e-12) go to ONE call of mdvAll(dtau) (:633-636).
"""
import functools
import importlib.util
import math
import os

import numpy as np

LAT = [4, 4, 4, 6]                   # 384 sites: every extent at the Naik / fat7 minimum of 4 or just above
SEED = 123456789                     # serial-seed = parallel-seed (:60-61)
SERIAL_INDEX = 987654321             # self.milc.seed(self.seed, 987654321) (:160)
BETA, MASS = 12.0, 0.1               # :65-66
CP, CR = 1.0, -1.0 / 20.0            # :47-50, eqn. (A2) of arXiv:1004.0342 at u0 = 1
TAU, WARM = 0.1, 0.3
LAMBDA = 0.1931833275037836          # mdevolve's Omelyan2MN default
ACTION_R2, FORCE_R2 = 1e-20, 1e-24   # ActionCGTol (:40); the force tolerance is tightened from ForceCGTol = 1e-12 (:41), which
MAXITS = 10000                       # moves dH by 2.6e-7 and the end momenta by 1e-7 on this trajectory: see test_hisq_hmc_ref.py
# what the product is held to against this replay (tests/test_gpu_hisq_hmc.py): energy terms at RTOL times their scale (the figure
# and the scales of tests/test_gpu_hisq_md.py), dH absolute, links and momenta in relative norm (the figures tests/test_smear.py
# holds the HISQ and nHYP force chains to)
RTOL, DH_TOL, LINK_TOL, MOM_TOL = 2e-11, 1e-6, 1e-12, 1e-11


def schedule(tau, steps):
    """[(time, [dt_member0, dt_member1, ...])]: the V updates of the 2MN members with `steps[m]` steps each, in time order"""
    ev = []
    for m, n in enumerate(steps):
        dt = tau / n
        for s in range(n):
            for frac in (LAMBDA, 1.0 - LAMBDA):
                ev.append(((s + frac) * dt, m))
    ev.sort()
    out = []
    for t, m in ev:
        if not out or t - out[-1][0] >= 1e-12:
            out.append((t, [0.0] * len(steps)))
        out[-1][1][m] += 0.5 * tau / steps[m]
    return out


def smear_rephase(o, lo, g):
    """smearRephase (:405-414): g.rephase; smearGetForce(g, su, sul); g.rephase back.  Returns (phased thin links, su, sul)."""
    gp = g.copy()
    o.rephase(lo, gp)
    su, sul = o.hisq_smear(lo, gp)
    return gp, su, sul


def fermion_action(o, lo, g, phi, mass, r2req, maxits=MAXITS):
    """fermionAction (:431-440): 1/2 |D(-m)^-1 phi|^2 on the HISQ links of g"""
    _, su, sul = smear_rephase(o, lo, g)
    psi = o.solve(lo, su, sul, phi, -mass, r2req, maxits)[0]
    return 0.5 * float((psi * psi).sum())


def outer_products(o, lo, psi):
    """fermionForce steps 1 and 2 (:504-526): f1 = psi(x) psi(x + mu)^+, f3 = psi(x) psi(x + 3 mu)^+, odd sites times -1"""
    f1, f3 = lo.new_gauge(), lo.new_gauge()
    o.stag_outer(lo, f1, psi, 1.0, -1.0, False, hop=1)
    o.stag_outer(lo, f3, psi, 1.0, -1.0, False, hop=3)
    return f1, f3


def fermion_force(o, lo, g, phi, mass, r2req, maxits=MAXITS):
    """fermionForce (:541-545 with :496-539): psi = D(+m)^-1 phi, the outer products, the HISQ chain on the phased links,
    f = TAH(ff u^+) with the phased u (the reference rephases g for steps 2-4 and back).  No step factor: mdvAll applies it."""
    gp, su, sul = smear_rephase(o, lo, g)
    psi = o.solve(lo, su, sul, phi, mass, r2req, maxits)[0]
    f1, f3 = outer_products(o, lo, psi)
    f = o.hisq_force(lo, gp, f1, f3)
    o.force_projTAH(lo, f, gp, adj=False)
    return f


class Replay:
    """One run of hisqhmc.nim's main program (:647-657) with a warm start"""

    def __init__(self, o, lat=LAT, beta=BETA, mass=MASS, tau=TAU, gsteps=3, fsteps=2, seed=SEED, warm=WARM,
                 action_r2=ACTION_R2, force_r2=FORCE_R2, maxits=MAXITS):
        self.o, self.lo = o, o.Layout(lat)
        self.beta, self.mass, self.tau, self.steps = beta, mass, tau, (gsteps, fsteps)
        self.action_r2, self.force_r2, self.maxits = action_r2, force_r2, maxits
        self.rf = o.RngField(self.lo, o.RNG_MILC6, seed)                     # newParallelRNG (:148-156)
        self.deviates = o.milc6_stream(seed, SERIAL_INDEX, 64)[0]            # newSerialRNG (:158-165), srng.uniform (:341-344)
        self.ntraj = 0
        self.g = o.gauge_warm(self.lo, warm, self.rf)                        # gauge-start, warm(u, s, prng) (:368-371)
        self.p = self.phi = self.g0 = None

    # ---- hamiltonian (:422-455) ----
    def energies(self):
        o, lo = self.o, self.lo
        kinetic = 0.5 * float((self.p * self.p).sum()) - 16.0 * lo.vol                     # kineticAction (:422-429)
        gauge = o.gauge_action(lo, self.g, self.beta * CP, self.beta * CR, 0)              # gc.gaugeAction1(u) (:446)
        fermion = fermion_action(o, lo, self.g, self.phi, self.mass, self.action_r2, self.maxits)
        return (kinetic, gauge, fermion)

    # ---- prepare (:469-474) ----
    def prepare(self):
        o, lo = self.o, self.lo
        self.g0 = self.g.copy()                                              # backup
        _, su, sul = smear_rephase(o, lo, self.g)                            # smear
        self.p = o.gauge_random_tah(lo, self.rf)                             # momentumHeatbath (:463)
        psi = o.vector_gaussian(lo, self.rf)                                 # fermionHeatbath (:464-467)
        self.phi = o.D(lo, su, sul, psi, -self.mass)                         # stag.D(phi, psi, -mass) (:459)
        self.phi[lo.vol // 2:] = 0                                           # phi.odd := 0 (:461)
        self.hi = self.energies()
        return self.hi

    # ---- mdt / mdvAll (:630-636) ----
    def mdt(self, dtau):
        self.o.gauge_exp_update(self.lo, self.g, self.p, dtau)               # updateGauge (:549-552)

    def mdv_all(self, dtau):
        o, lo = self.o, self.lo
        dtau_g, dtau_f = dtau[0], -0.5 * dtau[1] / self.mass                 # :634
        if dtau_g != 0.0:                                # updateMomentumGauge (:570-572): p -= dtauG f
            self.p -= dtau_g * o.gauge_force_general(lo, self.g, self.beta * CP, self.beta * CR, 0)
        if dtau_f != 0.0:                                # updateMomentumFermion (:566-568): p -= dtauF f
            self.p -= dtau_f * fermion_force(o, lo, self.g, self.phi, self.mass, self.force_r2, self.maxits)

    def evolve(self):                                                        # integrator.evolve(tau); integrator.finish (:483-485)
        now = 0.0
        for t, dtau in schedule(self.tau, self.steps):
            self.mdt(t - now)
            now = t
            self.mdv_all(dtau)
        self.mdt(self.tau - now)

    # ---- finish (:574-596) ----
    def finish(self):
        self.hf = self.energies()
        dH = sum(self.hf) - sum(self.hi)
        rnd = float(self.deviates[self.ntraj])
        self.ntraj += 1
        accepted = rnd <= (math.exp(-dH) if dH > -700.0 else float("inf"))
        if accepted:
            self.o.gauge_projectSU(self.lo, self.g)                          # reunit (:123-133)
        else:
            self.g = self.g0.copy()                                          # revert (:481)
        return accepted, dH, rnd

    def trajectory(self):
        """prepare, evolve, finish: everything the tests compare, as a dict"""
        hi = self.prepare()
        g_start, p_start = self.g.copy(), self.p.copy()
        self.evolve()
        g_evolved, p_evolved = self.g.copy(), self.p.copy()
        accepted, dH, rnd = self.finish()
        return dict(hi=hi, hf=self.hf, dH=dH, rnd=rnd, accepted=accepted, g_start=g_start, p_start=p_start, phi=self.phi.copy(),
                    g_evolved=g_evolved, p_evolved=p_evolved, g_final=self.g.copy(), p_final=self.p.copy())

    def reverse_check(self):
        """forward, p -> -p, back (after prepare): the largest deviation of a link element from the start; fields put back"""
        g1, p1 = self.g.copy(), self.p.copy()
        self.evolve()
        self.p = -self.p
        self.evolve()
        dev = float(np.abs(self.g - g1).max())
        self.g, self.p = g1, p1
        return dev


# ---- shared by tests/test_hisq_hmc_ref.py and tests/test_gpu_hisq_hmc.py ----
@functools.lru_cache(maxsize=None)
def trajectory(gsteps, fsteps, force_r2=FORCE_R2, action_r2=ACTION_R2):
    """one trajectory of the replay at the parameters above; computed once per session, never written"""
    from oracle import oracle as o

    o.build()
    r = Replay(o, gsteps=gsteps, fsteps=fsteps, force_r2=force_r2, action_r2=action_r2).trajectory()
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def energy_scales(ref, vol):
    """T and S_g carry the 16 V offset, S_f is relative to itself (tests/test_gpu_hisq_md.py)"""
    return [max(abs(ref[0]), 16.0 * vol), max(abs(ref[1]), 16.0 * vol), abs(ref[2])]


def load_example():
    """examples/hisqhmc.py as a module of its own (it imports without a GPU: nothing touches the device before HisqHMC is built)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("hisqhmc_example", os.path.join(root, "examples", "hisqhmc.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def gradient_deviation(S, F, X, eps):
    """| central difference of S(eps, X) along X  -  sum X o F | / | sum X o F |"""
    num, ana = (S(eps, X) - S(-eps, X)) / (2.0 * eps), float((X * F).sum())
    return abs(num - ana) / abs(ana)


def single_link(X, i, mu):
    Xd = np.zeros_like(X)
    Xd[i, mu] = X[i, mu]
    return Xd
