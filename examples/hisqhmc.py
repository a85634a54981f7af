#!/usr/bin/env python
"""src/examples/hisqhmc.nim -- HMC with one HISQ staggered pseudofermion field and the Symanzik (plaquette + rectangle)
gauge action -- with every field operation in libqexhip and, by default, every field resident on the device.

    python examples/hisqhmc.py [-lat 8 8 8 8] [-beta 12] [-mass 0.1] [-tau 1] [-gsteps 15] [-fsteps 15] [-trajs 1]
                               [-seed 123456789] [-warm 0.5] [-host] [-reverse] [-time]

The main program is hisqhmc.nim:613-659 with the trajectory of :416-596 (file:line in the docstrings): prepare (backup,
smearRephase, momentum and fermion heatbath, H_i), the two 2MN integrators of the gauge and the fermion force on a shared time
axis (mdevolve's ParallelEvolution, as examples/staghmc_spv.py restates it) with mdt and mdvAll, finish (smear, H_f, Metropolis
with the serial stream, reunit or revert), the plaquettes.  The parameters are the reference's defaultInputs (:54-79).

Default: links, momenta, pseudofermion, solutions and forces stay in HBM (qexhip_md_*, qexhip_md_hisq_*, qexhip_dev_*,
qexhip_rng_dev_*); between the start configuration and the last printed number only scalars and the generator states cross
PCIe.  -host drives the same trajectory through the host-pointer entry points (what a drop-in for QEX's host-resident fields
calls): the yardstick for tests/test_gpu_hisq_md.py and for the timings in profiles/hisq_md_32x4.log.
-reverse adds the reversibility check (ReversibilityCheck, :14): forward, flip the momenta, back, and the largest link deviation."""
import argparse
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import qex_amd as q  # noqa: E402

LAMBDA_2MN = 0.1931833275037836      # mdevolve's Omelyan2MN default
CP, CR = 1.0, -1.0 / 20.0            # hisqhmc.nim:47-50: eqn. (A2) of arXiv:1004.0342, u0 = 1
ACTION_TOL, FORCE_TOL, MAXITS = 1e-20, 1e-12, 10000      # :39-43


class SerialRng:
    """`self.milc.seed(self.seed, 987654321)` (hisqhmc.nim:158-161): RngMilc6, the accept/reject stream"""

    def __init__(self, seed, index=987654321):
        m = 0xFFFFFFFF
        s, self.r = seed & m, []
        for _ in range(7):
            s = ((69607 + 8 * index) * s + 12345) & m
            self.r.append((s >> 8) & 0xFFFFFF)
        self.ic = ((69607 + 8 * index) * s + 12345) & m
        self.mult = (100005 + 8 * index) & m

    def uniform(self):
        r = self.r
        t = (((r[5] >> 7) | (r[6] << 17)) ^ ((r[4] >> 1) | (r[5] << 23))) & 0xFFFFFF
        self.r = [t] + r[:6]
        self.ic = (self.ic * self.mult + 12345) & 0xFFFFFFFF
        return float(np.float32(t ^ ((self.ic >> 8) & 0xFFFFFF)) * np.float32(1.0 / 16777216.0))


class HisqHMC:
    def __init__(self, lat, beta=12.0, mass=0.1, tau=1.0, gsteps=15, fsteps=15, seed=123456789, warm=None, host=False):
        self.lat, self.beta, self.mass, self.tau, self.gsteps, self.fsteps, self.host = list(lat), beta, mass, tau, gsteps, fsteps, host
        self.lo = q.Layout(self.lat)
        self.ctx = q.Context(self.lat)
        self.md = q.ResidentMD(self.ctx)
        self.hc = q.HisqCoefs()
        self.prng = q.RngField(self.lat, q.RngMilc6, seed)
        self.srng = SerialRng(seed)
        self.gc = dict(plaq=beta * CP, rect=beta * CR)               # GaugeActionCoeffs(plaq: beta*Cp, rect: beta*Cr) (:309)
        self.iters = dict(action=0, force=0)
        g = q.unit(self.lo) if warm is None else self.prng.warm(float(warm))      # gauge-start (:326-331)
        if host:
            self.g, self.p, self.phi = g, None, None
            self.sf = self.stag = None
        else:
            self.md.begin(g, None)                                   # the links go up once; momenta are born on the device
            self.phi, self.psi = self.ctx.field_new(), self.ctx.field_new()

    # ---- smearRephase (:405-420) + stag = newStag3(su, sul) (:332) ----
    def smear(self):
        if self.host:
            gp = self.g.copy()
            q.rephase(self.lo, gp)                                   # threads: g.rephase
            self.sf = self.hc.smearGetForce(self.ctx, gp)
            self.stag = q.Staggered(self.ctx, None, smear=self.hc)
        else:
            self.md.hisq_prepare(set_links=True)

    # ---- momentumHeatbath / fermionHeatbath (:457-467) ----
    def heatbath(self):
        if self.host:
            self.p = self.prng.randomTAH()
            psi = self.prng.gaussian_vector()
            self.phi = np.zeros_like(psi)
            self.stag.D(self.phi, psi, -self.mass)                   # stag.D(phi, psi, -mass)
            self.phi[self.lo.vol // 2:] = 0                          # phi.odd := 0
        else:
            self.prng.dev_momenta(self.ctx)
            self.prng.dev_gaussian_vector(self.ctx, self.psi)
            self.ctx.dev_D(self.phi, self.psi, -self.mass)
            self.ctx.dev_zero(self.phi, "odd")

    # ---- hamiltonian (:422-455) ----
    def hamiltonian(self):
        vol = self.lo.vol
        if self.host:
            kinetic = 0.5 * float((self.p * self.p).sum()) - 16.0 * vol
            gauge = q.gaugeAction(self.ctx, self.g, **self.gc)
            psi = np.zeros_like(self.phi)
            sp = q.SolverParams(r2req=ACTION_TOL, maxits=MAXITS, verbosity=0)
            its = self.stag.solve_batch([psi], [self.phi], [-self.mass], sp)       # stag.solve(psi, phi, -mass, spa)
            fermion = 0.5 * float((psi * psi).sum())
        else:
            kinetic = 0.5 * self.md.momentum_norm2() - 16.0 * vol
            gauge = q.gaugeAction(self.ctx, None, **self.gc)
            its, _ = self.ctx.dev_solve_batch([self.psi], [self.phi], [-self.mass], ACTION_TOL, MAXITS)
            fermion = 0.5 * self.ctx.dev_norm2(self.psi)
        self.iters["action"] += its[0]
        self.terms = (kinetic, gauge, fermion)                       # what the line below prints, for callers that drive the class
        print("kinetic = %r, gauge = %r, fermion = %r" % (kinetic, gauge, fermion))
        return kinetic + gauge + fermion

    # ---- backup / revert (:476-481), reunit (:123-133) ----
    def backup(self):
        if self.host:
            self.g0 = self.g.copy()
        else:
            self.md.save_links()

    def revert(self):
        if self.host:
            self.g = self.g0
        else:
            self.md.restore_links()

    def reunit(self):
        if self.host:
            q.reunit(self.ctx, self.g)
        else:
            self.md.reunit_links()

    def prepare(self):                                               # :469-474
        self.backup()
        self.smear()
        self.heatbath()
        self.hi = self.hamiltonian()

    # ---- mdt / mdvAll (:630-636) ----
    def mdt(self, dtau):                                             # updateGauge: u := exp(dtau p) u
        if self.host:
            q.gaugeUpdate(self.ctx, self.g, self.p, dtau)
        else:
            self.md.update_links(dtau)

    def mdv_all(self, dtau):
        dtauG, dtauF = dtau[0], -0.5 * dtau[1] / self.mass
        if dtauG != 0.0:                                             # updateMomentumGauge: gc.gaugeForce(u, f); p -= dtauG f
            if self.host:
                self.p -= dtauG * q.gaugeForce(self.ctx, self.g, cplaq=self.gc["plaq"], rect=self.gc["rect"])
            else:
                self.md.gauge_force(**self.gc)
                self.md.kick(self.md.GAUGE, -dtauG)
        if dtauF != 0.0:                                             # updateMomentumFermion: smearRephase, solve, fermionForce; p -= dtauF f
            self.smear()
            if self.host:
                psi = np.zeros_like(self.phi)
                sp = q.SolverParams(r2req=FORCE_TOL, maxits=MAXITS, verbosity=0)
                its = self.stag.solve_batch([psi], [self.phi], [self.mass], sp)
                f = np.zeros_like(self.g)
                self.sf.fermionForce(f, [psi], [1.0])
                self.p -= dtauF * f
            else:
                its = self.md.hisq_fforce_solve([self.phi], [self.mass], [1.0], FORCE_TOL, MAXITS, -dtauF)
            self.iters["force"] += its[0]

    def schedule(self):
        """newParallelEvolution(gaugeIntegrator(steps = gaugeSteps, V, T), fermionIntegrator(steps = fermionSteps, Vf, T)) (:642-645)
        with both members 2MN: the V updates of the two members on the shared time axis, coincident ones in one mdvAll"""
        ev = []
        for m, n in enumerate((self.gsteps, self.fsteps)):
            dt = self.tau / n
            for s in range(n):
                ev.append(((s + LAMBDA_2MN) * dt, m, 0.5 * dt))
                ev.append(((s + 1.0 - LAMBDA_2MN) * dt, m, 0.5 * dt))
        ev.sort(key=lambda e: (e[0], e[1]))
        out = []
        for t, m, h in ev:
            if out and abs(out[-1][0] - t) < 1e-12:
                out[-1][1][m] = h
            else:
                ts = [0.0, 0.0]
                ts[m] = h
                out.append((t, ts))
        return out

    def evolve(self):                                                # integrator.evolve(tau); integrator.finish (:483-485)
        now = 0.0
        for t, ts in self.schedule():
            self.mdt(t - now)
            now = t
            self.mdv_all(ts)
        self.mdt(self.tau - now)

    def finish(self):                                                # :574-596
        self.smear()
        self.hf = self.hamiltonian()
        dH = self.hf - self.hi
        expdH = math.exp(-dH) if dH > -700.0 else float("inf")
        rnd = self.srng.uniform()
        accepted = rnd <= expdH
        if accepted:
            self.reunit()
        else:
            self.revert()
        return accepted, dH, expdH, rnd

    def plaquette(self):                                             # :618-625
        pl = q.plaq(self.ctx, self.g if self.host else None)
        ps, pt = 2.0 * sum(pl[:3]), 2.0 * sum(pl[3:])
        print("MEASplaq ss: %r  st: %r  tot: %r" % (float(ps), float(pt), float(0.5 * (ps + pt))))

    # ---- the fields of either path on the host (checks only) ----
    def links(self):
        if self.host:
            return self.g.copy()
        g = self.lo.newGauge()
        self.md.end(g, None)
        return g

    def momenta(self):
        if self.host:
            return self.p.copy()
        p = self.lo.newGauge()
        self.md.end(None, p)
        return p

    def set_fields(self, g, p):
        if self.host:
            self.g, self.p = g.copy(), p.copy()
        else:
            self.md.begin(g, p)

    def reverse_check(self):
        """forward, p -> -p, back: the largest deviation of a link element from the start (ReversibilityCheck); links and
        momenta are put back as they were"""
        g0, p0 = self.links(), self.momenta()
        self.evolve()
        self.set_fields(self.links(), -self.momenta())
        self.evolve()
        dev = float(np.abs(self.links() - g0).max())
        self.set_fields(g0, p0)
        return dev


def main():
    ap = argparse.ArgumentParser(description="HISQ HMC (src/examples/hisqhmc.nim) on libqexhip")
    ap.add_argument("-lat", type=int, nargs=4, default=[8, 8, 8, 8])
    ap.add_argument("-beta", type=float, default=12.0)
    ap.add_argument("-mass", type=float, default=0.1)
    ap.add_argument("-tau", type=float, default=1.0, help="trajectory length")
    ap.add_argument("-gsteps", type=int, default=15, help="2MN steps of the gauge force")
    ap.add_argument("-fsteps", type=int, default=15, help="2MN steps of the fermion force")
    ap.add_argument("-trajs", type=int, default=1)
    ap.add_argument("-seed", type=int, default=123456789, help="seed of the parallel and of the serial RngMilc6")
    ap.add_argument("-warm", type=float, default=None, help="spread of a warm start (the reference: 0.5); default: cold start")
    ap.add_argument("-host", action="store_true", help="every step through the host-pointer entry points (fields live on the host)")
    ap.add_argument("-reverse", action="store_true", help="reversibility check after the heatbath of every trajectory")
    ap.add_argument("-time", action="store_true")
    a = ap.parse_args()
    if a.gsteps < 1 or a.fsteps < 1:
        ap.error("-gsteps and -fsteps must be >= 1")
    hmc = HisqHMC(a.lat, beta=a.beta, mass=a.mass, tau=a.tau, gsteps=a.gsteps, fsteps=a.fsteps, seed=a.seed, warm=a.warm, host=a.host)
    print(hmc.ctx.info())
    print("trajectory length: %r\nnumber of trajectories: %d\nbeta: %r\nmass: %r\ncp: %r\ncr: %r\nboundary conditions: pppa\nfields: %s" % (
        a.tau, a.trajs, a.beta, a.mass, CP, CR, "host" if a.host else "resident"))
    for n in range(a.trajs):
        t0 = time.time()
        hmc.prepare()
        if a.reverse:
            print("REVERSE: max link deviation %r" % hmc.reverse_check())
        t1 = time.time()
        hmc.evolve()
        hmc.ctx.sync()
        t2 = time.time()
        accepted, dH, expdH, rnd = hmc.finish()
        print("%s: %r, %r, %r" % ("ACC" if accepted else "REJ", dH, expdH, rnd))
        hmc.plaquette()
        if a.time:
            hmc.ctx.sync()
            print("TIME trajectory %d: %.3f s (MD evolution %.3f s); solver iterations %r" % (n, time.time() - t0, t2 - t1, hmc.iters))


if __name__ == "__main__":
    main()
