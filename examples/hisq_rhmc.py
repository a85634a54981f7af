#!/usr/bin/env python
"""Rooted HISQ: rational HMC with nf = 1, 2 or 3 tastes of one HISQ staggered field and the Symanzik gauge action, every field
resident on the device.  examples/hisqhmc.py with the pseudofermion action replaced by

    S_f = 1/2 Re <phi, r_act(M^+M) phi>_even,   r_act(x) ~ x^(-nf/4),   M^+M = m^2 - D_eo D_oe on the even sites,

the rooted staggered field of src/mcmc/fields/staggeredFields.nim:58-95,191-230,356-467 restated on M^+M (DESIGN.md "Rooted HISQ":
heatbath, action and force are rational functions of the same Hermitian operator, so the force IS the gradient of the action).

    python examples/hisq_rhmc.py [-nf 2] [-nterm 12] [-fterm 8] [-lo m^2] [-hi m^2+6] [-rational FILE.json] + the options of hisqhmc.py

  heatbath  phi.even = r_hb(M^+M) eta.even, r_hb ~ x^(nf/8), phi.odd = 0          (Context.dev_rational_xx, -nterm poles)
  action    1/2 Re<phi, r_act(M^+M) phi>_even                                      (dev_rational_xx + dev_redot, -nterm poles)
  force     ResidentMD.hisq_fforce_rational with r_md ~ x^(-nf/4), t = +dtau / 2   (one multi-shift solve, -fterm poles)

The rationals are fitted at start (qex_amd.rational.rationalFit on [lo, hi]) or read from -rational FILE.json:
{"heatbath": {...}, "action": {...}, "force": {...}}, each a Rational.to_json object.  At the first prepare() 30 power iterations
of the operator estimate the largest eigenvalue of M^+M; the program stops if it is not below hi."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qex_amd as q  # noqa: E402
from qex_amd.rational import Rational, rationalFit  # noqa: E402
import hisqhmc as parent  # noqa: E402

ACTION_TOL, FORCE_TOL, MAXITS = parent.ACTION_TOL, parent.FORCE_TOL, parent.MAXITS
POWER_ITERATIONS = 30


def fit_rationals(nf, lo, hi, nterm, fterm):
    """the three rationals and their measured errors: {"heatbath" | "action" | "force": (Rational, error)}"""
    return dict(heatbath=rationalFit(nf / 8.0, lo, hi, nterm), action=rationalFit(-nf / 4.0, lo, hi, nterm),
                force=rationalFit(-nf / 4.0, lo, hi, fterm))


def load_rationals(path):
    d = json.load(open(path))
    return {k: (Rational.from_json(d[k]), None) for k in ("heatbath", "action", "force")}


class HisqRHMC(parent.HisqHMC):
    def __init__(self, lat, rationals, lo, hi, nf=2, **kw):
        if kw.get("host"):
            raise ValueError("the rooted example keeps its fields on the device (no -host)")
        super().__init__(lat, **kw)
        self.nf, self.lo_x, self.hi_x = nf, float(lo), float(hi)
        self.r_hb, self.r_act, self.r_md = (rationals[k][0] for k in ("heatbath", "action", "force"))
        self.eta, self.chi = self.psi, self.ctx.field_new()
        self.checked = False

    def spectrum_check(self):
        """30 power iterations of A = 4 M^+M on the even sites (unnormalised: 30 factors of at most ~25 stay far inside double)"""
        ctx = self.ctx
        self.prng.dev_gaussian_vector(ctx, self.eta)
        ctx.dev_zero(self.eta, "odd")
        x, y = self.eta, self.chi
        for _ in range(POWER_ITERATIONS):
            ctx.dev_op_xx(y, x, self.mass * self.mass, True)
            x, y = y, x
        ctx.dev_op_xx(y, x, self.mass * self.mass, True)
        lam = 0.25 * ctx.dev_redot(x, y, "even") / ctx.dev_norm2(x, "even")
        print("spectrum: rational range [%r, %r], largest eigenvalue of M^+M estimated at %r (%d power iterations), m^2 = %r" % (
            self.lo_x, self.hi_x, lam, POWER_ITERATIONS, self.mass * self.mass))
        if not lam < self.hi_x:
            raise SystemExit("hisq_rhmc: the spectrum of M^+M reaches %r, outside the rational range (hi = %r): raise -hi" % (lam, self.hi_x))
        if self.mass * self.mass < self.lo_x:
            raise SystemExit("hisq_rhmc: m^2 = %r is below the rational range (lo = %r): lower -lo" % (self.mass * self.mass, self.lo_x))
        self.checked = True

    def heatbath(self):
        if not self.checked:
            self.spectrum_check()
        self.prng.dev_momenta(self.ctx)
        self.prng.dev_gaussian_vector(self.ctx, self.eta)
        r = self.r_hb
        its, _ = self.ctx.dev_rational_xx(self.phi, self.eta, self.mass, r.f0, r.alpha, r.beta, ACTION_TOL, MAXITS, True)
        self.iters["action"] += its                                  # (dev_rational_xx leaves phi.odd = 0)

    def hamiltonian(self):
        vol = self.lo.vol
        kinetic = 0.5 * self.md.momentum_norm2() - 16.0 * vol
        gauge = q.gaugeAction(self.ctx, None, **self.gc)
        r = self.r_act
        its, _ = self.ctx.dev_rational_xx(self.chi, self.phi, self.mass, r.f0, r.alpha, r.beta, ACTION_TOL, MAXITS, True)
        fermion = 0.5 * self.ctx.dev_redot(self.phi, self.chi, "even")
        self.iters["action"] += its
        self.terms = (kinetic, gauge, fermion)
        print("kinetic = %r, gauge = %r, fermion = %r" % (kinetic, gauge, fermion))
        return kinetic + gauge + fermion

    def mdv_all(self, dtau):
        if dtau[0] != 0.0:
            self.md.gauge_force(**self.gc)
            self.md.kick(self.md.GAUGE, -dtau[0])
        if dtau[1] != 0.0:
            # the parent: p -= dtauF f with dtauF = -0.5 dtau / m and scale 1; here the weights alpha_k / m_k carry the 1 / m_k
            self.smear()
            r = self.r_md
            self.iters["force"] += self.md.hisq_fforce_rational(self.phi, self.mass, r.alpha, r.beta, FORCE_TOL, MAXITS, 0.5 * dtau[1])


def main():
    ap = argparse.ArgumentParser(description="rooted HISQ RHMC on libqexhip (rational functions of M^+M)")
    ap.add_argument("-lat", type=int, nargs=4, default=[8, 8, 8, 8])
    ap.add_argument("-beta", type=float, default=12.0)
    ap.add_argument("-mass", type=float, default=0.1)
    ap.add_argument("-tau", type=float, default=1.0, help="trajectory length")
    ap.add_argument("-gsteps", type=int, default=15, help="2MN steps of the gauge force")
    ap.add_argument("-fsteps", type=int, default=15, help="2MN steps of the fermion force")
    ap.add_argument("-trajs", type=int, default=1)
    ap.add_argument("-seed", type=int, default=123456789, help="seed of the parallel and of the serial RngMilc6")
    ap.add_argument("-warm", type=float, default=None, help="spread of a warm start; default: cold start")
    ap.add_argument("-host", action="store_true", help="refused: the rooted example is resident only")
    ap.add_argument("-reverse", action="store_true", help="reversibility check after the heatbath of every trajectory")
    ap.add_argument("-time", action="store_true")
    ap.add_argument("-nf", type=int, choices=[1, 2, 3], default=2, help="tastes: the action is det(M^+M)^(nf/4)")
    ap.add_argument("-nterm", type=int, default=12, help="poles of the heatbath and action rationals")
    ap.add_argument("-fterm", type=int, default=8, help="poles of the force rational")
    ap.add_argument("-lo", type=float, default=None, help="lower end of the fit range (default mass^2)")
    ap.add_argument("-hi", type=float, default=None, help="upper end of the fit range (default mass^2 + 6)")
    ap.add_argument("-rational", metavar="FILE.json", default=None, help="the three rationals instead of fitting them")
    a = ap.parse_args()
    if a.gsteps < 1 or a.fsteps < 1:
        ap.error("-gsteps and -fsteps must be >= 1")
    if a.host:
        ap.error("-host: the rooted example keeps its fields on the device")
    lo = a.mass * a.mass if a.lo is None else a.lo
    hi = a.mass * a.mass + 6.0 if a.hi is None else a.hi
    rats = load_rationals(a.rational) if a.rational else fit_rationals(a.nf, lo, hi, a.nterm, a.fterm)
    hmc = HisqRHMC(a.lat, rats, lo, hi, nf=a.nf, beta=a.beta, mass=a.mass, tau=a.tau, gsteps=a.gsteps, fsteps=a.fsteps, seed=a.seed,
                   warm=a.warm)
    print(hmc.ctx.info())
    print("trajectory length: %r\nnumber of trajectories: %d\nbeta: %r\nmass: %r\ncp: %r\ncr: %r\nboundary conditions: pppa\nnf: %d" % (
        a.tau, a.trajs, a.beta, a.mass, parent.CP, parent.CR, a.nf))
    for k in ("heatbath", "action", "force"):
        r, err = rats[k]
        print("rational %s: %d poles, f0 = %r, max relative error %s on [%r, %r]" % (
            k, r.nterm, r.f0, "%.3e" % err if err is not None else "(from file)", lo, hi))
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
