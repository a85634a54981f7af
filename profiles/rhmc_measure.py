#!/usr/bin/env python
"""Timings of the rooted HISQ path (profiles/rhmc_32x4.log), one session, next to that session's copy bandwidth:

    python profiles/rhmc_measure.py [-lat 32 32 32 32] [-mass 0.1] [-runs 5] [-its 60]

0. The box's copy bandwidth (k_copy16 of libqexhip_tune, 1 GiB).
1. k_cgm_update_sum (timer "cgm_update_sum") against k_cgm_update (timer "cgm_update") at 4 / 10 / 16 shifts: `its` iterations of
   each solve (r2req = 0), the two alternating in one process on the same source; per-launch microseconds, and the bytes per site each
   has to move (r + the base direction + per further shift 2 or 4 vectors, + S) against the copy bandwidth.
2. One dev_rational_xx against one dev_solve_xx_multi at r2req 1e-20: host clock around calls that end in a synchronise.  The
   existing path would add nterm axpys on top of the solve to form the sum; there is no resident axpy entry, so the solve alone is
   timed -- a lower bound for the existing path.
3. hisq_fforce_rational (one multi-shift solve, nterm reconstructions) against hisq_fforce_solve with nterm copies of phi at the
   masses m_k (lock-step batches of four): the same force by both.
4. One trajectory of examples/hisq_rhmc.py (prepare, evolve, finish).
Medians of `runs` warm repetitions with the spread (min .. max); everything is warmed up by one untimed repetition."""
import argparse
import ctypes as C
import importlib.util
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stat(v):
    return "median %.3f  min %.3f  max %.3f  (n = %d)" % (statistics.median(v), min(v), max(v), len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-lat", type=int, nargs=4, default=[32, 32, 32, 32])
    ap.add_argument("-mass", type=float, default=0.1)
    ap.add_argument("-runs", type=int, default=5)
    ap.add_argument("-its", type=int, default=60)
    ap.add_argument("-gsteps", type=int, default=3)
    ap.add_argument("-fsteps", type=int, default=2)
    ap.add_argument("-skip-trajectory", action="store_true")
    a = ap.parse_args()
    from qex_amd import _lib
    from qex_amd.rational import rationalFit

    spec = importlib.util.spec_from_file_location("hisq_rhmc", os.path.join(ROOT, "examples", "hisq_rhmc.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    m = a.mass
    lo, hi = m * m, m * m + 6.0
    rats = ex.fit_rationals(2, lo, hi, 12, 8)
    hmc = ex.HisqRHMC(a.lat, rats, lo, hi, nf=2, mass=m, tau=0.1, gsteps=a.gsteps, fsteps=a.fsteps, warm=0.3)
    ctx, md = hmc.ctx, hmc.md
    print(ctx.info())
    gbs = C.c_double(0)
    _lib.tune_lib().qexhip_tune_stream(ctx._h, 1, 1024, 2048, 5, C.byref(gbs))
    print("copy bandwidth (k_copy16, 1 GiB): %.1f GB/s" % gbs.value)
    hmc.prepare()
    print("lattice %r HISQ fat + Naik (warm 0.3), mass %r; rationals: %s" % (
        a.lat, m, ", ".join("%s %d poles %.1e" % (k, r.nterm, e) for k, (r, e) in rats.items())))
    vh = int(np.prod(a.lat)) // 2

    # 1. the two update kernels
    b = ctx.field_new()
    hmc.prng.dev_gaussian_vector(ctx, b)
    out = ctx.field_new()
    xs = [ctx.field_new() for _ in range(16)]
    ctx.timers_enable(1)
    for n in (4, 10, 16):
        rat = rationalFit(-0.5, lo, hi, n)[0]
        sh = [float(np.sqrt(m * m + rat.beta[0]))] + [4.0 * (float(v) - float(rat.beta[0])) for v in rat.beta[1:]]
        t = {"cgm_update_sum": [], "cgm_update": []}
        for rep in range(a.runs + 1):
            for name in t:
                ctx.timers_reset()
                if name == "cgm_update_sum":
                    ctx.dev_rational_xx(out, b, m, rat.f0, rat.alpha, rat.beta, 0.0, a.its, True)
                else:
                    ctx.dev_solve_xx_multi(xs[:n], b, sh, 0.0, a.its, True)
                cnt, ms = ctx.timer(name)
                if rep:
                    t[name].append(1e3 * ms / cnt)
        for name, streams in (("cgm_update_sum", 2 + 2 + 2 * (n - 1) + 1), ("cgm_update", 2 + 1 + 4 * (n - 1))):
            # r read, p_0 read + written, per further shift p_k read + written (+ x_k read + written), S read + written
            byt = streams * 48 * vh
            med = statistics.median(t[name])
            print("%2d shifts  %-15s us per launch: %s   [%d vector streams, %.1f MB, %.0f GB/s = %.0f %% of copy]" % (
                n, name, stat(t[name]), streams, byt / 1e6, byt / med / 1e3, 100.0 * byt / med / 1e3 / gbs.value))
    ctx.timers_enable(0)

    # 2. one rational application against the multi-shift solve it replaces
    r = rats["action"][0]
    sh = [float(np.sqrt(m * m + r.beta[0]))] + [4.0 * (float(v) - float(r.beta[0])) for v in r.beta[1:]]
    t = {"dev_rational_xx": [], "dev_solve_xx_multi": []}
    its = {}
    for rep in range(a.runs + 1):
        for name in t:
            ctx.sync()
            t0 = time.time()
            if name == "dev_rational_xx":
                its[name] = ctx.dev_rational_xx(out, b, m, r.f0, r.alpha, r.beta, 1e-20, 10000, True)[0]
            else:
                its[name] = ctx.dev_solve_xx_multi(xs[:r.nterm], b, sh, 1e-20, 10000, True)[0]
            ctx.sync()
            if rep:
                t[name].append(1e3 * (time.time() - t0))
    for name in t:
        print("x^(-1/2), %d poles, r2req 1e-20  %-20s ms: %s   [%d iterations]" % (r.nterm, name, stat(t[name]), its[name]))

    # 3. the rational force against the batch force
    r = rats["force"][0]
    mk = [float(np.sqrt(m * m + v)) for v in r.beta]
    phis = [hmc.phi] + [ctx.field_new() for _ in range(r.nterm - 1)]
    for f in phis[1:]:
        ctx.field_upload(f, ctx.field_download(hmc.phi))
    t = {"hisq_fforce_rational": [], "hisq_fforce_solve": []}
    for rep in range(a.runs + 1):
        for name in t:
            ctx.sync()
            t0 = time.time()
            if name == "hisq_fforce_rational":
                its[name] = md.hisq_fforce_rational(hmc.phi, m, r.alpha, r.beta, 1e-12, 10000, 1e-6)
            else:
                its[name] = md.hisq_fforce_solve(phis, mk, [al / k for al, k in zip(r.alpha, mk)], 1e-12, 10000, 1e-6)
            ctx.sync()
            if rep:
                t[name].append(1e3 * (time.time() - t0))
    for name in t:
        print("force, %d poles, r2req 1e-12  %-22s ms: %s   [iterations %r]" % (r.nterm, name, stat(t[name]), its[name]))

    # 4. a trajectory of the example
    if not a.skip_trajectory:
        tt = []
        for rep in range(a.runs + 1):
            ctx.sync()
            t0 = time.time()
            hmc.prepare()
            hmc.evolve()
            acc = hmc.finish()
            ctx.sync()
            if rep:
                tt.append(time.time() - t0)
        print("trajectory (%d gauge, %d fermion 2MN steps, tau %r)  s: %s   [last dH %r; iterations so far %r]" % (
            a.gsteps, a.fsteps, hmc.tau, stat(tt), acc[1], hmc.iters))


if __name__ == "__main__":
    main()
