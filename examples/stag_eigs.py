#!/usr/bin/env python
"""The main program of src/eigens/hisqev.nim through libqexhip: low modes of the even/odd HISQ operator and a deflated
point-source solveEE.

    python examples/stag_eigs.py [-lat 8 8 8 8] [-mass 0.01] [-nev 16] [-nvecs 40] [-gauge file.lime] [-warm 0.3]

Links are loaded (SciDAC/LIME) or generated from the library's RngMilc6 field, rephased on the host as in QEX, and HISQ-smeared
on the GPU.  The nev lowest eigenpairs of H = -D_eo D_oe come from the thick-restart Lanczos with Chebyshev acceleration
(Staggered.eigs); they are printed as the reference prints its singular values (sv = sqrt(lambda), err = the residual of the
pair, err/sv).  Then solveEE at -mass from a point source, undeflated and deflated with np in {0, nev/2, nev} modes, printed
as the reference's `rsolve` lines."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import qex_amd as q  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("-lat", type=int, nargs=4, default=[8, 8, 8, 8])
ap.add_argument("-mass", type=float, default=0.01)
ap.add_argument("-nev", type=int, default=16)
ap.add_argument("-nvecs", type=int, default=40)
ap.add_argument("-abserr", type=float, default=1e-8)
ap.add_argument("-relerr", type=float, default=0.0)
ap.add_argument("-maxup", type=int, default=200)
ap.add_argument("-cheb", type=int, default=12, help="Chebyshev degree (0: plain Lanczos)")
ap.add_argument("-cheb_lo", type=float, default=0.3)
ap.add_argument("-r2req", type=float, default=1e-16)
ap.add_argument("-seed", type=int, default=987654321)
ap.add_argument("-warm", type=float, default=0.3)
ap.add_argument("-gauge", type=str, default=None)
a = ap.parse_args()

lo = q.Layout(a.lat)
if a.gauge:
    g, _ = q.loadGauge(a.gauge, a.lat)
else:
    g = q.RngField(a.lat, q.RngMilc6, a.seed).warm(a.warm)
q.rephase(lo, g)
ctx = q.Context(a.lat)
print(ctx.info())
s = q.Staggered(ctx, g, smear=q.HisqCoefs().init())
t = time.time()
B = s.eigs(a.nev, nvecs=a.nvecs, relerr=a.relerr, abserr=a.abserr, max_restarts=a.maxup, cheb_degree=a.cheb, cheb_lo=a.cheb_lo, seed=a.seed)
print("eigs: nconv %d of %d in %.3f s; %s" % (B.nconv, a.nev, time.time() - t, B.stats))
for i in range(a.nev):
    sv = float(np.sqrt(B.evals[i]))
    print("%3d  %-18.12g %-12.4g %-12.4g" % (i, sv, B.resid[i], B.resid[i] / sv))

src = np.zeros((lo.vol, 3, 2))
src[0, 0, 0] = 1.0                                                # point source, colour 0 at the origin (an even site)
x = np.zeros_like(src)
sp = q.SolverParams(r2req=a.r2req, maxits=100000, verbosity=0)
t = time.time()
s.solveEE(x, src, a.mass, sp)
print("undeflated  its: %d  time: %.4f  r2: %.3e" % (sp.iterations, time.time() - t, sp.r2))
for npd in sorted({0, a.nev // 2, a.nev}):
    sp = q.SolverParams(r2req=a.r2req, maxits=100000, verbosity=0)
    t = time.time()
    s.solveEE(x, src, a.mass, sp, deflate=B, nev=npd)
    print("np: %d  its: %d  time: %.4f  r2: %.3e" % (npd, sp.iterations, time.time() - t, sp.r2))
B.free()
