#!/usr/bin/env python
"""The main block of src/gauge/gaugefix.nim (:357-425) through libqexhip: a configuration is rotated by a random gauge
transformation (`t := g[0]` of a hot field, :372-375), its plaquettes and link trace are printed (pdisp, :393-400), the gauge
is fixed on the device with getGaugeFixTransform (:417), the transform is applied (:420) and the same numbers are printed again.
Only the metrics cross PCIe during the iteration.

    python examples/gauge_fix.py [-lat 8 8 8 8] [-dirs 0 1 2] [-gstop 1e-6] [-orf 1.5] [-warm 0.3] [-verb 0] [-wall T0]

-dirs 0 1 2 is Coulomb gauge (the default, as in the reference), 0 1 2 3 Landau gauge.  `-wall T0` then computes the local meson
table of a Coulomb-gauge wall source on slice T0 (sources.nim:4-8, fpvaMeas.nim:33-78) on the fixed configuration.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import qex_amd as q  # noqa: E402
from qex_amd._lib import check, lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("-lat", type=int, nargs=4, default=[8, 8, 8, 8])
ap.add_argument("-dirs", type=int, nargs="+", default=[0, 1, 2])
ap.add_argument("-gstop", type=float, default=1e-6)
ap.add_argument("-orf", type=float, default=1.5)
ap.add_argument("-maxits", type=int, default=100000)
ap.add_argument("-warm", type=float, default=0.3, help="spread of the warm start that is rotated and then fixed")
ap.add_argument("-seed", type=int, default=987654321)
ap.add_argument("-verb", type=int, default=0)
ap.add_argument("-wall", type=int, default=None, metavar="T0")
ap.add_argument("-mass", type=float, default=0.1)
a = ap.parse_args()

rf = q.RngField(a.lat, q.RngMilc6, a.seed)
g = rf.warm(a.warm)
rot = np.ascontiguousarray(rf.random()[:, 0])                       # t := g[0] of a hot field
ctx = q.Context(a.lat)
print(ctx.info())
print("gradient^2 stopping condition (gstop):", a.gstop)
print("overrelaxation factor (orf):", a.orf)


def pdisp():
    p = q.plaq(ctx)
    print("plaqs:", " ".join("%.16g" % v for v in p))
    print("%.16g" % (2.0 * p[:3].sum()))
    print("%.16g" % (2.0 * p[3:].sum()))
    print("link trace: %.16g" % q.linkTrace(ctx, a.dirs))


q.gaugeSet(ctx, g)
pdisp()
check(lib().qexhip_gfix_set_transform(ctx._h, rot.ctypes.data))     # the random rotation
q.gaugeTransform(ctx)
pdisp()
t0 = time.perf_counter()
t, info = q.getGaugeFixTransform(ctx, a.dirs, gstop=a.gstop, orf=a.orf, maxits=a.maxits, verb=a.verb)
dt = time.perf_counter() - t0
print("gauge fixing: %d iterations, gdsq %.3e, %.3f s" % (info["iters"], info["gdsq"], dt))
q.gaugeTransform(ctx)
pdisp()
print("post-fix link trace: %.16g" % q.linkTrace(ctx, a.dirs))

if a.wall is not None:
    lo = q.Layout(a.lat)
    gf = lo.newGauge()
    check(lib().qexhip_gauge_get(ctx._h, gf.ctypes.data))
    q.rephase(lo, gf)
    s = q.newStag(ctx, gf)
    c = np.zeros((a.lat[3], 8))
    for ic in range(3):
        v = np.zeros(3)
        v[ic] = 1.0
        src = q.wallSource(lo, a.wall, v)
        dest = lo.ColorVector()
        sp = q.SolverParams(r2req=1e-12, maxits=100000, verbosity=0)
        s.solve(dest, src, a.mass, sp)
        c += q.stagLocalMesons(ctx, dest, dest, a.wall)
    print("local mesons of the wall source at t0 = %d, mass %g:" % (a.wall, a.mass))
    q.printLocalMesons(c)
