#!/usr/bin/env python
"""The main program of src/gauge/stoutsmear.nim (:177-282) through libqexhip: a config-file smear / un-smear tool.  The
configuration is read from a SciDAC file (`-gaugefile`; a missing file means `g.random` on 8^4, :212-218,251-252), optionally
reunitarised (:248-249), then either smeared with the stout steps `-steps` in order, in place (:269-272), or -- `-backward 1` --
un-smeared from the last step to the first with the fixed-point inverse (:255-267); its plaquettes are printed as the reference's
MEASplaq lines after every step (:193-200) and the result is written to `-savefile` (:274-279).  The links stay on the device
between the steps of a forward run; only the plaquettes cross PCIe.

    python examples/stout_smear.py [-gaugefile f.lime] [-savefile out.lime] [-steps 0.1 0.1] [-backward 0|1] [-maxiter 1000]
                                   [-r2req 1e-24] [-reunitarize 0|1]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import qex_amd as q  # noqa: E402
from qex_amd._lib import check, lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("-gaugefile", default="")
ap.add_argument("-savefile", default=None)
ap.add_argument("-steps", type=float, nargs="+", default=[0.1], help="a list of smearing steps")
ap.add_argument("-backward", type=int, default=0, help="inverse flow, from the last to the first in steps")
ap.add_argument("-maxiter", type=int, default=1000)
ap.add_argument("-r2req", type=float, default=1e-24)
ap.add_argument("-reunitarize", type=int, default=1)
a = ap.parse_args()
savefile = a.savefile or (a.gaugefile + ".smear.lime" if a.gaugefile else "config.smear.lime")

have = os.path.exists(a.gaugefile)
if have:
    lat = q.getFileLattice(a.gaugefile)
else:
    if a.gaugefile:
        print("WARNING: Nonexistent gauge file:", a.gaugefile)
    lat = [8, 8, 8, 8]
ctx = q.Context(lat)
print(ctx.info())
if have:
    g, _ = q.loadGauge(a.gaugefile, lat)
    print("loaded gauge from file:", a.gaugefile)
    if a.reunitarize:
        q.reunit(ctx, g)
else:
    g = q.RngField(lat, q.RngMilc6, 17 ** 7).random()


def mplaq(label=""):
    """mplaq (:193-200) of the resident links"""
    pl = q.plaq(ctx)
    ps, pt = 2.0 * pl[:3].sum(), 2.0 * pl[3:].sum()
    print("MEASplaq %s ss: %.16g  st: %.16g  tot: %.16g" % (label, ps, pt, 0.5 * (ps + pt)))


q.gaugeSet(ctx, g)
mplaq()
if a.backward:
    fg = np.zeros_like(g)
    for i in range(len(a.steps) - 1, -1, -1):
        ss = q.newStoutSmear(ctx, a.steps[i])
        it, r2 = ss.inverse(fg, g, rdf2req=a.r2req, maxIter=a.maxiter)
        if it >= a.maxiter:
            print("WARNING: maximum iteration count reached")
        if ss.diverging:
            print("WARNING: df^2 increased during the iteration")
        print("inverse %d t %g iter %d r2 %.6g" % (i, a.steps[i], it, r2))
        fg, g = g, fg
        q.gaugeSet(ctx, g)
        mplaq(str(i))
else:
    for i, alpha in enumerate(a.steps):
        q.stoutSmear(ctx, None, alpha, None)            # ss.smear(gf, gf) on the resident links
        mplaq(str(i))
    check(lib().qexhip_gauge_get(ctx._h, g.ctypes.data))
q.saveGauge(g, lat, savefile)
print("saved gauge to file:", savefile)
