#!/usr/bin/env python3
"""The numbers of DESIGN.md section 4 "Low modes and deflation" for the deflated lock-step batch, measured in one session on the
MI355X (32^4 unless -lat is given):

  A  the box's copy bandwidth (k_copy16 of libqexhip_tune, 1 GiB), then kernel time (the library's event timers) of the
     multi-right-hand-side block dot / block axpy over 128 vectors at nrhs = 4 against FOUR calls of the single kernels.  Bytes: a
     half-volume vector is n2 * 16 B; the multi dot reads 128 + 4 vectors, four single dots 4 x 129; the multi axpy reads 128 + 4 and
     writes 4, four single ones read 4 x 129 and write 4.
  B  HISQ fat + Naik links (warm 0.3, seed 987654321): 64 pairs (nvecs = 128, abserr = 1e-8) as profiles/eig_measure.py computes
     them; wall time of the eigensolve.
  C  one Z4 / EO noise source of the scalar trace (2 nt solves, r2req = 1e-18, improved trace, batches of four) at m = 0.1 and
     m = 0.01 sqrt(2), fp64 and sloppy, without and with the 64 modes: iterations, wall time, time in the batched solves, the
     kernel time of the projections (block dot + block axpy, timers on in a second run) and the number of sources at which the
     eigensolve has paid for itself.

    python3 profiles/deflated_batch_measure.py [-lat 32 32 32 32] [-skip A]      (one JSON line per measurement on stdout)"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import qex_amd as q  # noqa: E402
from qex_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("-lat", type=int, nargs=4, default=[32, 32, 32, 32])
ap.add_argument("-skip", type=str, default="")
ap.add_argument("-nev", type=int, default=64)
ap.add_argument("-nvecs", type=int, default=128)
ap.add_argument("-degree", type=int, default=32)
ap.add_argument("-r2req", type=float, default=1e-18)
a = ap.parse_args()
lat = a.lat
vol = int(np.prod(lat))
VEC = (vol // 2 + 63) // 64 * 192 * 16          # bytes of one half-volume vector


def out(**kw):
    print(json.dumps(kw), flush=True)


ctx = q.Context(lat)
out(what="device", info=ctx.info(), vector_mbytes=VEC / 1e6)
rng = q.RngField(lat, q.RngMilc6, 987654321)
g = rng.warm(0.3)
q.rephase(q.Layout(lat), g)


def timed(names, fn, reps):
    """mean kernel milliseconds of the timer classes `names` over reps calls of fn (after one warm-up call)"""
    fn()
    ctx.sync()
    ctx.timers_enable(1)
    ctx.timers_reset()
    for _ in range(reps):
        fn()
    ctx.sync()
    ms = sum(ctx.timer(n)[1] for n in names)
    ctx.timers_enable(0)
    return ms / reps


if "A" not in a.skip:
    T = _lib.tune_lib()
    gbs = C.c_double(0)
    T.qexhip_tune_stream(ctx._h, 1, 1024, 2048, 5, C.byref(gbs))
    out(what="copy_bandwidth", kernel="k_copy16 1 GiB", gbytes_per_s=gbs.value)
    q.newStag(ctx, g)
    B = q.EigBasis(ctx, 128)
    ws = [ctx.field_new() for _ in range(4)]
    for w in ws:
        rng.dev_gaussian_vector(ctx, w)
    for i in range(128):
        B.set_vector(i, ws[i % 4])
    n = 128
    coef = np.full((4, n), 1e-3 + 1e-3j)
    for rep in range(2):                                    # twice, in both orders: the first arm of a session runs on a cold clock
        for arm in (("multi", "single") if rep == 0 else ("single", "multi")):
            if arm == "multi":
                ms = timed(["eig_dot"], lambda: B.block_dot_multi(0, n, ws), 10)
                nb = (n + 4) * VEC
            else:
                ms = timed(["eig_dot"], lambda: [B.block_dot(0, n, w) for w in ws], 10)
                nb = 4 * (n + 1) * VEC
            out(what="block_dot_x4", arm=arm, rep=rep, n=n, ms=ms, gbytes=nb / 1e9, gbytes_per_s=nb / ms / 1e6)
            if arm == "multi":
                ms = timed(["eig_axpy"], lambda: B.block_axpy_multi(0, coef, ws), 10)
                nb = (n + 8) * VEC
            else:
                ms = timed(["eig_axpy"], lambda: [B.block_axpy(0, coef[k], ws[k]) for k in range(4)], 10)
                nb = 4 * (n + 2) * VEC
            out(what="block_axpy_x4", arm=arm, rep=rep, n=n, ms=ms, gbytes=nb / 1e9, gbytes_per_s=nb / ms / 1e6)
    B.free()
    for w in ws:
        ctx.field_free(w)

s = q.Staggered(ctx, g, smear=q.HisqCoefs().init())
out(what="links", info=s.links_info())
basis = q.EigBasis(ctx, a.nvecs)
t = time.time()
rough = s.eigs(a.nev, nvecs=a.nvecs, relerr=0.0, abserr=1e-8, max_restarts=6, cheb_degree=0, basis=basis)
ctx.sync()
t_rough = time.time() - t
lo_ = 1.2 * float(rough.evals[-1])
t = time.time()
Bz = s.eigs(a.nev, nvecs=a.nvecs, relerr=0.0, abserr=1e-8, max_restarts=100, cheb_degree=a.degree, cheb_lo=lo_, cheb_hi=0.0, basis=basis)
ctx.sync()
t_eig = time.time() - t
out(what="eigs", nev=a.nev, nvecs=a.nvecs, degree=a.degree, cheb_lo=lo_, seconds=t_eig, rough_seconds=t_rough, nconv=Bz.nconv, stats=Bz.stats,
    lambda_0=float(Bz.evals[0]), lambda_last=float(Bz.evals[-1]), max_resid=float(Bz.resid.max()))

if "C" not in a.skip:
    qlo = q.Layout(lat)
    for mass in (0.1, 0.01 * np.sqrt(2.0)):
        for sloppy in (0, 1):
            rows = {}
            for name, kw in (("plain", {}), ("deflated", dict(deflate=Bz, nev=a.nev))):
                def run():
                    r = q.RngField(lat, q.RngMilc6, 987654321)
                    t0 = time.time()
                    _, es, st = q.scalarTrace(s, qlo, r, mass, a.r2req, dilute_type="EO", source_type="Z4", improved_trace=True, out=None,
                                              sloppy=sloppy, **kw)
                    ctx.sync()
                    return time.time() - t0, es, st
                run()                                       # warm-up (work fields, fp32 links)
                wall, es, st = run()
                ctx.timers_enable(1)
                ctx.timers_reset()
                wall_t, _, st_t = run()
                proj = ctx.timer("eig_dot")[1] + ctx.timer("eig_axpy")[1]
                ctx.timers_enable(0)
                its = st["iterations"][0]
                rows[name] = dict(wall_s=wall, solve_s=st["solve_s"], iterations=int(np.sum(its)), its_min=int(min(its)), its_max=int(max(its)),
                                  solves=len(its), projection_kernel_ms=proj, projection_share_of_solve=proj / 1e3 / st_t["solve_s"],
                                  est0=float(es[0][0]))
            gain = rows["plain"]["wall_s"] - rows["deflated"]["wall_s"]
            out(what="scalar_trace_source", mass=mass, sloppy=sloppy, r2req=a.r2req, rows=rows,
                iteration_ratio=rows["deflated"]["iterations"] / rows["plain"]["iterations"],
                break_even_sources=(t_eig / gain) if gain > 0 else None)
