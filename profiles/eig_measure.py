#!/usr/bin/env python3
"""The low-mode numbers DESIGN.md section 4 quotes, measured in one session on the MI355X (32^4 unless -lat is given):

  A  the box's copy bandwidth (k_copy16 of libqexhip_tune, 1 GiB), then per-call time and bytes/time of block dot and block axpy
     (n = 16, 128) and of the in-place rotation (m = 128, k = 64), against n calls of blas_cdot / blas_axpy.  Kernel time = the
     library's event timers around the launches.  Bytes: a half-volume vector is n2 * 16 B; block dot reads n + ceil(n/128) vectors,
     block axpy reads n + 1 and writes 1, the rotation reads m and writes k, cdot reads 2, axpy reads 2 and writes 1.
  B  HISQ fat + Naik links (warm 0.3, seed 987654321): nev = 64, nvecs = 128, abserr = 1e-8.  A short plain thick-restart run gives
     a rough lambda_63; the timed run is T_p on [1.2 lambda_63, auto].  Wall time, operator applications, share of the time in
     block dot + block axpy + rotation (event timers, a second run so that the wall time is taken with timers off).
  C  solveEE at m = 0.05 sqrt(2), r2req = 1e-14, fp64 and sloppy: undeflated (qexhip_dev_solve_xx / _sloppy) against deflated
     with 16, 32, 64 modes; iterations, milliseconds (host clock around the blocking call), and the number of solves at which the
     eigensolve of B has paid for itself.

    python3 profiles/eig_measure.py [-lat 32 32 32 32] [-skip A]      (one JSON line per measurement on stdout)"""
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
    s = q.newStag(ctx, g)
    B = q.EigBasis(ctx, 128)
    wid, yid = ctx.field_new(), ctx.field_new()
    rng.dev_gaussian_vector(ctx, wid)
    for i in range(128):
        if i % 16 == 0:
            rng.dev_gaussian_vector(ctx, yid)
        B.set_vector(i, yid)
    for n in (16, 128):
        ms = timed(["eig_dot"], lambda: B.block_dot(0, n, wid), 10)
        nb = (n + (n + 127) // 128) * VEC
        out(what="block_dot", n=n, ms=ms, gbytes=nb / 1e9, gbytes_per_s=nb / ms / 1e6)
        coef = np.full(n, 1e-3 + 1e-3j)
        ms = timed(["eig_axpy"], lambda: B.block_axpy(0, coef, yid), 10)
        nb = (n + 2) * VEC
        out(what="block_axpy", n=n, ms=ms, gbytes=nb / 1e9, gbytes_per_s=nb / ms / 1e6)
    # the parent's kernels, per call: blas_cdot on resident fields; blas_axpy through the host-pointer hook (the timer covers the kernel only)
    ms = timed(["blas"], lambda: ctx.dev_dot(wid, yid, "even"), 20)
    out(what="blas_cdot", ms=ms, gbytes=2 * VEC / 1e9, gbytes_per_s=2 * VEC / ms / 1e6, ms_x16=16 * ms, ms_x128=128 * ms)
    hx, hy = np.zeros((vol, 3, 2)), np.zeros((vol, 3, 2))
    ms = timed(["blas"], lambda: ctx.axpy(0.5, hx, hy, "even"), 3)
    out(what="blas_axpy", ms=ms, gbytes=3 * VEC / 1e9, gbytes_per_s=3 * VEC / ms / 1e6, ms_x16=16 * ms, ms_x128=128 * ms)
    Q = np.linalg.qr(np.random.default_rng(1).normal(size=(128, 128)))[0][:, :64]
    ms = timed(["eig_rotate"], lambda: B.rotate(Q), 5)
    nb = (128 + 64) * VEC
    out(what="rotate", m=128, k=64, ms=ms, gbytes=nb / 1e9, gbytes_per_s=nb / ms / 1e6, gflops=4.0 * 128 * 64 * (VEC / 16) / ms / 1e6)
    B.free()
    ctx.field_free(wid)
    ctx.field_free(yid)

s = q.Staggered(ctx, g, smear=q.HisqCoefs().init())
out(what="links", info=s.links_info())
basis = q.EigBasis(ctx, a.nvecs)
if "B" not in a.skip:
    t = time.time()
    rough = s.eigs(a.nev, nvecs=a.nvecs, relerr=0.0, abserr=1e-8, max_restarts=6, cheb_degree=0, basis=basis)
    ctx.sync()
    out(what="rough_plain_lanczos", seconds=time.time() - t, stats=rough.stats, lambda_0=float(rough.evals[0]), lambda_last=float(rough.evals[-1]),
        max_resid=float(rough.resid.max()))
    lo = 1.2 * float(rough.evals[-1])
    opts = dict(relerr=0.0, abserr=1e-8, max_restarts=100, cheb_degree=a.degree, cheb_lo=lo, cheb_hi=0.0, basis=basis)
    t = time.time()
    Bz = s.eigs(a.nev, nvecs=a.nvecs, **opts)
    ctx.sync()
    t_eig = time.time() - t
    out(what="eigs", nev=a.nev, nvecs=a.nvecs, degree=a.degree, cheb_lo=lo, seconds=t_eig, nconv=Bz.nconv, stats=Bz.stats,
        lambda_0=float(Bz.evals[0]), lambda_last=float(Bz.evals[-1]), max_resid=float(Bz.resid.max()))
    ctx.timers_enable(1)
    ctx.timers_reset()
    t = time.time()
    Bz = s.eigs(a.nev, nvecs=a.nvecs, **opts)
    ctx.sync()
    t2 = time.time() - t
    tm = {n: ctx.timer(n)[1] for n in ("eig_dot", "eig_axpy", "eig_rotate", "dslash", "blas", "reduce")}
    ctx.timers_enable(0)
    orth = tm["eig_dot"] + tm["eig_axpy"] + tm["eig_rotate"]
    out(what="eigs_anatomy", seconds_with_timers=t2, kernel_ms=tm, orth_rotate_share_of_wall=orth / 1e3 / t2)
else:
    Bz = s.eigs(a.nev, nvecs=a.nvecs, relerr=0.0, abserr=1e-8, max_restarts=100, cheb_degree=a.degree, cheb_lo=0.3, basis=basis)
    t_eig = float("nan")

if "C" not in a.skip:
    mass, r2req = 0.05 * np.sqrt(2.0), 1e-14
    bid, xid = ctx.field_new(), ctx.field_new()
    rng.dev_gaussian_vector(ctx, bid)
    for sloppy in (0, 1):
        def plain():
            if sloppy:
                return ctx.dev_solve_xx_sloppy(xid, bid, mass, r2req, 100000)[:2]
            return ctx.dev_solve_xx(xid, bid, mass, r2req, 100000)[:2]
        rows = []
        for nd in (None, 16, 32, 64):
            if nd is not None and nd > a.nev:
                continue
            fn = plain if nd is None else (lambda: ctx.dev_solve_xx_deflated(Bz, nd, xid, bid, mass, r2req, 100000, sloppy=sloppy))
            fn()
            ctx.sync()
            best = None
            for _ in range(3):
                t = time.time()
                its, r2 = fn()
                ctx.sync()
                dt = (time.time() - t) * 1e3
                best = dt if best is None else min(best, dt)
            rows.append(dict(modes=nd, its=its, ms=best, r2=r2))
        base = rows[0]["ms"]
        for r in rows[1:]:
            r["break_even_solves"] = t_eig * 1e3 / (base - r["ms"]) if base > r["ms"] else None
        out(what="solveEE", sloppy=sloppy, mass=mass, r2req=r2req, rows=rows)
