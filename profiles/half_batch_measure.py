#!/usr/bin/env python3
"""The numbers of DESIGN.md section 4 "16-bit batches" (sloppy = 2 on the batched entries with option "half_batch" = 1), measured in one
session on one MI355X at 32^4 (unless -lat L L L L is given), next to that session's copy bandwidth and the two yardsticks whose code is
older than the 16-bit batch: the fp32 batch (k_dslash_mrhs_lowp<StoreF32, ..>) and the single-system 16-bit solve (k_dslash_lowp<StoreHalf, ..>):

  wall     the box's copy bandwidth (k_copy16 of libqexhip_tune, 1 GiB); then, on g.random (8 links, format 1) and on HISQ fat + Naik
           links (16 links, format 0): the meson workload's four systems (point source at (0,0,0,2), colour 0, and its three
           symmetric shifts; m = 0.1, r2req = 1e-16; resident fields, warm, best of 3 and the spread) as the fp64 batch, the fp32
           batch, four single 16-bit solves and the 16-bit batch; then one Z4 / EO scalar-trace source on the HISQ links (64 solves,
           r2req = 1e-18) at m = 0.1 and 0.01 sqrt(2) with sloppy = 2 (options on), 1 and 0: seconds in the solves, iterations,
           updates and any fall-back
  kernels  four gaussian even-parity systems, r2req = 0, 100 iterations, "half_stall" out of reach, so that every launch has four live
           systems: the 16-bit batch, the fp32 batch and four single 16-bit solves on both link sets, as the workload of
               rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 profiles/half_batch_measure.py kernels
  stats    python3 profiles/half_batch_measure.py stats DIR/**/kernel_stats.csv COPY_GBS: the sweeps of that trace with calls, mean us,
           bytes per site and launch (links + masks + per system one vector element read and one written), TB/s against the copy
           bandwidth and us per system

one JSON line per measurement on stdout"""
import csv
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def out(**kw):
    print(json.dumps(kw), flush=True)


def sweep_bytes(kind, ndir, recon, n):
    """bytes per site and launch: kind 'half' or 'f32', n systems"""
    npair = ndir // 2
    if kind == "half":
        link, vec = (48 if recon else 72) * npair, 16
    else:
        link, vec = (96 if recon else 144) * npair, 24
    return link + (ndir * 8 / 64.0 if recon else 0.0) + 2 * vec * n


def stats(path, copy_gbs, vh):
    rows = []
    for r in csv.DictReader(open(path)):
        name = r["Name"]
        us = float(r["AverageNs"]) / 1e3
        m = re.match(r".*k_dslash_mrhs_lowp<Store(Half|F32), (\d+), (\d), (true|false)>", name)
        if m:
            kind, ndir, recon, n = m.group(1).lower(), int(m.group(2)), int(m.group(3)), 4
            sweep = "second" if m.group(4) == "true" else "first"
        else:
            m = re.match(r".*k_dslash_lowp<StoreHalf, (\d+), (?:true|false), (true|false), (true|false), (\d)>", name)
            if not m:
                if re.search(r"k_slphb_|k_slpb_|k_slph_|k_slph_stall", name):
                    rows.append(dict(kernel=name[:60], calls=int(r["Calls"]), us=round(us, 2)))
                continue
            kind, ndir, recon, n = "half", int(m.group(1)), int(m.group(4)), 1
            sweep = "second" if m.group(2) == "true" else "first"
        b = sweep_bytes(kind, ndir, recon, n)
        tbs = b * vh / us / 1e6
        rows.append(dict(kernel=name[:60], sweep=sweep, systems=n, calls=int(r["Calls"]), us=round(us, 2), bytes_per_site=round(b, 1),
                         tbytes_per_s=round(tbs, 3), of_copy=round(tbs * 1e3 / copy_gbs, 3), us_per_system=round(us / n, 2)))
    for row in sorted(rows, key=lambda d: d["kernel"]):
        out(what="kernel", **row)


def best_of(ctx, fn, reps=3):
    fn()
    ctx.sync()                       # warm
    ts = []
    for _ in range(reps):
        ctx.sync()
        t = time.perf_counter()
        r = fn()
        ctx.sync()
        ts.append((time.perf_counter() - t) * 1e3)
    return min(ts), max(ts) - min(ts), r


def links(q, ctx, rng, lat, kind):
    if kind == "random":
        g = rng.random()
        q.rephase(q.Layout(lat), g)
        return q.newStag(ctx, g)
    g = rng.warm(0.3)
    q.rephase(q.Layout(lat), g)
    return q.Staggered(ctx, g, smear=q.HisqCoefs().init())


def main():
    args = sys.argv[1:]
    lat = [32, 32, 32, 32]
    if "-lat" in args:
        i = args.index("-lat")
        lat = [int(v) for v in args[i + 1:i + 5]]
        del args[i:i + 5]
    mode = args[0] if args else "wall"
    if mode == "stats":
        return stats(args[1], float(args[2]), int(np.prod(lat)) // 2)
    import qex_amd as q
    from qex_amd import _lib

    ctx = q.Context(lat)
    lo = q.Layout(lat)
    out(what="device", info=ctx.info(), lat=lat)
    rng = q.RngField(lat, q.RngMilc6, 987654321)
    if mode == "kernels":
        ms = [0.1, 0.2, 0.4, 0.05]
        hb = [np.random.default_rng(j).standard_normal((lo.vol, 3, 2)) for j in range(4)]
        for b in hb:
            b[lo.vol // 2:] = 0
        hx = [np.zeros_like(b) for b in hb]
        fb, fx = [ctx.field_new(b) for b in hb], [ctx.field_new() for _ in range(4)]
        ctx.set_option("half", 1)
        ctx.set_option("half_stall", 1000000)
        for kind in ("random", "hisq"):
            s = links(q, ctx, rng, lat, kind)
            out(what="links", links=kind, info=s.links_info(), f32=ctx.links_info_f32(), half=ctx.links_info_half())
            for name, opt, sl in (("fp32 batch", 0, 1), ("16-bit batch", 1, 2)):
                ctx.set_option("half_batch", opt)
                its, fin, nup = s.solveXX_batch(hx, hb, ms, 0.0, 100, True, sloppy=sl)
                out(what="n4", links=kind, solver=name, iterations=its, updates=nup, last=ctx.sloppy_last_batch())
            for j in range(4):
                ctx.dev_solve_xx_sloppy(fx[j], fb[j], ms[j], 0.0, 100, True, 2)
            out(what="n4", links=kind, solver="4 x single 16-bit", last=ctx.sloppy_last())
        ctx.close()
        return
    gbs = C.c_double(0)
    _lib.tune_lib().qexhip_tune_stream(ctx._h, 1, 1024, 2048, 5, C.byref(gbs))
    out(what="copy_bandwidth", kernel="k_copy16 1 GiB", gbytes_per_s=gbs.value)
    masses = [0.1, 0.01 * np.sqrt(2.0)]
    if "-masses" in args:
        masses = [float(v) for v in args[args.index("-masses") + 1].split(",")]
    for kind in ("random", "hisq"):
        s = links(q, ctx, rng, lat, kind)
        ctx.set_option("half", 1)
        ctx.set_option("half_batch", 1)
        out(what="links", links=kind, info=s.links_info(), f32=ctx.links_info_f32(), half=ctx.links_info_half())
        m, r2req, maxits = 0.1, 1e-16, 100000
        src = ctx.field_new(q.pointSource(lo, [0, 0, 0, 2], 0))
        srcs = [ctx.field_new() for _ in range(3)]
        for mu in range(3):
            ctx.dev_sym_shift(srcs[mu], src, mu)
        bs, xs, pe = [src] + srcs, [ctx.field_new() for _ in range(4)], [True, False, False, False]
        runs = (("fp64 dev_solve_batch", lambda: ctx.dev_solve_batch(xs, bs, [m] * 4, r2req, maxits)),
                ("dev_solve_batch sloppy=1", lambda: ctx.dev_solve_batch(xs, bs, [m] * 4, r2req, maxits, sloppy=1)),
                ("4 x dev_solve_xx_sloppy SloppyHalf", lambda: [ctx.dev_solve_xx_sloppy(xs[j], bs[j], m, r2req, maxits, pe[j], 2) for j in range(4)]),
                ("dev_solve_batch sloppy=2 half_batch=1", lambda: ctx.dev_solve_batch(xs, bs, [m] * 4, r2req, maxits, sloppy=2)))
        for name, fn in runs:
            best, spread, r = best_of(ctx, fn)
            last = ctx.sloppy_last_batch() if name.startswith("dev_solve_batch") else []
            out(what="mesons", links=kind, solver=name, ms=round(best, 2), spread_ms=round(spread, 2), result=r,
                fell_back=[d["fell_back"] for d in last], half_iters=[d["half_iters"] for d in last])
        for f in bs + xs:
            ctx.field_free(f)
        if kind != "hisq":
            continue
        for mass in masses:
            for sl in (2, 1, 0):
                fell = []
                ts = []
                for rep in range(2):
                    r = q.RngField(lat, q.RngMilc6, 4711)
                    tr, est, st = q.scalarTrace(s, lo, r, mass, 1e-18, maxits=100000, source_type="Z4", dilute_type="EO", sloppy=sl, out=None)
                    ts.append(st["solve_s"])
                    fell.append(sum(d["fell_back"] for d in ctx.sloppy_last_batch()) if sl else 0)
                its, upd = st["iterations"][0], st["updates"][0]
                out(what="scalar_trace", links=kind, mass=mass, sloppy=sl, solves=len(its), solve_s=[round(t, 4) for t in ts],
                    iterations_min_max_sum=[min(its), max(its), sum(its)], updates_min_max=[min(upd), max(upd)],
                    fell_back_last_batch=fell, pbp_t0=float(est[0][0]))
    ctx.close()


if __name__ == "__main__":
    main()
