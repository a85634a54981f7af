#!/usr/bin/env python3
"""The scalar-trace numbers README.md and DESIGN.md section 4 quote, measured in one session on the MI355X (32^4 unless -lat is given):

  A  the box's copy bandwidth (k_copy16 of libqexhip_tune, 1 GiB), then kernel time (the library's event timers, class "trace") and
     bytes/time of dev_dilute and dev_trace_accum at n = 1 and n = 4 and of dev_cfield_slices.  Bytes per site: dilute 48 (1 + n)
     (src read, n destinations written), accum 96 n + 32 (improved, a = b: 48 n + 32), slices 16.
  B  one whole Z4 / EO noise source (2 nt solves) on HISQ links (warm 0.3, seed 987654321), m = 0.1, r2req = 1e-18, improved trace:
     qex_amd.scalarTrace with batch = 4 in fp64, batch = 4 with sloppy = 1, and batch = 1 -- against the path a user has without
     this feature, per pattern: numpy mask of the downloaded noise on the host, field_upload, one resident solve
     (dev_solve_batch of one system), field_download, numpy contraction; per-timeslice sums with numpy at the end.  Solve seconds
     (host clock around the blocking solves) and everything else are reported separately.

    python3 profiles/scalar_trace_measure.py [-lat 32 32 32 32] [-skip A]      (one JSON line per measurement on stdout)"""
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
ap.add_argument("-mass", type=float, default=0.1)
ap.add_argument("-r2req", type=float, default=1e-18)
a = ap.parse_args()
lat = a.lat
vol, nt = int(np.prod(lat)), lat[3]


def out(**kw):
    print(json.dumps(kw), flush=True)


ctx = q.Context(lat)
out(what="device", info=ctx.info(), sites=vol)
lo = q.Layout(lat)
rng = q.RngField(lat, q.RngMilc6, 987654321)


def timed(fn, reps):
    """mean kernel microseconds of the timer class "trace" over reps calls of fn (after one warm-up call)"""
    fn()
    ctx.sync()
    ctx.timers_enable(1)
    ctx.timers_reset()
    for _ in range(reps):
        fn()
    ctx.sync()
    ms = ctx.timer("trace")[1]
    ctx.timers_enable(0)
    return 1e3 * ms / reps


if "A" not in a.skip:
    T = _lib.tune_lib()
    gbs = C.c_double(0)
    T.qexhip_tune_stream(ctx._h, 1, 1024, 2048, 5, C.byref(gbs))
    copy = gbs.value
    out(what="copy_bandwidth", kernel="k_copy16 1 GiB", gbytes_per_s=copy)
    f = [ctx.field_new() for _ in range(9)]
    for fid in f:
        rng.dev_gaussian_vector(ctx, fid)
    tr = ctx.cfield_new()

    def row(what, n, us, bytes_per_site, **kw):
        gb = bytes_per_site * vol / 1e9
        out(what=what, n=n, us=us, bytes_per_site=bytes_per_site, gbytes_per_s=gb / us * 1e6, fraction_of_copy=gb / us * 1e6 / copy, **kw)

    for n in (1, 4):
        for kind, name in ((0, "EO"), (1, "CORNER")):
            us = timed(lambda: ctx.dev_dilute(f[1:1 + n], f[0], kind, [k & 1 for k in range(n)], [k // 2 for k in range(n)], 1.0), 20)
            row("dev_dilute", n, us, 48 * (1 + n), kind=name)
        us = timed(lambda: ctx.dev_trace_accum(tr, f[1:1 + n], f[5:5 + n], 1.0), 20)
        row("dev_trace_accum", n, us, 96 * n + 32, form="unimproved")
        us = timed(lambda: ctx.dev_trace_accum(tr, f[1:1 + n], f[1:1 + n], 0.1), 20)
        row("dev_trace_accum", n, us, 48 * n + 32, form="improved")
    us = timed(lambda: ctx.dev_cfield_slices(tr), 20)
    row("dev_cfield_slices", 0, us, 16)
    t = time.perf_counter()
    for _ in range(20):
        ctx.dev_cfield_slices(tr)
    out(what="dev_cfield_slices_call", us_host_clock_with_readback=(time.perf_counter() - t) / 20 * 1e6)
    for fid in f:
        ctx.field_free(fid)
    ctx.cfield_free(tr)

if "B" not in a.skip:
    g = rng.warm(0.3)
    q.rephase(lo, g)
    s = q.Staggered(ctx, g, smear=q.HisqCoefs().init())
    out(what="links", info=s.links_info(), f32=ctx.links_info_f32())
    ests = {}
    for name, kw in (("batch4_fp64", dict(batch=4)), ("batch4_sloppy1", dict(batch=4, sloppy=1)), ("batch1_fp64", dict(batch=1))):
        r = q.RngField(lat, q.RngMilc6, 987654321)
        ctx.sync()
        t = time.perf_counter()
        trs, es, st = q.scalarTrace(s, lo, r, a.mass, a.r2req, dilute_type="EO", source_type="Z4", improved_trace=True, out=None, **kw)
        wall = time.perf_counter() - t
        its = st["iterations"][0]
        ests[name] = es[0]
        out(what="scalarTrace", arm=name, solves=len(its), wall_s=wall, solve_s=st["solve_s"], non_solve_s=wall - st["solve_s"],
            noise_s=st["noise_s"], dilute_accum_slices_s=st["contract_s"], non_solve_share=(wall - st["solve_s"]) / wall,
            iterations=[min(its), max(its)], updates=[min(st["updates"][0]), max(st["updates"][0])])

    # the path without this feature
    r = q.RngField(lat, q.RngMilc6, 987654321)
    ctx.sync()
    t = time.perf_counter()
    solve_s, its = 0.0, []
    b_id, x_id = ctx.field_new(), ctx.field_new()
    u = r.uniform(3)                                # no Z4 fill exists there: the host thresholds the field's uniforms
    eta = np.stack([np.where(u < 0.25, 1.0, np.where(u < 0.5, 0.0, np.where(u < 0.75, -1.0, 0.0))),
                    np.where(u < 0.25, 0.0, np.where(u < 0.5, 1.0, np.where(u < 0.75, 0.0, -1.0)))], axis=-1)
    par = lo.coords.sum(axis=1) & 1
    trce = np.zeros(vol)
    for tt in range(nt):
        for idx in range(2):
            m = (lo.coords[:, 3] == tt) & (par == idx)
            b = np.zeros_like(eta)
            b[m] = eta[m]
            ctx.field_upload(b_id, b)
            ctx.sync()
            t1 = time.perf_counter()
            i1, _ = ctx.dev_solve_batch([x_id], [b_id], [a.mass], a.r2req, 100000)
            solve_s += time.perf_counter() - t1
            its += i1
            phi = ctx.field_download(x_id)
            trce += a.mass * (phi * phi).sum(axis=(1, 2))
    trce *= 1.0 / 3.0
    est = np.zeros(nt)
    np.add.at(est, lo.coords[:, 3], trce)
    est /= lat[0] * lat[1] * lat[2]
    wall = time.perf_counter() - t
    out(what="scalarTrace", arm="host_per_pattern", solves=len(its), wall_s=wall, solve_s=solve_s, non_solve_s=wall - solve_s,
        non_solve_share=(wall - solve_s) / wall, iterations=[min(its), max(its)])
    ref = ests["batch4_fp64"]
    out(what="est_agreement", scale=float(np.abs(ref).max()),
        **{k: float(np.abs(v - ref).max()) for k, v in list(ests.items()) + [("host_per_pattern", est)]})
