#!/usr/bin/env python3
"""The connected-correlator numbers README.md and DESIGN.md section 4 quote, measured in one session on the MI355X (32^4 unless -lat
is given):

  A  the box's copy bandwidth (k_copy16 of libqexhip_tune, 1 GiB), then kernel time (the library's event timers, class "trace") and
     bytes/time of dev_point_source and dev_conn_accum at n = 1 and n = 4: -rounds rounds of 20 calls each, median and min / max of
     the rounds' means.  Bytes per site: point source 48 n (n destinations written), accumulation 48 n + 32 (n vectors read, the
     cfield's 16 B read and 16 B written).
  B  one 16-point measurement (48 solves) on nHYP(0.4, 0.5, 0.5) links of g.warm 0.3 (seed 987654321), m = 0.1, r2req = 1e-18, points
     from randomPoint on GlobalRng(987654321): qex_amd.connMeson with batch = 4 in fp64, with sloppy = 1, and with sloppy = 2 and
     option half_batch -- against the path a user has without this feature, per system: the point source built with numpy,
     field_upload, one resident solve (dev_solve_batch of one system), field_download, |phi|^2 and np.roll over the four axes on
     the host; sign and per-timeslice sums with numpy at the end.  The arms alternate within each of -rounds rounds; median and
     min / max of the wall and solve seconds (host clock around work that ends in a synchronise) are reported.

    python3 profiles/conn4d_measure.py [-lat 32 32 32 32] [-skip A] [-rounds 3]      (one JSON line per measurement on stdout)"""
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
ap.add_argument("-num_source", type=int, default=16)
ap.add_argument("-rounds", type=int, default=3)
a = ap.parse_args()
lat = a.lat
vol, nt = int(np.prod(lat)), lat[3]


def out(**kw):
    print(json.dumps(kw), flush=True)


def stats(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


ctx = q.Context(lat)
out(what="device", info=ctx.info(), sites=vol)
lo = q.Layout(lat)
rng = q.RngField(lat, q.RngMilc6, 987654321)
R = q.GlobalRng(987654321)
pts = []
for _ in range(a.num_source):
    q.randomPoint(R, lat, pts, q.defaultSqMinDistance(lat, a.num_source))
out(what="points", sq_min_distance=q.defaultSqMinDistance(lat, a.num_source), pts=pts)


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
    f = [ctx.field_new() for _ in range(4)]
    for fid in f:
        rng.dev_gaussian_vector(ctx, fid)
    tr = ctx.cfield_new()
    odd = [[v % lat[i] for i, v in enumerate(p)] for p in ([1, 2, 4, 6], [3, 0, 2, 8], [2, 2, 2, 2], [5, 4, 30, 17])]

    def row(what, n, us, bytes_per_site, **kw):
        gb = bytes_per_site * vol / 1e9
        med = float(np.median(us))
        out(what=what, n=n, us=stats(us), bytes_per_site=bytes_per_site, gbytes_per_s=gb / med * 1e6, fraction_of_copy=gb / med * 1e6 / copy, **kw)

    for n in (1, 4):
        for name, p in (("even", pts[:n]), ("mixed parity", odd[:n])):
            us = [timed(lambda: ctx.dev_conn_accum(tr, f[:n], p, 1.0 / 16.0), 20) for _ in range(a.rounds)]
            row("dev_conn_accum", n, us, 48 * n + 32, points=name)
    for n in (1, 4):
        us = [timed(lambda: ctx.dev_point_source(f[:n], pts[:n], [k % 3 for k in range(n)]), 20) for _ in range(a.rounds)]
        row("dev_point_source", n, us, 48 * n)
    for fid in f:
        ctx.field_free(fid)
    ctx.cfield_free(tr)

if "B" not in a.skip:
    g = rng.warm(0.3)
    s = q.Staggered(ctx, g, smear=q.HypCoefs(0.4, 0.5, 0.5), bc="pppa")
    ctx.set_option("half", 1)
    out(what="links", info=s.links_info(), f32=ctx.links_info_f32())
    scal = 1.0 / len(pts)
    c = lo.coords

    def host_path():
        ctx.sync()
        t = time.perf_counter()
        solve_s, its = 0.0, []
        b_id, x_id = ctx.field_new(), ctx.field_new()
        locmes = np.zeros((lat[3], lat[2], lat[1], lat[0]))
        for pt in pts:
            site = lo.index(pt)
            for col in range(3):
                b = np.zeros((vol, 3, 2))
                b[site, col, 0] = 1.0
                ctx.field_upload(b_id, b)
                ctx.sync()
                t1 = time.perf_counter()
                i1, _ = ctx.dev_solve_batch([x_id], [b_id], [a.mass], a.r2req, 100000)
                solve_s += time.perf_counter() - t1
                its += i1
                phi = ctx.field_download(x_id)
                n2 = np.empty_like(locmes)
                n2[c[:, 3], c[:, 2], c[:, 1], c[:, 0]] = scal * (phi * phi).sum(axis=(1, 2))
                locmes += np.roll(n2, [-pt[3], -pt[2], -pt[1], -pt[0]], axis=(0, 1, 2, 3))
        sign = 1.0 - 2.0 * ((np.arange(lat[2])[:, None, None] + np.arange(lat[1])[None, :, None] + np.arange(lat[0])[None, None, :]) & 1)
        locmes *= sign[None]
        est = locmes.sum(axis=(1, 2, 3))
        wall = time.perf_counter() - t
        ctx.field_free(b_id)
        ctx.field_free(x_id)
        return wall, solve_s, its, [0], est

    def device(**kw):
        half = kw.pop("half_batch", 0)
        ctx.set_option("half_batch", half)
        ctx.sync()
        t = time.perf_counter()
        _, est, st = q.connMeson(s, lo, pts, a.mass, a.r2req, out=None, batch=4, **kw)
        wall = time.perf_counter() - t
        ctx.set_option("half_batch", 0)
        return wall, st["solve_s"], st["iterations"], st["updates"], est

    arms = (("batch4_fp64", lambda: device()), ("batch4_sloppy1", lambda: device(sloppy=1)),
            ("batch4_sloppy2_half", lambda: device(sloppy=2, half_batch=1)), ("host_per_system", host_path))
    for name, fn in arms[:3]:                  # warm-up: every shape of the timed rounds (the host arm's kernels are the fp64 batch's)
        fn()
    runs = {name: [] for name, _ in arms}
    for _ in range(a.rounds):
        for name, fn in arms:
            runs[name].append(fn())
    for name, _ in arms:
        r = runs[name]
        wall, solve = [x[0] for x in r], [x[1] for x in r]
        out(what="connMeson", arm=name, solves=len(r[0][2]), wall_s=stats(wall), solve_s=stats(solve),
            non_solve_s=stats([w - v for w, v in zip(wall, solve)]), non_solve_share=float(np.median([(w - v) / w for w, v in zip(wall, solve)])),
            iterations=[min(r[0][2]), max(r[0][2])], updates=[min(r[0][3]), max(r[0][3])])
    ref = runs["batch4_fp64"][0][4]
    out(what="est_agreement", scale=float(np.abs(ref).max()), **{k: float(np.abs(v[0][4] - ref).max()) for k, v in runs.items()})
    base = np.median([x[0] for x in runs["host_per_system"]])
    out(what="wall_ratio_to_host", **{k: float(np.median([x[0] for x in v]) / base) for k, v in runs.items()})
