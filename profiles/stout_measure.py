#!/usr/bin/env python3
"""The stout-smearing numbers DESIGN.md section 4 quotes, measured in one session on the MI355X (32^4 unless -lat is given), next
to the session's copy bandwidth (k_copy16 of libqexhip_tune, 1 GiB) and one RK3 stage of the Wilson flow:

  flow_stage      kernel time of one RK3 stage (timer "staple" of a one-step flow / 3), min / median / max over the repetitions:
                  the stage-to-stage spread every stout step below is judged against
  stout_step      one stout step on the resident links, nothing kept (qexhip_stout_smear): the same kernel launch
  stout_step_kept the same with the closure state kept (qexhip_stout_prepare, one level, g = NULL): kernel time, and the wall
                  time of the call, which adds the copy of the resident links into the level (576 B/site read + written)
  backward        k_stout_link and k_stout_stencil of a one-level chain (timers "stout_link", "stout_stencil"), the stencil kernel
                  against the 2304 B/site bound of the issue (gf, cg, deriv read + written), against the 2880 B/site it moves
                  here (the per-link TAH field t as well), and its share of the vector fp64 peak (78.6 TFLOP/s): 37 3x3 complex
                  products per link, 216 flop each
  force3          a three-level gauge force, f left on the device: wall time and its kernel classes
  inverse         one iteration of the inverse (timer "stout_inverse" over 8 iterations)

    python3 profiles/stout_measure.py [-lat 32 32 32 32] [-reps 10]      (one JSON line per measurement on stdout)"""
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
ap.add_argument("-reps", type=int, default=10)
ap.add_argument("-alpha", type=float, default=0.1)
a = ap.parse_args()
lat, vol = a.lat, int(np.prod(a.lat))
FP64_PEAK = 78.6e12


def out(**kw):
    print(json.dumps(kw), flush=True)


ctx = q.Context(lat)
out(what="device", info=ctx.info(), lat=lat)
T = _lib.tune_lib()
gbs = C.c_double(0)
T.qexhip_tune_stream(ctx._h, 1, 1024, 2048, 5, C.byref(gbs))
copy_gbs = gbs.value
out(what="copy_bandwidth", kernel="k_copy16 1 GiB", gbytes_per_s=copy_gbs)
g = q.RngField(lat, q.RngMilc6, 987654321).warm(0.3)
q.gaugeSet(ctx, g)


def kernel_ms(names, fn, reps=a.reps):
    """per repetition: {timer class: kernel ms} and the wall ms of fn (after one warm-up call)"""
    fn()
    ctx.sync()
    rows = []
    for _ in range(reps):
        ctx.timers_enable(1)
        ctx.timers_reset()
        t = time.perf_counter()
        fn()
        ctx.sync()
        wall = (time.perf_counter() - t) * 1e3
        row = {n: ctx.timer(n)[1] for n in names}
        ctx.timers_enable(0)
        row["wall"] = wall
        rows.append(row)
    return rows


def stats(v):
    v = sorted(v)
    return dict(min=v[0], median=v[len(v) // 2], max=v[-1])


rows = kernel_ms(["staple"], lambda: q.gaugeFlowResident(ctx, 1, 0.01))
stage = stats([r["staple"] / 3 for r in rows])
out(what="flow_stage", ms=stage, spread_ms=stage["max"] - stage["min"])
q.gaugeSet(ctx, g)
rows = kernel_ms(["staple"], lambda: q.stoutSmear(ctx, None, a.alpha, None))
step = stats([r["staple"] for r in rows])
out(what="stout_step", ms=step, wall_ms=stats([r["wall"] for r in rows]), excess_over_flow_stage_ms=step["median"] - stage["median"])
q.gaugeSet(ctx, g)
rows = kernel_ms(["staple"], lambda: q.stoutSmearGetForce(ctx, None, None, [a.alpha]))
kept = stats([r["staple"] for r in rows])
wall = stats([r["wall"] for r in rows])
out(what="stout_step_kept", ms=kept, wall_ms=wall, excess_over_flow_stage_ms=kept["median"] - stage["median"],
    closure_copy_bytes_per_site=1152, closure_copy_ms_at_copy_rate=1152.0 * vol / copy_gbs / 1e6,
    resident_bytes_per_level_per_site=1152, bytes_per_site_kept_by_the_reference=4 * 576)

sf = q.stoutSmearGetForce(ctx, None, None, [a.alpha])
rows = kernel_ms(["stout_link", "stout_stencil", "staple"], lambda: sf.gaugeForce(None, 6.0))
link, sten = stats([r["stout_link"] for r in rows]), stats([r["stout_stencil"] for r in rows])
flop = 37 * 216 * 4.0 * vol
out(what="backward", link_ms=link, stencil_ms=sten, action_deriv_ms=stats([r["staple"] for r in rows]),
    stencil_gbytes_bound=2304.0 * vol / 1e9, stencil_ms_of_the_bound_at_copy_rate=2304.0 * vol / copy_gbs / 1e6,
    stencil_fraction_of_2304_bound=2304.0 * vol / copy_gbs / 1e6 / sten["median"],
    stencil_fraction_of_2880_moved=2880.0 * vol / copy_gbs / 1e6 / sten["median"],
    stencil_tflops=flop / sten["median"] / 1e9, stencil_fraction_of_fp64_peak=flop / sten["median"] / 1e9 / (FP64_PEAK / 1e12),
    link_gbytes=6 * 576.0 * vol / 1e9, link_fraction_of_copy_rate=6 * 576.0 * vol / copy_gbs / 1e6 / link["median"])
sf = q.stoutSmearGetForce(ctx, None, None, [0.1, 0.09, 0.12])
rows = kernel_ms(["stout_link", "stout_stencil", "staple", "gauge_halo"], lambda: sf.gaugeForce(None, 6.0))
out(what="force3", wall_ms=stats([r["wall"] for r in rows]), link_ms=stats([r["stout_link"] for r in rows]),
    stencil_ms=stats([r["stout_stencil"] for r in rows]), action_deriv_ms=stats([r["staple"] for r in rows]))
sf.release()

fl, u = np.zeros_like(g), np.zeros_like(g)
q.stoutSmear(ctx, g, 0.02, fl)
ss = q.newStoutSmear(ctx, 0.02)
rows = kernel_ms(["stout_inverse"], lambda: ss.inverse(u, fl, maxIter=8), reps=3)
it = stats([r["stout_inverse"] / 8 for r in rows])
out(what="inverse", ms_per_iteration=it, flow_stage_ms=stage["median"], iterations_timed=8,
    gbytes_per_iteration_algorithmic=5 * 576.0 * vol / 1e9, fraction_of_copy_rate=5 * 576.0 * vol / copy_gbs / 1e6 / it["median"])
