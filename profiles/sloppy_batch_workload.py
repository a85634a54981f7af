"""The mixed-precision lock-step batch against its two references on 32^4 ("Batched"):

    python profiles/sloppy_batch_workload.py mesons warm|random     wall times: the meson workload's four systems (point source and
                                                                     its three symmetric shifts), resident fields, warm, best of 3
    python profiles/sloppy_batch_workload.py n4 warm|random         four gaussian even-parity systems, r2req = 0, 200 iterations, so
                                                                     that every launch has four live systems: run under
                                                                     rocprofv3 --kernel-trace --stats for the per-kernel times
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import qex_amd as q  # noqa: E402

mode, kind = sys.argv[1], sys.argv[2]
lat = [32, 32, 32, 32]
lo = q.Layout(lat)
ctx = q.Context(lat)
rng = q.RngField(lat, q.RngMilc6, 987654321)
g = rng.warm(0.5) if kind == "warm" else rng.random()
q.rephase(lo, g)
s = q.newStag(ctx, g)
print(kind, "links:", s.links_info(), "fp32:", ctx.links_info_f32(), flush=True)


def run(name, fn, reps=3):
    fn()
    ctx.sync()                       # warm
    ts = []
    for _ in range(reps):
        ctx.sync()
        t = time.perf_counter()
        r = fn()
        ctx.sync()
        ts.append((time.perf_counter() - t) * 1e3)
    print(f"{name}: ms {['%.2f' % v for v in ts]} best {min(ts):.2f} spread {max(ts) - min(ts):.2f} -> {r}", flush=True)
    return min(ts)


if mode == "mesons":
    m, r2req, maxits = 0.1, 1e-16, 100000
    src = ctx.field_new(q.pointSource(lo, [0, 0, 0, 2], 0))
    srcs = [ctx.field_new() for _ in range(3)]
    for mu in range(3):
        ctx.dev_sym_shift(srcs[mu], src, mu)
    bs, xs, pe = [src] + srcs, [ctx.field_new() for _ in range(4)], [True, False, False, False]
    a = run("(a) fp64 dev_solve_batch", lambda: ctx.dev_solve_batch(xs, bs, [m] * 4, r2req, maxits))
    b = run("(b) 4 x dev_solve_xx_sloppy", lambda: [ctx.dev_solve_xx_sloppy(xs[j], bs[j], m, r2req, maxits, pe[j], 1) for j in range(4)])
    n = run("(new) dev_solve_batch sloppy=1", lambda: ctx.dev_solve_batch(xs, bs, [m] * 4, r2req, maxits, sloppy=1))
    print(f"speed-up over (a) {a / n:.3f}, over (b) {b / n:.3f}", flush=True)
else:
    ms = [0.1, 0.2, 0.4, 0.05]
    hb = [np.random.default_rng(j).standard_normal((lo.vol, 3, 2)) for j in range(4)]
    for b in hb:
        b[lo.vol // 2:] = 0
    hx = [np.zeros_like(b) for b in hb]
    fb, fx = [ctx.field_new(b) for b in hb], [ctx.field_new() for _ in range(4)]
    run("fp64 xx batch n=4 (host arrays)", lambda: s.solveXX_batch(hx, hb, ms, 0.0, 200, True))
    run("sloppy xx batch n=4 (host arrays)", lambda: s.solveXX_batch(hx, hb, ms, 0.0, 200, True, sloppy=1))
    run("4 x single sloppy xx", lambda: [ctx.dev_solve_xx_sloppy(fx[j], fb[j], ms[j], 0.0, 200, True, 1) for j in range(4)])
ctx.close()
