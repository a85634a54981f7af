#!/usr/bin/env python3
"""Wall time per iteration of the four reduced-precision host loops (bench.py times none of them), to hold a change that moves only
host code against a build of its parent:

    [QEXHIP_LIB=PARENT_BUILD/libqexhip.so] python3 profiles/batch_lowp_speed.py

32^4 g.random, r2req = 0 and maxits = 200 so that no solve stops early; the single solveXX and the full solve's batch of four
(dev_solve_batch: its inner lock-step solveXX), fp32 and 16-bit storage; five timed repeats behind one warm-up each, every repeat
printed (us per iteration the call reports), the median last."""
import statistics
import time

import numpy as np

from lowp_refactor_bits import setup

ITS, REPEATS = 200, 5


def main():
    import qex_amd as q

    lat = [32, 32, 32, 32]
    ctx, s, _ = setup(q, lat, "random")
    vol = int(np.prod(lat))
    fb = [ctx.field_new(np.random.default_rng(100 + j).standard_normal((vol, 3, 2))) for j in range(4)]
    fx = [ctx.field_new() for _ in range(4)]
    cases = []
    for name, sl in (("fp32", 1), ("16-bit", 2)):
        cases.append(("single %s" % name, lambda sl=sl: ctx.dev_solve_xx_sloppy(fx[0], fb[0], 0.1, 0.0, ITS, True, sl)[0]))
        cases.append(("batch n=4 %s" % name, lambda sl=sl: ctx.dev_solve_batch(fx, fb, [0.1] * 4, 0.0, ITS, sloppy=sl)[0][0]))
    for name, run in cases:
        run()
        ctx.sync()
        us = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            its = run()
            ctx.sync()
            us.append(1e6 * (time.perf_counter() - t0) / its)
        print("%-18s us/iteration %s  median %.1f" % (name, " ".join("%.1f" % v for v in us), statistics.median(us)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
