#!/usr/bin/env python3
"""The numbers of DESIGN.md section 4 "16-bit storage on t-sharded lattices": SloppyHalf with option "half" = 1 against SloppySingle
and the fp64 CG on a lattice split along t over the ranks of one job.  Started under the launcher, one process per rank:

    python -m torch.distributed.run --nproc-per-node 2 profiles/half_ranks_measure.py [-cases 48x96-random,48x96-hisq,32x32-random]

(what tests/ranks.py launch() runs).  On a one-GPU machine the ranks share the device and talk over the peer-memory transport: nothing
here crosses xGMI.  The yardstick is SloppySingle in the same run: with "half" = 0 -- and before 16-bit storage ran on sharded
lattices -- SloppyHalf on such a context IS that solve.

  per_iteration   microseconds per CG iteration of fp64, SloppySingle and SloppyHalf on resident fields: ITS iterations at r2req = 0
                  (no stop on the residual) with half_stall out of reach, the three alternated, REPS rounds behind one warm-up round;
                  median, minimum and maximum of the rounds
  solve           time to r2req 1e-14 at m = 0.1 and m = 0.01 sqrt(2): iterations, reliable updates, milliseconds, and whether the
                  16-bit solve's stall guard fired (once each, behind the rounds above)
  copy_bandwidth  k_copy16 of libqexhip_tune over 1 GiB on rank 0 alone, the other ranks idle

one JSON line per measurement from rank 0 on stdout; wall times are host clocks around calls that end in a device synchronise, taken
behind a barrier of the ranks."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ITS, REPS = 200, 5
SOLVERS = (("fp64", 0), ("single", 1), ("half", 2))
CASES = {"48x96-random": ([48, 48, 48, 96], "random"), "48x96-hisq": ([48, 48, 48, 96], "hisq"), "32x32-random": ([32, 32, 32, 32], "random")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-cases", default=",".join(CASES))
    a = ap.parse_args()
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch.distributed as dist

    dist.init_process_group("gloo")
    world, rank = dist.get_world_size(), dist.get_rank()
    import qex_amd as q
    from qex_amd import _lib

    def out(**kw):
        if rank == 0:
            print(json.dumps(kw), flush=True)

    first = True
    for case in a.cases.split(","):
        glat, links = CASES[case]
        lt = glat[3] // world
        lat = glat[:3] + [lt]
        ctx = q.Context(lat, device=rank % q.device_count(), rank_geom=(1, 1, 1, world), rank_coord=(0, 0, 0, rank))
        uid = [q.Context.unique_id() if rank == 0 else None]
        dist.broadcast_object_list(uid, src=0)
        ctx.comm_init(uid[0], world, rank)
        if first:
            out(what="device", info=ctx.info(), ranks=world, transport=ctx.comm_transport()[0])
            if rank == 0:
                gbs = C.c_double(0)
                _lib.tune_lib().qexhip_tune_stream(ctx._h, 1, 1024, 2048, 5, C.byref(gbs))
                out(what="copy_bandwidth", kernel="k_copy16 1 GiB, rank 0 alone", gbytes_per_s=gbs.value)
            dist.barrier()
            first = False
        rng = q.RngField(lat, q.RngMilc6, 987654321, glat=glat, t_offset=rank * lt)
        lo = q.Layout(lat)
        if links == "random":
            g = rng.random()
            q.rephase(lo, g, t_offset=rank * lt, t_global=glat[3])
            s = q.newStag(ctx, g)
        else:
            g = rng.warm(0.3)
            q.rephase(lo, g, t_offset=rank * lt, t_global=glat[3])
            s = q.Staggered(ctx, g, smear=q.HisqCoefs().init())
        ctx.set_option("half", 1)
        fb, fx = ctx.field_new(), ctx.field_new()
        rng.dev_gaussian_vector(ctx, fb)
        out(what="links", case=case, lat=glat, local_lat=lat, info=s.links_info(), f32=ctx.links_info_f32(), half=ctx.links_info_half(),
            sweep=ctx.sweep_info())

        def timed(sl, mass, r2req, maxits):
            dist.barrier()
            ctx.sync()
            t0 = time.perf_counter()
            its, fin, nup = ctx.dev_solve_xx_sloppy(fx, fb, mass, r2req, maxits, True, sl)
            ms = (time.perf_counter() - t0) * 1e3
            return its, fin, nup, ms, (ctx.sloppy_last() if sl else {})

        # microseconds per iteration: a fixed count, no stop, no hand-over to fp32
        ctx.set_option("half_stall", 1 << 20)
        us = {name: [] for name, _ in SOLVERS}
        for rep in range(REPS + 1):
            for name, sl in SOLVERS:
                its, fin, nup, ms, last = timed(sl, 0.1, 0.0, ITS)
                assert its == ITS and (sl != 2 or (last["precision"] == 2 and last["fell_back"] == 0)), (name, its, last)
                if rep:
                    us[name].append(ms * 1e3 / ITS)
        for name, _ in SOLVERS:
            v = us[name]
            out(what="per_iteration", case=case, solver=name, iterations=ITS, rounds=REPS, us_median=round(statistics.median(v), 1),
                us_min=round(min(v), 1), us_max=round(max(v), 1))
        ctx.set_option("half_stall", 2)
        # time to r2req 1e-14
        for mass in (0.1, 0.01 * np.sqrt(2.0)):
            for name, sl in SOLVERS:
                its, fin, nup, ms, last = timed(sl, mass, 1e-14, 20000)
                out(what="solve", case=case, mass=mass, solver=name, iterations=its, updates=nup, r2_over_b2=fin, ms=round(ms, 2), **last)
        ctx.field_free(fb)
        ctx.field_free(fx)
        ctx.close()
    dist.barrier()


if __name__ == "__main__":
    main()
