#!/usr/bin/env python3
"""The numbers of DESIGN.md section 4 "Mixed-precision batches on t-sharded lattices": the lock-step batches of four under option
"batch_ranks" = 1 on a lattice split along t over the ranks of one job, against their two yardsticks FROM THE SAME RUN -- the sharded
fp64 batch and four single-system sharded sloppy solves.  Started under the launcher, one process per rank:

    python -m torch.distributed.run --nproc-per-node 2 profiles/sloppy_batch_ranks_measure.py [-cases 48x96-random,48x96-hisq,32x32-random]

On a one-GPU machine the ranks share the device and talk over the peer-memory transport: nothing here crosses xGMI, and ranks on
distinct GPUs are NOT measured by this.

Four gaussian sources without an odd part on resident fields, so that the batched full solve (dev_solve_batch: reconstruct-right) is one
solveEE batch plus a handful of fp64 sweeps around it -- a cost the batch arms carry and the single-system solveEE arms do not.  Arms,
alternated within every round:
  fp64_batch    dev_solve_batch, sloppy = 0
  f32_batch     dev_solve_batch, sloppy = 1
  half_batch    dev_solve_batch, sloppy = 2 with "half_batch" = 1
  f32_single    four dev_solve_xx_sloppy in a row, SloppySingle
  half_single   four dev_solve_xx_sloppy in a row, SloppyHalf with "half" = 1

  per_iteration   microseconds per lock-step iteration (of four systems): ITS iterations at r2req = 0 with half_stall out of reach, REPS
                  rounds behind one warm-up round; median, minimum and maximum of the rounds.  For the single arms: the four solves' time
                  over ITS, i.e. the cost of advancing four systems by one iteration
  solve           time to r2req 1e-14 at m = 0.1 and m = 0.01 sqrt(2) for the four systems: iterations, reliable updates, fall-backs,
                  milliseconds (once each, behind the rounds above)
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

ITS, REPS, N = 100, 5, 4
ARMS = ("fp64_batch", "f32_batch", "half_batch", "f32_single", "half_single")
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
        for name in ("half", "half_batch", "batch_ranks"):
            ctx.set_option(name, 1)
        fb, fx = [ctx.field_new() for _ in range(N)], [ctx.field_new() for _ in range(N)]
        for f in fb:
            rng.dev_gaussian_vector(ctx, f)
            ctx.dev_zero(f, "odd")
        out(what="links", case=case, lat=glat, local_lat=lat, info=s.links_info(), f32=ctx.links_info_f32(), half=ctx.links_info_half(),
            sweep=ctx.sweep_info())

        def timed(arm, mass, r2req, maxits):
            """(iterations, r2, updates, fall-backs, ms) of the four systems"""
            dist.barrier()
            ctx.sync()
            t0 = time.perf_counter()
            if arm.endswith("_batch"):
                sl = ARMS.index(arm)
                its, fin, nup = ctx.dev_solve_batch(fx, fb, [mass] * N, r2req, maxits, sloppy=sl)
                ms = (time.perf_counter() - t0) * 1e3
                fell = [l["fell_back"] for l in ctx.sloppy_last_batch()] if sl else []
            else:
                sl, its, fin, nup, fell = (1 if arm == "f32_single" else 2), [], [], [], []
                for j in range(N):
                    i, f, u = ctx.dev_solve_xx_sloppy(fx[j], fb[j], mass, r2req, maxits, True, sl)
                    its.append(i), fin.append(f), nup.append(u), fell.append(ctx.sloppy_last()["fell_back"])
                ms = (time.perf_counter() - t0) * 1e3
            return its, fin, nup, fell, ms

        # microseconds per lock-step iteration: a fixed count, no stop, no hand-over to fp32
        ctx.set_option("half_stall", 1 << 20)
        us = {arm: [] for arm in ARMS}
        for rep in range(REPS + 1):
            for arm in ARMS:
                its, fin, nup, fell, ms = timed(arm, 0.1, 0.0, ITS)
                assert min(its) == max(its) == ITS and not any(fell), (arm, its, fell)
                if rep:
                    us[arm].append(ms * 1e3 / ITS)
        for arm in ARMS:
            v = us[arm]
            out(what="per_iteration", case=case, arm=arm, systems=N, iterations=ITS, rounds=REPS, us_median=round(statistics.median(v), 1),
                us_min=round(min(v), 1), us_max=round(max(v), 1))
        ctx.set_option("half_stall", 2)
        # time to r2req 1e-14
        for mass in (0.1, 0.01 * np.sqrt(2.0)):
            for arm in ARMS:
                its, fin, nup, fell, ms = timed(arm, mass, 1e-14, 20000)
                out(what="solve", case=case, mass=mass, arm=arm, iterations=its, updates=nup, fell_back=fell, r2_over_b2=fin, ms=round(ms, 2))
        for f in fb + fx:
            ctx.field_free(f)
        ctx.close()
    dist.barrier()


if __name__ == "__main__":
    main()
