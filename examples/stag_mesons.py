#!/usr/bin/env python
"""src/observables/fpvaMeas.nim through libqexhip: local and one-link (symmetric spatial shift) staggered meson correlators
from point-source propagators.

    python examples/stag_mesons.py [-lat 8 8 8 8] [-mass 0.1] [-t0 2] [-seed 987654321] [-warm 0.5] [-sloppy 0] [-half 0] [-batch_ranks 0]
                                   [-nev 0] [-nvecs N] [-cheb 12] [-cheb_lo 0.3]
    python -m torch.distributed.run --nproc-per-node N examples/stag_mesons.py ...     # t-sharded over N ranks

For each colour the point source at (0,0,0,t0) and its three symmetric one-link shifts are solved in one lock-step batch of four
(qexhip_dev_solve_batch), the shifted propagators are shifted back at the sink, and the four tables are contracted on the device;
no propagator leaves the GPU.  The tables are printed as printLocalMesons prints them: Walsh-Hadamard transform over the corner
bits, normalisation nt / physVol.  The configuration is the library's RngMilc6 warm start (as examples/stag_prop.py), seeded by
global site, so every partition sees the same gauge field.  -sloppy 1 runs the batches in mixed precision (fp32 iterations with
fp64 reliable updates, qexhip_dev_solve_batch_sloppy): one rank only unless -batch_ranks 1 is given (every rank then sets the
context option "batch_ranks" and the batches run t-sharded); -half 1 lets
-sloppy 2 iterate on 16-bit storage (the context options "half" and "half_batch"; default 0: it runs single).  -nev N computes the N lowest eigenpairs of the even/odd
operator once (Staggered.eigs; -nvecs, -cheb, -cheb_lo as in examples/stag_eigs.py) and deflates every batch with them; the
measurement is then also run without deflation and the eigensolve time and the iterations with / without are printed."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import qex_amd as q  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("-lat", type=int, nargs=4, default=[8, 8, 8, 8])
ap.add_argument("-mass", type=float, default=0.1)
ap.add_argument("-t0", type=int, default=2)
ap.add_argument("-seed", type=int, default=987654321)
ap.add_argument("-warm", type=float, default=0.5)
ap.add_argument("-r2req", type=float, default=1e-16)
ap.add_argument("-sloppy", type=int, default=0, choices=[0, 1, 2])
ap.add_argument("-half", type=int, default=0, choices=[0, 1], help="1: -sloppy 2 iterates on 16-bit storage (options half, half_batch)")
ap.add_argument("-batch_ranks", type=int, default=0, choices=[0, 1],
                help="1: on more than one rank, -sloppy 1 / 2 runs the mixed-precision lock-step batches t-sharded (option batch_ranks)")
ap.add_argument("-nev", type=int, default=0, help="deflate every batch with this many low modes (0: no eigensolve)")
ap.add_argument("-nvecs", type=int, default=0, help="size of the Lanczos basis (default max(2 nev, nev + 8))")
ap.add_argument("-cheb", type=int, default=12, help="Chebyshev degree (0: plain Lanczos)")
ap.add_argument("-cheb_lo", type=float, default=0.3)
a = ap.parse_args()
if a.sloppy and int(os.environ.get("WORLD_SIZE", "1")) > 1 and not a.batch_ranks:
    sys.exit("stag_mesons.py: -sloppy %d needs a single rank: the mixed-precision lock-step batch is not built for t-sharded "
             "lattices (run without -sloppy, or on one rank)" % a.sloppy)

world, rank, dist = 1, 0, None
if int(os.environ.get("WORLD_SIZE", "1")) > 1:
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch.distributed as dist

    dist.init_process_group("gloo")
    world, rank = dist.get_world_size(), dist.get_rank()
glat = list(a.lat)
lt = glat[3] // world
lat = glat[:3] + [lt]
lo = q.Layout(lat)
if world > 1:
    ctx = q.Context(lat, device=rank % q.device_count(), rank_geom=(1, 1, 1, world), rank_coord=(0, 0, 0, rank))
    uid = [q.Context.unique_id() if rank == 0 else None]
    dist.broadcast_object_list(uid, src=0)
    ctx.comm_init(uid[0], world, rank)
    if a.batch_ranks:                             # (the same options on every rank)
        ctx.set_option("batch_ranks", 1)
        if a.half:
            ctx.set_option("half", 1)
            ctx.set_option("half_batch", 1)
    rng = q.RngField(lat, q.RngMilc6, a.seed, glat=glat, t_offset=rank * lt)
else:
    ctx = q.Context(lat)
    if a.half:
        ctx.set_option("half", 1)
        ctx.set_option("half_batch", 1)
    rng = q.RngField(lat, q.RngMilc6, a.seed)
if rank != 0:
    sys.stdout = open(os.devnull, "w")            # one log, rank 0's
print(ctx.info(), "ranks", world)
g = rng.warm(a.warm)                                              # g.warm
q.rephase(lo, g, t_offset=rank * lt, t_global=glat[3])            # g.setBC; g.stagPhase
s = q.newStag(ctx, g)
print("links per site, storage format, max deviation:", s.links_info())
if a.sloppy:
    print("mixed-precision batches: fp32 link format, max deviation:", ctx.links_info_f32())
defl = {}
if a.nev > 0:
    t = time.perf_counter()
    B = s.eigs(a.nev, nvecs=a.nvecs or None, cheb_degree=a.cheb, cheb_lo=a.cheb_lo)
    ctx.sync()
    print("eigs: nconv %d of %d in %.3f s; %s" % (B.nconv, a.nev, time.perf_counter() - t, B.stats))
    defl = dict(deflate=B, nev=a.nev)
    _, _, st0 = q.localMesonTables(s, lo, a.mass, a.t0, a.r2req, t_offset=rank * lt, sloppy=a.sloppy)
t = time.perf_counter()
if a.sloppy:
    cl, cs, st = q.localMesonTables(s, lo, a.mass, a.t0, a.r2req, t_offset=rank * lt, sloppy=a.sloppy, **defl)
else:
    cl, cs, st = q.localMesonTables(s, lo, a.mass, a.t0, a.r2req, t_offset=rank * lt, **defl)
total = time.perf_counter() - t
if a.nev > 0:
    print("iterations: %d with %d modes, %d without (%.4f s of solves without)" %
          (int(np.sum(st["iterations"])), a.nev, int(np.sum(st0["iterations"])), st0["solve_s"]))
print("solves: %.4f s (iterations per colour [local, x, y, z]: %s)" % (st["solve_s"], st["iterations"]))
if a.sloppy:
    print("reliable updates per colour [local, x, y, z]: %s" % (st["updates"],))
print("contractions: %.6f s (%.3f %% of the measurement, %.4f s)" % (st["contract_s"], 100.0 * st["contract_s"] / total, total))
f = glat[3] / float(np.prod(glat))                                # nt / physVol
q.printLocalMesons(cl, f)
for mu in range(3):
    q.printLocalMesons(cs[mu], f)
if dist is not None:
    dist.barrier()
ctx.close()
