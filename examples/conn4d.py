#!/usr/bin/env python
"""src/observables/conn4d.nim through libqexhip: the connected part of the flavour-singlet scalar correlator from point sources at
random (or given) points, each propagator's |phi|^2 translated so that its source lands on the origin.

    python examples/conn4d.py [-inlat FILE | -lat 4 4 4 8] [-outfn scprop.out] [-mass 0.1] [-sources x y z t x y z t ...]
                              [-cg_prec 1e-9] [-cg_max 100000] [-num_source 16] [-sq_min_distance N] [-seed N] [-sloppy 2]
                              [-half 0] [-batch 4] [-nev 0]
    python -m torch.distributed.run --nproc-per-node N examples/conn4d.py -sloppy 0 ...     # t-sharded over N ranks

The parameters are the reference program's, -sloppy 2 (SloppyHalf) by default as there.  Without -inlat the configuration is the
unit gauge.  The links are re-unitarised, nHYP(0.4, 0.5, 0.5) smeared and given the antiperiodic boundary in t and the staggered
phases on the device; the points come from -sources or from randomPoint on the global RngMilc6 stream of the seed (every rank draws
the same points); the 3 * num_source point sources are built, solved in lock-step batches of -batch systems and contracted on the
device (qex_amd.connMeson).  locmes is written as one SciDAC record of 8-byte sites.  -sloppy 1 or 2 solves in mixed precision: one
rank only unless -batch_ranks 1 is given (the context option "batch_ranks" on every rank: the batches run t-sharded); -half 1 lets -sloppy 2 iterate on 16-bit storage (the context options "half" and "half_batch"; default 0: it runs
single).  -nev N computes the N lowest eigenpairs of the even/odd operator once and deflates every batch with them."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import qex_amd as q  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("-inlat", default="")
ap.add_argument("-lat", type=int, nargs=4, default=[4, 4, 4, 8])
ap.add_argument("-outfn", default="scprop.out")
ap.add_argument("-mass", type=float, default=0.1)
ap.add_argument("-sources", type=int, nargs="*", default=[], help="use specific source locations: x y z t of every point")
ap.add_argument("-cg_prec", type=float, default=1e-9)
ap.add_argument("-cg_max", type=int, default=100000)
ap.add_argument("-num_source", type=int, default=0, help="number of point sources (default: those of -sources, else 16)")
ap.add_argument("-sq_min_distance", type=int, default=None)
ap.add_argument("-seed", type=int, default=int(1000 * time.time()))
ap.add_argument("-sloppy", type=int, default=2, choices=[0, 1, 2])
ap.add_argument("-half", type=int, default=0, choices=[0, 1], help="1: -sloppy 2 iterates on 16-bit storage (options half, half_batch)")
ap.add_argument("-batch_ranks", type=int, default=0, choices=[0, 1],
                help="1: on more than one rank, -sloppy 1 / 2 runs the mixed-precision lock-step batches t-sharded (option batch_ranks)")
ap.add_argument("-batch", type=int, default=4, choices=[1, 2, 3, 4])
ap.add_argument("-nev", type=int, default=0, help="deflate every batch with this many low modes (0: no eigensolve)")
a = ap.parse_args()
if len(a.sources) % 4 != 0:
    sys.exit("sources should be an integer array with its length divisable by 4\n  received: %s" % (a.sources,))
if a.sloppy and int(os.environ.get("WORLD_SIZE", "1")) > 1 and not a.batch_ranks:
    sys.exit("conn4d.py: -sloppy %d needs a single rank: the mixed-precision lock-step batch is not built for t-sharded "
             "lattices (run with -sloppy 0, or on one rank)" % a.sloppy)

world, rank, dist = 1, 0, None
if int(os.environ.get("WORLD_SIZE", "1")) > 1:
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch.distributed as dist

    dist.init_process_group("gloo")
    world, rank = dist.get_world_size(), dist.get_rank()
if a.inlat and not os.path.exists(a.inlat):
    print("Nonexistent gauge file: ", a.inlat)
    a.inlat = ""
glat = q.getFileLattice(a.inlat) if a.inlat else list(a.lat)
nt = glat[3]
lt = nt // world
lat = glat[:3] + [lt]
glo, lo = q.Layout(glat), q.Layout(lat)
num_source = a.num_source or (len(a.sources) // 4 if a.sources else 16)
sq_min_distance = a.sq_min_distance if a.sq_min_distance is not None else q.defaultSqMinDistance(glat, num_source)
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
else:
    ctx = q.Context(lat)
    if a.half:
        ctx.set_option("half", 1)
        ctx.set_option("half_batch", 1)
if rank != 0:
    sys.stdout = open(os.devnull, "w")            # one log, rank 0's
print(ctx.info(), "ranks", world)
print("rank %d/%d" % (rank, world))
metadata_prefix = "l%d.t%d.m%s" % (glat[0], nt, a.mass)
R = q.GlobalRng(a.seed, 987654321)                # global RNG: the same stream on every rank

g = q.loadGaugeSlab(a.inlat, glat, rank * lt, lt) if a.inlat else q.unit(lo)
print("latsize = ", glat)
print("volume = ", glo.vol)


def checkSU(g):
    """gaugeUtils.nim:1407-1422: sqrt of the mean / of the largest |U^+ U - 1|^2 + |det U - 1|^2 per link, over 2 (nc^2 + 1)"""
    u = (g[..., 0] + 1j * g[..., 1]).reshape(-1, 3, 3)
    d = (np.abs(np.einsum("nki,nkj->nij", u.conj(), u) - np.eye(3)) ** 2).sum(axis=(1, 2)) + np.abs(np.linalg.det(u) - 1.0) ** 2
    s, m = float(d.sum()), float(d.max())
    if dist is not None:
        parts = [None] * world
        dist.all_gather_object(parts, (s, m))
        s, m = sum(p[0] for p in parts), max(p[1] for p in parts)
    c = 2.0 * (3 * 3 + 1)
    return np.sqrt(s / (c * 4 * glo.vol)), np.sqrt(m / c)


def printPlaq():
    p = q.plaq(ctx, g)
    print("plaq ", list(p))
    print("plaq ss: ", 2.0 * (p[0] + p[1] + p[2]), " st: ", 2.0 * (p[3] + p[4] + p[5]), " tot: ", p.sum())


d = checkSU(g)
print("unitary deviation avg: ", d[0], " max: ", d[1])
printPlaq()
q.reunit(ctx, g)                                                       # g.projectSU
d = checkSU(g)
print("new unitary deviation avg: ", d[0], " max: ", d[1])
printPlaq()
print("smear = HypCoefs(alpha1: 0.4, alpha2: 0.5, alpha3: 0.5)")
s = q.Staggered(ctx, g, smear=q.HypCoefs(0.4, 0.5, 0.5), bc="pppa")       # sg.smear g; sg.setBC; sg.stagPhase; sg.newStag
print("links per site, storage format, max deviation:", s.links_info())

pts = []
if a.sources:
    if len(a.sources) < 4 * num_source:
        sys.exit("exhauseted provided sources.")
    pts = [a.sources[4 * i:4 * i + 4] for i in range(num_source)]
else:
    for _ in range(num_source):
        q.randomPoint(R, glat, pts, sq_min_distance)
for i, pt in enumerate(pts):
    print("point source %d, living at %s." % (i, pt))

defl = {}
if a.nev > 0:
    t0 = time.perf_counter()
    B = s.eigs(a.nev)
    ctx.sync()
    print("eigs: nconv %d of %d in %.3f s; %s" % (B.nconv, a.nev, time.perf_counter() - t0, B.stats))
    defl = dict(deflate=B, nev=a.nev)
t0 = time.perf_counter()
locmes, est, st = q.connMeson(s, lo, pts, a.mass, a.cg_prec * a.cg_prec, maxits=a.cg_max, t_offset=rank * lt, sloppy=a.sloppy,
                              batch=a.batch, **defl)
total = time.perf_counter() - t0
print("solves: %.4f s, sources + accumulation + sign + slice sums: %.6f s (%.3f %% of the measurement, %.4f s)" %
      (st["solve_s"], st["contract_s"], 100.0 * st["contract_s"] / total, total))
print("iterations per system:", st["iterations"])
for t in range(nt):
    print("%d  %r" % (t, float(est[t])))

if dist is not None:                       # the slabs go to rank 0, which holds the file
    parts = [None] * world
    dist.all_gather_object(parts, locmes)
    locmes = np.zeros(glo.vol)
    for r in range(world):
        locmes[glo.shard_indices(world, r)[1]] = parts[r]
if rank == 0:
    # "QDP_" & name(IOtype) (src/io/qioInternal.nim:37-40) with float64 sites for an lo.Real field written with precision "D"
    q.writeField(np.ascontiguousarray(locmes), glat, a.outfn, filemd=metadata_prefix, recordmd=metadata_prefix,
                 datatype="QDP_float64", colors=3)
if dist is not None:
    dist.barrier()
ctx.close()
