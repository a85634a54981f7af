#!/usr/bin/env python
"""src/observables/scalarTrace.nim through libqexhip: the stochastic scalar-density trace Tr (D+m)^-1(x,x) (disconnected pbp) from
noise sources diluted in time and even/odd or the eight 3-d corners.

    python examples/scalar_trace.py [-inlat FILE | -lat 4 4 4 8] [-outfn output] [-mass 0.1] [-sloppy 0] [-half 0] [-cg_prec 1e-9]
                                    [-cg_max 100000] [-num_stoch 1] [-improved_trace 1] [-source_type Z4] [-dilute_type EO]
                                    [-seed N] [-smear 0] [-batch 4] [-nev 0] [-nvecs N] [-cheb 12] [-cheb_lo 0.3] [-lma 0]
    python -m torch.distributed.run --nproc-per-node N examples/scalar_trace.py ...     # t-sharded over N ranks

The parameters are the reference program's.  Without -inlat the configuration is g.random of the seed's RngMilc6 field, whose
streams then go on into the noise, as there; -smear 1 builds the operator on nHYP(0.4, 0.5, 0.5) links (the reference always
smears).  The noise is drawn, diluted, solved in lock-step batches of -batch patterns and contracted on the device
(qex_amd.scalarTrace); each trace is written as one SciDAC record of 16-byte sites, read back, and its per-timeslice sums are
printed once more, as `loadsrc` lines.  -sloppy 1 or 2 solves in mixed precision: one rank only unless -batch_ranks 1 is
given (the context option "batch_ranks" on every rank: the batches run t-sharded); -half 1 lets -sloppy 2 iterate on
16-bit storage (the context options "half" and "half_batch"; default 0: it runs single).  -nev N computes the N lowest
eigenpairs of the even/odd operator once (Staggered.eigs; -nvecs, -cheb, -cheb_lo as in examples/stag_eigs.py) and deflates every
batch with them, the odd-parity patterns included; the first source is then also solved without deflation and the eigensolve
time and the iterations with / without deflation are printed.  -lma 1 (needs -nev > 0; not in the reference) averages those modes
exactly: their part L(x) of the trace is computed once without noise, every solution is projected off them before it is contracted,
and the exact part is printed once as `lowsrc ... timeslice t pbp` lines."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import qex_amd as q  # noqa: E402

# what the reference's writer puts into the record for an lo.Complex field: "QDP_" & name(IOtype) (src/io/qioInternal.nim:37-40,
# writerQiolite.nim:134) with IOtype = DComplex = ComplexProxy[ComplexObj[float64, float64]] (qcdTypes.nim:66, complexType.nim:11-21)
TRACE_DATATYPE = "QDP_ComplexProxy[ComplexObj[system.float64, system.float64]]"

ap = argparse.ArgumentParser()
ap.add_argument("-inlat", default="")
ap.add_argument("-lat", type=int, nargs=4, default=[4, 4, 4, 8])
ap.add_argument("-outfn", default="output")
ap.add_argument("-mass", type=float, default=0.1)
ap.add_argument("-sloppy", type=int, default=0, choices=[0, 1, 2])
ap.add_argument("-half", type=int, default=0, choices=[0, 1], help="1: -sloppy 2 iterates on 16-bit storage (options half, half_batch)")
ap.add_argument("-batch_ranks", type=int, default=0, choices=[0, 1],
                help="1: on more than one rank, -sloppy 1 / 2 runs the mixed-precision lock-step batches t-sharded (option batch_ranks)")
ap.add_argument("-cg_prec", type=float, default=1e-9)
ap.add_argument("-cg_max", type=int, default=100000)
ap.add_argument("-num_stoch", type=int, default=1)
ap.add_argument("-improved_trace", type=int, default=1, choices=[0, 1])
ap.add_argument("-source_type", default="Z4", choices=["Z4", "Z2", "U1", "Gauss"])
ap.add_argument("-dilute_type", default="EO", choices=["EO", "CORNER"])
ap.add_argument("-seed", type=int, default=int(1000 * time.time()))
ap.add_argument("-smear", type=int, default=0, choices=[0, 1])
ap.add_argument("-batch", type=int, default=4, choices=[1, 2, 3, 4])
ap.add_argument("-nev", type=int, default=0, help="deflate every batch with this many low modes (0: no eigensolve)")
ap.add_argument("-nvecs", type=int, default=0, help="size of the Lanczos basis (default max(2 nev, nev + 8))")
ap.add_argument("-cheb", type=int, default=12, help="Chebyshev degree (0: plain Lanczos)")
ap.add_argument("-cheb_lo", type=float, default=0.3)
ap.add_argument("-lma", type=int, default=0, choices=[0, 1],
                help="1: low-mode averaging with the -nev modes (needs -nev > 0): their part of the trace is summed exactly")
a = ap.parse_args()
if a.lma and a.nev <= 0:
    sys.exit("scalar_trace.py: -lma 1 needs -nev > 0 (the low modes that are averaged exactly)")
if a.sloppy and int(os.environ.get("WORLD_SIZE", "1")) > 1 and not a.batch_ranks:
    sys.exit("scalar_trace.py: -sloppy %d needs a single rank: the mixed-precision lock-step batch is not built for t-sharded "
             "lattices (run without -sloppy, or on one rank)" % a.sloppy)

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
print("rank %d/%d" % (rank, world))
imp = "1" if a.improved_trace else "0"
metadata_prefix = "l%d.t%d.m%s.cfg%s" % (glat[0], nt, a.mass, a.inlat)


def trace_file(i):
    return "%s.trace%d.%s.imp%s.%s" % (a.outfn, i, a.source_type, imp, a.dilute_type)


def trace_meta(i):
    return "%s.type%s.src%d.imp%s.%s" % (metadata_prefix, a.source_type, i, imp, a.dilute_type)


g = q.loadGaugeSlab(a.inlat, glat, rank * lt, lt) if a.inlat else rng.random()
print("latsize = ", glat)
print("volume = ", glo.vol)
q.reunit(ctx, g)                                                       # g.projectSU
p = q.plaq(ctx)
print("plaq ", list(p))
print("plaq ss: ", 2.0 * (p[0] + p[1] + p[2]), " st: ", 2.0 * (p[3] + p[4] + p[5]), " tot: ", p.sum())
if a.smear:
    print("smear = HypCoefs(alpha1: 0.4, alpha2: 0.5, alpha3: 0.5)")
    s = q.Staggered(ctx, g, smear=q.HypCoefs(0.4, 0.5, 0.5), bc="pppa")       # sg.setBC; sg.stagPhase; sg.newStag
else:
    q.rephase(lo, g, t_offset=rank * lt, t_global=nt)
    s = q.newStag(ctx, g)
print("links per site, storage format, max deviation:", s.links_info())

defl = {}
if a.nev > 0:
    t0 = time.perf_counter()
    B = s.eigs(a.nev, nvecs=a.nvecs or None, cheb_degree=a.cheb, cheb_lo=a.cheb_lo)
    ctx.sync()
    print("eigs: nconv %d of %d in %.3f s; %s" % (B.nconv, a.nev, time.perf_counter() - t0, B.stats))
    defl = dict(deflate=B, nev=a.nev)
    # the first source once more without deflation, on a copy of the generator's state: the iterations deflation saves
    state = rng.state()
    _, _, st0 = q.scalarTrace(s, lo, rng, a.mass, a.cg_prec * a.cg_prec, maxits=a.cg_max, num_stoch=1, source_type=a.source_type,
                              dilute_type=a.dilute_type, improved_trace=bool(a.improved_trace), t_offset=rank * lt, sloppy=a.sloppy,
                              batch=a.batch, out=None)
    rng.set_state(state)
    if a.lma:
        defl["lma"] = True
t0 = time.perf_counter()
traces, ests, st = q.scalarTrace(s, lo, rng, a.mass, a.cg_prec * a.cg_prec, maxits=a.cg_max, num_stoch=a.num_stoch,
                                 source_type=a.source_type, dilute_type=a.dilute_type, improved_trace=bool(a.improved_trace),
                                 t_offset=rank * lt, sloppy=a.sloppy, batch=a.batch, **defl)
total = time.perf_counter() - t0
if a.nev > 0:
    print("iterations of source 0: %d with %d modes, %d without (%.4f s of solves without)" %
          (sum(st["iterations"][0]), a.nev, sum(st0["iterations"][0]), st0["solve_s"]))
print("solves: %.4f s, dilution + contraction + slice sums: %.6f s (%.3f %% of the measurement, %.4f s)" %
      (st["solve_s"], st["contract_s"], 100.0 * st["contract_s"] / total, total))
print("iterations per pattern:", st["iterations"])
if a.lma:
    print("low-mode averaging: L(x) of %d modes in %.4f s, projections %.4f s" % (a.nev, st["lowmode_s"], st["project_s"]))
    for t in range(nt):
        print("lowsrc mom 0 0 0 timeslice %d pbp %r" % (t, float(st["low_est"][t])))

spatv = glat[0] * glat[1] * glat[2]
for i in range(a.num_stoch):
    tr = traces[i]
    if dist is not None:                       # the slabs go to rank 0, which holds the file
        parts = [None] * world
        dist.all_gather_object(parts, tr)
        tr = np.zeros((glo.vol, 2))
        for r in range(world):
            tr[glo.shard_indices(world, r)[1]] = parts[r]
    if rank == 0:
        q.writeField(np.ascontiguousarray(tr), glat, trace_file(i), filemd=trace_meta(i), recordmd=trace_meta(i),
                     datatype=TRACE_DATATYPE, colors=3)
# Test loading traces
for i in range(a.num_stoch):
    if rank != 0:
        continue
    tr, dt = q.readField(trace_file(i), glat, (2,))
    fmd, rmd = q.fileMetadata(trace_file(i))
    print("File metadata for trace %d: %s" % (i, fmd))
    print("Trace metadata for trace %d: %s" % (i, rmd))
    est = np.zeros(nt)
    np.add.at(est, glo.coords[:, 3], tr[:, 0])
    for t in range(nt):
        print("loadsrc %d mom 0 0 0 timeslice %d pbp %r" % (i, t, float(est[t] / spatv)))
if dist is not None:
    dist.barrier()
ctx.close()
