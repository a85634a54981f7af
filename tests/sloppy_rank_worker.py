"""Worker of tests/test_gpu_sloppy_ranks.py: the mixed-precision CG (SolverParams.sloppySolve) on a t-sharded lattice.

Started by torch.distributed.run, one process per rank, every rank on device 0 (the peer-memory transport between processes that
share one GPU).  Every rank builds the same GLOBAL problem with the oracle, hands its t-slab to a sharded context, and keeps a
one-rank context of the whole lattice beside it as the reference.

  --op      the fp32 operator: dev_op_xx_sloppy on the slab equals the slab of the one-rank dev_op_xx_sloppy, bit for bit, for
            g.random links (fp32 sign format), g.random fat + Naik links (ghost depth 3) and HISQ links (18 reals), both parities,
            in the sweep forms exchange-first (overlap 0), split by sites (overlap 1, hop_split 0) and overlap 1 with hop_split 2
            (the fp64 sweep's fused form: the fp32 sweep runs split by sites)
  --solve   solveEE and the full solve (ReconL, and ReconR on a source with no odd part) to r2req 1e-8 and 1e-14 at mass 0.1: the true
            residual of the gathered solution, recomputed by the oracle's fp64 operator, is <= r2req; every rank reports the same
            iterations and reliable updates; the counts are those of the one-rank sloppy solve to within a few iterations

usage: python -m torch.distributed.run --nproc-per-node N sloppy_rank_worker.py LX LY LZ LT [--op] [--solve]
Exit status 0 and one line `SLOPPY_RANKS_OK [json per rank]` from rank 0, non-zero on the first failed check.
"""
import argparse
import json
import sys

import numpy as np

import ranks

SEED = 987654321
FORMS = (("exchange_first", 0, 0), ("by_sites", 1, 0), ("fused_requested", 1, 2))     # (name, overlap, hop_split)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lat", type=int, nargs=4)
    ap.add_argument("--op", action="store_true")
    ap.add_argument("--solve", action="store_true")
    args = ap.parse_args()
    rank, world, dist, ctx, loc, idx, sl = rk = ranks.shard(args.lat)
    import qex_amd as q
    from oracle import oracle as o

    glat = list(args.lat)
    olo = o.Layout(glat)
    rf = o.RngField(olo, o.RNG_MILC6, SEED)
    fat = o.gauge_random(olo, rf)
    o.rephase(olo, fat)
    lng = o.gauge_random(olo, rf)
    o.rephase(olo, lng)
    b = o.vector_gaussian(olo, rf)
    links = {"random": (fat, None, 1), "random_naik": (fat, lng, 1)}
    if args.op:
        hfat, hlng = o.hisq_smear(olo, o.gauge_warm(olo, 0.5, rf))
        o.rephase(olo, hfat)
        o.rephase(olo, hlng)
        links["hisq"] = (hfat, hlng, 0)
    ref = q.Context(glat, device=0)                                   # the one-rank operator / solve on the whole lattice
    res = {"rank": rank}

    def stag(c, f, l, slab):
        return q.newStag3(c, sl(f) if slab else f, sl(l) if slab else l) if l is not None else q.newStag(c, sl(f) if slab else f)

    def op(c, src, m2, par_even):
        fx, fr = c.field_new(src), c.field_new()
        c.dev_op_xx_sloppy(fr, fx, m2, par_even)
        r = c.field_download(fr)
        c.field_free(fx)
        c.field_free(fr)
        return r

    if args.op:
        res["op"] = {}
        for kind, (f, l, fmt) in links.items():
            stag(ref, f, l, False)
            want = {pe: op(ref, b, m2, pe) for pe, m2 in ((True, 0.01), (False, 0.04))}
            assert ref.links_info_f32()[0] == fmt, (kind, ref.links_info_f32())
            for name, overlap, hop_split in FORMS:
                ctx.set_option("overlap", overlap)
                ctx.set_option("hop_split", hop_split)
                stag(ctx, f, l, True)                                  # collective set_links (+ the sweep measurement)
                got_fmt, got_dev = ctx.links_info_f32()
                assert got_fmt == fmt, (kind, got_fmt, got_dev)
                ctx.timers_enable(3)
                ctx.timers_reset()
                for pe, m2 in ((True, 0.01), (False, 0.04)):
                    r = op(ctx, sl(b), m2, pe)
                    if not np.array_equal(r, sl(want[pe])):
                        d = np.abs(r - sl(want[pe])).max()
                        raise AssertionError("rank %d %s %s par_even=%s: sharded fp32 operator differs from the one-rank one (max %g)"
                                             % (rank, kind, name, pe, d))
                nbnd, nint, nx = ctx.timer("dslash_f32_bnd")[0], ctx.timer("dslash_f32")[0], ctx.timer("exchange")[0]
                ctx.timers_enable(0)
                split = ctx.sweep_info()["overlap"]                    # (a slab without interior sites, Naik on Lt = 4: one launch)
                assert split == (overlap == 1 and (loc.lat[3] > 6 or l is None)), (kind, name, split)
                assert nx == nint == 4 and nbnd == (4 if split else 0), (kind, name, nx, nint, nbnd)
                res["op"]["%s/%s" % (kind, name)] = {"fmt": got_fmt, "launches": [nint, nbnd], "exchanges": nx}

    if args.solve:
        ctx.set_option("overlap", -1)
        ctx.set_option("hop_split", -1)
        s_sh, s_1 = stag(ctx, fat, None, True), stag(ref, fat, None, False)
        mass = 0.1
        even = slice(0, olo.vol // 2)
        b_even = b.copy()
        b_even[olo.vol // 2:] = 0                                     # no odd part: solveReconR
        res["solve"] = {}

        def gather(xl):
            parts = [None] * world
            dist.all_gather_object(parts, (rank, xl))
            xg = np.zeros_like(b)
            for r, xr in parts:
                xg[q.Layout(glat).shard_indices(world, r)[1]] = xr
            return xg

        for what, src in (("solveEE", b), ("solve_reconL", b), ("solve_reconR", b_even)):
            for r2req in (1e-8, 1e-14):
                sp = q.SolverParams(r2req=r2req, maxits=5000, verbosity=0, sloppySolve=q.SloppySingle)
                sp1 = q.SolverParams(r2req=r2req, maxits=5000, verbosity=0, sloppySolve=q.SloppySingle)
                xl, x1 = np.zeros_like(sl(src)), np.zeros_like(src)
                res_key = "%s/%g" % (what, r2req)
                if what == "solveEE":
                    s_sh.solveEE(xl, sl(src), mass, sp)
                    s_1.solveEE(x1, src, mass, sp1)
                else:
                    s_sh.solve(xl, sl(src), mass, sp)
                    s_1.solve(x1, src, mass, sp1)
                xg = gather(xl)
                if what == "solveEE":
                    ax = o.stagD2xx(olo, fat, None, xg, mass * mass, True)
                    r2 = float(np.sum((src[even] - ax[even]) ** 2) / np.sum(src[even] ** 2))
                else:
                    dx = o.D(olo, fat, None, xg, mass)
                    r2 = float(np.sum((src - dx) ** 2) / np.sum(src ** 2))
                mine = {"its": sp.iterations, "nupd": sp.reliableUpdates, "r2": sp.r2, "oracle_r2": r2,
                        "one_rank_its": sp1.iterations, "one_rank_nupd": sp1.reliableUpdates}
                allr = [None] * world
                dist.all_gather_object(allr, mine)
                print("rank %d %s: %s" % (rank, res_key, json.dumps(mine)), file=sys.stderr, flush=True)
                assert len({(a["its"], a["nupd"]) for a in allr}) == 1, (res_key, allr)
                assert r2 <= r2req * 1.001, (res_key, mine)
                assert abs(sp.iterations - sp1.iterations) <= max(5, sp1.iterations // 20), (res_key, mine)
                res["solve"][res_key] = mine

    ranks.finish(rk, "SLOPPY_RANKS_OK", res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
