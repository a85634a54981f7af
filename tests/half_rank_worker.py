"""Worker of tests/test_gpu_half_ranks.py: SloppyHalf on 16-bit storage (option "half" = 1) on a t-sharded lattice.

Started by torch.distributed.run, one process per rank, every rank on device 0 (the peer-memory transport between processes that
share one GPU).  Every rank builds the same GLOBAL problem with the oracle, hands its t-slab to a sharded context, and keeps a
one-rank context of the whole lattice with "half" = 1 beside it as the reference.

  --op      the 16-bit operator: dev_op_xx_half on the slab equals the slab of the one-rank dev_op_xx_half, bit for bit, for g.random
            links (format 1), g.random fat + Naik links (format 1, ghost depth 3) and HISQ links (format 0: the scales are the largest
            |entry| of the WHOLE lattice), both parities, in the sweep forms exchange-first (overlap 0), split by sites (overlap 1,
            hop_split 0) and overlap 1 with hop_split 2 (no fused 16-bit sweep: it runs split by sites); links_info_half on every
            rank is the one-rank (format, s_fat, s_long); launches and exchanges are counted from the timers
  --solve   solveEE and the full solve (ReconL, and ReconR on a source with no odd part) to r2req 1e-8 and 1e-14 at mass 0.1 on
            g.random links: the true residual of the gathered solution, recomputed by the oracle's fp64 operator, is <= r2req; every
            rank reports the same iterations, updates, sloppy_last and r2; precision 2; the iteration count is the one-rank 16-bit
            solve's to within max(5, its // 20); with half_stall = 0 every rank falls back to fp32 alike; with maxits = 10 every rank
            stops at 10

usage: python -m torch.distributed.run --nproc-per-node N half_rank_worker.py LX LY LZ LT [--op] [--solve]
Exit status 0 and one line `HALF_RANKS_OK [json per rank]` from rank 0, non-zero on the first failed check.
"""
import argparse
import json
import sys

import numpy as np

import ranks

SEED = 987654321
FORMS = (("exchange_first", 0, 0), ("by_sites", 1, 0), ("fused_requested", 1, 2))     # (name, overlap, hop_split)


def margin(its):
    """iterations a sharded 16-bit solve may differ from the one-rank one by (tests/test_gpu_half_ranks.py says where it comes from)"""
    return max(5, its // 20)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lat", type=int, nargs=4)
    ap.add_argument("--op", action="store_true")
    ap.add_argument("--solve", action="store_true")
    args = ap.parse_args()
    w = ranks.shard(args.lat)
    rank, world, dist, ctx, loc, idx, sl = w
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
    ref = q.Context(glat, device=0)                                   # the one-rank 16-bit operator / solve on the whole lattice
    ref.set_option("half", 1)
    ctx.set_option("half", 1)
    res = {"rank": rank}

    def stag(c, f, l, slab):
        return q.newStag3(c, sl(f) if slab else f, sl(l) if slab else l) if l is not None else q.newStag(c, sl(f) if slab else f)

    def op(c, src, m2, par_even):
        fx, fr = c.field_new(src), c.field_new()
        c.dev_op_xx_half(fr, fx, m2, par_even)
        r = c.field_download(fr)
        c.field_free(fx)
        c.field_free(fr)
        return r

    if args.op:
        res["op"] = {}
        for kind, (f, l, fmt) in links.items():
            stag(ref, f, l, False)
            want = {pe: op(ref, b, m2, pe) for pe, m2 in ((True, 0.01), (False, 0.04))}
            info1 = ref.links_info_half()
            assert info1[0] == fmt, (kind, info1)
            for name, overlap, hop_split in FORMS:
                ctx.set_option("overlap", overlap)
                ctx.set_option("hop_split", hop_split)
                stag(ctx, f, l, True)                                  # collective set_links (+ the sweep measurement)
                info = ctx.links_info_half()                           # collective: the 16-bit copy is rebuilt here
                print("rank %d %s/%s: links_info_half %r (one rank %r)" % (rank, kind, name, info[:3], info1[:3]), file=sys.stderr, flush=True)
                assert info[:3] == info1[:3], (kind, name, info, info1)
                ctx.timers_enable(3)
                ctx.timers_reset()
                for pe, m2 in ((True, 0.01), (False, 0.04)):
                    r = op(ctx, sl(b), m2, pe)
                    if not np.array_equal(r, sl(want[pe])):
                        d = np.abs(r - sl(want[pe])).max()
                        raise AssertionError("rank %d %s %s par_even=%s: sharded 16-bit operator differs from the one-rank one (max %g)"
                                             % (rank, kind, name, pe, d))
                nbnd, nint, nx = ctx.timer("dslash_half_bnd")[0], ctx.timer("dslash_half")[0], ctx.timer("exchange")[0]
                ctx.timers_enable(0)
                split = ctx.sweep_info()["overlap"]                    # (a slab without interior sites, Naik on Lt = 4: one launch)
                assert split == (overlap == 1 and (loc.lat[3] > 6 or l is None)), (kind, name, split)
                assert nx == nint == 4 and nbnd == (4 if split else 0), (kind, name, nx, nint, nbnd)
                res["op"]["%s/%s" % (kind, name)] = {"fmt": info[0], "s_fat": info[1], "s_long": info[2], "launches": [nint, nbnd],
                                                     "exchanges": nx}

    if args.solve:
        ctx.set_option("overlap", -1)
        ctx.set_option("hop_split", -1)
        s_sh, s_1 = stag(ctx, fat, None, True), stag(ref, fat, None, False)
        mass = 0.1
        even = slice(0, olo.vol // 2)
        b_even = b.copy()
        b_even[olo.vol // 2:] = 0                                     # no odd part: solveReconR
        res["solve"] = {}

        def gather_x(xl):
            xg = np.zeros_like(b)
            for r, xr in ranks.gather(w, (rank, xl)):
                xg[q.Layout(glat).shard_indices(world, r)[1]] = xr
            return xg

        def true_r2(what, src, xg):
            if what == "solveEE":
                ax = o.stagD2xx(olo, fat, None, xg, mass * mass, True)
                return float(np.sum((src[even] - ax[even]) ** 2) / np.sum(src[even] ** 2))
            dx = o.D(olo, fat, None, xg, mass)
            return float(np.sum((src - dx) ** 2) / np.sum(src ** 2))

        def run(what, src, r2req, maxits=5000, one_rank=True):
            """the sharded solve (and the one-rank one): this rank's record, after the checks every case shares"""
            sp = q.SolverParams(r2req=r2req, maxits=maxits, verbosity=0, sloppySolve=q.SloppyHalf)
            xl = np.zeros_like(sl(src))
            (s_sh.solveEE if what == "solveEE" else s_sh.solve)(xl, sl(src), mass, sp)
            last = ctx.sloppy_last()
            mine = {"its": sp.iterations, "nupd": sp.reliableUpdates, "r2": sp.r2, "last": last}
            if one_rank:
                sp1 = q.SolverParams(r2req=r2req, maxits=maxits, verbosity=0, sloppySolve=q.SloppyHalf)
                x1 = np.zeros_like(src)
                (s_1.solveEE if what == "solveEE" else s_1.solve)(x1, src, mass, sp1)
                mine.update(one_rank_its=sp1.iterations, one_rank_nupd=sp1.reliableUpdates, one_rank_last=ref.sloppy_last())
            mine["oracle_r2"] = true_r2(what, src, gather_x(xl))
            allr = ranks.gather(w, mine)
            print("rank %d %s r2req=%g maxits=%d: %s" % (rank, what, r2req, maxits, json.dumps(mine)), file=sys.stderr, flush=True)
            assert all((a["its"], a["nupd"], a["r2"], a["last"]) == (mine["its"], mine["nupd"], mine["r2"], mine["last"]) for a in allr), allr
            assert last["precision"] == 2 and last["half_iters"] > 0, mine
            assert last["half_iters"] + last["f32_iters"] == sp.iterations, mine
            return mine

        for what, src in (("solveEE", b), ("solve_reconL", b), ("solve_reconR", b_even)):
            for r2req in (1e-8, 1e-14):
                mine = run(what, src, r2req)
                assert mine["oracle_r2"] <= r2req * 1.001, mine
                assert mine["last"]["fell_back"] == 0 and mine["one_rank_last"]["precision"] == 2, mine
                assert abs(mine["its"] - mine["one_rank_its"]) <= margin(mine["one_rank_its"]), mine
                res["solve"]["%s/%g" % (what, r2req)] = mine
        # the stall guard at the first reliable update: every rank hands over to fp32, at the same iteration
        ctx.set_option("half_stall", 0)
        mine = run("solveEE", b, 1e-14, one_rank=False)
        assert mine["last"]["fell_back"] == 1 and mine["last"]["f32_iters"] > 0, mine
        assert mine["oracle_r2"] <= 1e-14 * 1.001, mine
        res["solve"]["fallback"] = mine
        ctx.set_option("half_stall", 2)
        # maxits: every rank stops at the same count, below convergence, without error
        mine = run("solveEE", b, 1e-14, maxits=10, one_rank=False)
        assert mine["its"] == 10 and mine["r2"] > 1e-14 and mine["last"]["fell_back"] == 0, mine
        res["solve"]["maxits"] = mine

    ranks.finish(w, "HALF_RANKS_OK", res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
