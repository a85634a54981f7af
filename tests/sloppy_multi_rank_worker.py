"""Worker of tests/test_gpu_sloppy_multi_ranks.py: the mixed-precision multi-shift CG on a t-sharded lattice.

Started by torch.distributed.run, one process per rank, every rank on device 0 (the peer-memory transport between processes that
share one GPU).  Every rank builds the same GLOBAL problem with the oracle and hands its t-slab to a sharded context.  For g.random
links, plain and with Naik links (ghost depth 3), 4 shifts at r2req 1e-14, both parities: every rank returns the same iterations,
updates, refinement iterations and residuals, and the gathered solutions' true residuals, recomputed by the oracle's fp64 operator,
are <= r2req (1 + 1e-4) and agree with the returned ones to that margin.

usage: python -m torch.distributed.run --nproc-per-node N sloppy_multi_rank_worker.py LX LY LZ LT
Exit status 0 and one line `SLOPPY_MULTI_RANKS_OK [json per rank]` from rank 0, non-zero on the first failed check.
"""
import argparse
import json
import sys

import numpy as np

import ranks

SEED = 987654321
MASSES = [0.05, 0.1, 0.2, 0.4]
R2REQ = 1e-14


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lat", type=int, nargs=4)
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
    sh = [MASSES[0]] + [4.0 * (m * m - MASSES[0] ** 2) for m in MASSES[1:]]
    h = olo.vol // 2
    res = {"rank": rank}

    def gather(xl):
        parts = [None] * world
        dist.all_gather_object(parts, (rank, xl))
        xg = np.zeros_like(b)
        for r, xr in parts:
            xg[q.Layout(glat).shard_indices(world, r)[1]] = xr
        return xg

    for kind, l3 in (("random", None), ("random_naik", lng)):
        s = q.newStag3(ctx, sl(fat), sl(l3)) if l3 is not None else q.newStag(ctx, sl(fat))      # collective set_links
        for par_even in (True, False):
            key = "%s/%s" % (kind, "even" if par_even else "odd")
            sp = q.SolverParams(r2req=R2REQ, maxits=5000, verbosity=0)
            xl = [np.zeros_like(sl(b)) for _ in sh]
            fin = s.solveXX_multi(xl, sl(b), sh, sp, parEven=par_even, sloppy=1)
            par = slice(0, h) if par_even else slice(h, 2 * h)
            b2 = float(np.sum(b[par] ** 2))
            oracle_r2 = []
            for k in range(len(sh)):
                xg = gather(xl[k])
                ax = o.stagD2xx(olo, fat, l3, xg, sh[0] ** 2 + (0.25 * sh[k] if k else 0.0), par_even)
                oracle_r2.append(float(np.sum((b[par] - ax[par]) ** 2)) / b2)
            mine = {"its": sp.iterations, "nupd": sp.reliableUpdates, "refine": sp.refineIterations, "r2": fin, "oracle_r2": oracle_r2}
            allr = [None] * world
            dist.all_gather_object(allr, mine)
            print("rank %d %s: %s" % (rank, key, json.dumps(mine)), file=sys.stderr, flush=True)
            assert len({json.dumps([a["its"], a["nupd"], a["refine"], a["r2"]]) for a in allr}) == 1, (key, allr)
            assert sp.iterations < 5000 and sp.reliableUpdates >= 1, (key, mine)
            for k in range(len(sh)):
                assert oracle_r2[k] <= R2REQ * (1.0 + 1e-4), (key, k, mine)
                assert abs(fin[k] - oracle_r2[k]) <= 1e-4 * oracle_r2[k], (key, k, mine)
            res[key] = mine

    ranks.finish(rk, "SLOPPY_MULTI_RANKS_OK", res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
