"""Worker of tests/test_gpu_gaugefix_ranks.py: gauge fixing on a t-sharded lattice.

Started by torch.distributed.run, one process per rank, every rank on device 0 (the peer-memory transport between processes that
share one GPU).  Every rank builds the same GLOBAL links (gaugefix_ref.warm_rotated), hands its t-slab to a sharded context, and
keeps a one-rank context of the whole lattice beside it as the reference.  For Coulomb and Landau gauge:
  * after 40 pure-relax iterations (gstop = 0) the rank's slab of t is np.array_equal to the slab of the one-rank t -- the relax
    update is site-local -- and the history agrees to 1e-12 (the rank sums are grouped differently);
  * the full fix (gstop 1e-8) stops after the same iterations on every rank; the gathered t has gdsq <= gstop (numpy, global) and
    is in SU(3) to 1e-12; the iterations are within 2 % (at least 2) of the one-rank fix;
  * after gaugeTransform the plaquettes equal those of the one-rank run to 1e-13.

usage: python -m torch.distributed.run --nproc-per-node N gaugefix_rank_worker.py LX LY LZ LT
Exit status 0 and one line `GAUGEFIX_RANKS_OK [json per rank]` from rank 0, non-zero on the first failed check.
"""
import json
import sys

import numpy as np

import ranks

GSTOP = 1e-8


def main():
    glat = [int(v) for v in sys.argv[1:5]]
    rank, world, dist, ctx, loc, idx, sl = rk = ranks.shard(glat)
    import qex_amd as q
    from oracle import oracle as o
    import gaugefix_ref as R

    o.build()
    glo, g = R.warm_rotated(o, tuple(glat))
    ref = q.Context(glat, device=0)
    res = {"rank": rank}

    def gather(tl):
        parts = [None] * world
        dist.all_gather_object(parts, (rank, tl))
        tg = np.zeros((glo.vol, 3, 3, 2))
        for r, tr in parts:
            tg[glo.shard_indices(world, r)[1]] = tr
        return tg

    for name, dirs in (("coulomb", R.COULOMB), ("landau", R.LANDAU)):
        q.gaugeSet(ctx, np.ascontiguousarray(g[idx]))
        q.gaugeSet(ref, g)
        t1, i1 = q.getGaugeFixTransform(ref, dirs, gstop=0.0, orf=1.8, maxits=40)
        tl, il = q.getGaugeFixTransform(ctx, dirs, gstop=0.0, orf=1.8, maxits=40)
        if not np.array_equal(tl, t1[idx]):
            raise AssertionError("rank %d %s: the slab of t differs from the one-rank t after 40 relax iterations (max %g)"
                                 % (rank, name, np.abs(tl - t1[idx]).max()))
        dh = float(np.max(np.abs(il["hist"] / i1["hist"] - 1)))
        assert il["iters"] == 40 and dh < 1e-12, (name, dh)
        t1, i1 = q.getGaugeFixTransform(ref, dirs, gstop=GSTOP, orf=1.8, maxits=5000)
        tl, il = q.getGaugeFixTransform(ctx, dirs, gstop=GSTOP, orf=1.8, maxits=5000)
        tg = R.cmat(gather(tl))
        met, gre, gro = R.metrics(glo, R.gradient(glo, R.links(g), tg, dirs), tg, len(dirs))
        mine = {"iters": il["iters"], "one_rank_iters": i1["iters"], "gdsq": il["gdsq"], "numpy_gdsq": float(gre + gro), "hist_dev_40": dh}
        allr = [None] * world
        dist.all_gather_object(allr, mine)
        print("rank %d %s: %s" % (rank, name, json.dumps(mine)), file=sys.stderr, flush=True)
        assert len({(a["iters"], a["gdsq"]) for a in allr}) == 1, (name, allr)
        assert gre + gro <= GSTOP and abs(met - il["met"]) < 1e-13, (name, mine, met, il["met"])
        assert np.abs(R.mul(tg, R.adj(tg)) - np.eye(3)).max() < 1e-12 and np.abs(np.linalg.det(tg) - 1).max() < 1e-12
        assert abs(il["iters"] - i1["iters"]) <= max(2, 0.02 * i1["iters"]), (name, mine)
        # the one-rank context applies the gathered t of the sharded fix: the same transformation on both
        tall = np.ascontiguousarray(gather(tl))
        q._lib.check(q.lib().qexhip_gfix_set_transform(ref._h, tall.ctypes.data))
        q.gaugeTransform(ref)
        q.gaugeTransform(ctx)
        p1, pl = q.plaq(ref), q.plaq(ctx)
        lt1, ltl = q.linkTrace(ref, dirs), q.linkTrace(ctx, dirs)
        assert np.abs(pl - p1).max() < 1e-13 and abs(ltl - lt1) < 1e-13 and abs(ltl - il["met"]) < 1e-13, (name, pl, p1, ltl, lt1)
        res[name] = mine

    ranks.finish(rk, "GAUGEFIX_RANKS_OK", res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
