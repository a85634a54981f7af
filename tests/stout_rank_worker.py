"""Worker of tests/test_gpu_stout_ranks.py: stout smearing on a t-sharded lattice.

Started by torch.distributed.run, one process per rank, every rank on device 0 (the peer-memory transport between processes that
share one GPU).  Every rank builds the same GLOBAL configuration (stout_ref.reference_config), hands its t-slab to a sharded
context, and keeps a one-rank context of the whole lattice beside it as the reference:
  * the rank's slab of the smeared links (one step, and the three-level chain) and of the three-level force is np.array_equal to
    the slab of the one-rank result -- the arithmetic per link is local once the ghost slices are right;
  * the inverse (alpha = 0.02) stops after the same iterations on every rank, within +-1 of the one-rank count (the rank sums are
    grouped differently), and the gathered result has del2 <= 1e-24 against the configuration that was smeared.

usage: python -m torch.distributed.run --nproc-per-node N stout_rank_worker.py LX LY LZ LT
Exit status 0 and one line `STOUT_RANKS_OK [json per rank]` from rank 0, non-zero on the first failed check.
"""
import json
import sys

import numpy as np

import ranks

ALPHAS = (0.1, 0.09, 0.12)


def main():
    glat = [int(v) for v in sys.argv[1:5]]
    rank, world, dist, ctx, loc, idx, sl = rk = ranks.shard(glat)
    import qex_amd as q
    from oracle import oracle as o
    import stout_ref as R

    o.build()
    olo = o.Layout(glat)
    glo = q.Layout(glat)
    g = R.reference_config(olo, 0.1)
    rf = o.RngField(olo, o.RNG_MILC6, 21)
    chain = o.gauge_random_tah(olo, rf) + 0.3 * o.gauge_random(olo, rf)
    ref = q.Context(glat, device=0)
    res = {"rank": rank}

    def same(what, mine, whole):
        if not np.array_equal(mine, whole[idx]):
            raise AssertionError("rank %d: the slab of %s differs from the one-rank result (max %g)" % (rank, what, np.abs(mine - whole[idx]).max()))

    # one step, host-pointer and resident form
    f1, fl = np.zeros_like(g), np.zeros_like(sl(g))
    q.stoutSmear(ref, g, 0.1, f1)
    q.stoutSmear(ctx, sl(g), 0.1, fl)
    same("one stout step", fl, f1)
    q.gaugeSet(ctx, sl(g))
    q.stoutSmear(ctx, None, 0.1, None)
    q._lib.check(q.lib().qexhip_gauge_get(ctx._h, fl.ctypes.data))
    same("one resident stout step", fl, f1)
    # three levels and their force
    s1, sl3 = np.zeros_like(g), np.zeros_like(fl)
    sf1 = q.stoutSmearGetForce(ref, g, s1, ALPHAS)
    sfl = q.stoutSmearGetForce(ctx, sl(g), sl3, ALPHAS)
    same("the three-level links", sl3, s1)
    d1, dl = np.zeros_like(g), np.zeros_like(fl)
    sf1(d1, chain)
    sfl(dl, sl(chain))
    same("the three-level force", dl, d1)
    sf1.gaugeForce(d1, 6.0)
    sfl.gaugeForce(dl, 6.0)
    same("the three-level gauge force", dl, d1)
    sf1.release()
    sfl.release()
    # the inverse
    gi = R.reference_config(olo, 0.02)
    fi = np.zeros_like(g)
    q.stoutSmear(ref, gi, 0.02, fi)
    u1, ul = np.zeros_like(g), np.zeros_like(fl)
    it1, r21 = q.newStoutSmear(ref, 0.02).inverse(u1, fi)
    itl, r2l = q.newStoutSmear(ctx, 0.02).inverse(ul, sl(fi))
    parts = [None] * world
    dist.all_gather_object(parts, (rank, ul))
    ug = np.zeros_like(g)
    for r, ur in parts:
        ug[glo.shard_indices(world, r)[1]] = ur
    d2 = R.del2(olo, ug, gi)
    mine = {"iters": itl, "one_rank_iters": it1, "rdf2": r2l, "one_rank_rdf2": r21, "del2": d2}
    allr = [None] * world
    dist.all_gather_object(allr, mine)
    print("rank %d inverse: %s" % (rank, json.dumps(mine)), file=sys.stderr, flush=True)
    assert len({(a["iters"], a["rdf2"]) for a in allr}) == 1, allr
    assert abs(itl - it1) <= 1 and d2 <= 1e-24, mine
    res["inverse"] = mine

    ranks.finish(rk, "STOUT_RANKS_OK", res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
