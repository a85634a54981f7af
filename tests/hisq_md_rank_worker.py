"""Worker of tests/test_gpu_hisq_md_ranks.py: the resident HISQ molecular dynamics on a t-sharded lattice.

Started by torch.distributed.run, one process per rank, every rank on device 0 (the peer-memory transport between processes that
share one GPU).  Every rank draws the same GLOBAL links, momenta and vectors (qex_amd.RngField of the whole lattice), hands its
t-slab to a sharded context, and keeps a one-rank context of the whole lattice beside it as the reference.  Two MD steps
(update_links, hisq_prepare, hisq_fforce with three vectors) on both; then
  * the rank's slab of the force, of the momenta and of the links is np.array_equal to the slab of the one-rank result: the
    closure, the outer products (hop 1 and hop 3 across the slab boundary), the chain and the kick are local arithmetic once the
    ghost slices are right;
  * hisq_fforce_solve stops after the same iterations on every rank (the ranks agree on the loop control); its force differs
    from the one-rank force only through the solutions, whose rank sums are grouped differently -- the deviation is reported.

usage: python -m torch.distributed.run --nproc-per-node N hisq_md_rank_worker.py LX LY LZ LT
Exit status 0 and one line `HISQ_MD_RANKS_OK [json per rank]` from rank 0, non-zero on the first failed check.
"""
import json
import sys

import numpy as np

import ranks

SCALES = [0.7, -1.3, 0.45]
DT, T = 0.05, -0.37


def main():
    glat = [int(v) for v in sys.argv[1:5]]
    rank, world, dist, ctx, loc, idx, sl = rk = ranks.shard(glat)
    import qex_amd as q

    rng = q.RngField(glat, q.RngMilc6, 4711)
    g, p = rng.warm(0.3), rng.randomTAH()
    v = [rng.gaussian_vector() for _ in range(3)]
    ref = q.Context(glat, device=0)

    def same(what, mine, whole):
        if not np.array_equal(mine, whole[idx]):
            raise AssertionError("rank %d: the slab of %s differs from the one-rank result (max %g)" % (rank, what, np.abs(mine - whole[idx]).max()))

    out = []
    for c, cut in ((ref, lambda a: a), (ctx, sl)):
        md = q.ResidentMD(c)
        md.begin(cut(g), cut(p))
        ids = [c.field_new(cut(x)) for x in v]
        for _ in range(2):
            md.update_links(DT)
            md.hisq_prepare(set_links=True)
            md.hisq_fforce(ids, SCALES, T)
        f = md.hisq_force()
        gg, pp = np.zeros_like(f), np.zeros_like(f)
        md.end(gg, pp)
        its = md.hisq_fforce_solve(ids, [0.5, 0.3, 0.8], SCALES, 1e-20, 2000, T)
        out.append((f, gg, pp, its, md.hisq_force()))
    (f1, g1, p1, its1, fs1), (fl, gl, pl, itsl, fsl) = out
    same("the force after two MD steps", fl, f1)
    same("the momenta after two MD steps", pl, p1)
    same("the links after two MD steps", gl, g1)
    assert np.abs(f1).max() > 0 and not np.array_equal(g1, g)
    dev = float(np.abs(fsl - fs1[idx]).max() / np.abs(fs1).max())
    mine = {"rank": rank, "iters": itsl, "one_rank_iters": its1, "solve_force_dev": dev}
    print("rank %d solve + force: %s" % (rank, json.dumps(mine)), file=sys.stderr, flush=True)
    allres = ranks.gather(rk, mine)
    assert len({tuple(a["iters"]) for a in allres}) == 1, allres
    ranks.finish(rk, "HISQ_MD_RANKS_OK", mine)
    return 0


if __name__ == "__main__":
    sys.exit(main())
