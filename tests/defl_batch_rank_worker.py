"""Worker of tests/test_gpu_defl_batch_ranks.py: the deflated lock-step batch on a t-sharded lattice.

Started by torch.distributed.run, one process per rank, every rank on device 0 (the peer-memory transport between processes that
share one GPU).  Every rank builds the same GLOBAL inputs (tests/eig_ref.py), hands its t-slab to a sharded context, and keeps a
one-rank context of the whole lattice beside it.  nev = 8, nvecs = 24, abserr = 1e-9; four Gaussian sources, masses (0.01, 0.01,
0.02, 0.05), r2req = 1e-20, fp64, on both parities:
  * every rank returns the same iterations and true residuals, bit for bit, and every residual is <= r2req (1 + 1e-3);
  * the iterations are within 2 % (at least 2) of the one-rank context's;
  * the solutions gathered from the slabs are within 1e-9 (relative) of the one-rank ones;
  * sloppy = 1 returns QEXHIP_ERR_ARG on the sharded context.

usage: python -m torch.distributed.run --nproc-per-node N defl_batch_rank_worker.py LX LY LZ LT
Exit status 0 and one line `DEFL_BATCH_RANKS_OK [json per rank]` from rank 0, non-zero on the first failed check.
"""
import ctypes as C
import json
import sys

import numpy as np

import ranks

NEV, NVECS, R2REQ = 8, 24, 1e-20
MS = [0.01, 0.01, 0.02, 0.05]
OPTS = dict(relerr=0.0, abserr=1e-9, cheb_degree=8, cheb_lo=0.3, cheb_hi=0.0, max_restarts=60)     # those of eig_rank_worker.py


def main():
    glat = tuple(int(v) for v in sys.argv[1:5])
    rank, world, dist, ctx, loc, idx, sl = rk = ranks.shard(glat)
    import qex_amd as q
    import eig_ref as R
    from oracle import oracle as o

    lo, g, _, b = R.inputs(glat)
    rf = o.RngField(lo, o.RNG_MILC6, 4242)
    bs = [np.ascontiguousarray(b)] + [o.vector_gaussian(lo, rf) for _ in range(3)]
    glo = q.Layout(list(glat))
    ctx.force_halo(True)                                              # (t is sharded: the halo is on already)
    assert ctx.sweep_info()["halo"]
    ref = q.Context(list(glat), device=0)
    s, s1 = q.newStag(ctx, sl(g)), q.newStag(ref, g)
    B = s.eigs(NEV, nvecs=NVECS, **OPTS)
    B1 = s1.eigs(NEV, nvecs=NVECS, **OPTS)
    assert B.nconv == NEV and B1.nconv == NEV, (B.nconv, B1.nconv)

    def gather(xl):
        parts = [None] * world
        dist.all_gather_object(parts, (rank, xl))
        xg = np.zeros((lo.vol, 3, 2))
        for r, xr in parts:
            xg[glo.shard_indices(world, r)[1]] = xr
        return xg

    bid, xid = [ctx.field_new(sl(v)) for v in bs], [ctx.field_new() for _ in bs]
    bid1, xid1 = [ref.field_new(v) for v in bs], [ref.field_new() for _ in bs]
    mine = {"rank": rank}
    for name, par_even in (("even", True), ("odd", False)):
        its, r2, _ = ctx.dev_solve_xx_batch_deflated(B, NEV, xid, bid, MS, R2REQ, 5000, par_even=par_even)
        its1, r21, _ = ref.dev_solve_xx_batch_deflated(B1, NEV, xid1, bid1, MS, R2REQ, 5000, par_even=par_even)
        xerr = 0.0
        for k in range(4):
            xg, x1 = gather(ctx.field_download(xid[k])), ref.field_download(xid1[k])
            xerr = max(xerr, float(np.linalg.norm(xg - x1) / np.linalg.norm(x1)))
        mine[name] = {"its": its, "r2": r2, "one_rank_its": its1, "one_rank_r2": r21, "xerr": xerr}
        assert all(v <= R2REQ * (1 + 1e-3) for v in r2), r2
        assert all(abs(a - c) <= max(2, 0.02 * c) for a, c in zip(its, its1)), (its, its1)
        assert xerr <= 1e-9, xerr
    n = 4
    it4, f4, u4 = (C.c_int * n)(), (C.c_double * n)(), (C.c_int * n)()
    before = ctx.field_download(xid[0])
    mine["sloppy_rc"] = q.lib().qexhip_dev_solve_xx_batch_deflated(ctx._h, B.id, NEV, n, (C.c_int * n)(*xid), (C.c_int * n)(*bid),
                                                                   (C.c_double * n)(*MS), (C.c_double * n)(*([R2REQ] * n)), 5000, 1, 1, it4, f4, u4)
    assert mine["sloppy_rc"] == -1, mine["sloppy_rc"]
    assert np.array_equal(ctx.field_download(xid[0]), before)         # nothing was launched
    print("rank %d: %s" % (rank, json.dumps(mine)), file=sys.stderr, flush=True)
    allr = ranks.gather(rk, mine)
    for name in ("even", "odd"):
        assert len({(tuple(a[name]["its"]), tuple(a[name]["r2"])) for a in allr}) == 1, allr
    ranks.finish(rk, "DEFL_BATCH_RANKS_OK", mine)
    B.free()
    B1.free()
    return 0


if __name__ == "__main__":
    sys.exit(main())
