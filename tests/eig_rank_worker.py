"""Worker of tests/test_gpu_eig_ranks.py: the low-mode eigensolver and the deflated solve on a t-sharded lattice.

Started by torch.distributed.run, one process per rank, every rank on device 0 (the peer-memory transport between processes that
share one GPU).  Every rank builds the same GLOBAL inputs and dense reference (tests/eig_ref.py), hands its t-slab to a sharded
context, and keeps a one-rank context of the whole lattice beside it.  nev = 8, nvecs = 24, abserr = 1e-9:
  * every rank returns the same evals / resid, bit for bit, and nconv = 8;
  * |lambda_i - lambda_i^dense| <= resid_i + 1e-12 lambda_max, index by index;
  * the vectors gathered from the slabs have the oracle residual |H v - lambda v| <= resid_i + 1e-12 and |V^+ V - 1| <= 1e-12;
  * the deflated solve (m = 0.01, r2req = 1e-20) takes the one-rank deflated solve's iterations to within 2 % (at least 2).

usage: python -m torch.distributed.run --nproc-per-node N eig_rank_worker.py LX LY LZ LT
Exit status 0 and one line `EIG_RANKS_OK [json per rank]` from rank 0, non-zero on the first failed check.
"""
import json
import sys

import numpy as np

import ranks

NEV, NVECS, MASS, R2REQ = 8, 24, 0.01, 1e-20
OPTS = dict(relerr=0.0, abserr=1e-9, cheb_degree=8, cheb_lo=0.3, cheb_hi=0.0, max_restarts=60)     # (a numpy model: 9 restarts)


def main():
    glat = tuple(int(v) for v in sys.argv[1:5])
    rank, world, dist, ctx, loc, idx, sl = rk = ranks.shard(glat)
    import qex_amd as q
    import eig_ref as R

    lo, g, _, b = R.inputs(glat)
    _, w, _ = R.dense(glat)
    vh = lo.vol // 2
    ctx.force_halo(True)                                              # (t is sharded: the halo is on already)
    assert ctx.sweep_info()["halo"]
    ref = q.Context(list(glat), device=0)
    s, s1 = q.newStag(ctx, sl(g)), q.newStag(ref, g)
    B = s.eigs(NEV, nvecs=NVECS, **OPTS)
    B1 = s1.eigs(NEV, nvecs=NVECS, **OPTS)

    def gather(xl):
        parts = [None] * world
        dist.all_gather_object(parts, (rank, xl))
        xg = np.zeros((lo.vol, 3, 2))
        for r, xr in parts:
            xg[q.Layout(list(glat)).shard_indices(world, r)[1]] = xr
        return xg

    mine = {"rank": rank, "nconv": B.nconv, "evals": [float(v) for v in B.evals], "resid": [float(v) for v in B.resid], "stats": B.stats}
    allr = [None] * world
    dist.all_gather_object(allr, mine)
    assert all(a["evals"] == mine["evals"] and a["resid"] == mine["resid"] for a in allr), allr
    assert B.nconv == NEV and B1.nconv == NEV, (B.nconv, B1.nconv)
    V = np.stack([R.cvec(gather(B.vector(i)), vh) for i in range(NEV)], axis=1)
    orth = float(np.abs(V.conj().T @ V - np.eye(NEV)).max())
    worst = 0.0
    for i in range(NEV):
        ro = float(np.linalg.norm(R.oracle_H(glat, False, V[:, i]) - B.evals[i] * V[:, i]))
        worst = max(worst, ro)
        assert B.resid[i] <= 1e-9 and ro <= B.resid[i] + 1e-12, (i, ro, B.resid[i])
        assert abs(B.evals[i] - w[i]) <= B.resid[i] + 1e-12 * w[-1], (i, B.evals[i], w[i])
    assert orth <= 1e-12, orth
    bid, xid = ctx.field_new(sl(b)), ctx.field_new()
    its, r2 = ctx.dev_solve_xx_deflated(B, NEV, xid, bid, MASS, R2REQ, 5000)
    its0, _, _ = ctx.dev_solve_xx(xid, bid, MASS, R2REQ, 5000)
    bid1, xid1 = ref.field_new(np.ascontiguousarray(b)), ref.field_new()
    its1, r21 = ref.dev_solve_xx_deflated(B1, NEV, xid1, bid1, MASS, R2REQ, 5000)
    mine.update({"deflated_its": its, "plain_its": its0, "one_rank_deflated_its": its1, "r2": r2, "one_rank_r2": r21,
                 "oracle_resid_max": worst, "orth": orth, "max_eval_dev": float(np.abs(B.evals - w[:NEV]).max())})
    print("rank %d: %s" % (rank, json.dumps(mine)), file=sys.stderr, flush=True)
    allr = ranks.gather(rk, mine)
    assert len({(a["deflated_its"], a["r2"]) for a in allr}) == 1, allr
    assert abs(its - its1) <= max(2, 0.02 * its1), (its, its1)
    assert r2 <= R2REQ * (1 + 1e-3), r2
    ranks.finish(rk, "EIG_RANKS_OK", mine)
    B.free()
    B1.free()
    return 0


if __name__ == "__main__":
    sys.exit(main())
