"""Worker of tests/test_gpu_lma_ranks.py: low-mode averaging of the scalar trace on a t-sharded lattice.

Started by torch.distributed.run, one process per rank, every rank on device 0 (the peer-memory transport between processes that
share one GPU).  Every rank builds the same GLOBAL inputs (tests/eig_ref.py), keeps a one-rank context of the whole lattice beside its
sharded one, computes nev = 8 pairs on the one-rank context and loads the slabs of those very vectors into the sharded basis.  Then
  * lowmode_diag: the slab of L is within 1e-12 of max L of the one-rank L;
  * project_out of four Gaussian fields: every slab within 1e-12 of max|phi| of the one-rank result;
  * scalarTrace(lma=True) (Z4, EO, fp64, mass 0.1, r2req 1e-24): trace slab and est[t] within 1e-9 of max|trace| of the one-rank
    run, low_trace within 1e-12, and est identical on every rank.
The rank sums reorder additions, so no bit equality with the one-rank context is claimed.

usage: python -m torch.distributed.run --nproc-per-node N lma_rank_worker.py LX LY LZ LT
Exit status 0 and one line `LMA_RANKS_OK [json per rank]` from rank 0, non-zero on the first failed check.
"""
import json
import sys

import numpy as np

import ranks

NEV, NVECS, MASS, R2REQ = 8, 24, 0.1, 1e-24
OPTS = dict(relerr=0.0, abserr=1e-9, cheb_degree=8, cheb_lo=0.3, cheb_hi=0.0, max_restarts=60)     # those of eig_rank_worker.py


def main():
    glat = tuple(int(v) for v in sys.argv[1:5])
    rank, world, dist, ctx, loc, idx, sl = rk = ranks.shard(glat)
    import qex_amd as q
    import eig_ref as R

    lo, g, _, _ = R.inputs(glat)
    glo = q.Layout(list(glat))
    lt = loc.lat[3]
    ref = q.Context(list(glat), device=0)
    s, s1 = q.newStag(ctx, sl(g)), q.newStag(ref, g)
    B1 = s1.eigs(NEV, nvecs=NVECS, **OPTS)
    assert B1.nconv == NEV, B1.nconv
    B = q.EigBasis(ctx, NEV)
    for i in range(NEV):
        B.set_vector(i, sl(B1.vector(i)))
    lam, lam1 = B.rayleigh(NEV), B1.rayleigh(NEV)
    assert np.abs(lam - lam1).max() < 1e-13, (lam, lam1)
    mine = {"rank": rank}

    c, c1 = ctx.cfield_new(), ref.cfield_new()
    B.lowmode_diag(NEV, MASS, c)
    B1.lowmode_diag(NEV, MASS, c1)
    got, want = ctx.cfield_download(c), ref.cfield_download(c1)
    mine["low_dev"] = float(np.abs(got - want[idx]).max() / want.max())
    assert mine["low_dev"] < 1e-12, mine

    rng = np.random.default_rng(sum(glat))
    phis = [rng.standard_normal((glo.vol, 3, 2)) for _ in range(4)]
    ids, ids1 = [ctx.field_new(sl(p)) for p in phis], [ref.field_new(p) for p in phis]
    B.project_out(NEV, ids)
    B1.project_out(NEV, ids1)
    mine["project_dev"] = max(float(np.abs(ctx.field_download(a) - ref.field_download(b)[idx]).max() / np.abs(p).max())
                              for a, b, p in zip(ids, ids1, phis))
    assert mine["project_dev"] < 1e-12, mine
    mine["project_changed"] = float(np.abs(ctx.field_download(ids[0]) - sl(phis[0])).max())
    assert mine["project_changed"] > 1e-3

    t1, e1, st1 = q.scalarTrace(s1, glo, q.RngField(list(glat), q.RngMilc6, R.SEED), MASS, R2REQ, out=None, deflate=B1, nev=NEV, lma=True)
    tn, en, stn = q.scalarTrace(s, loc, q.RngField(loc.lat, q.RngMilc6, R.SEED, glat=list(glat), t_offset=rank * lt), MASS, R2REQ,
                                t_offset=rank * lt, out=None, deflate=B, nev=NEV, lma=True)
    scale = np.abs(t1[0]).max()
    mine["trace_dev"] = float(np.abs(tn[0] - t1[0][idx]).max() / scale)
    mine["est_dev"] = float(np.abs(en[0] - e1[0]).max() / scale)
    mine["low_trace_dev"] = float(np.abs(stn["low_trace"] - st1["low_trace"][idx]).max() / scale)
    mine["low_est_dev"] = float(np.abs(stn["low_est"] - st1["low_est"]).max() / scale)
    mine["est"] = [float(v) for v in en[0]]
    print("rank %d: %s" % (rank, json.dumps({k: v for k, v in mine.items() if k != "est"})), file=sys.stderr, flush=True)
    assert mine["trace_dev"] < 1e-9 and mine["est_dev"] < 1e-9 and mine["low_trace_dev"] < 1e-12 and mine["low_est_dev"] < 1e-12, mine
    allr = ranks.gather(rk, mine)
    assert len({tuple(a["est"]) for a in allr}) == 1, allr
    ranks.finish(rk, "LMA_RANKS_OK", mine)
    B.free()
    B1.free()
    ctx.close()
    ref.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
