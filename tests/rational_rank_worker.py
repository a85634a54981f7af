"""Worker of tests/test_gpu_rational_ranks.py: the accumulating multi-shift solve and the rational HISQ force on a t-sharded lattice.

Started by torch.distributed.run, one process per rank, every rank on device 0 (the peer-memory transport between processes that
share one GPU).  Every rank draws the same GLOBAL links, momenta and source, hands its t-slab to a sharded context, and keeps a
one-rank context of the whole lattice beside it.  On both, with the HISQ links of md.hisq_prepare:
  * S = r(M^+M) b by dev_rational_xx with five poles at r2req 1e-24.  The rank's slab of the sharded S must not be further from the
    binary128 reference (tests/rational_ref.py on the oracle's HISQ links of the same field) than 4 x the one-rank EXISTING path
    (dev_solve_xx_multi, summed in numpy) is on that slab, plus 1e-15 relative: the relation of tests/test_gpu_rational.py;
  * the slab of the hisq_fforce_rational force against the one-rank force at 2e-11 in relative norm (two paths of one trajectory,
    tests/test_gpu_hisq_md.py): the rank sums of the solve are grouped differently, the rest is local arithmetic;
  * every rank stops after the same iterations in both calls.

usage: python -m torch.distributed.run --nproc-per-node N rational_rank_worker.py LX LY LZ LT
Exit status 0 and one line `RATIONAL_RANKS_OK [json per rank]` from rank 0, non-zero on the first failed check.
"""
import json
import sys

import numpy as np

import ranks

MASS, F0 = 0.3, 0.37
ALPHA, BETA = [0.3, -0.5, 0.9, 1.7, 0.6], [0.4, 0.05, 6.0, 1.5, 0.0]
T, MAXITS = -0.37, 5000


def main():
    glat = [int(v) for v in sys.argv[1:5]]
    rank, world, dist, ctx, loc, idx, sl = rk = ranks.shard(glat)
    import qex_amd as q
    import rational_ref as RR
    from oracle import oracle as o

    rng = q.RngField(glat, q.RngMilc6, 4711)
    g, p = rng.warm(0.3), rng.randomTAH()
    b = rng.gaussian_vector()
    phi = b.copy()
    phi[phi.shape[0] // 2:] = 0
    ref = q.Context(glat, device=0)

    out = []
    for c, cut in ((ref, lambda a: a), (ctx, sl)):
        md = q.ResidentMD(c)
        md.begin(cut(g), cut(p))
        md.hisq_prepare(set_links=True)
        bid, sid, pid = c.field_new(cut(b)), c.field_new(), c.field_new(cut(phi))
        its, hist = c.dev_rational_xx(sid, bid, MASS, F0, ALPHA, BETA, 1e-24, MAXITS, True, histcap=MAXITS)
        S = c.field_download(sid)
        fits = md.hisq_fforce_rational(pid, MASS, ALPHA, BETA, 1e-28, MAXITS, T)
        out.append((S, its, md.hisq_force(), fits, c, bid))
    (S1, its1, f1, fits1, _, bid1), (Sl, itsl, fl, fitsl, _, _) = out

    # the one-rank existing path on the same links
    order, sh = RR.mapped_shifts(MASS, ALPHA, BETA)
    xs = [ref.field_new() for _ in ALPHA]
    its0, _ = ref.dev_solve_xx_multi(xs, bid1, sh, 1e-24, MAXITS, True)
    old = F0 * b
    old[b.shape[0] // 2:] = 0
    h = b.shape[0] // 2
    for j, k in enumerate(order):
        old[:h] += 4.0 * ALPHA[k] * ref.field_download(xs[j])[:h]

    # binary128 reference on the oracle's HISQ links of the phased field
    o.build()
    olo = o.Layout(glat)
    gp = g.copy()
    o.rephase(olo, gp)
    fat, lng = o.hisq_smear(olo, gp)
    want = RR.rational_ref(o, olo, fat, lng, b, MASS, F0, ALPHA, BETA, True)

    nr = float(np.linalg.norm(want[idx]))
    dn = float(np.linalg.norm(Sl - want[idx]))
    do = float(np.linalg.norm(old[idx] - want[idx]))
    d1 = float(np.linalg.norm(S1[idx] - want[idx]))
    fdev = float(np.linalg.norm(fl - f1[idx]) / np.linalg.norm(f1[idx]))
    mine = {"rank": rank, "iters": itsl, "one_rank_iters": its1, "existing_iters": its0, "force_iters": fitsl, "one_rank_force_iters": fits1,
            "sum_dev": dn / nr, "existing_dev": do / nr, "one_rank_sum_dev": d1 / nr, "force_dev": fdev}
    print("rank %d rational: %s" % (rank, json.dumps(mine)), file=sys.stderr, flush=True)
    assert nr > 0 and np.abs(f1).max() > 1e-3
    assert dn <= 4.0 * do + 1e-15 * nr, (rank, dn / nr, do / nr)
    assert fdev <= 2e-11, (rank, fdev)
    allres = ranks.gather(rk, mine)
    assert len({(a["iters"], a["force_iters"]) for a in allres}) == 1, allres
    ranks.finish(rk, "RATIONAL_RANKS_OK", mine)
    return 0


if __name__ == "__main__":
    sys.exit(main())
