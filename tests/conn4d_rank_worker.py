"""Worker of tests/test_gpu_conn4d_ranks.py: point sources, the translated accumulation, the staggered sign, the slice table and the
connMeson driver on a t-sharded lattice.

Started by torch.distributed.run, one process per rank, every rank on device 0 (the peer-memory transport between processes that
share one GPU).  Every rank builds the same GLOBAL random fields, uploads its t-slab to a sharded context and the whole fields to a
one-rank context of the whole lattice, and checks:
  * dev_point_source (points on both slabs): every destination's slab is np.array_equal to the slab of the one-rank destination,
    and only the owner of pt_t holds the one;
  * dev_conn_accum with pt_t = 0, 2, 4, 6 and an odd-sum point (2 crosses the rank boundary inside a slab; 4 is the local extent
    of two ranks on nt = 8, so the whole slab comes from the other rank), in groups of 4 + 1, then once more one at a time into a
    second cfield; cfield_stag_sign: the slab of the cfield is np.array_equal to the one-rank cfield's, which equals numpy's;
  * dev_cfield_slices: the whole (nt, 2) table is np.array_equal on every rank;
  * with `e2e` as fifth argument: connMeson (fp64, mass 0.1, r2req 1e-20, three points) on the sharded context gives the one-rank
    locmes slab and est within the solver bound of tests/test_gpu_conn4d.py, and sloppy = 1 is refused with dev_solve_batch's
    message.

usage: python -m torch.distributed.run --nproc-per-node N conn4d_rank_worker.py LX LY LZ LT [e2e]
Exit status 0 and one line `CONN4D_RANKS_OK [json per rank]` from rank 0, non-zero on the first failed check.
"""
import json
import sys

import numpy as np

import ranks

SEED = 987654321
MASS, R2REQ = 0.1, 1e-20


def main():
    glat = [int(v) for v in sys.argv[1:5]]
    e2e = len(sys.argv) > 5 and sys.argv[5] == "e2e"
    rank, world, dist, ctx, loc, idx, sl = rk = ranks.shard(glat)
    import conn4d_ref as R
    import qex_amd as q

    glo = q.Layout(glat)
    lt, nt = loc.lat[3], glat[3]
    ref = q.Context(glat, device=0)
    res = {"rank": rank}
    far = [v - 1 for v in glat]

    rng = np.random.default_rng(sum(glat))
    pts = [[2, 0, 4, 0], [0, 2, 2, 2], [4, 4, 0, 4], [far[0] - 1, far[1] - 1, far[2] - 1, 6], [1, 2, 3, 3]]
    assert [p[3] for p in pts[:4]] == [0, 2, 4, 6] and sum(pts[4]) % 2 == 1
    F = [rng.standard_normal((glo.vol, 3, 2)) for _ in pts]
    fl = [ctx.field_new(np.ascontiguousarray(f[idx])) for f in F]
    fg = [ref.field_new(f) for f in F]

    # point sources into scratch fields pre-filled with noise
    sl_, sg_ = [ctx.field_new(np.ascontiguousarray(F[0][idx])) for _ in range(4)], [ref.field_new(F[0]) for _ in range(4)]
    for grp, ic in (([pts[0], pts[3], pts[4], pts[4]], [0, 2, 1, 2]), ([pts[2]], [1]), ([far, pts[1], [0, 0, 0, lt]], [2, 0, 1])):
        n = len(grp)
        ctx.dev_point_source(sl_[:n], grp, ic)
        ref.dev_point_source(sg_[:n], grp, ic)
        for k in range(n):
            got, want = ctx.field_download(sl_[k]), ref.field_download(sg_[k])
            if not np.array_equal(want, R.point_source(glo.coords, grp[k], ic[k])):
                raise AssertionError("one-rank point source differs from numpy")
            if not np.array_equal(got, want[idx]):
                raise AssertionError("rank %d: point source %s colour %d differs from the one-rank result" % (rank, grp[k], ic[k]))
            owned = rank * lt <= grp[k][3] < (rank + 1) * lt
            assert got.any() == owned and (got.sum() == 1.0) == owned, (rank, grp[k])
    res["point"] = "equal"

    # accumulation (4 + 1, on a pre-filled cfield), the sign and the slice table
    tl, tg, tl1, tg1 = ctx.cfield_new(), ref.cfield_new(), ctx.cfield_new(), ref.cfield_new()
    for c, f, t, t1 in ((ctx, fl, tl, tl1), (ref, fg, tg, tg1)):
        c.dev_trace_accum(t, f[0:1], f[1:2], 1.0)
        c.dev_trace_accum(t1, f[0:1], f[1:2], 1.0)
        c.dev_conn_accum(t, f[0:4], pts[0:4], 0.2)
        c.dev_conn_accum(t, f[4:5], pts[4:5], 0.2)
        for k in range(5):
            c.dev_conn_accum(t1, [f[k]], [pts[k]], 0.2)
    got, want = ctx.cfield_download(tl), ref.cfield_download(tg)
    if not np.array_equal(got, want[idx]):
        raise AssertionError("rank %d: the slab of the accumulated cfield differs from the one-rank cfield (max %g)" %
                             (rank, np.abs(got - want[idx]).max()))
    if not (np.array_equal(ctx.cfield_download(tl1), got) and np.array_equal(ref.cfield_download(tg1), want)):
        raise AssertionError("rank %d: one system a call differs from the grouped calls" % rank)
    # the one-rank result against numpy: 8 eps sum_k scal |phi_k|^2 per site (tests/test_gpu_conn4d.py)
    tp = ref.cfield_new()
    ref.dev_trace_accum(tp, fg[0:1], fg[1:2], 1.0)
    pre = ref.cfield_download(tp)
    npref, bound = pre[:, 0].copy(), np.zeros(glo.vol)
    for k in range(5):
        R.conn_accum(npref, F[k], glo.coords, glat, pts[k], 0.2)
        bound += R.translate(0.2 * R.site_norm2(F[k]), glo.coords, glat, pts[k])
    eps = np.finfo(np.float64).eps
    assert (np.abs(want[:, 0] - npref) <= 8 * eps * (bound + np.abs(pre[:, 0]))).all() and np.array_equal(want[:, 1], pre[:, 1])
    for c, t in ((ctx, tl), (ref, tg)):
        c.cfield_stag_sign(t)
    got, want = ctx.cfield_download(tl), ref.cfield_download(tg)
    if not np.array_equal(got, want[idx]):
        raise AssertionError("rank %d: the slab of the signed cfield differs from the one-rank cfield" % rank)
    sl1, sg1 = ctx.dev_cfield_slices(tl), ref.dev_cfield_slices(tg)
    if not np.array_equal(sl1, sg1):
        raise AssertionError("rank %d: slice table differs from the one-rank table (max %g)" % (rank, np.abs(sl1 - sg1).max()))
    res["accum"], res["sign"], res["slices"] = "equal", "equal", "equal"

    if e2e:
        g = q.RngField(glat, q.RngMilc6, SEED).warm(0.5)
        q.rephase(glo, g)
        s1 = q.newStag(ref, g)
        sn = q.newStag(ctx, np.ascontiguousarray(g[idx]))
        mpts = [[0, 0, 0, 0], [2, 4, 2, nt - 2], [1, 2, 0, lt]]
        l1, e1, st1 = q.connMeson(s1, glo, mpts, MASS, R2REQ, out=None)
        ln, en, stn = q.connMeson(sn, loc, mpts, MASS, R2REQ, t_offset=rank * lt, out=None)
        # two solutions with |b - (D+m)x|^2 <= r2req |b|^2, |b| = 1, differ by at most eps = 2 sqrt(r2req) / m in norm, so per site
        # |d locmes| <= sum_systems scal (2 max|phi| eps + eps^2).  max|phi| from the one-rank run: every term scal |phi_k|^2 is
        # non-negative, so scal |phi_k(y)|^2 <= |locmes| at the site y lands on, and max|phi| <= sqrt(max|locmes| / scal)
        eps_s = 2.0 * np.sqrt(R2REQ) / MASS
        maxphi = float(np.sqrt(len(mpts) * np.abs(l1).max()))
        bound_s = 3 * len(mpts) * (1.0 / len(mpts)) * (2.0 * maxphi * eps_s + eps_s * eps_s)
        dl, de = float(np.abs(ln - l1[idx]).max()), float(np.abs(en - e1).max())
        res["e2e"] = {"locmes_dev": dl, "est_dev": de, "bound": bound_s, "slice_sites": glo.vol // nt,
                      "iterations": [min(stn["iterations"]), max(stn["iterations"])],
                      "one_rank_iterations": [min(st1["iterations"]), max(st1["iterations"])]}
        print("rank %d e2e: %s" % (rank, json.dumps(res["e2e"])), file=sys.stderr, flush=True)
        assert dl <= bound_s and de <= (glo.vol // nt) * bound_s, res["e2e"]
        try:
            q.connMeson(sn, loc, mpts, MASS, 1e-12, t_offset=rank * lt, sloppy=1, out=None)
            raise AssertionError("sloppy = 1 on a sharded context was not refused")
        except q.QexHipError as e:
            assert "batched sloppy solve: t-sharded contexts" in str(e), str(e)
            res["e2e"]["sloppy_refused"] = True

    ranks.finish(rk, "CONN4D_RANKS_OK", res)
    ctx.close()
    ref.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
