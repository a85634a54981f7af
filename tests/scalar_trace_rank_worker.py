"""Worker of tests/test_gpu_scalar_trace_ranks.py: dilution, trace accumulation, slice sums and the scalarTrace driver on a
t-sharded lattice.

Started by torch.distributed.run, one process per rank, every rank on device 0 (the peer-memory transport between processes that
share one GPU).  Every rank builds the same GLOBAL random fields, uploads its t-slab to a sharded context and the whole fields to a
one-rank context of the whole lattice, and checks:
  * dev_dilute (both kinds, groups that mix time slices of both slabs): every destination's slab is np.array_equal to the slab of
    the one-rank destination;
  * dev_trace_accum (unimproved n = 4, then improved n = 3 on top) and cfield_scale: the slab of the cfield is np.array_equal;
  * dev_cfield_slices: the whole (nt, 2) table is np.array_equal on every rank;
  * with `e2e` as sixth argument: scalarTrace (Z4, EO, fp64, mass 0.1, r2req 1e-24) on the sharded context gives the one-rank
    est[t] and trace slab to 1e-9 of max|trace| (the bound of the oracle comparison in tests/test_gpu_scalar_trace.py).

usage: python -m torch.distributed.run --nproc-per-node N scalar_trace_rank_worker.py LX LY LZ LT [e2e]
Exit status 0 and one line `SCALAR_TRACE_RANKS_OK [json per rank]` from rank 0, non-zero on the first failed check.
"""
import json
import sys

import numpy as np

import ranks

SEED = 987654321


def main():
    glat = [int(v) for v in sys.argv[1:5]]
    e2e = len(sys.argv) > 5 and sys.argv[5] == "e2e"
    rank, world, dist, ctx, loc, idx, sl = rk = ranks.shard(glat)
    import qex_amd as q
    import scalar_trace_ref as R

    glo = q.Layout(glat)
    lt = loc.lat[3]
    ref = q.Context(glat, device=0)
    res = {"rank": rank}

    rng = np.random.default_rng(sum(glat))
    F = [rng.standard_normal((glo.vol, 3, 2)) for _ in range(8)]
    fl = [ctx.field_new(np.ascontiguousarray(f[idx])) for f in F]
    fg = [ref.field_new(f) for f in F]

    # dilution: destinations 4..7, source 0
    nt = glat[3]
    for kind in (R.EO, R.CORNER):
        hi = R.NPAT[kind] - 1
        for ids_, ts in (([0, hi, 1, hi], [0, lt - 1, lt, nt - 1]), ([hi, 0], [lt, lt - 1]), ([1], [nt - 1])):
            n = len(ts)
            ctx.dev_dilute(fl[4:4 + n], fl[0], kind, ids_, ts, 1.0 / np.sqrt(2.0))
            ref.dev_dilute(fg[4:4 + n], fg[0], kind, ids_, ts, 1.0 / np.sqrt(2.0))
            for k in range(n):
                got, want = ctx.field_download(fl[4 + k]), ref.field_download(fg[4 + k])
                if not np.array_equal(got, want[idx]):
                    raise AssertionError("rank %d: dilute kind %d idx %d t %d differs from the one-rank result" % (rank, kind, ids_[k], ts[k]))
                if not np.array_equal(want, R.dilute(F[0], glo.coords, kind, ids_[k], ts[k], 1.0 / np.sqrt(2.0))):
                    raise AssertionError("one-rank dilute differs from numpy")
                owned = rank * lt <= ts[k] < (rank + 1) * lt
                assert got.any() == owned, (rank, ts[k])              # a rank that does not own t[k] writes zeros
    res["dilute"] = "equal"

    # accumulation and slice sums on the uploaded fields 0..3
    for k in range(4, 8):
        ctx.field_upload(fl[k], np.ascontiguousarray(F[k][idx]))
        ref.field_upload(fg[k], F[k])
    tl, tg = ctx.cfield_new(), ref.cfield_new()
    for c, f, t in ((ctx, fl, tl), (ref, fg, tg)):
        c.dev_trace_accum(t, f[0:4], f[4:8], 1.0)
        c.dev_trace_accum(t, f[1:4], f[1:4], 0.1)
        c.cfield_scale(t, 1.0 / 3.0)
    got, want = ctx.cfield_download(tl), ref.cfield_download(tg)
    if not np.array_equal(got, want[idx]):
        raise AssertionError("rank %d: the slab of the cfield differs from the one-rank cfield" % rank)
    sl, sg = ctx.dev_cfield_slices(tl), ref.dev_cfield_slices(tg)
    if not (np.array_equal(sl, sg) and np.array_equal(ctx.dev_cfield_slices(tl), sl)):
        raise AssertionError("rank %d: slice table differs from the one-rank table (max %g)" % (rank, np.abs(sl - sg).max()))
    assert np.abs(sg - R.slice_sums(want, glo.coords, nt)).max() < 1e-12 * np.abs(want).sum()
    res["accum"], res["slices"] = "equal", "equal"

    if e2e:
        g = q.RngField(glat, q.RngMilc6, SEED).warm(0.5)
        q.rephase(glo, g)
        s1 = q.newStag(ref, g)
        sl_ = q.newStag(ctx, np.ascontiguousarray(g[idx]))
        t1, e1, st1 = q.scalarTrace(s1, glo, q.RngField(glat, q.RngMilc6, SEED), 0.1, 1e-24, out=None)
        tn, en, stn = q.scalarTrace(sl_, loc, q.RngField(loc.lat, q.RngMilc6, SEED, glat=glat, t_offset=rank * lt), 0.1, 1e-24,
                                    t_offset=rank * lt, out=None)
        scale = np.abs(t1[0]).max()
        de, dt = float(np.abs(en[0] - e1[0]).max() / scale), float(np.abs(tn[0] - t1[0][idx]).max() / scale)
        res["e2e"] = {"est_dev": de, "trace_dev": dt, "iterations": [min(stn["iterations"][0]), max(stn["iterations"][0])],
                      "one_rank_iterations": [min(st1["iterations"][0]), max(st1["iterations"][0])]}
        print("rank %d e2e: %s" % (rank, json.dumps(res["e2e"])), file=sys.stderr, flush=True)
        assert de < 1e-9 and dt < 1e-9, res["e2e"]

    ranks.finish(rk, "SCALAR_TRACE_RANKS_OK", res)
    ctx.close()
    ref.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
