"""Worker of tests/test_gpu_sloppy_batch_ranks.py: the mixed-precision lock-step batches (fp32, and 16-bit under "half_batch" = 1) on a
t-sharded lattice under option "batch_ranks" = 1.

Started by torch.distributed.run, one process per rank, every rank on device 0 (the peer-memory transport between processes that
share one GPU).  Every rank builds the same GLOBAL problem with the oracle, hands its t-slab to a sharded context, and keeps a
one-rank context of the whole lattice beside it as the reference.

  --op      n = 3 systems with distinct m^2: every system's slab from dev_op_xx_sloppy_batch / dev_op_xx_half_batch equals
            (np.array_equal) the slab of the one-rank SINGLE-system dev_op_xx_sloppy / dev_op_xx_half, for g.random links, g.random
            fat + Naik links and HISQ links, both parities, in the sweep forms exchange-first (overlap 0), split by sites (overlap 1,
            hop_split 0) and overlap 1 with hop_split 2 (no fused form: split by sites).  From the timers: ONE exchange per sweep (two
            per operator application, not 2 n), boundary launches only where sweep_info()["overlap"] says the sweep was split
  --solve   three systems, masses 0.1 / 0.2 / 0.05 to r2req 1e-8 / 1e-14 / 1e-10 (they finish in different chunks: a message count
            that depended on `done` would hang here, and the launcher's limit would end the test), g.random links, sloppy = 1 and
            sloppy = 2: every system's x, iterations, true r2 and updates are bit for bit the single-system dev_solve_xx_sloppy's on
            the SAME sharded context; every rank reports the same numbers and the same sloppy_last_batch; the oracle's fp64 residual
            of the gathered solution is <= r2req * 1.001; maxits = 10 stops every system at 10; half_stall = 0 sends every 16-bit
            system to fp32 on every rank alike and still reaches r2req; the full solve (solve_batch, dev_solve_batch) on a ReconL
            source and on a source without an odd part stays within r2req by the oracle
  --top     connMeson with sloppy = 1 on the sharded context against the one-rank fp64 connMeson, within the solver bound that
            tests/conn4d_rank_worker.py derives (the same r2req, mass and formula)

usage: python -m torch.distributed.run --nproc-per-node N sloppy_batch_rank_worker.py LX LY LZ LT [--op] [--solve] [--top]
Exit status 0 and one line `SLOPPY_BATCH_RANKS_OK [json per rank]` from rank 0, non-zero on the first failed check.
"""
import argparse
import json
import sys

import numpy as np

import ranks

SEED = 987654321
FORMS = (("exchange_first", 0, 0), ("by_sites", 1, 0), ("fused_requested", 1, 2))     # (name, overlap, hop_split)
MS = [0.1, 0.2, 0.05]
R2 = [1e-8, 1e-14, 1e-10]
M2 = [0.01, 0.04, 0.0025]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lat", type=int, nargs=4)
    ap.add_argument("--op", action="store_true")
    ap.add_argument("--solve", action="store_true")
    ap.add_argument("--top", action="store_true")
    args = ap.parse_args()
    w = ranks.shard(args.lat)
    rank, world, dist, ctx, loc, idx, sl = w
    import qex_amd as q
    from oracle import oracle as o

    glat = list(args.lat)
    olo = o.Layout(glat)
    rf = o.RngField(olo, o.RNG_MILC6, SEED)
    fat = o.gauge_random(olo, rf)
    o.rephase(olo, fat)
    lng = o.gauge_random(olo, rf)
    o.rephase(olo, lng)
    bs = [o.vector_gaussian(olo, rf) for _ in MS]
    ref = q.Context(glat, device=0)                                   # one rank, the whole lattice: single-system probes
    for c in (ref, ctx):
        c.set_option("half", 1)
        c.set_option("half_batch", 1)
    ctx.set_option("batch_ranks", 1)
    res = {"rank": rank}

    def stag(c, f, l, slab):
        return q.newStag3(c, sl(f) if slab else f, sl(l) if slab else l) if l is not None else q.newStag(c, sl(f) if slab else f)

    if args.op:
        hfat, hlng = o.hisq_smear(olo, o.gauge_warm(olo, 0.5, rf))
        o.rephase(olo, hfat)
        o.rephase(olo, hlng)
        res["op"] = {}
        for kind, (f, l) in {"random": (fat, None), "random_naik": (fat, lng), "hisq": (hfat, hlng)}.items():
            stag(ref, f, l, False)
            want = {}
            for name, single in (("f32", ref.dev_op_xx_sloppy), ("half", ref.dev_op_xx_half)):
                for pe in (True, False):
                    for j, b in enumerate(bs):
                        fx, fr = ref.field_new(b), ref.field_new()
                        single(fr, fx, M2[j], pe)
                        want[name, pe, j] = sl(ref.field_download(fr))
                        ref.field_free(fx)
                        ref.field_free(fr)
            for form, overlap, hop_split in FORMS:
                ctx.set_option("overlap", overlap)
                ctx.set_option("hop_split", hop_split)
                stag(ctx, f, l, True)                                  # collective set_links (+ the sweep measurement)
                ctx.links_info_half()                                  # collective: the 16-bit copy is rebuilt here
                fx, fr = [ctx.field_new(sl(b)) for b in bs], [ctx.field_new() for _ in bs]
                ctx.dev_op_xx_sloppy_batch(fr, fx, M2, True)           # (the fp32 copy is rebuilt here, outside the counted part)
                split = ctx.sweep_info()["overlap"]                    # (a slab without interior sites, Naik on Lt = 4: one launch)
                assert split == (overlap == 1 and (loc.lat[3] > 6 or l is None)), (kind, form, split)
                counts = {}
                for name, batch in (("f32", ctx.dev_op_xx_sloppy_batch), ("half", ctx.dev_op_xx_half_batch)):
                    ctx.timers_enable(3)
                    ctx.timers_reset()
                    for pe in (True, False):
                        for fid in fr:
                            ctx.dev_zero(fid)                          # (the probe writes one parity; the reference field was new)
                        batch(fr, fx, M2, pe)
                        for j in range(len(bs)):
                            r = ctx.field_download(fr[j])
                            if not np.array_equal(r, want[name, pe, j]):
                                raise AssertionError("rank %d %s %s %s par_even=%s system %d: the sharded batched operator differs from the "
                                                     "one-rank single-system one (max %g)" % (rank, kind, form, name, pe, j,
                                                                                               np.abs(r - want[name, pe, j]).max()))
                    nbnd, nint, nx = ctx.timer("dslash_batch_%s_bnd" % name)[0], ctx.timer("dslash_batch_%s" % name)[0], ctx.timer("exchange")[0]
                    ctx.timers_enable(0)
                    # two applications of two sweeps each: one exchange and one (interior) launch per sweep, whatever n is
                    assert nx == nint == 4 and nbnd == (4 if split else 0), (kind, form, name, nx, nint, nbnd)
                    counts[name] = [nint, nbnd, nx]
                for fid in fx + fr:
                    ctx.field_free(fid)
                res["op"]["%s/%s" % (kind, form)] = {"split": int(split), "counts": counts}

    if args.solve:
        ctx.set_option("overlap", -1)
        ctx.set_option("hop_split", -1)
        s_sh = stag(ctx, fat, None, True)
        even = slice(0, olo.vol // 2)
        res["solve"] = {}

        def gather_x(xl):
            xg = np.zeros_like(bs[0])
            for r, xr in ranks.gather(w, (rank, xl)):
                xg[q.Layout(glat).shard_indices(world, r)[1]] = xr
            return xg

        def oracle_r2(full, src, xg, mass):
            if not full:
                ax = o.stagD2xx(olo, fat, None, xg, mass * mass, True)
                return float(np.sum((src[even] - ax[even]) ** 2) / np.sum(src[even] ** 2))
            dx = o.D(olo, fat, None, xg, mass)
            return float(np.sum((src - dx) ** 2) / np.sum(src ** 2))

        def single(j, sloppy, maxits):
            fb, fx = ctx.field_new(sl(bs[j])), ctx.field_new()
            its, fin, nup = ctx.dev_solve_xx_sloppy(fx, fb, MS[j], R2[j], maxits, True, sloppy)
            x = ctx.field_download(fx)
            ctx.field_free(fb)
            ctx.field_free(fx)
            return x, its, fin, nup, ctx.sloppy_last()

        def batch_xx(sloppy, maxits=5000, alone=True):
            """solveXX_batch on the sharded context: this rank's record after the checks every case shares"""
            xs = [np.zeros_like(sl(b)) for b in bs]
            its, fin, nup = s_sh.solveXX_batch(xs, [sl(b) for b in bs], MS, R2, maxits, True, sloppy=sloppy)
            last = ctx.sloppy_last_batch()
            mine = {"its": its, "nupd": nup, "r2": fin, "last": last}
            if alone:
                for j in range(len(bs)):
                    x1, its1, fin1, nup1, last1 = single(j, sloppy, maxits)
                    same = (its[j], fin[j], nup[j], last[j]) == (its1, fin1, nup1, last1) and np.array_equal(xs[j], x1)
                    if not same:
                        raise AssertionError("rank %d sloppy %d system %d: batch %r, alone %r, max |dx| %g" %
                                             (rank, sloppy, j, (its[j], fin[j], nup[j], last[j]), (its1, fin1, nup1, last1),
                                              np.abs(xs[j] - x1).max()))
            mine["oracle_r2"] = [oracle_r2(False, bs[j], gather_x(xs[j]), MS[j]) for j in range(len(bs))]
            allr = ranks.gather(w, mine)
            print("rank %d solveXX_batch sloppy=%d maxits=%d: %s" % (rank, sloppy, maxits, json.dumps(mine)), file=sys.stderr, flush=True)
            assert all((a["its"], a["nupd"], a["r2"], a["last"]) == (its, nup, fin, last) for a in allr), allr
            return mine

        for sloppy in (1, 2):
            mine = batch_xx(sloppy)
            assert all(r2 <= rq * 1.001 for r2, rq in zip(mine["oracle_r2"], R2)), mine
            assert all(l["precision"] == sloppy and l["fell_back"] == 0 for l in mine["last"]), mine
            assert len({(i + 31) // 32 for i in mine["its"]}) > 1, mine          # (they do finish in different chunks)
            res["solve"]["xx/%d" % sloppy] = mine
            # maxits: every system on every rank stops at the same count, below convergence, without error
            mine = batch_xx(sloppy, maxits=10, alone=False)
            assert mine["its"] == [10, 10, 10] and all(r2 > rq for r2, rq in zip(mine["r2"], R2)), mine
            res["solve"]["maxits/%d" % sloppy] = mine
        # the stall guard at the first reliable update: every system on every rank hands over to fp32 alike
        ctx.set_option("half_stall", 0)
        mine = batch_xx(2)
        assert all(l["fell_back"] == 1 and l["f32_iters"] > 0 for l in mine["last"]), mine
        assert all(r2 <= rq * 1.001 for r2, rq in zip(mine["oracle_r2"], R2)), mine
        res["solve"]["fallback"] = mine
        ctx.set_option("half_stall", 2)
        # the full solve: ReconL, and ReconR on a source with no odd part
        b_even = bs[1].copy()
        b_even[olo.vol // 2:] = 0
        srcs = [bs[0], b_even, bs[2]]
        sps = [q.SolverParams(r2req=rq, maxits=5000, verbosity=0) for rq in R2]
        xs = [np.zeros_like(sl(b)) for b in srcs]
        s_sh.solve_batch(xs, [sl(b) for b in srcs], MS, sps, sloppy=1)
        fb, fx = [ctx.field_new(sl(b)) for b in srcs], [ctx.field_new() for _ in srcs]
        its_d, fin_d, nup_d = ctx.dev_solve_batch(fx, fb, MS, min(R2), 5000, sloppy=1)
        full = {"its": [sp.iterations for sp in sps], "r2": [sp.r2 for sp in sps], "nupd": [sp.reliableUpdates for sp in sps],
                "oracle_r2": [oracle_r2(True, srcs[j], gather_x(xs[j]), MS[j]) for j in range(3)],
                "dev_oracle_r2": [oracle_r2(True, srcs[j], gather_x(ctx.field_download(fx[j])), MS[j]) for j in range(3)],
                "dev_its": its_d}
        for fid in fb + fx:
            ctx.field_free(fid)
        print("rank %d solve_batch sloppy=1: %s" % (rank, json.dumps(full)), file=sys.stderr, flush=True)
        assert all(r2 <= rq * 1.001 for r2, rq in zip(full["oracle_r2"], R2)), full
        assert all(r2 <= min(R2) * 1.001 for r2 in full["dev_oracle_r2"]), full
        assert all((a["its"], a["r2"], a["nupd"], a["dev_its"]) == (full["its"], full["r2"], full["nupd"], full["dev_its"])
                   for a in ranks.gather(w, full))
        res["solve"]["full"] = full

    if args.top:
        # as tests/conn4d_rank_worker.py's e2e: the same configuration, points, mass, r2req and bound; here the sharded side is sloppy = 1
        MASS, R2REQ = 0.1, 1e-20
        glo = q.Layout(glat)
        lt, nt = loc.lat[3], glat[3]
        ctx.set_option("overlap", -1)
        ctx.set_option("hop_split", -1)
        g = q.RngField(glat, q.RngMilc6, SEED).warm(0.5)
        q.rephase(glo, g)
        s1 = q.newStag(ref, g)
        sn = q.newStag(ctx, np.ascontiguousarray(g[idx]))
        mpts = [[0, 0, 0, 0], [2, 4, 2, nt - 2], [1, 2, 0, lt]]
        l1, e1, st1 = q.connMeson(s1, glo, mpts, MASS, R2REQ, out=None)
        ln, en, stn = q.connMeson(sn, loc, mpts, MASS, R2REQ, t_offset=rank * lt, sloppy=1, out=None)
        # two solutions with |b - (D+m)x|^2 <= r2req |b|^2, |b| = 1, differ by at most eps = 2 sqrt(r2req) / m in norm, so per site
        # |d locmes| <= sum_systems scal (2 max|phi| eps + eps^2); max|phi| <= sqrt(max|locmes| / scal)   (conn4d_rank_worker.py)
        eps_s = 2.0 * np.sqrt(R2REQ) / MASS
        maxphi = float(np.sqrt(len(mpts) * np.abs(l1).max()))
        bound_s = 3 * len(mpts) * (1.0 / len(mpts)) * (2.0 * maxphi * eps_s + eps_s * eps_s)
        dl, de = float(np.abs(ln - l1[idx]).max()), float(np.abs(en - e1).max())
        res["top"] = {"locmes_dev": dl, "est_dev": de, "bound": bound_s, "slice_sites": glo.vol // nt,
                      "iterations": [min(stn["iterations"]), max(stn["iterations"])],
                      "one_rank_iterations": [min(st1["iterations"]), max(st1["iterations"])],
                      "precision": sorted({l["precision"] for l in ctx.sloppy_last_batch()})}
        print("rank %d top: %s" % (rank, json.dumps(res["top"])), file=sys.stderr, flush=True)
        assert dl <= bound_s and de <= (glo.vol // nt) * bound_s, res["top"]
        assert res["top"]["precision"] == [1], res["top"]

    ranks.finish(w, "SLOPPY_BATCH_RANKS_OK", res)
    ctx.close()
    ref.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
