"""Worker of tests/test_gpu_lossless.py, test_gpu_link_packed.py and test_gpu_link_ortho.py (lossless_links.two_ranks): two ranks
sharing device 0 on the peer transport, t-sharded, the fused sweep forced (overlap 1, hop_split 2).  Each rank takes QEX g.random on
its slab and computes D, stagD2ee and a fixed-length CG with option lossless = FORM (1 the 108-byte residual form, 2 the packed
100-byte form, 3 the orthogonal 92-byte form) and then 0; everything must agree bit for bit.

  python -m torch.distributed.run --nproc-per-node 2 tests/lossless_rank_worker.py FORM LX LY LZ LT_GLOBAL

Prints one line `LOSSLESS rank r {...}` per rank.
"""
import json
import os
import sys

import numpy as np

import ranks


def main():
    form = int(sys.argv[1])
    lat = [int(v) for v in sys.argv[2:6]]
    os.environ["QEXHIP_TRANSPORT"] = "peer"           # insisted on, not found out by comparing devices
    rk = ranks.shard(lat)
    rank, ctx = rk.rank, rk.ctx
    import qex_amd as q
    from oracle import oracle as o

    lo = o.Layout(rk.loc.lat)
    rf = o.RngField(lo, o.RNG_MILC6, 987654321 + rank)
    g = o.gauge_random(lo, rf)
    o.rephase(lo, g)
    b = o.vector_gaussian(lo, rf)
    ctx.set_option("overlap", 1)
    ctx.set_option("hop_split", 2)
    res, out = {}, {"rank": rank}
    for lossless in (form, 0):
        ctx.set_option("lossless", lossless)
        s = q.newStag(ctx, g)
        r = {"storage": s.links_storage(), "form": 2 if ctx.sweep_tuning()["form"] == "fused" else 0}
        d = np.zeros_like(b)
        s.D(d, b, 0.1)
        r["D"] = d.copy()
        s.stagD2ee(d, b, 0.01)
        r["stagD2ee"] = d.copy()
        sp = q.SolverParams(r2req=0.0, maxits=60, verbosity=0)
        x = np.zeros_like(b)
        s.solveEE(x, b, 0.1, sp, histcap=80)
        r["hist"], r["x"], r["its"] = np.array(sp.r2hist), x.copy(), int(sp.iterations)
        res[lossless] = r
    out["storage"], out["storage_ref"], out["form"] = res[form]["storage"], res[0]["storage"], res[form]["form"]
    out["equal"] = {k: bool(np.array_equal(res[form][k], res[0][k])) for k in ("D", "stagD2ee", "hist", "x", "its")}
    sys.stdout.write("\nLOSSLESS rank %d %s\n" % (rank, json.dumps(out)))
    sys.stdout.flush()
    os._exit(0)


if __name__ == "__main__":
    main()
