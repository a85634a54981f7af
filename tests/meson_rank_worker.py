"""Worker of tests/test_gpu_mesons.py::test_ranks_give_bit_identical_tables: one process per rank (torch.distributed.run), every
rank on device 0, the lattice split along t.  Every rank builds the same GLOBAL fields, uploads its t-slab and checks:

  meson tables (qexhip_dev_meson_corners)   printed as hex floats: the test holds 1, 2 and 4 ranks to the same bits
  symShift of its slab                      against the global numpy result, 1e-14
  norm2slice along x and t                  against numpy, 1e-14

usage: python -m torch.distributed.run --nproc-per-node N meson_rank_worker.py LX LY LZ LT
Exit status 0, a line `MESON_RANK_OK <rank> <json>` per rank and `MESON_TABLES <json>` from rank 0."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

import ranks

SEED = 987654321


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lat", type=int, nargs=4)
    args = ap.parse_args()
    # (one rank: a context without a communicator; the transport is not asserted here)
    rank, world, dist, ctx, loc, idx, sl = ranks.shard(args.lat, peer=False, comm=int(os.environ["WORLD_SIZE"]) > 1)
    import qex_amd as q
    import meson_ref as mr
    from oracle import oracle as o

    glat = list(args.lat)
    glo, olo = q.Layout(glat), o.Layout(glat)
    rf = o.RngField(olo, o.RNG_MILC6, SEED)
    g = o.gauge_warm(olo, 0.5, rf)
    o.rephase(olo, g)
    rng = np.random.default_rng(7)
    fs = [rng.standard_normal((glo.vol, 3, 2)) for _ in range(6)]
    lt = glat[3] // world
    ids = [ctx.field_new(np.ascontiguousarray(f[idx])) for f in fs]
    tables = {}
    for name, xs, ys, t0 in (("pairs3", ids[:3], ids[3:6], 3), ("one_wrap", ids[:1], ids[1:2], glat[3] - 1), ("norm", ids[:1], ids[:1], 0)):
        c = ctx.dev_meson_corners(xs, ys, t0)
        ref = mr.local_mesons(glo, [fs[ids.index(i)] for i in xs], [fs[ids.index(i)] for i in ys], t0)
        err = float(np.abs(c - ref).max() / np.abs(ref).max())
        assert err < 1e-13, (name, err)
        tables[name] = [float(v).hex() for v in c.ravel()]
    s = q.newStag(ctx, np.ascontiguousarray(g[idx]))
    assert s.links_info()[1] == 1
    fr = ctx.field_new()
    for mu in range(3):
        s.symShift(fr, ids[0], mu)
        ref = mr.sym_shift(glo, g, fs[0], mu)[idx]
        err = float(np.abs(ctx.field_download(fr) - ref).max() / np.abs(ref).max())
        assert err < 1e-14, (mu, err)
    for d in (0, 3):
        ref = np.zeros(glat[d])
        np.add.at(ref, glo.coords[:, d], (fs[2] ** 2).sum(axis=(1, 2)))
        got = ctx.dev_norm2slice(ids[2], d)
        err = float(np.abs(got - ref).max() / np.abs(ref).max())
        assert got.shape == (glat[d],) and err < 1e-14, (d, err)
    # one short line per rank (long lines of several processes interleave in the launcher's pipe): the digest of the tables it
    # received; rank 0 adds the tables themselves
    digest = hashlib.sha256(json.dumps(tables, sort_keys=True).encode()).hexdigest()
    print("MESON_RANK_OK %d %s" % (rank, json.dumps({"digest": digest, "lt": lt})), flush=True)
    dist.barrier()
    if rank == 0:
        print("MESON_TABLES %s" % json.dumps(tables), flush=True)
    dist.barrier()
    for fid in ids + [fr]:
        ctx.field_free(fid)
    ctx.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
