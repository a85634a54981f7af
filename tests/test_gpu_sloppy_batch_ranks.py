"""Mixed-precision lock-step batches on t-sharded lattices (option "batch_ranks" = 1): the HALO form of the lock-step reduced-precision
sweep, all systems' faces in one exchange, one collective per reduction point for all systems, and the per-system agreement check.

The ranks are started by torch.distributed.run as fresh processes that all bind GPU 0 and talk over the peer-memory transport
(tests/sloppy_batch_rank_worker.py checks every rank's slab against a one-rank context of the whole lattice and every batched system
against its single-system solve on the same sharded context; operator, solve and workload checks share ONE launch per shape).  A hang
-- ranks that post different numbers of messages -- ends at the launcher's limit and fails the test.  The one-rank halo path runs in
tests/test_gpu_sloppy_batch_halo.py.  Observed values are printed (pytest -s)."""
import pytest

from ranks import launch_ok
from sloppy_batch_rank_worker import R2

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nranks,lat,top", [(2, [8, 8, 8, 8], True), (2, [8, 8, 8, 16], False), (4, [8, 8, 8, 16], False)])
def test_sharded_sloppy_batches(nranks, lat, top):
    """2 ranks x 8^4: local Lt = 4, the Naik slab has no interior and runs one launch whatever `overlap` says; 2 ranks x 8.8.8.16: local
    Lt = 8, the split form runs all three site ranges, upper == lower; 4 ranks x 8.8.8.16: upper and lower are distinct processes.
    Operator: every system of dev_op_xx_sloppy_batch / dev_op_xx_half_batch on every slab == the slab of the one-rank single-system
    probe, for g.random, g.random + Naik and HISQ links in the three sweep forms, one exchange per sweep.  Solve and workload: see the
    worker."""
    res = launch_ok(nranks, "sloppy_batch_rank_worker.py", lat + ["--op", "--solve"] + (["--top"] if top else []), "SLOPPY_BATCH_RANKS_OK",
                    600, env={"QEXHIP_PEER_TIMEOUT": "60"})
    for r in res:
        assert len(r["op"]) == 9, r["op"].keys()
        assert r["op"]["random/fused_requested"]["split"] == 1 and r["op"]["random/exchange_first"]["split"] == 0
        assert r["op"]["random/by_sites"]["counts"] == {"f32": [4, 4, 4], "half": [4, 4, 4]}
        assert len(r["solve"]) == 6, r["solve"].keys()
    for key, v in res[0]["solve"].items():
        print(f"{nranks} ranks {lat} {key}: its {v['its']} updates {v['nupd']} r2 {v['r2']} oracle r2 {v['oracle_r2']} last {v.get('last')}")
        assert all(r["solve"][key]["its"] == v["its"] and r["solve"][key]["r2"] == v["r2"] and r["solve"][key].get("last") == v.get("last")
                   for r in res)
    for s in (1, 2):
        assert all(o <= rq * 1.001 for o, rq in zip(res[0]["solve"]["xx/%d" % s]["oracle_r2"], R2))
    if top:
        for r in res:
            e = r["top"]
            print("%d ranks %s rank %d connMeson sloppy=1: %s" % (nranks, lat, r["rank"], e))
            assert e["locmes_dev"] <= e["bound"] and e["est_dev"] <= e["slice_sites"] * e["bound"]
