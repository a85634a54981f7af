"""Low-mode averaging of the scalar trace on a t-sharded lattice: the single-parity sweeps of lowmode_diag and project_out with their
face exchange, the multi-right-hand-side block dots that end in one rank sum, and scalarTrace(lma=True) end to end.

The ranks are started by torch.distributed.run as fresh processes that all bind GPU 0 and talk over the peer-memory transport;
tests/lma_rank_worker.py checks the sharded run against a one-rank context of the whole lattice holding the same basis vectors.
Sharding in t needs X*Y*Z/2 to be a multiple of 64 and an even local t extent, so 4.4.4.8 cannot be split: the lattice is 4.4.8.8
as 2 x (4.4.8.4), that of the sharded deflated batch.  Observed values are printed (pytest -s)."""
import pytest

from ranks import launch_ok

pytestmark = pytest.mark.gpu


def test_sharded_lma_is_the_one_rank_lma():
    res = launch_ok(2, "lma_rank_worker.py", [4, 4, 8, 8], "LMA_RANKS_OK", 300, env={"QEXHIP_PEER_TIMEOUT": "60"})
    for r in res:
        print("2 ranks 4.4.8.8 rank %d: %s" % (r["rank"], {k: v for k, v in r.items() if k != "est"}))
        assert r["low_dev"] < 1e-12 and r["project_dev"] < 1e-12 and r["low_trace_dev"] < 1e-12 and r["low_est_dev"] < 1e-12
        assert r["trace_dev"] < 1e-9 and r["est_dev"] < 1e-9
    assert res[0]["est"] == res[1]["est"]
