"""The deflated lock-step batch on a t-sharded lattice: the multi-right-hand-side block dot that ends in ONE rank sum, the single-parity
sweeps of the odd projection with their face exchange, and the agreement of the ranks on every host-side decision.

The ranks are started by torch.distributed.run as fresh processes that all bind GPU 0 and talk over the peer-memory transport;
tests/defl_batch_rank_worker.py checks the sharded run against a one-rank context of the whole lattice.  Observed values are printed
(pytest -s)."""
import pytest

from ranks import launch_ok

pytestmark = pytest.mark.gpu


def test_sharded_deflated_batch_on_both_parities():
    """4.4.8.8 as 2 x (4.4.8.4), fp64, four systems per parity: identical iterations and residuals on both ranks, iterations within
    2 % (at least 2) of the one-rank run's, the gathered solutions within 1e-9 of the one-rank ones; sloppy = 1 is refused"""
    res = launch_ok(2, "defl_batch_rank_worker.py", [4, 4, 8, 8], "DEFL_BATCH_RANKS_OK", 300, env={"QEXHIP_PEER_TIMEOUT": "60"})
    v = res[0]
    for par in ("even", "odd"):
        print("2 ranks, %s: deflated %s its (one rank %s), r2/b2 %s, max |x - one rank| %.2e" %
              (par, v[par]["its"], v[par]["one_rank_its"], ["%.3e" % r for r in v[par]["r2"]], v[par]["xerr"]))
        assert all(r[par]["its"] == v[par]["its"] and r[par]["r2"] == v[par]["r2"] for r in res)
        assert all(abs(a - b) <= max(2, 0.02 * b) for a, b in zip(v[par]["its"], v[par]["one_rank_its"]))
        assert v[par]["xerr"] <= 1e-9
    assert all(r["sloppy_rc"] == -1 for r in res)
