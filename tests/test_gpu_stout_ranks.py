"""Stout smearing on t-sharded lattices: the ghost slices of the links of every level and of cg in the backward stencil, the
rank-global sums of the inverse and the agreement of the ranks on its loop control.

The ranks are started by torch.distributed.run as fresh processes that all bind GPU 0 and talk over the peer-memory transport;
tests/stout_rank_worker.py checks every rank's slab against a one-rank context of the whole lattice.  Observed values are printed
(pytest -s)."""
import pytest

from ranks import launch_ok

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nranks,lat", [(2, [8, 8, 8, 8]), (4, [8, 8, 8, 16])])
def test_sharded_stout_smearing_is_the_one_rank_stout_smearing(nranks, lat):
    """Every rank's slab of the smeared links (one step, three levels) and of the three-level force is the one-rank result bit for
    bit (asserted by the worker); the inverse stops after the same iterations on every rank, within +-1 of the one-rank count, and
    the gathered result has del2 <= 1e-24."""
    res = launch_ok(nranks, "stout_rank_worker.py", lat, "STOUT_RANKS_OK", 600, env={"QEXHIP_PEER_TIMEOUT": "60"})
    v = res[0]["inverse"]
    print("%d ranks %s: inverse %d iterations (one rank: %d), rdf2 %.3e, del2 %.3e" % (nranks, lat, v["iters"], v["one_rank_iters"], v["rdf2"], v["del2"]))
    assert all(r["inverse"]["iters"] == v["iters"] for r in res)
    assert abs(v["iters"] - v["one_rank_iters"]) <= 1 and v["del2"] <= 1e-24
