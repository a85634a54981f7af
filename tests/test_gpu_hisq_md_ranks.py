"""The resident HISQ molecular dynamics on t-sharded lattices: the ghost slices of the phased links and of every level of the
closure, the hop-1 and hop-3 neighbours of the outer products across the slab boundary, the chain's exchanges.

The ranks are started by torch.distributed.run as fresh processes that all bind GPU 0 and talk over the peer-memory transport;
tests/hisq_md_rank_worker.py checks every rank's slab against a one-rank context of the whole lattice.  Observed values are printed
(pytest -s)."""
import pytest

from ranks import launch_ok

pytestmark = pytest.mark.gpu


def test_sharded_hisq_md_is_the_one_rank_hisq_md():
    """2 ranks on 8^4: every rank's slab of the force, the momenta and the links after two MD steps (update_links, hisq_prepare,
    hisq_fforce with three vectors) is the one-rank result bit for bit (asserted by the worker); hisq_fforce_solve stops after the
    same iterations on every rank"""
    res = launch_ok(2, "hisq_md_rank_worker.py", [8, 8, 8, 8], "HISQ_MD_RANKS_OK", 600, env={"QEXHIP_PEER_TIMEOUT": "60"})
    v = res[0]
    print("2 ranks 8^4: solve + force iterations %r (one rank: %r), force deviation from one rank %.3e of max |f|" % (
        v["iters"], v["one_rank_iters"], max(r["solve_force_dev"] for r in res)))
    assert all(r["iters"] == v["iters"] for r in res)
