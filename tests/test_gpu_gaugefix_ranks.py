"""Gauge fixing on t-sharded lattices: the ghost slices of the links, the t-faces of the transform field (Landau gauge), the
rank-global metrics and the agreement of the ranks on the loop control.

The ranks are started by torch.distributed.run as fresh processes that all bind GPU 0 and talk over the peer-memory transport;
tests/gaugefix_rank_worker.py checks every rank's slab against a one-rank context of the whole lattice.  Observed values are
printed (pytest -s)."""
import pytest

from ranks import launch_ok

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nranks,lat", [(2, [8, 8, 8, 8]), (4, [8, 8, 8, 16])])
def test_sharded_gauge_fixing_is_the_one_rank_gauge_fixing(nranks, lat):
    """Coulomb and Landau: the slab of t after 40 relax iterations is the one-rank t bit for bit; the full fix converges with the
    same iterations on every rank, the gathered t has gdsq <= gstop and is in SU(3); plaquettes after the transform agree to 1e-13."""
    res = launch_ok(nranks, "gaugefix_rank_worker.py", lat, "GAUGEFIX_RANKS_OK", 600, env={"QEXHIP_PEER_TIMEOUT": "60"})
    for name in ("coulomb", "landau"):
        v = res[0][name]
        print("%d ranks %s %s: %d iterations (one rank: %d), gdsq %.3e (numpy %.3e)" %
              (nranks, lat, name, v["iters"], v["one_rank_iters"], v["gdsq"], v["numpy_gdsq"]))
        assert all(r[name]["iters"] == v["iters"] for r in res)
