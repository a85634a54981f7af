"""The stochastic scalar trace on t-sharded lattices: dilution by GLOBAL time, the cfield of a slab, the rank-global slice table and
the scalarTrace driver.

The ranks are started by torch.distributed.run as fresh processes that all bind GPU 0 and talk over the peer-memory transport;
tests/scalar_trace_rank_worker.py checks every rank's slab against a one-rank context of the whole lattice, bit for bit.

Sharding in t needs X*Y*Z/2 to be a multiple of 64 and an even local t extent (geom_init), so 4.4.4.8 and 4.6.10.6 cannot be split:
beside 8^4 the second lattice is 8.8.6.8, whose 192-site slices of one parity end in a partial 256-site chunk, and the driver runs
end to end on it.  Observed values are printed (pytest -s)."""
import pytest

from ranks import launch_ok

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("lat,extra", [([8, 8, 8, 8], ()), ([8, 8, 6, 8], ("e2e",))])
def test_sharded_scalar_trace_is_the_one_rank_scalar_trace(lat, extra):
    """dilute, accumulate and the slice table on identical uploaded global fields: every rank's slab and the whole table equal the
    one-rank result bit for bit; with e2e, scalarTrace (fp64) gives the one-rank est[t] and trace to 1e-9 of max|trace|"""
    res = launch_ok(2, "scalar_trace_rank_worker.py", lat + list(extra), "SCALAR_TRACE_RANKS_OK", 300, env={"QEXHIP_PEER_TIMEOUT": "60"})
    for r in res:
        assert r["dilute"] == r["accum"] == r["slices"] == "equal"
        if extra:
            print("2 ranks %s rank %d: %s" % (lat, r["rank"], r["e2e"]))
            assert r["e2e"]["est_dev"] < 1e-9 and r["e2e"]["trace_dev"] < 1e-9
