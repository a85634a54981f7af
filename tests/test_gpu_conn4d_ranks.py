"""The connected scalar correlator on t-sharded lattices: point sources by GLOBAL coordinate, the translation across the rank
boundary, the sign, the rank-global slice table and the connMeson driver.

The ranks are started by torch.distributed.run as fresh processes that all bind GPU 0 and talk over the peer-memory transport;
tests/conn4d_rank_worker.py checks every rank's slab against a one-rank context of the whole lattice, bit for bit.

Lattices as in tests/test_gpu_scalar_trace_ranks.py: 8^4, and 8.8.6.8 whose 192-site slices of one parity end in a partial 256-site
chunk; the driver runs end to end on the second.  Observed values are printed (pytest -s)."""
import pytest

from ranks import launch_ok

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("lat,extra", [([8, 8, 8, 8], ()), ([8, 8, 6, 8], ("e2e",))])
def test_sharded_conn4d_is_the_one_rank_conn4d(lat, extra):
    """point sources, accumulation with pt_t = 0, 2, 4, 6 and an odd-sum point, sign and slice table on identical uploaded global
    fields: every rank's slab and the whole table equal the one-rank result bit for bit; with e2e, connMeson (fp64) gives the
    one-rank locmes and est within the solver bound, and sloppy = 1 is refused as dev_solve_batch refuses it"""
    res = launch_ok(2, "conn4d_rank_worker.py", lat + list(extra), "CONN4D_RANKS_OK", 300, env={"QEXHIP_PEER_TIMEOUT": "60"})
    for r in res:
        assert r["point"] == r["accum"] == r["sign"] == r["slices"] == "equal"
        if extra:
            e = r["e2e"]
            print("2 ranks %s rank %d: %s" % (lat, r["rank"], e))
            assert e["locmes_dev"] <= e["bound"] and e["est_dev"] <= e["slice_sites"] * e["bound"] and e["sloppy_refused"]
