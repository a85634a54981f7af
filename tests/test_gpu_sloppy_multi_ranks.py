"""Mixed-precision multi-shift CG on a t-sharded lattice: two ranks, started by torch.distributed.run as fresh processes that both
bind GPU 0 and talk over the peer-memory transport (tests/sloppy_multi_rank_worker.py holds the checks: the same iterations, updates,
refinement iterations and residuals on every rank; the gathered solutions' true residuals against the oracle).  Observed values are
printed (pytest -s)."""
import pytest

from ranks import launch_ok

pytestmark = pytest.mark.gpu


def test_two_ranks_multi_shift_sloppy():
    """2 ranks on 8^4, g.random plain and with Naik links, 4 shifts at r2req 1e-14, both parities"""
    res = launch_ok(2, "sloppy_multi_rank_worker.py", [8, 8, 8, 8], "SLOPPY_MULTI_RANKS_OK", 600, env={"QEXHIP_PEER_TIMEOUT": "60"})
    keys = [k for k in res[0] if k != "rank"]
    assert sorted(keys) == ["random/even", "random/odd", "random_naik/even", "random_naik/odd"]
    for key in keys:
        v = res[0][key]
        print(f"2 ranks 8^4 {key}: {v['its']} its / {v['nupd']} updates, refine {v['refine']}, true r2/b2 {v['oracle_r2']}")
        assert all(r[key]["its"] == v["its"] and r[key]["nupd"] == v["nupd"] and r[key]["refine"] == v["refine"] and r[key]["r2"] == v["r2"]
                   for r in res)
        assert all(x <= 1e-14 * (1.0 + 1e-4) for x in v["oracle_r2"])
