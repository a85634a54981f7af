"""The low-mode eigensolver and the deflated solve on a t-sharded lattice: block dots that end in ONE rank sum, the operator's face
exchange inside the Lanczos recurrence, and the agreement of the ranks on every host-side decision.

The ranks are started by torch.distributed.run as fresh processes that all bind GPU 0 and talk over the peer-memory transport;
tests/eig_rank_worker.py checks the sharded run against the dense spectrum and a one-rank context of the whole lattice.  Observed
values are printed (pytest -s)."""
import pytest

from ranks import launch_ok

pytestmark = pytest.mark.gpu


def test_sharded_eigensolver_and_deflated_solve():
    """4.4.8.8 as 2 x (4.4.8.4): identical evals / resid on both ranks, Weyl's bound against the dense spectrum, the oracle residual
    of the gathered vectors, and the deflated solve's iterations within 2 % (at least 2) of the one-rank run's."""
    res = launch_ok(2, "eig_rank_worker.py", [4, 4, 8, 8], "EIG_RANKS_OK", 300, env={"QEXHIP_PEER_TIMEOUT": "60"})
    v = res[0]
    print("2 ranks: nconv %d, %s; deflated %d its (one rank %d, undeflated %d); max oracle resid %.2e, |V^+V - 1| %.2e, max |lambda - dense| %.2e"
          % (v["nconv"], v["stats"], v["deflated_its"], v["one_rank_deflated_its"], v["plain_its"], v["oracle_resid_max"], v["orth"], v["max_eval_dev"]))
    assert all(r["evals"] == v["evals"] and r["resid"] == v["resid"] and r["deflated_its"] == v["deflated_its"] for r in res)
    assert v["nconv"] == 8
