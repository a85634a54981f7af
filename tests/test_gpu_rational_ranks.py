"""The accumulating multi-shift solve and the rational HISQ force on t-sharded lattices: both are collective, the new kernels are
site-local, the scalar side is the sharded branch of the multi-shift solve.

The ranks are started by torch.distributed.run as fresh processes that all bind GPU 0 and talk over the peer-memory transport;
tests/rational_rank_worker.py checks every rank's slab against a one-rank context of the whole lattice and the binary128
reference.  Observed values are printed (pytest -s)."""
import pytest

from ranks import launch_ok

pytestmark = pytest.mark.gpu


def test_sharded_rational_solve_and_force_are_the_one_rank_ones():
    """2 ranks on 8^4, five poles: every rank's slab of S within the relation of tests/test_gpu_rational.py to the binary128
    reference (yardstick: the one-rank existing path), the force slab at 2e-11 of the one-rank force (both asserted by the worker),
    the same iteration counts on both ranks."""
    res = launch_ok(2, "rational_rank_worker.py", [8, 8, 8, 8], "RATIONAL_RANKS_OK", 300, env={"QEXHIP_PEER_TIMEOUT": "60"})
    v = res[0]
    print("2 ranks 8^4: rational solve %d iterations (one rank %d, existing path %d), force solve %d (one rank %d)" % (
        v["iters"], v["one_rank_iters"], v["existing_iters"], v["force_iters"], v["one_rank_force_iters"]))
    for r in res:
        print("  rank %d: |S - ref| %.3e (existing path %.3e, one-rank new %.3e) of |ref| on the slab; force %.3e" % (
            r["rank"], r["sum_dev"], r["existing_dev"], r["one_rank_sum_dev"], r["force_dev"]))
    assert all(r["iters"] == v["iters"] and r["force_iters"] == v["force_iters"] for r in res)
