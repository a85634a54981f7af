"""The accumulating multi-shift solve and the rational HISQ force on t-sharded lattices: both are collective, the new kernels are
site-local, the scalar side is the sharded branch of the multi-shift solve.

The ranks are started by torch.distributed.run as fresh processes that all bind GPU 0 and talk over the peer-memory transport;
tests/rational_rank_worker.py checks every rank's slab against a one-rank context of the whole lattice and the binary128
reference.  Observed values are printed (pytest -s)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    import socket

    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def _launch(nranks, lat, timeout=300):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", QEXHIP_PEER_TIMEOUT="60",
               OMP_NUM_THREADS=str(max(1, min(16, len(os.sched_getaffinity(0))) // nranks)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nranks), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "rational_rank_worker.py")] + [str(v) for v in lat]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, cwd=ROOT, env=env)
    ok = [ln for ln in p.stdout.splitlines() if ln.startswith("RATIONAL_RANKS_OK ")]
    print(p.stderr[-6000:] if (p.returncode != 0 or len(ok) != 1) else "\n".join(ln for ln in p.stderr.splitlines() if ln.startswith("rank ")))
    assert p.returncode == 0 and len(ok) == 1, (p.returncode, p.stdout[-2000:])
    res = json.loads(ok[0].split(" ", 1)[1])
    assert [r["rank"] for r in res] == list(range(nranks))
    return res


def test_sharded_rational_solve_and_force_are_the_one_rank_ones():
    """2 ranks on 8^4, five poles: every rank's slab of S within the relation of tests/test_gpu_rational.py to the binary128
    reference (yardstick: the one-rank existing path), the force slab at 2e-11 of the one-rank force (both asserted by the worker),
    the same iteration counts on both ranks."""
    res = _launch(2, [8, 8, 8, 8])
    v = res[0]
    print("2 ranks 8^4: rational solve %d iterations (one rank %d, existing path %d), force solve %d (one rank %d)" % (
        v["iters"], v["one_rank_iters"], v["existing_iters"], v["force_iters"], v["one_rank_force_iters"]))
    for r in res:
        print("  rank %d: |S - ref| %.3e (existing path %.3e, one-rank new %.3e) of |ref| on the slab; force %.3e" % (
            r["rank"], r["sum_dev"], r["existing_dev"], r["one_rank_sum_dev"], r["force_dev"]))
    assert all(r["iters"] == v["iters"] and r["force_iters"] == v["force_iters"] for r in res)
