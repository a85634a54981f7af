"""The deflated lock-step batch on a t-sharded lattice: the multi-right-hand-side block dot that ends in ONE rank sum, the single-parity
sweeps of the odd projection with their face exchange, and the agreement of the ranks on every host-side decision.

The ranks are started by torch.distributed.run as fresh processes that all bind GPU 0 and talk over the peer-memory transport;
tests/defl_batch_rank_worker.py checks the sharded run against a one-rank context of the whole lattice.  Observed values are printed
(pytest -s)."""
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


def _launch(nranks, lat, limit=300):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", QEXHIP_PEER_TIMEOUT="60",
               OMP_NUM_THREADS=str(max(1, min(16, len(os.sched_getaffinity(0))) // nranks)))
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nranks),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "defl_batch_rank_worker.py")] + [str(v) for v in lat]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=limit + 30, cwd=ROOT, env=env)
    ok = [ln for ln in p.stdout.splitlines() if ln.startswith("DEFL_BATCH_RANKS_OK ")]
    print(p.stderr[-6000:] if (p.returncode != 0 or len(ok) != 1) else "\n".join(ln for ln in p.stderr.splitlines() if ln.startswith("rank ")))
    assert p.returncode == 0 and len(ok) == 1, (p.returncode, p.stdout[-2000:])
    res = json.loads(ok[0].split(" ", 1)[1])
    assert [r["rank"] for r in res] == list(range(nranks))
    return res


def test_sharded_deflated_batch_on_both_parities():
    """4.4.8.8 as 2 x (4.4.8.4), fp64, four systems per parity: identical iterations and residuals on both ranks, iterations within
    2 % (at least 2) of the one-rank run's, the gathered solutions within 1e-9 of the one-rank ones; sloppy = 1 is refused"""
    res = _launch(2, [4, 4, 8, 8])
    v = res[0]
    for par in ("even", "odd"):
        print("2 ranks, %s: deflated %s its (one rank %s), r2/b2 %s, max |x - one rank| %.2e" %
              (par, v[par]["its"], v[par]["one_rank_its"], ["%.3e" % r for r in v[par]["r2"]], v[par]["xerr"]))
        assert all(r[par]["its"] == v[par]["its"] and r[par]["r2"] == v[par]["r2"] for r in res)
        assert all(abs(a - b) <= max(2, 0.02 * b) for a, b in zip(v[par]["its"], v[par]["one_rank_its"]))
        assert v[par]["xerr"] <= 1e-9
    assert all(r["sloppy_rc"] == -1 for r in res)
