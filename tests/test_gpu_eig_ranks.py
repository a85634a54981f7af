"""The low-mode eigensolver and the deflated solve on a t-sharded lattice: block dots that end in ONE rank sum, the operator's face
exchange inside the Lanczos recurrence, and the agreement of the ranks on every host-side decision.

The ranks are started by torch.distributed.run as fresh processes that all bind GPU 0 and talk over the peer-memory transport;
tests/eig_rank_worker.py checks the sharded run against the dense spectrum and a one-rank context of the whole lattice.  Observed
values are printed (pytest -s)."""
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
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "eig_rank_worker.py")] + [str(v) for v in lat]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=limit + 30, cwd=ROOT, env=env)
    ok = [ln for ln in p.stdout.splitlines() if ln.startswith("EIG_RANKS_OK ")]
    print(p.stderr[-6000:] if (p.returncode != 0 or len(ok) != 1) else "\n".join(ln for ln in p.stderr.splitlines() if ln.startswith("rank ")))
    assert p.returncode == 0 and len(ok) == 1, (p.returncode, p.stdout[-2000:])
    res = json.loads(ok[0].split(" ", 1)[1])
    assert [r["rank"] for r in res] == list(range(nranks))
    return res


def test_sharded_eigensolver_and_deflated_solve():
    """4.4.8.8 as 2 x (4.4.8.4): identical evals / resid on both ranks, Weyl's bound against the dense spectrum, the oracle residual
    of the gathered vectors, and the deflated solve's iterations within 2 % (at least 2) of the one-rank run's."""
    res = _launch(2, [4, 4, 8, 8])
    v = res[0]
    print("2 ranks: nconv %d, %s; deflated %d its (one rank %d, undeflated %d); max oracle resid %.2e, |V^+V - 1| %.2e, max |lambda - dense| %.2e"
          % (v["nconv"], v["stats"], v["deflated_its"], v["one_rank_deflated_its"], v["plain_its"], v["oracle_resid_max"], v["orth"], v["max_eval_dev"]))
    assert all(r["evals"] == v["evals"] and r["resid"] == v["resid"] and r["deflated_its"] == v["deflated_its"] for r in res)
    assert v["nconv"] == 8
