"""Stout smearing on t-sharded lattices: the ghost slices of the links of every level and of cg in the backward stencil, the
rank-global sums of the inverse and the agreement of the ranks on its loop control.

The ranks are started by torch.distributed.run as fresh processes that all bind GPU 0 and talk over the peer-memory transport;
tests/stout_rank_worker.py checks every rank's slab against a one-rank context of the whole lattice.  Observed values are printed
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


def _launch(nranks, lat, timeout=600):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", QEXHIP_PEER_TIMEOUT="60",
               OMP_NUM_THREADS=str(max(1, min(16, len(os.sched_getaffinity(0))) // nranks)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nranks), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "stout_rank_worker.py")] + [str(v) for v in lat]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, cwd=ROOT, env=env)
    ok = [ln for ln in p.stdout.splitlines() if ln.startswith("STOUT_RANKS_OK ")]
    print(p.stderr[-6000:] if (p.returncode != 0 or len(ok) != 1) else "\n".join(ln for ln in p.stderr.splitlines() if ln.startswith("rank ")))
    assert p.returncode == 0 and len(ok) == 1, (p.returncode, p.stdout[-2000:])
    res = json.loads(ok[0].split(" ", 1)[1])
    assert [r["rank"] for r in res] == list(range(nranks))
    return res


@pytest.mark.parametrize("nranks,lat", [(2, [8, 8, 8, 8]), (4, [8, 8, 8, 16])])
def test_sharded_stout_smearing_is_the_one_rank_stout_smearing(nranks, lat):
    """Every rank's slab of the smeared links (one step, three levels) and of the three-level force is the one-rank result bit for
    bit (asserted by the worker); the inverse stops after the same iterations on every rank, within +-1 of the one-rank count, and
    the gathered result has del2 <= 1e-24."""
    res = _launch(nranks, lat)
    v = res[0]["inverse"]
    print("%d ranks %s: inverse %d iterations (one rank: %d), rdf2 %.3e, del2 %.3e" % (nranks, lat, v["iters"], v["one_rank_iters"], v["rdf2"], v["del2"]))
    assert all(r["inverse"]["iters"] == v["iters"] for r in res)
    assert abs(v["iters"] - v["one_rank_iters"]) <= 1 and v["del2"] <= 1e-24
