"""The resident HISQ molecular dynamics on t-sharded lattices: the ghost slices of the phased links and of every level of the
closure, the hop-1 and hop-3 neighbours of the outer products across the slab boundary, the chain's exchanges.

The ranks are started by torch.distributed.run as fresh processes that all bind GPU 0 and talk over the peer-memory transport;
tests/hisq_md_rank_worker.py checks every rank's slab against a one-rank context of the whole lattice.  Observed values are printed
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
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "hisq_md_rank_worker.py")] + [str(v) for v in lat]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, cwd=ROOT, env=env)
    ok = [ln for ln in p.stdout.splitlines() if ln.startswith("HISQ_MD_RANKS_OK ")]
    print(p.stderr[-6000:] if (p.returncode != 0 or len(ok) != 1) else "\n".join(ln for ln in p.stderr.splitlines() if ln.startswith("rank ")))
    assert p.returncode == 0 and len(ok) == 1, (p.returncode, p.stdout[-2000:])
    res = json.loads(ok[0].split(" ", 1)[1])
    assert [r["rank"] for r in res] == list(range(nranks))
    return res


def test_sharded_hisq_md_is_the_one_rank_hisq_md():
    """2 ranks on 8^4: every rank's slab of the force, the momenta and the links after two MD steps (update_links, hisq_prepare,
    hisq_fforce with three vectors) is the one-rank result bit for bit (asserted by the worker); hisq_fforce_solve stops after the
    same iterations on every rank"""
    res = _launch(2, [8, 8, 8, 8])
    v = res[0]
    print("2 ranks 8^4: solve + force iterations %r (one rank: %r), force deviation from one rank %.3e of max |f|" % (
        v["iters"], v["one_rank_iters"], max(r["solve_force_dev"] for r in res)))
    assert all(r["iters"] == v["iters"] for r in res)
