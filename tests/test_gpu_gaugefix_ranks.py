"""Gauge fixing on t-sharded lattices: the ghost slices of the links, the t-faces of the transform field (Landau gauge), the
rank-global metrics and the agreement of the ranks on the loop control.

The ranks are started by torch.distributed.run as fresh processes that all bind GPU 0 and talk over the peer-memory transport;
tests/gaugefix_rank_worker.py checks every rank's slab against a one-rank context of the whole lattice.  Observed values are
printed (pytest -s)."""
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
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "gaugefix_rank_worker.py")] + [str(v) for v in lat]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, cwd=ROOT, env=env)
    ok = [ln for ln in p.stdout.splitlines() if ln.startswith("GAUGEFIX_RANKS_OK ")]
    print(p.stderr[-6000:] if (p.returncode != 0 or len(ok) != 1) else "\n".join(ln for ln in p.stderr.splitlines() if ln.startswith("rank ")))
    assert p.returncode == 0 and len(ok) == 1, (p.returncode, p.stdout[-2000:])
    res = json.loads(ok[0].split(" ", 1)[1])
    assert [r["rank"] for r in res] == list(range(nranks))
    return res


@pytest.mark.parametrize("nranks,lat", [(2, [8, 8, 8, 8]), (4, [8, 8, 8, 16])])
def test_sharded_gauge_fixing_is_the_one_rank_gauge_fixing(nranks, lat):
    """Coulomb and Landau: the slab of t after 40 relax iterations is the one-rank t bit for bit; the full fix converges with the
    same iterations on every rank, the gathered t has gdsq <= gstop and is in SU(3); plaquettes after the transform agree to 1e-13."""
    res = _launch(nranks, lat)
    for name in ("coulomb", "landau"):
        v = res[0][name]
        print("%d ranks %s %s: %d iterations (one rank: %d), gdsq %.3e (numpy %.3e)" %
              (nranks, lat, name, v["iters"], v["one_rank_iters"], v["gdsq"], v["numpy_gdsq"]))
        assert all(r[name]["iters"] == v["iters"] for r in res)
