"""The stochastic scalar trace on t-sharded lattices: dilution by GLOBAL time, the cfield of a slab, the rank-global slice table and
the scalarTrace driver.

The ranks are started by torch.distributed.run as fresh processes that all bind GPU 0 and talk over the peer-memory transport;
tests/scalar_trace_rank_worker.py checks every rank's slab against a one-rank context of the whole lattice, bit for bit.

Sharding in t needs X*Y*Z/2 to be a multiple of 64 and an even local t extent (geom_init), so 4.4.4.8 and 4.6.10.6 cannot be split:
beside 8^4 the second lattice is 8.8.6.8, whose 192-site slices of one parity end in a partial 256-site chunk, and the driver runs
end to end on it.  Observed values are printed (pytest -s)."""
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


def _launch(nranks, lat, extra=(), timeout=300):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", QEXHIP_PEER_TIMEOUT="60",
               OMP_NUM_THREADS=str(max(1, min(16, len(os.sched_getaffinity(0))) // nranks)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nranks), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "scalar_trace_rank_worker.py")] + [str(v) for v in lat] + list(extra)
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, cwd=ROOT, env=env)
    ok = [ln for ln in p.stdout.splitlines() if ln.startswith("SCALAR_TRACE_RANKS_OK ")]
    print(p.stderr[-6000:] if (p.returncode != 0 or len(ok) != 1) else "\n".join(ln for ln in p.stderr.splitlines() if ln.startswith("rank ")))
    assert p.returncode == 0 and len(ok) == 1, (p.returncode, p.stdout[-2000:])
    res = json.loads(ok[0].split(" ", 1)[1])
    assert [r["rank"] for r in res] == list(range(nranks))
    return res


@pytest.mark.parametrize("lat,extra", [([8, 8, 8, 8], ()), ([8, 8, 6, 8], ("e2e",))])
def test_sharded_scalar_trace_is_the_one_rank_scalar_trace(lat, extra):
    """dilute, accumulate and the slice table on identical uploaded global fields: every rank's slab and the whole table equal the
    one-rank result bit for bit; with e2e, scalarTrace (fp64) gives the one-rank est[t] and trace to 1e-9 of max|trace|"""
    res = _launch(2, lat, extra)
    for r in res:
        assert r["dilute"] == r["accum"] == r["slices"] == "equal"
        if extra:
            print("2 ranks %s rank %d: %s" % (lat, r["rank"], r["e2e"]))
            assert r["e2e"]["est_dev"] < 1e-9 and r["e2e"]["trace_dev"] < 1e-9
