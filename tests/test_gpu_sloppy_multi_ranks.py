"""Mixed-precision multi-shift CG on a t-sharded lattice: two ranks, started by torch.distributed.run as fresh processes that both
bind GPU 0 and talk over the peer-memory transport (tests/sloppy_multi_rank_worker.py holds the checks: the same iterations, updates,
refinement iterations and residuals on every rank; the gathered solutions' true residuals against the oracle).  Observed values are
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


def _launch(nranks, script_args, timeout=600):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", QEXHIP_PEER_TIMEOUT="60",
               OMP_NUM_THREADS=str(max(1, min(16, len(os.sched_getaffinity(0))) // nranks)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nranks), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "sloppy_multi_rank_worker.py")] + script_args
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, cwd=ROOT, env=env)
    ok = [ln for ln in p.stdout.splitlines() if ln.startswith("SLOPPY_MULTI_RANKS_OK ")]
    print(p.stderr[-6000:] if (p.returncode != 0 or len(ok) != 1) else "\n".join(ln for ln in p.stderr.splitlines() if ln.startswith("rank ")))
    assert p.returncode == 0 and len(ok) == 1, (p.returncode, p.stdout[-2000:])
    res = json.loads(ok[0].split(" ", 1)[1])
    assert [r["rank"] for r in res] == list(range(nranks))
    return res


def test_two_ranks_multi_shift_sloppy():
    """2 ranks on 8^4, g.random plain and with Naik links, 4 shifts at r2req 1e-14, both parities"""
    res = _launch(2, ["8", "8", "8", "8"])
    keys = [k for k in res[0] if k != "rank"]
    assert sorted(keys) == ["random/even", "random/odd", "random_naik/even", "random_naik/odd"]
    for key in keys:
        v = res[0][key]
        print(f"2 ranks 8^4 {key}: {v['its']} its / {v['nupd']} updates, refine {v['refine']}, true r2/b2 {v['oracle_r2']}")
        assert all(r[key]["its"] == v["its"] and r[key]["nupd"] == v["nupd"] and r[key]["refine"] == v["refine"] and r[key]["r2"] == v["r2"]
                   for r in res)
        assert all(x <= 1e-14 * (1.0 + 1e-4) for x in v["oracle_r2"])
