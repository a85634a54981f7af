"""The sharded-lattice tests' one launcher and one rank prologue.

Launcher half (pytest side): launch / launch_ok start a script under torch.distributed.run, one fresh process per rank, and hold it to a
time limit that the ranks do not outlive.  The agent starts every rank in a session of its own, so no signal sent to the agent or to its
process group reaches them: at the limit the agent gets SIGTERM, which it answers by shutting its ranks down, and SIGKILL only GRACE
seconds later.

Worker half (rank scripts): shard turns the process into one rank of a t-sharded context, finish prints the gathered `TAG [json per
rank]` line that launch_ok reads.

Neither torch nor qex_amd is imported before a worker asks for its context.
"""
import json
import os
import socket
import subprocess
import sys
from typing import NamedTuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRACE = 10          # seconds between SIGTERM and SIGKILL for an agent past its limit


def free_port():
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def launch(nranks, argv, limit, env=None):
    """`argv` (script and arguments) on `nranks` ranks from the repository root, at most `limit` seconds: the CompletedProcess"""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0",      # (a GPU box leases 16 cores whatever cpu_count() says)
               OMP_NUM_THREADS=str(max(1, min(16, len(os.sched_getaffinity(0))) // nranks)), **(env or {}))
    cmd = ["timeout", "-k", str(GRACE), str(limit), sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nranks),
           "--master-addr", "127.0.0.1", "--master-port", str(free_port())] + [str(a) for a in argv]
    # (the limit of run() is the backstop for ranks that outlive a killed agent and keep its pipes open)
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=limit + 3 * GRACE, cwd=ROOT, env=env)
    if p.returncode in (124, 128 + 9):                           # timeout's own status: the limit, the limit and then SIGKILL
        print(p.stdout[-3000:])
        print(p.stderr[-6000:])
        raise AssertionError("%d ranks of %s: status %d, the time limit of %d s" % (nranks, argv[0], p.returncode, limit))
    return p


def launch_ok(nranks, worker, args, tag, limit, env=None):
    """tests/`worker` on `nranks` ranks must exit 0 and print one line `TAG [json per rank]`: the records, which are in rank order"""
    p = launch(nranks, [os.path.join(ROOT, "tests", worker)] + list(args), limit, env)
    ok = [ln for ln in p.stdout.splitlines() if ln.startswith(tag + " ")]
    good = p.returncode == 0 and len(ok) == 1
    print("\n".join(ln for ln in p.stderr.splitlines() if ln.startswith("rank ")) if good else p.stderr[-6000:])
    assert good, (p.returncode, p.stdout[-2000:])
    res = json.loads(ok[0].split(" ", 1)[1])
    assert [r["rank"] for r in res] == list(range(nranks))
    return res


class Shard(NamedTuple):
    rank: int
    world: int
    dist: object        # torch.distributed, gloo group up: the control plane only (unique id, gathers, barriers)
    ctx: object         # qex_amd.Context of this rank's t-slab, communicator up
    loc: object         # qex_amd.Layout of the slab
    idx: object         # global indices of the slab's sites, in the slab's order
    sl: object          # sl(a): this rank's slab of a global field, contiguous


def shard(glat, device=0, peer=True, comm=True):
    """This process as rank RANK of WORLD_SIZE of the lattice `glat` split along t (rank_geom 1.1.1.N).  peer: the ranks share a device,
    so the communicator must have taken the peer-memory transport.  comm = False leaves the context without a communicator."""
    import numpy as np

    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import qex_amd as q

    loc, idx = q.Layout(list(glat)).shard_indices(world, rank)
    ctx = q.Context(loc.lat, device=device, rank_geom=(1, 1, 1, world), rank_coord=(0, 0, 0, rank))
    if comm:
        uid = [q.Context.unique_id() if rank == 0 else None]
        dist.broadcast_object_list(uid, src=0)
        ctx.comm_init(uid[0], world, rank)
        assert not peer or ctx.comm_transport()[0] == "peer"
    return Shard(rank, world, dist, ctx, loc, idx, lambda a: np.ascontiguousarray(a[idx]))


def gather(w, obj):
    """`obj` of every rank, in rank order, on every rank"""
    out = [None] * w.world
    w.dist.all_gather_object(out, obj)
    return out


def finish(w, tag, res):
    """Rank 0 prints `tag [res of every rank]` (one line: the ranks' stdout interleaves); nobody leaves before it is out"""
    allres = gather(w, res)
    if w.rank == 0:
        print("%s %s" % (tag, json.dumps(allres)), flush=True)
    w.dist.barrier()
