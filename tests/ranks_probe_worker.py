"""Worker of tests/test_ranks_harness.py: a rank that touches no GPU and imports no qex_amd.

  ok          gloo group, then ranks.finish: one line `PROBE_RANKS_OK [{"rank": r} per rank]`
  fail        rank 0 prints that line complete by itself, rank 1 exits with status 3
  sleep DIR   writes its pid to DIR/<rank> and sleeps ten minutes
"""
import json
import os
import sys
import time

import ranks

rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
mode = sys.argv[1]
if mode == "ok":
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    ranks.finish(ranks.Shard(rank, world, dist, None, None, None, None), "PROBE_RANKS_OK", {"rank": rank})
elif mode == "fail":
    if rank == 0:
        print("PROBE_RANKS_OK %s" % json.dumps([{"rank": r} for r in range(world)]), flush=True)
    sys.exit(3 * rank)
else:
    with open(os.path.join(sys.argv[2], str(rank)), "w") as f:
        f.write(str(os.getpid()))
    time.sleep(600)
