"""The -batch_ranks parameter of the three measurement examples (no GPU: both exits happen before a context exists): a value outside
{0, 1} exits from argparse, and without the flag a sloppy run on more than one rank keeps its early exit and its text."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLES = ["scalar_trace.py", "stag_mesons.py", "conn4d.py"]


def _run(example, args, world):
    env = dict(os.environ, WORLD_SIZE=str(world), RANK="0")
    return subprocess.run([sys.executable, os.path.join(ROOT, "examples", example)] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=120, cwd=ROOT, env=env)


@pytest.mark.parametrize("example", EXAMPLES)
def test_batch_ranks_outside_0_1_exits_from_argparse(example):
    for world in (1, 2):
        p = _run(example, ["-sloppy", "1", "-batch_ranks", "2"], world)
        assert p.returncode == 2 and "-batch_ranks" in p.stderr and "invalid choice" in p.stderr, (p.returncode, p.stderr[-500:])


@pytest.mark.parametrize("example", EXAMPLES)
def test_early_exit_without_the_flag_is_unchanged(example):
    for args in (["-sloppy", "1"], ["-sloppy", "1", "-batch_ranks", "0"]):
        p = _run(example, args, 2)
        assert p.returncode == 1 and p.stdout == "", (p.returncode, p.stdout[-300:])
        want = ("%s: -sloppy 1 needs a single rank: the mixed-precision lock-step batch is not built for t-sharded lattices" % example)
        assert p.stderr.startswith(want), p.stderr[-500:]
