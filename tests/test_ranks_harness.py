"""tests/ranks.py on ranks that touch no GPU (tests/ranks_probe_worker.py): what launch_ok returns, what it refuses, and that a
launch past its time limit leaves no rank behind."""
import os
import time

import pytest

import ranks

LIMIT = 8          # seconds: the agent has started its two ranks, and they have written their pids, well within it


def test_two_records_come_back_in_rank_order():
    res = ranks.launch_ok(2, "ranks_probe_worker.py", ["ok"], "PROBE_RANKS_OK", 120)
    assert res == [{"rank": 0}, {"rank": 1}]


def test_a_rank_that_exits_nonzero_fails_the_launch():
    with pytest.raises(AssertionError):
        ranks.launch_ok(2, "ranks_probe_worker.py", ["fail"], "PROBE_RANKS_OK", 120)


def test_the_time_limit_ends_the_ranks_with_the_launch(tmp_path):
    """The agent gets SIGTERM at the limit and takes its ranks, which run in sessions of their own, down with it: the launch fails
    within limit + grace + a few seconds, and no recorded pid is alive afterwards."""
    t0 = time.time()
    with pytest.raises(AssertionError, match="limit"):
        ranks.launch(2, [os.path.join(ranks.ROOT, "tests", "ranks_probe_worker.py"), "sleep", str(tmp_path)], LIMIT)
    assert time.time() - t0 < LIMIT + ranks.GRACE + 5
    pids = [int((tmp_path / str(r)).read_text()) for r in range(2)]
    assert len(set(pids)) == 2
    for pid in pids:
        with pytest.raises(ProcessLookupError):
            os.kill(pid, 0)
