"""CPU-only tests of the mixed-precision lock-step batch's host layer: the three C-ABI entries in the header, the ctypes table and
the built library, the explicit `sloppy` keyword of the batched Python methods, and the checks that fire before any library call."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("qexhip_stag_solve_xx_batch_sloppy", "qexhip_stag_solve_batch_sloppy", "qexhip_dev_solve_batch_sloppy")


def test_batch_sloppy_entries_declared_bound_and_exported():
    import qex_amd
    from qex_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "qexhip.h")).read()
    hpp = open(os.path.join(ROOT, "include", "qexhip.hpp")).read()
    bound = {s[0]: s for s in _lib.SYMBOLS}
    L = qex_amd.lib()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in bound, name
        assert getattr(L, name) is not None
    # argument counts of the ctypes table = those of the header's declarations
    for name in ENTRIES:
        decl = re.search(r"^int\s+%s\s*\(([^;]*)\)\s*;" % name, hdr, re.M).group(1)
        assert len(decl.split(",")) == len(bound[name][2]), name
    assert "qexhip_stag_solve_batch_sloppy" in hpp
    mk = open(os.path.join(ROOT, "qex_amd", "Makefile")).read()
    assert "csrc/batch_f32.hip" in mk


def test_sloppy_keyword_on_the_three_methods():
    import qex_amd as q

    for fn in (q.Staggered.solve_batch, q.Staggered.solveXX_batch, q.Context.dev_solve_batch):
        p = inspect.signature(fn).parameters
        assert "sloppy" in p and p["sloppy"].default is None, fn
    from qex_amd import mesons

    p = inspect.signature(mesons.localMesonTables).parameters
    assert p["sloppy"].default == 0


def _bare_staggered():
    import qex_amd as q

    s = object.__new__(q.Staggered)       # no context: the checks below must fire before any library call
    s.ctx, s.nlinks = None, 4
    return s


def test_sloppy_none_keeps_the_refusal_and_names_the_keyword():
    import qex_amd as q

    s = _bare_staggered()
    b = np.zeros((16, 3, 2))
    for sl in (q.SloppySingle, q.SloppyHalf):
        sp = q.SolverParams(sloppySolve=sl)
        with pytest.raises(ValueError, match="sloppy="):
            s.solve_batch([np.zeros_like(b)], [b], [0.1], sp)
        with pytest.raises(ValueError, match="sloppy="):
            s.solve_batch([np.zeros_like(b)], [b], [0.1], sp, sloppy=None)
        with pytest.raises(ValueError):
            s.solve_batch([np.zeros_like(b)] * 2, [b] * 2, [0.1, 0.2], [q.SolverParams(), sp])


@pytest.mark.parametrize("bad", [3, -1, 7, 1.0, "1", True])
def test_bad_sloppy_raises_before_any_library_call(bad):
    import qex_amd as q

    s = _bare_staggered()
    b = np.zeros((16, 3, 2))
    sp = q.SolverParams()
    with pytest.raises(ValueError):
        s.solve_batch([np.zeros_like(b)], [b], [0.1], sp, sloppy=bad)
    with pytest.raises(ValueError):
        s.solveXX_batch([np.zeros_like(b)], [b], [0.1], 1e-10, 100, True, sloppy=bad)
    ctx = object.__new__(q.Context)       # no handle: a library call would fail on the missing attribute, not with ValueError
    with pytest.raises(ValueError):
        ctx.dev_solve_batch([1], [2], [0.1], 1e-10, 100, sloppy=bad)
    assert sp.calls == 0 and sp.reliableUpdates == 0
