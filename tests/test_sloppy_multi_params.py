"""CPU-only tests of the mixed-precision multi-shift solve's host layer: the three C-ABI entries in the header, the ctypes table and
the built library, the explicit `sloppy` keyword of the three Python methods, and the checks that fire before any library call."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("qexhip_stag_solve_xx_multi_sloppy", "qexhip_dev_solve_xx_multi_sloppy", "qexhip_stag_solve_multi_sloppy")


def test_multi_sloppy_entries_declared_bound_and_exported():
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
    assert len(bound["qexhip_stag_solve_xx_multi_sloppy"][2]) == 13 and len(bound["qexhip_stag_solve_multi_sloppy"][2]) == 11
    assert "qexhip_stag_solve_xx_multi_sloppy" in hpp and "qexhip_stag_solve_multi_sloppy" in hpp
    mk = open(os.path.join(ROOT, "qex_amd", "Makefile")).read()
    assert "csrc/multishift_f32.hip" in mk


def test_sloppy_keyword_on_the_three_methods():
    import qex_amd as q

    for fn in (q.Staggered.solveXX_multi, q.Context.dev_solve_xx_multi, q.Staggered.solve):
        p = inspect.signature(fn).parameters
        assert "sloppy" in p and p["sloppy"].default is None, fn
    sp = q.SolverParams()
    assert sp.refineIterations == []
    sp.refineIterations = [0, 3]
    sp.resetStats()
    assert sp.refineIterations == []


def _bare_staggered():
    import qex_amd as q

    s = object.__new__(q.Staggered)       # no context: the checks below must fire before any library call
    s.ctx, s.nlinks = None, 4
    return s


@pytest.mark.parametrize("bad", [3, -1, 1.0, "1", True])
def test_bad_sloppy_raises_before_any_library_call(bad):
    import qex_amd as q

    s = _bare_staggered()
    b = np.zeros((16, 3, 2))
    sp = q.SolverParams()
    with pytest.raises(ValueError):
        s.solveXX_multi([np.zeros_like(b)], b, [0.1], sp, sloppy=bad)
    with pytest.raises(ValueError):
        s.solve([np.zeros_like(b), np.zeros_like(b)], b, [0.1, 0.2], sp, sloppy=bad)
    ctx = object.__new__(q.Context)       # no handle: a library call would fail on the missing attribute, not with ValueError
    with pytest.raises(ValueError):
        ctx.dev_solve_xx_multi([1], 2, [0.1], 1e-10, 100, sloppy=bad)
    assert sp.calls == 0 and sp.iterations == 0 and sp.reliableUpdates == 0 and sp.refineIterations == []


def test_history_is_refused_with_the_keyword():
    import qex_amd as q

    s = _bare_staggered()
    b = np.zeros((16, 3, 2))
    with pytest.raises(ValueError, match="history"):
        s.solveXX_multi([np.zeros_like(b)], b, [0.1], q.SolverParams(), histcap=8, sloppy=1)
    ctx = object.__new__(q.Context)
    with pytest.raises(ValueError, match="history"):
        ctx.dev_solve_xx_multi([1], 2, [0.1], 1e-10, 100, histcap=8, sloppy=1)


def test_sloppy_params_without_the_keyword_still_refused_and_names_it():
    import qex_amd as q

    s = _bare_staggered()
    b = np.zeros((16, 3, 2))
    for sl in (q.SloppySingle, q.SloppyHalf):
        sp = q.SolverParams(sloppySolve=sl)
        with pytest.raises(ValueError, match="sloppy="):
            s.solve([np.zeros_like(b), np.zeros_like(b)], b, [0.1, 0.2], sp)
        with pytest.raises(ValueError, match="sloppy="):
            s.solveXX_multi([np.zeros_like(b)], b, [0.1], sp)
        with pytest.raises(ValueError, match="sloppy="):
            s.solveXX_multi([np.zeros_like(b)], b, [0.1], sp, sloppy=None)
