"""CPU-only tests of the mixed-precision solve's host layer: SolverParams.sloppySolve and its constants (solverBase.nim:8-15),
the C-ABI entries in the ctypes table and header, and the out-of-scope forms rejected before anything reaches a GPU."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("qexhip_stag_solve_xx_sloppy", "qexhip_stag_solve_sloppy", "qexhip_dev_solve_xx_sloppy", "qexhip_dev_op_xx_sloppy",
           "qexhip_stag_links_info_f32")


def test_solver_params_sloppy_default_and_constants():
    import qex_amd as q

    assert (q.SloppyNone, q.SloppySingle, q.SloppyHalf) == (0, 1, 2)
    sp = q.SolverParams()
    assert sp.sloppySolve == q.SloppyNone and sp.reliableUpdates == 0
    sp = q.SolverParams(r2req=1e-10, sloppySolve=q.SloppyHalf)
    assert sp.sloppySolve == 2
    sp.reliableUpdates = 5
    sp.resetStats()
    assert sp.reliableUpdates == 0 and sp.sloppySolve == 2


def test_sloppy_entries_declared_bound_and_exported():
    import qex_amd
    from qex_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "qexhip.h")).read()
    bound = {s[0] for s in _lib.SYMBOLS}
    L = qex_amd.lib()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in bound, name
        assert getattr(L, name) is not None
    hpp = open(os.path.join(ROOT, "include", "qexhip.hpp")).read()
    assert "sloppySolve" in hpp


def _bare_staggered():
    import qex_amd as q

    s = object.__new__(q.Staggered)       # no context: the checks below must fire before any library call
    s.ctx, s.nlinks = None, 4
    return s


def test_sloppy_mass_list_and_batch_rejected():
    import qex_amd as q

    s = _bare_staggered()
    b = np.zeros((16, 3, 2))
    sp = q.SolverParams(sloppySolve=q.SloppySingle)
    with pytest.raises(ValueError):
        s.solve([np.zeros_like(b), np.zeros_like(b)], b, [0.1, 0.2], sp)
    with pytest.raises(ValueError):
        s.solveXX_multi([np.zeros_like(b)], b, [0.1], sp)
    with pytest.raises(ValueError):
        s.solve_batch([np.zeros_like(b)], [b], [0.1], sp)
