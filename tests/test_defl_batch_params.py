"""CPU-only tests of the deflated lock-step batch's host layer: the four C-ABI entries and the two kernel hooks in the header, the
ctypes table, the built library and the C++ twin, and the keyword checks that fire before any library call."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("qexhip_dev_solve_xx_batch_deflated", "qexhip_stag_solve_xx_batch_deflated", "qexhip_dev_solve_batch_deflated",
           "qexhip_stag_solve_batch_deflated")
HOOKS = ("qexhip_eig_block_dot_multi", "qexhip_eig_block_axpy_multi")


def test_entries_and_hooks_declared_bound_exported_and_wrapped():
    import qex_amd
    from qex_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "qexhip.h")).read()
    hpp = open(os.path.join(ROOT, "include", "qexhip.hpp")).read()
    bound = {s[0]: s for s in _lib.SYMBOLS}
    L = qex_amd.lib()
    for name in ENTRIES + HOOKS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in bound, name
        assert getattr(L, name) is not None
        decl = re.search(r"^int\s+%s\s*\(([^;]*)\)\s*;" % name, hdr, re.M).group(1)
        decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
        assert len(decl.split(",")) == len(bound[name][2]), name
    for name in HOOKS + ("qexhip_stag_solve_batch_deflated", "qexhip_stag_solve_xx_batch_deflated"):
        assert name in hpp, name


def test_keywords_on_the_methods_and_drivers():
    import qex_amd as q

    for fn in (q.Staggered.solve_batch, q.Staggered.solveXX_batch, q.Context.dev_solve_batch, q.Staggered.solveOO, q.scalarTrace,
               q.localMesonTables):
        p = inspect.signature(fn).parameters
        assert p["deflate"].default is None and p["nev"].default is None, fn
    assert "par_even" in inspect.signature(q.Context.dev_solve_xx_batch_deflated).parameters


def _bare():
    import qex_amd as q

    s = object.__new__(q.Staggered)       # no context, no handle: the checks below must fire before any library call
    s.ctx, s.nlinks = None, 4
    ctx = object.__new__(q.Context)
    B = object.__new__(q.EigBasis)
    B.ctx, B.nvecs, B.id, B.nconv = None, 40, 1, 16
    return q, s, ctx, B


@pytest.mark.parametrize("bad", ["basis", 3, 0.5, True])
def test_deflate_that_is_no_basis_raises_before_any_library_call(bad):
    q, s, ctx, _ = _bare()
    b = np.zeros((16, 3, 2))
    sp = q.SolverParams()
    with pytest.raises(ValueError, match="EigBasis"):
        s.solve_batch([np.zeros_like(b)], [b], [0.1], sp, deflate=bad)
    with pytest.raises(ValueError, match="EigBasis"):
        s.solveXX_batch([np.zeros_like(b)], [b], [0.1], 1e-10, 100, False, deflate=bad)
    with pytest.raises(ValueError, match="EigBasis"):
        s.solveOO(np.zeros_like(b), b, 0.1, sp, deflate=bad)
    with pytest.raises(ValueError, match="EigBasis"):
        ctx.dev_solve_batch([1], [2], [0.1], 1e-10, 100, deflate=bad)
    with pytest.raises(ValueError, match="EigBasis"):
        ctx.dev_solve_xx_batch_deflated(bad, 4, [1], [2], [0.1], 1e-10, 100)
    with pytest.raises(ValueError, match="EigBasis"):
        ctx.dev_solve_batch([1], [2], [0.1], 1e-10, 100, nev=4)          # nev= without deflate=
    assert sp.calls == 0


@pytest.mark.parametrize("bad", [-1, 41, 1.0, "4", True])
def test_nev_out_of_range_raises_before_any_library_call(bad):
    q, s, ctx, B = _bare()
    b = np.zeros((16, 3, 2))
    with pytest.raises(ValueError, match="nev"):
        s.solveXX_batch([np.zeros_like(b)], [b], [0.1], 1e-10, 100, True, deflate=B, nev=bad)
    with pytest.raises(ValueError, match="nev"):
        s.solve_batch([np.zeros_like(b)], [b], [0.1], q.SolverParams(), deflate=B, nev=bad)
    with pytest.raises(ValueError, match="nev"):
        ctx.dev_solve_batch([1], [2], [0.1], 1e-10, 100, deflate=B, nev=bad)
    with pytest.raises(ValueError, match="nev"):
        ctx.dev_solve_xx_batch_deflated(B, bad, [1], [2], [0.1], 1e-10, 100)


def test_more_than_four_systems_raise_before_any_library_call():
    q, s, ctx, B = _bare()
    b = np.zeros((16, 3, 2))
    with pytest.raises(ValueError, match="1..4"):
        s.solveXX_batch([np.zeros_like(b)] * 5, [b] * 5, [0.1] * 5, 1e-10, 100, False, deflate=B)
    with pytest.raises(ValueError, match="1..4"):
        ctx.dev_solve_xx_batch_deflated(B, 16, [1, 2, 3, 4, 5], [6, 7, 8, 9, 10], [0.1] * 5, 1e-10, 100)
    with pytest.raises(ValueError, match="sloppy"):
        ctx.dev_solve_xx_batch_deflated(B, 16, [1], [2], [0.1], 1e-10, 100, sloppy=3)
