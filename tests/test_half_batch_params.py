"""CPU-only tests of the 16-bit lock-step batch's host layer: the two new C-ABI entries in the header, the C++ mirror, the ctypes
table and the built library with matching argument counts, the new source file in the Makefile, the two Context methods, and the
examples' -half switch."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("qexhip_dev_op_xx_half_batch", "qexhip_stag_sloppy_last_batch")


def test_half_batch_entries_declared_bound_and_exported():
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
        assert name in hpp, name
        # argument counts of the ctypes table = those of the header's declarations
        decl = re.search(r"^int\s+%s\s*\(([^;]*)\)\s*;" % name, hdr, re.M).group(1)
        assert len(decl.split(",")) == len(bound[name][2]), name
    assert '"half_batch"' in hdr


def test_entries_refuse_a_null_handle():
    import qex_amd

    L = qex_amd.lib()
    assert L.qexhip_dev_op_xx_half_batch(None, 1, None, None, None, 1) == -1
    assert L.qexhip_stag_sloppy_last_batch(None, 4, None, None, None, None, None) == -1


def test_source_and_header_in_the_makefile():
    mk = open(os.path.join(ROOT, "qex_amd", "Makefile")).read()
    src = re.search(r"^SRC_HIP\s*=(.*)$", mk, re.M).group(1).split()
    hdr = re.search(r"^HDR\s*=(.*)$", mk, re.M).group(1).split()
    assert "csrc/batch_half.hip" in src
    assert "csrc/dslash_half_core.h" in hdr
    for f in ("batch_half.hip", "dslash_half_core.h"):
        assert os.path.exists(os.path.join(ROOT, "qex_amd", "csrc", f))


def test_context_methods_exist():
    import inspect

    import qex_amd as q

    assert list(inspect.signature(q.Context.sloppy_last_batch).parameters) == ["self"]
    p = inspect.signature(q.Context.dev_op_xx_half_batch).parameters
    assert list(p) == ["self", "r_ids", "x_ids", "m2s", "par_even"] and p["par_even"].default is True
    # no new keywords on the batch methods
    for fn in (q.Staggered.solve_batch, q.Staggered.solveXX_batch, q.Context.dev_solve_batch):
        assert not [k for k in inspect.signature(fn).parameters if "half" in k], fn


def test_examples_accept_half():
    for ex in ("scalar_trace.py", "stag_mesons.py"):
        path = os.path.join(ROOT, "examples", ex)
        src = open(path).read()
        m = re.search(r'add_argument\("-half",([^\n]*)\)', src)
        assert m and "default=0" in m.group(1) and "choices=[0, 1]" in m.group(1), ex
        assert 'set_option("half", 1)' in src and 'set_option("half_batch", 1)' in src, ex
        # the parser itself: -half 2 is refused before anything is set up (argparse exits with status 2)
        r = subprocess.run([sys.executable, path, "-half", "2"], capture_output=True, text=True)
        assert r.returncode == 2 and "-half" in r.stderr, (ex, r.returncode, r.stderr[-300:])
