"""Resident HISQ molecular dynamics, the part that needs no GPU: the four entries qexhip_md_hisq_* exist in every ABI layer, and
examples/hisqhmc.py parses its options and fails loudly where there is no device."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["qexhip_md_hisq_prepare", "qexhip_md_hisq_fforce", "qexhip_md_hisq_fforce_solve", "qexhip_md_hisq_force_get"]
EXAMPLE = os.path.join(ROOT, "examples", "hisqhmc.py")


def test_entries_are_declared_bound_exported_and_mirrored():
    import qex_amd
    from qex_amd import _lib

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qexhip.h")).read(), flags=re.S)
    hpp = open(os.path.join(ROOT, "include", "qexhip.hpp")).read()
    nim = open(os.path.join(ROOT, "qex_amd", "nim", "qexhip.nim")).read()
    bound = {s[0]: s for s in _lib.SYMBOLS}
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    L = qex_amd.lib()
    for name in ENTRIES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name + " is not declared in include/qexhip.h"
        assert name in bound and hasattr(L, name), name + " is not bound in qex_amd/_lib.py"
        assert re.search(r" T %s$" % name, exported, flags=re.M), name + " is not exported by libqexhip.so"
        assert name + "(" in hpp, name + " is not mirrored in include/qexhip.hpp"
        assert "proc %s(" % name in nim, name + " is not mirrored in qex_amd/nim/qexhip.nim"
    # the argument counts of the bindings are those of the declarations
    for name in ENTRIES:
        args = re.search(r"\bint %s\s*\((.*?)\);" % name, hdr, flags=re.S).group(1)
        assert len(bound[name][2]) == len(args.split(",")), name
    for m in ("hisq_prepare", "hisq_fforce", "hisq_fforce_solve", "hisq_force"):
        assert callable(getattr(qex_amd.ResidentMD, m))


def test_example_prints_its_options():
    p = subprocess.run([sys.executable, EXAMPLE, "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    for opt in ("-lat", "-beta", "-mass", "-tau", "-gsteps", "-fsteps", "-trajs", "-seed", "-warm", "-host"):
        assert opt in p.stdout, opt


def test_example_fails_loudly_without_a_device():
    """no GPU (hidden from the runtime here, so the test holds on a GPU machine too): a non-zero exit and the library's error,
    not a trajectory computed some other way"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    for extra in ([], ["-host"]):
        p = subprocess.run([sys.executable, EXAMPLE, "-lat", "4", "4", "4", "4"] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True, timeout=120, env=env)
        assert p.returncode != 0
        assert "QexHipError" in p.stderr and "MEASplaq" not in p.stdout and "kinetic" not in p.stdout, (p.stdout, p.stderr)
