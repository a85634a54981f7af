"""Rooted HISQ, the part that needs no GPU: the three rational entries exist in every ABI layer, qex_amd.rational fits what the
example needs, tests/rational_ref.py (the yardstick of tests/test_gpu_rational.py) satisfies the algebra it is built on, and
examples/hisq_rhmc.py parses its options and fails loudly where there is no device."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import rational_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["qexhip_dev_rational_xx", "qexhip_stag_rational_xx", "qexhip_md_hisq_fforce_rational"]
EXAMPLE = os.path.join(ROOT, "examples", "hisq_rhmc.py")
LAT, SEED, MASS = [4, 4, 4, 6], 987654321, 0.3
FIT_LO, FIT_HI, FIT_NTERM = 0.01, 8.0, 12


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
    for name in ENTRIES:
        args = re.search(r"\bint %s\s*\((.*?)\);" % name, hdr, flags=re.S).group(1)
        assert len(bound[name][2]) == len(args.split(",")), name
        nargs = re.search(r"proc %s\((.*?)\): cint" % name, nim, flags=re.S).group(1)
        # nim groups parameters of one type: a, b: T -- count the names
        nnames = sum(len(grp.split(":")[0].split(",")) for grp in nargs.split(";"))
        assert nnames == len(args.split(",")), name
    assert callable(qex_amd.Context.dev_rational_xx) and callable(qex_amd.Staggered.rationalXX)
    assert callable(qex_amd.ResidentMD.hisq_fforce_rational)


@pytest.mark.parametrize("power", [-0.25, 0.125, -0.5])
def test_rational_fit(power):
    """12 poles on [0.01, 8]: below 1e-6 (a CPU prototype of this fit gave 4.1e-8, 2.5e-8 and 9.3e-8), the reported error is the
    error, the residues have the sign that keeps r(M^+M) definite, JSON round-trips exactly.
    Observed: 4.15e-08 (x^-1/4), 4.09e-08 (x^+1/8), 1.32e-07 (x^-1/2)."""
    from qex_amd.rational import Rational, grid, max_rel_error, rationalFit

    rat, err = rationalFit(power, FIT_LO, FIT_HI, FIT_NTERM)
    print("x^%g: %d poles, max relative error %.3e, f0 %r, poles %.3e .. %.3e" % (power, rat.nterm, err, rat.f0, rat.beta.min(), rat.beta.max()))
    assert rat.nterm == FIT_NTERM and err < 1e-6
    x = grid(FIT_LO, FIT_HI)
    assert x.size == 4001 and x[0] == FIT_LO and abs(x[-1] - FIT_HI) < 1e-14
    direct = np.abs((rat.f0 + sum(a / (x + b) for a, b in zip(rat.alpha, rat.beta))) / x ** power - 1.0).max()
    assert abs(direct - err) <= 1e-12 and max_rel_error(rat, power, FIT_LO, FIT_HI) == err
    assert np.all(rat.alpha > 0) if power < 0 else np.all(rat.alpha < 0)
    assert np.all(rat.beta > 0) and np.all(np.diff(rat.beta) > 0)
    back = Rational.from_json(rat.to_json())
    assert back.f0 == rat.f0 and np.array_equal(back.alpha, rat.alpha) and np.array_equal(back.beta, rat.beta)
    with pytest.raises(ValueError):
        Rational(1.0, [1.0, 2.0], [0.5])


@functools.lru_cache(maxsize=None)
def hisq_case():
    from oracle import oracle as o

    o.build()
    lo = o.Layout(LAT)
    rf = o.RngField(lo, o.RNG_MILC6, SEED)
    g = o.gauge_warm(lo, 0.3, rf)
    o.rephase(lo, g)
    fat, lng = o.hisq_smear(lo, g)
    b = o.vector_gaussian(lo, rf)
    return o, lo, fat, lng, b


def test_reference_one_pole_is_the_inverse():
    """f0 = 0, alpha = [1], beta = [0]: r(M^+M) b = (A/4)^-1 b = 4 x the oracle's solveXX solution.  The oracle stops at
    |r|^2 <= 1e-24 |b|^2, so its solution is within 1e-12 |b| / lambda_min(A) of exact: 1e-12 / (4 m^2) relative to |b|.
    Observed: 1.6e-12 relative to the solution."""
    o, lo, fat, lng, b = hisq_case()
    h = lo.vol // 2
    for par_even in (True, False):
        sl = slice(0, h) if par_even else slice(h, 2 * h)
        x = o.solveXX(lo, fat, lng, b, MASS, 1e-24, 5000, par_even)[0]
        ref = RR.rational_ref(o, lo, fat, lng, b, MASS, 0.0, [1.0], [0.0], par_even)
        other = slice(h, 2 * h) if par_even else slice(0, h)
        assert not ref[other].any()
        dev = np.linalg.norm(ref[sl] - 4.0 * x[sl])
        print("parity %s: |ref - 4 x| / |ref| = %.2e" % ("even" if par_even else "odd", dev / np.linalg.norm(ref[sl])))
        assert dev <= 4.0 * 1e-12 * np.linalg.norm(b[sl]) / (4.0 * MASS * MASS)


def test_reference_inverse_square_root_twice_is_the_inverse():
    """r ~ x^(-1/2) with 12 poles on [m^2, m^2 + 6], which holds the spectrum of M^+M here (largest eigenvalue 5.5): r(r(b)) against
    (M^+M)^-1 b.  r^2 x = (1 + e)^2 with |e| <= err per eigencomponent, and the components of the inverse are spread over hi / lo in
    size: bound err * hi / lo relative to the inverse.  Observed: 4.3e-09 against a bound of 8.2e-07 (fit error 1.2e-08, hi / lo 67.7)."""
    from qex_amd.rational import rationalFit

    o, lo, fat, lng, b = hisq_case()
    h = lo.vol // 2
    flo, fhi = MASS * MASS, MASS * MASS + 6.0
    rat, err = rationalFit(-0.5, flo, fhi, 12)
    once = RR.rational_ref(o, lo, fat, lng, b, MASS, rat.f0, rat.alpha, rat.beta, True)
    once.setflags(write=False)
    twice = RR.rational_ref(o, lo, fat, lng, once, MASS, rat.f0, rat.alpha, rat.beta, True)
    inv = RR.rational_ref(o, lo, fat, lng, b, MASS, 0.0, [1.0], [0.0], True)
    dev = np.linalg.norm(twice[:h] - inv[:h]) / np.linalg.norm(inv[:h])
    print("r(r(b)) against the inverse: %.2e (fit error %.2e, hi / lo %.1f, bound %.2e)" % (dev, err, fhi / flo, err * fhi / flo))
    assert dev <= err * fhi / flo
    assert dev > 1e-12                      # it is a rational approximation, not the inverse handed back


def test_reference_force_vectors_solve_the_full_system():
    """psi_k of rational_ref.force_vectors is D(m_k)^-1 phi with phi.odd = 0: D(m_k) psi_k = phi at 1e-12"""
    o, lo, fat, lng, b = hisq_case()
    h = lo.vol // 2
    phi = b.copy()
    phi[h:] = 0
    phi.setflags(write=False)
    alpha, beta = [0.3, 0.9], [0.02, 0.9]
    for (psi, w), a, be in zip(RR.force_vectors(o, lo, fat, lng, phi, MASS, alpha, beta), alpha, beta):
        mk = np.sqrt(MASS * MASS + be)
        assert abs(w - a / mk) < 1e-15
        dev = np.linalg.norm(o.D(lo, fat, lng, psi, mk) - phi) / np.linalg.norm(phi)
        print("beta %g: |D(m_k) psi_k - phi| / |phi| = %.2e" % (be, dev))
        assert dev < 1e-12


def test_example_prints_its_options():
    p = subprocess.run([sys.executable, EXAMPLE, "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    for opt in ("-nf", "-nterm", "-fterm", "-lo", "-hi", "-rational", "-lat", "-beta", "-mass", "-tau", "-gsteps", "-fsteps", "-trajs",
                "-seed", "-warm"):
        assert opt in p.stdout, opt


def test_example_fails_loudly_without_a_device():
    """no GPU (hidden from the runtime here, so the test holds on a GPU machine too): a non-zero exit and the library's error, not a
    trajectory computed some other way"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, EXAMPLE, "-lat", "4", "4", "4", "4", "-nterm", "6", "-fterm", "4"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=120, env=env)
    assert p.returncode != 0
    assert "QexHipError" in p.stderr and "MEASplaq" not in p.stdout and "kinetic" not in p.stdout, (p.stdout, p.stderr)
