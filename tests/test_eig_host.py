"""Host side of the low-mode eigensolver (no GPU): the dense symmetric eigensolver the thick-restart Lanczos calls at every restart
(qexhip_symeig_host, qex_amd/csrc/symeig_host.cpp), the same file under AddressSanitizer + UBSan as a stand-alone program, and the
option checks of Staggered.eigs."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 2, 7, 40, 200]


def _random_symmetric(n, rng):
    a = rng.uniform(-1, 1, (n, n))
    return 0.5 * (a + a.T)


def _arrow_tridiagonal(n, rng):
    """the projected matrix after a thick restart: k kept Ritz values, their couplings to vector k, a tridiagonal tail"""
    k = n // 2
    a = np.diag(2.0 + rng.uniform(-1, 1, n))
    for i in range(k):
        a[i, k] = a[k, i] = 1e-3 * rng.uniform(-1, 1)
    for i in range(k, n - 1):
        a[i, i + 1] = a[i + 1, i] = 0.5 + 0.5 * rng.uniform(0, 1)
    return a


@pytest.mark.parametrize("kind", ["random", "arrow"])
@pytest.mark.parametrize("n", SIZES)
def test_symeig_host_against_numpy(kind, n):
    import qex_amd as q

    rng = np.random.default_rng(1000 * n + (kind == "arrow"))
    a = _random_symmetric(n, rng) if kind == "random" else _arrow_tridiagonal(n, rng)
    w, z = q.symeig_host(a)
    wr = np.linalg.eigh(a)[0]
    na = np.linalg.norm(a)
    dev, orth = np.abs(w - wr).max(), np.abs(z.T @ z - np.eye(n)).max()
    res = np.abs(a @ z - z * w).max()
    print("%s n = %d: |w - eigh| %.2e (bound %.2e), |Z^T Z - 1| %.2e, |A Z - Z W| %.2e" % (kind, n, dev, 1e-13 * na, orth, res))
    assert np.all(np.diff(w) >= 0)
    assert dev <= 1e-13 * na
    assert orth <= 1e-13
    # not in the issue's list: z's columns belong to THEIR eigenvalues.  Bound: the rounding of ~10 sweeps of n rotations per
    # column, 10 n^(1/2) eps |a| < 1e-12 |a| up to n = 200
    assert res <= 1e-12 * na


def test_symeig_host_rejects_bad_arguments():
    import qex_amd as q

    import ctypes as C

    L, pd = q.lib(), C.POINTER(C.c_double)
    a, w = np.eye(2), np.zeros(2)
    assert L.qexhip_symeig_host(a.ctypes.data_as(pd), -1, w.ctypes.data_as(pd), None) == -1
    assert L.qexhip_symeig_host(None, 2, w.ctypes.data_as(pd), None) == -1
    assert L.qexhip_symeig_host(None, 0, None, None) == 0
    a[0, 1] = a[1, 0] = np.nan
    assert L.qexhip_symeig_host(a.ctypes.data_as(pd), 2, w.ctypes.data_as(pd), None) == -1


def test_symeig_host_under_asan_and_ubsan(tmp_path):
    """tests/cpp/test_symeig_san.cpp + qex_amd/csrc/symeig_host.cpp compiled together with -fsanitize=address,undefined: a
    stand-alone program with its own main (the library loaded into Python is not involved), run as it is."""
    exe = str(tmp_path / "test_symeig_san")
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_symeig_san.cpp"),
                           os.path.join(ROOT, "qex_amd", "csrc", "symeig_host.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, env=env)
    print(p.stdout[-3000:])
    print(p.stderr[-3000:])
    assert p.returncode == 0 and "symeig sanitizer run: Passed" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr and "LeakSanitizer" not in p.stderr


GOOD = dict(nev=16, nvecs=40, relerr=0.0, abserr=1e-9, max_restarts=100, cheb_degree=8, cheb_lo=0.3, cheb_hi=0.0, seed=1)


@pytest.mark.parametrize("change", [
    dict(nev=41), dict(nev=0), dict(nvecs=513), dict(nvecs=0, nev=0), dict(cheb_degree=-1), dict(max_restarts=-1), dict(relerr=-1.0),
    dict(abserr=float("nan")), dict(cheb_lo=0.0), dict(cheb_lo=2.0, cheb_hi=1.0), dict(cheb_hi=-1.0),
])
def test_eig_options_are_refused_without_a_device(change):
    """nev > nvecs, nvecs over the cap (QEXHIP_EIG_MAX_NVECS = 512), a negative degree, ... : QEXHIP_ERR_ARG from the host-only check
    that qexhip_stag_eigs runs before it looks at its handle"""
    import qex_amd as q

    assert q.eig_check_opts(**GOOD) == 0
    assert q.eig_check_opts(**dict(GOOD, cheb_degree=0, cheb_lo=0.0)) == 0
    assert q.eig_check_opts(**dict(GOOD, **change)) == -1
    assert q.lib().qexhip_last_error()


def test_eig_entries_refuse_bad_sizes_before_touching_the_handle():
    import ctypes as C

    import qex_amd as q

    L = q.lib()
    bid = C.c_int(0)
    assert L.qexhip_eig_new(None, 513, C.byref(bid)) == -1 and b"nvecs" in L.qexhip_last_error()
    assert L.qexhip_eig_new(None, 0, C.byref(bid)) == -1
    o = q.EigOpts(**dict(GOOD, nev=41))
    assert L.qexhip_stag_eigs(None, 1, C.byref(o), None, None, None, None) == -1 and b"nev > nvecs" in L.qexhip_last_error()
