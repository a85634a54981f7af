"""Shared reference data of the low-mode tests (test_gpu_eig.py, eig_rank_worker.py): inputs, the dense even-even operator and
its spectrum, a numpy CG.  Everything is computed once per lattice and cached; nothing here touches a GPU.

Inputs: gauge_warm(0.3) from RngMilc6 seed 987654321, rephased; H = stagD2xx(m2 = 0) / 4 = -D_eo D_oe on the even sites, built one
oracle application per unit vector (the operator is complex-linear, so the 3 Vh real unit vectors give all columns)."""
import functools

import numpy as np

SEED = 987654321


def cvec(field, vh):
    """even half of a host field (vol, 3, 2) as a complex vector of 3 vh entries"""
    e = np.asarray(field)[:vh]
    return (e[..., 0] + 1j * e[..., 1]).reshape(-1)


def field_of(vec, vol):
    """complex vector on the even sites -> host field (odd sites zero)"""
    f = np.zeros((vol, 3, 2))
    v = np.asarray(vec).reshape(vol // 2, 3)
    f[: vol // 2, :, 0], f[: vol // 2, :, 1] = v.real, v.imag
    return f


@functools.lru_cache(maxsize=None)
def inputs(lat, hisq=False):
    """(layout, fat links, long links or None, gaussian vector b)"""
    from oracle import oracle as o

    o.build()
    lo = o.Layout(list(lat))
    rf = o.RngField(lo, o.RNG_MILC6, SEED)
    g = o.gauge_warm(lo, 0.3, rf)
    o.rephase(lo, g)
    b = o.vector_gaussian(lo, rf)
    if hisq:
        fl, ll = o.hisq_smear(lo, g)
        return lo, fl, ll, b
    return lo, g, None, b


@functools.lru_cache(maxsize=None)
def dense(lat, hisq=False):
    """(H as a complex (3 Vh, 3 Vh) matrix, eigenvalues ascending, eigenvectors in columns)"""
    from oracle import oracle as o

    lo, fat, lng, _ = inputs(lat, hisq)
    vh = lo.vol // 2
    n = 3 * vh
    H = np.zeros((n, n), dtype=np.complex128)
    x = lo.new_vector()
    for k in range(n):
        x[k // 3, k % 3, 0] = 1.0
        H[:, k] = cvec(o.stagD2xx(lo, fat, lng, x, 0.0, True), vh) / 4.0
        x[k // 3, k % 3, 0] = 0.0
    assert np.abs(H - H.conj().T).max() < 1e-13
    w, v = np.linalg.eigh(0.5 * (H + H.conj().T))
    return H, w, v


def oracle_H(lat, hisq, vec):
    """H vec with the oracle operator itself (not the dense matrix)"""
    from oracle import oracle as o

    lo, fat, lng, _ = inputs(lat, hisq)
    return cvec(o.stagD2xx(lo, fat, lng, field_of(vec, lo.vol), 0.0, True), lo.vol // 2) / 4.0


# ---------------------------------------------------------------- integer test data of the block kernels (test_gpu_eig_blocks.py)
# Small integers make every product, fma and partial sum of the block kernels exact in any order, so a device result has to be
# np.array_equal to the integer reference: a wrong, missing or doubled element cannot hide in a tolerance.  The values come from
# a 64-bit mixing function (the finaliser of splitmix64) of (site, colour, re/im, vector), so that no two vectors, tiles, colours
# or re/im planes are alike -- a linear formula mod 17 would repeat every 17 vectors and every 17 tiles.
_M1, _M2, _M3 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xC2B2AE3D27D4EB4F), np.uint64(0x165667B19E3779F9)
_F1, _F2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def _mix(x):
    x = x ^ (x >> np.uint64(30))
    x = x * _F1
    x = x ^ (x >> np.uint64(27))
    x = x * _F2
    return x ^ (x >> np.uint64(31))


def int_pattern(vh, js, salt=0):
    """int8 array (vh, 3, 2, len(js)) with entries in -8 .. 7: element (site c, colour a, re/im p) of vector js[.]"""
    js = np.asarray(js, dtype=np.uint64)
    out = np.empty((vh, 6, len(js)), dtype=np.int8)
    with np.errstate(over="ignore"):
        c = (np.arange(vh, dtype=np.uint64) + np.uint64(1)) * _M1
        ap = (np.arange(6, dtype=np.uint64) + np.uint64(1 + 8 * salt)) * _M3
        j = (js + np.uint64(1)) * _M2
        ca = c[:, None] ^ ap[None, :]
        for s in range(0, len(js), 32):          # 32 vectors at a time: the 64-bit temporaries stay small
            x = _mix(ca[:, :, None] + j[None, None, s:s + 32])
            out[:, :, s:s + 32] = (x >> np.uint64(60)).astype(np.int8) - np.int8(8)
    return out.reshape(vh, 3, 2, len(js))


def int_matrix(m, k, salt=0):
    """integer (m, k) matrix with entries in {-2, -1, 1, 2} as float64 (Q of a rotation; two columns make complex axpy
    coefficients).  No zeros: every input vector then counts in every output, so reading a wrong one always shows."""
    with np.errstate(over="ignore"):
        r = (np.arange(m, dtype=np.uint64) + np.uint64(1)) * _M1
        c = (np.arange(k, dtype=np.uint64) + np.uint64(1 + 1000 * salt)) * _M2
        x = _mix(r[:, None] + c[None, :])
    return np.array([-2.0, -1.0, 1.0, 2.0])[(x >> np.uint64(62)).astype(np.int64)]


def exact_matmul(A, B):
    """A @ B of integer-valued float64 matrices as int64.  max|A| max|B| (inner dimension) bounds every partial sum in any order;
    below 2^53 the float64 product (BLAS, any blocking) is therefore the exact integer result."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    assert np.abs(A).max() * np.abs(B).max() * A.shape[-1] < 2.0 ** 53
    C = A @ B
    assert np.array_equal(C, np.rint(C))
    return C.astype(np.int64)


def cg(A, b, x0, r2req, maxits=100000):
    """CG of src/solvers/cg.nim on the dense A from x0, stopping on the recursive |r|^2 <= r2req |b|^2: (x, iterations)"""
    x = x0.copy()
    r = b - A @ x
    b2 = np.vdot(b, b).real
    r2 = np.vdot(r, r).real
    p = r.copy()
    its = 0
    while its < maxits and r2 > r2req * b2:
        Ap = A @ p
        alpha = r2 / np.vdot(p, Ap).real
        x += alpha * p
        r -= alpha * Ap
        r2n = np.vdot(r, r).real
        p = r + (r2n / r2) * p
        r2 = r2n
        its += 1
    return x, its
