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
