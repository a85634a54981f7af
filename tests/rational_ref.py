"""Reference for the rational functions of M^+M behind qexhip_dev_rational_xx / qexhip_md_hisq_fforce_rational, on the oracle.

    M^+M = m^2 - D_eo D_oe = A(m) / 4 on one parity,   r(x) = f0 + sum_k alpha_k / (x + beta_k).

Mapping (include/qexhip.h): terms sorted by beta, base mass m_0 = sqrt(m^2 + beta_min), shifts sigma_k = 4 (beta_k - beta_min),
(A(m_0) + sigma_k) y_k = b, r(M^+M) b = f0 b + sum_k 4 alpha_k y_k.

The y_k are solved in binary128.  oracle.solveXX_multi_ext, the binary128 multi-shift CG, returns the history and the count only,
so every y_k comes from the binary128 single-mass CG qo_solveXX_ext at the mass m_k = sqrt(m_0^2 + sigma_k / 4), which IS system k
(A(m_0) + sigma_k = A(m_k)); the multi-shift twin supplies the iteration count and history of the mapped shifts.  The sum is formed
in long double from the y_k rounded to double: 1e-16 relative, far below the 1e-12 at which the fp64 solvers stop.
Shifted solutions are cached per (links, source, parity, m_k), so rationals that share poles share solves."""
import ctypes as C

import numpy as np

REF_R2 = 1e-34       # binary128 solves: |r|^2 <= 1e-34 |b|^2
REF_MAXITS = 20000
_cache = {}


def mapped_shifts(mass, alpha, beta):
    """(order, [m_0, sigma_1, ...]) as the library maps them"""
    beta = np.asarray(beta, dtype=np.float64)
    order = np.argsort(beta, kind="stable")
    bmin = float(beta[order[0]])
    m0 = float(np.sqrt(mass * mass + bmin))
    return order, [m0] + [4.0 * (float(beta[k]) - bmin) for k in order[1:]]


def pole_mass(mass, beta_k):
    return float(np.sqrt(mass * mass + beta_k))


def solve_ext(o, lo, fat, lng, b, m, par_even=True):
    """y with A(m) y = b on the parity, binary128 CG, rounded to double at the end"""
    key = (id(fat), id(lng), id(b), bool(par_even), float(m))
    if key not in _cache:
        L = o.lib()
        L.qo_solveXX_ext.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_int,
                                     C.c_void_p, C.c_int, C.POINTER(C.c_double)]
        x = np.zeros_like(b)
        fin = C.c_double(0)
        hist = np.zeros(1)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        its = L.qo_solveXX_ext(lo._h, p(fat), p(lng), p(x), p(b), float(m), REF_R2, REF_MAXITS, 1 if par_even else 0, p(hist), 0, C.byref(fin))
        assert its < REF_MAXITS, "binary128 reference solve did not converge"
        x.setflags(write=False)
        _cache[key] = (x, fat, lng, b)              # the arrays are kept alive: their ids are the key
    return _cache[key][0]


def rational_ref(o, lo, fat, lng, b, mass, f0, alpha, beta, par_even=True):
    """r(M^+M) b on the parity (the other parity zero), summed in long double"""
    h = lo.vol // 2
    sl = slice(0, h) if par_even else slice(h, 2 * h)
    acc = np.zeros(b.shape, dtype=np.longdouble)
    acc[sl] = np.longdouble(f0) * b[sl]
    for a, be in zip(alpha, beta):
        y = solve_ext(o, lo, fat, lng, b, pole_mass(mass, be), par_even)
        acc[sl] += np.longdouble(4.0 * a) * y[sl]
    return np.asarray(acc, dtype=np.float64)


def history_ref(o, lo, fat, lng, b, mass, alpha, beta, r2req, maxits, par_even=True, histcap=0):
    """(iterations, history) of the binary128 multi-shift CG with the mapped shifts"""
    _, sh = mapped_shifts(mass, alpha, beta)
    return o.solveXX_multi_ext(lo, fat, lng, b, sh, r2req, maxits, par_even, histcap)


def force_vectors(o, lo, fat, lng, phi, mass, alpha, beta):
    """[(psi_k, alpha_k / m_k)]: psi_k = D(m_k)^-1 phi with phi.odd = 0 -- psi_k.even = 4 m_k y_k, the odd sites by eoReconstruct"""
    h = lo.vol // 2
    zero = np.zeros_like(phi)
    out = []
    for a, be in zip(alpha, beta):
        mk = pole_mass(mass, be)
        psi = np.zeros_like(phi)
        psi[:h] = 4.0 * mk * solve_ext(o, lo, fat, lng, phi, mk, True)[:h]
        o.eoReconstruct(lo, fat, lng, psi, zero, mk)
        out.append((psi, a / mk))
    return out
