"""numpy restatement of the low-mode averaging of the scalar trace (include/qexhip.h "LOW-MODE AVERAGING"): the projector P onto
the even low modes and their odd partners, the exact low-mode diagonal L(x), and the LMA trace on top of scalar_trace_ref.  Nothing
here touches a GPU; links and spectra come from eig_ref (gauge_warm(0.3), seed 987654321, one-hop links).

Vectors are complex arrays of 3 vol entries, (site, colour) with the even sites first -- the host field order -- or (3 vol, k)
matrices of such columns.  D is the oracle's Staggered.D at m = 0, either applied column by column (`oracle_D`) or as the dense
matrix built from one oracle application per unit vector (`dense_D`)."""
import functools

import numpy as np

import eig_ref as E
import scalar_trace_ref as R


def cfull(field):
    f = np.asarray(field)
    return (f[..., 0] + 1j * f[..., 1]).reshape(-1)


def field_full(vec, vol):
    v = np.asarray(vec).reshape(vol, 3)
    return np.ascontiguousarray(np.stack([v.real, v.imag], axis=-1))


def oracle_D(lat):
    """X -> D X with the oracle operator, column by column"""
    from oracle import oracle as o

    lo, g, _, _ = E.inputs(tuple(lat))

    def mul(X):
        X = np.asarray(X)
        cols = X.reshape(X.shape[0], -1)
        out = np.stack([cfull(o.D(lo, g, None, field_full(cols[:, k], lo.vol), 0.0)) for k in range(cols.shape[1])], axis=1)
        return out.reshape(X.shape)

    return mul


@functools.lru_cache(maxsize=None)
def dense_Doe(lat):
    """D_oe as a complex (3 Vh, 3 Vh) matrix: oracle.D(m = 0) on the even unit vectors"""
    from oracle import oracle as o

    lo, g, _, _ = E.inputs(tuple(lat))
    n = 3 * (lo.vol // 2)
    Doe = np.zeros((n, n), dtype=np.complex128)
    x = lo.new_vector()
    for k in range(n):
        x[k // 3, k % 3, 0] = 1.0
        Doe[:, k] = cfull(o.D(lo, g, None, x, 0.0))[n:]
        x[k // 3, k % 3, 0] = 0.0
    return Doe


@functools.lru_cache(maxsize=None)
def dense_D(lat):
    """the full anti-Hermitian D = [[0, D_eo], [D_oe, 0]] with D_eo = -D_oe^+"""
    Doe = dense_Doe(tuple(lat))
    n = Doe.shape[0]
    D = np.zeros((2 * n, 2 * n), dtype=np.complex128)
    D[n:, :n] = Doe
    D[:n, n:] = -Doe.conj().T
    return D


class Projector:
    """P onto span{(v_i, 0), (0, D_oe v_i / sqrt(lam_i))} from the even vectors V (3 Vh, nev) and their lam; mul: X -> D X.
    On the odd sites P phi_o = -D_oe V diag(1/lam) V^+ D_eo phi_o; a mode with lam_i <= 0 has no odd partner."""

    def __init__(self, V, lam, mul):
        self.V, self.lam, self.mul = np.asarray(V), np.asarray(lam, dtype=np.float64), mul
        self.n = self.V.shape[0]
        self.inv = np.where(self.lam > 0, 1.0 / np.where(self.lam > 0, self.lam, 1.0), 0.0)

    def P(self, X):
        X = np.asarray(X)
        n, V = self.n, self.V
        out = np.zeros_like(X, dtype=np.complex128)
        out[:n] = V @ (V.conj().T @ X[:n])
        xo = np.zeros_like(out)
        xo[n:] = X[n:]
        c = V.conj().T @ self.mul(xo)[:n]                       # V^+ D_eo phi_o
        c = (self.inv * c.T).T
        ye = np.zeros_like(out)
        ye[:n] = V @ c
        out[n:] = -self.mul(ye)[n:]
        return out

    def Q(self, X):
        return np.asarray(X) - self.P(X)

    def diag(self, mass):
        """L(x), the site diagonal of P (D+m)^-1 summed over colour: (vol,) real, even sites first"""
        n, V = self.n, self.V
        w = mass / (mass * mass + self.lam)
        Ve = np.zeros((2 * n, V.shape[1]), dtype=np.complex128)
        Ve[:n] = V
        DV = self.mul(Ve)[n:]
        Le = (np.abs(V) ** 2) @ w
        Lo = (np.abs(DV) ** 2) @ (w * self.inv)
        return np.concatenate([Le, Lo]).reshape(-1, 3).sum(axis=1)


def lma_trace(proj, pairs, coords, nt, mass, improved, nc=3):
    """The LMA trace of one noise source from the (b_d, phi_d) pairs of scalar_trace_ref.scalar_trace (its third return value):
    (trce (vol, 2), est (nt,), low (vol,) = L / nc)"""
    vol = pairs[0][0].shape[0]
    trce = np.zeros((vol, 2))
    for b, phi in pairs:
        qphi = field_full(proj.Q(cfull(phi)), vol)
        if improved:
            R.accumulate(trce, qphi, qphi, mass)
        else:
            R.accumulate(trce, b, qphi, 1.0)
    L = proj.diag(mass)
    trce[:, 0] += L
    trce *= 1.0 / nc
    return trce, R.slice_sums(trce, coords, nt)[:, 0] / (vol // nt), L / nc
