"""The 16-bit operator of the SloppyHalf solves in numpy: links and vectors quantised with the restatement of the formats
(test_half_pack.pack_np / unpack_np), the hop sums by the oracle's stagD2.  Shared by tests/test_gpu_half.py (the operator against
the device) and tests/sloppy_ref.py (the 16-bit CG iteration step by step).  No device needed."""
import numpy as np

from test_half_pack import pack_np, unpack_np


def _cplx(a):
    return a[..., 0] + 1j * a[..., 1]


def _real(z):
    return np.ascontiguousarray(np.stack([z.real, z.imag], axis=-1))


def _q16(x, sc):
    return np.clip(np.rint(x * sc), -32767.0, 32767.0) / sc


def _links_fmt0(g):
    """18 reals as int16 of u 32767 / s, s = the largest |entry| of the field"""
    s = float(np.abs(g).max())
    return _q16(g, 32767.0 / s), s


def _links_fmt1(U):
    """complex (..., 3, 3): rows 0,1 as int16 of u 32767 (clamped), row 2 = +-conj(row0 x row1) of the STORED rows, the sign from the
    full-precision link"""
    rows = _q16(U[..., :2, :].real, 32767.0) + 1j * _q16(U[..., :2, :].imag, 32767.0)
    r2 = np.conj(np.cross(rows[..., 0, :], rows[..., 1, :]))
    r2_full = np.conj(np.cross(U[..., 0, :], U[..., 1, :]))
    neg = (U[..., 2, :] * np.conj(r2_full)).real.sum(axis=-1) < 0
    r2 = np.where(neg[..., None], -r2, r2)
    return np.concatenate([rows, r2[..., None, :]], axis=-2)


def _adj(U):
    return np.conj(np.swapaxes(U, -1, -2))


def _mul_i(a):
    return np.ascontiguousarray(np.stack([-a[..., 1], a[..., 0]], axis=-1))


def _mul_mi(a):
    return np.ascontiguousarray(np.stack([a[..., 1], -a[..., 0]], axis=-1))


def quant_sites(v):
    """v (n, 3, 2) -> the values as the 16-bit site format stores them"""
    qq, nn = pack_np(v.reshape(-1, 6))
    return unpack_np(qq, nn).reshape(-1, 3, 2)


class Model:
    """The 16-bit operator in numpy: links and vectors quantised with the restatement of the formats, the hop sums by the oracle's
    stagD2.  In format 1 the forward link of a pair stores rows 0,1 of U and the backward link rows 0,1 of U^+, so the two hop
    directions see different matrices: with H(G) = F(G) - B(G) (forward minus backward hops), F linear and B antilinear in G,
    F + B = -i H(i G) separates them."""

    def __init__(self, o, lo, fat, lng, fmt):
        self.o, self.lo, self.fmt = o, lo, fmt
        if fmt == 0:
            self.fat, self.s_fat = _links_fmt0(fat)
            self.lng, self.s_long = _links_fmt0(lng) if lng is not None else (None, 0.0)
        else:
            def both(g):
                U = _cplx(g)
                return _real(_links_fmt1(U)), _real(_adj(_links_fmt1(_adj(U))))
            self.fat_f, self.fat_b = both(fat)
            self.lng_f, self.lng_b = both(lng) if lng is not None else (None, None)
            mi = lambda g: None if g is None else _mul_i(g)   # noqa: E731
            self.ifat_f, self.ilng_f, self.ifat_b, self.ilng_b = mi(self.fat_f), mi(self.lng_f), mi(self.fat_b), mi(self.lng_b)

    def _H(self, fat, lng, x, parity):
        r = np.zeros_like(x)
        self.o.stagD2(self.lo, fat, lng, r, x, parity, 0.0, 0.0)
        return r

    def hops(self, x, parity):
        if self.fmt == 0:
            return self._H(self.fat, self.lng, x, parity)
        ha, hia = self._H(self.fat_f, self.lng_f, x, parity), self._H(self.ifat_f, self.ilng_f, x, parity)
        hb, hib = self._H(self.fat_b, self.lng_b, x, parity), self._H(self.ifat_b, self.ilng_b, x, parity)
        fwd = 0.5 * (ha + _mul_mi(hia))
        bwd = 0.5 * (_mul_mi(hib) - hb)
        return fwd - bwd

    @staticmethod
    def quant(v, sl, pre=None):
        """the sites of sl as stored; pre: applied to the values in front of the pack (tests/sloppy_ref.py's rounding noise)"""
        out = np.zeros_like(v)
        w = v[sl] if pre is None else pre(v[sl])
        out[sl] = quant_sites(w)
        return out

    def op_xx(self, x, m2, par_even, pre=None):
        """pre: applied in front of the two packs of computed values (the intermediate and the result), not of the input's"""
        h = self.lo.vol // 2
        sx, sy = (slice(0, h), slice(h, 2 * h)) if par_even else (slice(h, 2 * h), slice(0, h))
        px = 0 if par_even else 1
        xq = self.quant(x, sx)
        t = self.quant(self.hops(xq, 1 - px), sy, pre)
        r = np.zeros_like(x)
        r[sx] = 4.0 * m2 * xq[sx] - self.hops(t, px)[sx]
        return self.quant(r, sx, pre)
