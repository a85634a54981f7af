"""numpy restatement of the meson measurement of src/observables/fpvaMeas.nim (symShift :16-31, stagLocalMesons :33-61) on host
fields in the V=1 even-odd order (qex_amd.layout.Layout): the yardstick of tests/test_mesons.py, tests/test_gpu_mesons.py and
tests/meson_rank_worker.py."""
import numpy as np


def cvec(v):
    """(vol, 3, 2) -> (vol, 3) complex"""
    return v[..., 0] + 1j * v[..., 1]


def rvec(z):
    return np.ascontiguousarray(np.stack([z.real, z.imag], axis=-1))


def corners(lo):
    x = lo.coords
    return (x[:, 0] & 1) | ((x[:, 1] & 1) << 1) | ((x[:, 2] & 1) << 2)


def local_mesons(lo, v1s, v2s, t0=0):
    """sum over the pairs of stagLocalMesons(v1, v2, t0): c[(t - t0) mod nt][corner] += Re<v1(x), v2(x)>"""
    nt = lo.lat[3]
    tt = (lo.coords[:, 3] - t0) % nt
    s = corners(lo)
    c = np.zeros((nt, 8))
    for a, b in zip(v1s, v2s):
        np.add.at(c, (tt, s), (a * b).sum(axis=(1, 2)))
    return c


def neighbours(lo, mu):
    """site indices of x + mu and x - mu"""
    fw, bw = lo.coords.copy(), lo.coords.copy()
    fw[:, mu] = (fw[:, mu] + 1) % lo.lat[mu]
    bw[:, mu] = (bw[:, mu] - 1) % lo.lat[mu]

    def idx(c):
        lex = c[:, 0] + lo.lat[0] * (c[:, 1] + lo.lat[1] * (c[:, 2] + lo.lat[2] * c[:, 3]))
        return lo._idx_of_lex[lex]

    return idx(fw), idx(bw)


def sym_shift(lo, g, x, mu):
    """r(x) = U_mu(x) x(x+mu) + U_mu(x-mu)^+ x(x-mu) with the links g (vol, 4, 3, 3, 2) as they are (phases included)"""
    U = g[:, mu, :, :, 0] + 1j * g[:, mu, :, :, 1]
    z = cvec(x)
    fw, bw = neighbours(lo, mu)
    r = np.einsum("sij,sj->si", U, z[fw]) + np.einsum("sji,sj->si", U[bw].conj(), z[bw])
    return rvec(r)


def fpva_tables(lo, g, solve, t0, point_source):
    """fpvaMeas.nim:112-127 with `solve(b) -> x` and `point_source(ic) -> src`: (cl, [cx, cy, cz]) raw tables"""
    nt = lo.lat[3]
    cl = np.zeros((nt, 8))
    cs = [np.zeros((nt, 8)) for _ in range(3)]
    for ic in range(3):
        src = point_source(ic)
        dest = solve(src)
        cl += local_mesons(lo, [dest], [dest], t0)
        for mu in range(3):
            destS = solve(sym_shift(lo, g, src, mu))
            cs[mu] += local_mesons(lo, [dest], [sym_shift(lo, g, destS, mu)], t0)
    return cl, cs
