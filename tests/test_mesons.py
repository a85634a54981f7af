"""Host side of the meson measurement (src/observables/fpvaMeas.nim, src/observables/sources.nim): the Walsh-Hadamard transform
of printLocalMesons, point and wall sources in the even/odd order, and the numpy restatement of stagLocalMesons that the GPU tests
(tests/test_gpu_mesons.py) hold the kernels to, checked here against a site-by-site loop written straight from fpvaMeas.nim:33-61."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import qex_amd as q  # noqa: E402
import meson_ref as mr  # noqa: E402


def hadamard8():
    return np.array([[(-1) ** bin(s & k).count("1") for s in range(8)] for k in range(8)], dtype=np.float64)


def test_sft_is_the_walsh_hadamard_transform_over_the_corner_bits():
    rng = np.random.default_rng(5)
    c = rng.standard_normal((6, 8))
    ref = c @ hadamard8().T                      # out[t][k] = sum_s (-1)^popcount(s & k) c[t][s]
    d = c.copy()
    for b in (1, 2, 4):
        q.sft(d, b)
    assert np.allclose(d, ref, rtol=0, atol=1e-13)
    lines = []
    e = c.copy()
    q.printLocalMesons(e, 0.25, out=lines.append)
    assert np.allclose(e, ref, rtol=0, atol=1e-13)             # in place, like the reference's `var c`
    assert len(lines) == 8 * 7 and lines[0] == "corner: 0" and lines[7] == "corner: 1"
    for s in range(8):
        for t in range(6):
            tt, val = lines[s * 7 + 1 + t].split()
            assert int(tt) == t and abs(float(val) - 0.25 * ref[t, s]) < 1e-13


def test_sft_single_bit_butterfly():
    c = np.arange(16, dtype=np.float64).reshape(2, 8)
    d = q.sft(c.copy(), 2)
    for s in range(8):
        if s & 2 == 0:
            assert np.array_equal(d[:, s], c[:, s] + c[:, s + 2]) and np.array_equal(d[:, s + 2], c[:, s] - c[:, s + 2])


@pytest.mark.parametrize("lat", [[4, 4, 4, 4], [4, 6, 10, 6]])
def test_point_source_lands_on_the_site_in_even_odd_order(lat):
    lo = q.Layout(lat)
    for coord, ic in (([0, 0, 0, 2], 1), ([1, 2, 3, lat[3] - 1], 2), ([3, 1, 0, 0], 0)):
        v = q.pointSource(lo, coord, ic)
        nz = np.argwhere(v != 0)
        assert len(nz) == 1
        i, c, ri = nz[0]
        assert lo.coord(i) == coord and c == ic and ri == 0 and v[i, c, ri] == 1.0
        par = sum(coord) & 1
        assert (i >= lo.vol // 2) == bool(par)


def test_point_source_on_a_t_sharded_lattice_is_set_by_the_owner_only():
    glo = q.Layout([4, 4, 4, 8])
    coord = [1, 2, 3, 5]
    full = q.pointSource(glo, coord, 1)
    owners = 0
    for rank in range(4):
        loc, idx = glo.shard_indices(4, rank)
        v = q.pointSource(loc, coord, 1, t_offset=rank * 2)
        assert np.array_equal(v, full[idx])
        owners += int(v.any())
    assert owners == 1


def test_wall_source_fills_the_slice():
    glo = q.Layout([4, 4, 2, 8])
    w = np.array([1 + 2j, -0.5j, 3.0])
    full = q.wallSource(glo, 5, w)
    on = glo.coords[:, 3] == 5
    assert np.array_equal(mr.cvec(full)[on], np.broadcast_to(w, (on.sum(), 3)))
    assert not full[~on].any()
    for rank in range(2):
        loc, idx = glo.shard_indices(2, rank)
        assert np.array_equal(q.wallSource(loc, 5, w, t_offset=rank * 4), full[idx])


def loop_mesons(lo, v1, v2, t0):
    """stagLocalMesons, fpvaMeas.nim:33-61, site by site"""
    nt = lo.lat[3]
    c = [[0.0] * 8 for _ in range(nt)]
    for i in range(lo.vol):
        x = lo.coord(i)
        t = x[3]
        s = (x[0] & 1) + ((x[1] & 1) << 1) + ((x[2] & 1) << 2)
        tt = (t + nt - t0) % nt
        acc = 0.0
        for k in range(3):
            acc += v1[i, k, 0] * v2[i, k, 0] + v1[i, k, 1] * v2[i, k, 1]
        c[tt][s] += acc
    return np.array(c)


@pytest.mark.parametrize("lat,t0", [([4, 4, 4, 4], 0), ([4, 6, 2, 6], 5), ([2, 4, 4, 8], 3)])
def test_numpy_restatement_against_the_site_loop(lat, t0):
    lo = q.Layout(lat)
    rng = np.random.default_rng(sum(lat) + t0)
    a, b = rng.standard_normal((2, lo.vol, 3, 2))
    ref = loop_mesons(lo, a, b, t0)
    got = mr.local_mesons(lo, [a], [b], t0)
    assert np.allclose(got, ref, rtol=0, atol=1e-12 * np.abs(ref).max())
    two = mr.local_mesons(lo, [a, b], [b, b], t0)
    assert np.allclose(two, ref + loop_mesons(lo, b, b, t0), rtol=0, atol=1e-12 * np.abs(two).max())


def test_numpy_sym_shift_of_a_point_is_two_links():
    lo = q.Layout([4, 4, 4, 4])
    rng = np.random.default_rng(3)
    g = rng.standard_normal((lo.vol, 4, 3, 3, 2))
    x0 = [1, 2, 3, 0]
    src = q.pointSource(lo, x0, 2)
    for mu in range(3):
        r = mr.cvec(mr.sym_shift(lo, g, src, mu))
        lo_c, hi_c = list(x0), list(x0)
        lo_c[mu] -= 1
        hi_c[mu] = (hi_c[mu] + 1) % 4
        i_lo, i_hi = lo.index(lo_c), lo.index(hi_c)
        assert set(np.flatnonzero(np.abs(r).sum(axis=1))) == {i_lo, i_hi}
        U = g[:, mu, :, :, 0] + 1j * g[:, mu, :, :, 1]
        assert np.allclose(r[i_lo], U[i_lo][:, 2])                 # U_mu(x0 - mu) x(x0): the site below reads forward
        assert np.allclose(r[i_hi], U[lo.index(x0)].conj()[2, :])  # U_mu(x0)^+ x(x0): the site above reads backward
