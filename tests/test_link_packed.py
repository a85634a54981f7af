"""The packed lossless link format's encoder and decoder (qex_amd/csrc/link_residual.h, lp_encode / lp_decode) run on the host
through qexhip_link_packed_host: the same functions the encoding kernel and the Dslash sweep run.  No device needed.

Every link that is not escaped must decode to its 18 reals bit for bit; the window edges of rows 0,1 (2^-15 <= |v| < 2) and the
edges of the 19-bit residual range must either round-trip exactly or be escaped."""
import numpy as np
import pytest

import qex_amd as q
from oracle import oracle as o

KMAX = 262143


def _adjoints(m):
    return np.ascontiguousarray(np.swapaxes(m, 1, 2) * np.array([1.0, -1.0]))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _check_roundtrip(m):
    esc, dec = q.link_packed_host(m)
    ok = ~esc
    assert np.array_equal(_bits(dec[ok]), _bits(m[ok]))
    return esc, dec


def test_random_32x4_escape_rate_and_bitwise_decode():
    """QEX g.random at 32^4 (the benchmark's links), forward links and the stored backward adjoints (CPU estimate with numpy
    rebuilds: 0.12-0.13 % escaped)."""
    lat = [32, 32, 32, 32]
    lo = o.Layout(lat)
    rf = o.RngField(lo, o.RNG_MILC6, 987654321)
    g = o.gauge_random(lo, rf)
    o.rephase(lo, g)
    m = g.reshape(-1, 3, 3, 2)
    e1, _ = _check_roundtrip(m)
    e2, _ = _check_roundtrip(_adjoints(m))
    frac = np.concatenate([e1, e2]).mean()
    print("escaped fraction of 32^4 g.random, forward + adjoint: %.5f %%" % (100 * frac))
    assert 0 < frac < 0.0025, frac


def _su3(rng, n):
    z = rng.standard_normal((n, 3, 3)) + 1j * rng.standard_normal((n, 3, 3))
    qm, r = np.linalg.qr(z)
    qm = qm * (np.diagonal(r, axis1=1, axis2=2) / np.abs(np.diagonal(r, axis1=1, axis2=2)))[:, None, :]
    qm = qm / np.linalg.det(qm)[:, None, None] ** (1.0 / 3.0)
    return np.stack([qm.real, qm.imag], axis=-1)


def _in_window(m):
    """links whose rows 0,1 all lie in the window (a random SU(3) has the odd entry below 2^-15)"""
    a = np.abs(m[:, :2])
    return ((a >= 2.0 ** -15) & (a < 2.0)).all(axis=(1, 2, 3))


def _rebuilt(m):
    """The decoder's rebuild of row 2: the residual format's decode of an escaped link (k = 0) -- the packed form runs the same
    lr_rebuild on the same rows 0,1."""
    big = m.copy()
    big[:, 2] += 1.0
    esc, row2 = q.link_residual_host(big)
    assert esc.all()
    return row2


def _links(seed, n):
    m = _su3(np.random.default_rng(seed), n)
    return m[_in_window(m)]


@pytest.mark.parametrize("v,escaped", [(2.0 ** -15, False), (np.nextafter(2.0, 0.0), False), (-(2.0 ** -15), False),
                                       (-np.nextafter(2.0, 0.0), False), (np.nextafter(2.0 ** -15, 0.0), True), (2.0, True),
                                       (0.0, True), (-0.0, True), (5e-320, True), (np.inf, True), (-np.inf, True), (np.nan, True)])
def test_window_edges(v, escaped):
    """One entry of rows 0,1 set to v, row 2 made the exact rebuild of the changed rows (k = 0): the window alone decides.  Every one
    of the 12 positions takes its turn."""
    base = _links(4, 64)[:12]
    m = base.copy()
    for i in range(12):
        m[i].reshape(18)[i] = v
    if np.isfinite(v):
        m[:, 2] = _rebuilt(m)
    esc, dec = _check_roundtrip(m)
    assert (esc == escaped).all(), (v, esc)
    if not escaped:
        got = np.array([dec[i].reshape(18)[i] for i in range(12)])
        assert np.array_equal(_bits(got), _bits(np.full(12, v)))       # (the sign too)


@pytest.mark.parametrize("k,escaped", [(0, False), (1, False), (-1, False), (32768, False), (-32768, False), (KMAX, False),
                                       (-KMAX, False), (KMAX + 1, True), (-KMAX - 1, True)])
def test_residual_range(k, escaped):
    m = _links(2, 256)
    rec = _rebuilt(m)
    ulp = np.spacing(np.abs(rec)).astype(np.float64)
    # stay inside the binade of rec: a residual that crosses it is an inexact multiple of ulp(rec) -> escaped
    row2 = rec + k * ulp
    same_binade = np.frexp(row2)[1] == np.frexp(rec)[1]
    sel = same_binade.all(axis=(1, 2))
    m2 = m.copy()
    m2[:, 2] = row2
    esc, _ = _check_roundtrip(m2[sel])
    assert sel.sum() > 20
    assert (esc == escaped).all(), (k, esc.mean())


def test_random_residuals_in_every_position_round_trip():
    """Random k in all six positions at once, random rows: every payload bit of the 12 slots and the extra word takes both values."""
    rng = np.random.default_rng(6)
    m = _links(7, 4096)
    rec = _rebuilt(m)
    ulp = np.spacing(np.abs(rec)).astype(np.float64)
    k = rng.integers(-KMAX, KMAX + 1, size=rec.shape)
    k[:6] = np.array([[KMAX] * 6, [-KMAX] * 6, [0x2AAAA] * 6, [-0x2AAAA] * 6, [0x15555] * 6, [-0x15555] * 6]).reshape(6, 3, 2)
    row2 = rec + k * ulp
    sel = (np.frexp(row2)[1] == np.frexp(rec)[1]).all(axis=(1, 2))
    m2 = m.copy()
    m2[:, 2] = row2
    esc, _ = _check_roundtrip(m2[sel])
    assert sel.sum() > 1000
    assert not esc.any(), esc.mean()
    # the six positions are told apart: the decoded row 2 is the one stored (checked bitwise above), for distinct k per position
    assert (np.abs(k[sel]).reshape(-1, 6).std(axis=1) > 0).mean() > 0.99


def test_negative_determinant_round_trips():
    m = _links(1, 1024)
    esc, _ = _check_roundtrip(-m)          # det -1: the sign bit
    assert esc.mean() < 0.01
