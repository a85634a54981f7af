"""The orthogonal lossless link format's encoder and decoder (qex_amd/csrc/link_residual.h, lo_encode / lo_decode) run on the host
through qexhip_link_ortho_host: the same functions the encoding kernel and the Dslash sweep run.  No device needed.

The format stores a0, a1, a2, b0, b1 of rows 0,1 and rebuilds b2 (orthogonality of the two rows, 23-bit residuals) and row 2
(20-bit residuals).  Every link that is not escaped must decode to its 18 reals bit for bit; the window edges of the ten stored
reals (2^-15 <= |v| < 2) and the edges of both residual ranges must either round-trip exactly or be escaped."""
import numpy as np
import pytest

import qex_amd as q
from oracle import oracle as o

K2MAX = 2 ** 19 - 1         # row 2: 20 bits
KBMAX = 2 ** 22 - 1         # b2: 23 bits
STORED = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]          # a0, a1, a2, b0, b1 (re, im) among the 18 reals


def _adjoints(m):
    return np.ascontiguousarray(np.swapaxes(m, 1, 2) * np.array([1.0, -1.0]))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _check_roundtrip(m):
    esc, dec = q.link_ortho_host(m)
    ok = ~esc
    assert np.array_equal(_bits(dec[ok]), _bits(m[ok]))
    return esc, dec


def test_random_16x4_escape_rate_and_bitwise_decode():
    """QEX g.random at 16^4, forward links and the stored backward adjoints (CPU estimate with numpy rebuilds: 0.09-0.15 % escaped;
    the cap is the project's 1 % fallback rule)."""
    lat = [16, 16, 16, 16]
    lo = o.Layout(lat)
    rf = o.RngField(lo, o.RNG_MILC6, 987654321)
    g = o.gauge_random(lo, rf)
    o.rephase(lo, g)
    m = g.reshape(-1, 3, 3, 2)
    e1, _ = _check_roundtrip(m)
    e2, _ = _check_roundtrip(_adjoints(m))
    esc = np.concatenate([e1, e2])
    pk = np.concatenate([q.link_packed_host(m)[0], q.link_packed_host(_adjoints(m))[0]])
    print("escaped of 16^4 g.random, forward + adjoint: %d of %d = %.5f %% (packed form: %d = %.5f %%)"
          % (esc.sum(), esc.size, 100 * esc.mean(), pk.sum(), 100 * pk.mean()))
    assert 0 < esc.mean() <= 0.01, esc.mean()


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


def _links(seed, n):
    m = _su3(np.random.default_rng(seed), n)
    return m[_in_window(m)]


def _exact(m):
    """The links with b2 and row 2 replaced by the decoder's own rebuilds (all eight residuals 0).  b2: pushed far off, the link is
    escaped and decodes to the rebuild; row 2 likewise, through the residual format on the completed rows 0,1."""
    big = m.copy()
    big[:, 1, 2] += 1.0
    esc, dec = q.link_ortho_host(big)
    assert esc.all()
    out = m.copy()
    out[:, 1, 2] = dec[:, 1, 2]
    big = out.copy()
    big[:, 2] += 1.0
    esc, row2 = q.link_residual_host(big)
    assert esc.all()
    out[:, 2] = row2
    return out


def _with_residuals(m, kb, k2):
    """exact links with residuals kb (n, 2) on b2 and k2 (n, 3, 2) on row 2, and which of them keep every shifted real inside the
    binade of its rebuild (a residual that crosses it is an inexact multiple of ulp(rec) -> escaped).  Row 2's rebuild depends on
    b2, so it is taken after b2 has moved."""
    e = _exact(m)
    recb = e[:, 1, 2]
    b2 = recb + kb * np.spacing(np.abs(recb))
    selb = (np.frexp(b2)[1] == np.frexp(recb)[1]).all(axis=1)
    e[:, 1, 2] = b2
    big = e.copy()
    big[:, 2] += 1.0
    rec2 = q.link_residual_host(big)[1]
    row2 = rec2 + k2 * np.spacing(np.abs(rec2))
    sel2 = (np.frexp(row2)[1] == np.frexp(rec2)[1]).all(axis=(1, 2))
    e[:, 2] = row2
    return e, selb & sel2


def test_exact_links_have_zero_residuals_and_round_trip():
    m = _exact(_links(3, 512))
    esc, _ = _check_roundtrip(m)
    assert not esc.any()


@pytest.mark.parametrize("v,escaped", [(2.0 ** -15, False), (np.nextafter(2.0, 0.0), False), (-(2.0 ** -15), False),
                                       (-np.nextafter(2.0, 0.0), False), (np.nextafter(2.0 ** -15, 0.0), True), (2.0, True),
                                       (0.0, True), (-0.0, True), (5e-320, True), (np.inf, True), (-np.inf, True), (np.nan, True)])
def test_window_edges(v, escaped):
    """One stored real set to v, b2 and row 2 made the exact rebuilds of the changed link (k = 0): the window alone decides.  Every
    one of the 10 stored positions takes its turn."""
    base = _links(4, 64)[:10]
    m = base.copy()
    for i, pos in enumerate(STORED):
        m[i].reshape(18)[pos] = v
    if np.isfinite(v):
        m = _exact(m)
    esc, dec = _check_roundtrip(m)
    assert (esc == escaped).all(), (v, esc)
    if not escaped:
        got = np.array([dec[i].reshape(18)[pos] for i, pos in enumerate(STORED)])
        assert np.array_equal(_bits(got), _bits(np.full(10, v)))       # (the sign too)


def test_b2_outside_the_window_round_trips():
    """b2 is rebuilt, not stored: the slot window does not apply to it"""
    rng = np.random.default_rng(9)
    n = 256
    r0 = rng.standard_normal((n, 3)) + 1j * rng.standard_normal((n, 3))
    r0 /= np.linalg.norm(r0, axis=1)[:, None]
    r1 = rng.standard_normal((n, 3)) + 1j * rng.standard_normal((n, 3))
    r1[:, 2] = 0
    # orthogonal to row 0 with b2 = 0: b0 conj(a0) + b1 conj(a1) = 0
    r1[:, 1] = -r1[:, 0] * np.conj(r0[:, 0]) / np.conj(r0[:, 1])
    r1 /= np.linalg.norm(r1, axis=1)[:, None]
    r1[:, 2] = 1e-9 * (1 + 1j)
    mm = np.stack([r0, r1, np.conj(np.cross(r0, r1))], axis=1)
    m = np.stack([mm.real, mm.imag], axis=-1)
    st = np.abs(m.reshape(n, 18)[:, STORED])
    keep = ((st >= 2.0 ** -15) & (st < 2.0)).all(axis=1)
    m = _exact(m[keep])
    assert keep.sum() > 100 and (np.abs(m[:, 1, 2]) < 2.0 ** -15).any()
    esc, _ = _check_roundtrip(m)
    assert not esc.any()


@pytest.mark.parametrize("k,escaped", [(0, False), (1, False), (-1, False), (K2MAX, False), (-K2MAX, False), (K2MAX + 1, True),
                                       (-K2MAX - 1, True)])
def test_row_2_residual_range(k, escaped):
    m = _links(2, 256)
    m2, sel = _with_residuals(m, np.zeros((len(m), 2)), np.full((len(m), 3, 2), float(k)))
    esc, _ = _check_roundtrip(m2[sel])
    assert sel.sum() > 20
    assert (esc == escaped).all(), (k, esc.mean())


@pytest.mark.parametrize("k,escaped", [(1, False), (-1, False), (K2MAX + 1, False), (-K2MAX - 1, False), (KBMAX, False),
                                       (-KBMAX, False), (KBMAX + 1, True), (-KBMAX - 1, True)])
def test_b2_residual_range(k, escaped):
    m = _links(2, 256)
    m2, sel = _with_residuals(m, np.full((len(m), 2), float(k)), np.zeros((len(m), 3, 2)))
    esc, _ = _check_roundtrip(m2[sel])
    assert sel.sum() > 20
    assert (esc == escaped).all(), (k, esc.mean())


def test_random_residuals_in_every_position_round_trip():
    """Random k in all eight positions at once, random rows: every payload bit of the ten slots and the two extra words takes both
    values (the first links carry the extremes and the alternating patterns)."""
    rng = np.random.default_rng(6)
    m = _links(7, 4096)
    n = len(m)
    k2 = rng.integers(-K2MAX, K2MAX + 1, size=(n, 3, 2))
    kb = rng.integers(-KBMAX, KBMAX + 1, size=(n, 2))
    pat2 = [K2MAX, -K2MAX, 0x55555, -0x55555, 0x2AAAA, -0x2AAAA]
    patb = [KBMAX, -KBMAX, 0x2AAAAA, -0x2AAAAA, 0x155555, -0x155555]
    for i in range(6):
        k2[i], kb[i] = pat2[i], patb[i]
    m2, sel = _with_residuals(m, kb.astype(float), k2.astype(float))
    esc, _ = _check_roundtrip(m2[sel])
    assert sel.sum() > 1000
    assert not esc.any(), esc.mean()
    # the eight positions are told apart: the decoded reals are the ones stored (checked bitwise above), for distinct k per position
    assert (np.abs(k2[sel]).reshape(-1, 6).std(axis=1) > 0).mean() > 0.99
    both = np.concatenate([k2.reshape(n, 6), kb], axis=1)[sel] & 0x7FFFFF
    assert (np.bitwise_or.reduce(both, axis=0)[:6] & 0xFFFFF == 0xFFFFF).all() and (np.bitwise_or.reduce(both, axis=0)[6:] == 0x7FFFFF).all()
    assert (np.bitwise_and.reduce(both, axis=0) == 0).all()


@pytest.mark.parametrize("mag", [2.0 ** -15, 2.0 ** -14])
def test_a2_at_the_lower_edge_of_the_window(mag):
    """|Re a2| = |Im a2| = the window's lower edge (the division's smallest denominator, |a2|^2 = 2^-29): rebuilt b2 loses ~14 bits
    there, which the 23-bit residual absorbs -- the links, unitary to rounding, still round-trip or are escaped, and most round-trip."""
    rng = np.random.default_rng(12)
    n = 2048
    r0 = rng.standard_normal((n, 3)) + 1j * rng.standard_normal((n, 3))
    r0[:, 2] = 0
    r0 /= np.linalg.norm(r0, axis=1)[:, None]
    r0[:, 2] = mag * (1 + 1j)
    r0[:, :2] *= np.sqrt(1 - 2 * mag * mag)
    r1 = rng.standard_normal((n, 3)) + 1j * rng.standard_normal((n, 3))
    r1 -= np.sum(np.conj(r0) * r1, axis=1)[:, None] * r0
    r1 /= np.linalg.norm(r1, axis=1)[:, None]
    mm = np.stack([r0, r1, np.conj(np.cross(r0, r1))], axis=1)
    m = np.stack([mm.real, mm.imag], axis=-1)
    assert (m[:, 0, 2] == mag).all()
    m = m[_in_window(m)]
    esc, _ = _check_roundtrip(m)
    print("|a2| at 2^%d: escaped %d of %d" % (int(np.log2(mag)), esc.sum(), len(m)))
    assert len(m) > 1000
    # s = a0 conj(b0) + a1 conj(b1) carries an absolute error of a few 2^-53 and is divided by |a2| <= 2^-13: b2 is rebuilt to about
    # 2^16 / |b2| ulp of 2^22 available, so only rows with |b2| below ~2^-6 (a few per cent of random rows at most) can escape
    assert esc.mean() < 0.05, esc.mean()
    # exact rebuilds on the same rows: the format itself holds at the edge
    esc0, _ = _check_roundtrip(_exact(m))
    assert not esc0.any()


def test_negative_determinant_round_trips():
    m = _links(1, 1024)
    esc, _ = _check_roundtrip(-m)          # det -1: the sign bit
    assert esc.mean() < 0.01
