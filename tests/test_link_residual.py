"""The lossless link format's encoder and decoder (qex_amd/csrc/link_residual.h) run on the host through
qexhip_link_residual_host: the same functions the encoding kernel and the Dslash sweep run.  No device needed.

Every link that is not escaped must decode to its stored row 2 bit for bit; edge cases (zeros, subnormals, powers of two,
defects at and beyond the int16 range) must either round-trip exactly or be escaped."""
import numpy as np
import pytest

import qex_amd as q
from oracle import oracle as o


def _adjoints(m):
    return np.ascontiguousarray(np.swapaxes(m, 1, 2) * np.array([1.0, -1.0]))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _check_roundtrip(m):
    esc, row2 = q.link_residual_host(m)
    ok = ~esc
    assert np.array_equal(_bits(row2[ok]), _bits(m[ok, 2]))
    return esc, row2


def test_random_32x4_escape_rate_and_bitwise_decode():
    """QEX g.random at 32^4 (the benchmark's links), forward links and the stored backward adjoints: 0.4 % escaped."""
    lat = [32, 32, 32, 32]
    lo = o.Layout(lat)
    rf = o.RngField(lo, o.RNG_MILC6, 987654321)
    g = o.gauge_random(lo, rf)
    o.rephase(lo, g)
    m = g.reshape(-1, 3, 3, 2)
    e1, _ = _check_roundtrip(m)
    e2, _ = _check_roundtrip(_adjoints(m))
    frac = np.concatenate([e1, e2]).mean()
    assert 0.003 < frac < 0.005, frac


def _su3(rng, n):
    z = rng.standard_normal((n, 3, 3)) + 1j * rng.standard_normal((n, 3, 3))
    qm, r = np.linalg.qr(z)
    qm = qm * (np.diagonal(r, axis1=1, axis2=2) / np.abs(np.diagonal(r, axis1=1, axis2=2)))[:, None, :]
    qm = qm / np.linalg.det(qm)[:, None, None] ** (1.0 / 3.0)
    return np.stack([qm.real, qm.imag], axis=-1)


def _rebuilt(m):
    """The decoder's rebuild of row 2 (what an escaped link decodes to: k = 0) -- force the escape with a huge defect."""
    big = m.copy()
    big[:, 2] += 1.0
    esc, row2 = q.link_residual_host(big)
    assert esc.all()
    return row2


def test_unitary_links_and_their_negatives_round_trip():
    rng = np.random.default_rng(1)
    m = _su3(rng, 4096)
    esc, _ = _check_roundtrip(m)
    assert esc.mean() < 0.01
    esc, _ = _check_roundtrip(-m)          # det -1: the sign bit
    assert esc.mean() < 0.01


@pytest.mark.parametrize("k,escaped", [(0, False), (1, False), (-1, False), (32767, False), (-32767, False), (32768, True),
                                       (-40000, True)])
def test_residual_range(k, escaped):
    rng = np.random.default_rng(2)
    m = _su3(rng, 256)
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


def test_edge_cases():
    rng = np.random.default_rng(3)
    base = _su3(rng, 8)
    cases = []
    cases.append(np.zeros((3, 3, 2)))                      # all zero: rebuild 0, row 2 0 -> exact
    z = base[0].copy(); z[2] = -0.0                        # rows 0,1 zero, row 2 -0.0: the rebuild gives +0 -> escaped
    z[:2] = 0.0; cases.append(z)
    s = np.zeros((3, 3, 2)); s[0, 0, 0] = 5e-320; s[1, 1, 0] = 1.0   # subnormal rebuild (no ulp scale): exact only if equal
    s[2, 2, 0] = 5e-320
    cases.append(s)
    s2 = s.copy(); s2[2, 2, 0] = np.nextafter(5e-320, 1.0)
    cases.append(s2)
    p2 = np.zeros((3, 3, 2)); p2[0, 0, 0] = 1.0; p2[1, 1, 0] = 1.0; p2[2, 2, 0] = 1.0            # identity: rebuild exactly 1
    cases.append(p2)
    p3 = p2.copy(); p3[2, 2, 0] = np.nextafter(1.0, 0.0)   # just below a power of two: other binade, half an ulp of 1
    cases.append(p3)
    p4 = p2.copy(); p4[2, 2, 0] = 1.0 + 2.0 ** -52         # one ulp above
    cases.append(p4)
    d = base[1].copy(); d[2, 1, 1] += 1e-6                 # large defect
    cases.append(d)
    n = base[2].copy(); n[2, 0, 0] = np.nan                # not a number
    cases.append(n)
    m = np.stack(cases)
    esc, _ = _check_roundtrip(m)
    assert list(esc) == [False, True, False, True, False, True, False, True, True], esc
