"""The 16-bit vector format of the SloppyHalf solves on the host (qexhip_half_pack_host / qexhip_half_unpack_host) against a
numpy restatement, bit for bit: six int16 and one fp32 norm per site, q = rint(v 32767 / norm).  No device needed."""
import numpy as np
import pytest

import qex_amd as q

FLT_MIN = np.finfo(np.float32).tiny


def pack_np(v):
    """the format in numpy: v (n, 6) float64 -> (q int16 (n, 6), norm float32 (n,)), double arithmetic"""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 6)
    norm = np.abs(v).max(axis=1).astype(np.float32)
    norm[norm < FLT_MIN] = 0.0
    s = np.zeros(len(v))
    nz = norm > 0
    s[nz] = 32767.0 / norm[nz].astype(np.float64)
    qq = np.clip(np.rint(v * s[:, None]), -32767.0, 32767.0)
    return qq.astype(np.int16), norm


def unpack_np(qq, norm):
    return qq.astype(np.float64) * (norm.astype(np.float64) / 32767.0)[:, None]


def _sites():
    rng = np.random.default_rng(20261019)
    gauss = rng.standard_normal((257, 6))
    zero = np.zeros((1, 6))
    one = np.zeros((6, 6))
    one[np.arange(6), np.arange(6)] = [1.0, -2.5, 3e-7, -4e5, 0.125, 1e-3]          # one nonzero component, each position
    span = rng.standard_normal((61, 6)) * 10.0 ** np.linspace(-30, 30, 61)[:, None]  # sites spanning 1e-30 .. 1e30
    return {"gauss": gauss, "zero": zero, "one": one, "span": span, "all": np.concatenate([gauss, zero, one, span])}


@pytest.mark.parametrize("kind", ["gauss", "zero", "one", "span", "all"])
def test_pack_matches_numpy_bit_for_bit(kind):
    v = _sites()[kind]
    qq, norm = q.half_pack_host(v.reshape(-1, 3, 2))
    qn, nn = pack_np(v)
    assert qq.dtype == np.int16 and norm.dtype == np.float32
    assert np.array_equal(qq, qn)
    assert np.array_equal(norm.view(np.uint32), nn.view(np.uint32))
    u = q.half_unpack_host(qq, norm).reshape(-1, 6)
    assert np.array_equal(u.view(np.uint64), unpack_np(qn, nn).view(np.uint64))
    if kind == "zero":
        assert not qq.any() and not norm.any() and not u.any()
    nz = norm > 0
    assert np.all(np.abs(qq[nz]).max(axis=1) == 32767)                       # the largest component takes the top of the range


@pytest.mark.parametrize("kind", ["gauss", "zero", "one", "span"])
def test_roundtrip_error_and_idempotence(kind):
    v = _sites()[kind]
    qq, norm = q.half_pack_host(v.reshape(-1, 3, 2))
    u = q.half_unpack_host(qq, norm).reshape(-1, 6)
    # half a step of norm / 32767 per component
    assert np.all(np.abs(u - v) <= norm.astype(np.float64)[:, None] / 65534.0)
    q2, n2 = q.half_pack_host(u.reshape(-1, 3, 2))
    assert np.array_equal(q2, qq) and np.array_equal(n2.view(np.uint32), norm.view(np.uint32))


def test_complex_input_and_tiny_sites():
    rng = np.random.default_rng(7)
    z = rng.standard_normal((5, 3)) + 1j * rng.standard_normal((5, 3))
    qa, na = q.half_pack_host(z)
    qb, nb = q.half_pack_host(np.stack([z.real, z.imag], axis=-1))
    assert np.array_equal(qa, qb) and np.array_equal(na, nb)
    # below the smallest normal fp32 number a site is stored as zero
    tiny = np.full((1, 3, 2), 1e-39)
    qt, nt = q.half_pack_host(tiny)
    assert not qt.any() and nt[0] == 0.0
    with pytest.raises(Exception):
        q.half_pack_host(np.full((1, 3, 2), 1e39))
