"""The packed lossless link format (qex_amd/csrc/link_residual.h, 100 B per link, option lossless = 2) on the device: every result
must be BITWISE the one of the 18-real links (option lossless = 0) -- the format stores the same operator, not an approximation.

  D, stagD2ee / stagD2oo, stagD          8^4, 4.6.10.6 (a last tile with empty lanes) and 16^4 (128 workgroups: the XCD swizzle and
                                         the logical-block slot of the dot partials), QEX g.random, both parities
  CG (solveEE)                           16^4: residual history, solution and iteration count
  injected escapes                       a rows-0,1 entry outside the window escapes the link (read whole from the 18 reals) and keeps
                                         the bits; above 1 % escaped the choice falls to the 108-byte format under its own rule, then
                                         to 18 reals
  two ranks sharing one device           t-sharded, peer transport, the fused sweep forced (tests/lossless_rank_worker.py 2)
  lock-step batch                        solveXX_batch, 1..4 systems: it keeps reading the 18 reals, the results are those of lossless = 0
"""
import numpy as np
import pytest

from oracle import oracle as o
from lossless_links import OPS, _ctx, _gauge, _ops, _ref, two_ranks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("lat", [[8, 8, 8, 8], [4, 6, 10, 6], [16, 16, 16, 16]])
def test_operator_bitwise_equal_to_18_real_links(lat):
    lo, g, x = _gauge(lat)
    ref = _ref(lat)
    _, new = _ops(_ctx(lat), g, x, 2)
    assert ref["storage"] == (144, 0)
    assert new["storage"][0] == 100, new["storage"]
    # the values are the 18-real links: links_info keeps reporting format 0
    assert new["info"][1] == 0 and ref["info"][1] == 0
    nlinks = 2 * 4 * lo.vol
    print("escaped", new["storage"][1], "of", nlinks)
    assert 0 < new["storage"][1] <= 0.01 * nlinks, new["storage"]
    for k in OPS:
        assert np.array_equal(ref[k], new[k]), k
    # and they are the operator (not two identical wrong answers)
    assert np.linalg.norm(new["D"] - o.D(lo, g, None, x, 0.1)) / np.linalg.norm(new["D"]) < 1e-13


def test_cg_bitwise_equal_to_18_real_links_16x4():
    import qex_amd as q

    lat = [16, 16, 16, 16]
    _, g, b = _gauge(lat)
    ctx = _ctx(lat)
    res = {}
    for lossless in (0, 2):
        ctx.set_option("lossless", lossless)
        s = q.newStag(ctx, g)
        sp = q.SolverParams(r2req=1e-14, maxits=2000, verbosity=0)
        x = np.zeros_like(b)
        s.solveEE(x, b, 0.1, sp, histcap=4096)
        res[lossless] = (x.copy(), int(sp.iterations), np.array(sp.r2hist), s.links_storage()[0])
    assert res[0][3] == 144 and res[2][3] == 100
    assert res[0][1] == res[2][1] and res[2][1] > 100
    assert np.array_equal(res[0][2], res[2][2])
    assert np.array_equal(res[0][0], res[2][0])


def test_entries_outside_the_window_escape_and_keep_the_bits():
    lat = [8, 8, 8, 8]
    lo, g, x = _gauge(lat, seed=5)
    ctx = _ctx(lat)
    _, base = _ops(ctx, g, x, 2)
    rng = np.random.default_rng(3)
    g2 = g.copy()
    # one entry of rows 0,1 far below 2^-15 in 20 links (of 32768 stored): escaped, read whole from the 18 reals
    for _ in range(20):
        site, mu = int(rng.integers(lo.vol)), int(rng.integers(4))
        g2[site, mu, int(rng.integers(2)), int(rng.integers(3)), int(rng.integers(2))] = 1e-7
    _, ref = _ops(ctx, g2, x, 0)
    _, new = _ops(ctx, g2, x, 2)
    assert new["storage"][0] == 100
    # each changed link is stored twice (forward, and as the backward link of its neighbour)
    assert new["storage"][1] >= base["storage"][1] + 20, (new["storage"], base["storage"])
    assert new["info"][1] == 0
    for k in OPS:
        assert np.array_equal(ref[k], new[k]), k


def test_row_2_defects_above_one_percent_fall_back_to_18_reals():
    lat = [8, 8, 8, 8]
    lo, g, x = _gauge(lat, seed=5)
    ctx = _ctx(lat)
    rng = np.random.default_rng(4)
    g3 = g.copy()
    sel = rng.random((lo.vol, 4)) < 0.03
    g3[sel, 2] += 1e-7
    _, fb = _ops(ctx, g3, x, 2)
    assert fb["storage"][0] == 144 and fb["storage"][1] > 0.01 * 2 * 4 * lo.vol, fb["storage"]
    _, fb0 = _ops(ctx, g3, x, 0)
    for k in OPS:
        assert np.array_equal(fb[k], fb0[k]), k


def _unitary_with_small_entry(rng, n, eps):
    """n matrices unitary to rounding (Gram-Schmidt, row 2 = conj(row0 x row1)) whose entry [0][0] is about eps"""
    r0 = rng.standard_normal((n, 3)) + 1j * rng.standard_normal((n, 3))
    r0[:, 0] = 0.0
    r0 /= np.linalg.norm(r0, axis=1)[:, None]
    r0[:, 0] = eps
    r0 /= np.linalg.norm(r0, axis=1)[:, None]
    r1 = rng.standard_normal((n, 3)) + 1j * rng.standard_normal((n, 3))
    r1 -= np.sum(np.conj(r0) * r1, axis=1)[:, None] * r0
    r1 /= np.linalg.norm(r1, axis=1)[:, None]
    r2 = np.conj(np.cross(r0, r1))
    m = np.stack([r0, r1, r2], axis=1)
    return np.stack([m.real, m.imag], axis=-1)


def test_packed_above_one_percent_lands_on_the_108_byte_format():
    """3 % of the links unitary with an entry of 1e-6 in rows 0,1 (theirs and their adjoints'): the packed form escapes them, the
    int16 rule does not."""
    import qex_amd as q

    lat = [8, 8, 8, 8]
    lo, g, x = _gauge(lat, seed=5)
    ctx = _ctx(lat)
    rng = np.random.default_rng(5)
    g4 = g.copy()
    sel = rng.random((lo.vol, 4)) < 0.03
    g4[sel] = _unitary_with_small_entry(rng, int(sel.sum()), 1e-6)
    # the case is what it is meant to be: on the host, forward links and the stored adjoints
    m = g4.reshape(-1, 3, 3, 2)
    both = np.concatenate([m, np.ascontiguousarray(np.swapaxes(m, 1, 2) * np.array([1.0, -1.0]))])
    pk = q.link_packed_host(both)[0]
    rs = q.link_residual_host(both)[0]
    msel = np.concatenate([sel.reshape(-1), sel.reshape(-1)])
    assert pk[msel].all() and not rs[msel].any()
    assert pk.mean() > 0.01 and rs.mean() <= 0.01, (pk.mean(), rs.mean())
    _, ref = _ops(ctx, g4, x, 0)
    _, new = _ops(ctx, g4, x, 2)
    assert new["storage"][0] == 108, new["storage"]
    assert 0 < new["storage"][1] <= 0.01 * 2 * 4 * lo.vol, new["storage"]
    for k in OPS:
        assert np.array_equal(ref[k], new[k]), k


def test_two_ranks_sharing_one_device_fused_sweep():
    ok = two_ranks(2)
    for r in ok:
        assert r["form"] == 2 and r["storage"][0] == 100 and r["storage_ref"][0] == 144, r
        assert r["equal"] == {"D": True, "stagD2ee": True, "hist": True, "x": True, "its": True}, r


@pytest.mark.parametrize("lat", [[8, 8, 8, 8], [4, 6, 10, 6]])
def test_lock_step_batch_bitwise_equal_to_18_real_links(lat):
    """solveXX_batch with 1..4 systems, both parities: the fp64 lock-step batch reads the 18 reals kept beside the packed rows, so
    every system's solution, iteration count and final residual are those of lossless = 0."""
    import qex_amd as q

    lo, g, b0 = _gauge(lat)
    ctx = _ctx(lat)
    rng = np.random.default_rng(11)
    bs = [b0] + [rng.standard_normal(b0.shape) for _ in range(3)]
    ms = [0.1, 0.2, 0.4, 0.05]
    res = {}
    for lossless in (0, 2):
        ctx.set_option("lossless", lossless)
        s = q.newStag(ctx, g)
        out = [s.links_storage()[0]]
        for n in (1, 2, 3, 4):
            for par_even in (True, False):
                xs = [np.zeros_like(b) for b in bs[:n]]
                its, fin = s.solveXX_batch(xs, bs[:n], ms[:n], 1e-14, 300, par_even)
                out.append((list(its), list(fin), xs))
        res[lossless] = out
    assert res[0][0] == 144 and res[2][0] == 100
    for (i0, f0, x0), (i2, f2, x2) in zip(res[0][1:], res[2][1:]):
        assert i0 == i2 and min(i2) > 10, (i0, i2)
        assert f0 == f2, (f0, f2)
        for a, c in zip(x0, x2):
            assert np.array_equal(a, c)
