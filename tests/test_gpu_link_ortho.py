"""The orthogonal lossless link format (qex_amd/csrc/link_residual.h, 92 B per link, option lossless = 3) on the device: every
result must be BITWISE the one of the 18-real links (option lossless = 0) -- the format stores the same operator, not an
approximation.

  D, stagD2ee / stagD2oo, stagD          8^4, 4.6.10.6 (a last tile with empty lanes) and 16^4 (128 workgroups: the XCD swizzle and
                                         the logical-block slot of the dot partials), QEX g.random, both parities; the device's
                                         escape count is the host encoder's
  CG (solveEE)                           16^4: residual history, solution and iteration count
  injected escapes                       a stored entry outside the window escapes the link (read whole from the 18 reals) and keeps
                                         the bits; above 1 % escaped the choice falls to the packed 100-byte form under its own rule,
                                         and on to 18 reals
  two ranks sharing one device           t-sharded, peer transport, the fused sweep forced (tests/lossless_rank_worker.py 3)
"""
import numpy as np
import pytest

from oracle import oracle as o
from lossless_links import OPS, _ctx, _gauge, _ops, _ref, _stored, two_ranks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("lat", [[8, 8, 8, 8], [4, 6, 10, 6], [16, 16, 16, 16]])
def test_operator_bitwise_equal_to_18_real_links(lat):
    import qex_amd as q

    lo, g, x = _gauge(lat)
    ref = _ref(lat)
    _, new = _ops(_ctx(lat), g, x, 3)
    assert ref["storage"] == (144, 0)
    assert new["storage"][0] == 92, new["storage"]
    # the values are the 18-real links: links_info keeps reporting format 0
    assert new["info"][1] == 0 and ref["info"][1] == 0
    nlinks = 2 * 4 * lo.vol
    host = int(q.link_ortho_host(_stored(g))[0].sum())
    print("escaped", new["storage"][1], "of", nlinks, "host encoder", host)
    assert 0 < new["storage"][1] <= 0.01 * nlinks, new["storage"]
    assert new["storage"][1] == host, (new["storage"], host)
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
    for lossless in (0, 3):
        ctx.set_option("lossless", lossless)
        s = q.newStag(ctx, g)
        sp = q.SolverParams(r2req=1e-14, maxits=2000, verbosity=0)
        x = np.zeros_like(b)
        s.solveEE(x, b, 0.1, sp, histcap=4096)
        res[lossless] = (x.copy(), int(sp.iterations), np.array(sp.r2hist), s.links_storage()[0])
    assert res[0][3] == 144 and res[3][3] == 92
    assert res[0][1] == res[3][1] and res[3][1] > 100
    assert np.array_equal(res[0][2], res[3][2])
    assert np.array_equal(res[0][0], res[3][0])


def test_entries_outside_the_window_escape_and_keep_the_bits():
    lat = [8, 8, 8, 8]
    lo, g, x = _gauge(lat, seed=5)
    ctx = _ctx(lat)
    _, base = _ops(ctx, g, x, 3)
    rng = np.random.default_rng(3)
    g2 = g.copy()
    # one entry of the first two rows AND columns (stored by the link and by its adjoint) far below 2^-15 in 20 links (of 32768
    # stored): escaped, read whole from the 18 reals
    for _ in range(20):
        site, mu = int(rng.integers(lo.vol)), int(rng.integers(4))
        g2[site, mu, int(rng.integers(2)), int(rng.integers(2)), int(rng.integers(2))] = 1e-7
    _, ref = _ops(ctx, g2, x, 0)
    _, new = _ops(ctx, g2, x, 3)
    assert new["storage"][0] == 92
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
    _, fb = _ops(ctx, g3, x, 3)
    assert fb["storage"][0] == 144 and fb["storage"][1] > 0.01 * 2 * 4 * lo.vol, fb["storage"]
    _, fb0 = _ops(ctx, g3, x, 0)
    for k in OPS:
        assert np.array_equal(fb[k], fb0[k]), k


def test_ortho_above_one_percent_lands_on_the_100_byte_format():
    """1.2 % of the links with b2 moved by 1e-7 and row 2 made conj(row0 x row1) of the moved rows: rows 0,1 are no longer orthogonal
    (the orthogonal form escapes the link, and its adjoint, whose rows are the columns), row 2 still is its rebuild (the packed form
    keeps the forward link and escapes only the adjoint)."""
    import qex_amd as q

    lat = [8, 8, 8, 8]
    lo, g, x = _gauge(lat, seed=5)
    ctx = _ctx(lat)
    rng = np.random.default_rng(5)
    g4 = g.copy()
    sel = rng.random((lo.vol, 4)) < 0.012
    m = g4[sel]
    m[:, 1, 2] += 1e-7
    c = m[..., 0] + 1j * m[..., 1]
    r2 = np.conj(np.cross(c[:, 0], c[:, 1]))
    m[:, 2] = np.stack([r2.real, r2.imag], axis=-1)
    g4[sel] = m
    # the case is what it is meant to be: on the host, forward links and the stored adjoints
    both = _stored(g4)
    ot = q.link_ortho_host(both)[0]
    pk = q.link_packed_host(both)[0]
    msel = np.concatenate([sel.reshape(-1), sel.reshape(-1)])
    assert ot[msel].all()
    assert ot.mean() > 0.01 and pk.mean() <= 0.01, (ot.mean(), pk.mean())
    _, ref = _ops(ctx, g4, x, 0)
    _, new = _ops(ctx, g4, x, 3)
    assert new["storage"] == (100, int(pk.sum())), (new["storage"], pk.sum())
    for k in OPS:
        assert np.array_equal(ref[k], new[k]), k


def test_two_ranks_sharing_one_device_fused_sweep():
    ok = two_ranks(3)
    for r in ok:
        assert r["form"] == 2 and r["storage"][0] == 92 and r["storage_ref"][0] == 144, r
        assert r["equal"] == {"D": True, "stagD2ee": True, "hist": True, "x": True, "its": True}, r
