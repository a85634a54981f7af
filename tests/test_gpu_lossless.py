"""The lossless 108-byte link format (qex_amd/csrc/link_residual.h) on the device: every result must be BITWISE the one of the
18-real links (option lossless = 0) -- the format stores the same operator, not an approximation of it.

  D, stagD2ee / stagD2oo                 8^4 and 32^4 QEX g.random, both parities
  CG (solveEE)                           32^4: residual history, solution and iteration count; the history checks the sweeps'
                                         DOT partial sums (<p, Ap> of every iteration comes from them)
  two ranks sharing one device           t-sharded, peer transport, the fused sweep forced (tests/lossless_rank_worker.py 1)
  injected defects                       escaped links (row 2 read from the 18 reals) keep the bits; above 1 % escaped the choice
                                         falls back to 18 reals
"""
import numpy as np
import pytest

from oracle import oracle as o
from lossless_links import _gauge, _ops, two_ranks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("lat", [[8, 8, 8, 8], [32, 32, 32, 32]])
def test_operator_bitwise_equal_to_18_real_links(lat):
    import qex_amd as q

    lo, g, x = _gauge(lat)
    ctx = q.Context(lat)
    _, ref = _ops(ctx, g, x, 0)
    _, new = _ops(ctx, g, x, 1)
    assert ref["storage"][0] == 144 and ref["storage"][1] == 0
    assert new["storage"][0] == 108, new["storage"]
    # the values are the 18-real links: links_info keeps reporting format 0
    assert new["info"][1] == 0 and ref["info"][1] == 0
    nlinks = 2 * 4 * lo.vol
    assert 0 < new["storage"][1] <= 0.01 * nlinks, new["storage"]
    for k in ("D", "stagD2ee", "stagD2oo", "stagD_even", "stagD_odd"):
        assert np.array_equal(ref[k], new[k]), k
    # and they are the operator (not two identical wrong answers)
    assert np.linalg.norm(new["D"] - o.D(lo, g, None, x, 0.1)) / np.linalg.norm(new["D"]) < 1e-13


def test_cg_bitwise_equal_to_18_real_links_32x4():
    import qex_amd as q

    lat = [32, 32, 32, 32]
    _, g, b = _gauge(lat)
    ctx = q.Context(lat)
    res = {}
    for lossless in (0, 1):
        ctx.set_option("lossless", lossless)
        s = q.newStag(ctx, g)
        sp = q.SolverParams(r2req=1e-14, maxits=2000, verbosity=0)
        x = np.zeros_like(b)
        s.solveEE(x, b, 0.1, sp, histcap=4096)
        res[lossless] = (x.copy(), int(sp.iterations), np.array(sp.r2hist), s.links_storage()[0])
    assert res[0][3] == 144 and res[1][3] == 108
    assert res[0][1] == res[1][1] and res[1][1] > 100
    assert np.array_equal(res[0][2], res[1][2])
    assert np.array_equal(res[0][0], res[1][0])


def test_injected_defects_escape_and_keep_the_bits():
    import qex_amd as q

    lat = [8, 8, 8, 8]
    lo, g, x = _gauge(lat, seed=5)
    ctx = q.Context(lat)
    _, base = _ops(ctx, g, x, 1)
    rng = np.random.default_rng(3)
    g2 = g.copy()
    # defects far beyond 32767 ulp of row 2 in 20 links (of 32768 stored): escaped, read from the 18 reals
    for _ in range(20):
        site, mu = int(rng.integers(lo.vol)), int(rng.integers(4))
        g2[site, mu, 2] += 1e-7 * rng.standard_normal((3, 2))
    _, ref = _ops(ctx, g2, x, 0)
    _, new = _ops(ctx, g2, x, 1)
    assert new["storage"][0] == 108
    # each defective link is stored twice (forward, and as the backward link of its neighbour)
    assert new["storage"][1] >= base["storage"][1] + 20, (new["storage"], base["storage"])
    assert new["info"][1] == 0
    for k in ("D", "stagD2ee", "stagD2oo", "stagD_even", "stagD_odd"):
        assert np.array_equal(ref[k], new[k]), k
    # more than 1 % of the links escaped: 18 reals
    g3 = g.copy()
    sel = rng.random((lo.vol, 4)) < 0.03
    g3[sel, 2] += 1e-7
    _, fb = _ops(ctx, g3, x, 1)
    assert fb["storage"][0] == 144 and fb["storage"][1] > 0.01 * 2 * 4 * lo.vol, fb["storage"]
    _, fb0 = _ops(ctx, g3, x, 0)
    assert np.array_equal(fb["D"], fb0["D"])


def test_recon_0_keeps_the_format_off_and_compressible_links_keep_theirs():
    import qex_amd as q

    lat = [8, 8, 8, 8]
    lo = o.Layout(lat)
    rf = o.RngField(lo, o.RNG_MILC6, 5)
    gw = o.gauge_warm(lo, 0.5, rf)
    o.rephase(lo, gw)
    _, g, x = _gauge(lat)
    ctx = q.Context(lat)
    ctx.set_option("recon", 0)
    s = q.newStag(ctx, g)
    assert s.links_storage() == (144, 0)
    ctx.set_option("recon", 2)
    # exactly unitary links: format 1 as before (96 B), the residual format is not tried
    s = q.newStag(ctx, gw)
    assert s.links_info()[1] == 1 and s.links_storage() == (96, 0)


def test_two_ranks_sharing_one_device_fused_sweep():
    ok = two_ranks(1)
    for r in ok:
        assert r["form"] == 2 and r["storage"][0] == 108 and r["storage_ref"][0] == 144, r
        assert r["equal"] == {"D": True, "stagD2ee": True, "hist": True, "x": True, "its": True}, r
