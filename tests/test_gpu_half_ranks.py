"""SloppyHalf on 16-bit storage (option "half" = 1) on t-sharded lattices: the 16-bit face exchange (16 B per site), the halo form of
the 16-bit sweep, the rank-global link scales and the rank-global reductions and stall guard of the 16-bit reliable-update CG.

The ranks are started by torch.distributed.run as fresh processes that all bind GPU 0 and talk over the peer-memory transport
(tests/half_rank_worker.py checks every rank's slab against a one-rank context of the whole lattice with "half" = 1; operator and
solve checks share ONE launch per shape).  The one-rank halo path -- ghost zones filled by the periodic wrap, exchanges delayed by the
transport emulation -- runs in this process.  Observed values are printed (pytest -s).

The iteration margin.  A sharded solve sums the <p,Ap> and |r_s|^2 partials in another grouping than the one-rank solve, so its
iteration count may differ.  The margin is the fp32 sharded test's, max(5, its // 20), after this check of it: the CPU model
tests/sloppy_ref.py with half=True on 8^4 (g.random, m = 0.1, sloppy_check 4), run with its dot products formed from 256-site partials
summed as one group, as two groups and as four groups (the ranks' sums, then their sum), took 132 / 132 / 132 iterations and 4 updates
to r2req 1e-8 and 224 / 224 / 224 iterations and 7 updates to 1e-14: an observed difference of 0, inside the margin of 6 and 11, so
the margin stands as it is."""
import numpy as np
import pytest

from half_rank_worker import margin
from ranks import launch_ok

pytestmark = pytest.mark.gpu
SEED = 987654321


@pytest.mark.parametrize("nranks,lat", [(2, [8, 8, 8, 8]), (2, [8, 8, 8, 16]), (4, [8, 8, 8, 16])])
def test_sharded_half_operator_and_solve_against_one_rank(nranks, lat):
    """2 ranks x 8^4: local Lt = 4, the Naik slab has no interior and runs one launch whatever `overlap` says; 2 ranks x 8.8.8.16: local
    Lt = 8, the split form runs all three site ranges, upper == lower; 4 ranks x 8.8.8.16: upper and lower are distinct processes.
    Operator: dev_op_xx_half on every slab == the slab of the one-rank dev_op_xx_half (np.array_equal) and links_info_half == the
    one-rank (format, s_fat, s_long) for g.random, g.random + Naik and HISQ links in the three sweep forms.  Solve: see the worker."""
    res = launch_ok(nranks, "half_rank_worker.py", lat + ["--op", "--solve"], "HALF_RANKS_OK", 600, env={"QEXHIP_PEER_TIMEOUT": "60"})
    for r in res:
        assert len(r["op"]) == 9, r["op"].keys()
        assert r["op"]["random/fused_requested"]["launches"][1] == 4 and r["op"]["hisq/fused_requested"]["fmt"] == 0
        assert len(r["solve"]) == 8, r["solve"].keys()
    # HISQ: the scales are whole-lattice maxima, the same on every rank
    assert len({(r["op"]["hisq/by_sites"]["s_fat"], r["op"]["hisq/by_sites"]["s_long"]) for r in res}) == 1
    for key, v in res[0]["solve"].items():
        print(f"{nranks} ranks {lat} {key}: {v['its']} its / {v['nupd']} updates (one rank: {v.get('one_rank_its')} / "
              f"{v.get('one_rank_nupd')}), true r2/b2 {v['oracle_r2']:.2e}, last {v['last']}")
        assert all(r["solve"][key]["its"] == v["its"] and r["solve"][key]["last"] == v["last"] for r in res)


def _one_rank(o, lat, naik, halo, half, emu_us=0):
    import qex_amd as q

    lo = o.Layout(lat)
    rf = o.RngField(lo, o.RNG_MILC6, SEED)
    fat = o.gauge_random(lo, rf)
    o.rephase(lo, fat)
    lng = o.gauge_random(lo, rf)
    o.rephase(lo, lng)
    b = o.vector_gaussian(lo, rf)
    ctx = q.Context(lat)
    if halo:
        ctx.force_halo(True)
        ctx.set_option("emu_exchange_us", emu_us)
    s = q.newStag3(ctx, fat, lng) if naik else q.newStag(ctx, fat)
    ctx.set_option("half", half)
    return lo, ctx, s, b


def _op(ctx, b, m2, par_even):
    fx, fr = ctx.field_new(b), ctx.field_new()
    ctx.dev_op_xx_half(fr, fx, m2, par_even)
    r = ctx.field_download(fr)
    ctx.field_free(fx)
    ctx.field_free(fr)
    return r


@pytest.mark.parametrize("naik", [False, True])
def test_one_rank_halo_half_is_bit_identical_under_delayed_exchanges(oracle, naik):
    """One rank with ghost zones (force_halo), every exchange delayed by 40 us, "half" = 1: the 16-bit operator gives the bits of the
    context without a halo in both sweep forms, and the exchange-first SloppyHalf solve gives the no-halo solve's bits (solution,
    iterations, updates, r2, sloppy_last).  Split by sites groups the <p,Ap> partials differently: that solve converges within the
    margin."""
    import qex_amd as q

    o = oracle
    lat = [8, 8, 8, 8]
    lo, c0, s0, b = _one_rank(o, lat, naik, False, 1)
    _, c1, s1, _ = _one_rank(o, lat, naik, True, 1, emu_us=40)
    assert c1.sweep_info()["halo"] and not c0.sweep_info()["halo"]
    assert c1.links_info_half() == c0.links_info_half()
    for overlap in (0, 1):
        c1.set_option("overlap", overlap)
        c1.timers_enable(3)
        c1.timers_reset()
        for pe, m2 in ((True, 0.01), (False, 0.04)):
            assert np.array_equal(_op(c1, b, m2, pe), _op(c0, b, m2, pe)), (overlap, pe)
        assert c1.timer("exchange")[0] == 4 and c1.timer("dslash_half")[0] == 4 and c1.timer("dslash_half_bnd")[0] == (4 if overlap else 0)
        c1.timers_enable(0)
    mass = 0.1
    for r2req in (1e-8, 1e-14):
        sp0 = q.SolverParams(r2req=r2req, maxits=5000, verbosity=0, sloppySolve=q.SloppyHalf)
        x0 = np.zeros_like(b)
        s0.solveEE(x0, b, mass, sp0)
        last0 = c0.sloppy_last()
        assert last0["precision"] == 2
        for overlap in (0, 1):
            c1.set_option("overlap", overlap)
            sp = q.SolverParams(r2req=r2req, maxits=5000, verbosity=0, sloppySolve=q.SloppyHalf)
            x = np.zeros_like(b)
            s1.solveEE(x, b, mass, sp)
            last = c1.sloppy_last()
            print(f"one-rank halo half naik={naik} overlap={overlap} r2req={r2req:g}: {sp.iterations} its / {sp.reliableUpdates} updates, "
                  f"r2 {sp.r2:.3e}, last {last} (no halo: {sp0.iterations} / {sp0.reliableUpdates}, {sp0.r2:.3e})")
            assert last["precision"] == 2 and last["half_iters"] > 0
            if overlap == 0:
                assert np.array_equal(x, x0)
                assert (sp.iterations, sp.reliableUpdates, sp.r2, last) == (sp0.iterations, sp0.reliableUpdates, sp0.r2, last0)
            else:
                assert sp.r2 <= r2req and abs(sp.iterations - sp0.iterations) <= margin(sp0.iterations)


def test_one_rank_halo_half_option_off_runs_single(oracle):
    """ "half" = 0 on the halo context: SloppyHalf gives the bits of SloppySingle."""
    import qex_amd as q

    _, c1, s1, b = _one_rank(oracle, [8, 8, 8, 8], False, True, 0, emu_us=40)
    out = []
    for mode in (q.SloppyHalf, q.SloppySingle):
        sp = q.SolverParams(r2req=1e-14, maxits=5000, verbosity=0, sloppySolve=mode)
        x = np.zeros_like(b)
        s1.solveEE(x, b, 0.1, sp)
        out.append((x, sp.iterations, sp.reliableUpdates, sp.r2))
        assert c1.sloppy_last()["precision"] == 1
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1:] == out[1][1:]
