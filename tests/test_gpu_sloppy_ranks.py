"""Mixed-precision CG (SolverParams.sloppySolve) on t-sharded lattices: the fp32 face exchange, the halo form of the fp32 sweep and the
rank-global reductions of the reliable-update CG.

The ranks are started by torch.distributed.run as fresh processes that all bind GPU 0 and talk over the peer-memory transport
(tests/sloppy_rank_worker.py checks every rank's slab against a one-rank context of the whole lattice).  The one-rank halo path --
ghost zones filled by the periodic wrap, exchanges delayed by the transport emulation -- runs in this process.  Observed values are
printed (pytest -s)."""
import numpy as np
import pytest

from ranks import launch_ok

pytestmark = pytest.mark.gpu
SEED = 987654321


@pytest.mark.parametrize("nranks,lat", [(2, [8, 8, 8, 8]), (2, [16, 16, 16, 32]), (4, [8, 8, 8, 16])])
def test_sharded_fp32_operator_is_the_one_rank_operator_bit_for_bit(nranks, lat):
    """dev_op_xx_sloppy on every rank's slab == the slab of the one-rank dev_op_xx_sloppy (np.array_equal): g.random links (sign
    format), g.random + Naik (ghost depth 3), HISQ (18 reals); exchange-first, split by sites, and hop_split 2 (the fp32 sweep has no
    fused form and runs split by sites there: the worker counts its boundary launches)."""
    res = launch_ok(nranks, "sloppy_rank_worker.py", lat + ["--op"], "SLOPPY_RANKS_OK", 600, env={"QEXHIP_PEER_TIMEOUT": "60"})
    for r in res:
        assert len(r["op"]) == 9, r["op"].keys()
        assert r["op"]["random/fused_requested"]["launches"][1] == 4 and r["op"]["hisq/fused_requested"]["fmt"] == 0


@pytest.mark.parametrize("nranks,lat", [(2, [8, 8, 8, 8]), (4, [8, 8, 8, 16])])
def test_sharded_sloppy_solve_converges_on_the_true_residual(nranks, lat):
    """solveEE and solve (ReconL / ReconR) at r2req 1e-8 and 1e-14: true residual of the gathered solution <= r2req (oracle, fp64),
    the same iterations and reliable updates on every rank, within a few iterations of the one-rank sloppy solve."""
    res = launch_ok(nranks, "sloppy_rank_worker.py", lat + ["--solve"], "SLOPPY_RANKS_OK", 600, env={"QEXHIP_PEER_TIMEOUT": "60"})
    for key, v in res[0]["solve"].items():
        print(f"{nranks} ranks {lat} {key}: {v['its']} its / {v['nupd']} updates (one rank: {v['one_rank_its']} / {v['one_rank_nupd']}), "
              f"true r2/b2 {v['oracle_r2']:.2e}")
        assert all(r["solve"][key]["its"] == v["its"] and r["solve"][key]["nupd"] == v["nupd"] for r in res)


def _one_rank(o, lat, naik, halo, emu_us=0):
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
    return lo, ctx, s, b


def _op(ctx, b, m2, par_even):
    fx, fr = ctx.field_new(b), ctx.field_new()
    ctx.dev_op_xx_sloppy(fr, fx, m2, par_even)
    r = ctx.field_download(fr)
    ctx.field_free(fx)
    ctx.field_free(fr)
    return r


@pytest.mark.parametrize("naik", [False, True])
def test_one_rank_halo_path_is_bit_identical_under_delayed_exchanges(oracle, naik):
    """One rank with ghost zones (qexhip_comm_force_halo) and every exchange delayed by 40 us (emu_exchange_us): the fp32 operator
    gives the bits of the context without a halo in both sweep forms -- split by sites puts the boundary launch behind the delayed
    exchange on the comm stream --, and the exchange-first sloppy solve gives the no-halo solve's bits (solution, iterations,
    updates, residual).  Split by sites groups the <p,Ap> partials differently: that solve converges to the same residual."""
    import qex_amd as q

    o = oracle
    lat = [8, 8, 8, 8]
    lo, c0, s0, b = _one_rank(o, lat, naik, False)
    _, c1, s1, _ = _one_rank(o, lat, naik, True, emu_us=40)
    assert c1.sweep_info()["halo"] and not c0.sweep_info()["halo"]
    for overlap in (0, 1):
        c1.set_option("overlap", overlap)
        c1.timers_enable(3)
        c1.timers_reset()
        for pe, m2 in ((True, 0.01), (False, 0.04)):
            assert np.array_equal(_op(c1, b, m2, pe), _op(c0, b, m2, pe)), (overlap, pe)
        assert c1.timer("exchange")[0] == 4 and c1.timer("dslash_f32_bnd")[0] == (4 if overlap else 0)
        c1.timers_enable(0)
    mass = 0.1
    for r2req in (1e-8, 1e-14):
        sp0 = q.SolverParams(r2req=r2req, maxits=5000, verbosity=0, sloppySolve=q.SloppySingle)
        x0 = np.zeros_like(b)
        s0.solveEE(x0, b, mass, sp0)
        for overlap in (0, 1):
            c1.set_option("overlap", overlap)
            sp = q.SolverParams(r2req=r2req, maxits=5000, verbosity=0, sloppySolve=q.SloppySingle)
            x = np.zeros_like(b)
            s1.solveEE(x, b, mass, sp)
            print(f"one-rank halo naik={naik} overlap={overlap} r2req={r2req:g}: {sp.iterations} its / {sp.reliableUpdates} updates, "
                  f"r2 {sp.r2:.3e} (no halo: {sp0.iterations} / {sp0.reliableUpdates}, {sp0.r2:.3e})")
            if overlap == 0:
                assert np.array_equal(x, x0) and (sp.iterations, sp.reliableUpdates, sp.r2) == (sp0.iterations, sp0.reliableUpdates, sp0.r2)
            else:
                assert sp.r2 <= r2req and abs(sp.iterations - sp0.iterations) <= max(5, sp0.iterations // 20)
