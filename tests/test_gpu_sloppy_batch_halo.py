"""Mixed-precision lock-step batches on a one-rank context with ghost zones in t (force_halo) under option "batch_ranks" = 1: the HALO
form of the lock-step sweep, all systems' faces in one exchange (here the periodic wrap, delayed by the transport emulation), and the
option's handling.  The sharded runs are tests/test_gpu_sloppy_batch_ranks.py.  Observed values are printed (pytest -s).

What is compared is bits: a system solved in a batch returns what it returns alone, and exchange-first keeps the one-rank workgroup
partition, so there the batch on the halo context returns what the batch on the context without a halo returns."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = 987654321
LAT = [8, 8, 8, 8]
MS = [0.1, 0.2, 0.05]
R2 = [1e-8, 1e-14, 1e-10]


def _ctx(o, naik, halo):
    import qex_amd as q

    lo = o.Layout(LAT)
    rf = o.RngField(lo, o.RNG_MILC6, SEED)
    fat = o.gauge_random(lo, rf)
    o.rephase(lo, fat)
    lng = o.gauge_random(lo, rf)
    o.rephase(lo, lng)
    bs = [o.vector_gaussian(lo, rf) for _ in MS]
    ctx = q.Context(LAT)
    if halo:
        ctx.force_halo(True)
        ctx.set_option("emu_exchange_us", 40)
    s = q.newStag3(ctx, fat, lng) if naik else q.newStag(ctx, fat)
    ctx.set_option("half", 1)
    ctx.set_option("half_batch", 1)
    return ctx, s, bs


def _batch(ctx, s, bs, sloppy):
    xs = [np.zeros_like(b) for b in bs]
    its, fin, nup = s.solveXX_batch(xs, bs, MS, R2, 5000, True, sloppy=sloppy)
    return xs, its, fin, nup, ctx.sloppy_last_batch()


def _single(ctx, b, m, r2req, sloppy):
    fb, fx = ctx.field_new(b), ctx.field_new()
    its, fin, nup = ctx.dev_solve_xx_sloppy(fx, fb, m, r2req, 5000, True, sloppy)
    x = ctx.field_download(fx)
    ctx.field_free(fb)
    ctx.field_free(fx)
    return x, its, fin, nup, ctx.sloppy_last()


@pytest.mark.parametrize("sloppy", [1, 2])
@pytest.mark.parametrize("naik", [False, True])
def test_one_rank_halo_batch_bits(oracle, naik, sloppy):
    """overlap 0: the bits of the batch without a halo (x, iterations, r2, updates, sloppy_last_batch); overlap 1 (split by sites): the
    bits of the single-system solves on the same halo context with overlap 1.  fp32 and 16-bit."""
    c0, s0, bs = _ctx(oracle, naik, False)
    c1, s1, _ = _ctx(oracle, naik, True)
    c1.set_option("batch_ranks", 1)
    assert c1.sweep_info()["halo"] and not c0.sweep_info()["halo"]
    want = _batch(c0, s0, bs, sloppy)
    assert all(l["precision"] == sloppy for l in want[4]), want[4]
    c1.set_option("overlap", 0)
    c1.timers_enable(3)
    c1.timers_reset()
    got = _batch(c1, s1, bs, sloppy)
    tb = "dslash_batch_half" if sloppy == 2 else "dslash_batch_f32"
    nsweep, nbnd = c1.timer(tb)[0], c1.timer(tb + "_bnd")[0]
    c1.timers_enable(0)
    print(f"halo batch naik={naik} sloppy={sloppy} overlap=0: its {got[1]} updates {got[3]} r2 {got[2]} last {got[4]}; "
          f"{nsweep} sweeps, {nbnd} boundary launches")
    assert nsweep > 0 and nbnd == 0
    assert got[1:] == want[1:], (got[1:], want[1:])
    for j in range(len(MS)):
        assert np.array_equal(got[0][j], want[0][j]), j
    c1.set_option("overlap", 1)
    assert c1.sweep_info()["overlap"] == 1
    c1.timers_enable(3)
    c1.timers_reset()
    got = _batch(c1, s1, bs, sloppy)
    nsweep, nbnd = c1.timer(tb)[0], c1.timer(tb + "_bnd")[0]
    c1.timers_enable(0)
    assert nbnd == nsweep > 0, (nsweep, nbnd)
    for j in range(len(MS)):
        x, its, fin, nup, last = _single(c1, bs[j], MS[j], R2[j], sloppy)
        print(f"halo batch naik={naik} sloppy={sloppy} overlap=1 system {j}: its {got[1][j]} updates {got[3][j]} r2 {got[2][j]:.3e} "
              f"(alone: {its} / {nup} / {fin:.3e}) last {got[4][j]}")
        assert (got[1][j], got[2][j], got[3][j], got[4][j]) == (its, fin, nup, last)
        assert np.array_equal(got[0][j], x), j
        assert fin <= R2[j]
    c0.close()
    c1.close()


def _raw(L, ctx, which, xs, bs, ids, sloppy=1):
    n = len(xs)
    xp = (C.c_void_p * n)(*[a.ctypes.data for a in xs])
    bp = (C.c_void_p * n)(*[a.ctypes.data for a in bs])
    mv, rv = (C.c_double * n)(*MS[:n]), (C.c_double * n)(*R2[:n])
    its, fin, nup = (C.c_int * n)(), (C.c_double * n)(), (C.c_int * n)()
    if which == "xx":
        return L.qexhip_stag_solve_xx_batch_sloppy(ctx._h, n, xp, bp, mv, rv, 100, 1, sloppy, its, fin, nup)
    if which == "full":
        return L.qexhip_stag_solve_batch_sloppy(ctx._h, n, xp, bp, mv, rv, 100, sloppy, its, fin, nup)
    xi, bi = (C.c_int * n)(*ids[0]), (C.c_int * n)(*ids[1])
    return L.qexhip_dev_solve_batch_sloppy(ctx._h, n, xi, bi, mv, rv, 100, sloppy, its, fin, nup)


def test_option_handling(oracle):
    """batch_ranks = 0 (the default) on a halo context: the three entries return -1 with "shard" in the message and write nothing, and the
    batched probes refuse; batch_ranks = 1: they run; values other than 0 and 1 are refused."""
    from qex_amd._lib import lib

    L = lib()
    ctx, s, bs = _ctx(oracle, False, True)
    bs = bs[:2]
    ids = ([ctx.field_new() for _ in bs], [ctx.field_new(b) for b in bs])
    for v in (2, -1):
        with pytest.raises(Exception):
            ctx.set_option("batch_ranks", v)
    for which in ("xx", "full", "dev"):
        xs = [np.full_like(b, 3.0) for b in bs]
        rc = _raw(L, ctx, which, xs, bs, ids)
        msg = L.qexhip_last_error().decode()
        assert rc == -1 and "shard" in msg, (which, rc, msg)
        assert all((x == 3.0).all() for x in xs)
    for probe in (ctx.dev_op_xx_half_batch, ctx.dev_op_xx_sloppy_batch):
        with pytest.raises(Exception):
            probe(ids[0], ids[1], [0.01, 0.04])
    ctx.set_option("batch_ranks", 1)
    for which in ("xx", "full", "dev"):
        xs = [np.full_like(b, 3.0) for b in bs]
        assert _raw(L, ctx, which, xs, bs, ids) == 0, (which, L.qexhip_last_error())
        assert which == "dev" or not any((x == 3.0).all() for x in xs)
    ctx.set_option("batch_ranks", 0)
    assert _raw(L, ctx, "xx", [np.zeros_like(b) for b in bs], bs, ids) == -1
    ctx.close()


@pytest.mark.parametrize("naik", [False, True])
def test_one_rank_halo_batched_probes(oracle, naik):
    """both batched operator probes on the halo context, overlap 0 and 1: every system equals the single-system probe on the context
    without a halo, bit for bit; one exchange per sweep (two per application, not 2 n)"""
    c0, s0, bs = _ctx(oracle, naik, False)
    c1, s1, _ = _ctx(oracle, naik, True)
    c1.set_option("batch_ranks", 1)
    m2 = [0.01, 0.04, 0.0025]
    for single, batch in ((c0.dev_op_xx_sloppy, c1.dev_op_xx_sloppy_batch), (c0.dev_op_xx_half, c1.dev_op_xx_half_batch)):
        for pe in (True, False):
            want = []
            for b, m in zip(bs, m2):
                fx, fr = c0.field_new(b), c0.field_new()
                single(fr, fx, m, pe)
                want.append(c0.field_download(fr))
                c0.field_free(fx)
                c0.field_free(fr)
            for overlap in (0, 1):
                c1.set_option("overlap", overlap)
                fx, fr = [c1.field_new(b) for b in bs], [c1.field_new() for _ in bs]
                c1.timers_enable(3)
                c1.timers_reset()
                batch(fr, fx, m2, pe)
                c1.sync()
                assert c1.timer("exchange")[0] == 2
                c1.timers_enable(0)
                for j, f in enumerate(fr):
                    assert np.array_equal(c1.field_download(f), want[j]), (pe, overlap, j)
                for f in fx + fr:
                    c1.field_free(f)
    c0.close()
    c1.close()


@pytest.mark.parametrize("transport", ["rccl", "rccl+mbox"])
def test_one_rank_communicator_paths(oracle, transport):
    """What a rank of a job on distinct GPUs executes, on one GPU (as test_gpu_parity.py::test_multi_rank_code_path_on_one_rank): a
    ONE-RANK RCCL communicator carries all systems' faces in one group (ncclSend / ncclRecv to self) and, with option "multi_reduce",
    the partial sums of all systems go through one all-reduce per reduction point -- RCCL's over the partial vectors, or with rccl+mbox
    the mailbox kernel with the deferred join in its prologue.  Split by sites, fp32 and 16-bit: every system's bits are those of its
    single-system solve on the same context."""
    import qex_amd as q

    lo = oracle.Layout(LAT)
    rf = oracle.RngField(lo, oracle.RNG_MILC6, SEED)
    fat = oracle.gauge_random(lo, rf)
    oracle.rephase(lo, fat)
    bs = [oracle.vector_gaussian(lo, rf) for _ in MS]
    ctx = q.Context(LAT)
    if transport == "rccl+mbox":
        ctx.set_option("transport", 3)
    ctx.comm_init(q.Context.unique_id(), 1, 0)
    assert ctx.comm_transport()[0] == transport
    ctx.force_halo(True)
    ctx.set_option("overlap", 1)
    ctx.set_option("multi_reduce", 1)
    for name in ("half", "half_batch", "batch_ranks"):
        ctx.set_option(name, 1)
    s = q.newStag(ctx, fat)
    for sloppy in (1, 2):
        ctx.timers_enable(3)
        ctx.timers_reset()
        got = _batch(ctx, s, bs, sloppy)
        nred = ctx.timer("allreduce")[0]
        ctx.timers_enable(0)
        assert nred > 0
        for j in range(len(MS)):
            x, its, fin, nup, last = _single(ctx, bs[j], MS[j], R2[j], sloppy)
            print(f"{transport} sloppy={sloppy} system {j}: its {got[1][j]} updates {got[3][j]} r2 {got[2][j]:.3e} (alone: {its} / {nup} / {fin:.3e})")
            assert (got[1][j], got[2][j], got[3][j], got[4][j]) == (its, fin, nup, last)
            assert np.array_equal(got[0][j], x), j
            assert fin <= R2[j]
    ctx.close()
