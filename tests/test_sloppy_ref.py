"""The numpy model of the mixed-precision CG iterations (tests/sloppy_ref.py) tested on the CPU: with float64 storage and the updates
switched off it IS the oracle's CG and multi-shift CG; a solve cut at maxits = k is what the one-pass ladder forks at k; the
sensitivity ensemble leaves the update schedule alone, far from every threshold; and each wrong-logic variant of the iteration --
the defects tests/test_gpu_sloppy_steps.py exists to catch -- leaves the unperturbed model by at least 100 x the tolerance
(8 sens_k) that module allows the library, on both lattices.  No device needed.

Measured (8^4 and 4.6.10.6, m = 0.5, sloppy_check 4, K = 24): see the table in DESIGN.md "Engineering checks"."""
import numpy as np
import pytest

import sloppy_ref as R

LATS = [(8, 8, 8, 8), (4, 6, 10, 6)]
K = 24
SH = R.shifts_of(R.MULTI_MASSES)


# ---- 1. the same CG as the oracle's ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("par_even", [True, False])
@pytest.mark.parametrize("lat,kind", [((8, 8, 8, 8), "random"), ((4, 6, 10, 6), "naik")])
def test_float64_model_is_the_oracle_cg(lat, kind, par_even):
    o, lo, fat, lng, b, _ = R.inputs(lat, kind, "gauss")
    P = R.Problem(o, lo, fat, lng, b, 0.1, par_even, store=np.float64)
    got = R.single(P, R.R2REQ_LADDER, 20, 4, updates=False)
    assert got.update_steps == []
    for k in (1, 7, 20):
        xo, its, fin, hist = o.solveXX(lo, fat, lng, b, 0.1, R.R2REQ_LADDER, k, par_even, histcap=64)
        assert its == k
        assert R.relerr(got.x[k - 1], xo[P.sl]) <= 1e-10
        assert abs(got.r2[k - 1] / fin - 1.0) <= 1e-10              # the true residual of x_k against the recursion's
    assert np.abs(np.array(got.r2s) / hist[1:21] - 1.0).max() <= 1e-10


@pytest.mark.parametrize("par_even", [True, False])
@pytest.mark.parametrize("lat,kind", [((8, 8, 8, 8), "random"), ((4, 6, 10, 6), "naik")])
def test_float64_model_is_the_oracle_multishift_cg(lat, kind, par_even):
    o, lo, fat, lng, b, _ = R.inputs(lat, kind, "gauss")
    P = R.Problem(o, lo, fat, lng, b, R.MULTI_MASSES[0], par_even, store=np.float64)
    for k in (1, 7, 20):                                               # (cut at k: the last iteration takes the `pending` path)
        got = R.multi(P, SH, R.R2REQ_LADDER, k, 4, updates=False)
        xo, its, hist = o.solveXX_multi(lo, fat, lng, b, SH, R.R2REQ_LADDER, k, par_even, histcap=64)
        assert its == k == got.its and got.update_steps == [k]         # (the cut's own flush)
        for j in range(len(SH)):
            assert R.relerr(got.x[j], xo[j][P.sl]) <= 1e-10
        assert np.abs(np.array(got.r2s) / hist[1:k + 1] - 1.0).max() <= 1e-10


# ---- 2. the ladder is the cut solve ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True])
def test_fork_at_k_is_the_solve_cut_at_k(half):
    lat = (4, 6, 10, 6)
    P = R.problem(lat, "random", "gauss", True, half, 0.5)
    for every in (1, 3, 4):
        lad = R.single(P, R.R2REQ_LADDER, 18, every)
        for k in (1, 8, 9, 10, 16, 17, 18):
            cut = R.single(P, R.R2REQ_LADDER, None, every, maxits=k)
            assert cut.its == k and cut.nupd[0] == lad.nupd[k - 1]
            assert np.array_equal(cut.x[0], lad.x[k - 1]) and cut.r2[0] == lad.r2[k - 1]


# ---- 3. schedule, margins, sensitivity ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("lat", LATS)
def test_schedule_margin_and_sensitivity(lat, half):
    ref, sens, spread = R.single_case(lat, "random", "gauss", True, half, 0.5, K, 4)
    print(f"{lat} half={half}: updates at {ref.update_steps}, margin {ref.margin:.3f}, sens {sens.min():.2e} .. {sens.max():.2e}, "
          f"r2 spread {spread.min():.2e} .. {spread.max():.2e}")
    assert ref.update_steps == [8, 16, 24]
    assert ref.nupd == [1] * 8 + [2] * 8 + [3] * 8                     # a cut at k counts its own forced update
    assert ref.margin >= 1e-3
    # float32 eps = 6e-8 and the 16-bit step = 3e-5 set the scale: an ensemble far below or above either has lost its meaning
    lo_, hi_ = (3e-7, 1e-4) if half else (3e-9, 2e-6)
    assert lo_ <= sens.min() and sens.max() <= hi_
    ref1 = R.single_case(lat, "random", "gauss", True, half, 0.1, 12, 4)[0]
    assert ref1.update_steps == [] and ref1.margin >= 1e-3             # m = 0.1: no update before the cut


# ---- 4. wrong logic is far outside the tolerance ------------------------------------------------------------------------------
@pytest.mark.parametrize("wrong", R.WRONG_SINGLE)
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("lat", LATS)
def test_wrong_single_iteration_is_caught(lat, half, wrong):
    P = R.problem(lat, "random", "gauss", True, half, 0.5)
    ref, sens, _ = R.single_case(lat, "random", "gauss", True, half, 0.5, K, 4)
    bad = R.single(P, R.R2REQ_LADDER, K, 4, wrong=wrong)
    ratio = np.array([R.relerr(bad.x[k], ref.x[k]) / (8.0 * sens[k]) for k in range(K)])
    print(f"{lat} half={half} {wrong}: deviation / (8 sens_k) up to {ratio.max():.3g} (k = {1 + int(ratio.argmax())}), first > 1 at "
          f"k = {1 + int(np.argmax(ratio > 1))}")
    assert np.all(ratio[:8] == 0)                                      # up to the first update the defects change nothing
    assert ratio.max() >= 100.0


@pytest.mark.parametrize("wrong", R.WRONG_MULTI)
@pytest.mark.parametrize("lat", LATS)
def test_wrong_multishift_iteration_is_caught(lat, wrong):
    P = R.problem(lat, "random", "gauss", True, False, R.MULTI_MASSES[0])
    best = 0.0
    for k in (9, 17, 23):                                              # a cut at k: the last iteration takes the `pending` path
        ref, sens, _ = R.multi_case(lat, "random", "gauss", True, R.R2REQ_LADDER, 4, maxits=k)
        bad = R.multi(P, SH, R.R2REQ_LADDER, k, 4, wrong=wrong)
        best = max(best, max(R.relerr(bad.x[j], ref.x[j]) / (8.0 * sens[j]) for j in range(len(SH))))
    print(f"{lat} {wrong}: deviation / (8 sens) up to {best:.3g}")
    assert best >= 100.0


# ---- 5. the multi-shift cases of the GPU module are what it says they are -------------------------------------------------------
def test_multishift_cases_on_random_links():
    for r2req, its, nupd in ((1e-6, 20, 3), (1e-8, 28, 4), (1e-10, 32, 4)):
        ref, sens, r2k = R.multi_case((8, 8, 8, 8), "random", "gauss", True, r2req, 4)
        print(f"r2req {r2req:g}: its {ref.its} updates at {ref.update_steps} margin {ref.margin:.3f} sens {sens} r2_k/r2req "
              f"{[v / r2req for v in r2k]}")
        assert (ref.its, ref.nupd) == (its, nupd) and ref.margin >= 1e-3
        assert ref.r2 <= r2req and max(r2k[1:]) * 500.0 <= r2req
        assert sens.max() <= 2e-6
