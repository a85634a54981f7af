"""The mixed-precision CG iterations held to a step-by-step reference: SloppySingle (k_slp_*), SloppyHalf with half = 1 (k_slph_*)
and phase 1 of the fp32 multi-shift solve (k_msf_*) against the numpy model of tests/sloppy_ref.py.

A solve cut at maxits = k returns the iterate x_k, its true residual and the update count, so the state after every step is
observable: the single solves run the ladder k = 1..K and every x_k, r2, iteration and update count is compared with the model's.
Phase 2 of the multi-shift solve reuses maxits, so that one is cut by its tolerance, at cases where the model says no shift needs
refining.  The tolerance is 8 x the sensitivity of the model's own x_k to the roundings it does not reproduce (an ensemble of 8
perturbed runs, tests/sloppy_ref.py Noise; the factor covers the ensemble under-sampling its maximum and the device's reduction
order).  Wrong iteration logic -- beta without sigma / sigma_p, r_s not rebuilt or x_s not zeroed by an update, the multi-shift
unit conversion or zeta recurrence -- is 1e2 .. 1e10 times outside it (tests/test_sloppy_ref.py).  At this tolerance the 16-bit
ladder holds the recurrence and its units, not the rounding mode of a pack: tests/test_half_pack.py and test_gpu_half.py's operator
test keep that.  A model case whose decisions come closer than 1e-3 to a threshold would leave the update schedule open: such a
case is invalid and fails, it is not skipped.

The grid-stride loops of k_slp_* wrap beyond 2048 workgroups of 256 float2 (3 Vh > 524288) and those of k_msf_* beyond 2048 x 256
float4 (96 ntile > 524288): one case each.  The 16-bit kernels walk one lane per site and wrap only beyond 32^4, where the model
takes minutes: left out.

Measured on MI355X: see the table in DESIGN.md "Engineering checks".  Observed values are printed (pytest -s)."""
import functools
import os
import re

import numpy as np
import pytest

import sloppy_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATS = [(8, 8, 8, 8), (4, 6, 10, 6)]            # the second: a ragged last tile
K = 24                                          # m = 0.5: the updates of steps 8, 16, 24 (sloppy_check 4) fall inside
MASS = 0.5
MARGIN = 8.0


@functools.lru_cache(maxsize=None)
def _op(lat, kind):
    import qex_amd as q

    o, lo, fat, lng, b, fmt = R.inputs(lat, kind, "gauss")
    ctx = q.Context(list(lat))
    s = q.newStag3(ctx, fat, lng) if lng is not None else q.newStag(ctx, fat)
    return ctx, s


def _caps():
    """the grid caps of the iteration kernels, read from the source: (k_slp_* workgroups, k_msf_* workgroups)"""
    def one(name, pat):
        with open(os.path.join(ROOT, "qex_amd", "csrc", name)) as f:
            m = re.search(pat, f.read())
        assert m, "%s no longer matches %r: update the wrap conditions of this module" % (name, pat)
        return int(m.group(1))

    slp = one("dslash_f32.hip", r"static inline int grid_for\(size_t n\) \{\s*size_t nb = \(n \+ 255\) / 256;\s*if \(nb > (\d+)\) nb = ")
    msf = one("multishift_f32.hip", r"static inline int grid4\(size_t n4\) \{[^}]*\(n4 \+ 255\) / 256, (\d+)\)")
    return slp, msf


def _ladder(lat, kind, source, par_even, half, mass, steps, every):
    """the library's solves cut at maxits = k, k in steps, against the model's ladder; returns the worst ratios (x, r2)"""
    import qex_amd as q

    ref, sens, spread = R.single_case(lat, kind, source, par_even, half, mass, max(steps), every)
    assert ref.margin >= 1e-3, "invalid case: a decision of the model is within %.1e of its threshold" % ref.margin
    b = R.inputs(lat, kind, source)[4]
    P = R.problem(lat, kind, source, par_even, half, mass)
    other = slice(P.h, 2 * P.h) if par_even else slice(0, P.h)
    ctx, s = _op(lat, kind)
    ctx.set_option("half", 1 if half else 0)
    ctx.set_option("sloppy_check", every)
    if half:
        assert ctx.links_info_half()[0] == R.KINDS[kind][2]
    rx, rr = [], []
    for k in steps:
        sp = q.SolverParams(r2req=R.R2REQ_LADDER, maxits=k, verbosity=0, sloppySolve=q.SloppyHalf if half else q.SloppySingle)
        x = np.zeros_like(b)
        s.solveXX(x, b, mass, sp, par_even)
        assert sp.iterations == k
        assert sp.reliableUpdates == ref.nupd[k - 1], (k, sp.reliableUpdates, ref.nupd[k - 1], ref.update_steps)
        assert not x[other].any()
        last = ctx.sloppy_last()
        if half:
            assert (last["precision"], last["fell_back"], last["half_iters"], last["f32_iters"]) == (2, 0, k, 0), (k, last)
        else:
            assert last == dict(precision=1, half_iters=0, f32_iters=k, fell_back=0), (k, last)
        rx.append(R.relerr(x[P.sl], ref.x[k - 1]) / (MARGIN * sens[k - 1]))
        rr.append(abs(sp.r2 / ref.r2[k - 1] - 1.0) / (MARGIN * spread[k - 1]))
    kx, kr = int(np.argmax(rx)), int(np.argmax(rr))
    print(f"steps {lat} {kind} {source} par_even={par_even} half={half} m={mass} check={every}: updates at {ref.update_steps}, "
          f"margin {ref.margin:.3f}, sens {sens.min():.2e} .. {sens.max():.2e}; |x_k - model| / (8 sens_k) <= {rx[kx]:.3f} "
          f"(k = {steps[kx]}), |r2 / model - 1| / (8 spread_k) <= {rr[kr]:.3f} (k = {steps[kr]})")
    assert rx[kx] <= 1.0, ("x_k", steps[kx], rx)
    assert rr[kr] <= 1.0, ("r2", steps[kr], rr)
    return rx[kx], rr[kr]


# ---- 1. SloppySingle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every", [1, 3, 4])
@pytest.mark.parametrize("source", ["gauss", "point"])
@pytest.mark.parametrize("kind", ["random", "warm", "naik"])
@pytest.mark.parametrize("par_even", [True, False])
@pytest.mark.parametrize("lat", LATS)
def test_single_steps(oracle, lat, par_even, kind, source, every):
    _ladder(lat, kind, source, par_even, False, MASS, range(1, K + 1), every)


# ---- 2. SloppyHalf on 16-bit storage ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("every", [1, 3, 4])
@pytest.mark.parametrize("source", ["gauss", "point"])
@pytest.mark.parametrize("kind", ["random", "warm", "naik", "scaled"])
@pytest.mark.parametrize("par_even", [True, False])
@pytest.mark.parametrize("lat", LATS)
def test_half_steps(oracle, lat, par_even, kind, source, every):
    _ladder(lat, kind, source, par_even, True, MASS, range(1, K + 1), every)


# ---- 3. m = 0.1: no update before the cut ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("lat", LATS)
def test_steps_without_an_update(oracle, lat, half):
    ref = R.single_case(lat, "random", "gauss", True, half, 0.1, 12, 4)[0]
    assert ref.update_steps == [] and ref.nupd == [1] * 12
    _ladder(lat, "random", "gauss", True, half, 0.1, range(1, 13), 4)


# ---- 4. fp32 multi-shift, phase 1 -------------------------------------------------------------------------------------------
def _multi(lat, kind, par_even, r2req, every, masses=R.MULTI_MASSES, maxits=5000):
    import qex_amd as q

    ref, sens, r2k = R.multi_case(lat, kind, "gauss", par_even, r2req, every, maxits, masses)
    assert ref.margin >= 1e-3, "invalid case: a decision of the model is within %.1e of its threshold" % ref.margin
    # no shift is refined, so the x_k returned are phase 1's: the model's shifted residuals are at least 4 x below the threshold
    assert (ref.r2 <= r2req or ref.its == maxits) and 4.0 * max(r2k[1:]) <= r2req, (ref.r2, r2k)
    b = R.inputs(lat, kind, "gauss")[4]
    P = R.problem(lat, kind, "gauss", par_even, False, masses[0])
    sh = R.shifts_of(masses)
    ctx, s = _op(lat, kind)
    ctx.set_option("half", 0)
    ctx.set_option("sloppy_check", every)
    xs = [np.zeros_like(b) for _ in sh]
    sp = q.SolverParams(r2req=r2req, maxits=maxits, verbosity=0)
    fin = s.solveXX_multi(xs, b, sh, sp, parEven=par_even, sloppy=1)
    ratio = [R.relerr(xs[j][P.sl], ref.x[j]) / (MARGIN * sens[j]) for j in range(len(sh))]
    print(f"multi steps {lat} {kind} par_even={par_even} r2req={r2req:g} check={every}: its {sp.iterations} (model {ref.its}), updates "
          f"{sp.reliableUpdates} (model {ref.nupd} at {ref.update_steps}), refine {sp.refineIterations}, margin {ref.margin:.3f}, sens "
          f"{sens.min():.2e} .. {sens.max():.2e}; |x_k - model| / (8 sens_k) = {['%.3f' % v for v in ratio]}; r2_k / r2req model "
          f"{['%.1e' % (v / r2req) for v in r2k]} library {['%.1e' % (v / r2req) for v in fin]}")
    assert sp.refineIterations == [0] * len(sh)
    assert (sp.iterations, sp.reliableUpdates) == (ref.its, ref.nupd)
    assert max(ratio) <= 1.0, ratio
    return max(ratio)


@pytest.mark.parametrize("r2req", [1e-6, 1e-8, 1e-10])
@pytest.mark.parametrize("kind", ["random", "warm", "naik"])
@pytest.mark.parametrize("par_even", [True, False])
@pytest.mark.parametrize("lat", LATS)
def test_multi_steps(oracle, lat, par_even, kind, r2req):
    if lat == LATS[0] and kind == "random" and par_even:
        ref = R.multi_case(lat, kind, "gauss", par_even, r2req, 4)[0]
        assert (ref.its, ref.nupd) == {1e-6: (20, 3), 1e-8: (28, 4), 1e-10: (32, 4)}[r2req]
    _multi(lat, kind, par_even, r2req, 4)


@pytest.mark.parametrize("par_even", [True, False])
@pytest.mark.parametrize("lat", LATS)
def test_multi_steps_cut_at_maxits(oracle, lat, par_even):
    """maxits = 18 ends phase 1 between two posted updates: the last iteration's increments of the shifted systems run with the
    recurrences already stopped (`pending`), and the shifted residuals are below r2req, so phase 2 leaves phase 1's x_k alone"""
    ref = R.multi_case(lat, "random", "gauss", par_even, 1e-6, 4, 18)[0]
    assert ref.its == 18 and ref.update_steps == [8, 16, 18]
    _multi(lat, "random", par_even, 1e-6, 4, maxits=18)


# ---- 5. the grid-stride loops past their first pass -------------------------------------------------------------------------
def test_single_steps_wrapped_grid(oracle):
    lat = (24, 24, 24, 26)
    vh = int(np.prod(lat)) // 2
    assert 3 * (-(-vh // 64) * 64) > _caps()[0] * 256, "the element loops of k_slp_* do not wrap"
    _ladder(lat, "random", "gauss", True, False, MASS, [1, 2], 4)
    _op.cache_clear()                                    # (the large contexts and inputs are not kept)
    R.single_case.cache_clear()


def test_multi_steps_wrapped_grid(oracle):
    lat = (28, 28, 28, 32)
    ntile = -(-(int(np.prod(lat)) // 2) // 64)
    assert ntile * 96 > _caps()[1] * 256, "the element loops of k_msf_* do not wrap"
    ref = R.multi_case(lat, "random", "gauss", True, 1e-3, 1, 5000, (2.0, 2.5, 3.0, 4.0))[0]
    assert ref.its <= 3
    _multi(lat, "random", True, 1e-3, 1, (2.0, 2.5, 3.0, 4.0))
    _op.cache_clear()
    R.multi_case.cache_clear()
    R.problem.cache_clear()
    R.inputs.cache_clear()
