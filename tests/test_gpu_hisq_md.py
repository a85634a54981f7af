"""HISQ molecular dynamics resident on the device (qexhip_md_hisq_*, ResidentMD.hisq_*, examples/hisqhmc.py) against the
host-pointer entries, which tests/test_smear.py holds to the oracle: the closure built from the resident links is the one built
from a host field, the resident force is the host-pointer force bit for bit, and a trajectory of the example is the same
trajectory on either path.  Observed figures are printed (pytest -s).
Everything here compares the library with itself.  The trajectory as a whole (schedule, heatbath, the three energy terms, link
update, reunit / revert, accept/reject stream) is held to the oracle replay of hisqhmc.nim by tests/test_gpu_hisq_hmc.py, and the
pairing of the force with the action it integrates (odd-site sign, hop-3 term, TAH(F u^+), the step factor -1/2 dt / m) by the
gradient and dH ~ dt^2 tests there (product) and in tests/test_hisq_hmc_ref.py (oracle, no GPU)."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# [4, 6, 10, 6]: 720 sites per parity = 11.25 tiles (ragged last tile), no paired tile order, extents of 4 (Naik and fat7 minimum)
SHAPES = [[8, 8, 8, 8], [4, 6, 10, 6]]
CASES = [(SHAPES[0], "warm"), (SHAPES[0], "random"), (SHAPES[1], "warm"), (SHAPES[1], "random")]
SCALES = [0.7, -1.3, 0.45, 1.9, -0.6]
T = -0.37
RTOL = 2e-11          # tests/test_golden_hmc.py: two paths of one trajectory


@functools.lru_cache(maxsize=None)
def _setup(lat, start):
    """the fields of one case, and the host-pointer reference results on a context of their own; computed once, never written"""
    import qex_amd as q

    lat = list(lat)
    lo = q.Layout(lat)
    rng = q.RngField(lat, q.RngMilc6, 4711)
    g = rng.warm(0.3) if start == "warm" else rng.random()
    p = rng.randomTAH()
    v = [rng.gaussian_vector() for _ in range(5)]
    ctx = q.Context(lat)
    gp = g.copy()
    q.rephase(lo, gp)                                        # setBC + stagPhase, as smearRephase
    hc = q.HisqCoefs()
    sf = hc.smearGetForce(ctx, gp)
    s = q.Staggered(ctx, None, smear=hc)
    Dx = np.zeros_like(v[0])
    s.D(Dx, v[0], 0.2)
    forces = {}
    for n in (1, 3, 5):
        f = np.zeros_like(g)
        sf.fermionForce(f, v[:n], SCALES[:n])
        forces[n] = f
    for a in [g, p, Dx] + v + list(forces.values()):
        a.setflags(write=False)
    return dict(g=g, p=p, v=v, Dx=Dx, forces=forces)


def _resident(S, lat):
    import qex_amd as q

    ctx = q.Context(list(lat))
    md = q.ResidentMD(ctx)
    md.begin(S["g"].copy(), S["p"].copy())
    md.hisq_prepare(set_links=True)
    return ctx, md


def _dev_D(ctx, x, m):
    xi = ctx.field_new(np.ascontiguousarray(x))
    ri = ctx.field_new()
    ctx.dev_D(ri, xi, m)
    return ctx.field_download(ri)


def _one_rounding_of(p1, p0, t, f):
    """p1 == fl(p0 + fl(t f)) or p1 == fma(t, f, p0), element by element.  The fma is checked through error-free transformations:
    t f = hi + lo (Dekker), hi + p0 = s + e (Knuth), and the correctly rounded sum is within half an ulp of s + e + lo."""
    plain = p0 + t * f
    split = 134217729.0 * f
    fh = split - (split - f)
    fl_ = f - fh
    ts = 134217729.0 * t
    th = ts - (ts - t)
    tl = t - th
    hi = t * f
    lo = ((th * fh - hi) + th * fl_ + tl * fh) + tl * fl_
    s = hi + p0
    bb = s - hi
    e = (hi - (s - bb)) + (p0 - bb)
    r = (s - p1) + e + lo
    fused = np.abs(r) <= 0.5 * np.spacing(np.abs(p1)) * (1.0 + 1e-12)
    return (p1 == plain) | fused


@pytest.mark.parametrize("lat,start", CASES)
def test_prepare_builds_the_closure_of_the_phased_host_field(lat, start):
    S = _setup(tuple(lat), start)
    ctx, md = _resident(S, lat)
    got = _dev_D(ctx, S["v"][0], 0.2)
    assert np.array_equal(got, S["Dx"]), np.abs(got - S["Dx"]).max()
    g2, p2 = np.zeros_like(S["g"]), np.zeros_like(S["p"])
    md.end(g2, p2)
    assert np.array_equal(g2, S["g"]) and np.array_equal(p2, S["p"])        # the resident thin links are not rephased, not touched
    # set_links = False leaves the operator's links alone: after another prepare on moved links D is still the old operator
    md.update_links(0.05)
    md.hisq_prepare(set_links=False)
    assert np.array_equal(_dev_D(ctx, S["v"][0], 0.2), S["Dx"])
    md.hisq_prepare(set_links=True)
    assert not np.array_equal(_dev_D(ctx, S["v"][0], 0.2), S["Dx"])
    ctx.close()


@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("lat,start", CASES)
def test_resident_force_is_the_host_pointer_force(lat, start, n):
    """n = 5: a second launch of k_outer13, which accumulates onto the first four vectors' sums"""
    S = _setup(tuple(lat), start)
    ctx, md = _resident(S, lat)
    ids = [ctx.field_new(np.ascontiguousarray(x)) for x in S["v"][:n]]
    ref = S["forces"][n]
    for fused in (3, 0):                 # k_outer13 + k_projtah_kick, and the launches they replace: the same bits
        ctx.set_option("hisq_md_fused", fused)
        md.begin(None, S["p"].copy())
        md.hisq_fforce(ids, SCALES[:n], T)
        f = md.hisq_force()
        assert np.array_equal(f, ref), (fused, np.abs(f - ref).max())
        p1 = np.zeros_like(S["p"])
        md.end(None, p1)
        ok = _one_rounding_of(p1, S["p"], T, ref)
        print("%s %s n=%d fused=%d: max |f| %.3e, momenta off one rounding: %d of %d" % (lat, start, n, fused, np.abs(f).max(), (~ok).sum(), ok.size))
        assert ok.all()
        assert not np.array_equal(p1, S["p"])
    g2 = np.zeros_like(S["g"])
    md.end(g2, None)
    assert np.array_equal(g2, S["g"])
    ctx.close()


@pytest.mark.parametrize("lat,start", [(SHAPES[0], "warm"), (SHAPES[1], "random")])
def test_solve_and_force_is_the_batch_solve_then_the_force(lat, start):
    S = _setup(tuple(lat), start)
    ctx, md = _resident(S, lat)
    n = 5                                 # a batch of four and a batch of one
    masses = [0.5, 0.3, 0.8, 0.4, 0.6]
    phi = [ctx.field_new(np.ascontiguousarray(x)) for x in S["v"][:n]]
    xs = [ctx.field_new() for _ in range(n)]
    its = md.hisq_fforce_solve(phi, masses, SCALES[:n], 1e-16, 2000, T)
    f = md.hisq_force()
    p1 = np.zeros_like(S["p"])
    md.end(None, p1)
    its_ref, _ = ctx.dev_solve_batch(xs, phi, masses, 1e-16, 2000)
    print("%s %s: iterations %r (dev_solve_batch %r)" % (lat, start, its, its_ref))
    assert its == its_ref and min(its) > 5
    md.begin(None, S["p"].copy())
    md.hisq_fforce(xs, SCALES[:n], T)
    f_ref = md.hisq_force()
    p_ref = np.zeros_like(S["p"])
    md.end(None, p_ref)
    assert np.array_equal(f, f_ref), np.abs(f - f_ref).max()
    assert np.array_equal(p1, p_ref)
    for k in range(n):                    # the sources are read only
        assert np.array_equal(ctx.field_download(phi[k]), S["v"][k])
    ctx.close()


def _run_example(extra):
    cmd = [sys.executable, os.path.join(ROOT, "examples", "hisqhmc.py"), "-lat", "8", "8", "8", "8", "-mass", "0.1", "-gsteps", "3", "-fsteps", "2",
           "-trajs", "1", "-warm", "0.3", "-reverse"] + extra
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-4000:]
    return p.stdout


def test_example_trajectory_resident_against_host():
    """one trajectory of examples/hisqhmc.py at 8^4, mass 0.1, 3 gauge and 2 fermion 2MN steps, resident and with -host: every
    energy term, dH and the plaquettes at the tolerance of tests/test_golden_hmc.py, the same verdict, and a reversibility
    deviation within twice the host path's"""
    res, host = _run_example([]), _run_example(["-host"])
    keep = re.compile(r"^(kinetic = |ACC: |REJ: |MEASplaq |REVERSE: )")
    num = re.compile(r"[-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?|inf")
    a_lines = [ln for ln in res.splitlines() if keep.search(ln)]
    b_lines = [ln for ln in host.splitlines() if keep.search(ln)]
    print("\n".join("resident  " + ln for ln in a_lines))
    print("\n".join("host      " + ln for ln in b_lines))
    assert len(a_lines) == len(b_lines) == 5, (res, host)          # H_i terms, REVERSE, H_f terms, verdict, plaquettes
    vol = 8 ** 4
    compared = 0
    for a, b in zip(a_lines, b_lines):
        assert a.split()[0] == b.split()[0], (a, b)                # same kind of line, same accept / reject decision
        na, nb = [float(v) for v in num.findall(a)], [float(v) for v in num.findall(b)]
        assert na and len(na) == len(nb), (a, b)
        if a.startswith("REVERSE"):
            print("reversibility: max link deviation resident %.3e, host %.3e" % (na[0], nb[0]))
            assert na[0] <= 2.0 * nb[0], (na[0], nb[0])
            assert nb[0] < 1e-8                                    # (a trajectory that does not come back would make the bound empty)
            continue
        if a.startswith("kinetic"):
            scales = [max(abs(nb[0]), 16.0 * vol), max(abs(nb[1]), 16.0 * vol), abs(nb[2])]      # T, Sg carry the 16 V offset; Sf of itself
        elif a.startswith(("ACC", "REJ")):
            scales = [1e-6 / RTOL, 1e-6 / RTOL * max(1.0, abs(nb[1])), 0.0]                      # dH absolute 1e-6; the uniform deviate exactly
        else:
            scales = [max(abs(y), 0.1) for y in nb]
        for x, y, sc in zip(na, nb, scales):
            assert abs(x - y) <= RTOL * sc, (a, b)
            compared += 1
    assert compared == 12


def test_argument_and_state_errors_come_before_any_launch():
    import qex_amd as q

    lat = SHAPES[1]
    S = _setup(tuple(lat), "warm")
    L = q.lib()
    ARG, STATE = -1, -3
    ctx = q.Context(lat)
    h = ctx._h
    ids1 = (C.c_int * 1)(0)
    one = (C.c_double * 1)(1.0)
    f = np.zeros_like(S["g"])
    fp = f.ctypes.data_as(C.c_void_p)
    assert L.qexhip_md_hisq_prepare(h, None, None, 1) == STATE                       # no resident links
    ids1[0] = ctx.field_new(np.ascontiguousarray(S["v"][0]))
    assert L.qexhip_md_hisq_fforce(h, 1, ids1, one, 0.1) == STATE                    # ... for the force either
    q.gaugeSet(ctx, S["g"].copy())
    assert L.qexhip_md_hisq_fforce(h, 1, ids1, one, 0.1) == STATE                    # no momenta
    md = q.ResidentMD(ctx)
    md.begin(None, S["p"].copy())
    assert L.qexhip_md_hisq_fforce(h, 1, ids1, one, 0.1) == STATE                    # no prepare
    assert L.qexhip_md_hisq_fforce_solve(h, 1, ids1, one, one, one, 10, 0.1, None) == STATE
    md.hisq_prepare(set_links=False)
    assert L.qexhip_md_hisq_force_get(h, fp) == STATE                                # no force yet
    assert L.qexhip_md_hisq_fforce_solve(h, 1, ids1, one, one, one, 10, 0.1, None) == STATE     # the operator has no links
    md.hisq_prepare(set_links=True)
    second = ctx.field_new(np.ascontiguousarray(S["v"][1]))
    two, twice, unknown = (C.c_double * 2)(1.0, 2.0), (C.c_int * 2)(ids1[0], ids1[0]), (C.c_int * 2)(ids1[0], second + 1000)
    for rc in (L.qexhip_md_hisq_fforce(h, 0, ids1, one, 0.1), L.qexhip_md_hisq_fforce(h, -2, ids1, one, 0.1),
               L.qexhip_md_hisq_fforce(h, 1, None, one, 0.1), L.qexhip_md_hisq_fforce(h, 1, ids1, None, 0.1),
               L.qexhip_md_hisq_fforce(h, 2, twice, two, 0.1), L.qexhip_md_hisq_fforce(h, 2, unknown, two, 0.1),
               L.qexhip_md_hisq_fforce_solve(h, 0, ids1, one, one, one, 10, 0.1, None),
               L.qexhip_md_hisq_fforce_solve(h, 1, ids1, None, one, one, 10, 0.1, None),
               L.qexhip_md_hisq_fforce_solve(h, 1, ids1, one, None, one, 10, 0.1, None),
               L.qexhip_md_hisq_fforce_solve(h, 1, ids1, one, one, None, 10, 0.1, None),
               L.qexhip_md_hisq_fforce_solve(h, 2, twice, two, two, two, 10, 0.1, None),
               L.qexhip_md_hisq_force_get(h, None), L.qexhip_md_hisq_prepare(None, None, None, 1)):
        assert rc == ARG
    # nothing was launched: no force exists, links and momenta are as they were
    assert L.qexhip_md_hisq_force_get(h, fp) == STATE
    g2, p2 = np.zeros_like(S["g"]), np.zeros_like(S["p"])
    md.end(g2, p2)
    assert np.array_equal(g2, S["g"]) and np.array_equal(p2, S["p"])
    # the host-pointer entries still refuse what they refused
    assert L.qexhip_hisq_prepare(h, None, None, None) == ARG
    psi = (C.c_void_p * 1)(S["v"][0].ctypes.data)
    assert L.qexhip_hisq_fermion_force(h, None, psi, one, 1) == ARG
    # release drops the state
    md.hisq_fforce([ids1[0]], [1.0], 0.1)
    assert L.qexhip_md_hisq_force_get(h, fp) == 0 and np.abs(f).max() > 0
    assert L.qexhip_hisq_release(h) == 0
    assert L.qexhip_md_hisq_fforce(h, 1, ids1, one, 0.1) == STATE
    ctx.close()
