"""The connected scalar correlator without a GPU (qex_amd/conn4d.py, qex_amd/rng.py: GlobalRng; tests/conn4d_ref.py;
src/observables/conn4d.nim): the sense of the translation, pinned by the physics on the oracle's solves, the point generator's
rules, and the global stream.  Observed deviations are printed (pytest -s)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import conn4d_ref as R  # noqa: E402
import qex_amd as q  # noqa: E402
from oracle import oracle as o  # noqa: E402

LAT = [4, 4, 4, 8]


def test_sense_of_the_translation():
    """Unit gauge with the boundary condition and the phases on: a translation by an even vector keeps the phases, and the moved
    antiperiodic boundary is a +-1 gauge transformation, which |phi|^2 does not see.  So |phi_pt|^2 translated by pt (the source
    point lands on the origin) is |phi_0|^2 up to the solver: two solutions with |b - (D+m)x|^2 <= r2req |b|^2, |b| = 1, differ by
    at most eps = 2 sqrt(r2req) / m in norm, and per site | |a|^2 - |b|^2 | <= 2 max|phi| eps + eps^2.  The opposite sense puts
    the source at 2 pt instead: off by the size of the field itself."""
    lo, olo = q.Layout(LAT), o.Layout(LAT)
    g = o.gauge_unit(olo)
    o.rephase(olo, g)
    mass, r2req = 0.1, 1e-20
    eps = 2.0 * np.sqrt(r2req) / mass

    def n2(pt):
        x, its, _ = o.solve(olo, g, None, R.point_source(lo.coords, pt, 1), mass, r2req, 100000)
        return R.site_norm2(x), np.abs(x).max(), its

    ref, big, its0 = n2([0, 0, 0, 0])
    bound = 2.0 * big * eps + eps * eps
    for pt in ([2, 0, 2, 2], [0, 2, 0, 6]):
        f, _, its = n2(pt)
        good = np.abs(R.translate(f, lo.coords, LAT, pt) - ref).max()
        bad = np.abs(R.translate(f, lo.coords, LAT, pt, sense=-1) - ref).max()
        print("pt %s (%d / %d iterations): translated by +pt deviates %.3e (bound %.3e), by -pt %.3e; max|phi|^2 = %.3e" %
              (pt, its, its0, good, bound, bad, ref.max()))
        assert good <= bound
        assert bad > 1e6 * bound and bad > 0.5 * ref.max()
    # the accumulation is that translation
    f, _, _ = n2([2, 0, 2, 2])
    x, _, _ = o.solve(olo, g, None, R.point_source(lo.coords, [2, 0, 2, 2], 1), mass, r2req, 100000)
    acc = R.conn_accum(np.zeros(lo.vol), x, lo.coords, LAT, [2, 0, 2, 2], 0.25)
    assert np.array_equal(acc, R.translate(0.25 * f, lo.coords, LAT, [2, 0, 2, 2]))


def _far(raw, pts, lat, sq):
    return all(sum(min(abs(p[i] - raw[i]), lat[i] - abs(p[i] - raw[i])) ** 2 for i in range(4)) >= sq for p in pts)


@pytest.mark.parametrize("lat,num", [([4, 4, 4, 8], 4), ([8, 8, 8, 16], 16)])
def test_random_point_rules(lat, num):
    sq = q.defaultSqMinDistance(lat, num)
    assert sq == int(np.floor(0.25 * np.sqrt(float(np.prod(lat)) / num)))
    Rg, pts, trace = q.GlobalRng(11), [], []
    for _ in range(num):
        R.random_point(Rg.uniform, lat, pts, sq, trace=trace)
    # the product restates the same function: same seed, same list
    Rp, got = q.GlobalRng(11), []
    for _ in range(num):
        p = q.randomPoint(Rp, lat, got, sq)
        assert p is got[-1]
    again = []
    Rq = q.GlobalRng(11)
    for _ in range(num):
        q.randomPoint(Rq, lat, again, sq)
    print("lat %s: %d points from %d draws, sq_min_distance %d: %s" % (lat, num, len(trace), sq, got))
    assert got == pts == again and len(got) == num
    assert all(0 <= v < lat[i] and v % 2 == 0 for p in got for i, v in enumerate(p))
    # every accepted draw was far from all earlier points on the UNROUNDED coordinates, every rejected one was not
    acc = []
    for raw, far in trace:
        assert far == _far(raw, acc, lat, sq)
        if far:
            acc.append([v - v % 2 for v in raw])
    assert acc == got
    assert q.GlobalRng(12).uniform() != q.GlobalRng(11).uniform()


def test_random_point_gives_up_with_the_reference_text():
    pts = []
    Rg = q.GlobalRng(3)
    q.randomPoint(Rg, LAT, pts, 1000, maxiter=5)               # the first point has nothing to be far from
    with pytest.raises(RuntimeError, match=r"max iteration reached without finding a random point\.\nPerhaps sq_min_distance=1000 is too large\."):
        q.randomPoint(Rg, LAT, pts, 1000, maxiter=7)
    assert len(pts) == 1
    with pytest.raises(RuntimeError, match="max iteration reached"):
        R.random_point(q.GlobalRng(3).uniform, LAT, [[0, 0, 0, 0]], 1000, maxiter=7)


def test_global_rng_stream():
    """the first draws of `R.seed(seed, 987654321)`, computed once and copied here"""
    a, b = q.GlobalRng(987654321), q.GlobalRng(5, 987654321)
    assert [a.uniform() for _ in range(3)] == [0.06697195768356323, 0.7282310724258423, 0.2604483962059021]
    assert [b.uniform() for _ in range(3)] == [0.7936791181564331, 0.5769090056419373, 0.20306509733200073]
    # ... which is the oracle's single MILC stream
    u, _ = o.milc6_stream(5, 987654321, 8)
    c = q.GlobalRng(5)
    assert [c.uniform() for _ in range(8)] == [float(v) for v in u]


def test_ref_pieces():
    lo = q.Layout([4, 6, 10, 6])
    lat = lo.lat
    src = R.point_source(lo.coords, [3, 5, 9, 5], 2)
    assert src.sum() == 1.0 and src[lo.index([3, 5, 9, 5]), 2, 0] == 1.0
    f = np.arange(lo.vol, dtype=float)
    t = R.translate(f, lo.coords, lat, [1, 2, 3, 4])
    assert t[lo.index([0, 0, 0, 0])] == f[lo.index([1, 2, 3, 4])] and t[lo.index([3, 5, 9, 5])] == f[lo.index([0, 1, 2, 3])]
    s = R.stag_sign(f, lo.coords)
    assert s[lo.index([1, 0, 0, 3])] == -f[lo.index([1, 0, 0, 3])] and s[lo.index([1, 1, 0, 1])] == f[lo.index([1, 1, 0, 1])]
    assert np.array_equal(R.stag_sign(s, lo.coords), f)
