"""numpy restatement of the connected scalar correlator from point sources (src/observables/conn4d.nim): point sources, the
translated |phi|^2 accumulation, the staggered sign, the whole measurement around a solver passed in, and randomPoint.  Colour
vectors are (vol, 3, 2) arrays in the V=1 even-odd host order, site fields (vol,) arrays, `coords` the (vol, 4) GLOBAL coordinates
(x, y, z, t) of their sites, `lat` the global extents."""
import math

import numpy as np


def point_source(coords, pt, ic):
    """conn4d.nim:173-182: r := 0; r{pt}[ic] := 1"""
    coords = np.asarray(coords)
    r = np.zeros((coords.shape[0], 3, 2))
    r[(coords == np.asarray(pt)).all(axis=1), ic, 0] = 1.0
    return r


def to_grid(f, coords, lat):
    """site field -> [t, z, y, x] array"""
    c = np.asarray(coords)
    g = np.empty((lat[3], lat[2], lat[1], lat[0]) + f.shape[1:], dtype=f.dtype)
    g[c[:, 3], c[:, 2], c[:, 1], c[:, 0]] = f
    return g


def from_grid(g, coords):
    c = np.asarray(coords)
    return g[c[:, 3], c[:, 2], c[:, 1], c[:, 0]]


def translate(f, coords, lat, pt, sense=1):
    """conn4d.nim:184-195: pt[mu] forward shifts in every direction; a forward shift reads the site s + mu (shiftX.nim:76-81), so
    the result at x is f(x + pt): np.roll by -pt on every axis.  sense = -1 is the opposite translation (for the test that pins
    the sense)."""
    g = to_grid(f, coords, lat)
    for mu in range(4):
        g = np.roll(g, -sense * int(pt[mu]), axis=3 - mu)
    return from_grid(g, coords)


def site_norm2(phi):
    return (phi ** 2).sum(axis=(1, 2))


def conn_accum(locmes, phi, coords, lat, pt, scal):
    """conn4d.nim:223-229: n2phi := scal * |phi|^2; locmes += translate(n2phi, pt)"""
    locmes += translate(scal * site_norm2(phi), coords, lat, pt)
    return locmes


def stag_sign(f, coords):
    """conn4d.nim:238-245: f(x) := -f(x) where x0 + x1 + x2 is odd"""
    c = np.asarray(coords)
    odd = ((c[:, 0] + c[:, 1] + c[:, 2]) & 1).astype(bool)
    return np.where(odd.reshape((-1,) + (1,) * (f.ndim - 1)), -f, f)


def slice_sums(f, coords, nt):
    out = np.zeros(nt)
    np.add.at(out, np.asarray(coords)[:, 3], f)
    return out


def conn_meson(solve, coords, lat, pts, nc=3):
    """conn4d.nim:197-248: solve(b) -> phi with (D + mass) phi = b.  Returns (locmes (vol,), est (nt,), phis) with the phis in
    (point, colour) order."""
    locmes = np.zeros(np.asarray(coords).shape[0])
    scal = 1.0 / float(len(pts))
    phis = []
    for pt in pts:
        for c in range(nc):
            phi = solve(point_source(coords, pt, c))
            phis.append(phi)
            conn_accum(locmes, phi, coords, lat, pt, scal)
    locmes = stag_sign(locmes, coords)
    return locmes, slice_sums(locmes, coords, lat[3]), phis


def random_point(uniform, lat, pts, sq_min_distance, maxiter=1_000_000_000, trace=None):
    """conn4d.nim:128-158 with `uniform()` as R.uniform().  Appends to pts and returns the point; `trace`, if a list, receives
    (unrounded draw, accepted) for every iteration."""
    nd = len(lat)
    for _ in range(maxiter):
        raw = [int(math.floor(lat[i] * uniform())) for i in range(nd)]
        far = all(sum(min(abs(p[i] - raw[i]), lat[i] - abs(p[i] - raw[i])) ** 2 for i in range(nd)) >= sq_min_distance for p in pts)
        if trace is not None:
            trace.append((list(raw), far))
        if far:
            pts.append([v - v % 2 for v in raw])
            return pts[-1]
    raise RuntimeError("max iteration reached without finding a random point.\nPerhaps sq_min_distance=%s is too large." % (sq_min_distance,))
