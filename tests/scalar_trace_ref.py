"""numpy restatement of the stochastic scalar trace (src/observables/scalarTrace.nim:146-218, src/algorithms/dilution.nim):
dilution masks, both forms of the trace, the per-timeslice sums and the whole measurement around a solver passed in.  Fields are
(vol, 3, 2) arrays in the V=1 even-odd host order, `coords` the (vol, 4) GLOBAL coordinates of their sites."""
import numpy as np

EO, CORNER = 0, 1
NPAT = {EO: 2, CORNER: 8}


def patterns(kind, nt):
    """(t, idx) in the reference's order: t outer, the patterns 0..high of the kind inner (scalarTrace.nim:169-170)"""
    return [(t, i) for t in range(nt) for i in range(NPAT[kind])]


def pattern_of(coords, kind):
    x = np.asarray(coords)
    if kind == EO:
        return (x[:, 0] + x[:, 1] + x[:, 2] + x[:, 3]) & 1
    return (x[:, 0] & 1) | ((x[:, 1] & 1) << 1) | ((x[:, 2] & 1) << 2)


def mask(coords, kind, idx, t):
    return (np.asarray(coords)[:, 3] == t) & (pattern_of(coords, kind) == idx)


def dilute(src, coords, kind, idx, t, scale=1.0):
    """tmps := 0; tmps{i} := scale * eta{i} on the sites of the pattern at time t"""
    r = np.zeros_like(src)
    m = mask(coords, kind, idx, t)
    r[m] = scale * src[m]
    return r


def cplx(v):
    return v[..., 0] + 1j * v[..., 1]


def site_dot(a, b):
    """a[i].dot b[i] = sum_colour conj(a) b per site, as (vol, 2)"""
    z = (np.conj(cplx(a)) * cplx(b)).sum(axis=1)
    return np.stack([z.real, z.imag], axis=-1)


def accumulate(trce, a, b, coef=1.0):
    trce += coef * site_dot(a, b)
    return trce


def slice_sums(trce, coords, nt):
    """(nt, 2): Re, Im of the sum over every time slice"""
    out = np.zeros((nt, 2))
    np.add.at(out, np.asarray(coords)[:, 3], trce)
    return out


def scalar_trace(solve, eta, coords, nt, mass, kind, improved, scale=1.0, nc=3):
    """One noise source: solve(b) -> phi with (D + mass) phi = b.  Returns (trce (vol, 2), est (nt,), phis) with
    est[t] = Re slice sum / spatial volume."""
    trce = np.zeros((eta.shape[0], 2))
    phis = []
    for t, idx in patterns(kind, nt):
        b = dilute(eta, coords, kind, idx, t, scale)
        phi = solve(b)
        phis.append((b, phi))
        if improved:
            accumulate(trce, phi, phi, mass)
        else:
            accumulate(trce, b, phi, 1.0)
    trce *= 1.0 / nc
    spatv = eta.shape[0] // nt
    return trce, slice_sums(trce, coords, nt)[:, 0] / spatv, phis


def z4_from_uniform(u):
    """distributionUtils.nim:126-140: (vol, 3) uniforms -> (vol, 3, 2)"""
    re = np.where(u < 0.25, 1.0, np.where(u < 0.5, 0.0, np.where(u < 0.75, -1.0, 0.0)))
    im = np.where(u < 0.25, 0.0, np.where(u < 0.5, 1.0, np.where(u < 0.75, 0.0, -1.0)))
    return np.stack([re, im], axis=-1)


def z2_from_uniform(u):
    return np.stack([np.where(u < 0.5, 1.0, -1.0), np.zeros_like(u)], axis=-1)
