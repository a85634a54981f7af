"""numpy restatement of src/gauge/gaugefix.nim on host fields in the V=1 even-odd order (qex_amd.layout.Layout): gaugeTransform
(:8-20), gtGradient (:22-57), linkTrace (:135-142), gfMetrics (:145-174), gfLineMin (:197-227), overRelaxSu2 (:241-284, the same
order of operations), relaxE / relaxO (:286-310), getGaugeFixTransform (:312-355, plus a bound `maxits` on the updates).
Vectorised over sites.  The relax path runs in any numpy float type (`dtype=np.longdouble` is the yardstick of the fp64 run); the
line-minimisation step (exp, projectSU) is fp64.  The yardstick of tests/test_gaugefix_ref.py, tests/test_gpu_gaugefix.py and
tests/gaugefix_rank_worker.py."""
import numpy as np

from meson_ref import neighbours

PAIRS = ((0, 1), (1, 2), (0, 2))


def cmat(a, dtype=np.float64):
    """(..., 3, 3, 2) -> (..., 3, 3) complex of the given real type"""
    a = np.asarray(a, dtype=dtype)
    return a[..., 0] + 1j * a[..., 1]


def rmat(z):
    return np.ascontiguousarray(np.stack([z.real, z.imag], axis=-1).astype(np.float64))


def adj(m):
    return np.conj(np.swapaxes(m, -1, -2))


def mul(a, b):
    return np.einsum("sij,sjk->sik", a, b)


def links(g, dtype=np.float64):
    return [cmat(g[:, mu], dtype) for mu in range(4)]


def gauge_transform(lo, G, t):
    """gt[mu] = t * (g[mu] * t(x+mu).adj), all four directions"""
    return [mul(t, mul(G[mu], adj(t[neighbours(lo, mu)[0]]))) for mu in range(4)]


def gradient(lo, G, t, dirs):
    gd = np.zeros_like(t)
    for mu in dirs:
        fw, bw = neighbours(lo, mu)
        gd = gd + mul(G[mu], adj(t[fw])) + adj(mul(t[bw], G[mu][bw]))
    return gd


def tah(m):
    a = (m - adj(m)) * 0.5
    tr = np.einsum("sii->s", a) / 3
    a = a.copy()
    for i in range(3):
        a[:, i, i] -= tr
    return a


def norm2(m):
    return (m.real ** 2 + m.imag ** 2).sum(axis=(1, 2))


def link_trace(lo, G, dirs):
    s = sum(np.einsum("sii->s", G[mu]).real.sum() for mu in dirs)
    return s / (len(dirs) * lo.vol * 3)


def metrics(lo, gd, t, nd):
    """(met, gre, gro) of gfMetrics"""
    sf = 0.5 / (nd * lo.vol * 3)
    sfg = 2.0 * sf * nd
    m = mul(t, gd)
    n = norm2(tah(m))
    h = lo.vol // 2
    return sf * np.einsum("sii->s", m).real.sum(), sfg * n[:h].sum(), sfg * n[h:].sum()


def gf_metric(lo, G, t, dirs):
    return metrics(lo, gradient(lo, G, t, dirs), t, len(dirs))[0]


def over_relax_su2(r, x, i, j, o):
    """overRelaxSu2 on the rows i, j of r (n, 3, 3), in place"""
    r0 = x[:, i, i].real + x[:, j, j].real
    r1 = -x[:, j, i].imag - x[:, i, j].imag
    r2 = x[:, j, i].real - x[:, i, j].real
    r3 = x[:, j, j].imag - x[:, i, i].imag
    n = np.sqrt(r0 * r0 + r1 * r1 + r2 * r2 + r3 * r3)
    r0 = r0 + n * (1 - o) / o
    small = np.abs(r0) < 1e-12
    r0 = np.where(small, np.where(r0 < 0, -1e-12, 1e-12).astype(r0.dtype), r0)
    nn = 1 / np.sqrt(r0 * r0 + r1 * r1 + r2 * r2 + r3 * r3)
    u00 = nn * r0 + 1j * (nn * r3)
    u01 = nn * r2 + 1j * (nn * r1)
    ri, rj = r[:, i, :].copy(), r[:, j, :].copy()
    r[:, i, :] = u00[:, None] * ri + u01[:, None] * rj
    r[:, j, :] = np.conj(u00)[:, None] * rj - np.conj(u01)[:, None] * ri


def relax(lo, t, gd, parity, orf):
    """relaxE (parity 0) / relaxO (parity 1), in place"""
    h = lo.vol // 2
    sl = slice(0, h) if parity == 0 else slice(h, lo.vol)
    ts, gs = t[sl].copy(), gd[sl]
    for i, j in PAIRS:
        over_relax_su2(ts, mul(ts, gs), i, j, orf)
    t[sl] = ts


def expm(m):
    """exp of matexp.nim: order-4 Taylor of expm1 at m / 2^20, 20 squarings r <- r (r + 2), + 1"""
    ms = m / float(1 << 20)
    m2 = mul(ms, ms)
    a = m2 / 24 + ms / 6
    a = a + 0.5 * np.eye(3)
    e = mul(a, m2) + ms
    for _ in range(20):
        e = mul(e, e) + 2 * e
    return e + np.eye(3)


def project_su(m):
    """projectSU: m (m^+ m)^(-1/2), then the determinant's phase removed"""
    w, v = np.linalg.eigh(mul(adj(m), m))
    u = mul(m, mul(v * (w ** -0.5)[:, None, :], adj(v)))
    ph = np.angle(np.linalg.det(u)) / -3.0
    return u * np.exp(1j * ph)[:, None, None]


def line_min(lo, G, gd, t, dirs, eps, m0):
    """gfLineMin: returns (t, eps)"""
    a = tah(mul(t, gd))
    t0 = t
    step = expm(-eps * a)
    t1 = mul(step, t0)
    m1 = gf_metric(lo, G, t1, dirs)
    t2 = mul(step, t1)
    m2 = gf_metric(lo, G, t2, dirs)
    x = eps * (3 * m0 - 4 * m1 + m2) / (2 * m0 - 4 * m1 + 2 * m2)
    x = 0.0 if x <= 0 else x
    x = 2 * eps if 2 * eps <= x else x
    return project_su(mul(expm(-x * a), t0)), x


def get_gauge_fix_transform(lo, g, dirs, gstop=1e-5, orf=1.8, maxits=100000, t0=None, dtype=np.float64, keep=()):
    """getGaugeFixTransform from t0 (None: the identity): (t, info).  info: iters (updates done), hist (iters, 3) = met, gre, gro
    of the evaluation before every update, met / gre / gro / gdsq of the last evaluation, kinds (update type per iteration),
    and states[k] = t before update k for k in `keep`."""
    G = links(g, dtype)
    cdt = G[0].dtype
    t = np.tile(np.eye(3, dtype=cdt), (lo.vol, 1, 1)) if t0 is None else cmat(t0, dtype).astype(cdt)
    dirs = list(dirs)
    eps, polish, its = 0.1, 0, 0
    hist, kinds, states = [], [], {}
    while True:
        gd = gradient(lo, G, t, dirs)
        met, gre, gro = metrics(lo, gd, t, len(dirs))
        gdsq = gre + gro
        polish = polish + 1 if gdsq <= gstop else 0
        if polish > 10 or its >= maxits:
            break
        if its in keep:
            states[its] = t.copy()
        hist.append((met, gre, gro))
        its += 1
        kind = 2 if polish > 0 else its % 2
        kinds.append(kind)
        if kind == 2:
            t, eps = line_min(lo, G, gd, t, dirs, eps, met)
        else:
            relax(lo, t, gd, kind, orf)
    info = {"iters": its, "hist": np.array(hist, dtype=dtype).reshape(-1, 3), "met": met, "gre": gre, "gro": gro, "gdsq": gdsq,
            "kinds": kinds, "states": states}
    return t, info


def plaq(lo, G):
    """the six plane averages of Re tr plaquette / 3"""
    out = []
    for mu in range(1, 4):
        for nu in range(mu):
            fmu, fnu = neighbours(lo, mu)[0], neighbours(lo, nu)[0]
            a = mul(G[mu], G[nu][fmu])
            b = mul(G[nu], G[mu][fnu])
            out.append((a * np.conj(b)).sum().real / (lo.vol * 3))
    return np.array(out)


def random_su3(lo, seed):
    """a random SU(3) matrix per site, (vol, 3, 3) complex: Gram-Schmidt of a Gaussian matrix, row 2 = conj(row 0 x row 1)"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((lo.vol, 2, 3)) + 1j * rng.standard_normal((lo.vol, 2, 3))
    r0 = a[:, 0] / np.linalg.norm(a[:, 0], axis=1)[:, None]
    r1 = a[:, 1] - np.sum(r0.conj() * a[:, 1], axis=1)[:, None] * r0
    r1 /= np.linalg.norm(r1, axis=1)[:, None]
    return np.stack([r0, r1, np.conj(np.cross(r0, r1))], axis=1)


def rotated_gauge(lo, g, seed):
    """the links g (vol, 4, 3, 3, 2) transformed by a random SU(3) field"""
    gt = gauge_transform(lo, links(g), random_su3(lo, seed))
    return np.ascontiguousarray(np.stack([rmat(m) for m in gt], axis=1))


# ---- the inputs and recorded CPU results the GPU tests share ----
SEED, ROT_SEED = 987654321, 11
COULOMB, LANDAU = (0, 1, 2), (0, 1, 2, 3)
LATS = ((8, 8, 8, 8), (4, 6, 10, 6))
# Iterations of get_gauge_fix_transform(orf = 1.8) on warm_rotated(lat), measured on the CPU.  tests/test_gaugefix_ref.py re-measures the
# 4x6x10x6 rows at gstop 1e-5 in every run and all rows, with the 8^4 yardsticks, under `pytest -m slow` (about two minutes).
# QEX's own self-test input (g.random transformed by t = g[0], gaugefix.nim:372-375; grandom_rotated below) was measured at 8^4, orf 1.8,
# gstop 1e-5: 910 iterations (Coulomb, met 0.676207) and 2057 (Landau, met 0.593078) -- GRANDOM_ITERS, re-measured under `-m slow`.
# It converges, but four to nine times slower than the warm start, so the GPU tests, which have a few seconds each, use the warm one.
GRANDOM_ITERS = {COULOMB: 910, LANDAU: 2057}
REF_ITERS = {
    ((8, 8, 8, 8), COULOMB, 1e-5): 183, ((8, 8, 8, 8), COULOMB, 1e-10): 437,
    ((8, 8, 8, 8), LANDAU, 1e-5): 228, ((8, 8, 8, 8), LANDAU, 1e-10): 561,
    ((4, 6, 10, 6), COULOMB, 1e-5): 239, ((4, 6, 10, 6), COULOMB, 1e-10): 631,
    ((4, 6, 10, 6), LANDAU, 1e-5): 345, ((4, 6, 10, 6), LANDAU, 1e-10): 857,
}
# Yardstick of the 40 pure-relax iterations (gstop = 0): how far the fp64 run of this file strays from its np.longdouble run,
# (history: max relative deviation of met, gre, gro over the 41 evaluations; t: max absolute deviation of an element), measured on
# the CPU (tests/test_gaugefix_ref.py re-measures the 4x6x10x6 rows).
YARDSTICK = {
    ((4, 6, 10, 6), COULOMB, 1.8): (4.679e-16, 2.004e-15), ((4, 6, 10, 6), COULOMB, 1.0): (2.017e-15, 1.637e-15),
    ((4, 6, 10, 6), LANDAU, 1.8): (2.972e-15, 2.138e-15), ((4, 6, 10, 6), LANDAU, 1.0): (6.564e-15, 2.001e-15),
    ((8, 8, 8, 8), COULOMB, 1.8): (7.455e-16, 2.124e-15), ((8, 8, 8, 8), COULOMB, 1.0): (7.777e-16, 1.897e-15),
    ((8, 8, 8, 8), LANDAU, 1.8): (2.516e-15, 2.104e-15), ((8, 8, 8, 8), LANDAU, 1.0): (2.516e-15, 2.431e-15),
}


def bound(yard):
    """the rule of tests/parity_log.py for a history compared with its reference: max(1e-12, 3 x yardstick)"""
    return max(1e-12, 3.0 * yard)


def warm_rotated(o, lat):
    """(lo, g): the oracle's gauge_warm(0.3) (RngMilc6, SEED) transformed by a random SU(3) field"""
    from qex_amd.layout import Layout

    lo, olo = Layout(list(lat)), o.Layout(list(lat))
    return lo, rotated_gauge(lo, o.gauge_warm(olo, 0.3, o.RngField(olo, o.RNG_MILC6, SEED)), ROT_SEED)


def full_history(info):
    return np.vstack([info["hist"], [[info["met"], info["gre"], info["gro"]]]])


def grandom_rotated(o, lat):
    """(lo, g): QEX's self-test input, the oracle's g.random (RngMilc6, SEED) transformed by t = g[0]"""
    from qex_amd.layout import Layout

    lo, olo = Layout(list(lat)), o.Layout(list(lat))
    G = links(o.gauge_random(olo, o.RngField(olo, o.RNG_MILC6, SEED)))
    return lo, np.ascontiguousarray(np.stack([rmat(m) for m in gauge_transform(lo, G, G[0])], axis=1))
