"""numpy restatement of src/gauge/stoutsmear.nim on host fields (vol, 4, 3, 3, 2) in the V=1 even-odd order: smear (:15-34),
inverse (:36-89), gaugeForceDeriv (:97-146), smearDeriv (:148-175), with expm1Deriv at scale 20 and polynomial order 4
(src/maths/matexp.nim:686-713, :100-117, called from matrixFunctions.nim:471-481), the smearTest0 pair of
tests/base/tstoutderiv.nim:90-117 and the differentiator of src/algorithms/numdiff.nim.  gaugeActionDeriv, gaugeAction1,
contractProjectTAH, exp and the site neighbours come from the oracle (o.gauge_deriv, o.gauge_action, o.force_projTAH,
o.gauge_exp_update = qo_exp per link, lo.neighbor).  The yardstick of tests/test_stout_ref.py, tests/test_gpu_stout.py and
tests/stout_rank_worker.py."""
import numpy as np

from oracle import oracle as o

NC = 3.0
# iterations the restated inverse takes on the reference's configuration (8^4, g.random + ten steps) at alpha = 0.02, rdf2req = 1e-24,
# measured and asserted by tests/test_stout_ref.py; the GPU tests hold the device to +-1 of it
INVERSE_ITERS = 16
# a step size at which the restated inverse reports "df^2 increased" within five iterations on that configuration (same test file)
DIVERGING_ALPHA = 0.5
C2, C3, C4 = 0.5, 1.0 / 6.0, 1.0 / 24.0      # matexp.nim:10-12


def cm(a):
    """(..., 3, 3, 2) -> (..., 3, 3) complex"""
    a = np.asarray(a, dtype=np.float64)
    return a[..., 0] + 1j * a[..., 1]


def rm(z):
    return np.ascontiguousarray(np.stack([z.real, z.imag], axis=-1))


def adj(m):
    return np.conj(np.swapaxes(m, -1, -2))


def tah(m):
    """projectTAH (matrixFunctions.nim:375-380)"""
    a = 0.5 * (m - adj(m))
    tr = np.einsum("...ii->...", a) / 3.0
    a = a.copy()
    for i in range(3):
        a[..., i, i] -= tr
    return a


_NBR = {}


def neighbours(lo):
    """fw[mu][s] = index of x+mu, bw[mu][s] = index of x-mu (lo.neighbor of the oracle's layout)"""
    key = tuple(lo.lat)
    if key not in _NBR:
        fw = np.array([[lo.neighbor(s, mu, 1) for s in range(lo.vol)] for mu in range(4)])
        bw = np.array([[lo.neighbor(s, mu, -1) for s in range(lo.vol)] for mu in range(4)])
        _NBR[key] = (fw, bw)
    return _NBR[key]


# ---- src/maths/matexp.nim ----
def expm1_poly4(m):
    """expm1Poly4 (:80-85)"""
    m2 = m @ m
    a = C4 * m2 + C3 * m + C2 * np.eye(3)
    return a @ m2 + m


def expm1(m, scale=20):
    """expm1 (:634-649)"""
    ms = m * (1.0 / float(1 << scale))
    r = expm1_poly4(ms)
    for _ in range(scale):
        r = r @ (r + 2.0 * np.eye(3))
    return r


def exp(m):
    """exp (:707-710; matrixFunctions.nim:436-449: scale 20, ekPoly, order 4)"""
    return expm1(m) + np.eye(3)


def expm1_poly4_deriv(m, w):
    """expm1Poly4Deriv (:100-117)"""
    md = adj(m)
    g = C4 * md
    f = g + C3 * np.eye(3)
    e = w @ f
    a = g @ w + e
    d = e @ md + C2 * w
    c = d @ md + w
    h = md @ a + d
    return md @ h + c


def exp_deriv(m, w, scale=20):
    """expDeriv (matrixFunctions.nim:471-481) = expm1Deriv (matexp.nim:686-705) with scale 20, ekPoly, order 4"""
    ms = m * (1.0 / float(1 << scale))
    e = expm1_poly4(ms)
    we = 0.5 * (w @ adj(e) + adj(e) @ w) + w
    for _ in range(2, scale + 1):
        e = e @ (e + 2.0 * np.eye(3))
        we = we + 0.5 * (we @ adj(e) + adj(e) @ we)
    return expm1_poly4_deriv(ms, we)


# ---- src/gauge/stoutsmear.nim ----
class StoutSmear:
    """newStoutSmear (:10-13): alpha and the fields smear leaves for smearDeriv"""

    def __init__(self, lo, alpha):
        self.lo, self.alpha = lo, float(alpha)
        self.gf = self.f = self.expaf = self.ds = None

    def smear(self, gf):
        """smear (:15-34): returns fl; gf, f, expaf, ds are kept"""
        lo = self.lo
        a = -self.alpha * NC
        gf = np.ascontiguousarray(gf)
        ds = o.gauge_deriv(lo, gf, 1.0)                       # :24
        f = ds.copy()
        o.force_projTAH(lo, f, gf, adj=True)                  # :28-31  t = TAH(gf ds^+)
        expaf = o.gauge_unit(lo)
        o.gauge_exp_update(lo, expaf, f, a)                   # :32-33  exp(alpha t)
        fl = gf.copy()
        o.gauge_exp_update(lo, fl, f, a)                      # :34     t gf
        self.gf, self.f, self.expaf, self.ds = gf.copy(), f, expaf, ds
        return fl

    def smear_deriv(self, chain):
        """smearDeriv (:148-175)"""
        a = -self.alpha * NC
        gf, f, expaf, c = cm(self.gf), cm(self.f), cm(self.expaf), cm(chain)
        d = a * exp_deriv(a * f, c @ adj(gf))                 # :168
        d, _ = gauge_force_deriv(self.lo, gf, d, cm(self.ds))   # :169
        d = d + adj(expaf) @ c                                # :175
        return rm(d)

    def inverse(self, fl, rdf2req=1e-24, max_iter=1000):
        """inverse (:36-89): returns (gf, iter, rdf2, increased) -- increased lists the iterations of the "df^2 increased" warning"""
        lo = self.lo
        a = self.alpha * NC                                   # :45
        fl = np.ascontiguousarray(fl)
        gf = fl.copy()                                        # :52
        f = np.zeros_like(fl)                                 # :53
        it, rdf2, df2o, increased = 0, 0.0, -1.0, []
        while it < max_iter:
            it += 1
            ds = o.gauge_deriv(lo, gf, 1.0)                   # :60
            t = ds
            o.force_projTAH(lo, t, gf, adj=True)              # :66-68
            df2 = float(((t - f) ** 2).sum())                 # :69
            f2 = float((t ** 2).sum())                        # :70
            f = t                                             # :71
            gf = fl.copy()
            o.gauge_exp_update(lo, gf, t, a)                  # :72-73
            rdf2 = df2 / f2                                   # :78
            if df2o >= 0 and df2o < df2:
                increased.append(it)                          # :81-83
            df2o = df2
            if rdf2 < rdf2req:                                # :87
                break
        return gf, it, rdf2, increased


def gauge_force_deriv(lo, gf, chain, f):
    """gaugeForceDeriv (:97-146) on complex (vol, 4, 3, 3) fields: returns (deriv, cg).
    Transporters (src/layout/shifts.nim:466-557): (t[nu] ^* y)(x) = gf_nu(x) y(x+nu), (td[nu] ^* y)(x) = gf_nu(x-nu)^+ y(x-nu);
    shiftExpr(t[mu].sb, ..., y[ix]) hands y(x+mu) to the expression as `it`."""
    fw, bw = neighbours(lo)
    t = tah(chain)                                            # :116-117
    deriv = t @ f                                             # :118
    cg = adj(t) @ gf                                          # :119
    cp = 1.0 / NC                                             # :128
    for mu in range(4):
        for nu in range(4):
            if nu == mu:
                continue
            xn, xm, xb = fw[nu], fw[mu], bw[nu]
            # :138-139  t[nu] ^* gf[mu] = gf_nu(x) gf_mu(x+nu); it = cg_nu(x+mu)
            deriv[:, mu] += cp * (gf[:, nu] @ gf[xn, mu]) @ adj(cg[xm, nu])
            # :140-141  t[nu] ^* cg[mu]; it = gf_nu(x+mu)
            deriv[:, mu] += cp * (gf[:, nu] @ cg[xn, mu]) @ adj(gf[xm, nu])
            # :142-143  ct[nu] ^* gf[mu]; it = gf_nu(x+mu)
            deriv[:, mu] += cp * (cg[:, nu] @ gf[xn, mu]) @ adj(gf[xm, nu])
            # :144  td[nu] ^* t[mu] ^* cg[nu] = gf_nu(x-nu)^+ [gf_mu(y) cg_nu(y+mu)](y = x-nu)
            inner = gf[:, mu] @ cg[xm, nu]
            deriv[:, mu] += cp * (adj(gf[:, nu]) @ inner)[xb]
            # :145  td[nu] ^* ct[mu] ^* gf[nu]
            inner = cg[:, mu] @ gf[xm, nu]
            deriv[:, mu] += cp * (adj(gf[:, nu]) @ inner)[xb]
            # :146  ctd[nu] ^* t[mu] ^* gf[nu]
            inner = gf[:, mu] @ gf[xm, nu]
            deriv[:, mu] += cp * (adj(cg[:, nu]) @ inner)[xb]
    return deriv, cg


# ---- tests/base/tstoutderiv.nim ----
def smear_test0(lo, ss, gf):
    """smearTest0 (:90-105): fl = exp(alpha t), no factor gf"""
    a = -ss.alpha * NC
    gf = np.ascontiguousarray(gf)
    ds = o.gauge_deriv(lo, gf, 1.0)
    f = ds.copy()
    o.force_projTAH(lo, f, gf, adj=True)
    fl = o.gauge_unit(lo)
    o.gauge_exp_update(lo, fl, f, a)
    ss.gf, ss.f, ss.ds = gf.copy(), f, ds
    return fl


def smear_test0_deriv(lo, ss, chain):
    """smearTest0Deriv (:107-117)"""
    a = -ss.alpha * NC
    d = a * exp_deriv(a * cm(ss.f), cm(chain))
    d, _ = gauge_force_deriv(lo, cm(ss.gf), d, cm(ss.ds))
    return rm(d)


def contract_project_tah(lo, g, f):
    """contractProjectTAH(g, f): f <- TAH(g f^+) (gaugeUtils.nim:389-398)"""
    f = np.ascontiguousarray(f).copy()
    o.force_projTAH(lo, f, np.ascontiguousarray(g), adj=True)
    return f


def addnoise(lo, x, p, g):
    """addnoise (:39-46): ng = exp(x p) g"""
    ng = np.ascontiguousarray(g).copy()
    o.gauge_exp_update(lo, ng, np.ascontiguousarray(p), float(x))
    return ng


def redot(p, f):
    return float((p * f).sum())


def chain_action(lo, alphas, g, cplaq=6.0):
    """smearedAction / smeared2Action / smeared3Action (:133-178): gaugeAction1 (plaq: cplaq) of the smeared links"""
    for a in alphas:
        g = StoutSmear(lo, a).smear(g)
    return o.gauge_action(lo, g, cplaq)


def chain_force(lo, alphas, g, cplaq=6.0):
    """smearedForce / smeared2Force / smeared3Force (:137-193)"""
    levels = []
    for a in alphas:
        ss = StoutSmear(lo, a)
        g_next = ss.smear(g if not levels else levels[-1][1])
        levels.append((ss, g_next))
    f = o.gauge_deriv(lo, levels[-1][1], cplaq)
    for ss, _ in reversed(levels):
        f = ss.smear_deriv(f)
    return contract_project_tah(lo, g, f)


def chain_deriv(lo, alphas, g, chain):
    """the smeared links and smearDeriv from the last level to the first of an arbitrary chain field (no projection)"""
    levels, cur = [], g
    for a in alphas:
        ss = StoutSmear(lo, a)
        cur = ss.smear(cur)
        levels.append(ss)
    f = chain
    for ss in reversed(levels):
        f = ss.smear_deriv(f)
    return cur, f


# ---- src/algorithms/numdiff.nim ----
def ndiff(f, x, dx, scale=2.0, ord_max=8):
    """ndiff (:17-58): Ridders' extrapolation of central differences; returns (derivative, error estimate)"""
    s2 = scale * scale
    A = []
    for _ in range(ord_max):
        A.append((f(x + dx) - f(x - dx)) * (0.5 / dx))
        dx /= scale
    b = s2
    c = 1.0 / (b - 1.0)
    for j in range(ord_max - 1, 1, -1):
        for i in range(j):
            A[i] = (A[i + 1] * b - A[i]) * c
        b *= s2
        c = 1.0 / (b - 1.0)
    a1, a0 = A[1], A[0]
    a = (a1 * b - a0) * c
    return a, max(abs(a - a0), abs(a - a1))


def del2(lo, u, g):
    """tstoutinverse.nim:39-51: sum |u g^+ - 1|^2 / (2 (nc^2 + 1) nd vol)"""
    d = cm(u) @ adj(cm(g)) - np.eye(3)
    return float((d.real ** 2 + d.imag ** 2).sum()) / float(2 * 10 * 4 * lo.vol)


def reference_config(lo, alpha, steps=10):
    """g.random, then `steps` in-place stout steps (tstoutderiv.nim:19-23, tstoutinverse.nim:22-26)"""
    g = o.gauge_random(lo)
    for _ in range(steps):
        g = StoutSmear(lo, alpha).smear(g)
    return g
