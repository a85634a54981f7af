"""The three mixed-precision CG iterations restated in numpy, kernel by kernel, for the step-by-step checks of
tests/test_sloppy_ref.py (the model itself, CPU) and tests/test_gpu_sloppy_steps.py (the library against the model).

  single()  SloppySingle (dslash_f32.hip k_slp_*, host loop solve_xx_sloppy_dev) and, with fmt = a 16-bit link format, SloppyHalf
            with half = 1 (dslash_half.hip k_slph_*, solve_xx_half_dev)
  multi()   phase 1 of the fp32 multi-shift solve (multishift_f32.hip k_msf_*, solve_xx_multi_sloppy_dev)

Storage is float32 for r_s, p_s, Ap_s, x_s (16-bit: the site format of test_half_pack for r_s, p_s, Ap_s; x_s stays float32), every
scalar is a double, alpha / beta / the zeta coefficients are cast to float32 where the kernels cast them, and a float32 fma is
float32(float64(a) * x + y).  The fp32 operator is the oracle's stagD2xx on the fp64 links rounded to float32; the 16-bit operator is
half_ref.Model.  What the model does NOT reproduce -- fp32 links, the fp32 accumulation of the two sweeps, the reduction order -- is
stood for by `Noise`: an estimate, see DESIGN.md "Engineering checks".

A solve cut at maxits = k forces a reliable update at step k and returns x_k with its true residual; single() walks the iteration
once and forks that forced update at every k.  No device needed."""
import functools
import types

import numpy as np

from half_ref import Model, quant_sites

DELTA = 0.1            # SLP_DELTA (qexhip_internal.h)
F32, F64 = np.float32, np.float64
WRONG_SINGLE = ("beta_units", "no_rebuild", "no_zero")
WRONG_MULTI = ("no_unit_conversion", "zeta_stuck", "no_pending_last")


def relerr(a, ref):
    return float(np.linalg.norm(np.asarray(a, F64) - ref) / np.linalg.norm(ref))


class Noise:
    """The roundings the model leaves out, as random perturbations: every component of a computed Ap (and, 16-bit, of every vector
    in front of a pack) relatively by a normal deviate of standard deviation 2^-22, every float32 coefficient by -1, 0 or +1 ulp."""

    def __init__(self, seed, sd=2.0 ** -22):
        self.rng, self.sd = np.random.default_rng(seed), sd

    def vec(self, v):
        return v * (1.0 + self.sd * self.rng.standard_normal(v.shape))

    def ulp(self, a):
        a = F32(a)
        step = int(self.rng.integers(-1, 2))
        return a if step == 0 else np.nextafter(a, F32(np.inf if step > 0 else -np.inf))


class Margin:
    """the smallest relative distance of any decision from its threshold"""

    def __init__(self):
        self.v = np.inf

    def lt(self, a, b):
        """a < b, recorded"""
        d = max(abs(a), abs(b))
        if d > 0:
            self.v = min(self.v, abs(a - b) / d)
        return a < b


class Problem:
    """one right-hand side on one parity: the fp64 operator (the oracle's), the iteration's operator, the storage format"""

    def __init__(self, o, lo, fat, lng, b, mass, par_even, fmt=None, store=F32):
        self.o, self.lo, self.fat, self.lng = o, lo, fat, lng
        self.h = lo.vol // 2
        self.sl = slice(0, self.h) if par_even else slice(self.h, 2 * self.h)
        self.par_even, self.m2 = par_even, mass * mass
        self.b = np.array(b[self.sl], dtype=F64)
        self.half = fmt is not None
        self.store = store
        self.model = Model(o, lo, fat, lng, fmt) if self.half else None

    def full(self, v):
        f = np.zeros((self.lo.vol, 3, 2))
        f[self.sl] = v
        return f

    def A64(self, x, m2=None):
        return self.o.stagD2xx(self.lo, self.fat, self.lng, self.full(x), self.m2 if m2 is None else m2, self.par_even)[self.sl]

    def put(self, v, noise=None):
        """v (float64 values of an fp32 computation) as stored: float32, or the 16-bit site format"""
        if self.half:
            return quant_sites(noise.vec(v) if noise else v)
        return v.astype(self.store)

    def A(self, p, noise=None):
        """the iteration's operator on a stored vector, as stored"""
        if self.half:
            return self.model.op_xx(self.full(p), self.m2, self.par_even, noise.vec if noise else None)[self.sl]
        r = self.A64(np.asarray(p, F64))
        return (noise.vec(r) if noise else r).astype(self.store)


def _fma(a, x, y, dt=F32):
    """fmaf(a, x, y) of float32 operands (dt = float64: the same in double, for the comparison with the oracle's CG)"""
    return (F64(a) * np.asarray(x, F64) + np.asarray(y, F64)).astype(dt)


def _coef(v, dt, noise):
    """a double cast to float32 where a kernel casts it (float64 storage: kept, for the comparison with the oracle's CG)"""
    if noise:
        return noise.ulp(v)
    return F32(v) if dt is F32 else F64(v)


def _dot(a, b):
    return float(np.sum(np.asarray(a, F64) * np.asarray(b, F64)))


def _slp_init(P, r2req, maxits):
    s = types.SimpleNamespace()
    s.b2 = _dot(P.b, P.b)
    s.r2stop = r2req * s.b2
    s.r2t = s.b2
    s.maxits = maxits
    s.done = not (0 < maxits and s.r2t > s.r2stop)
    s.sigma = 1.0 if s.done else np.sqrt(s.r2t)
    s.sigma_p = s.sigma
    s.r2s = s.r2s_old = s.maxr2s = 1.0
    s.conv, s.first, s.upd, s.k, s.nupd = True, True, False, 0, 0
    return s


def _slp_close(s, r2, mg, updates):
    s.k += 1
    s.r2s_old, s.sigma_p = s.r2s, s.sigma
    s.r2s = r2
    s.maxr2s = max(s.maxr2s, r2)
    due = mg.lt(r2, DELTA * DELTA * s.maxr2s)
    due = (not mg.lt(s.r2stop, r2 * s.sigma * s.sigma)) or due
    due = (due and updates) or s.k >= s.maxits
    s.upd = s.upd or due
    s.conv = s.first = False


def _slp_rclose(s, r2t, mg):
    s.r2t = r2t
    s.nupd += 1
    s.upd = False
    if not mg.lt(s.r2stop, r2t) or s.k >= s.maxits:
        s.done = True
    else:
        s.r2s = 1.0
        s.sigma = np.sqrt(r2t)
        s.maxr2s = 1.0
        s.conv = True
        if not s.r2s_old > 0:
            s.first = True


def single(P, r2req, K, every, noise=None, updates=True, wrong=None, maxits=None):
    """SloppySingle / 16-bit SloppyHalf on problem P.  maxits None: the iteration runs on past K, and the result holds, for
    k = 1..K, what a solve cut at maxits = k returns: x[k-1], r2[k-1] (true |b - A x_k|^2 / |b|^2), nupd[k-1].  maxits given: that
    solve itself, literally (x, r2, nupd of length 1; `its` its iteration count).  Also update_steps, margin, r2s (the iteration's
    own |r_s|^2 sigma^2 / b2 after every step)."""
    assert wrong is None or wrong in WRONG_SINGLE
    dt = P.store
    fork = maxits is None
    s = _slp_init(P, r2req, 1 << 30 if fork else maxits)
    mg = Margin()
    x, r = np.zeros_like(P.b), P.b.copy()
    xs = np.zeros(P.b.shape, dt)
    rs = ps = None
    out = types.SimpleNamespace(x=[], r2=[], nupd=[], update_steps=[], r2s=[], its=0)
    n = K if fork else maxits
    k = 0
    while not s.done and k < n:
        # k_slp_xpay / k_slph_xpay
        beta = (s.r2s * s.sigma) / (s.r2s_old * s.sigma_p)
        if wrong == "beta_units":
            beta = s.r2s / s.r2s_old
        beta = _coef(beta, dt, noise)
        if s.conv and not (wrong == "no_rebuild" and rs is not None):
            rs = P.put((r / s.sigma).astype(dt).astype(F64), noise)
        ps = rs.copy() if s.first else P.put(_fma(beta, ps, rs, dt).astype(F64), noise)
        # the two sweeps, <p, Ap> in double
        Ap = P.A(ps, noise)
        pAp = _dot(ps, Ap)
        # k_slp_update / k_slph_update
        alpha = s.r2s / pAp
        alpha = _coef(alpha, dt, noise)
        xs = _fma(alpha, ps, xs, dt)
        rs = P.put(_fma(-alpha, Ap, rs, dt).astype(F64), noise)
        _slp_close(s, _dot(rs, rs), mg, updates)
        out.r2s.append(s.r2s * s.sigma * s.sigma / s.b2)
        k += 1
        posted = k % every == 0 or k >= s.maxits
        xk = x + s.sigma * xs.astype(F64)                      # k_slp_flush, of this step or forced by a cut here
        rk = P.b - P.A64(xk)
        if fork:
            out.x.append(xk)
            out.r2.append(_dot(rk, rk) / s.b2)
            out.nupd.append(s.nupd + 1)
        if posted and s.upd:
            x, r = xk, rk
            if wrong != "no_zero":
                xs = np.zeros_like(xs)
            _slp_rclose(s, _dot(rk, rk), mg)
            out.update_steps.append(k)
    if not fork:
        out.x, out.r2, out.nupd = [x], [s.r2t / s.b2], [s.nupd]
    out.its, out.margin = s.k, mg.v
    return out


def multi(P, shifts, r2req, maxits, every, noise=None, updates=True, wrong=None):
    """phase 1 of the fp32 multi-shift solve: shifts[0] = the base mass (P's), shifts[k] = sigma_k.  Returns x (per shift), its, nupd,
    update_steps, margin, r2 (the base system's true |r|^2 / b2 as returned), r2s (the iteration's own residual after every step)."""
    assert wrong is None or wrong in WRONG_MULTI
    dt = P.store
    nm = len(shifts)
    sg_k = [0.0] + [float(v) for v in shifts[1:]]
    s = _slp_init(P, r2req, maxits)
    mg = Margin()
    sg0 = s.sigma                                              # k_msf_init
    inv = 1.0 / sg0
    r = P.b.copy()
    x = [np.zeros_like(P.b) for _ in range(nm)]
    rs = (inv * P.b).astype(dt)                                # k_msf_start
    ps = [rs.copy() for _ in range(nm)]
    xs = [np.zeros(P.b.shape, dt) for _ in range(nm)]
    zi, zim1 = [1.0] * nm, [1.0] * nm
    alphaim1, betaim1 = -1.0, 0.0
    out = types.SimpleNamespace(update_steps=[], r2s=[])
    k = 0
    while not s.done and k < maxits:
        Ap = P.A(ps[0], noise)
        pAp = _dot(ps[0], Ap)
        # k_msf_base
        u = 1.0 if wrong == "no_unit_conversion" else (s.sigma * s.sigma) / (sg0 * sg0)
        r2i = s.r2s * u
        alpha = r2i / pAp if pAp != 0.0 else 0.0
        alpha_f = _coef(alpha, dt, noise)
        if s.conv:
            rs = (inv * r).astype(dt)
        xs[0] = _fma(alpha_f, ps[0], xs[0], dt)
        rs = _fma(-alpha_f, Ap, rs, dt)
        r2n = _dot(rs, rs)
        # k_msf_close
        beta = r2n / r2i if r2i != 0.0 else 0.0
        itn = s.k + 1
        cont = itn < s.maxits
        axz, zip1f, bzz = [None] * nm, [None] * nm, [None] * nm
        for j in range(1, nm):
            zip1d = alpha * betaim1 * (zim1[j] - zi[j]) + zim1[j] * alphaim1 * (1.0 + sg_k[j] * alpha)
            zip1 = zi[j] * zim1[j] * alphaim1 / zip1d if zip1d != 0.0 else 0.0
            zr = zip1 / zi[j] if zi[j] != 0.0 else 0.0
            cf = [alpha * zr, zip1, beta * zr * zr]
            axz[j], zip1f[j], bzz[j] = [_coef(c, dt, noise) for c in cf]
            if cont and wrong != "zeta_stuck":
                zim1[j], zi[j] = zi[j], zip1
        beta_f = _coef(beta, dt, noise)
        alphaim1, betaim1 = alpha, beta
        _slp_close(s, r2n / u, mg, updates)
        out.r2s.append(r2n * sg0 * sg0 / s.b2)
        # k_msf_update
        if cont:
            ps[0] = _fma(beta_f, ps[0], rs, dt)
        for j in range(1, nm):
            if cont or wrong != "no_pending_last":
                xs[j] = _fma(axz[j], ps[j], xs[j], dt)
            if cont:
                zr_ = (F64(zip1f[j]) * rs.astype(F64)).astype(dt)
                ps[j] = _fma(bzz[j], ps[j], zr_, dt)
        k += 1
        if (k % every == 0 or k >= maxits) and s.upd:
            for j in range(nm):                                # k_msf_flush
                x[j] = x[j] + sg0 * xs[j].astype(F64)
                xs[j] = np.zeros_like(xs[j])
            r = P.b - P.A64(x[0])
            _slp_rclose(s, _dot(r, r), mg)
            out.update_steps.append(k)
    out.x, out.its, out.nupd, out.margin, out.r2 = x, s.k, s.nupd, mg.v, s.r2t / s.b2
    return out


def shifted_r2(P, shifts, x):
    """the oracle's |b - A_k x_k|^2 / |b|^2 of every shift (A_k = A_0 + shifts[k]: stagD2xx at m0^2 + shifts[k] / 4)"""
    b2 = _dot(P.b, P.b)
    res = []
    for j, xj in enumerate(x):
        rj = P.b - P.A64(xj, P.m2 + (0.25 * shifts[j] if j else 0.0))
        res.append(_dot(rj, rj) / b2)
    return res


def ensemble(run, nseeds=8, seed0=1000):
    """run(noise) -> a model result.  Returns (the unperturbed result, sens, spread): per returned x the largest relative deviation
    over the seeds from the unperturbed one, and the same for r2 (None where the result has no list of r2)."""
    ref = run(None)
    sens = np.zeros(len(ref.x))
    spread = np.zeros(len(ref.x)) if isinstance(ref.r2, list) else None
    for i in range(nseeds):
        got = run(Noise(seed0 + i))
        assert (got.its, got.nupd, got.update_steps) == (ref.its, ref.nupd, ref.update_steps), "the noise moved the update schedule"
        for j in range(len(ref.x)):
            sens[j] = max(sens[j], relerr(got.x[j], ref.x[j]))
            if spread is not None:
                spread[j] = max(spread[j], abs(got.r2[j] / ref.r2[j] - 1.0))
    return ref, sens, spread


# ---- the cases' inputs ---------------------------------------------------------------------------------------------------
SEED = 987654321
# Seeds chosen so that no decision of any case comes within 1e-3 of its threshold (the margin test_gpu_sloppy_steps.py asserts): with
# SEED the odd-parity Gaussian ladder on 4.6.10.6 Naik links at sloppy_check 1 passes one at 7e-4.
CASE_SEED = {((4, 6, 10, 6), "naik"): 12345}
KINDS = {"random": ("random", False, 1), "warm": ("warm", False, 1), "naik": ("random", True, 1), "scaled": ("scaled", False, 0)}


@functools.lru_cache(maxsize=None)
def inputs(lat, kind, source):
    """(oracle, layout, fat, lng, b, the link format of the sloppy copies) as tests/test_gpu_half.py builds them; source "point": one
    nonzero site on each parity, every other site exactly zero"""
    from oracle import oracle as o

    o.build()
    base, naik, fmt = KINDS[kind]
    lo = o.Layout(list(lat))
    rf = o.RngField(lo, o.RNG_MILC6, CASE_SEED.get((lat, kind), SEED))
    if base == "scaled":                               # rows not unitary: 18 reals
        fat = 1.01 * o.gauge_warm(lo, 0.5, rf)
        o.rephase(lo, fat)
        lng = None
    else:
        gen = (lambda: o.gauge_warm(lo, 0.5, rf)) if base == "warm" else (lambda: o.gauge_random(lo, rf))
        fat = gen()
        o.rephase(lo, fat)
        lng = None
        if naik:
            lng = gen()
            o.rephase(lo, lng)
    b = o.vector_gaussian(lo, rf)
    if source == "point":
        b = np.zeros_like(b)
        b[0, 0, 0] = 1.0
        b[lo.vol // 2 + 3, 1, 0] = 1.0
    for a in (fat, lng, b):
        if a is not None:
            a.setflags(write=False)
    return o, lo, fat, lng, b, fmt


# ---- the cases, computed once per process -----------------------------------------------------------------------------------
R2REQ_LADDER = 1e-30          # a ladder of cut solves never stops on its tolerance
MULTI_MASSES = (0.5, 0.7, 1.0, 1.5)


def shifts_of(masses):
    return [masses[0]] + [4.0 * (m * m - masses[0] ** 2) for m in masses[1:]]      # stagSolve.nim:391-394


@functools.lru_cache(maxsize=None)
def problem(lat, kind, source, par_even, half, mass):
    o, lo, fat, lng, b, fmt = inputs(lat, kind, source)
    return Problem(o, lo, fat, lng, b, mass, par_even, fmt=fmt if half else None)


@functools.lru_cache(maxsize=16)                      # (a ladder holds K vectors: the GPU module walks ~170 of them, each once)
def single_case(lat, kind, source, par_even, half, mass, K, every):
    """(the model's ladder k = 1..K, sens_k, the spread of r2_k) of one case"""
    P = problem(lat, kind, source, par_even, half, mass)
    return ensemble(lambda nz: single(P, R2REQ_LADDER, K, every, noise=nz))


@functools.lru_cache(maxsize=None)
def multi_case(lat, kind, source, par_even, r2req, every, maxits=5000, masses=MULTI_MASSES):
    """(the model's phase 1, sens per shift, the oracle's |b - A_k x_k|^2 / |b|^2 per shift) of one case"""
    P = problem(lat, kind, source, par_even, False, masses[0])
    sh = shifts_of(masses)
    ref, sens, _ = ensemble(lambda nz: multi(P, sh, r2req, maxits, every, noise=nz))
    return ref, sens, shifted_r2(P, sh, ref.x)
