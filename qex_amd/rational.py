"""Partial-fraction rationals r(x) = f0 + sum_k alpha_k / (x + beta_k) for the rooted staggered action (host, numpy only).

The library applies such an r to M^+M with one multi-shift solve (Context.dev_rational_xx, Staggered.rationalXX,
ResidentMD.hisq_fforce_rational).  The coefficients are the caller's; rationalFit makes usable ones for x**power on [lo, hi]:
geometrically spaced poles, residues and f0 by linear least squares in the relative error, the two ends of the pole range scanned.
It is not a minimax (Remez) fit -- it reports the error it measured, and refuses a fit whose residues change sign, because only
residues of one sign keep r(M^+M) definite for every spectrum inside the range."""
import json

import numpy as np

GRID = 4001
_LO_FACTORS = np.geomspace(1e-3, 1.0, 13)
_HI_FACTORS = np.geomspace(1.0, 1e3, 13)


class Rational:
    def __init__(self, f0, alpha, beta):
        self.f0 = float(f0)
        self.alpha = np.array(alpha, dtype=np.float64).reshape(-1)
        self.beta = np.array(beta, dtype=np.float64).reshape(-1)
        if self.alpha.shape != self.beta.shape or self.alpha.size < 1:
            raise ValueError("Rational: %d residues, %d poles" % (self.alpha.size, self.beta.size))

    @property
    def nterm(self):
        return int(self.alpha.size)

    def eval(self, x):
        x = np.asarray(x, dtype=np.float64)
        return self.f0 + (self.alpha / (x[..., None] + self.beta)).sum(axis=-1)

    def to_json(self):
        # repr of a Python float round-trips exactly
        return json.dumps({"f0": self.f0, "alpha": [float(v) for v in self.alpha], "beta": [float(v) for v in self.beta]})

    @classmethod
    def from_json(cls, s):
        d = json.loads(s) if isinstance(s, str) else s
        return cls(d["f0"], d["alpha"], d["beta"])

    def __repr__(self):
        return "Rational(f0=%r, nterm=%d)" % (self.f0, self.nterm)


def grid(lo, hi):
    """the logarithmic grid on which fits are made and their errors measured"""
    return np.geomspace(float(lo), float(hi), GRID)


def max_rel_error(rat, power, lo, hi):
    x = grid(lo, hi)
    return float(np.abs(rat.eval(x) / x ** power - 1.0).max())


def _fit_poles(x, target, beta):
    # columns scaled by 1/target: the residual IS the relative error
    A = np.concatenate([np.ones((x.size, 1)), 1.0 / (x[:, None] + beta[None, :])], axis=1) / target[:, None]
    sol = np.linalg.lstsq(A, np.ones(x.size), rcond=None)[0]
    return Rational(sol[0], sol[1:], beta)


def rationalFit(power, lo, hi, nterm):
    """(Rational, max relative error against x**power on the 4001-point logarithmic grid of [lo, hi]).  Only fits whose residues
    all have the right sign (alpha > 0 for a negative power, alpha < 0 for a positive one) are candidates of the scan; ValueError
    if no pole range of the scan gives one."""
    power, lo, hi, nterm = float(power), float(lo), float(hi), int(nterm)
    if not (0.0 < lo < hi) or nterm < 1 or power == 0.0 or not -1.0 < power < 1.0:
        raise ValueError("rationalFit: 0 < lo < hi, nterm >= 1, 0 < |power| < 1")
    x = grid(lo, hi)
    target = x ** power
    want = 1.0 if power < 0 else -1.0
    best = None
    for a in _LO_FACTORS:
        for b in _HI_FACTORS:
            beta = np.geomspace(a * lo, b * hi, nterm) if nterm > 1 else np.array([np.sqrt(a * lo * b * hi)])
            rat = _fit_poles(x, target, beta)
            err = float(np.abs(rat.eval(x) / target - 1.0).max())
            if not np.all(want * rat.alpha > 0):
                continue                     # a fit with mixed signs is never a candidate
            if best is None or err < best[1]:
                best = (rat, err)
    if best is None:
        raise ValueError("rationalFit(%g, [%g, %g], %d): the residues are not all %s -- r(M^+M) would not be definite; use fewer "
                         "terms or a narrower range" % (power, lo, hi, nterm, "positive" if want > 0 else "negative"))
    return best
