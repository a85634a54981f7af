"""Stout smearing (src/gauge/stoutsmear.nim) through libqexhip: the reference's names and argument order.

    newStoutSmear(l, alpha)             stoutsmear.nim:10-13
    ss.smear(gf, fl)                    stoutsmear.nim:15-34
    ss.inverse(gf, fl, rdf2req, ...)    stoutsmear.nim:36-89
    ss.smearDeriv(deriv, chain)         stoutsmear.nim:148-175

A StoutSmear object is one level.  The device keeps one chain per context (qexhip_stout_prepare); an object whose level is no
longer the resident one smears its input again before smearDeriv, so objects chain through host arrays as in
tests/base/tstoutderiv.nim:149-193.  stoutSmearGetForce is the n-level chain kept on the device, in the style of
HypCoefs.smearGetForce.  All arithmetic is in libqexhip.
"""
import ctypes as C

from ._lib import QexHipError, check, lib
from .staggered import _p


class StoutSmear:
    def __init__(self, ctx, alpha):
        self.ctx, self.alpha = ctx, float(alpha)
        self._gf = None          # the reference keeps a reference to its input (ss.gf = gf, :22): here a copy, taken when fl is not gf
        self._smeared = False
        self.diverging = False   # the last inverse() saw df^2 increase (the reference's warning, :81-83)

    def _prepare(self, g, fl):
        a = (C.c_double * 1)(self.alpha)
        check(lib().qexhip_stout_prepare(self.ctx._h, _p(g), a, 1, _p(fl)))
        self.ctx._stout_owner = self      # whose level the context's resident chain is

    def smear(self, gf, fl):
        """fl = exp(-alpha nc TAH(gf ds^+)) gf; fl may be gf (tstoutderiv.nim:22-23), after which smearDeriv is refused"""
        self._gf = None if fl is gf else gf.copy()
        self._smeared = True
        self._prepare(gf, fl)

    def smearDeriv(self, deriv, chain):
        """deriv = d/d(gf)^+ of what chain = d/d(fl)^+ is the derivative of; deriv may be chain"""
        if not self._smeared:
            raise QexHipError("StoutSmear.smearDeriv: call smear first")
        if self._gf is None:
            raise QexHipError("StoutSmear.smearDeriv: the level was smeared in place, its input links are gone (stoutsmear.nim:22)")
        if getattr(self.ctx, "_stout_owner", None) is not self or lib().qexhip_stout_force(self.ctx._h, _p(deriv), _p(chain)) != 0:
            # another level or chain took the device since, or the workspace was released: smear the kept input again
            self._prepare(self._gf, None)
            check(lib().qexhip_stout_force(self.ctx._h, _p(deriv), _p(chain)))

    def inverse(self, gf, fl, rdf2req=1e-24, maxIter=1000):
        """gf with smear(gf) = fl by fixed-point iteration from gf = fl; returns (iter, rdf2); gf and fl must be distinct"""
        it, r2, dv = C.c_int(0), C.c_double(0), C.c_int(0)
        check(lib().qexhip_stout_inverse(self.ctx._h, _p(fl), self.alpha, float(rdf2req), int(maxIter), _p(gf), C.byref(it), C.byref(r2),
                                         C.byref(dv)))
        self.diverging = bool(dv.value)
        return it.value, r2.value


def newStoutSmear(ctx, alpha):
    return StoutSmear(ctx, alpha)


def stoutSmear(ctx, g, alpha, fl):
    """one stout step without any state kept; g None = the resident links, fl None = the result replaces the resident links"""
    check(lib().qexhip_stout_smear(ctx._h, _p(g), float(alpha), _p(fl)))


def stoutSmearGetForce(ctx, g, fl, alphas):
    """Smear g (None: the resident links) with the levels `alphas` in order, into fl if given, and return the closure
    smearedForce(f, chain) = smearDeriv from the last level to the first; every level's state stays on the device until the
    closure's release() (or the next chain on this context).  smearedForce.gaugeForce(f, cplaq, crect, cadj) is smearedForce of
    tests/base/tstoutderiv.nim:137-143: the action's derivative on the smeared links, the chain, TAH(g f^+).  f None leaves a
    force on the device as MD source 1."""
    n = len(alphas)
    arr = (C.c_double * max(n, 1))(*[float(v) for v in alphas])
    check(lib().qexhip_stout_prepare(ctx._h, _p(g), arr, n, _p(fl)))
    ctx._stout_owner = None

    def smearedForce(f, chain):
        check(lib().qexhip_stout_force(ctx._h, _p(f), _p(chain)))

    def gaugeForce(f, cplaq=1.0, crect=0.0, cadj=0.0):
        check(lib().qexhip_stout_gauge_force(ctx._h, _p(f), float(cplaq), float(crect), float(cadj)))

    def release():
        check(lib().qexhip_stout_release(ctx._h))
        ctx._stout_owner = None

    smearedForce.gaugeForce, smearedForce.release = gaugeForce, release
    return smearedForce
