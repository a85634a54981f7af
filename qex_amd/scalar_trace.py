"""Stochastic estimate of the scalar-density trace Tr (D+m)^-1(x,x) (disconnected pbp): the host mirror of

    the main program of                src/observables/scalarTrace.nim:140-223
    DilutionKind, Dilution, dilution, parseDilution   src/algorithms/dilution.nim:3-21,47-64

Everything between the noise fill and the per-timeslice table stays on the device: one noise fill (RngField.dev_*_vector), then for
every group of up to `batch` (<= 4) dilution patterns one qexhip_dev_dilute, one lock-step batched solve (qexhip_dev_solve_batch or
its mixed-precision variant) and one qexhip_dev_trace_accum into a resident complex site field; qexhip_dev_cfield_slices sums it per
time slice.  The accumulation adds pattern after pattern in the reference's order (t outer, dl inner) whatever the grouping, so the
trace does not depend on `batch`.
"""
import enum
import math
import time
from collections import namedtuple


class DilutionKind(enum.IntEnum):
    dkEvenOdd = 0
    dkCorners3D = 1

    @property
    def high(self):
        return 1 if self == DilutionKind.dkEvenOdd else 7

    def __str__(self):
        return "EO" if self == DilutionKind.dkEvenOdd else "CORNER"


class Dilution(namedtuple("Dilution", "kind idx")):
    def __str__(self):
        return ("EvenOdd %d" if self.kind == DilutionKind.dkEvenOdd else "Corners3D %d") % self.idx


def dilution(dl):
    """iterator dilution (dilution.nim:47-56): the patterns of a kind, 0..high"""
    dl = DilutionKind(dl)
    for i in range(dl.high + 1):
        yield Dilution(dl, i)


def parseDilution(dl):
    if dl == "EO":
        return DilutionKind.dkEvenOdd
    if dl == "CORNER":
        return DilutionKind.dkCorners3D
    raise ValueError("unsupported dilution type: %s" % (dl,))


_NOISE = {"Z4": "dev_z4_vector", "Z2": "dev_z2_vector", "U1": "dev_u1_vector", "Gauss": "dev_gaussian_vector"}


def scalarTrace(stag, lo, rng, mass, r2req, maxits=100000, num_stoch=1, source_type="Z4", dilute_type="EO", improved_trace=True,
                t_offset=0, sloppy=0, batch=4, out=print, deflate=None, nev=None, lma=False):
    """scalarTrace.nim:146-218 on resident fields.  stag: the operator (its context holds the links); lo: the rank-local Layout and
    t_offset its first global t; rng: the rank's RngMilc6 RngField (seeded by global site, so every partition draws the same noise).
    For each of num_stoch noise sources of source_type (Z4, Z2, U1, Gauss) the source is diluted in time and dilute_type ("EO",
    "CORNER" or a DilutionKind), every diluted source is solved to r2req, and
        trce += mass * phi.dot phi   (improved_trace)      or      trce += src.dot phi,
    scaled by 1/nc at the end.  Returns (traces, ests, stats): per source the trace of the local lattice as a (vol, 2) array in host
    site order and est[t] = Re sum_{x in slice t} trce / spatial volume over the GLOBAL t; stats = {"solve_s", "contract_s",
    "noise_s", "log_s", "iterations", "updates"} (seconds in the batched solves; in dilution, accumulation, scaling and slice sums;
    in the noise fill; in the norms of the log lines; iterations and reliable updates per pattern and source).
    sloppy = 1 (or 2) solves in mixed precision (one rank; t-sharded with the context option "batch_ranks" = 1
    on every rank).  deflate = an EigBasis of the operator's even sites: every batch is
    deflated from it with its leading nev vectors (None: deflate.nconv), the odd-parity patterns included.  out receives the reference's log lines (None: none, and the
    norms they print are not computed).
    lma = True (needs deflate=): low-mode averaging, an extension the reference does not have.  With P the orthogonal projector onto
    the leading nev modes (v_i, 0) and their odd partners (0, D_oe v_i / sqrt(lambda_i)), Q = 1 - P and L(x) the site diagonal of
    P (D+m)^-1 (EigBasis.lowmode_diag: exact, no noise), the trace becomes
        trce = L + sum_d mass * |Q phi_d|^2   (improved_trace)      or      trce = L + sum_d src_d.dot Q phi_d.
    L is computed once; the solves are exactly those of lma = False (same bits, iterations and updates), each batch is followed by
    EigBasis.project_out, and L is added after the last pattern.  Both forms have the expectation of the plain estimator when the
    eigenpairs are exact; with eigenvectors of finite residual P is still an orthogonal projector but no longer commutes with D, and
    the estimate carries a bias of the order of the eigenvector residuals.  stats gains "lowmode_s", "project_s", "low_trace" (L/nc
    as a (vol, 2) array) and "low_est" (its slice table, as est).  The "dest norm2" log lines are those of the unprojected solutions."""
    ctx = stag.ctx
    if list(lo.lat) != list(ctx.lat):
        raise ValueError("lo is not the layout of the context's local lattice")
    if int(t_offset) != ctx.lat[3] * ctx.rank_coord[3]:
        raise ValueError("t_offset = %d is not the first global t of the context's slab" % t_offset)
    dk = dilute_type if isinstance(dilute_type, DilutionKind) else parseDilution(dilute_type)
    if source_type not in _NOISE:
        raise ValueError("Invalid noise type %s." % (source_type,))
    defl = {} if deflate is None and nev is None else {"deflate": deflate, "nev": nev}
    if lma and deflate is None:
        raise ValueError("lma = True needs deflate= (an EigBasis of the operator's even sites)")
    batch = int(batch)
    if not 1 <= batch <= 4:
        raise ValueError("batch = %d, must be 1..4" % batch)
    nt = ctx.lat[3] * ctx.rank_geom[3]
    spatv = ctx.lat[0] * ctx.lat[1] * ctx.lat[2]
    nc = 3
    scale = 1.0 / math.sqrt(2.0) if source_type == "Gauss" else 1.0
    say = out if out is not None else (lambda s: None)
    patterns = [(t, dl) for t in range(nt) for dl in dilution(dk)]
    fields, trce, low = [], None, None
    stats = {"solve_s": 0.0, "contract_s": 0.0, "noise_s": 0.0, "log_s": 0.0, "iterations": [], "updates": []}
    traces, ests = [], []
    try:
        eta = ctx.field_new()
        fields.append(eta)
        tmps = [ctx.field_new() for _ in range(batch)]
        phi = [ctx.field_new() for _ in range(batch)]
        fields += tmps + phi
        trce = ctx.cfield_new()
        if lma:
            from .staggered import _deflate_args

            nlow = _deflate_args(deflate, nev, None)
            t0 = time.perf_counter()
            low = ctx.cfield_new()
            deflate.lowmode_diag(nlow, mass, low)
            ctx.sync()
            stats["lowmode_s"] = time.perf_counter() - t0
            stats["project_s"] = 0.0
        for i in range(num_stoch):
            ctx.cfield_zero(trce)
            say("Generating a %s noise source." % source_type)
            t0 = time.perf_counter()
            getattr(rng, _NOISE[source_type])(ctx, eta)
            stats["noise_s"] += time.perf_counter() - t0
            if out is not None:
                t0 = time.perf_counter()
                say("noise norm2: %r" % (scale * scale * ctx.dev_norm2(eta),))
                stats["log_s"] += time.perf_counter() - t0
            its_src, upd_src = [], []
            for k0 in range(0, len(patterns), batch):
                grp = patterns[k0:k0 + batch]
                n = len(grp)
                t0 = time.perf_counter()
                ctx.dev_dilute(tmps[:n], eta, int(dk), [dl.idx for _, dl in grp], [t for t, _ in grp], scale)
                ctx.sync()
                t1 = time.perf_counter()
                if sloppy:
                    its, _, nup = ctx.dev_solve_batch(phi[:n], tmps[:n], [mass] * n, r2req, maxits, sloppy=sloppy, **defl)
                else:
                    its, _ = ctx.dev_solve_batch(phi[:n], tmps[:n], [mass] * n, r2req, maxits, **defl)
                    nup = [0] * n
                t2 = time.perf_counter()
                stats["solve_s"] += t2 - t1
                if lma:
                    if out is not None:
                        dest2 = [ctx.dev_norm2(phi[j]) for j in range(n)]
                        stats["log_s"] += time.perf_counter() - t2
                        t2 = time.perf_counter()
                    deflate.project_out(nlow, phi[:n])
                    ctx.sync()
                    stats["project_s"] += time.perf_counter() - t2
                    t2 = time.perf_counter()
                if improved_trace:
                    ctx.dev_trace_accum(trce, phi[:n], phi[:n], mass)
                else:
                    ctx.dev_trace_accum(trce, tmps[:n], phi[:n], 1.0)
                t3 = time.perf_counter()
                stats["contract_s"] += (t1 - t0) + (t3 - t2)
                its_src += its
                upd_src += nup
                if out is not None:
                    for j in range(n):
                        say("src norm2: %r" % (ctx.dev_norm2(tmps[j]),))
                        say("dest norm2: %r" % (dest2[j] if lma else ctx.dev_norm2(phi[j]),))
                        say("Computing the improved trace." if improved_trace else "Computing the unimproved trace.")
                    stats["log_s"] += time.perf_counter() - t3
            t0 = time.perf_counter()
            if lma:
                ctx.cfield_axpy(trce, 1.0, low)
            ctx.cfield_scale(trce, 1.0 / nc)
            sl = ctx.dev_cfield_slices(trce)
            stats["contract_s"] += time.perf_counter() - t0
            est = sl[:, 0] / float(spatv)
            for t in range(nt):
                say("initsrc %d timeslice %d pbp %r" % (i, t, float(est[t])))
            traces.append(ctx.cfield_download(trce))
            ests.append(est)
            stats["iterations"].append(its_src)
            stats["updates"].append(upd_src)
        if lma:
            ctx.cfield_scale(low, 1.0 / nc)
            stats["low_trace"] = ctx.cfield_download(low)
            stats["low_est"] = ctx.dev_cfield_slices(low)[:, 0] / float(spatv)
        return traces, ests, stats
    finally:
        for fid in fields:
            ctx.field_free(fid)
        if trce is not None:
            ctx.cfield_free(trce)
        if low is not None:
            ctx.cfield_free(low)
