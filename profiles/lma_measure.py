#!/usr/bin/env python3
"""The numbers of DESIGN.md section 4 "Low-mode averaging", measured in one session on the MI355X (32^4 unless -lat is given):

  A  the box's copy bandwidth (k_copy16 of libqexhip_tune, 1 GiB); then, on a basis of -nev Gaussian vectors, one
     EigBasis.block_norm2_accum over all of them against the chain it replaces (-nev times get_vector + dev_trace_accum): host clock
     around -reps calls that end in a synchronise, -rounds rounds, median and min .. max of the rounds' means.  Bytes of the kernel:
     48 B per site and vector, 16 B per site for the cfield.
  B  HISQ fat + Naik links (warm 0.3, seed 987654321) and -nev pairs (nvecs = 2 nev, abserr = 1e-8) as
     profiles/deflated_batch_measure.py computes them.
  C  per mass (0.1 and 0.01 sqrt(2)): the premises of the estimator at this size (both sum rules of L; m |M^-1 (v_i, 0)|^2 against
     m/(m^2 + lambda_i) for the first and the last mode, through the solve; <P phi, Q phi> / |phi|^2 and the change under a second
     projection on a Gaussian field), then EigBasis.lowmode_diag and EigBasis.project_out of
     a batch of four, the same clock.
  D  per mass and per seed of -seeds: -num_stoch Z4 / EO noise sources (r2req = 1e-18, improved trace, batches of four, deflated,
     -sloppy) from the same seed without and with lma: wall seconds per source, the per-source volume-averaged pbp of both arms,
     their paired difference (mean, standard error, and each source's in units of the exact low-mode part), and the sample variance
     over the sources of the volume-averaged pbp and of est[t] (summed over t).  The plain / LMA variance ratio comes with the
     16 % .. 84 % interval of a paired bootstrap over the sources (2000 resamples), its sampling uncertainty.  Last, the paired
     difference over the sources of all seeds: the two arms have the same expectation, so its mean must be compatible with 0.

    python3 profiles/lma_measure.py [-lat 32 32 32 32] [-skip A]      (one JSON line per measurement on stdout)"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import qex_amd as q  # noqa: E402
from qex_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("-lat", type=int, nargs=4, default=[32, 32, 32, 32])
ap.add_argument("-skip", type=str, default="")
ap.add_argument("-nev", type=int, default=64)
ap.add_argument("-degree", type=int, default=32)
ap.add_argument("-r2req", type=float, default=1e-18)
ap.add_argument("-sloppy", type=int, default=1)
ap.add_argument("-num_stoch", type=int, default=16)
ap.add_argument("-seeds", type=int, nargs="+", default=[987654321, 20261021, 4242])
ap.add_argument("-rounds", type=int, default=5)
ap.add_argument("-reps", type=int, default=10)
a = ap.parse_args()
lat = a.lat
vol = int(np.prod(lat))
SEED = 987654321


def out(**kw):
    print(json.dumps(kw), flush=True)


def stats(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


ctx = q.Context(lat)
out(what="device", info=ctx.info(), sites=vol)
qlo = q.Layout(lat)
rng = q.RngField(lat, q.RngMilc6, SEED)
g = rng.warm(0.3)
q.rephase(qlo, g)


def clock(fn):
    """mean milliseconds of fn: one warm-up call, then -rounds rounds of -reps calls, each round between two synchronises"""
    fn()
    ctx.sync()
    ms = []
    for _ in range(a.rounds):
        t = time.perf_counter()
        for _ in range(a.reps):
            fn()
        ctx.sync()
        ms.append(1e3 * (time.perf_counter() - t) / a.reps)
    return ms


if "A" not in a.skip:
    T = _lib.tune_lib()
    gbs = C.c_double(0)
    T.qexhip_tune_stream(ctx._h, 1, 1024, 2048, 5, C.byref(gbs))
    copy = gbs.value
    out(what="copy_bandwidth", kernel="k_copy16 1 GiB", gbytes_per_s=copy)
    q.newStag(ctx, g)
    B0 = q.EigBasis(ctx, a.nev)
    ws = [ctx.field_new() for _ in range(4)]
    for w in ws:
        rng.dev_gaussian_vector(ctx, w)
    for i in range(a.nev):
        B0.set_vector(i, ws[i % 4])
    wgt = 1.0 / (1.0 + np.arange(a.nev))
    cf, f = ctx.cfield_new(), ctx.field_new()

    def chain():
        for j in range(a.nev):
            B0.get_vector(j, f)
            ctx.dev_trace_accum(cf, [f], [f], wgt[j])

    gb = (48 * a.nev + 16) * (vol // 2) / 1e9
    for rep in range(2):                                    # both orders: the first arm of a session runs on a cold clock
        for arm in (("kernel", "chain") if rep == 0 else ("chain", "kernel")):
            ms = clock((lambda: B0.block_norm2_accum(0, wgt, cf)) if arm == "kernel" else chain)
            row = dict(what="block_norm2_accum", arm=arm, rep=rep, n=a.nev, ms=stats(ms))
            if arm == "kernel":
                row.update(gbytes=gb, gbytes_per_s=gb / np.median(ms) * 1e3, fraction_of_copy=gb / np.median(ms) * 1e3 / copy)
            out(**row)
    B0.free()
    ctx.cfield_free(cf)
    for w in ws + [f]:
        ctx.field_free(w)

s = q.Staggered(ctx, g, smear=q.HisqCoefs().init())
out(what="links", info=s.links_info())
basis = q.EigBasis(ctx, 2 * a.nev)
t = time.time()
rough = s.eigs(a.nev, nvecs=2 * a.nev, relerr=0.0, abserr=1e-8, max_restarts=6, cheb_degree=0, basis=basis)
ctx.sync()
t_rough = time.time() - t
lo_ = 1.2 * float(rough.evals[-1])
t = time.time()
Bz = s.eigs(a.nev, nvecs=2 * a.nev, relerr=0.0, abserr=1e-8, max_restarts=100, cheb_degree=a.degree, cheb_lo=lo_, cheb_hi=0.0, basis=basis)
ctx.sync()
t_eig = time.time() - t
out(what="eigs", nev=a.nev, nvecs=2 * a.nev, degree=a.degree, cheb_lo=lo_, seconds=t_eig, rough_seconds=t_rough, nconv=Bz.nconv,
    lambda_0=float(Bz.evals[0]), lambda_last=float(Bz.evals[-1]), max_resid=float(Bz.resid.max()))


def var_ratio(plain, lma, nboot=2000):
    """sum over the columns of the sample variances, plain / LMA, with the 16 % .. 84 % interval of a paired bootstrap over the rows"""
    plain, lma = np.atleast_2d(plain.T).T, np.atleast_2d(lma.T).T
    n = plain.shape[0]
    ratio = lambda i: plain[i].var(axis=0, ddof=1).sum() / lma[i].var(axis=0, ddof=1).sum()
    r = np.random.default_rng(1)
    boots = [ratio(r.integers(0, n, n)) for _ in range(nboot)]
    return dict(ratio=float(ratio(np.arange(n))), lo=float(np.percentile(boots, 16)), hi=float(np.percentile(boots, 84)),
                var_plain=float(plain.var(axis=0, ddof=1).sum()), var_lma=float(lma.var(axis=0, ddof=1).sum()))


for mass in (0.1, 0.01 * np.sqrt(2.0)):
    if "C" not in a.skip:
        # the premises of the estimator at this size: both sum rules of L, and m |M^-1 (v_i, 0)|^2 = m/(m^2 + lambda_i) through the
        # SOLVE (the modes are eigenvectors of the operator the solves invert)
        lam = Bz.rayleigh(a.nev)
        w = mass / (mass * mass + lam)
        cf = ctx.cfield_new()
        Bz.lowmode_diag(a.nev, mass, cf)
        L = ctx.cfield_download(cf)[:, 0]
        f, x = ctx.field_new(), ctx.field_new()
        thru = []
        for i in (0, a.nev - 1):
            Bz.get_vector(i, f)
            ctx.dev_solve_batch([x], [f], [mass], 1e-24, 100000)
            thru.append(float(mass * ctx.dev_norm2(x) / w[i] - 1.0))
        rng.dev_gaussian_vector(ctx, f)                     # P is an orthogonal projector: <P phi, Q phi> = 0, Q Q phi = Q phi
        phi = ctx.field_download(f)
        Bz.project_out(a.nev, [f])
        qphi = ctx.field_download(f)
        Bz.project_out(a.nev, [f])
        out(what="premises", mass=mass, sum_w=float(w.sum()), sum_L_even=float(L[:vol // 2].sum()), sum_L_odd=float(L[vol // 2:].sum()),
            lambda_median=float(np.median(lam)), mode_through_the_solve_rel_dev=thru,
            p_dot_q_over_phi2=float(((phi - qphi) * qphi).sum() / (phi ** 2).sum()), p2_over_phi2=float(((phi - qphi) ** 2).sum() / (phi ** 2).sum()),
            second_projection_max_change=float(np.abs(ctx.field_download(f) - qphi).max()))
        for fid in (f, x):
            ctx.field_free(fid)
        ms = clock(lambda: Bz.lowmode_diag(a.nev, mass, cf))
        out(what="lowmode_diag", mass=mass, nev=a.nev, ms=stats(ms))
        ctx.cfield_free(cf)
        ws = [ctx.field_new() for _ in range(4)]
        for fid in ws:
            rng.dev_gaussian_vector(ctx, fid)
        ms = clock(lambda: Bz.project_out(a.nev, ws))
        out(what="project_out", mass=mass, nev=a.nev, n=4, ms=stats(ms))
        for fid in ws:
            ctx.field_free(fid)
    if "D" not in a.skip:
        diffs = []
        for seed in a.seeds:
            rows = {}
            for name, kw in (("plain", {}), ("lma", dict(lma=True))):
                def run(n):
                    r = q.RngField(lat, q.RngMilc6, seed)
                    ctx.sync()
                    t0 = time.perf_counter()
                    _, es, st = q.scalarTrace(s, qlo, r, mass, a.r2req, num_stoch=n, dilute_type="EO", source_type="Z4", improved_trace=True,
                                              out=None, sloppy=a.sloppy, deflate=Bz, nev=a.nev, **kw)
                    ctx.sync()
                    return time.perf_counter() - t0, np.array(es), st
                run(1)                                          # warm-up (work fields, fp32 links)
                wall, es, st = run(a.num_stoch)
                low_s = st.get("lowmode_s", 0.0)
                rows[name] = dict(wall_s=wall, per_source_s=(wall - low_s) / a.num_stoch, lowmode_s=low_s, project_s=st.get("project_s", 0.0),
                                  solve_s=st["solve_s"], contract_s=st["contract_s"], iterations=int(np.sum(st["iterations"])),
                                  pbp_mean=float(es.mean()), pbp_err=float(es.mean(axis=1).std(ddof=1) / np.sqrt(a.num_stoch)))
                rows[name]["est"] = es
                if name == "lma":
                    rows[name]["low_pbp"] = low_pbp = float(st["low_est"].mean())
            ep, el = rows["plain"].pop("est"), rows["lma"].pop("est")
            d = ep.mean(axis=1) - el.mean(axis=1)
            diffs.append(d)
            out(what="scalar_trace_sources", mass=mass, seed=seed, sloppy=a.sloppy, r2req=a.r2req, num_stoch=a.num_stoch, nev=a.nev, rows=rows,
                time_ratio=rows["lma"]["per_source_s"] / rows["plain"]["per_source_s"],
                pbp_plain=[float(v) for v in ep.mean(axis=1)], pbp_lma=[float(v) for v in el.mean(axis=1)],
                paired_difference=dict(mean=float(d.mean()), stderr=float(d.std(ddof=1) / np.sqrt(len(d))), over_low_pbp=[float(v / low_pbp) for v in d]),
                variance_pbp=var_ratio(ep.mean(axis=1), el.mean(axis=1)), variance_est_t=var_ratio(ep, el))
        d = np.concatenate(diffs)
        out(what="paired_difference_all_seeds", mass=mass, sources=len(d), mean=float(d.mean()), stderr=float(d.std(ddof=1) / np.sqrt(len(d))),
            mean_over_low_pbp=float(d.mean() / low_pbp), sigmas=float(d.mean() / (d.std(ddof=1) / np.sqrt(len(d)))))
