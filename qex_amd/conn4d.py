"""Connected part of the flavour-singlet scalar correlator from point sources: the host mirror of

    randomPoint, getPoint                src/observables/conn4d.nim:127-171
    the source loop and the correlator   src/observables/conn4d.nim:197-248
    sq_min_distance's default            src/observables/conn4d.nim:34-35

Everything between the coordinates and the per-timeslice table stays on the device: for every group of up to `batch` (<= 4) of the
3 * len(pts) systems (point, colour) one qexhip_dev_point_source, one lock-step batched solve (qexhip_dev_solve_batch or its
mixed-precision variant) and one qexhip_dev_conn_accum into a resident complex site field; then qexhip_cfield_stag_sign, the slice
sums of qexhip_dev_cfield_slices and one download.  The accumulation adds system after system in the reference's order (point
outer, colour inner) whatever the grouping, so the result does not depend on `batch`.
"""
import math
import time


def defaultSqMinDistance(glat, num_source):
    """conn4d.nim:34-35: floor(0.25 * sqrt(volume / num_source))"""
    vol = 1
    for v in glat:
        vol *= int(v)
    return int(math.floor(0.25 * math.sqrt(float(vol) / float(num_source))))


def randomPoint(R, glat, pts, sq_min_distance, maxiter=1_000_000_000):
    """conn4d.nim:128-158.  R: the global generator (GlobalRng); glat: the GLOBAL lattice; pts: the points so far, a list the new
    point is appended to (and returned).  A draw floor(L_i * R.uniform()) per coordinate is accepted when its periodic squared
    distance to every earlier point, measured BEFORE the coordinates are rounded down to even, is not below sq_min_distance."""
    nd = len(glat)
    for _ in range(int(maxiter)):
        pt = []
        for i in range(nd):
            li = int(glat[i])
            v = int(math.floor(li * R.uniform()))
            assert 0 <= v < li
            pt.append(v)
        far = True
        for prev in pts:
            d = 0
            for i in range(nd):
                dx1 = abs(prev[i] - pt[i])
                dx = min(dx1, int(glat[i]) - dx1)
                d += dx * dx
            if d < sq_min_distance:
                far = False
                break
        pt = [v - v % 2 for v in pt]          # "Force the point to lay on a unit corner."
        if far:
            pts.append(pt)
            return pt
    raise RuntimeError("max iteration reached without finding a random point.\n"
                       "Perhaps sq_min_distance=%s is too large." % (sq_min_distance,))


def connMeson(stag, lo, pts, mass, r2req, maxits=100000, t_offset=0, sloppy=0, batch=4, deflate=None, nev=None, out=print):
    """conn4d.nim:197-248 on resident fields.  stag: the operator (its context holds the links); lo: the rank-local Layout and
    t_offset its first global t; pts: the source points, GLOBAL (x, y, z, t) each.  For every point and colour a point source is
    solved to r2req and
        locmes(x) += |phi(x (+) pt)|^2 / len(pts),
    then locmes(x) *= (-1)^(x0+x1+x2).  Returns (locmes, est, stats): locmes the (vol,) field of the local lattice in host site
    order, est[t] = sum_{x in slice t} locmes over the GLOBAL t, stats = {"solve_s", "contract_s", "iterations", "updates"}
    (seconds in the batched solves; in sources, accumulation, sign and slice sums; iterations and reliable updates per system in
    (point, colour) order).  sloppy = 1 (or 2) solves in mixed precision (one rank; t-sharded with the context option
    "batch_ranks" = 1 on every rank).  deflate = an EigBasis of the operator's
    even sites, used with its leading nev vectors (None: deflate.nconv).  out receives the reference's log lines (None: none, and
    the norms they print are not computed)."""
    ctx = stag.ctx
    if list(lo.lat) != list(ctx.lat):
        raise ValueError("lo is not the layout of the context's local lattice")
    if int(t_offset) != ctx.lat[3] * ctx.rank_coord[3]:
        raise ValueError("t_offset = %d is not the first global t of the context's slab" % t_offset)
    batch = int(batch)
    if not 1 <= batch <= 4:
        raise ValueError("batch = %d, must be 1..4" % batch)
    pts = [[int(v) for v in p] for p in pts]
    if not pts or any(len(p) != 4 for p in pts):
        raise ValueError("pts must be a non-empty list of points with four coordinates each")
    defl = {} if deflate is None and nev is None else {"deflate": deflate, "nev": nev}
    nc = 3
    scal = 1.0 / float(len(pts))
    say = out if out is not None else (lambda s: None)
    systems = [(p, c) for p in pts for c in range(nc)]
    fields, locmes = [], None
    stats = {"solve_s": 0.0, "contract_s": 0.0, "iterations": [], "updates": []}
    try:
        eta = [ctx.field_new() for _ in range(batch)]
        phi = [ctx.field_new() for _ in range(batch)]
        fields += eta + phi
        locmes = ctx.cfield_new()
        for k0 in range(0, len(systems), batch):
            grp = systems[k0:k0 + batch]
            n = len(grp)
            gp, gc = [p for p, _ in grp], [c for _, c in grp]
            t0 = time.perf_counter()
            ctx.dev_point_source(eta[:n], gp, gc)
            ctx.sync()
            t1 = time.perf_counter()
            if sloppy:
                its, _, nup = ctx.dev_solve_batch(phi[:n], eta[:n], [mass] * n, r2req, maxits, sloppy=sloppy, **defl)
            else:
                its, _ = ctx.dev_solve_batch(phi[:n], eta[:n], [mass] * n, r2req, maxits, **defl)
                nup = [0] * n
            t2 = time.perf_counter()
            ctx.dev_conn_accum(locmes, phi[:n], gp, scal)
            ctx.sync()
            t3 = time.perf_counter()
            stats["solve_s"] += t2 - t1
            stats["contract_s"] += (t1 - t0) + (t3 - t2)
            stats["iterations"] += list(its)
            stats["updates"] += list(nup)
            if out is not None:
                for j in range(n):
                    say("Color %d" % gc[j])
                    say("norm2: %r" % (ctx.dev_norm2(phi[j]),))
        t0 = time.perf_counter()
        ctx.cfield_stag_sign(locmes)
        est = ctx.dev_cfield_slices(locmes)[:, 0].copy()
        stats["contract_s"] += time.perf_counter() - t0
        return ctx.cfield_download(locmes)[:, 0].copy(), est, stats
    finally:
        for fid in fields:
            ctx.field_free(fid)
        if locmes is not None:
            ctx.cfield_free(locmes)
