"""Local staggered meson correlators: the host mirror of

    stagLocalMesons, sft, printLocalMesons, pointSource   src/observables/fpvaMeas.nim:6-78
    stagMesons                                           src/physics/stagMesonLocal.nim:14-51
    wallSource, norm2slice                               src/observables/sources.nim:4-18

The sums over sites run in libqexhip.so (qexhip_dev_meson_corners / qexhip_dev_norm2slice) on resident fields; host arrays are
uploaded first.  sft / printLocalMesons work on the small (nt, 8) tables and pointSource / wallSource build host fields: pure numpy.
"""
import numpy as np


def _ids(ctx, v):
    """field id(s) or host array(s) -> (list of ids, list of ids to free afterwards)"""
    vs = list(v) if isinstance(v, (list, tuple)) else [v]
    ids, tmp = [], []
    for f in vs:
        if isinstance(f, np.ndarray):
            fid = ctx.field_new(np.ascontiguousarray(f, dtype=np.float64))
            ids.append(fid)
            tmp.append(fid)
        else:
            ids.append(int(f))
    return ids, tmp


def stagLocalMesons(ctx, v1, v2, t0=0):
    """c[(t - t0) mod nt][corner] += Re<v1(x), v2(x)> (fpvaMeas.nim:33-61), rank-global (nt, 8) array.  v1, v2: a field (id or host
    array) or equal-length lists of fields, summed pair by pair -- up to four pairs go in one launch (three colours at once)."""
    x, tx = _ids(ctx, v1)
    y, ty = _ids(ctx, v2)
    try:
        if len(x) != len(y):
            raise ValueError("v1 and v2 hold different numbers of fields")
        nt = ctx.lat[3] * ctx.rank_geom[3]
        c = np.zeros((nt, 8))
        for k in range(0, len(x), 4):
            c += ctx.dev_meson_corners(x[k:k + 4], y[k:k + 4], t0)
        return c
    finally:
        for fid in tx + ty:
            ctx.field_free(fid)


def stagMesons(ctx, v, out=print):
    """stagMesons (stagMesonLocal.nim:14-51): |v|^2 per (t, corner), printed as `corner: s` blocks and the `sum:` over corners"""
    c = stagLocalMesons(ctx, v, v, 0)
    for s in range(8):
        out("corner: %d" % s)
        for t in range(c.shape[0]):
            out("%d %r" % (t, float(c[t, s])))
    out("sum:")
    for t in range(c.shape[0]):
        r = c[t, 0]
        for s in range(1, 8):
            r += c[t, s]
        out("%d %r" % (t, float(r)))
    return c


def norm2slice(ctx, f, s):
    """norm2slice (sources.nim:10-18): |f|^2 summed over the slices x_s = const, rank-global; f a field id or host array"""
    ids, tmp = _ids(ctx, f)
    try:
        return ctx.dev_norm2slice(ids[0], s)
    finally:
        for fid in tmp:
            ctx.field_free(fid)


def sft(c, b):
    """sft (fpvaMeas.nim:63-70): one butterfly of the Walsh-Hadamard transform over corner bit b, in place"""
    for s in range(8):
        if s & b == 0:
            c0, c1 = c[:, s].copy(), c[:, s + b].copy()
            c[:, s] = c0 + c1
            c[:, s + b] = c0 - c1
    return c


def printLocalMesons(c, f=1.0, out=print):
    """printLocalMesons (fpvaMeas.nim:72-78): Walsh-Hadamard transform over the three corner bits (in place), then every corner's
    correlator scaled by f"""
    sft(c, 1)
    sft(c, 2)
    sft(c, 4)
    for s in range(8):
        out("corner: %d" % s)
        for t in range(c.shape[0]):
            out("%d %r" % (t, float(f * c[t, s])))
    return c


def _owned(lo, t, t_offset):
    return t_offset <= t < t_offset + lo.lat[3]


def pointSource(lo, coord, ic, t_offset=0):
    """pointSource (fpvaMeas.nim:6-14): unit vector in colour ic at the GLOBAL coordinate `coord`, zero elsewhere.  lo is the
    rank-local Layout and t_offset its first global t; on a t-sharded lattice only the rank that owns the point sets it."""
    r = lo.ColorVector()
    if _owned(lo, int(coord[3]), t_offset):
        r[lo.index([coord[0], coord[1], coord[2], int(coord[3]) - t_offset]), int(ic), 0] = 1.0
    return r


def wallSource(lo, t0, v, t_offset=0):
    """wallSource (sources.nim:4-8): v (three complex numbers, or a (3, 2) array of re, im) on every site of the global slice t0"""
    r = lo.ColorVector()
    v = np.asarray(v)
    if np.iscomplexobj(v) or v.shape == (3,):
        v = np.stack([np.real(v), np.imag(v)], axis=-1).astype(np.float64)
    if _owned(lo, int(t0), t_offset):
        r[lo.coords[:, 3] == int(t0) - t_offset] = v
    return r


def localMesonTables(stag, lo, mass, t0, r2req, maxits=100000, t_offset=0, sloppy=0, deflate=None, nev=None):
    """The measurement of fpvaMeas.nim's main block (:80-138) on resident fields: for each colour ic, the point source src at
    (0,0,0,t0) and its three symmetric shifts are solved in ONE lock-step batch of four, the shifted propagators are shifted back at
    the sink, and the contractions of all three colours run on the device in one launch per table:
        cl     = stagLocalMesons(dest, dest, t0)
        cs[mu] = stagLocalMesons(dest, symShift(solve(symShift(src, mu)), mu), t0)        mu = 0, 1, 2
    lo is the rank-local Layout, t_offset its first global t.  Returns (cl, [cx, cy, cz], stats) with the raw (nt, 8) tables
    (printLocalMesons transforms and scales them) and stats = {"solve_s", "contract_s", "iterations", "updates"}.
    sloppy = 1 (or 2) runs the batches in mixed precision (Context.dev_solve_batch(..., sloppy=...): one rank, or t-sharded with
    the context option "batch_ranks" = 1 on every rank); "updates" then
    holds the reliable updates per colour and system, and zeros for the fp64 batch.  deflate = an EigBasis of the operator's even
    sites: every batch is deflated from it with its leading nev vectors (None: deflate.nconv)."""
    import time

    defl = {} if deflate is None and nev is None else {"deflate": deflate, "nev": nev}

    ctx = stag.ctx
    keep = []

    def new():
        fid = ctx.field_new()
        keep.append(fid)
        return fid

    try:
        dest = [new() for _ in range(3)]
        rs = [[new() for _ in range(3)] for _ in range(3)]      # rs[mu][ic]
        src, srcs, dests = new(), [new() for _ in range(3)], [new() for _ in range(3)]
        stats = {"solve_s": 0.0, "contract_s": 0.0, "iterations": [], "updates": []}
        for ic in range(3):
            ctx.field_upload(src, pointSource(lo, [0, 0, 0, t0], ic, t_offset))
            for mu in range(3):
                ctx.dev_sym_shift(srcs[mu], src, mu)
            ctx.sync()
            t = time.perf_counter()
            if sloppy:
                its, _, nup = ctx.dev_solve_batch([dest[ic]] + dests, [src] + srcs, [mass] * 4, r2req, maxits, sloppy=sloppy, **defl)
            else:
                its, _ = ctx.dev_solve_batch([dest[ic]] + dests, [src] + srcs, [mass] * 4, r2req, maxits, **defl)
                nup = [0] * 4
            stats["solve_s"] += time.perf_counter() - t
            stats["iterations"].append(its)
            stats["updates"].append(nup)
            for mu in range(3):
                ctx.dev_sym_shift(rs[mu][ic], dests[mu], mu)
        ctx.sync()
        t = time.perf_counter()
        cl = ctx.dev_meson_corners(dest, dest, t0)
        cs = [ctx.dev_meson_corners(dest, rs[mu], t0) for mu in range(3)]
        stats["contract_s"] = time.perf_counter() - t
        return cl, cs, stats
    finally:
        for fid in keep:
            ctx.field_free(fid)
