#!/usr/bin/env python3
"""The bits of the reduced-precision operators and solves, one sha256 per case, to hold a change that claims to change nothing (the
fp32 and 16-bit sweeps behind one body, csrc/dslash_lowp.h) against a build of its parent commit:

    [QEXHIP_LIB=PARENT_BUILD/libqexhip.so] python3 profiles/lowp_refactor_bits.py > OUT

run once per build (qex_amd/_lib.py: QEXHIP_LIB names another build of the library) in the same session; the two outputs must be
identical line for line (profiles/lowp_refactor_bits_parent.txt, profiles/lowp_refactor_bits_branch.txt).  Links and vectors come from
the library's own generators.

  op      dev_op_xx_sloppy, dev_op_xx_half and dev_op_xx_half_batch (n = 3) at 8^4 and 4x6x10x6 on g.random (8 links, format 1) and on
          HISQ-like fat + Naik links (16 links, format 0), both parities
  solve   one solveXX per path at 8^4 on both link sets: fp32 single, 16-bit single, fp32 batch and 16-bit batch (n = 3), with
          iterations, reliable updates and the solutions' hash
  halo    the one-rank context with ghost zones (force_halo): the fp32 and the 16-bit operator exchange-first and split by sites"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def setup(q, lat, kind, halo=False):
    ctx = q.Context(lat)
    if halo:
        ctx.force_halo(True)
    g = q.RngField(lat, q.RngMilc6, 987654321)
    u = g.random() if kind == "random" else g.warm(0.3)
    q.rephase(q.Layout(lat), u)
    s = q.newStag(ctx, u) if kind == "random" else q.Staggered(ctx, u, smear=q.HisqCoefs().init())
    ctx.set_option("half", 1)
    ctx.set_option("half_batch", 1)
    vol = int(np.prod(lat))
    vs = [np.random.default_rng(100 + j).standard_normal((vol, 3, 2)) for j in range(3)]
    return ctx, s, vs


def ops(ctx, vs, tag):
    fx, fr = [ctx.field_new(v) for v in vs], [ctx.field_new() for _ in vs]
    m2s = [0.01, 0.04, 0.25]
    for pe in (True, False):
        for name, fn in (("sloppy", ctx.dev_op_xx_sloppy), ("half", ctx.dev_op_xx_half)):
            fn(fr[0], fx[0], m2s[0], pe)
            print("op %s dev_op_xx_%s par_even=%d %s" % (tag, name, pe, sha(ctx.field_download(fr[0]))), flush=True)
        if not ctx.sweep_info()["halo"]:
            ctx.dev_op_xx_half_batch(fr, fx, m2s, pe)
            print("op %s dev_op_xx_half_batch n=3 par_even=%d %s" % (tag, pe, sha(*[ctx.field_download(f) for f in fr])), flush=True)
    for f in fx + fr:
        ctx.field_free(f)


def main():
    import qex_amd as q

    for lat in ([8, 8, 8, 8], [4, 6, 10, 6]):
        for kind in ("random", "hisq"):
            ctx, s, vs = setup(q, lat, kind)
            tag = "%s %s f32fmt=%d halffmt=%d" % ("x".join(map(str, lat)), kind, ctx.links_info_f32()[0], ctx.links_info_half()[0])
            ops(ctx, vs, tag)
            if lat == [8, 8, 8, 8]:
                fb, fx = ctx.field_new(vs[0]), ctx.field_new()
                for name, sl in (("fp32", 1), ("16-bit", 2)):
                    its, fin, nup = ctx.dev_solve_xx_sloppy(fx, fb, 0.1, 1e-12, 5000, True, sl)
                    print("solve %s single %s its=%d updates=%d r2=%r last=%s %s"
                          % (tag, name, its, nup, fin, sorted(ctx.sloppy_last().items()), sha(ctx.field_download(fx))), flush=True)
                xs = [np.zeros_like(v) for v in vs]
                for name, sl in (("fp32", 1), ("16-bit", 2)):
                    its, fin, nup = s.solveXX_batch(xs, vs, [0.1, 0.2, 0.05], 1e-12, 5000, True, sloppy=sl)
                    print("solve %s batch n=3 %s its=%s updates=%s r2=%r %s" % (tag, name, list(its), list(nup), list(fin), sha(*xs)), flush=True)
            ctx.close()
    for kind in ("random", "hisq"):
        ctx, s, vs = setup(q, [8, 8, 8, 8], kind, halo=True)
        for overlap in (0, 1):
            ctx.set_option("overlap", overlap)
            ctx.timers_enable(3)
            ctx.timers_reset()
            ops(ctx, vs, "8x8x8x8 %s halo overlap=%d" % (kind, overlap))
            print("halo %s overlap=%d launches: exchange %d, dslash_f32 %d + bnd %d, dslash_half %d + bnd %d"
                  % ((kind, overlap) + tuple(ctx.timer(t)[0] for t in ("exchange", "dslash_f32", "dslash_f32_bnd", "dslash_half", "dslash_half_bnd"))),
                  flush=True)
            ctx.timers_enable(0)
        ctx.close()


if __name__ == "__main__":
    main()
