#!/usr/bin/env python3
"""The bits of every host loop that csrc/batch_lowp.h and solver.cpp's one single-system loop replaced, one sha256 per case, against a
build of the parent commit (lowp_refactor_bits.py's method and helpers):

    [QEXHIP_LIB=PARENT_BUILD/libqexhip.so] python3 profiles/batch_lowp_bits.py > OUT

run once per build in the same session; the two outputs must be identical line for line (profiles/batch_lowp_bits_parent.txt,
profiles/batch_lowp_bits_branch.txt).  All at 8^4, on g.random (8 links) and on HISQ fat + Naik links (16 links), on both parities:

  single  solveXX in fp32 and in 16-bit storage
  batch   n = 3 (masses 0.1, 0.2, 0.05) in fp32 and in 16-bit storage
  halo    the same batches on the one-rank context with ghost zones (force_halo, option batch_ranks 1)
  stall   option half_stall 0 (the guard trips at the first update), one system at mass 0.05, single and batched: the fp32 finish ran
  probe   dev_op_xx_sloppy_batch and dev_op_xx_half_batch, n = 3"""
import numpy as np

from lowp_refactor_bits import setup, sha

LAT = [8, 8, 8, 8]
MASSES = [0.1, 0.2, 0.05]


def solves(ctx, s, vs, tag):
    fb, fx = ctx.field_new(vs[0]), ctx.field_new()
    for pe in (True, False):
        for name, sl in (("fp32", 1), ("16-bit", 2)):
            its, fin, nup = ctx.dev_solve_xx_sloppy(fx, fb, 0.1, 1e-12, 5000, pe, sl)
            print("single %s %s par_even=%d its=%d updates=%d r2=%r last=%s %s"
                  % (tag, name, pe, its, nup, fin, sorted(ctx.sloppy_last().items()), sha(ctx.field_download(fx))), flush=True)
        batches(ctx, s, vs, tag, pe)
    ctx.field_free(fb)
    ctx.field_free(fx)


def batches(ctx, s, vs, tag, pe):
    xs = [np.zeros_like(v) for v in vs]
    for name, sl in (("fp32", 1), ("16-bit", 2)):
        its, fin, nup = s.solveXX_batch(xs, vs, MASSES, 1e-12, 5000, pe, sloppy=sl)
        print("batch %s n=3 %s par_even=%d its=%s updates=%s r2=%r last=%s %s"
              % (tag, name, pe, list(its), list(nup), list(fin), [sorted(d.items()) for d in ctx.sloppy_last_batch()], sha(*xs)), flush=True)


def stall(ctx, s, vs, tag):
    ctx.set_option("half_stall", 0)
    fb, fx = ctx.field_new(vs[0]), ctx.field_new()
    for pe in (True, False):
        its, fin, nup = ctx.dev_solve_xx_sloppy(fx, fb, 0.05, 1e-12, 5000, pe, 2)
        last = ctx.sloppy_last()
        assert last["fell_back"] == 1 and last["f32_iters"] > 0, last
        print("stall %s single par_even=%d its=%d updates=%d r2=%r last=%s %s"
              % (tag, pe, its, nup, fin, sorted(last.items()), sha(ctx.field_download(fx))), flush=True)
        x = [np.zeros_like(vs[0])]
        its, fin, nup = s.solveXX_batch(x, vs[:1], [0.05], 1e-12, 5000, pe, sloppy=2)
        last = ctx.sloppy_last_batch()
        assert last[0]["fell_back"] == 1 and last[0]["f32_iters"] > 0, last
        print("stall %s batch n=1 par_even=%d its=%s updates=%s r2=%r last=%s %s"
              % (tag, pe, list(its), list(nup), list(fin), [sorted(d.items()) for d in last], sha(*x)), flush=True)
    ctx.field_free(fb)
    ctx.field_free(fx)
    ctx.set_option("half_stall", 2)


def probes(ctx, vs, tag):
    fx, fr = [ctx.field_new(v) for v in vs], [ctx.field_new() for _ in vs]
    for pe in (True, False):
        for name, fn in (("sloppy", ctx.dev_op_xx_sloppy_batch), ("half", ctx.dev_op_xx_half_batch)):
            fn(fr, fx, [0.01, 0.04, 0.25], pe)
            print("probe %s dev_op_xx_%s_batch n=3 par_even=%d %s" % (tag, name, pe, sha(*[ctx.field_download(f) for f in fr])), flush=True)
    for f in fx + fr:
        ctx.field_free(f)


def main():
    import qex_amd as q

    for kind in ("random", "hisq"):
        ctx, s, vs = setup(q, LAT, kind)
        tag = "%s f32fmt=%d halffmt=%d" % (kind, ctx.links_info_f32()[0], ctx.links_info_half()[0])
        probes(ctx, vs, tag)
        solves(ctx, s, vs, tag)
        stall(ctx, s, vs, tag)
        ctx.close()
        ctx, s, vs = setup(q, LAT, kind, halo=True)
        ctx.set_option("batch_ranks", 1)
        for pe in (True, False):
            batches(ctx, s, vs, "%s halo batch_ranks=1" % kind, pe)
        probes(ctx, vs, "%s halo batch_ranks=1" % kind)
        ctx.close()


if __name__ == "__main__":
    main()
