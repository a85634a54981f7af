#!/usr/bin/env python3
"""The bits of everything that addresses the natural-layout gauge field through csrc/gauge_index.h, one sha256 per output array, to
hold a change that moves only addressing against a build of its parent commit (lowp_refactor_bits.py's method and helper):

    [QEXHIP_LIB=PARENT_BUILD/libqexhip.so] python3 profiles/gauge_index_bits.py > OUT

run once per build in the same session; the two outputs must be identical line for line (profiles/gauge_index_bits_parent.txt,
profiles/gauge_index_bits_branch.txt).  Without arguments: 8^4, 6^4 (half-volume no multiple of 64: the ragged last tile and the
padding entries of the visiting order), 4.4.8.8 on one rank with ghost zones (force_halo), and 4.4.8.8 on two t-ranks that share the
device (this script again under torch.distributed.run, with the rank prologue of tests/ranks.py; every rank's slab is hashed).
An entry that refuses a shape prints its error text, which has to agree as well.

  plaq, s4_gauge; gaugeForce for the plaquette, rectangle and adjoint actions; one Wilson-flow step with flowMeasure; Polyakov loops;
  fat7, HISQ and nHYP smearing with their force chains; stout smear, force and inverse; Landau and Coulomb gauge fixing with the
  transform applied; stagDeriv / outer with and without accumulate; qexhip_md_refresh_momenta"""
import os
import sys

import numpy as np

from lowp_refactor_bits import sha

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAT7 = (0.5, 0.1, 0.05, 0.02, 0.03)


def cases(q, ctx, lat, g, chain, x, rng, emit):
    """every entry on the configuration g (chain: a second gauge-shaped field, x: a colour vector), all on ctx"""
    def run(name, fn):
        try:
            emit(name, fn())
        except Exception as e:  # noqa: BLE001 -- a refusal is a result too
            emit(name, "refused: %s" % e)

    def get():
        out = np.zeros_like(g)
        q._lib.check(q.lib().qexhip_gauge_get(ctx._h, out.ctypes.data))
        return out

    run("plaq", lambda: sha(q.plaq(ctx, g)))
    run("s4_gauge", lambda: sha(q.s4_gauge(ctx, g)))
    run("gaugeForce plaq", lambda: sha(q.gaugeForce(ctx, g, 1.0)))
    run("gaugeForce rect", lambda: sha(q.gaugeForce(ctx, g, 1.0, rect=-0.05)))
    run("gaugeForce adj", lambda: sha(q.gaugeForce(ctx, g, 1.0, adjplaq=0.1)))

    def flow():
        q.gaugeSet(ctx, g)
        q.gaugeFlowResident(ctx, 1, 0.01)
        pl, eq = q.flowMeasure(ctx)
        return sha(pl, eq, get())
    run("flow step + flowMeasure", flow)
    run("ploops", lambda: sha(np.array(q.ploops(ctx, g))))

    def fat7():
        fl, ll = np.zeros_like(g), np.zeros_like(g)
        q.makeImpLinks(ctx, fl, g, FAT7, ll, naik=-0.04)
        return sha(fl, ll)
    run("fat7 smear", fat7)
    run("fat7 deriv", lambda: sha(q.fat7lDeriv(ctx, g, chain, FAT7, dll=g, naik=-0.04)))

    def hisq():
        fl, ll, f = np.zeros_like(g), np.zeros_like(g), np.zeros_like(g)
        sf = q.HisqCoefs().init().smearGetForce(ctx, g, fl, ll)
        sf(f, chain, g)
        sf.release()
        return sha(fl, ll, f)
    run("HISQ smear + force", hisq)

    def nhyp():
        fl, f, gf = np.zeros_like(g), np.zeros_like(g), np.zeros_like(g)
        sf = q.HypCoefs().smearGetForce(ctx, g, fl)
        sf(f, chain)
        sf.gforce(gf, 1.0)
        sf.release()
        return sha(fl, f, gf)
    run("nHYP smear + force + gforce", nhyp)

    def stout():
        f1, fl, d, gf = np.zeros_like(g), np.zeros_like(g), np.zeros_like(g), np.zeros_like(g)
        q.stoutSmear(ctx, g, 0.1, f1)
        sf = q.stoutSmearGetForce(ctx, g, fl, (0.1, 0.09, 0.12))
        sf(d, chain)
        sf.gaugeForce(gf, 6.0)
        sf.release()
        return sha(f1, fl, d, gf)
    run("stout smear + force", stout)

    def stout_inverse():
        fi, u = np.zeros_like(g), np.zeros_like(g)
        q.stoutSmear(ctx, g, 0.02, fi)
        its, r2 = q.newStoutSmear(ctx, 0.02).inverse(u, fi)
        return "its=%d rdf2=%r %s" % (its, r2, sha(u))
    run("stout inverse", stout_inverse)

    def gfix(dirs):
        q.gaugeSet(ctx, g)
        t, info = q.getGaugeFixTransform(ctx, dirs, gstop=0.0, orf=1.8, maxits=20)
        q.gaugeTransform(ctx)
        return sha(t, get())
    run("gauge fixing Landau", lambda: gfix([0, 1, 2, 3]))
    run("gauge fixing Coulomb", lambda: gfix([0, 1, 2]))

    def outer():
        s = q.newStag(ctx, g)
        f = np.zeros_like(g)
        out = []
        s.outer(f, x, 0.7, False)
        out.append(f.copy())
        s.outer(f, x, -0.3, True)
        out.append(f.copy())
        s.stagDeriv(f, x)
        return sha(f, *out)
    run("outer, outer accumulate, stagDeriv", outer)

    def momenta():
        md = q.ResidentMD(ctx)
        md.begin(g, None)
        rng.dev_momenta(ctx)
        p = np.zeros_like(g)
        md.end(p=p)
        return sha(p)
    run("md_refresh_momenta", momenta)


def inputs(q, glat):
    r = q.RngField(glat, q.RngMilc6, 987654321)
    g = r.warm(0.3)
    chain = r.randomTAH() + 0.3 * r.random()
    vol = int(np.prod(glat))
    x = np.random.default_rng(100).standard_normal((vol, 3, 2))
    return g, chain, x


def one_rank(lat, halo):
    import qex_amd as q

    tag = ".".join(map(str, lat)) + (" force_halo" if halo else "")
    g, chain, x = inputs(q, lat)
    ctx = q.Context(lat)
    if halo:
        ctx.force_halo(True)
    cases(q, ctx, lat, g, chain, x, q.RngField(lat, q.RngMilc6, 4711), lambda name, v: print("%s: %s: %s" % (tag, name, v), flush=True))
    ctx.close()


def rank(glat):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ranks

    w = ranks.shard(glat)
    import qex_amd as q

    g, chain, x = inputs(q, glat)
    rng = q.RngField(w.loc.lat, q.RngMilc6, 4711, glat=glat, t_offset=w.rank * w.loc.lat[3])
    lines = []
    cases(q, w.ctx, w.loc.lat, w.sl(g), w.sl(chain), w.sl(x), rng, lambda name, v: lines.append("%s: %s" % (name, v)))
    allr = ranks.gather(w, lines)
    if w.rank == 0:
        for k in range(len(lines)):
            for r in range(w.world):
                print("%s %d ranks: rank %d: %s" % (".".join(map(str, glat)), w.world, r, allr[r][k]), flush=True)
    w.dist.barrier()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "rank":
        return rank([int(v) for v in sys.argv[2:6]])
    sys.path.insert(0, ROOT)
    import qex_amd as q

    print("library: %s" % q.LIB_PATH, file=sys.stderr)
    one_rank([8, 8, 8, 8], False)
    one_rank([6, 6, 6, 6], False)
    one_rank([4, 4, 8, 8], True)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ranks

    p = ranks.launch(2, [os.path.abspath(__file__), "rank", 4, 4, 8, 8], 240)
    sys.stdout.write("".join(ln + "\n" for ln in p.stdout.splitlines() if ln.startswith("4.4.8.8 2 ranks: ")))    # (not the rendezvous' chatter)
    if p.returncode:
        sys.stdout.write("4.4.8.8 2 ranks: exit status %d\n%s\n" % (p.returncode, p.stderr[-3000:]))
    return p.returncode


if __name__ == "__main__":
    sys.exit(main())
