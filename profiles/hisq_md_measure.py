#!/usr/bin/env python
"""Timings of the resident HISQ molecular dynamics against the host-pointer path (profiles/hisq_md_32x4.log):

    python profiles/hisq_md_measure.py [-lat 32 32 32 32] [-mass 0.1] [-gsteps 3] [-fsteps 2] [-runs 5]
    python profiles/hisq_md_measure.py -copies DIR      # sums the memory-copy trace a rocprofv3 run of examples/hisqhmc.py left in DIR

1. k_outer13 against the 2n k_outer launches it replaces (n = 1, 4) and k_projtah_kick against k_force_projtah + k_links_axpy:
   device events around the launches (the library's timers "outer" and "projtah_kick"), the two forms alternating in one process
   (option "hisq_md_fused"), on the same fields.
2. One fermion-force update of the momenta (smearRephase, solve, fermionForce, p -= dt f) on each path: host clock around work
   that ends in a device synchronise.
3. A whole trajectory (prepare, evolve, finish) on each path, the paths alternating.
Medians of `runs` warm repetitions with the spread (min .. max); every shape is warmed up by one untimed repetition."""
import argparse
import json
import glob
import importlib.util
import os
import statistics
import sys
import time


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stat(v):
    return "median %.3f  min %.3f  max %.3f  (n = %d)" % (statistics.median(v), min(v), max(v), len(v))


def copies(d):
    """calls and bytes by direction from the memory_copy records of `rocprofv3 --memory-copy-trace --output-format json -d DIR`"""
    tot = {}
    for fn in glob.glob(os.path.join(d, "**", "*results.json"), recursive=True):
        for tool in json.load(open(fn))["rocprofiler-sdk-tool"]:
            names = {}
            for k in tool.get("strings", {}).get("buffer_records", []):
                if "MEMORY_COPY" in str(k.get("kind", "")):
                    names = dict(enumerate(k.get("operations", [])))
            for r in tool.get("buffer_records", {}).get("memory_copy", []):
                c = tot.setdefault(names.get(r.get("operation"), "operation %r" % r.get("operation")), [0, 0])
                c[0] += 1
                c[1] += int(r["bytes"])
    for k, (n, b) in sorted(tot.items()):
        print("copies %-40s %8d calls %16d bytes  (%.1f MB)" % (k, n, b, b / 1e6))
    if not tot:
        print("no memory_copy records under " + d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-lat", type=int, nargs=4, default=[32, 32, 32, 32])
    ap.add_argument("-mass", type=float, default=0.1)
    ap.add_argument("-gsteps", type=int, default=3)
    ap.add_argument("-fsteps", type=int, default=2)
    ap.add_argument("-runs", type=int, default=5)
    ap.add_argument("-copies", default=None)
    ap.add_argument("-skip-trajectory", action="store_true")
    a = ap.parse_args()
    if a.copies:
        return copies(a.copies)
    spec = importlib.util.spec_from_file_location("hisqhmc", os.path.join(ROOT, "examples", "hisqhmc.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    kw = dict(mass=a.mass, gsteps=a.gsteps, fsteps=a.fsteps, warm=0.3)
    res = ex.HisqHMC(a.lat, host=False, **kw)
    print(res.ctx.info())
    print("lattice %r mass %r: %d gauge and %d fermion 2MN steps per trajectory (%d fermion forces, %d gauge forces)" % (
        a.lat, a.mass, a.gsteps, a.fsteps, 2 * a.fsteps, 2 * a.gsteps))
    ctx, md = res.ctx, res.md
    res.prepare()

    # 1. the two kernels against the launches they replace
    vec = [ctx.field_new() for _ in range(4)]
    for i in vec:
        res.prng.dev_gaussian_vector(ctx, i)
    ctx.timers_enable(1)
    for n in (1, 4):
        t = {3: [], 0: []}
        for rep in range(a.runs + 1):
            for fused in (3, 0):
                ctx.set_option("hisq_md_fused", fused)
                ctx.timers_reset()
                md.hisq_fforce(vec[:n], [1.0] * n, 1e-6)
                ctx.sync()
                if rep:
                    t[fused].append((ctx.timer("outer")[1], ctx.timer("projtah_kick")[1], ctx.timer("outer")[0]))
        for fused, name in ((3, "k_outer13"), (0, "%d x k_outer" % (2 * n))):
            print("outer products n = %d  %-14s ms: %s   [%d launches]" % (n, name, stat([v[0] for v in t[fused]]), t[fused][0][2]))
        if n == 1:
            print("TAH + kick         %-28s ms: %s" % ("k_projtah_kick", stat([v[1] for v in t[3]])))
            print("TAH + kick         %-28s ms: %s" % ("k_force_projtah + k_links_axpy", stat([v[1] for v in t[0]])))
    ctx.timers_enable(0)
    ctx.set_option("hisq_md_fused", 3)
    for i in vec:
        ctx.field_free(i)

    # 2. one fermion-force update on each path
    host = ex.HisqHMC(a.lat, host=True, **kw)
    host.prepare()
    h = 0.5 * res.tau / a.fsteps
    t = {"resident": [], "host": []}
    for rep in range(a.runs + 1):
        for name, m in (("resident", res), ("host", host)):
            m.ctx.sync()
            t0 = time.time()
            m.mdv_all([0.0, h])
            m.ctx.sync()
            if rep:
                t[name].append(time.time() - t0)
    for name in t:
        print("fermion-force update (smear, solve, force, kick)  %-8s s: %s" % (name, stat(t[name])))
    print("solver iterations so far: resident %r, host %r" % (res.iters, host.iters))

    # 3. a whole trajectory on each path
    if not a.skip_trajectory:
        t = {"resident": [], "host": []}
        for rep in range(a.runs + 1):
            for name, m in (("resident", res), ("host", host)):
                m.ctx.sync()
                t0 = time.time()
                m.prepare()
                m.evolve()
                acc = m.finish()
                m.ctx.sync()
                if rep:
                    t[name].append(time.time() - t0)
                print("  %-8s trajectory %d: %.3f s  %s dH %r" % (name, rep, time.time() - t0, "ACC" if acc[0] else "REJ", acc[1]))
        for name in t:
            print("trajectory (prepare, evolve, finish)  %-8s s: %s" % (name, stat(t[name])))


if __name__ == "__main__":
    main()
