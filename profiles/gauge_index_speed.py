#!/usr/bin/env python3
"""Kernel times of the bench.py legs that run the gauge, smearing and force kernels (flow_step_32x4, nhyp_smear_force_32x4, and the HISQ
link build's consumer naik_multishift_32x4), a build of the parent commit against this one in one session on one GPU:

    python3 profiles/gauge_index_speed.py PARENT_BUILD/libqexhip.so [OTHER_BUILD/libqexhip.so] > profiles/gauge_index_speed.log

(OTHER_BUILD: what runs as "branch" instead of this tree's library; the parent's own build there makes the run an A/A control of the bound.)

bench.py --gpus 1 --steps 200 --warmup 20 --full --no-cpu --no-48x96 --no-shard-check, four runs in the order parent, branch, parent, branch
(QEXHIP_LIB names the parent's library), each in a fresh process.  Every figure is the legs' own kernel timer (hipEvents around the
launches).  The bound is the parent's own spread: with lo, hi the parent's two figures, a figure of this commit has to lie in
[lo - (hi - lo), hi + (hi - lo)]; the last column says whether it does, and the exit status is 1 if one does not."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIGURES = (
    ("flow_step_32x4", "stage_kernel_us"), ("flow_step_32x4", "kernel_ms", "staple"), ("flow_step_32x4", "kernel_ms", "expupdate"),
    ("flow_step_32x4", "stage_kernel_us_reference_exp_algorithm"), ("flow_step_32x4", "observables_kernel_us", "plaq"),
    ("flow_step_32x4", "observables_kernel_us", "clover_E_Q"),
    ("flow_step_32x4", "observables_kernel_us", "plaq_and_clover_E_Q_one_pass (flow_measure)"),
    ("nhyp_smear_force_32x4", "smear_kernel_ms"), ("nhyp_smear_force_32x4", "force_chain_kernel_ms"),
    ("nhyp_smear_force_32x4", "resident_md", "smear_kernel_ms"), ("nhyp_smear_force_32x4", "resident_md", "force_chain_kernel_ms"),
    ("naik_multishift_32x4", "kernel_us_per_step", "dslash_2_sweeps"),
)


def bench(lib):
    env = dict(os.environ)
    if lib:
        env["QEXHIP_LIB"] = os.path.abspath(lib)
    else:
        env.pop("QEXHIP_LIB", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "200", "--warmup", "20", "--full", "--no-cpu", "--no-48x96",
           "--no-shard-check"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT, env=env, timeout=600)
    if p.returncode:
        sys.exit("bench.py: status %d\n%s" % (p.returncode, p.stderr[-3000:]))
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    out = []
    for path in FIGURES:
        v = res
        for k in path:
            v = v[k]
        out.append(float(v))
    return out, res.get("ms_per_step")


def main(parent_lib, branch_lib=None):
    runs = []
    for tag, lib in (("parent-1", parent_lib), ("branch-1", branch_lib), ("parent-2", parent_lib), ("branch-2", branch_lib)):
        vals, ms = bench(lib)
        runs.append(vals)
        print("%s  done: headline ms_per_step %s" % (tag, ms), file=sys.stderr, flush=True)
    print("%-78s %10s %10s %10s %10s   %s" % ("figure", "parent-1", "parent-2", "branch-1", "branch-2", "branch within parent's range + its spread"))
    bad = 0
    for k, path in enumerate(FIGURES):
        p1, b1, p2, b2 = (r[k] for r in runs)
        lo, hi = min(p1, p2), max(p1, p2)
        lo, hi = lo - (hi - lo), hi + (hi - lo)
        ok = all(lo <= b <= hi for b in (b1, b2))
        bad += not ok
        print("%-78s %10.3f %10.3f %10.3f %10.3f   %s [%.3f, %.3f]" % (" / ".join(path), p1, p2, b1, b2, "yes" if ok else "NO", lo, hi))
    print("figures outside: %d" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
