#!/usr/bin/env python3
"""The table of profiles/batch_lowp_resources.txt: every kernel of the four reduced-precision files at the parent commit against this
one, which moved their host loops (csrc/batch_lowp.h, solver.cpp) and must not have moved any device code.  In qex_amd/ of each
checkout, for f in dslash_f32 dslash_half batch_f32 batch_half:

    hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S -Rpass-analysis=kernel-resource-usage csrc/$f.hip -o DIR/$f.s 2> DIR/$f.rpass

then  python3 profiles/batch_lowp_resources.py PARENT_DIR BRANCH_DIR [FILE ...]  (other files than those four: the table of
profiles/gauge_index_resources.txt names its own).  No GPU is involved.  "identical" is kernels()' of
lowp_refactor_resources.py: the same instruction stream line for line; the kernel-argument segment sizes come from the code objects'
metadata.  A kernel that is missing or differs is named: "reordered" when it has the parent's instructions in another order and
the parent's register, scratch, LDS and occupancy figures.  Exit status 1 if a kernel of the parent is missing or differs, or if one was added."""
import re
import sys

from lowp_refactor_resources import FILES, demangle, kernels


def kernarg_sizes(d, f):
    """demangled name -> .kernarg_segment_size"""
    size, out = None, {}
    for line in open("%s/%s.s" % (d, f)):
        m = re.match(r"\s+\.kernarg_segment_size:\s+(\d+)", line)
        if m:
            size = int(m.group(1))
        m = re.match(r"\s+\.name:\s+(_Z\w+)$", line)
        if m and size is not None:
            out[m.group(1)] = size
            size = None
    dm = demangle(list(out))
    return {re.sub(r"^void |\(.*$", "", dm[k].replace("(anonymous namespace)::", "")): v for k, v in out.items()}


def family(name):
    return re.sub(r"<.*", "", name)


def main(pd, bd, files=FILES):
    bad = 0
    for f in files:
        P, B = kernels(pd, f), kernels(bd, f)
        KP, KB = kernarg_sizes(pd, f), kernarg_sizes(bd, f)
        rows, notes = {}, []
        for name in P:
            same = name in B and P[name][1] == B[name][1] and P[name][0] == B[name][0] and KP[name] == KB.get(name)
            bad += not same
            if name not in B:
                notes.append("missing: " + name)
            elif not same:
                reordered = sorted(P[name][1]) == sorted(B[name][1]) and P[name][0] == B[name][0] and KP[name] == KB.get(name)
                notes.append("%s: %s  %s" % ("reordered" if reordered else "DIFFERENT", name, P[name][0]))
            r = rows.setdefault(family(name), [0, 0, set(), set()])
            r[0] += 1
            r[1] += same
            r[2].add(KP[name])
            r[3].add(P[name][0]["VGPRs"])
        added = sorted(set(B) - set(P))
        bad += len(added)
        for fam, (n, same, ka, vg) in rows.items():
            print("%-16s %-24s %3d kernels, %3d identical   kernarg bytes %-12s VGPRs %d..%d"
                  % (f + ".hip", fam, n, same, "/".join(map(str, sorted(ka))), min(vg), max(vg)))
        for n in notes:
            print("%-16s %s" % (f + ".hip", n))
        print("%-16s added: %s" % (f + ".hip", ", ".join(added) if added else "none"))
    print("kernels missing, different or added: %d" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2], tuple(sys.argv[3:]) or FILES))
