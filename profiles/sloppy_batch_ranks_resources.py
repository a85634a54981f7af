#!/usr/bin/env python3
"""The table of profiles/sloppy_batch_ranks_resources.txt: the lock-step reduced-precision sweep kernels' generated gfx950 code at the
parent commit (k_dslash_mrhs_lowp<St, NDIR, RECON, SECOND>) against this one (.., SECOND, HALO>).  In qex_amd/ of each checkout, for f
in batch_f32 batch_half:

    hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S -Rpass-analysis=kernel-resource-usage csrc/$f.hip -o DIR/$f.s 2> DIR/$f.rpass

then  python3 profiles/sloppy_batch_ranks_resources.py PARENT_DIR BRANCH_DIR.  No GPU is involved.

Part 1: every HALO = false instantiation against the parent's kernel of the same <St, NDIR, RECON, SECOND>: kernel arguments (bytes of
the kernarg segment), resources and instruction stream; "identical" as profiles/lowp_refactor_resources.py defines it (line for line once
comments, local label numbers and kernel names are taken out).
Part 2: the new HALO = true instantiations' VGPRs, scratch bytes per lane and waves/SIMD beside their HALO = false twins."""
import re
import subprocess
import sys

from lowp_refactor_resources import kernels

FILES = ("batch_f32", "batch_half")
NAME = re.compile(r"k_dslash_mrhs_lowp<(\w+), (\d+), (\d+), (true|false)(?:, (true|false))?>")


def kernarg(d, f):
    """<St, NDIR, RECON, SECOND[, HALO]> -> bytes of the kernel's kernarg segment (the metadata lists the size ahead of the name)"""
    sizes, size = {}, None
    for line in open("%s/%s.s" % (d, f)):
        m = re.match(r"\s+\.kernarg_segment_size:\s+(\d+)", line)
        if m:
            size = int(m.group(1))
        m = re.match(r"\s+\.name:\s+(_Z\w+)$", line)
        if m and size is not None:
            sizes[m.group(1)], size = size, None
    names = list(sizes)
    dm = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return {NAME.search(t).groups(): sizes[n] for n, t in zip(names, dm) if NAME.search(t)}


def main(pd, bd):
    nsame = ntotal = 0
    halo_rows = []
    for f in FILES:
        P, B = kernels(pd, f), kernels(bd, f)
        kp, kb = kernarg(pd, f), kernarg(bd, f)
        pk = {NAME.search(k).groups(): v for k, v in P.items() if NAME.search(k)}
        bk = {NAME.search(k).groups(): v for k, v in B.items() if NAME.search(k)}
        for key in sorted(pk):
            st, nd, rc, sec, _ = key
            new = (st, nd, rc, sec, "false")
            (rp, ip), (rb, ib) = pk[key], bk[new]
            ntotal += 1
            same = ip == ib
            nsame += same
            print("k_dslash_mrhs_lowp<%s, %2s, %s, %-5s, false>  kernarg %3s/%-3s B  VGPR %3d/%-3d SGPR %3d/%-3d scratch %d/%d occ %d/%d  insts %4d/%-4d  %s"
                  % (st, nd, rc, sec, kp.get(key, "?"), kb.get(new, "?"), rp["VGPRs"], rb["VGPRs"], rp["TotalSGPRs"], rb["TotalSGPRs"],
                     rp["ScratchSize"], rb["ScratchSize"], rp["Occupancy"], rb["Occupancy"], len(ip), len(ib),
                     "identical" if same else "DIFFERENT"))
            h = (st, nd, rc, sec, "true")
            rh, ih = bk[h]
            halo_rows.append("k_dslash_mrhs_lowp<%s, %2s, %s, %-5s, true >  kernarg %3s B  VGPR %3d (HALO = false: %3d)  scratch %d B/lane  %d waves/SIMD  insts %4d"
                             % (st, nd, rc, sec, kb.get(h, "?"), rh["VGPRs"], rb["VGPRs"], rh["ScratchSize"], rh["Occupancy"], len(ih)))
    print("HALO = false identical to the parent (parent/branch columns): %d of %d kernels" % (nsame, ntotal))
    print()
    print("the new HALO = true instantiations:")
    for r in halo_rows:
        print(r)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
