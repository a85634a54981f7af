#!/usr/bin/env python3
"""The table of profiles/lowp_refactor_resources.txt: the reduced-precision sweep kernels' generated gfx950 code at the parent commit
against this one.  In qex_amd/ of each checkout, for f in dslash_f32 dslash_half batch_f32 batch_half:

    hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S -Rpass-analysis=kernel-resource-usage csrc/$f.hip -o DIR/$f.s 2> DIR/$f.rpass

then  python3 profiles/lowp_refactor_resources.py PARENT_DIR BRANCH_DIR.  No GPU is involved.

A kernel is "identical" when its instruction stream is the parent's line for line once comments, local label numbers and kernel
names are taken out; otherwise the opcodes whose counts differ are listed (fp / conversion / memory opcodes marked with !)."""
import collections
import re
import subprocess
import sys

FILES = ("dslash_f32", "dslash_half", "batch_f32", "batch_half")
OLD = re.compile(r"k_dslash_(mrhs_)?(f32|half)<")
STORE = {"f32": "StoreF32", "half": "StoreHalf"}


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.splitlines()))


def kernels(d, f):
    """demangled name -> (resources, [normalised instruction lines])"""
    res, cur = {}, None
    for line in open("%s/%s.rpass" % (d, f)):
        m = re.search(r"remark:\s+(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if m and m.group(1) == "Function Name":
            cur = res.setdefault(m.group(2), {})
        elif m:
            cur[m.group(1).split()[0]] = int(m.group(2))
    body, name = {}, None
    for line in open("%s/%s.s" % (d, f)):
        m = re.match(r"(_Z\w+):", line)
        if m and m.group(1) in res:
            name = m.group(1)
            body[name] = []
        elif line.startswith(".Lfunc_end"):
            name = None
        elif name and line.startswith("\t") and not line.startswith("\t."):
            t = re.sub(r"\s*;.*", "", line.strip())
            t = re.sub(r"_Z\w+", "K", re.sub(r"\.LBB\d+_", ".LBB_", t))
            if t:
                body[name].append(t)
    dm = demangle(list(res))
    return {re.sub(r"^void |\(.*$", "", dm[k].replace("(anonymous namespace)::", "")): (res[k], body[k]) for k in res}


def new_name(old):
    m = OLD.search(old)
    return old[:m.start()] + "k_dslash_%slowp<%s, " % (m.group(1) or "", STORE[m.group(2)]) + old[m.end():]


def main(pd, bd):
    important = re.compile(r"^(v_(pk_)?(fma|mul_f|mul_legacy|add_f|sub_f|subrev_f|mac_f|mad_f|max_f|min_f|med3_f|rcp|rsq|sqrt|rndne|cvt|ldexp|dot)"
                           r"|global_|buffer_|flat_|s_load|s_buffer_load|ds_|scratch_)")
    nsame = 0
    for f in FILES:
        P, B = kernels(pd, f), kernels(bd, f)
        for old in P:
            if not OLD.search(old):
                continue
            (rp, ip), (rb, ib) = P[old], B[new_name(old)]
            cols = " ".join("%s %3d/%-3d" % (n, rp[k], rb[k]) for n, k in (("VGPR", "VGPRs"), ("SGPR", "TotalSGPRs"), ("scratch", "ScratchSize"),
                                                                           ("occ", "Occupancy")))
            note = "identical"
            if ip != ib:
                cp, cb = collections.Counter(x.split()[0] for x in ip), collections.Counter(x.split()[0] for x in ib)
                diff = ["%s%s %+d" % ("!" if important.match(o) else "", o, cb[o] - cp[o]) for o in sorted(set(cp) | set(cb)) if cp[o] != cb[o]]
                note = ", ".join(diff) if diff else "same opcode counts, other order or registers"
            else:
                nsame += 1
            print("%-52s %s  insts %4d/%-4d  %s" % (new_name(old), cols, len(ip), len(ib), note))
    print("identical to the parent: %d kernels" % nsame)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
