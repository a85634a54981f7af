#!/usr/bin/env python3
"""The numbers of DESIGN.md section 4 "16-bit storage" (SloppyHalf with option "half" = 1), measured in one session on the MI355X
(32^4 unless -lat is given) that also re-times the fp32 kernels:

  solves   solveEE on resident fields, wall time, r2req = 1e-14, at m = 0.1 and m = 0.01 sqrt(2), on g.random (8 links, sign
           format) and on HISQ fat + Naik links (16 links, 18 reals): iterations, reliable updates and milliseconds (second call)
           of the fp64 CG, SloppySingle and SloppyHalf, and whether the 16-bit solve's stall guard fired; first the box's copy
           bandwidth (k_copy16 of libqexhip_tune, 1 GiB)
  kernels  the same solves at m = 0.1 only, once each, as the workload of a kernel trace
               rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 profiles/half_measure.py kernels
  stats    python3 profiles/half_measure.py stats DIR/**/kernel_stats.csv COPY_GBS: the 16-bit and fp32 kernels of that trace
           with calls, mean us, bytes per site and TB/s against the copy bandwidth.  Bytes per site of a sweep: the links of
           the site, its sign masks, one read and one write of a vector element (a neighbour is read from HBM once), and
           the b-term source of the second sweep

one JSON line per measurement on stdout"""
import csv
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def out(**kw):
    print(json.dumps(kw), flush=True)


def sweep_bytes(kind, ndir, init_or_dot, recon):
    """bytes per site of one sweep: kind 'half' or 'f32'"""
    npair = ndir // 2
    if kind == "half":
        link, vec = (48 if recon else 72) * npair, 16
    else:
        link, vec = (96 if recon else 144) * npair, 24
    return link + (ndir * 8 / 64.0 if recon else 0.0) + vec * (3 if init_or_dot else 2)


def stats(path, copy_gbs, vh):
    rows = []
    for r in csv.DictReader(open(path)):
        name = r["Name"]
        m = re.match(r".*k_dslash_(half|f32)<(\d+), (?:(?:true|false), )?(true|false), (true|false), (\d)>", name)
        us = float(r["AverageNs"]) / 1e3
        if m and (m.group(1) == "half" or "false, " in name):
            kind, ndir, init, dot, recon = m.group(1), int(m.group(2)), m.group(3) == "true", m.group(4) == "true", int(m.group(5))
            b = sweep_bytes(kind, ndir, init or dot, recon)
            tbs = b * vh / us / 1e6
            rows.append(dict(kernel=name[:70], calls=int(r["Calls"]), us=round(us, 2), bytes_per_site=round(b, 1), tbytes_per_s=round(tbs, 3),
                             of_copy=round(tbs * 1e3 / copy_gbs, 3)))
        elif re.search(r"k_slph_|k_slp_xpay|k_slp_update|k_links_half|k_links_f32|k_links_absmax", name):
            # BLAS bytes per site: xpay reads r_s, p_s and writes p_s; update reads p_s, Ap_s, r_s, x_s and writes r_s, x_s
            per = {"k_slph_xpay": 48, "k_slph_update": 16 * 4 + 24 * 2, "k_slp_xpay": 72, "k_slp_update": 24 * 6}
            key = next((k for k in per if k + "(" in name or name.startswith(k)), None)
            row = dict(kernel=name[:70], calls=int(r["Calls"]), us=round(us, 2))
            if key:
                tbs = per[key] * vh / us / 1e6
                row.update(bytes_per_site=per[key], tbytes_per_s=round(tbs, 3), of_copy=round(tbs * 1e3 / copy_gbs, 3))
            rows.append(row)
    for row in sorted(rows, key=lambda d: d["kernel"]):
        out(what="kernel", **row)


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "solves"
    lat = [32, 32, 32, 32]
    if mode == "stats":
        return stats(sys.argv[2], float(sys.argv[3]), int(np.prod(lat)) // 2)
    import qex_amd as q
    from qex_amd import _lib

    ctx = q.Context(lat)
    out(what="device", info=ctx.info())
    if mode == "solves":
        gbs = C.c_double(0)
        _lib.tune_lib().qexhip_tune_stream(ctx._h, 1, 1024, 2048, 5, C.byref(gbs))
        out(what="copy_bandwidth", kernel="k_copy16 1 GiB", gbytes_per_s=gbs.value)
    rng = q.RngField(lat, q.RngMilc6, 987654321)
    fb, fx = ctx.field_new(), ctx.field_new()
    rng.dev_gaussian_vector(ctx, fb)
    masses = [0.1, 0.01 * np.sqrt(2.0)] if mode == "solves" else [0.1]
    for links in ("random", "hisq"):
        if links == "random":
            g = rng.random()
            q.rephase(q.Layout(lat), g)
            s = q.newStag(ctx, g)
        else:
            g = rng.warm(0.3)
            q.rephase(q.Layout(lat), g)
            s = q.Staggered(ctx, g, smear=q.HisqCoefs().init())
        ctx.set_option("half", 1)
        out(what="links", links=links, info=s.links_info(), f32=ctx.links_info_f32(), half=ctx.links_info_half())
        for mass in masses:
            for name, sl in (("fp64", 0), ("single", 1), ("half", 2)):
                for rep in range(2 if mode == "solves" else 1):
                    ctx.sync()
                    t0 = time.perf_counter()
                    its, fin, nup = ctx.dev_solve_xx_sloppy(fx, fb, mass, 1e-14, 20000, True, sl)
                    ms = (time.perf_counter() - t0) * 1e3
                last = ctx.sloppy_last() if sl else {}
                out(what="solveEE", links=links, mass=mass, solver=name, iterations=its, updates=nup, r2_over_b2=fin, ms=round(ms, 2),
                    us_per_iteration=round(ms * 1e3 / max(its, 1), 1), **last)
    ctx.close()


if __name__ == "__main__":
    main()
