"""What tests/test_gpu_lossless.py, test_gpu_link_packed.py and test_gpu_link_ortho.py share: QEX g.random links and a source, one
Context per lattice, everything the sweeps compute on a set of links under a given option lossless, the 18-real reference
(computed once per lattice and seed, never changed) and the two-rank launch of tests/lossless_rank_worker.py."""
import json
import os

import numpy as np

from oracle import oracle as o
from ranks import ROOT, launch

OPS = ("D", "stagD2ee", "stagD2oo", "stagD_even", "stagD_odd")
_cache = {}


def _gauge(lat, seed=987654321):
    key = ("g", tuple(lat), seed)
    if key not in _cache:
        lo = o.Layout(lat)
        rf = o.RngField(lo, o.RNG_MILC6, seed)
        g = o.gauge_random(lo, rf)
        o.rephase(lo, g)
        x = o.vector_gaussian(lo, rf)
        _cache[key] = (lo, g, x)
    return _cache[key]


def _ctx(lat):
    import qex_amd as q

    key = ("ctx", tuple(lat))
    if key not in _cache:
        _cache[key] = q.Context(lat)
    return _cache[key]


def _ops(ctx, g, x, lossless):
    """Everything the sweeps compute on these links, with option lossless as given."""
    import qex_amd as q

    ctx.set_option("lossless", lossless)
    s = q.newStag(ctx, g)
    out = {"info": s.links_info(), "storage": s.links_storage()}
    r = np.zeros_like(x)
    s.D(r, x, 0.1)
    out["D"] = r.copy()
    for name in ("stagD2ee", "stagD2oo"):
        r = np.zeros_like(x)
        getattr(s, name)(r, x, 0.01)
        out[name] = r.copy()
    for par in ("even", "odd"):
        r = np.zeros_like(x)
        s.stagD(r, x, par, 0.1)
        out["stagD_" + par] = r.copy()
    return s, out


def _ref(lat, seed=987654321):
    """the 18-real results on the unmodified links of (lat, seed): computed once"""
    key = ("ref", tuple(lat), seed)
    if key not in _cache:
        _, g, x = _gauge(lat, seed)
        _cache[key] = _ops(_ctx(lat), g, x, 0)[1]
    return _cache[key]


def _stored(g):
    """the links as the operator stores them: every link forward, and its adjoint as the backward link of its neighbour"""
    m = g.reshape(-1, 3, 3, 2)
    return np.concatenate([m, np.ascontiguousarray(np.swapaxes(m, 1, 2) * np.array([1.0, -1.0]))])


def two_ranks(form, lat=(16, 16, 16, 32)):
    """tests/lossless_rank_worker.py on two ranks sharing one device: the two `LOSSLESS rank r {...}` records"""
    p = launch(2, [os.path.join(ROOT, "tests", "lossless_rank_worker.py"), form] + list(lat), 300)
    ok = [json.loads(ln.split(" ", 3)[3]) for ln in p.stdout.splitlines() if ln.startswith("LOSSLESS rank")]
    if p.returncode != 0 or len(ok) != 2:
        print(p.stdout[-3000:])
        print(p.stderr[-6000:])
    assert p.returncode == 0 and len(ok) == 2
    return ok
