"""Meson tables, symmetric shift and slice norms on the GPU (csrc/meson.hip; src/observables/fpvaMeas.nim, sources.nim:10-18).

The reference stores no meson numbers, so the kernels are pinned four ways: a numpy restatement on identical uploaded fields
(tests/meson_ref.py, itself checked against a site loop in tests/test_mesons.py), the oracle's CG for the whole fpvaMeas chain,
exact identities (table sums = redot / norm2), and gauge invariance of the colour-summed tables."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import qex_amd as q  # noqa: E402
import meson_ref as mr  # noqa: E402
from oracle import oracle as o  # noqa: E402
from ranks import launch  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 987654321


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("lat", [[8, 8, 8, 8], [4, 6, 10, 6], [12, 6, 6, 10]])
def test_contraction_against_numpy(lat):
    lo = q.Layout(lat)
    ctx = q.Context(lat)
    rng = np.random.default_rng(sum(lat))
    fs = [rng.standard_normal((lo.vol, 3, 2)) for _ in range(6)]
    ids = [ctx.field_new(f) for f in fs]
    nt = lat[3]
    for t0 in (0, 3, nt - 1):
        for n in (1, 3):
            xs, ys = ids[:n], ids[3:3 + n]
            got = ctx.dev_meson_corners(xs, ys, t0)
            ref = mr.local_mesons(lo, fs[:n], fs[3:3 + n], t0)
            assert got.shape == (nt, 8) and _rel(got, ref) < 1e-13, (t0, n, _rel(got, ref))
            assert np.array_equal(got, ctx.dev_meson_corners(xs, ys, t0))          # fixed reduction order: same bits again
            # identity: the whole table is the sum of the pairs' redot
            red = sum(ctx.dev_redot(a, b) for a, b in zip(xs, ys))
            assert abs(got.sum() - red) < 1e-12 * abs(red) + 1e-12 * np.abs(got).sum()
        # the rows are a cyclic relabelling of t: a t0 shift rolls the table exactly
        base = ctx.dev_meson_corners(ids[:3], ids[:3], 0)
        assert np.array_equal(ctx.dev_meson_corners(ids[:3], ids[:3], t0), np.roll(base, -t0, axis=0))
    # stagMesons(v) = stagLocalMesons(v, v, 0): sums to norm2(v)
    lines = []
    c = q.stagMesons(ctx, fs[0], out=lines.append)
    assert abs(c.sum() - ctx.norm2(fs[0])) < 1e-12 * c.sum()
    assert lines[0] == "corner: 0" and lines[8 * (nt + 1)] == "sum:" and len(lines) == 9 * (nt + 1)
    # host arrays and lists go through the same kernel
    assert np.array_equal(q.stagLocalMesons(ctx, fs[:3], fs[3:6], 3), ctx.dev_meson_corners(ids[:3], ids[3:6], 3))
    # slice norms along every direction
    for d in range(4):
        ref = np.zeros(lat[d])
        np.add.at(ref, lo.coords[:, d], (fs[1] ** 2).sum(axis=(1, 2)))
        got = q.norm2slice(ctx, ids[1], d)
        assert got.shape == (lat[d],) and _rel(got, ref) < 1e-14, (d, _rel(got, ref))
    for fid in ids:
        ctx.field_free(fid)


def test_bad_arguments_raise():
    lat = [4, 4, 4, 4]
    ctx = q.Context(lat)
    a, b = ctx.field_new(), ctx.field_new()
    with pytest.raises(q.QexHipError, match="no links"):
        ctx.dev_sym_shift(a, b, 0)
    with pytest.raises(q.QexHipError, match="n = 5"):
        ctx.dev_meson_corners([a] * 5, [b] * 5, 0)
    with pytest.raises(q.QexHipError, match="n = 0"):
        ctx.dev_meson_corners([], [], 0)
    with pytest.raises(q.QexHipError, match="unknown field"):
        ctx.dev_meson_corners([a, 999], [b, b], 0)
    with pytest.raises(q.QexHipError, match="t0"):
        ctx.dev_meson_corners([a], [b], 4)
    with pytest.raises(q.QexHipError, match="dir"):
        ctx.dev_norm2slice(a, 4)
    with pytest.raises(q.QexHipError, match="unknown field"):
        ctx.dev_norm2slice(12345, 0)


def _operators(lo, olo, rf):
    """(name, builder(ctx) -> Staggered, the host one-hop links it shifts with, expected format, tolerance)"""
    gw = o.gauge_warm(olo, 0.5, rf)
    o.rephase(olo, gw)                            # SU(3) x phases: format 1
    gr = o.gauge_random(olo, rf)
    o.rephase(olo, gr)                            # g.random: unitary to ~1e-11 only -> format 0
    gn = gr + 0.05 * np.random.default_rng(1).standard_normal(gr.shape)     # non-unitary
    g3 = 0.3 * gr
    g0 = o.gauge_warm(olo, 0.5, rf)
    sm = o.nhyp_smear(olo, g0, 0.4, 0.5, 0.5)
    o.rephase(olo, sm)
    return [
        ("format0", lambda ctx: q.newStag(ctx, gn), gn, 0, 1e-14),
        ("format1", lambda ctx: q.newStag(ctx, gw), gw, 1, 1e-14),
        ("format2", lambda ctx: q.newStag(ctx, 1.01 * gw), 1.01 * gw, 2, 1e-14),
        ("nhyp", lambda ctx: q.Staggered(ctx, g0, smear=q.HypCoefs(), bc="pppa"), sm, 2, 1e-12),   # smeared on the device
        ("naik", lambda ctx: q.newStag3(ctx, gr, g3), gr, None, 1e-14),
    ]


@pytest.mark.parametrize("lat", [[8, 8, 8, 8], [4, 6, 10, 6]])
def test_sym_shift_against_numpy(lat):
    lo, olo = q.Layout(lat), o.Layout(lat)
    rf = o.RngField(olo, o.RNG_MILC6, SEED)
    x = o.vector_gaussian(olo, rf)
    ctx = q.Context(lat)
    fx, fr = ctx.field_new(x), ctx.field_new()
    for name, build, g, fmt, tol in _operators(lo, olo, rf):
        s = build(ctx)
        n, f, _ = s.links_info()
        if fmt is not None:
            assert f == fmt, (name, f)
        else:
            assert n == 16
        for mu in range(3):
            ref = mr.sym_shift(lo, g, x, mu)
            s.symShift(fr, fx, mu)
            got = ctx.field_download(fr)
            assert _rel(got, ref) < tol, (name, mu, _rel(got, ref))
            h = np.zeros_like(x)
            s.symShift(h, x, mu)                     # host arrays
            assert np.array_equal(h, got)
        with pytest.raises(q.QexHipError, match="mu = 3"):
            s.symShift(fr, fx, 3)
        with pytest.raises(q.QexHipError, match="unknown field"):
            s.symShift(fr, 4242, 0)
        with pytest.raises(q.QexHipError):
            s.symShift(fx, fx, 0)


def _device_tables(lat, g, t0=2, mass=0.1, r2req=1e-20):
    lo = q.Layout(lat)
    ctx = q.Context(lat)
    s = q.newStag(ctx, g)
    cl, cs, st = q.localMesonTables(s, lo, mass, t0, r2req, maxits=20000)
    ctx.close()
    return [cl] + cs, st


@pytest.mark.parametrize("lat", [[8, 8, 8, 8], [4, 6, 8, 8]])
def test_fpva_pipeline_against_the_oracle(lat):
    """fpvaMeas.nim:112-127: propagators from the oracle's CG, shifts and contractions in numpy"""
    olo, lo = o.Layout(lat), q.Layout(lat)
    rf = o.RngField(olo, o.RNG_MILC6, SEED)
    g = o.gauge_random(olo, rf)
    o.rephase(olo, g)
    t0, m = 2, 0.1
    got, st = _device_tables(lat, g, t0, m)
    assert all(max(its) < 20000 for its in st["iterations"])
    cl, cs = mr.fpva_tables(lo, g, lambda b: o.solve(olo, g, None, b, m, 1e-20, 20000)[0], t0,
                            lambda ic: q.pointSource(lo, [0, 0, 0, t0], ic))
    for k, (a, b) in enumerate(zip(got, [cl] + cs)):
        assert _rel(a, b) < 1e-8, (k, _rel(a, b))
    # the local pion (corner 0 after the transform) is positive
    pion = q.printLocalMesons(got[0].copy(), out=lambda s: None)[:, 0]
    assert (pion > 0).all()


def test_tables_are_gauge_invariant():
    lat = [8, 8, 8, 8]
    olo, lo = o.Layout(lat), q.Layout(lat)
    rf = o.RngField(olo, o.RNG_MILC6, SEED + 1)
    g0 = o.gauge_warm(olo, 0.5, rf)
    om = o.gauge_random(olo, rf)[:, 0]                # one random SU(3) matrix per site
    Om = om[..., 0] + 1j * om[..., 1]
    G = g0[..., 0] + 1j * g0[..., 1]
    Gp = np.empty_like(G)
    for mu in range(4):
        fw, _ = mr.neighbours(lo, mu)
        Gp[:, mu] = Om @ G[:, mu] @ Om[fw].conj().transpose(0, 2, 1)
    g1 = np.ascontiguousarray(np.stack([Gp.real, Gp.imag], axis=-1))
    g, gp = g0.copy(), g1
    o.rephase(olo, g)
    o.rephase(olo, gp)
    a, _ = _device_tables(lat, g)
    b, _ = _device_tables(lat, gp)
    for k in range(4):
        assert _rel(b[k], a[k]) < 1e-9, (k, _rel(b[k], a[k]))


# ---- ranks: every rank its own process (torch.distributed.run), all sharing the one device, as tests/test_gpu_two_ranks.py ----
def _worker(nranks, lat):
    p = launch(nranks, [os.path.join(ROOT, "tests", "meson_rank_worker.py")] + lat, 600, env={"QEXHIP_PEER_TIMEOUT": "60"})
    # (the launcher multiplexes the ranks' output and may join two records on one line: match records, not lines)
    ok = re.findall(r"MESON_RANK_OK \d+ (\{[^{}]*\})", p.stdout)
    if p.returncode != 0 or len(ok) != nranks:
        print(p.stdout[-4000:])
        print(p.stderr[-8000:])
    assert p.returncode == 0 and len(ok) == nranks, (p.returncode, len(ok))
    res = [json.loads(r) for r in ok]
    assert len({r["digest"] for r in res}) == 1                     # every rank holds the whole table
    tabs = re.findall(r"MESON_TABLES (\{[^{}]*\})", p.stdout)      # {"name": [hex floats], ...}: no nested braces
    assert len(tabs) == 1
    return {"tables": json.loads(tabs[0])}


def test_ranks_give_bit_identical_tables():
    lat = [8, 8, 8, 16]
    one = _worker(1, lat)
    for n in (2, 4):
        r = _worker(n, lat)
        assert r["tables"] == one["tables"], n          # hex floats: bit for bit


def _example_tables(out):
    tabs, cur = [], None
    for ln in out.splitlines():
        if ln.startswith("corner: "):
            if ln == "corner: 0":
                tabs.append([])
            cur = []
            tabs[-1].append(cur)
        elif cur is not None and len(ln.split()) == 2 and ln.split()[0].isdigit():
            cur.append(float(ln.split()[1]))
    return np.array(tabs)


def test_example_on_one_and_two_ranks():
    lat = ["-lat", "8", "8", "8", "16"]
    ex = os.path.join(ROOT, "examples", "stag_mesons.py")
    p1 = subprocess.run([sys.executable, ex] + lat, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, cwd=ROOT)
    assert p1.returncode == 0, p1.stderr[-4000:]
    p2 = launch(2, [ex] + lat, 600, env={"QEXHIP_PEER_TIMEOUT": "60"})
    if p2.returncode != 0:
        print(p2.stdout[-4000:])
        print(p2.stderr[-8000:])
    assert p2.returncode == 0
    a, b = _example_tables(p1.stdout), _example_tables(p2.stdout)
    assert a.shape == (4, 8, 16) and b.shape == a.shape
    assert np.abs(a - b).max() < 1e-10 * np.abs(a).max()
