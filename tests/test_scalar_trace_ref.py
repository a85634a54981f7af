"""CPU checks of the stochastic scalar trace's host pieces: the numpy reference (tests/scalar_trace_ref.py) against a plain site
loop, the host Z4 / Z2 fills against the oracle's per-site uniforms, and parseDilution / the pattern order against
src/algorithms/dilution.nim."""
import ctypes as C

import numpy as np
import pytest

import scalar_trace_ref as R

LAT = [4, 4, 4, 8]


@pytest.fixture(scope="module")
def lo():
    import qex_amd as q

    return q.Layout(LAT)


@pytest.fixture(scope="module")
def fields(lo):
    rs = np.random.RandomState(11)
    return [rs.standard_normal((lo.vol, 3, 2)) for _ in range(3)]


@pytest.mark.parametrize("kind", [R.EO, R.CORNER])
def test_reference_dilution_is_the_site_loop(lo, fields, kind):
    src = fields[0]
    for t, idx in R.patterns(kind, LAT[3]):
        for scale in (1.0, 1.0 / np.sqrt(2.0)):
            want = np.zeros_like(src)
            for i in range(lo.vol):
                x = lo.coords[i]
                pat = (x[0] + x[1] + x[2] + x[3]) % 2 if kind == R.EO else (x[0] % 2) + 2 * (x[1] % 2) + 4 * (x[2] % 2)
                if x[3] == t and pat == idx:
                    want[i] = scale * src[i]
            assert np.array_equal(R.dilute(src, lo.coords, kind, idx, t, scale), want)


def test_reference_trace_and_slices_are_the_site_loop(lo, fields):
    a, b, c = fields
    trce = np.zeros((lo.vol, 2))
    R.accumulate(trce, a, b, 1.0)
    R.accumulate(trce, c, c, 0.1)
    want = np.zeros(lo.vol, dtype=complex)
    for i in range(lo.vol):
        for col in range(3):
            want[i] += complex(a[i, col, 0], -a[i, col, 1]) * complex(b[i, col, 0], b[i, col, 1])
            want[i] += 0.1 * (c[i, col, 0] ** 2 + c[i, col, 1] ** 2)
    assert np.abs(R.cplx(trce) - want).max() < 1e-13
    sl = np.zeros((LAT[3], 2))
    for i in range(lo.vol):
        sl[lo.coords[i][3]] += trce[i]
    assert np.abs(R.slice_sums(trce, lo.coords, LAT[3]) - sl).max() < 1e-12
    # the whole measurement with the identity "solver" phi = b / mass: improved and unimproved traces are then the same field
    t1, e1, _ = R.scalar_trace(lambda v: v / 0.5, a, lo.coords, LAT[3], 0.5, R.EO, True)
    t0, e0, _ = R.scalar_trace(lambda v: v / 0.5, a, lo.coords, LAT[3], 0.5, R.CORNER, False)
    want = R.site_dot(a, a) / 0.5 / 3
    assert np.abs(t1 - want).max() < 1e-13 and np.abs(t0 - want).max() < 1e-13
    assert np.abs(e1 - e0).max() < 1e-13 and abs(e1.sum() * 64 - want[:, 0].sum()) < 1e-10


@pytest.mark.parametrize("kind", [R.EO, R.CORNER])
def test_patterns_partition_every_time_slice(lo, kind):
    for t in range(LAT[3]):
        cover = np.zeros(lo.vol, dtype=int)
        for idx in range(R.NPAT[kind]):
            cover += R.mask(lo.coords, kind, idx, t)
        assert np.array_equal(cover, (lo.coords[:, 3] == t).astype(int))
    # EO patterns are the layout's even / odd halves (dilution.nim:25-28)
    if kind == R.EO:
        assert np.array_equal(R.pattern_of(lo.coords, R.EO), (np.arange(lo.vol) >= lo.nEven).astype(int))


def test_parse_dilution_and_pattern_order():
    import qex_amd as q

    eo, co = q.parseDilution("EO"), q.parseDilution("CORNER")
    assert eo == q.DilutionKind.dkEvenOdd == R.EO and co == q.DilutionKind.dkCorners3D == R.CORNER
    assert [(d.kind, d.idx) for d in q.dilution(eo)] == [(eo, 0), (eo, 1)]
    assert [(d.kind, d.idx) for d in q.dilution(co)] == [(co, i) for i in range(8)]
    assert [str(d) for d in q.dilution(eo)] == ["EvenOdd 0", "EvenOdd 1"] and str(list(q.dilution(co))[5]) == "Corners3D 5"
    assert str(eo) == "EO" and str(co) == "CORNER"
    with pytest.raises(ValueError):
        q.parseDilution("WALL")
    # the driver walks t outer, dl inner (scalarTrace.nim:169-170): the reference file's order
    for kind, dk in ((R.EO, eo), (R.CORNER, co)):
        assert R.patterns(kind, 4) == [(t, d.idx) for t in range(4) for d in q.dilution(dk)]


@pytest.mark.parametrize("seed", [987654321, 17 ** 7])
def test_host_z4_z2_are_the_thresholds_on_the_oracles_uniforms(oracle, seed):
    import qex_amd as q

    o = oracle
    olo = o.Layout(LAT)
    rf = o.RngField(olo, o.RNG_MILC6, seed)
    r = q.RngField(LAT, q.RngMilc6, seed)
    for fill, ref in ((r.z4_vector, R.z4_from_uniform), (r.z2_vector, R.z2_from_uniform), (r.z4_vector, R.z4_from_uniform)):
        u = np.zeros((olo.vol, 3))                       # the next three uniforms of every site's stream, as o.vector_u1 draws them
        o.lib().qo_field_uniform(olo._h, rf._h, 3, u.ctypes.data_as(C.c_void_p), 0)
        v = fill()
        assert v.shape == (olo.vol, 3, 2) and np.array_equal(v, ref(u))
    # every value of Z4 occurs, and the draws advanced the generator as three uniforms per fill do
    z = R.cplx(r.z4_vector())
    assert set(np.unique(z)) == {1, -1, 1j, -1j}
    r2 = q.RngField(LAT, q.RngMilc6, seed)
    r2.uniform(12)
    assert np.array_equal(r2.state(), r.state())


def test_host_z4_z2_mrg32k3a():
    import qex_amd as q

    a, b = q.RngField(LAT, q.MRG32k3a, 5), q.RngField(LAT, q.MRG32k3a, 5)
    u = b.uniform(6)
    assert np.array_equal(a.z4_vector(), R.z4_from_uniform(u[:, :3])) and np.array_equal(a.z2_vector(), R.z2_from_uniform(u[:, 3:]))
