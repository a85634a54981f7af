"""The eigenvector block kernels of eig.hip (block dot, block axpy, in-place rotation and the multi-right-hand-side forms of the
first two) against numpy at the sizes the eigensolver and the deflated solves use them: more than 128 vectors, every
instantiation of k_rotate, the large-LDS launches, and every grid-stride loop wrapped.

Two kinds of data.
  * Integer data (eig_ref.int_pattern / int_matrix): vectors in -8 .. 7, Q and the real and imaginary parts of the axpy
    coefficients in {-2, -1, 1, 2} (no zeros: every input counts in every output).  Every partial sum stays far below 2^53
    (asserted), so every product and fma is exact in any order and the device result must be np.array_equal to the integer
    reference.
  * Gaussian data against a reference accumulated in np.longdouble, with the bound of the kernel's own summation (u = 2^-53):
      rotation   |got - ref| <= 2 m u (|V| @ |Q|)                      one fma chain of m terms per output
      axpy       |got - ref| <= 2 (2n + 1) u (|V| @ |coef| + |y|)      two fmas per vector, one for y
      block dot  |got - ref| <= D u sum_i |v_i| |w_i|,  D = 6 (colour chain) + 6 (wave_sum) + ceil(ntile / (4 nwg)) (tiles of a
                 wave) + 2 (four waves) + ceil(nwg / 256) (k_block_dot_final's loop) + 8 (block_sum_256)
    The worst ratio to the bound is printed (pytest -s).

Lattices: 4.6.4.6 (288 even sites = 4.5 tiles, one basis of 512 vectors) for the sizes in the number of vectors; 30.30.30.22
(297000 even sites, 4641 tiles, ragged) and 14.14.14.34 (46648 even sites, 729 tiles, ragged) are the smallest that wrap the
grid-stride loops -- the conditions are asserted against the caps read from eig.hip, so a changed cap cannot turn these tests
into no-ops unnoticed."""
import os
import re

import numpy as np
import pytest

import eig_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SMALL, BIG, MID = (4, 6, 4, 6), (30, 30, 30, 22), (14, 14, 14, 34)
NB = 512          # vectors of the small lattice's basis = EIG_MAX_NVECS


def caps():
    """the chunk size and the grid caps of eig.hip, read from its source"""
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qex_amd", "csrc", "eig.hip")) as f:
        src = f.read()

    def one(pat):
        m = re.search(pat, src)
        assert m, "eig.hip no longer matches %r: update the size conditions of this module" % pat
        return int(m.group(1))

    return dict(nj=one(r"#define EIG_NJ (\d+)"), dot_wg=one(r"#define EIG_DOT_WG (\d+)"),
                axpy_wg=one(r"grid_for\(size_t n2\) \{ return \(int\)std::min<size_t>\((\d+),"),
                rot_wg=one(r"std::min<size_t>\(nblk, (\d+)\)"))


def rot_R(m):
    return 64 if m <= 128 else 32 if m <= 256 else 16


class Rig:
    """a context, a basis and two resident fields for moving vectors; `tag` remembers which data set a basis vector holds"""

    def __init__(self, lat, nvecs):
        import qex_amd as q

        self.ctx = q.Context(list(lat), device=0)
        lat_seen = [int(v) for v in re.search(r"local=(\d+)x(\d+)x(\d+)x(\d+)", self.ctx.info()).groups()]
        assert lat_seen == list(lat)
        self.vol = int(np.prod(lat_seen))
        self.vh = self.vol // 2
        self.ntile = -(-self.vh // 64)
        self.n2 = self.ntile * 192
        self.B = q.EigBasis(self.ctx, nvecs)
        self.up, self.down = self.ctx.field_new(), self.ctx.field_new()
        self.buf = np.zeros((self.vol, 3, 2))
        self.tag = [None] * nvecs

    def put(self, i, even, tag=None):
        self.buf[:self.vh] = even
        self.ctx.field_upload(self.up, self.buf)
        self.B.set_vector(i, self.up)
        self.tag[i] = tag

    def ensure(self, tag, data, n):
        """basis vectors 0 .. n-1 hold data[..., i]"""
        for i in range(n):
            if self.tag[i] != tag:
                self.put(i, data[..., i], tag)

    def get(self, i):
        """(even half of basis vector i, its |v|^2 over the whole tiles: the spare lanes of the ragged tile included)"""
        self.B.get_vector(i, self.down)
        return self.ctx.field_download(self.down)[:self.vh], self.ctx.dev_norm2(self.down, "even")

    def field(self, even, odd):
        f = np.empty((self.vol, 3, 2))
        f[:self.vh], f[self.vh:] = even, odd
        return self.ctx.field_new(f), f

    def dot_depth(self, dot_wg):
        nwg = min(dot_wg, -(-self.ntile // 4))
        return 6 + 6 + -(-self.ntile // (4 * nwg)) + 2 + -(-nwg // 256) + 8

    def close(self):
        self.B.free()
        self.ctx.close()


def cdot_int(v, w):
    """<v_j, w> of integer data: v (vh, 3, 2, n), w (vh, 3, 2) -> (re, im) as int64, with the premise of exactness checked"""
    v, w = v.astype(np.int64), w.astype(np.int64)
    vr, vi, wr, wi = v[:, :, 0], v[:, :, 1], w[:, :, 0], w[:, :, 1]
    dot = lambda a, b: np.tensordot(a, b, axes=([0, 1], [0, 1]))
    re, im = dot(vr, wr) + dot(vi, wi), dot(vr, wi) - dot(vi, wr)
    assert np.abs(v).max() * np.abs(w).max() * 4 * v.shape[0] * 3 < 2 ** 53      # every partial sum, in any order
    assert max(np.abs(re).max(), np.abs(im).max()) < 2 ** 53
    return re, im


def caxpy_int(v, coef, y):
    """y + sum_j coef_j v_j of integer data: v (vh, 3, 2, n), coef complex (n,), y (vh, 3, 2) -> int64 (vh, 3, 2)"""
    v = v.astype(np.int64)
    cr, ci = np.rint(coef.real).astype(np.int64), np.rint(coef.imag).astype(np.int64)
    out = y.astype(np.int64).copy()
    out[..., 0] += v[:, :, 0] @ cr - v[:, :, 1] @ ci
    out[..., 1] += v[:, :, 0] @ ci + v[:, :, 1] @ cr
    assert np.abs(v).max() * 2 * 2 * len(coef) + np.abs(y).max() < 2 ** 53
    assert np.abs(out).max() < 2 ** 53
    return out


def int_coef(n, salt):
    c = R.int_matrix(n, 2, salt=salt)
    return c[:, 0] + 1j * c[:, 1]


def cplx(f):
    """(..., 3, 2[, n]) real/imag pairs on axis 2 -> complex"""
    return f[:, :, 0] + 1j * f[:, :, 1]


def dot_bound_ratio(got, V, w, depth):
    """worst |got - ref| / bound over the real and imaginary parts; V complex (sites, 3, n), w complex (sites, 3)"""
    Vl, wl = V.astype(np.clongdouble), w.astype(np.clongdouble)
    ref = np.tensordot(Vl.conj(), wl, axes=([0, 1], [0, 1]))
    bound = depth * U * np.tensordot(np.abs(V), np.abs(w), axes=([0, 1], [0, 1]))
    d = got.astype(np.clongdouble) - ref
    return float(max((np.abs(d.real) / bound).max(), (np.abs(d.imag) / bound).max()))


# ---------------------------------------------------------------- 4.6.4.6, 512 vectors
@pytest.fixture(scope="module")
def small():
    rig = Rig(SMALL, NB)
    assert rig.vh == 288 and rig.vh % 64 == 32
    rig.caps = caps()
    rig.Vint = R.int_pattern(rig.vh, range(NB)).astype(np.float64)
    rng = np.random.default_rng(R.SEED + 1)
    rig.Vg = rng.standard_normal((rig.vh, 3, 2, NB))
    rig.wg = [rng.standard_normal((rig.vol, 3, 2)) for _ in range(4)]
    rows = rig.Vint.reshape(-1, NB)
    assert len(np.unique(rows.T, axis=0)) == NB, "two integer vectors are alike"
    yield rig
    rig.close()


def _rotation_checked_exactly(rig, V, nvecs, m, k, salt, chunk=1 << 15):
    """rotate (m, k) with integer Q on a basis that holds the integer vectors V (int8 or float64, (vh, 3, 2, nvecs)), then read all
    nvecs vectors back: 0 .. k-1 the exact product, k .. nvecs-1 untouched, the spare lanes of the ragged tile still zero"""
    Q = R.int_matrix(m, k, salt=salt)
    assert len(np.unique(Q.T, axis=0)) == k, "two columns of Q are alike"
    rows = V.reshape(-1, nvecs)
    ref = np.concatenate([R.exact_matmul(rows[r:r + chunk, :m], Q) for r in range(0, rows.shape[0], chunk)])
    assert np.abs(ref).max() < 2 ** 53
    rig.B.rotate(Q)
    rig.tag[:k] = [None] * k
    for i in range(nvecs):
        x, n2 = rig.get(i)
        want = ref[:, i].reshape(rig.vh, 3, 2) if i < k else V[..., i]
        assert np.array_equal(x, want), "m = %d k = %d: vector %d %s" % (m, k, i, "is not V Q" if i < k else "was touched")
        assert n2 == float(np.square(x).sum()), "m = %d k = %d: vector %d has non-zero spare lanes" % (m, k, i)


@pytest.mark.parametrize("m", [64, 65, 128, 129, 256, 257, 512])
def test_rotation_exact_at_every_instantiation_and_edge(small, m):
    """64 is the last m without the LDS opt-in and 65 the first with it, 128 | 129 and 256 | 257 straddle the changes of R, 512 is
    the cap; k = 4G - 1, 4G, 4G + 1 (G = 256 / R) are around the end of the column loop's first pass, k = m runs it to the end"""
    G = 256 // rot_R(m)
    for k in sorted({k for k in (1, 4 * G - 1, 4 * G, 4 * G + 1, m) if k <= m}):
        small.ensure("int", small.Vint, NB)
        _rotation_checked_exactly(small, small.Vint, NB, m, k, salt=m)


def test_exact_matmul_is_the_int64_product(small):
    rows = small.Vint.reshape(-1, NB)[:, :65]
    Q = R.int_matrix(65, 17, salt=3)
    assert np.array_equal(R.exact_matmul(rows, Q), rows.astype(np.int64) @ Q.astype(np.int64))


DOT_CASES = [(0, 127), (0, 128), (0, 129), (0, 256), (0, 257), (0, 512), (5, 200)]


def _int_field(rig, salt):
    """a resident field of integer data on both parities: (id, host copy)"""
    return rig.field(R.int_pattern(rig.vh, [0], salt=salt)[..., 0], R.int_pattern(rig.vh, [0], salt=salt + 1)[..., 0])


@pytest.mark.parametrize("i0,n", DOT_CASES)
def test_block_dot_exact_beyond_one_chunk(small, i0, n):
    small.ensure("int", small.Vint, NB)
    wid, w = _int_field(small, 1)
    try:
        got = small.B.block_dot(i0, n, wid)
    finally:
        small.ctx.field_free(wid)
    re, im = cdot_int(small.Vint[..., i0:i0 + n], w[:small.vh])
    assert np.array_equal(got.real, re) and np.array_equal(got.imag, im)


@pytest.mark.parametrize("nrhs", [1, 2, 3, 4])
def test_block_dot_multi_exact_beyond_one_chunk(small, nrhs):
    """n = 300: three chunks, and the row stride 2 n of the whole call in k_block_dot_final_mrhs"""
    small.ensure("int", small.Vint, NB)
    fs = [_int_field(small, 10 + 2 * k) for k in range(nrhs)]
    try:
        for i0, n in [(0, 128), (0, 129), (0, 300), (5, 200)]:
            got = small.B.block_dot_multi(i0, n, [f[0] for f in fs])
            for k in range(nrhs):
                re, im = cdot_int(small.Vint[..., i0:i0 + n], fs[k][1][:small.vh])
                assert np.array_equal(got[k].real, re) and np.array_equal(got[k].imag, im), (n, k)
    finally:
        for f in fs:
            small.ctx.field_free(f[0])


@pytest.mark.parametrize("i0,n", DOT_CASES)
def test_block_axpy_and_multi_exact_beyond_128_vectors(small, i0, n):
    ctx, vh = small.ctx, small.vh
    small.ensure("int", small.Vint, NB)
    coef = np.stack([int_coef(n, 20 + k) for k in range(4)])
    assert len(np.unique(coef, axis=0)) == 4
    fs = [_int_field(small, 30 + 2 * k) for k in range(4)]
    one, y1 = _int_field(small, 30)
    try:
        small.B.block_axpy(i0, coef[0], one)
        got = ctx.field_download(one)
        assert np.array_equal(got[:vh], caxpy_int(small.Vint[..., i0:i0 + n], coef[0], y1[:vh]))
        assert np.array_equal(got[vh:], y1[vh:]), "block axpy touched the odd half"
        small.B.block_axpy_multi(i0, coef, [f[0] for f in fs])
        for k in range(4):
            got = ctx.field_download(fs[k][0])
            assert np.array_equal(got[:vh], caxpy_int(small.Vint[..., i0:i0 + n], coef[k], fs[k][1][:vh])), k
            assert np.array_equal(got[vh:], fs[k][1][vh:]), "block axpy multi touched the odd half"
    finally:
        for f in fs + [(one,)]:
            ctx.field_free(f[0])


# Gaussian data from here on: the tests above leave integer vectors in the basis, `ensure` replaces them once
@pytest.mark.parametrize("m,k", [(128, 64), (256, 128), (512, 256)])
def test_rotation_gaussian_within_the_fma_chain_bound(small, m, k):
    small.ensure("gauss", small.Vg, NB)
    Q = np.random.default_rng(m).uniform(-1, 1, (m, k))
    rows = small.Vg.reshape(-1, NB)[:, :m]
    ref = rows.astype(np.longdouble) @ Q.astype(np.longdouble)
    bound = 2 * m * U * (np.abs(rows) @ np.abs(Q))
    small.B.rotate(Q)
    small.tag[:k] = [None] * k
    got = np.stack([small.get(i)[0].reshape(-1) for i in range(k)], axis=1)
    ratio = float((np.abs(got - ref) / bound).max())
    print("rotate m = %d k = %d (R = %d): worst |got - ref| / bound %.3g" % (m, k, rot_R(m), ratio))
    assert ratio <= 1.0
    for i in sorted({k, m - 1, min(m, NB - 1), NB - 1}):       # left as they were: k .. m-1 and m .. 511
        assert np.array_equal(small.get(i)[0], small.Vg[..., i]), i


def test_block_dot_chunks_are_the_same_kernel_on_the_same_tiles(small):
    """block_dot(i0, 200) = block_dot(i0, 128) ++ block_dot(i0 + 128, 72) bit for bit, and within the summation bound"""
    small.ensure("gauss", small.Vg, NB)
    wid = small.ctx.field_new(small.wg[0])
    try:
        for i0 in (0, 5):
            whole = small.B.block_dot(i0, 200, wid)
            parts = np.concatenate([small.B.block_dot(i0, 128, wid), small.B.block_dot(i0 + 128, 72, wid)])
            assert np.array_equal(whole, parts), i0
            ratio = dot_bound_ratio(whole, cplx(small.Vg[..., i0:i0 + 200]), cplx(small.wg[0][:small.vh]), small.dot_depth(small.caps["dot_wg"]))
            print("block dot n = 200 i0 = %d: worst |got - ref| / bound %.3g (depth %d)" % (i0, ratio, small.dot_depth(small.caps["dot_wg"])))
            assert ratio <= 1.0
    finally:
        small.ctx.field_free(wid)


@pytest.mark.parametrize("n", [128, 129, 300])
@pytest.mark.parametrize("nrhs", [1, 2, 3, 4])
def test_block_dot_multi_rows_are_block_dot_bit_for_bit(small, nrhs, n):
    small.ensure("gauss", small.Vg, NB)
    ids = [small.ctx.field_new(w) for w in small.wg[:nrhs]]
    try:
        multi = small.B.block_dot_multi(0, n, ids)
        assert multi.shape == (nrhs, n)
        worst = 0.0
        for k in range(nrhs):
            assert np.array_equal(multi[k], small.B.block_dot(0, n, ids[k])), (k, "row differs from block_dot of that w alone")
            worst = max(worst, dot_bound_ratio(multi[k], cplx(small.Vg[..., :n]), cplx(small.wg[k][:small.vh]), small.dot_depth(small.caps["dot_wg"])))
        print("block dot multi nrhs = %d n = %d: worst |got - ref| / bound %.3g" % (nrhs, n, worst))
        assert worst <= 1.0
    finally:
        for f in ids:
            small.ctx.field_free(f)


@pytest.mark.parametrize("i0,n", [(0, 128), (0, 129), (0, 300), (5, 200), (0, 512)])
@pytest.mark.parametrize("nrhs", [1, 2, 3, 4])
def test_block_axpy_multi_is_block_axpy_bit_for_bit_and_within_the_bound(small, nrhs, i0, n):
    ctx, vh = small.ctx, small.vh
    small.ensure("gauss", small.Vg, NB)
    rng = np.random.default_rng(1000 * nrhs + n)
    coef = rng.standard_normal((nrhs, n)) + 1j * rng.standard_normal((nrhs, n))
    ids = [ctx.field_new(w) for w in small.wg[:nrhs]]
    one = ctx.field_new()
    V = cplx(small.Vg[..., i0:i0 + n]).reshape(-1, n)
    try:
        small.B.block_axpy_multi(i0, coef, ids)
        worst = 0.0
        for k in range(nrhs):
            ctx.field_upload(one, small.wg[k])
            small.B.block_axpy(i0, coef[k], one)
            got, want = ctx.field_download(ids[k]), ctx.field_download(one)
            assert np.array_equal(got, want), (k, "differs from block_axpy with that system's coefficients")
            assert np.array_equal(got[vh:], small.wg[k][vh:]), "the odd half was touched"
            y = cplx(small.wg[k][:vh]).reshape(-1)
            ref = y.astype(np.clongdouble) + V.astype(np.clongdouble) @ coef[k].astype(np.clongdouble)
            bound = 2 * (2 * n + 1) * U * (np.abs(V) @ np.abs(coef[k]) + np.abs(y))
            d = cplx(got[:vh]).reshape(-1).astype(np.clongdouble) - ref
            worst = max(worst, float((np.abs(d.real) / bound).max()), float((np.abs(d.imag) / bound).max()))
        print("block axpy nrhs = %d n = %d i0 = %d: worst |got - ref| / bound %.3g" % (nrhs, n, i0, worst))
        assert worst <= 1.0
    finally:
        for f in ids + [one]:
            ctx.field_free(f)


# ---------------------------------------------------------------- 30.30.30.22: every grid-stride loop of R = 64 and of the dots / axpys
@pytest.fixture(scope="module")
def big():
    rig = Rig(BIG, 5)
    cp = rig.caps = caps()
    nwg = min(cp["dot_wg"], -(-rig.ntile // 4))
    assert rig.vh % 64 != 0, "the last tile is not ragged"
    assert rig.ntile > 4 * cp["dot_wg"], "the tile loop of the block dots does not wrap"
    assert nwg > 256, "k_block_dot_final sums one partial per thread"
    assert rig.n2 > 256 * cp["axpy_wg"], "the element loops of k_block_axpy / k_eig_copy_scale do not wrap"
    assert -(-rig.n2 // 64) > cp["rot_wg"], "the block loop of k_rotate<64> does not wrap"
    rig.Vint = R.int_pattern(rig.vh, range(5))
    tiles = rig.Vint[:rig.vh // 64 * 64].reshape(rig.vh // 64, -1)
    assert len(np.unique(tiles, axis=0)) == rig.vh // 64, "two tiles of the integer vectors are alike"
    yield rig
    rig.close()


def test_wrapped_all_ones_count_exactly(big):
    """all-ones vectors and w: <v, w> = 3 Vh exactly -- every tile once, the spare lanes of the ragged tile not at all"""
    ones = np.zeros((big.vh, 3, 2))
    ones[..., 0] = 1.0
    for i in range(3):
        big.put(i, ones)
    c = big.B.block_dot(0, 3, big.up)
    print("all-ones block dot on %s:" % (BIG,), c)
    assert 3 * big.vh == 891000 and np.all(c == 891000.0)


def test_wrapped_block_dot_and_multi_exact(big):
    big.ensure("int", big.Vint, 5)
    fs = [_int_field(big, 10 + 2 * k) for k in range(4)]
    try:
        single = big.B.block_dot(0, 5, fs[0][0])
        multi = big.B.block_dot_multi(0, 5, [f[0] for f in fs])
        for k in range(4):
            re, im = cdot_int(big.Vint, fs[k][1][:big.vh])
            assert np.array_equal(multi[k].real, re) and np.array_equal(multi[k].imag, im), k
        assert np.array_equal(single, multi[0])
    finally:
        for f in fs:
            big.ctx.field_free(f[0])


def test_wrapped_block_axpy_and_multi_exact(big):
    ctx, vh = big.ctx, big.vh
    big.ensure("int", big.Vint, 5)
    coef = np.stack([int_coef(5, 20 + k) for k in range(4)])
    fs = [_int_field(big, 30 + 2 * k) for k in range(4)]
    one, y1 = _int_field(big, 30)
    try:
        big.B.block_axpy(0, coef[0], one)
        got = ctx.field_download(one)
        assert np.array_equal(got[:vh], caxpy_int(big.Vint, coef[0], y1[:vh]))
        assert np.array_equal(got[vh:], y1[vh:]), "block axpy touched the odd half"
        big.B.block_axpy_multi(0, coef, [f[0] for f in fs])
        for k in range(4):
            got = ctx.field_download(fs[k][0])
            assert np.array_equal(got[:vh], caxpy_int(big.Vint, coef[k], fs[k][1][:vh])), k
            assert np.array_equal(got[vh:], fs[k][1][vh:]), "block axpy multi touched the odd half"
    finally:
        for f in fs + [(one,)]:
            ctx.field_free(f[0])


def test_wrapped_rotation_exact(big):
    big.ensure("int", big.Vint, 5)
    _rotation_checked_exactly(big, big.Vint, 5, 5, 3, salt=5)


def test_wrapped_copy_round_trip(big):
    """set_vector then vector: k_eig_copy_scale both ways, bit for bit"""
    v = np.random.default_rng(7).standard_normal((big.vh, 3, 2))
    big.put(4, v)
    x, _ = big.get(4)
    assert np.array_equal(x, v)


# ---------------------------------------------------------------- 14.14.14.34: the block loops of k_rotate<32> and k_rotate<16>
@pytest.fixture(scope="module")
def mid():
    rig = Rig(MID, 257)
    assert rig.vh % 64 != 0, "the last tile is not ragged"
    rig.caps = caps()
    rig.Vint = R.int_pattern(rig.vh, range(257))
    yield rig
    rig.close()


@pytest.mark.parametrize("m,k", [(129, 33), (257, 65)])
def test_wrapped_rotation_of_the_narrow_instantiations(mid, m, k):
    """(129, 33): R = 32, (257, 65): R = 16; both with more blocks than workgroups and a second pass of the column loop"""
    r = rot_R(m)
    assert r == (32 if m == 129 else 16) and k > 4 * (256 // r)
    assert -(-mid.n2 // r) > mid.caps["rot_wg"], "the block loop of k_rotate<%d> does not wrap" % r
    mid.ensure("int", mid.Vint, 257)
    _rotation_checked_exactly(mid, mid.Vint, 257, m, k, salt=m)
