// trace.hip -- the stochastic scalar trace on resident fields: time / even-odd / corner dilution of a noise source, the site-wise
// accumulation of <a, b> into a complex site field, and its per-timeslice sums.
//
//   k_dilute        dst_k(x) = scale * src(x) where t_glob(x) = t[k] and x is in pattern idx[k], +0.0 elsewhere, k < n <= 4
//                   (the `tmps{i} := eta{i}` loop of src/observables/scalarTrace.nim:169-185 over the sites of
//                   src/algorithms/dilution.nim:23-45, with the Gaussian source's 1/sqrt(2) of scalarTrace.nim:157-160 as `scale`)
//   k_trace_accum   trce(x) += coef * sum_col conj(a_k(x)[col]) b_k(x)[col], one k after the other (scalarTrace.nim:194-202)
//   k_cfield_slices partials of sum_{x: t(x) = t} trce(x), Re and Im (scalarTrace.nim:210-217)
//
// The complex site field ("cfield", lo.Complex): double2 d[parity][ntile*64], indexed by the same checkerboard site number c as a
// colour vector, so the lane that holds site c of a vector holds trce(c) too; 16 B per site, no ghost slices (nothing hops).
//
// Order of the accumulation: a lane adds the n terms to its trce(x) one at a time in ascending k, every product and sum rounded as
// written (no contraction), so n pairs in one launch leave the bits of n launches with one pair each: the trace does not depend on
// how the dilution patterns were grouped into batches.
//
// Determinism of the slice sums: the scheme of k_meson_corners / k_bins_final (meson.hip).  A workgroup covers 256 consecutive sites
// of ONE local t-slice, both parities; its partials are summed in chunk order by one workgroup into the zeroed global table, where
// every entry has exactly one non-zero contribution in the rank sum.  The chunking depends on the spatial extents only: the table is
// the same bit for bit run to run and for 1, 2 or 4 ranks.
#pragma clang fp contract(off)
#include "qexhip_internal.h"
#include "site_index.h"
#include "reduce.h"

namespace {

struct DiluteArgs {
  double2 *dst[2][4];   // [parity][k]
  int idx[4], t[4];
};

// one lane per site (both parities); src is read once, and only where one of the n time slices is the lane's
__global__ void __launch_bounds__(256) k_dilute(Geom g, DiluteArgs A, int n, int kind, int toff, double scale, const double2 *s0,
                                                const double2 *s1) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * g.Vh) return;
  int p, c; linear_site(g, i, p, c);
  const SiteXYZT s = site_coord(g, c, p);
  const int tg = s.t + toff;
  const int pat = kind == 0 ? ((2 * s.xh + s.o + s.y + s.z + tg) & 1) : (s.o | ((s.y & 1) << 1) | ((s.z & 1) << 2));
  bool any = false;
  for (int k = 0; k < n; k++) any = any || A.t[k] == tg;
  double2 v[3];
#pragma unroll
  for (int col = 0; col < 3; col++) v[col] = make_double2(0.0, 0.0);
  if (any) {
    const double2 *src = p ? s1 : s0;
#pragma unroll
    for (int col = 0; col < 3; col++) {
      const double2 e = src[vec_off(c, col)];
      v[col] = make_double2(scale * e.x, scale * e.y);
    }
  }
  for (int k = 0; k < n; k++) {
    const bool on = A.t[k] == tg && A.idx[k] == pat;
#pragma unroll
    for (int col = 0; col < 3; col++) A.dst[p][k][vec_off(c, col)] = on ? v[col] : make_double2(0.0, 0.0);
  }
}

struct AccumArgs {
  const double2 *a[2][4], *b[2][4];   // [parity][k]; a == b: the vector is loaded once and the imaginary part is exactly 0
};

__global__ void __launch_bounds__(256) k_trace_accum(Geom g, AccumArgs A, int n, double coef, double2 *tr0, double2 *tr1) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * g.Vh) return;
  int p, c; linear_site(g, i, p, c);
  double2 *tr = (p ? tr1 : tr0) + c;
  double2 acc = *tr;
  for (int k = 0; k < n; k++) {
    const double2 *a = A.a[p][k], *b = A.b[p][k];
    double re = 0.0, im = 0.0;
    if (a == b) {
#pragma unroll
      for (int col = 0; col < 3; col++) {
        const double2 x = a[vec_off(c, col)];
        re = fma(x.x, x.x, fma(x.y, x.y, re));
      }
    } else {
#pragma unroll
      for (int col = 0; col < 3; col++) {
        const double2 x = a[vec_off(c, col)], y = b[vec_off(c, col)];
        re = fma(x.x, y.x, fma(x.y, y.y, re));
        im = fma(x.x, y.y, fma(-x.y, y.x, im));
      }
    }
    acc.x += coef * re;
    acc.y += coef * im;
  }
  *tr = acc;
}

// grid: (local t-slices) x nchunk workgroups of 256; partials[(t*nchunk + chunk)*2 + {Re, Im}]
__global__ void __launch_bounds__(256) k_cfield_slices(Geom g, const double2 *tr0, const double2 *tr1, int nchunk, double *partials) {
  const int t = blockIdx.x / nchunk, chunk = blockIdx.x - t * nchunk;
  const int i = chunk * 256 + threadIdx.x;
  double2 v = make_double2(0.0, 0.0);
  if (i < g.F) {
    const int c = t * g.F + i;
    const double2 e = tr0[c], o = tr1[c];
    v = make_double2(e.x + o.x, e.y + o.y);
  }
  const double re = block_sum_256(v.x), im = block_sum_256(v.y);
  if (threadIdx.x == 0) {
    partials[(size_t)blockIdx.x * 2] = re;
    partials[(size_t)blockIdx.x * 2 + 1] = im;
  }
}

__global__ void __launch_bounds__(256) k_cfield_scale(int n, double s, double2 *tr0, double2 *tr1) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * n) return;
  double2 *d = i >= n ? tr1 + (i - n) : tr0 + i;
  const double2 e = *d;
  *d = make_double2(s * e.x, s * e.y);
}

// dst += a * src on the body sites of both parities, product and sum rounded as written
__global__ void __launch_bounds__(256) k_cfield_axpy(int n, double a, double2 *d0, double2 *d1, const double2 *s0, const double2 *s1) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * n) return;
  double2 *d = i >= n ? d1 + (i - n) : d0 + i;
  const double2 s = i >= n ? s1[i - n] : s0[i], e = *d;
  *d = make_double2(e.x + a * s.x, e.y + a * s.y);
}

// host[p*Vh + c] = trce of parity p, site c: the V=1 even-odd site order of field_download
__global__ void __launch_bounds__(256) k_cfield_to_host(int n, double2 *__restrict__ host, const double2 *tr0, const double2 *tr1) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * n) return;
  host[i] = i >= n ? tr1[i - n] : tr0[i];
}

}  // namespace

int cfield_alloc(qexhip_ctx *c, DevCField &f) {
  f.half = (size_t)c->g.ntile * 64;
  HIPCHK(hipMalloc((void **)&f.d, 2 * f.half * sizeof(double2)));
  HIPCHK(hipMemsetAsync(f.d, 0, 2 * f.half * sizeof(double2), c->stream));
  return 0;
}

int cfield_zero(qexhip_ctx *c, DevCField &f) {
  HIPCHK(hipMemsetAsync(f.d, 0, 2 * f.half * sizeof(double2), c->stream));
  return 0;
}

int cfield_scale(qexhip_ctx *c, DevCField &f, double s) {
  ScopedTimer tm(c, "trace", c->stream);
  k_cfield_scale<<<(2 * c->g.Vh + 255) / 256, 256, 0, c->stream>>>(c->g.Vh, s, f.par(0), f.par(1));
  HIPCHK(hipGetLastError());
  return 0;
}

int cfield_axpy(qexhip_ctx *c, DevCField &dst, double a, const DevCField &src) {
  ScopedTimer tm(c, "trace", c->stream);
  k_cfield_axpy<<<(2 * c->g.Vh + 255) / 256, 256, 0, c->stream>>>(c->g.Vh, a, dst.par(0), dst.par(1), src.par(0), src.par(1));
  HIPCHK(hipGetLastError());
  return 0;
}

int cfield_download(qexhip_ctx *c, const DevCField &f, double *host) {
  const size_t bytes = (size_t)c->g.V * sizeof(double2);
  CHK(ensure_stage(c, bytes));
  k_cfield_to_host<<<(2 * c->g.Vh + 255) / 256, 256, 0, c->stream>>>(c->g.Vh, (double2 *)c->stage, f.par(0), f.par(1));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(host, c->stage, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int trace_dilute(qexhip_ctx *c, int n, DevField *const *dst, const DevField &src, int kind, const int *idx, const int *t, double scale) {
  const Geom &g = c->g;
  DiluteArgs A{};
  for (int k = 0; k < n; k++) {
    A.dst[0][k] = dst[k]->par(0);
    A.dst[1][k] = dst[k]->par(1);
    A.idx[k] = idx[k];
    A.t[k] = t[k];
  }
  ScopedTimer tm(c, "trace", c->stream);
  k_dilute<<<(2 * g.Vh + 255) / 256, 256, 0, c->stream>>>(g, A, n, kind, g.X[3] * c->rankCoord[3], scale, src.par(0), src.par(1));
  HIPCHK(hipGetLastError());
  return 0;
}

int trace_accum(qexhip_ctx *c, DevCField &tr, int n, DevField *const *a, DevField *const *b, double coef) {
  const Geom &g = c->g;
  AccumArgs A{};
  for (int k = 0; k < n; k++)
    for (int p = 0; p < 2; p++) { A.a[p][k] = a[k]->par(p); A.b[p][k] = b[k]->par(p); }
  ScopedTimer tm(c, "trace", c->stream);
  k_trace_accum<<<(2 * g.Vh + 255) / 256, 256, 0, c->stream>>>(g, A, n, coef, tr.par(0), tr.par(1));
  HIPCHK(hipGetLastError());
  return 0;
}

int cfield_slices(qexhip_ctx *c, const DevCField &tr, double *host_out) {
  const Geom &g = c->g;
  const int ntg = g.X[3] * c->rankGeom[3], toff = g.X[3] * c->rankCoord[3];
  const int nchunk = (g.F + 255) / 256, nblk = g.X[3] * nchunk;
  double *part, *out;
  CHK(meson_scratch(c, (size_t)nblk * 2, (size_t)ntg * 2, &part, &out));
  HIPCHK(hipMemsetAsync(out, 0, (size_t)ntg * 2 * sizeof(double), c->stream));
  {
    ScopedTimer tm(c, "trace", c->stream);
    k_cfield_slices<<<nblk, 256, 0, c->stream>>>(g, tr.par(0), tr.par(1), nchunk, part);
    HIPCHK(hipGetLastError());
    CHK(meson_bins_final(c, part, g.X[3], 2, nchunk, toff, 0, ntg, out));
  }
  if (multi_rank(c)) CHK(comm_allreduce(c, out, ntg * 2));
  return meson_read_table(c, out, (size_t)ntg * 2, host_out);
}
