// meson.hip -- local staggered meson tables, the symmetric one-link shift and slice norms on resident fields.
//
//   k_meson_corners  C[t][s] = sum_k sum_{x: t(x) = t, corner(x) = s} Re<x_k(x), y_k(x)>,  corner = (x0&1) | (x1&1)<<1 | (x2&1)<<2
//                    (stagLocalMesons, src/observables/fpvaMeas.nim:33-61; stagMesons, src/physics/stagMesonLocal.nim:14-51)
//   k_sym_shift      r(x) = U_mu(x) x(x+mu) + U_mu(x-mu)^+ x(x-mu), mu spatial (symShift, fpvaMeas.nim:16-31)
//   k_norm2slice     c[v] = sum_{x: x_dir = v} |f(x)|^2 (norm2slice, src/observables/sources.nim:10-18)
//
// Determinism of the t-tables: a workgroup of k_meson_corners covers 256 consecutive sites of ONE t-slice of the rank-local
// lattice (a slice of one parity is the contiguous range [t*F, (t+1)*F)), both parities of them, so its partials belong to one t
// whatever F is and wherever the slice falls relative to the 64-site tiles.  Lane partials -> wave shuffle -> LDS -> eight partials
// per workgroup; one workgroup then sums the partials of every (t, s) in chunk order.  The chunking of a slice depends on the
// spatial extents only, so 1, 2 or 4 ranks compute every entry with the same operations, and in the rank sum of the zeroed global
// table every entry has exactly one non-zero contribution: the tables agree bit for bit across partitions.
#include "qexhip_internal.h"
#include "site_index.h"
#include "reduce.h"
#include "dslash_core.h"

namespace {

struct MesonPairs {
  const double2 *x[2][4], *y[2][4];   // [parity][pair]
};

// grid: (local t-slices) x nchunk workgroups of 256; partials[(t*nchunk + chunk)*8 + s]
__global__ void __launch_bounds__(256) k_meson_corners(Geom g, MesonPairs P, int n, int nchunk, double *partials) {
  __shared__ double sm[4][8];
  const int t = blockIdx.x / nchunk, chunk = blockIdx.x - t * nchunk;
  const int i = chunk * 256 + threadIdx.x;
  double v[2] = {0.0, 0.0};                 // by x0&1 of the site: 0 / 1
  int syz = 0;                              // (x1&1)<<1 | (x2&1)<<2 (the same for both parities at one c)
  if (i < g.F) {
    const int c = t * g.F + i;
    const SiteXYZT s = site_coord(g, c, 0);
    syz = ((s.y & 1) << 1) | ((s.z & 1) << 2);
#pragma unroll
    for (int p = 0; p < 2; p++) {
      double a = 0.0;
      for (int k = 0; k < n; k++) {
#pragma unroll
        for (int col = 0; col < 3; col++) {
          const double2 xv = P.x[p][k][vec_off(c, col)], yv = P.y[p][k][vec_off(c, col)];
          a = fma(xv.x, yv.x, fma(xv.y, yv.y, a));
        }
      }
      const int o = (s.y + s.z + s.t + p) & 1;    // x0&1 of the parity-p site at c
      v[o] += a;
    }
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int s = 0; s < 8; s++) {
    const double r = wave_sum((s & 6) == syz ? v[s & 1] : 0.0);
    if (lane == 0) sm[w][s] = r;
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    const int s = threadIdx.x;
    partials[(size_t)blockIdx.x * 8 + s] = (sm[0][s] + sm[1][s]) + (sm[2][s] + sm[3][s]);
  }
}

// one workgroup: out[dst(b)*nsub + s] = sum over chunks, in chunk order, of partials[(b*nchunk + chunk)*nsub + s] for every local
// bin b; dst(b) = (b + off - t0) mod nglob (the row of the global table; t0 = 0, off = 0 and nglob = nbin: the identity)
__global__ void __launch_bounds__(256) k_bins_final(const double *partials, int nbin, int nsub, int nchunk, int off, int t0, int nglob,
                                                    double *out) {
  for (int o = threadIdx.x; o < nbin * nsub; o += 256) {
    const int b = o / nsub, s = o - b * nsub;
    double acc = 0.0;
    for (int k = 0; k < nchunk; k++) acc += partials[((size_t)b * nchunk + k) * nsub + s];
    int dst = (b + off - t0) % nglob;
    if (dst < 0) dst += nglob;
    out[(size_t)dst * nsub + s] = acc;
  }
}

// r of parity p from x of parity 1-p, both parities in one launch; mu < 3, so no hop leaves the slab
template <int RECON>
__global__ void __launch_bounds__(256) k_sym_shift(Geom g, const double2 *W, const unsigned long long *S, int ndir, int mu,
                                                   const double2 *x0, const double2 *x1, double2 *r0, double2 *r1) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * g.Vh) return;
  int p, c; linear_site(g, i, p, c);
  const SiteXYZT s = site_coord(g, c, p);
  constexpr int LROW = LinkFormat<RECON>::LROW;   // double2 per (tile, direction)
  const size_t row = ((size_t)p * g.ntile + (c >> 6)) * ndir + 2 * mu;  // (parity, tile, dir 2mu)
  const int lane = c & 63;
  const double2 *in = p ? x0 : x1;
  const int pf = nbr_pos<false>(g, c, s, mu, 1), pb = nbr_pos<false>(g, c, s, mu, -1);
  double2 U[9], v[3], acc[3];
#pragma unroll
  for (int k = 0; k < 3; k++) acc[k] = make_double2(0.0, 0.0);
  load_link<RECON>(U, W + row * LROW + lane, S ? S + row : nullptr, lane);            // U_mu(x)
#pragma unroll
  for (int k = 0; k < 3; k++) v[k] = in[vec_off(pf, k)];
  mv3<false>(acc, U, v);
  load_link<RECON>(U, W + (row + 1) * LROW + lane, S ? S + row + 1 : nullptr, lane);  // U_mu(x-mu)^+
#pragma unroll
  for (int k = 0; k < 3; k++) v[k] = in[vec_off(pb, k)];
  mv3<false>(acc, U, v);
  double2 *out = p ? r1 : r0;
#pragma unroll
  for (int k = 0; k < 3; k++) out[vec_off(c, k)] = acc[k];
}

// grid: L[dir] x nchunk workgroups; workgroup (v, chunk) sums |f|^2 over sites 256*chunk.. of the V/L sites with x_dir = v,
// enumerated with the other three coordinates in their own order (lowest direction fastest)
__global__ void __launch_bounds__(256) k_norm2slice(Geom g, const double2 *f0, const double2 *f1, int dir, int nchunk, double *partials) {
  const int v = blockIdx.x / nchunk, chunk = blockIdx.x - v * nchunk;
  const int m = g.V / g.X[dir];
  const int j = chunk * 256 + threadIdx.x;
  double a = 0.0;
  if (j < m) {
    int x[4], r = j;
    for (int d = 0; d < 4; d++) {
      if (d == dir) { x[d] = v; continue; }
      x[d] = r % g.X[d];
      r /= g.X[d];
    }
    const int lex = x[0] + g.X[0] * (x[1] + g.X[1] * (x[2] + g.X[2] * x[3]));
    const int c = lex >> 1;
    const double2 *f = ((x[0] + x[1] + x[2] + x[3]) & 1) ? f1 : f0;
#pragma unroll
    for (int col = 0; col < 3; col++) {
      const double2 e = f[vec_off(c, col)];
      a = fma(e.x, e.x, fma(e.y, e.y, a));
    }
  }
  const double r = block_sum_256(a);
  if (threadIdx.x == 0) partials[blockIdx.x] = r;
}

}  // namespace

// scratch of the table reductions (here and in trace.hip): [partials | global table]
int meson_scratch(qexhip_ctx *c, size_t npart, size_t nout, double **part, double **out) {
  const size_t need = npart + nout;
  if (c->meson_cap < need) {
    if (c->meson_buf) HIPCHK(hipFree(c->meson_buf));
    c->meson_buf = nullptr;
    c->meson_cap = 0;
    HIPCHK(hipMalloc((void **)&c->meson_buf, need * sizeof(double)));
    c->meson_cap = need;
  }
  *part = c->meson_buf;
  *out = c->meson_buf + npart;
  return 0;
}

int meson_read_table(qexhip_ctx *c, const double *dev, size_t n, double *host) {
  HIPCHK(hipMemcpyAsync(host, dev, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return peer_check(c);
}

int meson_bins_final(qexhip_ctx *c, const double *partials, int nbin, int nsub, int nchunk, int off, int t0, int nglob, double *out) {
  k_bins_final<<<1, 256, 0, c->stream>>>(partials, nbin, nsub, nchunk, off, t0, nglob, out);
  HIPCHK(hipGetLastError());
  return 0;
}

int meson_corners(qexhip_ctx *c, int n, DevField *const *x, DevField *const *y, int t0, double *host_out) {
  const Geom &g = c->g;
  const int ntg = g.X[3] * c->rankGeom[3], toff = g.X[3] * c->rankCoord[3];
  const int nchunk = (g.F + 255) / 256, nblk = g.X[3] * nchunk;
  double *part, *out;
  CHK(meson_scratch(c, (size_t)nblk * 8, (size_t)ntg * 8, &part, &out));
  MesonPairs P{};
  for (int p = 0; p < 2; p++)
    for (int k = 0; k < n; k++) { P.x[p][k] = x[k]->par(p); P.y[p][k] = y[k]->par(p); }
  HIPCHK(hipMemsetAsync(out, 0, (size_t)ntg * 8 * sizeof(double), c->stream));
  {
    ScopedTimer tm(c, "meson", c->stream);
    k_meson_corners<<<nblk, 256, 0, c->stream>>>(g, P, n, nchunk, part);
    k_bins_final<<<1, 256, 0, c->stream>>>(part, g.X[3], 8, nchunk, toff, t0, ntg, out);
    HIPCHK(hipGetLastError());
  }
  if (multi_rank(c)) CHK(comm_allreduce(c, out, ntg * 8));
  return meson_read_table(c, out, (size_t)ntg * 8, host_out);
}

int norm2slice(qexhip_ctx *c, const DevField &f, int dir, double *host_out) {
  const Geom &g = c->g;
  const int L = g.X[dir], m = g.V / L;
  const int lg = dir == 3 ? L * c->rankGeom[3] : L, off = dir == 3 ? L * c->rankCoord[3] : 0;
  const int nchunk = (m + 255) / 256, nblk = L * nchunk;
  double *part, *out;
  CHK(meson_scratch(c, (size_t)nblk, (size_t)lg, &part, &out));
  HIPCHK(hipMemsetAsync(out, 0, (size_t)lg * sizeof(double), c->stream));
  {
    ScopedTimer tm(c, "meson", c->stream);
    k_norm2slice<<<nblk, 256, 0, c->stream>>>(g, f.par(0), f.par(1), dir, nchunk, part);
    k_bins_final<<<1, 256, 0, c->stream>>>(part, L, 1, nchunk, off, 0, lg, out);
    HIPCHK(hipGetLastError());
  }
  if (multi_rank(c)) CHK(comm_allreduce(c, out, lg));
  return meson_read_table(c, out, (size_t)lg, host_out);
}

int sym_shift(qexhip_ctx *c, DevField &r, const DevField &x, int mu) {
  const Geom &g = c->g;
  const int nblk = (2 * g.Vh + 255) / 256;
  ScopedTimer tm(c, "symshift", c->stream);
  if (c->recon == 1)
    k_sym_shift<1><<<nblk, 256, 0, c->stream>>>(g, c->Wc, c->Ws, c->ndir, mu, x.par(0), x.par(1), r.par(0), r.par(1));
  else if (c->recon == 2)
    k_sym_shift<2><<<nblk, 256, 0, c->stream>>>(g, c->Wc, nullptr, c->ndir, mu, x.par(0), x.par(1), r.par(0), r.par(1));
  else
    k_sym_shift<0><<<nblk, 256, 0, c->stream>>>(g, c->W, nullptr, c->ndir, mu, x.par(0), x.par(1), r.par(0), r.par(1));
  HIPCHK(hipGetLastError());
  return 0;
}
