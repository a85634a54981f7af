// batch_half.hip -- the 16-bit storage of the reduced-precision lock-step batched CG (option "half_batch" = 1, sloppy = 2 on the batched
// entries): its iteration and stall-guard kernels, and the instantiations of the one driver and probe for StoreHalf.  The rule: batch_lowp.h.
#include "qexhip_internal.h"
#include "site_index.h"
#include "reduce.h"
#include "cg_device.h"
#include "batch_lowp.h"
#include <cstring>

// ---- k_slph_xpay / k_slph_update (dslash_half.hip) for n systems: system = blockIdx.y, each with the single-system grid (grid_sites)
// in x, so the |r_s|^2 partials group as they do alone ----
struct SlphBatch {
  const double2 *r[QX_MAXRHS];                   // fp64 true residual
  u4v *rs[QX_MAXRHS], *ps[QX_MAXRHS];
  const u4v *aps[QX_MAXRHS];
  float2 *xs[QX_MAXRHS];                         // the increment, fp32
  const double *dotp[QX_MAXRHS];
  double *r2p[QX_MAXRHS];
  const SlpScal *s;
};

__global__ void __launch_bounds__(256) k_slphb_xpay(SlphBatch B, size_t nsites) {
  const int j = blockIdx.y;
  const SlpScal *s = &B.s[j];
  if (s->done) return;
  const bool conv = s->conv, first = s->first;
  const double inv = 1.0 / s->sigma;
  const float beta = (float)((s->r2s * s->sigma) / (s->r2s_old * s->sigma_p));
  u4v *p = B.ps[j], *rs = B.rs[j];
  const double2 *r = B.r[j];
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nsites; i += (size_t)gridDim.x * 256) {
    float2 rv[3];
    u4v rh;
    if (conv) {
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const double2 d = r[vec_off((int)i, k)];
        rv[k] = make_float2((float)(inv * d.x), (float)(inv * d.y));
      }
      rh = pack_site(rv);
      rs[i] = rh;
    } else {
      rh = rs[i];
      unpack_site(rh, rv, HQ_INV);
    }
    if (first) {
      p[i] = rh;
    } else {
      float2 pv[3];
      unpack_site(p[i], pv, HQ_INV);
#pragma unroll
      for (int k = 0; k < 3; k++) pv[k] = make_float2(fmaf(beta, pv[k].x, rv[k].x), fmaf(beta, pv[k].y, rv[k].y));
      p[i] = pack_site(pv);
    }
  }
}

__global__ void __launch_bounds__(256) k_slphb_update(SlphBatch B, size_t nsites, int ndot) {
  const int j = blockIdx.y;
  const SlpScal *s = &B.s[j];
  if (s->done) return;
  const double pAp = cg_sum_parts(B.dotp[j], ndot);
  const float alpha = (float)(s->r2s / pAp);
  float2 *xs = B.xs[j];
  u4v *rs = B.rs[j];
  const u4v *p = B.ps[j], *Ap = B.aps[j];
  double acc = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nsites; i += (size_t)gridDim.x * 256) {
    float2 pv[3], av[3], rv[3];
    unpack_site(p[i], pv, HQ_INV);
    unpack_site(Ap[i], av, HQ_INV);
    unpack_site(rs[i], rv, HQ_INV);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const size_t o = vec_off((int)i, k);
      float2 xv = xs[o];
      xv.x = fmaf(alpha, pv[k].x, xv.x); xv.y = fmaf(alpha, pv[k].y, xv.y);
      xs[o] = xv;
      rv[k].x = fmaf(-alpha, av[k].x, rv[k].x); rv[k].y = fmaf(-alpha, av[k].y, rv[k].y);
    }
    rs[i] = pack_site(rv);
#pragma unroll
    for (int k = 0; k < 3; k++) acc = fma((double)rv[k].x, (double)rv[k].x, fma((double)rv[k].y, (double)rv[k].y, acc));
  }
  const double t = block_sum_256(acc);
  if (threadIdx.x == 0) B.r2p[j][blockIdx.x] = t;
}

// k_slph_stall_init / k_slph_stall per system: one lane per system
__global__ void k_slphb_stall_init(HalfStall *h, const SlpScal *s, int n) {
  const int j = threadIdx.x;
  if (j >= n) return;
  h[j].best = s[j].r2t; h[j].seen = 0; h[j].nfail = 0; h[j].stalled = 0; h[j].pad = 0;
}
__global__ void k_slphb_stall(HalfStall *hh, SlpScal *ss, int n, int limit) {
  const int j = threadIdx.x;
  if (j >= n) return;
  HalfStall *h = &hh[j];
  SlpScal *s = &ss[j];
  if (s->nupd == h->seen) return;
  h->seen = s->nupd;
  if (s->done) return;
  if (s->r2t < h->best) { h->best = s->r2t; h->nfail = 0; }
  else h->nfail += 1;
  if (h->nfail >= limit) { h->stalled = 1; s->done = 1; }
}

// ---- host: batch_lowp.h on 16-bit storage ---------------------------------------------------------------------------
template <>
struct BatchStore<StoreHalf> {
  static constexpr bool STALL = true;
  static constexpr const char *PROBE = "dev_op_xx_half_batch", *PROBE_SHARDED = "the 16-bit operator runs on one rank without ghost zones";
  static void *&slot(qexhip_ctx *c) { return c->batch_half; }
  static int links(qexhip_ctx *c, int *) { return half_links(c, nullptr, nullptr, nullptr, nullptr); }
  static int ensure(qexhip_ctx *c, DevFieldH &F) { return half_field_ensure(c, F); }
  static size_t extent(const qexhip_ctx *c) { return nsite_h(c); }                     // sites per parity
  static int grid(const qexhip_ctx *c) { return grid_sites(nsite_h(c)); }              // the k_slph_* grid
  using Iter = SlphBatch;
  static void iter_args(SlphBatch &H, const SlpBatch &L, int j, u4v *rs, u4v *ps, const u4v *aps) {
    H.r[j] = L.r[j]; H.rs[j] = rs; H.ps[j] = ps; H.aps[j] = aps; H.xs[j] = L.xs[j];
    H.dotp[j] = L.dotp[j]; H.r2p[j] = L.r2p[j];
    H.s = L.s;
  }
  static void xpay(qexhip_ctx *c, const SlphBatch &H, const SlpBatch &, int n) {
    k_slphb_xpay<<<dim3(grid(c), n), 256, 0, c->stream>>>(H, extent(c));
  }
  static void update(qexhip_ctx *c, const SlphBatch &H, const SlpBatch &, int n, int ndot) {
    k_slphb_update<<<dim3(grid(c), n), 256, 0, c->stream>>>(H, extent(c), ndot);
  }
  static int stall_init(qexhip_ctx *c, HalfStall *h, const SlpScal *s, int n) {
    k_slphb_stall_init<<<1, 64, 0, c->stream>>>(h, s, n);
    HIPCHK(hipGetLastError());
    return 0;
  }
  static int stall(qexhip_ctx *c, HalfStall *h, SlpScal *s, int n, int limit) {
    k_slphb_stall<<<1, 64, 0, c->stream>>>(h, s, n, limit);
    HIPCHK(hipGetLastError());
    return 0;
  }
  static int from_f64(qexhip_ctx *c, DevFieldH &y, const DevField &x, int px) { return half_from_f64(c, y.par(px), x.par(px)); }
  static int to_f64(qexhip_ctx *c, DevField &y, const DevFieldH &x, int px) { return half_to_f64(c, y.par(px), x.par(px)); }
};

void batch_half_state_free(qexhip_ctx *c) { batch_lowp_free<StoreHalf>(c); }
int solve_xx_batch_half_dev(qexhip_ctx *c, int n, DevField **x, DevField **b, const double *mass, const double *r2req,
                            int maxits, int par_even, int *iters, double *r2_over_b2, int *nupdates) {
  return solve_xx_batch_lowp<StoreHalf>(c, n, x, b, mass, r2req, maxits, par_even, iters, r2_over_b2, nupdates);
}
int half_op_xx_batch_probe(qexhip_ctx *c, int n, DevField **fr, DevField **fx, const double *m2, int par_even) {
  return op_xx_batch_probe<StoreHalf>(c, n, fr, fx, m2, par_even);
}

void slpb_last_reset(qexhip_ctx *c, int n) {
  auto &l = c->slpb_last;
  l.n = std::max(0, std::min(n, QX_MAXRHS));
  for (int j = 0; j < QX_MAXRHS; j++) { l.precision[j] = 0; l.half_iters[j] = 0; l.f32_iters[j] = 0; l.fell_back[j] = 0; l.map[j] = j; }
}

int solve_xx_batch_sloppy_any(qexhip_ctx *c, int sloppy, int n, DevField **x, DevField **b, const double *mass, const double *r2req,
                              int maxits, int par_even, int *iters, double *r2_over_b2, int *nupdates) {
  if (sloppy == 2 && c->opt_half_batch && ((c->nranks == 1 && !c->g.halo) || c->opt_batch_ranks))
    return solve_xx_batch_half_dev(c, n, x, b, mass, r2req, maxits, par_even, iters, r2_over_b2, nupdates);
  int its[QX_MAXRHS] = {0, 0, 0, 0};
  CHK(solve_xx_batch_sloppy_dev(c, n, x, b, mass, r2req, maxits, par_even, its, r2_over_b2, nupdates));
  for (int j = 0; j < n; j++) {
    const int q = c->slpb_last.map[j];
    if (c->slpb_last.precision[q] == 0) c->slpb_last.precision[q] = 1;
    c->slpb_last.f32_iters[q] += its[j];
    if (iters) iters[j] = its[j];
  }
  return 0;
}
