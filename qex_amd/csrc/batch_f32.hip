// batch_f32.hip -- the fp32 storage of the reduced-precision lock-step batched CG: the reliable-update CG's BLAS and bookkeeping kernels for
// n systems, and the instantiations of the one driver and probe for StoreF32.  The rule, the loop and the sharded form: batch_lowp.h.
#include "qexhip_internal.h"
#include "site_index.h"
#include "reduce.h"
#include "cg_device.h"
#include "batch_lowp.h"
#include <cstring>

// ---- the reliable-update CG's BLAS and bookkeeping kernels (dslash_f32.hip: k_slp_*) for n systems: system = blockIdx.y, each with
// the single-system kernel's grid in x, so the workgroup partials group as they do there ----

__global__ void __launch_bounds__(256) k_slpb_xpay(SlpBatch B, size_t n) {
  const int j = blockIdx.y;
  const SlpScal *s = &B.s[j];
  if (s->done) return;
  const bool conv = s->conv, first = s->first;
  const double inv = 1.0 / s->sigma;
  const float beta = (float)((s->r2s * s->sigma) / (s->r2s_old * s->sigma_p));
  float2 *p = B.ps[j], *rs = B.rs[j];
  const double2 *r = B.r[j];
  for (size_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    float2 rv;
    if (conv) {
      const double2 v = r[i];
      rv = make_float2((float)(inv * v.x), (float)(inv * v.y));
      rs[i] = rv;
    } else {
      rv = rs[i];
    }
    if (first) p[i] = rv;
    else {
      const float2 pv = p[i];
      p[i] = make_float2(fmaf(beta, pv.x, rv.x), fmaf(beta, pv.y, rv.y));
    }
  }
}

__global__ void __launch_bounds__(256) k_slpb_update(SlpBatch B, size_t n, int ndot) {
  const int j = blockIdx.y;
  const SlpScal *s = &B.s[j];
  if (s->done) return;
  const double pAp = cg_sum_parts(B.dotp[j], ndot);
  const float alpha = (float)(s->r2s / pAp);
  float2 *xs = B.xs[j], *rs = B.rs[j];
  const float2 *p = B.ps[j], *Ap = B.aps[j];
  double acc = 0;
  for (size_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float2 pv = p[i], av = Ap[i];
    float2 xv = xs[i], rv = rs[i];
    xv.x = fmaf(alpha, pv.x, xv.x); xv.y = fmaf(alpha, pv.y, xv.y);
    rv.x = fmaf(-alpha, av.x, rv.x); rv.y = fmaf(-alpha, av.y, rv.y);
    xs[i] = xv; rs[i] = rv;
    acc = fma((double)rv.x, (double)rv.x, fma((double)rv.y, (double)rv.y, acc));
  }
  const double t = block_sum_256(acc);
  if (threadIdx.x == 0) B.r2p[j][blockIdx.x] = t;
}

// one workgroup per system
__global__ void __launch_bounds__(256) k_slpb_close(SlpBatch B, int nparts, double delta2) {
  SlpScal *s = &B.s[blockIdx.x];
  if (s->done) return;
  const double r2 = cg_sum_parts(B.r2p[blockIdx.x], nparts);
  if (threadIdx.x == 0) {
    s->k += 1;
    s->r2s_old = s->r2s; s->sigma_p = s->sigma;
    s->r2s = r2;
    s->maxr2s = fmax(s->maxr2s, r2);
    const int due = r2 < delta2 * s->maxr2s || r2 * s->sigma * s->sigma <= s->r2stop || s->k >= s->maxits;
    s->upd = s->upd || due;
    s->noupd = !s->upd;
    s->conv = 0; s->first = 0;
  }
}

__global__ void __launch_bounds__(256) k_slpb_flush(SlpBatch B, size_t n) {
  const int j = blockIdx.y;
  const SlpScal *s = &B.s[j];
  if (!s->upd || s->done) return;
  const double sg = s->sigma;
  double2 *x = B.x[j];
  float2 *xs = B.xs[j];
  for (size_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float2 v = xs[i];
    double2 o = x[i];
    o.x = fma(sg, (double)v.x, o.x); o.y = fma(sg, (double)v.y, o.y);
    x[i] = o;
    xs[i] = make_float2(0.f, 0.f);
  }
}

__global__ void __launch_bounds__(256) k_slpb_resid(SlpBatch B, size_t n) {
  const int j = blockIdx.y;
  const SlpScal *s = &B.s[j];
  if (!s->upd || s->done) return;
  double2 *r = B.r[j];
  const double2 *b = B.b[j], *Ax = B.Ax[j];
  double acc = 0;
  for (size_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const double2 bv = b[i], av = Ax[i];
    const double2 rv = make_double2(bv.x - av.x, bv.y - av.y);
    r[i] = rv;
    acc = fma(rv.x, rv.x, fma(rv.y, rv.y, acc));
  }
  const double t = block_sum_256(acc);
  if (threadIdx.x == 0) B.r2p[j][blockIdx.x] = t;
}

// one workgroup per system
__global__ void __launch_bounds__(256) k_slpb_rclose(SlpBatch B, int nparts) {
  SlpScal *s = &B.s[blockIdx.x];
  if (!s->upd || s->done) return;
  const double r2t = cg_sum_parts(B.r2p[blockIdx.x], nparts);
  if (threadIdx.x == 0) {
    s->r2t = r2t;
    s->nupd += 1;
    s->upd = 0; s->noupd = 1;
    if (!(r2t > s->r2stop) || s->k >= s->maxits) {
      s->done = 1;
    } else {
      const double sg = sqrt(r2t);
      s->r2s = 1.0;
      s->sigma = sg;
      s->maxr2s = 1.0;
      s->conv = 1;
      if (!(s->r2s_old > 0)) s->first = 1;
    }
  }
}

// the bookkeeping launches, shared with another file's iteration kernels (batch_half.hip).  nparts |r_s|^2 partials per system in
// L.r2p[j] = L.r2p[0] + j r2stride: summed over the ranks first (one collective for all systems; one rank: nothing)
int slpb_close(qexhip_ctx *c, const SlpBatch &L, int n, int nparts, size_t r2stride) {
  int nr2 = nparts;
  CHK(comm_allreduce_parts_multi(c, n, L.r2p[0], r2stride, nparts, L.s, 1, &nr2));
  k_slpb_close<<<n, 256, 0, c->stream>>>(L, nr2, SLP_DELTA * SLP_DELTA);
  HIPCHK(hipGetLastError());
  return 0;
}
int slpb_flush(qexhip_ctx *c, const SlpBatch &L, int n, size_t nvec, int nbb) {
  k_slpb_flush<<<dim3(nbb, n), 256, 0, c->stream>>>(L, nvec);
  HIPCHK(hipGetLastError());
  return 0;
}
int slpb_resid(qexhip_ctx *c, const SlpBatch &L, int n, size_t nvec, int nbb, size_t r2stride) {
  k_slpb_resid<<<dim3(nbb, n), 256, 0, c->stream>>>(L, nvec);
  HIPCHK(hipGetLastError());
  int nr2 = nbb;
  CHK(comm_allreduce_parts_multi(c, n, L.r2p[0], r2stride, nbb, L.s, 2, &nr2));     // (posted whether or not an update is due, as slp_resid's)
  k_slpb_rclose<<<n, 256, 0, c->stream>>>(L, nr2);
  HIPCHK(hipGetLastError());
  return 0;
}

// what every batched sloppy entry checks before anything is launched
int batch_sloppy_check(qexhip_ctx *c, int n, const double *mass) {
  if (n < 1 || n > QX_MAXRHS) { qexhip_set_error("batch solve: 1 <= n <= %d", QX_MAXRHS); return -1; }
  if ((c->nranks > 1 || c->g.halo) && !c->opt_batch_ranks) {
    qexhip_set_error("batched sloppy solve: t-sharded contexts (more than one rank, or ghost zones in t) are not supported -- the "
                     "sharded form is not built; use the fp64 batch or single-system sloppy solves there");
    return -1;
  }
  for (int j = 0; j < n; j++)
    if (mass[j] == 0.0) { qexhip_set_error("batched sloppy solve: mass 0 unsupported (op_xx's <p,Ap> needs 4 m^2 > 0)"); return -1; }
  return 0;
}

// ---- host: batch_lowp.h on fp32 storage -----------------------------------------------------------------------------
template <>
struct BatchStore<StoreF32> {
  static constexpr bool STALL = false;
  static constexpr const char *PROBE = "dev_op_xx_sloppy_batch",
                              *PROBE_SHARDED = "the batched fp32 operator runs on one rank without ghost zones (t-sharded: option batch_ranks)";
  static void *&slot(qexhip_ctx *c) { return c->batch_f32; }
  static int links(qexhip_ctx *c, int *fmt) { return f32_links(c, fmt, nullptr); }
  static int ensure(qexhip_ctx *c, DevFieldF &F) { return f32_field_ensure(c, F); }
  static size_t extent(const qexhip_ctx *c) { return (size_t)c->g.ntile * 192; }      // float2 per parity
  static int grid(const qexhip_ctx *c) { return slp_grid(extent(c)); }
  struct Iter {};                                    // the iteration kernels take the bookkeeping's SlpBatch
  static void iter_args(Iter &, SlpBatch &L, int j, float2 *rs, float2 *ps, const float2 *aps) { L.rs[j] = rs; L.ps[j] = ps; L.aps[j] = aps; }
  static void xpay(qexhip_ctx *c, const Iter &, const SlpBatch &L, int n) {
    k_slpb_xpay<<<dim3(grid(c), n), 256, 0, c->stream>>>(L, extent(c));
  }
  static void update(qexhip_ctx *c, const Iter &, const SlpBatch &L, int n, int ndot) {
    k_slpb_update<<<dim3(grid(c), n), 256, 0, c->stream>>>(L, extent(c), ndot);
  }
  static int from_f64(qexhip_ctx *c, DevFieldF &y, const DevField &x, int px) { return f32_from_f64(c, y, x, px, 1.0); }
  static int to_f64(qexhip_ctx *c, DevField &y, const DevFieldF &x, int px) { return f32_to_f64(c, y, x, px, 1.0, 0); }
};

void batch_f32_state_free(qexhip_ctx *c) { batch_lowp_free<StoreF32>(c); }
// reports nothing to c->slpb_last itself: its callers do (solve_xx_batch_sloppy_any)
int solve_xx_batch_sloppy_dev(qexhip_ctx *c, int n, DevField **x, DevField **b, const double *mass, const double *r2req,
                              int maxits, int par_even, int *iters, double *r2_over_b2, int *nupdates) {
  return solve_xx_batch_lowp<StoreF32>(c, n, x, b, mass, r2req, maxits, par_even, iters, r2_over_b2, nupdates);
}
int f32_op_xx_batch_probe(qexhip_ctx *c, int n, DevField **fr, DevField **fx, const double *m2, int par_even) {
  return op_xx_batch_probe<StoreF32>(c, n, fr, fx, m2, par_even);
}
