// batch_f32.hip -- the mixed-precision form of the lock-step batched CG (batch.hip): up to four reliable-update solveXX's on the
// SAME links, their fp32 iterations advanced together so that the fp32 link copy (dslash_f32.hip) is streamed ONCE per sweep for
// all of them.  Where QEX's measurement code asks for it: src/observables/conn4d.nim:52 and scalarTrace.nim:42 default to a sloppy
// solve, which src/quda/qudaWrapperImpl.nim:194-197 hands on as mixed precision.
//
// The rule is batch.hip's: every system keeps its own state (SlpScal: sigma, alpha, beta, max|r_s|^2, upd / noupd / done, k, nupd) and
// its arithmetic is, operation for operation, that of the single-system solve_xx_sloppy_dev (solver.cpp) -- the sweep is
// k_dslash_mrhs_lowp<StoreF32, ..> (dslash_lowp.h: the single-system body per system), the BLAS kernels are k_slp_* with the system
// in blockIdx.y and the single-system grid per system, and the reliable update runs the fp64 op_xx per system behind that system's `noupd` word.  A
// system solved in a batch returns the bits -- solution, iterations, true residual, updates -- it returns alone.
//
// One rank without ghost zones by default: t-sharded contexts are refused unless option "batch_ranks" is 1.  With it the sweep takes its
// HALO form (dslash_lowp.h: sweep_mrhs, all systems' faces in one exchange), every set of partials is summed over the ranks for all
// systems in ONE collective per reduction point (comm_allreduce_parts_multi: each system's sum formed as comm_allreduce_parts forms it
// alone) and the n states read back at the end of a chunk are checked for agreement per system (slp_agree) before any rank acts on
// them.  "Alone" is then the single-system solve_xx_sloppy_dev on the same sharded context, sweep form and transport.  The INVARIANT
// above slp_update holds per system: rank-global sums, hence the same flags on every rank; the host posts the same exchanges and
// collectives on every rank whatever the flags say.
#include "qexhip_internal.h"
#include "site_index.h"
#include "reduce.h"
#include "cg_device.h"
#include "dslash_lowp.h"
#include <algorithm>
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

// ---- host ----------------------------------------------------------------------------------------------------------
enum { BF_R = 0, BF_P, BF_AP, BF_X, BF_T, BF_N };   // fp32 work fields per system

struct BatchF32State {
  DevFieldF f[BF_N * QX_MAXRHS];
  SlpScal *s = nullptr;
  double *partials = nullptr;
  size_t npart = 0;
};

void batch_f32_state_free(qexhip_ctx *c) {
  BatchF32State *S = (BatchF32State *)c->batch_f32;
  if (!S) return;
  for (auto &f : S->f) if (f.d) (void)hipFree(f.d);
  if (S->s) (void)hipFree(S->s);
  if (S->partials) (void)hipFree(S->partials);
  delete S;
  c->batch_f32 = nullptr;
}

// all systems' <p,Ap> partials, nbd apart, then all systems' |r_s|^2 / |b - A x|^2 partials, nbb apart: one contiguous range per reduction point
static int bf_partials(BatchF32State *S, int nbd, int nbb) {
  const size_t need = ((size_t)nbd + nbb) * QX_MAXRHS;
  if (S->npart < need) {
    if (S->partials) HIPCHK(hipFree(S->partials));
    S->partials = nullptr; S->npart = 0;
    HIPCHK(hipMalloc((void **)&S->partials, need * sizeof(double)));
    S->npart = need;
  }
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

// n (1..4) mixed-precision solveXX's in lock-step: solve_xx_batch_dev's semantics (own mass, r2req, iteration count; shared maxits),
// solve_xx_sloppy_dev's iteration per system.  iters: fp32 iterations; r2_over_b2: the TRUE residual; nupdates: reliable updates.
int solve_xx_batch_sloppy_dev(qexhip_ctx *c, int n, DevField **x, DevField **b, const double *mass, const double *r2req,
                              int maxits, int par_even, int *iters, double *r2_over_b2, int *nupdates) {
  const Geom &g = c->g;
  CHK(batch_sloppy_check(c, n, mass));
  int fmt = 0;
  CHK(f32_links(c, &fmt, nullptr));
  BatchF32State *S = (BatchF32State *)c->batch_f32;
  if (!S) { S = new BatchF32State(); c->batch_f32 = S; }
  if (!S->s) HIPCHK(hipMalloc((void **)&S->s, sizeof(SlpScal) * QX_MAXRHS));
  const size_t nvec = (size_t)g.ntile * 192;
  const int nbd = (g.Vh + 255) / 256 + 4;                                      // room for a sweep's <p,Ap> partials (a split sweep rounds up per range)
  const int nbb = (int)std::max<size_t>(1, std::min<size_t>((nvec + 255) / 256, 2048));   // the k_slp_* grid (grid_for)
  CHK(bf_partials(S, nbd, nbb));
  DevField *w64[2 * QX_MAXRHS];
  CHK(batch_work_fields(c, 2 * QX_MAXRHS, w64));                             // r, A x per system
  const int par = par_even ? 0 : 1;
  MrhsArgs<StoreF32> A1, A2;
  SlpBatch L;
  memset(&A1, 0, sizeof A1); memset(&A2, 0, sizeof A2); memset(&L, 0, sizeof L);
  double m2[QX_MAXRHS];
  DevField *rj[QX_MAXRHS], *axj[QX_MAXRHS];
  for (int j = 0; j < n; j++) {
    DevFieldF *const fj = &S->f[BF_N * j];
    for (int k = 0; k < BF_N; k++) CHK(f32_field_ensure(c, fj[k]));
    DevFieldF *rs = &fj[BF_R], *ps = &fj[BF_P], *aps = &fj[BF_AP], *xs = &fj[BF_X], *t = &fj[BF_T];
    rj[j] = w64[2 * j]; axj[j] = w64[2 * j + 1];
    m2[j] = mass[j] * mass[j];
    // exactly the start of solve_xx_sloppy_dev: x = 0, b2, r = b, x_s = 0, k_slp_init
    CHK(blas_zero(c, *x[j], 2));
    CHK(blas_norm2(c, *b[j], par, &c->dscal[0]));
    CHK(blas_copy(c, *rj[j], *b[j], par));
    HIPCHK(hipMemsetAsync(xs->par(par), 0, xs->half * sizeof(float2), c->stream));
    CHK(slp_init(c, &S->s[j], r2req[j], maxits));
    A1.in[j] = ps->par(par); A1.out[j] = t->par(1 - par);
    A2.in[j] = t->par(1 - par); A2.out[j] = aps->par(par); A2.xs[j] = ps->par(par);
    A2.cb[j] = (float)(4.0 * m2[j]);
    A2.partials[j] = S->partials + (size_t)nbd * j;
    L.x[j] = x[j]->par(par); L.r[j] = rj[j]->par(par); L.b[j] = b[j]->par(par); L.Ax[j] = axj[j]->par(par);
    L.rs[j] = rs->par(par); L.ps[j] = ps->par(par); L.xs[j] = xs->par(par); L.aps[j] = aps->par(par);
    L.dotp[j] = S->partials + (size_t)nbd * j; L.r2p[j] = S->partials + (size_t)nbd * QX_MAXRHS + (size_t)nbb * j;
  }
  L.s = S->s;
  CHK(mrhs_links(c, n, par, S->s, A1, A2, &fmt));
  SlpScal h[QX_MAXRHS];
  auto read_states = [&]() -> int {
    HIPCHK(hipMemcpyAsync(c->pinned, S->s, sizeof(SlpScal) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    memcpy(h, c->pinned, sizeof(SlpScal) * n);
    return 0;
  };
  // sharded: every rank holds the same n states before any of them acts on its copy (comm_allreduce_max takes four values: one call per system)
  auto agree = [&]() -> int { for (int j = 0; j < n; j++) CHK(slp_agree(c, h[j])); return 0; };
  auto all_done = [&]() { for (int j = 0; j < n; j++) if (!h[j].done) return false; return true; };
  CHK(read_states());
  const int every = std::max(1, c->opt_sloppy_check);
  int k = 0;
  while (!all_done() && k < maxits) {
    const int chunk = std::min(32, maxits - k);
    for (int i = 0; i < chunk; i++, k++) {
      {
        ScopedTimer tm(c, "blas", c->stream);
        k_slpb_xpay<<<dim3(nbb, n), 256, 0, c->stream>>>(L, nvec);
      }
      int ndot = 0;
      CHK(sweep_mrhs(c, A1, fmt, false));
      CHK(sweep_mrhs(c, A2, fmt, true, &ndot));
      CHK(comm_allreduce_parts_multi(c, n, L.dotp[0], nbd, ndot, L.s, 1, &ndot));
      CHK(devjoin_flush(c));            // (no-op when the all-reduce has taken the second sweep's join with it)
      {
        ScopedTimer tm(c, "blas", c->stream);
        k_slpb_update<<<dim3(nbb, n), 256, 0, c->stream>>>(L, nvec, ndot);
      }
      HIPCHK(hipGetLastError());
      CHK(slpb_close(c, L, n, nbb, nbb));
      // the (device-gated) reliable update of every system whose `upd` is up, posted as solve_xx_sloppy_dev posts its own; a system
      // that is done counts no further, so the host's k is each live system's own k
      if ((k + 1) % every == 0 || k + 1 >= maxits) {
        k_slpb_flush<<<dim3(nbb, n), 256, 0, c->stream>>>(L, nvec);
        HIPCHK(hipGetLastError());
        for (int j = 0; j < n; j++) CHK(op_xx(c, *axj[j], *x[j], m2[j], par_even, 0, &S->s[j].noupd));
        CHK(slpb_resid(c, L, n, nvec, nbb, nbb));
      }
    }
    CHK(read_states());
    CHK(agree());
  }
  for (int j = 0; j < n; j++) {
    if (iters) iters[j] = h[j].k;
    if (r2_over_b2) r2_over_b2[j] = (h[j].b2 != 0.0) ? h[j].r2t / h[j].b2 : 0.0;
    if (nupdates) nupdates[j] = h[j].nupd;
  }
  return 0;
}

// fr_j[px] = the batched fp32 operator at m2_j on fx_j[px] rounded to fp32, back in fp64 (qexhip_dev_op_xx_sloppy_batch): the fp32 twin of
// half_op_xx_batch_probe, on one rank and -- with option "batch_ranks" -- on t-sharded contexts
int f32_op_xx_batch_probe(qexhip_ctx *c, int n, DevField **fr, DevField **fx, const double *m2, int par_even) {
  if (n < 1 || n > QX_MAXRHS) { qexhip_set_error("dev_op_xx_sloppy_batch: 1 <= n <= %d", QX_MAXRHS); return -1; }
  if ((c->nranks > 1 || c->g.halo) && !c->opt_batch_ranks) {
    qexhip_set_error("the batched fp32 operator runs on one rank without ghost zones (t-sharded: option batch_ranks)");
    return -1;
  }
  int fmt = 0;
  CHK(f32_links(c, &fmt, nullptr));
  BatchF32State *S = (BatchF32State *)c->batch_f32;
  if (!S) { S = new BatchF32State(); c->batch_f32 = S; }
  if (!S->s) HIPCHK(hipMalloc((void **)&S->s, sizeof(SlpScal) * QX_MAXRHS));
  const int nbd = (c->g.Vh + 255) / 256 + 4;
  const size_t nvec = (size_t)c->g.ntile * 192;
  CHK(bf_partials(S, nbd, (int)std::max<size_t>(1, std::min<size_t>((nvec + 255) / 256, 2048))));
  HIPCHK(hipMemsetAsync(S->s, 0, sizeof(SlpScal) * QX_MAXRHS, c->stream));       // every system live
  const int px = par_even ? 0 : 1;
  MrhsArgs<StoreF32> A1, A2;
  memset(&A1, 0, sizeof A1); memset(&A2, 0, sizeof A2);
  for (int j = 0; j < n; j++) {
    DevFieldF *const fj = &S->f[BF_N * j];
    for (int k = 0; k < BF_N; k++) CHK(f32_field_ensure(c, fj[k]));
    CHK(f32_from_f64(c, fj[BF_P], *fx[j], px, 1.0));
    A1.in[j] = fj[BF_P].par(px); A1.out[j] = fj[BF_T].par(1 - px);
    A2.in[j] = fj[BF_T].par(1 - px); A2.out[j] = fj[BF_AP].par(px); A2.xs[j] = fj[BF_P].par(px);
    A2.cb[j] = (float)(4.0 * m2[j]);
    A2.partials[j] = S->partials + (size_t)nbd * j;
  }
  CHK(mrhs_links(c, n, px, S->s, A1, A2, &fmt));
  CHK(sweep_mrhs(c, A1, fmt, false));
  CHK(sweep_mrhs(c, A2, fmt, true));
  CHK(devjoin_flush(c));
  for (int j = 0; j < n; j++) CHK(f32_to_f64(c, *fr[j], S->f[BF_N * j + BF_AP], px, 1.0, 0));
  return 0;
}
