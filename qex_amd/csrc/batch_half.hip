// batch_half.hip -- the 16-bit form of the lock-step batched CG (option "half_batch" = 1, sloppy = 2 on the batched entries): up to four
// reliable-update solveXX's on the SAME links, their 16-bit iterations advanced together so that the int16 link copy (dslash_half.hip)
// is streamed ONCE per sweep for all of them.  QEX's measurement programs ask for SloppyHalf by default (scalarTrace.nim:42,
// conn4d.nim:52) and its GPU backend makes that 16-bit storage (qudaWrapperImpl.nim:197).
//
// The rule is batch_f32.hip's: every system keeps its own state (SlpScal, HalfStall) and its arithmetic is, operation for operation,
// that of the single-system solve_xx_half_dev -- the sweep is k_dslash_mrhs_lowp<StoreHalf, ..> (dslash_lowp.h: the single-system
// body per system), the BLAS kernels are k_slph_* with the system in blockIdx.y on the single-system grid, the bookkeeping and the
// reliable update are the fp32 batch's (k_slpb_*, the gated fp64 op_xx per system), and the stall guard runs per system.  A system solved here returns the bits --
// solution, iterations, true residual, updates, fall-back -- it returns from solve_xx_half_dev alone.
//
// One rank without ghost zones by default; with option "batch_ranks" on t-sharded contexts too, as batch_f32.hip describes: the HALO
// sweep with all systems' 16-bit faces in one exchange, one collective per reduction point for all systems, and the n states with each
// system's stall flag checked for agreement (slp_agree) at the end of every chunk.  The decision to enter half_finish_f32 -- itself
// sharded, it posts collectives -- is taken for every system from that agreed state alone, on all ranks or on none.
#include "qexhip_internal.h"
#include "site_index.h"
#include "reduce.h"
#include "cg_device.h"
#include "dslash_lowp.h"
#include <algorithm>
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

// ---- host ----------------------------------------------------------------------------------------------------------
enum { BH_R = 0, BH_P, BH_AP, BH_T, BH_N };   // 16-bit work fields per system

struct BatchHalfState {
  DevFieldH f[BH_N * QX_MAXRHS];
  DevFieldF xs[QX_MAXRHS];                    // the increments x_s, fp32
  SlpScal *s = nullptr;
  HalfStall *stall = nullptr;
  double *partials = nullptr;
  size_t npart = 0;
};

void batch_half_state_free(qexhip_ctx *c) {
  BatchHalfState *S = (BatchHalfState *)c->batch_half;
  if (!S) return;
  for (auto &f : S->f) if (f.d) (void)hipFree(f.d);
  for (auto &f : S->xs) if (f.d) (void)hipFree(f.d);
  if (S->s) (void)hipFree(S->s);
  if (S->stall) (void)hipFree(S->stall);
  if (S->partials) (void)hipFree(S->partials);
  delete S;
  c->batch_half = nullptr;
}

static int bh_state(qexhip_ctx *c, int n, size_t per, BatchHalfState **out) {
  BatchHalfState *S = (BatchHalfState *)c->batch_half;
  if (!S) { S = new BatchHalfState(); c->batch_half = S; }
  if (!S->s) HIPCHK(hipMalloc((void **)&S->s, sizeof(SlpScal) * QX_MAXRHS));
  if (!S->stall) HIPCHK(hipMalloc((void **)&S->stall, sizeof(HalfStall) * QX_MAXRHS));
  if (S->npart < per * QX_MAXRHS) {
    if (S->partials) HIPCHK(hipFree(S->partials));
    S->partials = nullptr; S->npart = 0;
    HIPCHK(hipMalloc((void **)&S->partials, per * QX_MAXRHS * sizeof(double)));
    S->npart = per * QX_MAXRHS;
  }
  for (int j = 0; j < n; j++) {
    for (int k = 0; k < BH_N; k++) CHK(half_field_ensure(c, S->f[BH_N * j + k]));
    CHK(f32_field_ensure(c, S->xs[j]));
  }
  *out = S;
  return 0;
}

// n (1..4) 16-bit solveXX's in lock-step: solve_xx_batch_sloppy_dev's loop (chunks of 32, one read of the n states per chunk, updates
// posted every opt_sloppy_check-th iteration and at maxits; shared maxits), solve_xx_half_dev's start, iteration, stall guard and fp32
// finish per system.  iters: 16-bit + fp32 iterations; r2_over_b2: the TRUE residual; nupdates: reliable updates.
int solve_xx_batch_half_dev(qexhip_ctx *c, int n, DevField **x, DevField **b, const double *mass, const double *r2req,
                            int maxits, int par_even, int *iters, double *r2_over_b2, int *nupdates) {
  const Geom &g = c->g;
  CHK(batch_sloppy_check(c, n, mass));
  CHK(half_links(c, nullptr, nullptr, nullptr, nullptr));
  const size_t nvec = (size_t)g.ntile * 192, nsites = nsite_h(c);
  const int nbd = (g.Vh + 255) / 256 + 4;                                      // room for a sweep's <p,Ap> partials (a split sweep rounds up per range)
  const int nbh = grid_sites(nsites);                                          // the k_slph_* grid
  const int nbb = (int)std::max<size_t>(1, std::min<size_t>((nvec + 255) / 256, 2048));   // the fp64 k_slp_* grid (grid_for)
  const size_t nbr = (size_t)std::max(nbh, nbb);                               // doubles between two systems' r2p
  const size_t per = (size_t)nbd + nbr;                                        // (layout: all dotp, nbd apart, then all r2p, nbr apart)
  BatchHalfState *S;
  CHK(bh_state(c, n, per, &S));
  DevField *w64[2 * QX_MAXRHS];
  CHK(batch_work_fields(c, 2 * QX_MAXRHS, w64));                             // r, A x per system
  const int par = par_even ? 0 : 1;
  MrhsArgs<StoreHalf> A1, A2;
  SlphBatch H;
  SlpBatch L;
  memset(&A1, 0, sizeof A1); memset(&A2, 0, sizeof A2); memset(&H, 0, sizeof H); memset(&L, 0, sizeof L);
  double m2[QX_MAXRHS];
  DevField *rj[QX_MAXRHS], *axj[QX_MAXRHS];
  for (int j = 0; j < n; j++) {
    DevFieldH *const fj = &S->f[BH_N * j];
    DevFieldH *rs = &fj[BH_R], *ps = &fj[BH_P], *aps = &fj[BH_AP], *t = &fj[BH_T];
    DevFieldF *xs = &S->xs[j];
    rj[j] = w64[2 * j]; axj[j] = w64[2 * j + 1];
    m2[j] = mass[j] * mass[j];
    // exactly the start of solve_xx_half_dev: x = 0, b2, r = b, x_s = 0, k_slp_init
    CHK(blas_zero(c, *x[j], 2));
    CHK(blas_norm2(c, *b[j], par, &c->dscal[0]));
    CHK(blas_copy(c, *rj[j], *b[j], par));
    HIPCHK(hipMemsetAsync(xs->par(par), 0, xs->half * sizeof(float2), c->stream));
    CHK(slp_init(c, &S->s[j], r2req[j], maxits));
    A1.in[j] = ps->par(par); A1.out[j] = t->par(1 - par);
    A2.in[j] = t->par(1 - par); A2.out[j] = aps->par(par); A2.xs[j] = ps->par(par);
    A2.cb[j] = (float)(4.0 * m2[j]);
    A2.partials[j] = S->partials + (size_t)nbd * j;
    H.r[j] = rj[j]->par(par); H.rs[j] = rs->par(par); H.ps[j] = ps->par(par); H.aps[j] = aps->par(par); H.xs[j] = xs->par(par);
    H.dotp[j] = S->partials + (size_t)nbd * j; H.r2p[j] = S->partials + (size_t)nbd * QX_MAXRHS + nbr * j;
    L.x[j] = x[j]->par(par); L.r[j] = rj[j]->par(par); L.b[j] = b[j]->par(par); L.Ax[j] = axj[j]->par(par);
    L.xs[j] = xs->par(par);
    L.dotp[j] = S->partials + (size_t)nbd * j; L.r2p[j] = H.r2p[j];
  }
  H.s = S->s; L.s = S->s;
  k_slphb_stall_init<<<1, 64, 0, c->stream>>>(S->stall, S->s, n);
  HIPCHK(hipGetLastError());
  int fmt = 0;
  CHK(mrhs_links(c, n, par, S->s, A1, A2, &fmt));
  SlpScal h[QX_MAXRHS];
  HalfStall hs[QX_MAXRHS];
  static_assert(sizeof(SlpScal) * QX_MAXRHS <= 2048 && sizeof(HalfStall) * QX_MAXRHS <= 2048, "pinned scratch layout");
  HalfStall *const pstall = (HalfStall *)((char *)c->pinned + 2048);     // (behind the SlpScal's)
  auto read_states = [&]() -> int {
    HIPCHK(hipMemcpyAsync(c->pinned, S->s, sizeof(SlpScal) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(pstall, S->stall, sizeof(HalfStall) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    memcpy(h, c->pinned, sizeof(SlpScal) * n);
    memcpy(hs, pstall, sizeof(HalfStall) * n);
    return 0;
  };
  // sharded: every rank holds the same n states and stall flags before any of them acts on its copy (one call per system)
  auto agree = [&]() -> int { for (int j = 0; j < n; j++) CHK(slp_agree(c, h[j], hs[j].stalled)); return 0; };
  auto all_done = [&]() { for (int j = 0; j < n; j++) if (!h[j].done) return false; return true; };
  CHK(read_states());
  const int every = std::max(1, c->opt_sloppy_check);
  int k = 0;
  while (!all_done() && k < maxits) {
    const int chunk = std::min(32, maxits - k);
    for (int i = 0; i < chunk; i++, k++) {
      {
        ScopedTimer tm(c, "blas", c->stream);
        k_slphb_xpay<<<dim3(nbh, n), 256, 0, c->stream>>>(H, nsites);
      }
      int ndot = 0;
      CHK(sweep_mrhs(c, A1, fmt, false));
      CHK(sweep_mrhs(c, A2, fmt, true, &ndot));
      CHK(comm_allreduce_parts_multi(c, n, L.dotp[0], nbd, ndot, L.s, 1, &ndot));
      CHK(devjoin_flush(c));            // (no-op when the all-reduce has taken the second sweep's join with it)
      {
        ScopedTimer tm(c, "blas", c->stream);
        k_slphb_update<<<dim3(nbh, n), 256, 0, c->stream>>>(H, nsites, ndot);
      }
      HIPCHK(hipGetLastError());
      CHK(slpb_close(c, L, n, nbh, nbr));
      // the (device-gated) reliable update of every system whose `upd` is up, and each system's stall guard behind it; a system that is
      // done counts no further, so the host's k is each live system's own k
      if ((k + 1) % every == 0 || k + 1 >= maxits) {
        CHK(slpb_flush(c, L, n, nvec, nbb));
        for (int j = 0; j < n; j++) CHK(op_xx(c, *axj[j], *x[j], m2[j], par_even, 0, &S->s[j].noupd));
        CHK(slpb_resid(c, L, n, nvec, nbb, nbr));
        k_slphb_stall<<<1, 64, 0, c->stream>>>(S->stall, S->s, n, c->opt_half_stall);
        HIPCHK(hipGetLastError());
      }
    }
    CHK(read_states());
    CHK(agree());
  }
  for (int j = 0; j < n; j++) {
    int its = h[j].k, nupd = h[j].nupd, its32 = 0, fell = 0;
    double r2t = h[j].r2t;
    if (hs[j].stalled && r2t > h[j].r2stop && its < maxits) {
      // (x_j holds every increment: the update that tripped the guard flushed x_s; r_j is its true residual)
      int nu32 = 0;
      CHK(half_finish_f32(c, *x[j], *b[j], *rj[j], *axj[j], mass[j], h[j].r2stop, maxits - its, par_even, &r2t, &its32, &nu32));
      nupd += nu32;
      fell = 1;
    }
    const int q = c->slpb_last.map[j];
    c->slpb_last.precision[q] = 2;
    c->slpb_last.half_iters[q] += its;
    c->slpb_last.f32_iters[q] += its32;
    if (fell) c->slpb_last.fell_back[q] = 1;
    if (iters) iters[j] = its + its32;
    if (r2_over_b2) r2_over_b2[j] = (h[j].b2 != 0.0) ? r2t / h[j].b2 : 0.0;
    if (nupdates) nupdates[j] = nupd;
  }
  return 0;
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

// fr_j[px] = the batched 16-bit operator at m2_j on fx_j[px] rounded to 16 bits, back in fp64 (qexhip_dev_op_xx_half_batch)
int half_op_xx_batch_probe(qexhip_ctx *c, int n, DevField **fr, DevField **fx, const double *m2, int par_even) {
  if (n < 1 || n > QX_MAXRHS) { qexhip_set_error("dev_op_xx_half_batch: 1 <= n <= %d", QX_MAXRHS); return -1; }
  if ((c->nranks > 1 || c->g.halo) && !c->opt_batch_ranks) { qexhip_set_error("the 16-bit operator runs on one rank without ghost zones"); return -1; }
  CHK(half_links(c, nullptr, nullptr, nullptr, nullptr));
  const int nbd = (c->g.Vh + 255) / 256 + 4;
  const size_t nvec = (size_t)c->g.ntile * 192;
  const int nbb = (int)std::max<size_t>(1, std::min<size_t>((nvec + 255) / 256, 2048));
  const size_t per = (size_t)nbd + std::max(grid_sites(nsite_h(c)), nbb);
  BatchHalfState *S;
  CHK(bh_state(c, n, per, &S));
  HIPCHK(hipMemsetAsync(S->s, 0, sizeof(SlpScal) * QX_MAXRHS, c->stream));       // every system live
  const int px = par_even ? 0 : 1;
  MrhsArgs<StoreHalf> A1, A2;
  memset(&A1, 0, sizeof A1); memset(&A2, 0, sizeof A2);
  for (int j = 0; j < n; j++) {
    DevFieldH *const fj = &S->f[BH_N * j];
    CHK(half_from_f64(c, fj[BH_P].par(px), fx[j]->par(px)));
    A1.in[j] = fj[BH_P].par(px); A1.out[j] = fj[BH_T].par(1 - px);
    A2.in[j] = fj[BH_T].par(1 - px); A2.out[j] = fj[BH_AP].par(px); A2.xs[j] = fj[BH_P].par(px);
    A2.cb[j] = (float)(4.0 * m2[j]);
    A2.partials[j] = S->partials + (size_t)nbd * j;
  }
  int fmt = 0;
  CHK(mrhs_links(c, n, px, S->s, A1, A2, &fmt));
  CHK(sweep_mrhs(c, A1, fmt, false));
  CHK(sweep_mrhs(c, A2, fmt, true));
  CHK(devjoin_flush(c));
  for (int j = 0; j < n; j++) CHK(half_to_f64(c, fr[j]->par(px), S->f[BH_N * j + BH_AP].par(px)));
  return 0;
}
