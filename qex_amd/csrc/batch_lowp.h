// batch_lowp.h -- THE host side of the reduced-precision lock-step batched CG (batch.hip's rule for the reliable-update solve): up to
// four solveXX's on the SAME links, their reduced-precision iterations advanced together so that the link copy is streamed ONCE per sweep
// for all of them.  One driver and one operator probe over the storage description St of dslash_lowp.h (StoreF32 / StoreHalf);
// batch_f32.hip and batch_half.hip instantiate them and keep what is theirs alone: the iteration kernels and BatchStore<St>, which says
// how a storage builds its links, sizes and launches its xpay / update kernels, converts a probe's operands and -- 16-bit -- guards
// against a stall.  Where QEX's measurement code asks for it: src/observables/conn4d.nim:52 and scalarTrace.nim:42 default to a sloppy
// solve, which src/quda/qudaWrapperImpl.nim:194-197 hands on as mixed precision, 16-bit storage for SloppyHalf.
//
// The rule: every system keeps its own state (SlpScal: sigma, alpha, beta, max|r_s|^2, upd / noupd / done, k, nupd; 16-bit: HalfStall
// too) and its arithmetic is, operation for operation, that of the single-system solve of the same storage (solver.cpp:
// solve_xx_sloppy_dev, solve_xx_half_dev) -- the sweep is k_dslash_mrhs_lowp<St, ..> (dslash_lowp.h: the single-system body per system),
// the iteration kernels are the single-system ones with the system in blockIdx.y and the single-system grid per system, the bookkeeping
// and the reliable update are k_slpb_* (batch_f32.hip) and the fp64 op_xx per system behind that system's `noupd` word, and the stall
// guard runs per system.  A system solved in a batch returns the bits -- solution, iterations, true residual, updates, fall-back -- it
// returns alone.
//
// One rank without ghost zones by default: t-sharded contexts are refused unless option "batch_ranks" is 1.  With it the sweep takes its
// HALO form (dslash_lowp.h: sweep_mrhs, all systems' faces in one exchange), every set of partials is summed over the ranks for all
// systems in ONE collective per reduction point (comm_allreduce_parts_multi: each system's sum formed as comm_allreduce_parts forms it
// alone) and the n states read back at the end of a chunk, each with its stall flag, are checked for agreement per system (slp_agree)
// before any rank acts on them.  "Alone" is then the single-system solve on the same sharded context, sweep form and transport.  The
// INVARIANT above slp_update holds per system: rank-global sums, hence the same flags on every rank; the host posts the same exchanges
// and collectives on every rank whatever the flags say.  The decision to enter half_finish_f32 -- itself sharded, it posts collectives --
// is taken for every system from the agreed state alone, on all ranks or on none.
#pragma once
#include "dslash_lowp.h"
#include <algorithm>

// The storage's side of the batch, specialised where its kernels are (batch_f32.hip, batch_half.hip):
//   STALL                      the stall guard and the fp32 finish exist (stall_init, stall: their launches)
//   PROBE, PROBE_SHARDED       the probe's name in its refusals, and its refusal on a t-sharded context
//   slot(c)                    the context's pointer to this storage's BatchLowpState
//   links(c, &fmt)             the storage's link copy, current
//   ensure(c, F)               a work field at the current geometry's size
//   extent(c), grid(c)         what the iteration kernels run over and their grid in x (the single-system kernels')
//   Iter, iter_args            the iteration kernels' argument for system j, from the bookkeeping's SlpBatch and the system's r_s, p_s, Ap_s
//   xpay, update               their launches on dim3(grid, n)
//   from_f64, to_f64           the probe's conversions on parity px
template <class St> struct BatchStore;

enum { BL_R = 0, BL_P, BL_AP, BL_T, BL_N };   // reduced-precision work fields per system

template <class St>
struct BatchLowpState {
  typename St::Field f[BL_N * QX_MAXRHS];
  DevFieldF xs[QX_MAXRHS];                    // the increments x_s, fp32 in both storages
  SlpScal *s = nullptr;
  HalfStall *stall = nullptr;                 // (16-bit storage alone allocates it)
  double *partials = nullptr;
  size_t npart = 0;
};

template <class St>
static void batch_lowp_free(qexhip_ctx *c) {
  auto *S = (BatchLowpState<St> *)BatchStore<St>::slot(c);
  if (!S) return;
  for (auto &f : S->f) if (f.d) (void)hipFree(f.d);
  for (auto &f : S->xs) if (f.d) (void)hipFree(f.d);
  if (S->s) (void)hipFree(S->s);
  if (S->stall) (void)hipFree(S->stall);
  if (S->partials) (void)hipFree(S->partials);
  delete S;
  BatchStore<St>::slot(c) = nullptr;
}

static inline int slp_grid(size_t nvec) { return (int)std::max<size_t>(1, std::min<size_t>((nvec + 255) / 256, 2048)); }   // the k_slp_* grid (grid_for)

// The partials of one batch: all systems' <p,Ap> ranges, nbd apart, then all systems' |r_s|^2 / |b - A x|^2 ranges, nbr apart -- one
// contiguous range per reduction point.  nbr holds the iteration kernels' grid nbx and the fp64 reliable-update kernels' grid nbb.
// (fp32 storage: nbx = nbb, so nbr = nbb -- (nbd + nbb) QX_MAXRHS doubles, <p,Ap> of system j at nbd j and |r_s|^2 at nbd QX_MAXRHS +
// nbb j, the layout the fp32 batch had before it shared this header.)
template <class St>
struct BatchLowpSizes {
  size_t nvec;     // float2 / double2 per parity: what the fp64 reliable-update kernels run over
  int nbd, nbb, nbx;
  size_t nbr;
  explicit BatchLowpSizes(qexhip_ctx *c)
      : nvec((size_t)c->g.ntile * 192),
        nbd((c->g.Vh + 255) / 256 + 4),                                        // room for a sweep's <p,Ap> partials (a split sweep rounds up per range)
        nbb(slp_grid(nvec)),
        nbx(BatchStore<St>::grid(c)),
        nbr((size_t)std::max(nbx, nbb)) {}
};

// the context's state of this storage with room for n systems
template <class St>
static int batch_lowp_ensure(qexhip_ctx *c, int n, const BatchLowpSizes<St> &z, BatchLowpState<St> **out) {
  using BS = BatchStore<St>;
  auto *S = (BatchLowpState<St> *)BS::slot(c);
  if (!S) { S = new BatchLowpState<St>(); BS::slot(c) = S; }
  if (!S->s) HIPCHK(hipMalloc((void **)&S->s, sizeof(SlpScal) * QX_MAXRHS));
  if constexpr (BS::STALL) {
    if (!S->stall) HIPCHK(hipMalloc((void **)&S->stall, sizeof(HalfStall) * QX_MAXRHS));
  }
  const size_t need = ((size_t)z.nbd + z.nbr) * QX_MAXRHS;
  if (S->npart < need) {
    if (S->partials) HIPCHK(hipFree(S->partials));
    S->partials = nullptr; S->npart = 0;
    HIPCHK(hipMalloc((void **)&S->partials, need * sizeof(double)));
    S->npart = need;
  }
  for (int j = 0; j < n; j++) {
    for (int k = 0; k < BL_N; k++) CHK(BS::ensure(c, S->f[BL_N * j + k]));
    CHK(f32_field_ensure(c, S->xs[j]));
  }
  *out = S;
  return 0;
}

// op_xx's two lock-step sweeps on parity px at m2[j]: Ap_j = 4 m2_j p_j - (2D)(2D) p_j through t_j, <p_j, Ap_j> partials nbd apart
template <class St>
static int batch_lowp_sweeps(qexhip_ctx *c, BatchLowpState<St> *S, const BatchLowpSizes<St> &z, int n, int px, const double *m2,
                             MrhsArgs<St> &A1, MrhsArgs<St> &A2, int *fmt) {
  memset(&A1, 0, sizeof A1); memset(&A2, 0, sizeof A2);
  for (int j = 0; j < n; j++) {
    typename St::Field *const fj = &S->f[BL_N * j];
    A1.in[j] = fj[BL_P].par(px); A1.out[j] = fj[BL_T].par(1 - px);
    A2.in[j] = fj[BL_T].par(1 - px); A2.out[j] = fj[BL_AP].par(px); A2.xs[j] = fj[BL_P].par(px);
    A2.cb[j] = (float)(4.0 * m2[j]);
    A2.partials[j] = S->partials + (size_t)z.nbd * j;
  }
  return mrhs_links(c, n, px, S->s, A1, A2, fmt);
}

// n (1..4) reduced-precision solveXX's in lock-step: solve_xx_batch_dev's semantics (own mass, r2req, iteration count; shared maxits),
// the single-system solve's start, iteration, stall guard and fp32 finish per system, in its loop: chunks of 32, one read of the n states
// per chunk, the reliable update posted every opt_sloppy_check-th iteration and at maxits.  iters: reduced-precision (+ fp32 finish)
// iterations; r2_over_b2: the TRUE residual; nupdates: reliable updates.  16-bit storage adds what it ran to c->slpb_last through its map.
template <class St>
static int solve_xx_batch_lowp(qexhip_ctx *c, int n, DevField **x, DevField **b, const double *mass, const double *r2req, int maxits,
                               int par_even, int *iters, double *r2_over_b2, int *nupdates) {
  using BS = BatchStore<St>;
  CHK(batch_sloppy_check(c, n, mass));
  int fmt = 0;
  CHK(BS::links(c, &fmt));
  const BatchLowpSizes<St> z(c);
  BatchLowpState<St> *S;
  CHK(batch_lowp_ensure(c, n, z, &S));
  DevField *w64[2 * QX_MAXRHS];
  CHK(batch_work_fields(c, 2 * QX_MAXRHS, w64));                             // r, A x per system
  const int par = par_even ? 0 : 1;
  typename BS::Iter H;
  SlpBatch L;
  memset(&H, 0, sizeof H); memset(&L, 0, sizeof L);
  L.s = S->s;
  double m2[QX_MAXRHS];
  DevField *rj[QX_MAXRHS], *axj[QX_MAXRHS];
  for (int j = 0; j < n; j++) {
    typename St::Field *const fj = &S->f[BL_N * j];
    DevFieldF *xs = &S->xs[j];
    rj[j] = w64[2 * j]; axj[j] = w64[2 * j + 1];
    m2[j] = mass[j] * mass[j];
    // exactly the start of the single-system solve: x = 0, b2, r = b, x_s = 0, k_slp_init
    CHK(blas_zero(c, *x[j], 2));
    CHK(blas_norm2(c, *b[j], par, &c->dscal[0]));
    CHK(blas_copy(c, *rj[j], *b[j], par));
    HIPCHK(hipMemsetAsync(xs->par(par), 0, xs->half * sizeof(float2), c->stream));
    CHK(slp_init(c, &S->s[j], r2req[j], maxits));
    L.x[j] = x[j]->par(par); L.r[j] = rj[j]->par(par); L.b[j] = b[j]->par(par); L.Ax[j] = axj[j]->par(par);
    L.xs[j] = xs->par(par);
    L.dotp[j] = S->partials + (size_t)z.nbd * j; L.r2p[j] = S->partials + (size_t)z.nbd * QX_MAXRHS + z.nbr * j;
    BS::iter_args(H, L, j, fj[BL_R].par(par), fj[BL_P].par(par), fj[BL_AP].par(par));
  }
  if constexpr (BS::STALL) CHK(BS::stall_init(c, S->stall, S->s, n));
  MrhsArgs<St> A1, A2;
  CHK(batch_lowp_sweeps(c, S, z, n, par, m2, A1, A2, &fmt));
  SlpScal h[QX_MAXRHS];
  HalfStall hs[QX_MAXRHS] = {};                                           // (no guard: never stalled)
  static_assert(sizeof(SlpScal) * QX_MAXRHS <= 2048 && sizeof(HalfStall) * QX_MAXRHS <= 2048, "pinned scratch layout");
  HalfStall *const pstall = (HalfStall *)((char *)c->pinned + 2048);     // (behind the SlpScal's)
  auto read_states = [&]() -> int {
    HIPCHK(hipMemcpyAsync(c->pinned, S->s, sizeof(SlpScal) * n, hipMemcpyDeviceToHost, c->stream));
    if constexpr (BS::STALL) HIPCHK(hipMemcpyAsync(pstall, S->stall, sizeof(HalfStall) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    memcpy(h, c->pinned, sizeof(SlpScal) * n);
    if constexpr (BS::STALL) memcpy(hs, pstall, sizeof(HalfStall) * n);
    return 0;
  };
  // sharded: every rank holds the same n states and stall flags before any of them acts on its copy (comm_allreduce_max takes four
  // values: one call per system)
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
        BS::xpay(c, H, L, n);
      }
      int ndot = 0;
      CHK(sweep_mrhs(c, A1, fmt, false));
      CHK(sweep_mrhs(c, A2, fmt, true, &ndot));
      CHK(comm_allreduce_parts_multi(c, n, L.dotp[0], z.nbd, ndot, L.s, 1, &ndot));
      CHK(devjoin_flush(c));            // (no-op when the all-reduce has taken the second sweep's join with it)
      {
        ScopedTimer tm(c, "blas", c->stream);
        BS::update(c, H, L, n, ndot);
      }
      HIPCHK(hipGetLastError());
      CHK(slpb_close(c, L, n, z.nbx, z.nbr));
      // the (device-gated) reliable update of every system whose `upd` is up, posted as the single-system solve posts its own, and each
      // system's stall guard behind it; a system that is done counts no further, so the host's k is each live system's own k
      if ((k + 1) % every == 0 || k + 1 >= maxits) {
        CHK(slpb_flush(c, L, n, z.nvec, z.nbb));
        for (int j = 0; j < n; j++) CHK(op_xx(c, *axj[j], *x[j], m2[j], par_even, 0, &S->s[j].noupd));
        CHK(slpb_resid(c, L, n, z.nvec, z.nbb, z.nbr));
        if constexpr (BS::STALL) CHK(BS::stall(c, S->stall, S->s, n, c->opt_half_stall));
      }
    }
    CHK(read_states());
    CHK(agree());
  }
  for (int j = 0; j < n; j++) {
    int its = h[j].k, nupd = h[j].nupd;
    double r2t = h[j].r2t;
    if constexpr (BS::STALL) {
      int its32 = 0, fell = 0;
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
      its += its32;
    }
    if (iters) iters[j] = its;
    if (r2_over_b2) r2_over_b2[j] = (h[j].b2 != 0.0) ? r2t / h[j].b2 : 0.0;
    if (nupdates) nupdates[j] = nupd;
  }
  return 0;
}

// fr_j[px] = the batched reduced-precision operator at m2_j on fx_j[px] rounded to the storage, back in fp64 (qexhip_dev_op_xx_sloppy_batch,
// qexhip_dev_op_xx_half_batch), on one rank and -- with option "batch_ranks" -- on t-sharded contexts
template <class St>
static int op_xx_batch_probe(qexhip_ctx *c, int n, DevField **fr, DevField **fx, const double *m2, int par_even) {
  using BS = BatchStore<St>;
  if (n < 1 || n > QX_MAXRHS) { qexhip_set_error("%s: 1 <= n <= %d", BS::PROBE, QX_MAXRHS); return -1; }
  if ((c->nranks > 1 || c->g.halo) && !c->opt_batch_ranks) { qexhip_set_error("%s", BS::PROBE_SHARDED); return -1; }
  int fmt = 0;
  CHK(BS::links(c, &fmt));
  const BatchLowpSizes<St> z(c);
  BatchLowpState<St> *S;
  CHK(batch_lowp_ensure(c, n, z, &S));
  HIPCHK(hipMemsetAsync(S->s, 0, sizeof(SlpScal) * QX_MAXRHS, c->stream));       // every system live
  const int px = par_even ? 0 : 1;
  for (int j = 0; j < n; j++) CHK(BS::from_f64(c, S->f[BL_N * j + BL_P], *fx[j], px));
  MrhsArgs<St> A1, A2;
  CHK(batch_lowp_sweeps(c, S, z, n, px, m2, A1, A2, &fmt));
  CHK(sweep_mrhs(c, A1, fmt, false));
  CHK(sweep_mrhs(c, A2, fmt, true));
  CHK(devjoin_flush(c));
  for (int j = 0; j < n; j++) CHK(BS::to_f64(c, *fr[j], S->f[BL_N * j + BL_AP], px));
  return 0;
}
