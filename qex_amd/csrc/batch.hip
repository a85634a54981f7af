// batch.hip -- several independent even/odd CG solves on the SAME links advanced in lock-step.
//
// QEX's HMC solves one system after another on unchanged links: the Hasenbusch chain of the action and
// of the force (src/examples/staghmc_sh.nim:339-364,394-404: masses m, h0, h1 per species), the pbp
// repetitions (:260-272), the fork's fforce loop (src/stagg_pv_hmc/staghmc_spv.nim:758-830).  Each is
// `stag.solve` -> solveXX -> CG (src/physics/stagSolve.nim:57-138, src/solvers/cg.nim:55-272).  The Dslash
// is HBM-bound and 89 % of its bytes are links, so streaming the links ONCE for up to four right-hand
// sides cuts the bytes per system from 864 to (768 + 96 n)/n (352 at n = 3, compressed links).  One sweep
// body, mrhs_body, behind the kernels k_dslash_mrhs (sites from the field) and k_dslash_mrhs_fused (fused_sweep.h).  Every
// system keeps its own CG state (alpha, beta, residual, iteration count, done flag) and its arithmetic
// is, operation for operation, that of the single-system path (same per-site accumulation order, same
// workgroup partials, same fixed-order final sums), so each solution and iteration count equals what
// qexhip_stag_solve_xx returns for that system alone.  t-sharded runs exchange the faces of all systems, then
// sweep the slab in one launch, and all-reduce the n scalars of a reduction in ONE call.
#include "qexhip_internal.h"
#include "site_index.h"
#include "reduce.h"
#include "dslash_core.h"
#include "fused_sweep.h"
#include "full_solve.h"
#include <algorithm>
#include <cstring>
#include <type_traits>
#include <vector>

#define QX_MAXRHS 4

struct MrhsArgs {
  Geom g;
  const double2 *W;
  const unsigned long long *S;
  const double2 *in[QX_MAXRHS];
  double2 *out[QX_MAXRHS];
  const double2 *xs[QX_MAXRHS];
  double cb[QX_MAXRHS];
  double *partials[QX_MAXRHS];
  const CgScal *st;            // st[j].done switches system j off
  int parity, nrhs, swz, ntstore;
  SweepRanges r;               // [c0, c1) for workgroups < nb1, [d0, d1) for the rest (both t-faces in one launch; fused: interior, low face)
  int part_off;                // first <xs, out> partial this launch writes
};
// what the fused launch carries beside them
struct MrhsFusedArgs {
  MrhsArgs a;
  FusedSweep fs;                    // e0..e1 high face, push, ghost words, bookkeeping
  const double2 *gh_hi[QX_MAXRHS], *gh_lo[QX_MAXRHS];
};
__device__ __forceinline__ const MrhsArgs &mrhs_args(const MrhsArgs &P) { return P; }
__device__ __forceinline__ const MrhsArgs &mrhs_args(const MrhsFusedArgs &P) { return P.a; }

// The lock-step sweep's one body, dslash_body (dslash.hip) for up to four systems: each pair of links is fetched once (LinkCursor) and
// applied to every live system.
//   SECOND = false: out_j = +sum_mu (U in_j(+mu) - U^+ in_j(-mu))              (stagDP, first half of stagD2ee)
//   SECOND = true : out_j = cb_j xs_j - sum_mu (...), partial <xs_j, out_j>   (stagDM + 4m^2 x + <p,Ap>)
//   Args = MrhsArgs (FUSED false): the sites of sweep_site, t-neighbours from the field (HALO: its ghost tiles); XCD swizzle as k_dslash
//   Args = MrhsFusedArgs (FUSED true): the sweep of a t-sharded slab on the peer transport as ONE launch on ONE stream, with the
//            workgroup roles of fused_sweep.h (the push workgroups send the faces of all systems, one piece each).  A system's arithmetic
//            is k_dslash_fused's: same hop order (local first), same partial slots; parked or not a block gives the same bits.
// Every hop loop stays rolled: four systems' accumulators leave no registers for a second pair of links in flight (220 VGPRs at
// <8,1,true,false>, 2 waves per SIMD; profiles/sweep_refactor_resources.txt).
template <int NDIR, int RECON, bool SECOND, bool HALO, class Args>
__device__ __forceinline__ void mrhs_body(const Args &P) {
  constexpr bool FUSED = std::is_same<Args, MrhsFusedArgs>::value;
  const MrhsArgs &A = mrhs_args(P);
  bool act[QX_MAXRHS];
  bool any = false;
#pragma unroll
  for (int j = 0; j < QX_MAXRHS; j++) { act[j] = j < A.nrhs && !A.st[j].done; any = any || act[j]; }
  const bool skip = !any;              // every system has converged: nothing is pushed, a fused launch still returns the credits it owes
  if (skip && !FUSED) return;
  FusedRole R;
  if constexpr (FUSED) {
    if (fused_push(P.fs, skip)) return;
    fused_enter(P.fs, A.r.nb1, R);
  } else {
    R.bid = blockIdx.x; R.cleanup = false; R.bnd = false; R.parked = false;
  }
  for (;;) {                               // one pass; a cleanup workgroup takes every fz.ncl-th parked block
    // (lb is fused_next_block's to set in the fused kernel: initialised from R.bid there as well, k_dslash_mrhs_fused<8,0,false> takes
    // 171 VGPRs instead of the 165 of the two-kernel form and drops from 3 to 2 waves per SIMD)
    int lb, clim, c;
    if constexpr (!FUSED) lb = R.bid;
    if constexpr (FUSED) {
      if (!fused_next_block(P.fs, R, lb)) break;
      c = fused_site(P.fs, R, lb, A.r, clim);
    } else {
      if (A.swz) lb = (lb & 7) * (A.swz >> 3) + (lb >> 3);
      sweep_site(A.r, lb, c, clim);
    }
    double dotv[QX_MAXRHS] = {0, 0, 0, 0};
    const bool active = c < clim && !skip;
    const Geom &g = A.g;
    const SiteXYZT s = site_coord(g, c, A.parity);
    const int tu = FUSED ? __builtin_amdgcn_readfirstlane(s.t) : 0;
    const bool hi1 = tu + 1 >= g.X[3], lo1 = tu - 1 < 0, hi3 = tu + 3 >= g.X[3], lo3 = tu - 3 < 0;
    double2 acc[QX_MAXRHS][3], xsv[QX_MAXRHS][3];
    const double sgn = SECOND ? -1.0 : 1.0;
    const LinkCursor<NDIR, RECON> L(A.W, A.S, c);
    auto pair = [&](const int pr, const bool do_f, const bool do_b) __attribute__((always_inline)) {
      const int mu = pr & 3;
      const int hop = pr >= 4 ? 3 : 1;
      const int pf = nbr_pos<HALO>(g, c, s, mu, hop);
      const int pb = nbr_pos<HALO>(g, c, s, mu, -hop);
      double2 U[9], Wm[9];
      L.fetch(pr, do_f, do_b, U, Wm);
      // fused: this hop leaves the slab (wavefront-uniform) and reads the neighbour's face where the neighbour wrote it
      const bool xf = FUSED && mu == 3 && (hop == 3 ? hi3 : hi1), xb = FUSED && mu == 3 && (hop == 3 ? lo3 : lo1);
#pragma unroll
      for (int j = 0; j < QX_MAXRHS; j++) {
        if (!act[j]) continue;
        double2 vf[3], vb[3];
        if (do_f) {
          const double2 *src = A.in[j];
          if constexpr (FUSED) src = xf ? P.gh_hi[j] : A.in[j];
#pragma unroll
          for (int k = 0; k < 3; k++) vf[k] = src[vec_off(pf, k)];
          mv3<false>(acc[j], U, vf);
        }
        if (do_b) {
          const double2 *src = A.in[j];
          if constexpr (FUSED) src = xb ? P.gh_lo[j] : A.in[j];
#pragma unroll
          for (int k = 0; k < 3; k++) vb[k] = src[vec_off(pb, k)];
          mv3<true>(acc[j], Wm, vb);
        }
      }
    };
    // boundary blocks of the fused sweep: `crossing` false takes every hop but the t-hops that leave the slab, true exactly those
    auto edge_pairs = [&](const bool crossing) __attribute__((always_inline)) {
      if (!crossing) {
        constexpr int NSP = NDIR / 2 - NDIR / 8;
#pragma unroll 1
        for (int q = 0; q < NSP; q++) pair(q + q / 3, true, true);
      }
#pragma unroll 1
      for (int pr = 3; pr < NDIR / 2; pr += 4) {
        const int hop = pr >= 4 ? 3 : 1;
        const bool xf = tu + hop >= g.X[3], xb = tu - hop < 0;
        pair(pr, crossing ? xf : !xf, crossing ? xb : !xb);
      }
    };
    if (active) {
#pragma unroll
      for (int j = 0; j < QX_MAXRHS; j++) {
        if (!act[j]) continue;
        if (SECOND) {
#pragma unroll
          for (int k = 0; k < 3; k++) xsv[j][k] = A.xs[j][vec_off(c, k)];
        }
        if (R.cleanup) {
#pragma unroll
          for (int k = 0; k < 3; k++) acc[j][k] = A.out[j][vec_off(c, k)];          // the raw accumulator its boundary workgroup parked here
        } else if (SECOND) {
#pragma unroll
          for (int k = 0; k < 3; k++) {
            acc[j][k].x = (sgn * A.cb[j]) * xsv[j][k].x;
            acc[j][k].y = (sgn * A.cb[j]) * xsv[j][k].y;
          }
        } else {
#pragma unroll
          for (int k = 0; k < 3; k++) acc[j][k] = make_double2(0.0, 0.0);
        }
      }
      if (!R.bnd) {
#pragma unroll 1
        for (int pr = 0; pr < NDIR / 2; pr++) pair(pr, true, true);
      } else if (!R.cleanup) {
        edge_pairs(false);
      }
    }
    if (R.bnd && !skip) {
      if constexpr (FUSED) fused_wait_faces(P.fs, R);
      if (active && !R.parked) edge_pairs(true);
    }
    if (active) {
#pragma unroll
      for (int j = 0; j < QX_MAXRHS; j++) {
        if (!act[j]) continue;
        if (R.parked) {
#pragma unroll
          for (int k = 0; k < 3; k++) A.out[j][vec_off(c, k)] = acc[j][k];
        } else {
#pragma unroll
          for (int k = 0; k < 3; k++) {
            acc[j][k].x *= sgn; acc[j][k].y *= sgn;
            if (FUSED || A.ntstore) {
              d2v t; t.x = acc[j][k].x; t.y = acc[j][k].y;
              __builtin_nontemporal_store(t, (d2v *)&A.out[j][vec_off(c, k)]);
            } else {
              A.out[j][vec_off(c, k)] = acc[j][k];
            }
          }
          if (SECOND) {
#pragma unroll
            for (int k = 0; k < 3; k++) dotv[j] = fma(xsv[j][k].x, acc[j][k].x, fma(xsv[j][k].y, acc[j][k].y, dotv[j]));
          }
        }
      }
    }
    if (SECOND && !skip && !R.parked) {
      int pidx = blockIdx.x;               // the dispatch slot, swizzled or not
      if constexpr (FUSED) pidx = fused_partial_slot(P.fs, R, lb);
#pragma unroll
      for (int j = 0; j < QX_MAXRHS; j++) {
        if (!act[j]) continue;             // uniform over the grid
        double r = block_sum_256(dotv[j]);
        if (threadIdx.x == 0) A.partials[j][A.part_off + pidx] = r;
      }
    }
    if (!R.cleanup) break;
  }
  if constexpr (FUSED) fused_finish(P.fs, R);
}

template <int NDIR, int RECON, bool SECOND, bool HALO>
__global__ void __launch_bounds__(256) k_dslash_mrhs(MrhsArgs A) { mrhs_body<NDIR, RECON, SECOND, HALO>(A); }
template <int NDIR, int RECON, bool SECOND>
__global__ void __launch_bounds__(256) k_dslash_mrhs_fused(MrhsFusedArgs F) { mrhs_body<NDIR, RECON, SECOND, true>(F); }

struct BatchBlas {
  double2 *x[QX_MAXRHS], *r[QX_MAXRHS], *p[QX_MAXRHS], *Ap[QX_MAXRHS];
  double *dotp[QX_MAXRHS], *r2p[QX_MAXRHS];
  CgScal *st;
  double *glob;      // multi-rank: [0..4) rank-summed <p,Ap>, [4..8) rank-summed |r|^2 (contiguous for one all-reduce)
  int ndot;          // > 0: deferred <p,Ap> partial sum inside k_cgb_update; 0: pAp from the state; -1: from glob
};
// the CG kernels of blas.hip in their round-1 form (xpay, update, one-block reduce + bookkeeping), system = blockIdx.y
__global__ void __launch_bounds__(256) k_cgb_xpay(BatchBlas B, size_t n) {
  const int j = blockIdx.y;
  const CgScal *s = &B.st[j];
  if (s->done) return;
  const bool first = (s->itn == 0);
  const double beta = s->r2 / s->rzo;
  double2 *p = B.p[j];
  const double2 *r = B.r[j];
  for (size_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    double2 rv = r[i];
    if (first) p[i] = rv;
    else {
      double2 pv = p[i];
      p[i] = make_double2(rv.x + beta * pv.x, rv.y + beta * pv.y);
    }
  }
}
__global__ void __launch_bounds__(256) k_cgb_update(BatchBlas B, size_t n) {
  const int j = blockIdx.y;
  const CgScal *s = &B.st[j];
  if (s->done) return;
  double pAp = B.ndot < 0 ? B.glob[j] : s->pAp;
  if (B.ndot > 0) {
    double a = 0;
    for (int i = threadIdx.x; i < B.ndot; i += 256) a += B.dotp[j][i];
    pAp = block_sum_256_all(a);
  }
  const double alpha = s->r2 / pAp;
  double2 *x = B.x[j], *r = B.r[j];
  const double2 *p = B.p[j], *Ap = B.Ap[j];
  double acc = 0;
  for (size_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    double2 pv = p[i], xv = x[i], rv = r[i], av = Ap[i];
    xv.x += alpha * pv.x; xv.y += alpha * pv.y;
    rv.x -= alpha * av.x; rv.y -= alpha * av.y;
    x[i] = xv; r[i] = rv;
    acc = fma(rv.x, rv.x, fma(rv.y, rv.y, acc));
  }
  double t = block_sum_256(acc);
  if (threadIdx.x == 0) B.r2p[j][blockIdx.x] = t;
}
// big local volumes: one-block final sum of the <p,Ap> partials per system (as reduce_partials does for the
// single-system path beyond 4096 workgroups); k_cgb_update then takes pAp from the state (ndot = 0)
__global__ void __launch_bounds__(256) k_cgb_reduce_dot(BatchBlas B, int n) {
  const int j = blockIdx.x;
  CgScal *s = &B.st[j];
  if (s->done) return;
  double acc = 0;
  for (int i = threadIdx.x; i < n; i += 256) acc += B.dotp[j][i];
  double r = block_sum_256(acc);
  if (threadIdx.x == 0) s->pAp = r;
}
// multi-rank pieces: local sums into the contiguous buffer (then ONE ncclAllReduce for all systems), bookkeeping from it
__global__ void __launch_bounds__(256) k_cgb_local_sum(BatchBlas B, int n, int which) {   // which 0: <p,Ap>, 1: |r|^2
  const int j = blockIdx.x;
  if (B.st[j].done) { if (threadIdx.x == 0) B.glob[4 * which + j] = 0.0; return; }
  const double *src = which ? B.r2p[j] : B.dotp[j];
  double acc = 0;
  for (int i = threadIdx.x; i < n; i += 256) acc += src[i];
  double r = block_sum_256(acc);
  if (threadIdx.x == 0) B.glob[4 * which + j] = r;
}
__global__ void k_cgb_finish_glob(BatchBlas B, int n) {
  for (int j = threadIdx.x; j < n; j += blockDim.x) {
    CgScal *s = &B.st[j];
    if (s->done) continue;
    s->rzo = s->r2;
    s->r2 = B.glob[4 + j];
    s->itn += 1;
    if (!(s->itn < s->maxits && s->r2 > s->r2stop)) s->done = 1;
  }
}
__global__ void __launch_bounds__(256) k_cgb_reduce_finish(BatchBlas B, int n) {
  const int j = blockIdx.x;
  CgScal *s = &B.st[j];
  if (s->done) return;
  double acc = 0;
  for (int i = threadIdx.x; i < n; i += 256) acc += B.r2p[j][i];
  double r = block_sum_256(acc);
  if (threadIdx.x == 0) {
    s->rzo = s->r2;
    s->r2 = r;
    s->itn += 1;
    if (!(s->itn < s->maxits && s->r2 > s->r2stop)) s->done = 1;
  }
}

struct BatchState {
  std::vector<DevField> f;     // r, p, Ap, t per system
  CgScal *st = nullptr;
  double *glob = nullptr;
  double *partials = nullptr;
  size_t npart = 0;
};
void batch_state_free(qexhip_ctx *c) {
  BatchState *b = (BatchState *)c->batch;
  if (!b) return;
  for (auto &f : b->f) (void)hipFree(f.d);
  if (b->st) (void)hipFree(b->st);
  if (b->glob) (void)hipFree(b->glob);
  if (b->partials) (void)hipFree(b->partials);
  delete b;
  c->batch = nullptr;
}

// the batch state with at least nfields work fields
static int batch_state(qexhip_ctx *c, int nfields, BatchState **out) {
  BatchState *B = (BatchState *)c->batch;
  if (!B) { B = new BatchState(); c->batch = B; }
  while ((int)B->f.size() < nfields) {
    DevField nf;
    CHK(field_alloc(c, nf));
    B->f.push_back(nf);
  }
  *out = B;
  return 0;
}

template <int NDIR, int RECON>
static void launch_mrhs(const qexhip_ctx *c, bool second, int nb, hipStream_t st, const MrhsArgs &A) {
  if (c->g.halo) {
    if (second) hipLaunchKernelGGL((k_dslash_mrhs<NDIR, RECON, true, true>), dim3(nb), dim3(256), 0, st, A);
    else hipLaunchKernelGGL((k_dslash_mrhs<NDIR, RECON, false, true>), dim3(nb), dim3(256), 0, st, A);
  } else {
    if (second) hipLaunchKernelGGL((k_dslash_mrhs<NDIR, RECON, true, false>), dim3(nb), dim3(256), 0, st, A);
    else hipLaunchKernelGGL((k_dslash_mrhs<NDIR, RECON, false, false>), dim3(nb), dim3(256), 0, st, A);
  }
}
template <int NDIR, int RECON>
static void launch_mrhs(const qexhip_ctx *, bool second, int nb, hipStream_t st, const MrhsFusedArgs &F) {
  if (second) hipLaunchKernelGGL((k_dslash_mrhs_fused<NDIR, RECON, true>), dim3(nb), dim3(256), 0, st, F);
  else hipLaunchKernelGGL((k_dslash_mrhs_fused<NDIR, RECON, false>), dim3(nb), dim3(256), 0, st, F);
}
// nb workgroups of the kernel for this context's links: k_dslash_mrhs for MrhsArgs, k_dslash_mrhs_fused for MrhsFusedArgs
template <class Args>
static void dispatch_mrhs(qexhip_ctx *c, const Args &P, bool second, int nb, hipStream_t st) {
  if (c->ndir == 8) {
    if (c->recon == 1) launch_mrhs<8, 1>(c, second, nb, st, P);
    else if (c->recon == 2) launch_mrhs<8, 2>(c, second, nb, st, P);
    else launch_mrhs<8, 0>(c, second, nb, st, P);
  } else {
    if (c->recon == 1) launch_mrhs<16, 1>(c, second, nb, st, P);
    else if (c->recon == 2) launch_mrhs<16, 2>(c, second, nb, st, P);
    else launch_mrhs<16, 0>(c, second, nb, st, P);
  }
}
// one launch over [c0, c1) (+ [d0, d1)); returns the number of workgroups = <xs, out> partials it writes from part_off on
static int launch_range(qexhip_ctx *c, MrhsArgs &A, bool second, int c0, int c1, int d0, int d1, int part_off, hipStream_t st) {
  const int nb = sweep_ranges(A.r, c0, c1, d0, d1);
  if (!nb) return 0;
  A.part_off = part_off;
  const bool whole = (c0 == 0 && c1 == c->g.Vh && d1 <= d0);
  A.swz = (whole && c->recon != 0 && nb >= 64 && (nb & 7) == 0) ? nb : 0;     // as dslash.hip: on for compressed links
  A.ntstore = 1;
  dispatch_mrhs(c, A, second, nb, st);
  return nb;
}
// t-sharded: the faces of every system's input field travel in ONE RCCL group; either exchange-first and one launch over the
// slab, or -- where dslash_sweep overlaps (sweep_plan) -- the group and the boundary launch on the comm stream beside the
// interior launch, exactly the structure of dslash_sweep.  *ndot = number of <xs, out> partials the sweep wrote.
static int sweep_mrhs(qexhip_ctx *c, MrhsArgs &A, bool second, int *ndot, DevField *const *infield = nullptr, int inpar = 0) {
  const Geom &g = c->g;
  int lo_end = 0, hi_beg = g.Vh, overlap = 0;
  if (g.halo) sweep_plan(c, &lo_end, &hi_beg, &overlap);
  // the decision of sweep_plan is for ONE system's faces; a batch moves nrhs times as much per exchange, and between distinct
  // GPUs that transfer is what the overlap is for: with a real communicator, overlap from 1 MiB of faces per direction on
  // -- unless the single-system form was MEASURED at set_links and lost: a measurement outranks the rule (round-4 advice)
  if (g.halo && !overlap && c->opt_overlap < 0 && c->nranks > 1 && hi_beg > lo_end && c->overlap_auto[c->ndir == 16] < 0 &&
      (size_t)A.nrhs * g.depth * g.F * 48 >= ((size_t)1 << 20)) overlap = 1;
  if (g.halo && overlap && sweep_form(c, overlap) == 2) {
    // the fused lock-step sweep (peer transport): the launch pushes all systems' faces itself and reads what arrives in the arena
    MrhsFusedArgs Fz;
    memset(&Fz, 0, sizeof Fz);
    CHK(devjoin_flush(c));
    int grid;
    CHK(fused_sweep_setup(c, A.nrhs, infield, inpar, lo_end, hi_beg, &Fz.fs, Fz.gh_hi, Fz.gh_lo, &grid, ndot));
    // interior | low face; the high face is Fz.fs's.  The fused form is an overlapped one, and sweep_plan overlaps only a non-empty
    // interior: the ranges are taken as given (no swap), as fused_sweep_setup counted them
    if (hi_beg <= lo_end || !sweep_ranges(A.r, lo_end, hi_beg, 0, lo_end)) { qexhip_set_error("internal: fused batch sweep without an interior"); return -3; }
    A.part_off = 0; A.swz = 0; A.ntstore = 1;
    Fz.a = A;
    ScopedTimer tm(c, "dslash_batch", c->stream);
    dispatch_mrhs(c, Fz, second, grid, c->stream);
    HIPCHK(hipGetLastError());
    return 0;
  }
  if (g.halo && overlap) HIPCHK(hipEventRecord(c->ev_ready, c->stream));
  if (g.halo) CHK(comm_halo_exchange_multi(c, A.nrhs, infield, inpar, overlap));
  ScopedTimer tm(c, "dslash_batch", c->stream);
  if (!overlap) {
    *ndot = launch_range(c, A, second, 0, g.Vh, 0, 0, 0, c->stream);
  } else {
    const int nb_int = launch_range(c, A, second, lo_end, hi_beg, 0, 0, 0, c->stream);
    const int nb_bnd = launch_range(c, A, second, 0, lo_end, hi_beg, g.Vh, nb_int, c->cstream);
    CHK(devjoin_signal(c, c->cstream));               // device-side join (as dslash_sweep): ~15 us instead of the ~28 us of an event dependency
    CHK(devjoin_wait(c, c->stream, c->cstream));
    *ndot = nb_int + nb_bnd;
  }
  HIPCHK(hipGetLastError());
  return 0;
}

// n (1..4) solveXX's in lock-step; x[j], b[j] device fields (x zeroed here, as solveXX does)
int solve_xx_batch_dev(qexhip_ctx *c, int n, DevField **x, DevField **b, const double *mass, const double *r2req,
                       int maxits, int par_even, int *iters, double *r2_over_b2) {
  const Geom &g = c->g;
  if (n < 1 || n > QX_MAXRHS) { qexhip_set_error("batch solve: 1 <= n <= %d", QX_MAXRHS); return -1; }
  if (!c->W) { qexhip_set_error("staggered links not set (qexhip_stag_set_links)"); return -3; }
  for (int j = 0; j < n; j++) if (mass[j] == 0.0) { qexhip_set_error("batch solve: mass must be non-zero"); return -1; }
  BatchState *B;
  CHK(batch_state(c, 4 * QX_MAXRHS, &B));
  if (!B->st) HIPCHK(hipMalloc((void **)&B->st, sizeof(CgScal) * QX_MAXRHS));
  if (!B->glob) { HIPCHK(hipMalloc((void **)&B->glob, sizeof(double) * 8)); HIPCHK(hipMemsetAsync(B->glob, 0, sizeof(double) * 8, c->stream)); }
  const int nbd = (g.Vh + 255) / 256 + 4;             // room for the <p,Ap> partials of a sweep per system (a split sweep rounds up per range)
  const size_t nvec = (size_t)g.ntile * 192;
  const int nbb = (int)std::min<size_t>((nvec + 255) / 256, 2048);
  const size_t per = (size_t)nbd + nbb;
  if (B->npart < per * QX_MAXRHS) {
    if (B->partials) HIPCHK(hipFree(B->partials));
    B->partials = nullptr; B->npart = 0;
    HIPCHK(hipMalloc((void **)&B->partials, per * QX_MAXRHS * sizeof(double)));
    B->npart = per * QX_MAXRHS;
  }
  const int par = par_even ? 0 : 1;
  MrhsArgs A1, A2;
  BatchBlas L;
  DevField *pf[QX_MAXRHS], *tf[QX_MAXRHS];
  memset(&A1, 0, sizeof A1); memset(&A2, 0, sizeof A2); memset(&L, 0, sizeof L);
  for (int j = 0; j < n; j++) {
    DevField &r = B->f[4 * j], &p = B->f[4 * j + 1], &Ap = B->f[4 * j + 2], &t = B->f[4 * j + 3];
    // exactly the start of solve_xx_dev (solver.cpp): x = 0, b2, r = b, r2, cg_init -> copy the state
    CHK(blas_zero(c, *x[j], 2));
    CHK(blas_norm2(c, *b[j], par, &c->dscal[0]));
    CHK(blas_copy(c, r, *b[j], par));
    CHK(blas_norm2(c, r, par, &c->dscal[1]));
    CHK(cg_init(c, r2req[j], maxits));
    HIPCHK(hipMemcpyAsync(&B->st[j], c->cg, sizeof(CgScal), hipMemcpyDeviceToDevice, c->stream));
    pf[j] = &p; tf[j] = &t;
    A1.in[j] = p.par(par); A1.out[j] = t.par(1 - par);
    A2.in[j] = t.par(1 - par); A2.out[j] = Ap.par(par); A2.xs[j] = p.par(par);
    A2.cb[j] = 4.0 * mass[j] * mass[j];
    A2.partials[j] = B->partials + per * j;
    L.x[j] = x[j]->par(par); L.r[j] = r.par(par); L.p[j] = p.par(par); L.Ap[j] = Ap.par(par);
    L.dotp[j] = B->partials + per * j; L.r2p[j] = B->partials + per * j + nbd;
  }
  const bool multi = c->nranks > 1 || c->opt_batch_multi;
  const bool deferred = !multi && nbd <= 4096;          // same switch as dslash_sweep / k_cg_update
  L.st = B->st; L.glob = B->glob; L.ndot = multi ? -1 : (deferred ? nbd : 0);
  for (MrhsArgs *A : {&A1, &A2}) {
    A->g = g; A->st = B->st; A->nrhs = n;
    A->parity = (A == &A1) ? 1 - par : par;
    stag_link_bases(c, A->parity, false, &A->W, &A->S);       // (lossless links: the batch reads the 18 reals kept beside them)
  }
  CgScal st[QX_MAXRHS];
  auto read_states = [&]() -> int {
    HIPCHK(hipMemcpyAsync(c->pinned, B->st, sizeof(CgScal) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    memcpy(st, c->pinned, sizeof(CgScal) * n);
    return 0;
  };
  CHK(read_states());
  for (;;) {
    int left = 0;
    for (int j = 0; j < n; j++) if (!st[j].done) left = std::max(left, st[j].maxits - st[j].itn);
    if (left <= 0) break;
    const int chunk = std::min(32, left);
    for (int i = 0; i < chunk; i++) {
      {
        ScopedTimer tm(c, "blas", c->stream);
        k_cgb_xpay<<<dim3(nbb, n), 256, 0, c->stream>>>(L, nvec);
      }
      int nd1 = 0, ndots = 0;
      CHK(sweep_mrhs(c, A1, false, &nd1, pf, par));
      CHK(sweep_mrhs(c, A2, true, &ndots, tf, 1 - par));
      if (!multi && deferred) L.ndot = ndots;
      if (multi) {
        k_cgb_local_sum<<<n, 256, 0, c->stream>>>(L, ndots, 0);
        CHK(comm_allreduce(c, B->glob, n));
      } else if (!deferred) {
        k_cgb_reduce_dot<<<n, 256, 0, c->stream>>>(L, ndots);
      }
      {
        ScopedTimer tm(c, "blas", c->stream);
        k_cgb_update<<<dim3(nbb, n), 256, 0, c->stream>>>(L, nvec);
      }
      if (multi) {
        k_cgb_local_sum<<<n, 256, 0, c->stream>>>(L, nbb, 1);
        CHK(comm_allreduce(c, B->glob + 4, n));
        k_cgb_finish_glob<<<1, 64, 0, c->stream>>>(L, n);
      } else {
        k_cgb_reduce_finish<<<n, 256, 0, c->stream>>>(L, nbb);
      }
      HIPCHK(hipGetLastError());
    }
    CHK(read_states());
  }
  for (int j = 0; j < n; j++) {
    if (iters) iters[j] = st[j].itn;
    if (r2_over_b2) r2_over_b2[j] = (st[j].b2 != 0.0) ? st[j].r2 / st[j].b2 : 0.0;
  }
  return 0;
}

// ---- n full solves D x_j = b_j (Staggered.solve, stagSolve.nim:224-294) with the even/odd CGs batched ----
// Per system the decisions of solve_full_dev / solve_inner (solver.cpp), from the same eo_plan (full_solve.h): reconstruct-right
// for one-parity sources (the HMC case: phi.odd = 0), reconstruct-left otherwise, true-residual outer loop.
namespace {
struct Sys {
  DevField *x, *b, *r, *y, *d;    // solution, source, residual, inner solution, inner source / work
  double m, r2req, b2, r2stop, r2e, r2o;
  int its, n;
  EoPlan pl;
  DevField *src;
};
}  // namespace

// sloppy > 0: the inner solveXX's are the mixed-precision lock-step batch (batch_f32.hip), nupdates[j] <- system j's reliable updates
// defl (with nev > 0): the inner solveXX groups of BOTH parities are the deflated batch (solver.cpp); the ReconL / ReconR decisions, the
// outer loop and the sharing of maxits are the same
static int solve_full_batch_impl(qexhip_ctx *c, int n, DevField **x, DevField **b, const double *mass, const double *r2req,
                                 int maxits, int *iters, double *r2_final, int sloppy, int *nupdates, EigBasis *defl = nullptr, int nev = 0) {
  if (n < 1 || n > QX_MAXRHS) { qexhip_set_error("batch solve: 1 <= n <= %d", QX_MAXRHS); return -1; }
  BatchState *B;
  CHK(batch_state(c, 7 * QX_MAXRHS, &B));        // 4 CG fields + r, y, d per system
  Sys S[QX_MAXRHS];
  std::vector<int> active;
  for (int j = 0; j < n; j++) {
    Sys &s = S[j];
    s.x = x[j]; s.b = b[j];
    s.r = &B->f[4 * QX_MAXRHS + 3 * j]; s.y = &B->f[4 * QX_MAXRHS + 3 * j + 1]; s.d = &B->f[4 * QX_MAXRHS + 3 * j + 2];
    s.m = mass[j]; s.r2req = r2req[j]; s.its = 0;
    if (nupdates) nupdates[j] = 0;
    CHK(blas_norm2(c, *s.b, 2, &c->dscal[2]));
    CHK(read_scalars(c, &c->dscal[2], 1, &s.b2));
    s.r2stop = s.r2req * s.b2;
    CHK(blas_zero(c, *s.x, 2));
    CHK(blas_copy(c, *s.r, *s.b, 2));
    CHK(norm2_eo(c, *s.r, &s.r2e, &s.r2o));
    if (s.r2e + s.r2o > s.r2stop) active.push_back(j);
  }
  while (!active.empty()) {
    // inner solve set-up per system (solve_inner)
    for (int j : active) {
      Sys &s = S[j];
      const double r2 = s.r2e + s.r2o, rq = s.r2stop / r2;
      s.pl = eo_plan(rq * r2, s.r2e, s.r2o, s.m);
      s.n = 0;
      s.src = s.r;
      if (s.pl.kind == EO_LEFT) {
        s.src = s.d;
        CHK(op_D(c, *s.d, *s.r, s.m, -1.0));
        CHK(blas_norm2(c, *s.d, 0, &c->dscal[2]));
        double d2e;
        CHK(read_scalars(c, &c->dscal[2], 1, &d2e));
        s.pl.rr = eo_left_target(rq, r2, s.m, d2e);
      }
    }
    for (int par = 1; par >= 0; par--) {
      DevField *xs[QX_MAXRHS], *bs[QX_MAXRHS];
      double ms[QX_MAXRHS], rrs[QX_MAXRHS];
      int idx[QX_MAXRHS], its[QX_MAXRHS], nup[QX_MAXRHS] = {0, 0, 0, 0}, k = 0, mx = 0;
      for (int j : active)
        if (S[j].pl.par == par) {
          xs[k] = S[j].y; bs[k] = S[j].src; ms[k] = S[j].m; rrs[k] = S[j].pl.rr; idx[k] = j;
          mx = std::max(mx, maxits - S[j].its);
          k++;
        }
      if (!k) continue;
      // systems of one group share maxits: the remaining budget of the one that has used least
      // (the sloppy batches report per system through c->slpb_last.map: system of this call <- system of the inner batch)
      int outer[QX_MAXRHS];
      for (int i = 0; i < QX_MAXRHS; i++) outer[i] = c->slpb_last.map[i];
      for (int i = 0; i < k; i++) c->slpb_last.map[i] = outer[idx[i]];
      int rc = 0;
      if (defl && nev > 0) rc = solve_xx_batch_deflated_dev(c, *defl, nev, k, xs, bs, ms, rrs, mx, par, sloppy, its, nullptr, nup);
      else if (sloppy) rc = solve_xx_batch_sloppy_any(c, sloppy, k, xs, bs, ms, rrs, mx, par, its, nullptr, nup);
      else rc = solve_xx_batch_dev(c, k, xs, bs, ms, rrs, mx, par, its, nullptr);
      for (int i = 0; i < QX_MAXRHS; i++) c->slpb_last.map[i] = outer[i];
      CHK(rc);
      for (int i = 0; i < k; i++) {
        S[idx[i]].n = its[i];
        if (nupdates) nupdates[idx[i]] += nup[i];
      }
    }
    std::vector<int> next;
    for (int j : active) {
      Sys &s = S[j];
      if (s.pl.par >= 0) {
        if (s.pl.kind == EO_RIGHT) {
          CHK(blas_scale(c, 4.0, *s.y, s.pl.par ? 0 : 1));
          CHK(blas_copy(c, *s.d, *s.y, 2));
          CHK(op_D(c, *s.y, *s.d, s.m, -1.0));
        } else {
          CHK(blas_scale(c, 4.0, *s.y, 0));
          CHK(op_eo_reconstruct_pub(c, *s.y, *s.r, s.m));
        }
      } else {
        CHK(blas_zero(c, *s.y, 2));
      }
      s.its += s.n;
      CHK(blas_axpy(c, 1.0, *s.y, *s.x, 2));
      CHK(resid_eo(c, *s.r, *s.b, *s.x, s.m, &s.r2e, &s.r2o));
      if (s.r2e + s.r2o > s.r2stop && s.its < maxits && s.pl.par >= 0) next.push_back(j);
    }
    active.swap(next);
  }
  for (int j = 0; j < n; j++) {
    if (iters) iters[j] = S[j].its;
    if (r2_final) r2_final[j] = (S[j].b2 != 0.0) ? (S[j].r2e + S[j].r2o) / S[j].b2 : 0.0;
  }
  return 0;
}

int solve_full_batch_dev(qexhip_ctx *c, int n, DevField **x, DevField **b, const double *mass, const double *r2req,
                         int maxits, int *iters, double *r2_final) {
  return solve_full_batch_impl(c, n, x, b, mass, r2req, maxits, iters, r2_final, 0, nullptr);
}
// n x Staggered.solve with the mixed-precision inner batch: the same ReconR / ReconL decisions and true-residual outer loop per system
int solve_full_batch_sloppy_dev(qexhip_ctx *c, int n, DevField **x, DevField **b, const double *mass, const double *r2req,
                                int maxits, int sloppy, int *iters, double *r2_final, int *nupdates) {
  if (!sloppy) {
    if (nupdates) for (int j = 0; j < n && j < QX_MAXRHS; j++) nupdates[j] = 0;
    return solve_full_batch_dev(c, n, x, b, mass, r2req, maxits, iters, r2_final);
  }
  CHK(batch_sloppy_check(c, n, mass));
  return solve_full_batch_impl(c, n, x, b, mass, r2req, maxits, iters, r2_final, sloppy, nupdates);
}
// the same with the inner batches deflated from the even basis B; nev = 0 is solve_full_batch_sloppy_dev
int solve_full_batch_deflated_dev(qexhip_ctx *c, EigBasis &B, int nev, int n, DevField **x, DevField **b, const double *mass,
                                  const double *r2req, int maxits, int sloppy, int *iters, double *r2_final, int *nupdates) {
  if (nev == 0) return solve_full_batch_sloppy_dev(c, n, x, b, mass, r2req, maxits, sloppy, iters, r2_final, nupdates);
  if (n < 1 || n > QX_MAXRHS) { qexhip_set_error("batch solve: 1 <= n <= %d", QX_MAXRHS); return -1; }
  if (nev < 0 || nev > B.nvecs) { qexhip_set_error("deflated solve: nev = %d of a basis of %d vectors", nev, B.nvecs); return -1; }
  if (B.gen != c->links_gen) { qexhip_set_error("deflated solve: the basis was computed on other links"); return -3; }
  if (sloppy) CHK(batch_sloppy_check(c, n, mass));
  return solve_full_batch_impl(c, n, x, b, mass, r2req, maxits, iters, r2_final, sloppy, nupdates, &B, nev);
}

// the first `count` (<= 4 per system) CG work fields of the batch state, for the mixed-precision batch (which leaves the fp64 CG's idle)
int batch_work_fields(qexhip_ctx *c, int count, DevField **out) {
  if (count < 0 || count > 4 * QX_MAXRHS) { qexhip_set_error("batch_work_fields: count"); return -1; }
  BatchState *B;
  CHK(batch_state(c, 4 * QX_MAXRHS, &B));        // (callers that hold pointers into B->f have grown it past this already)
  for (int i = 0; i < count; i++) out[i] = &B->f[i];
  return 0;
}

// device fields for the systems' sources and solutions (slots of the batch state)
int batch_io_fields(qexhip_ctx *c, int n, DevField **xs, DevField **bs) {
  if (n < 1 || n > QX_MAXRHS) { qexhip_set_error("batch solve: 1 <= n <= %d", QX_MAXRHS); return -1; }
  BatchState *B;
  CHK(batch_state(c, 9 * QX_MAXRHS, &B));        // 4 CG fields + r, y, d + x, b per system
  for (int j = 0; j < n; j++) { xs[j] = &B->f[7 * QX_MAXRHS + 2 * j]; bs[j] = &B->f[7 * QX_MAXRHS + 2 * j + 1]; }
  return 0;
}
