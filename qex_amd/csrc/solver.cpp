// solver.cpp -- host control flow of the operator compositions and solvers, device resident.
//
// Restates (file:line in ctpeterson/qex):
//   stagD / D / Ddag / eoReconstruct   src/physics/stagD.nim:406-409,566-586
//   stagD2ee / stagD2oo                src/physics/stagD.nim:434-469
//   solveXX (solveEE/solveOO)          src/physics/stagSolve.nim:57-138  + CG src/solvers/cg.nim:55-272
//   solveReconR / solveReconL / solve  src/physics/stagSolve.nim:141-294
//   multi-shift solveXX / solve        src/physics/stagSolve.nim:296-446 + src/solvers/cgm.nim:84-315
// All vectors stay in HBM; the CG scalars stay on the device (CgScal) and the host only reads
// the state back once per chunk of iterations.
#include "qexhip_internal.h"
#include "full_solve.h"
#include "../../include/qexhip.h"
#include <cmath>
#include <cstring>
#include <algorithm>
#include <vector>


int get_work(qexhip_ctx *c, int slot, DevField **f) {
  if (slot == WK_R || slot == WK_P || slot == WK_AP) c->cg_resume.valid = 0;     // whoever takes the CG's vectors ends a resumable solve
  if (c->wk[slot] == 0) {
    DevField nf;
    CHK(field_alloc(c, nf));
    int id = -(slot + 1);
    c->fields[id] = nf;
    c->wk[slot] = id;
  }
  *f = &c->fields[c->wk[slot]];
  return 0;
}

// r[px] = 4 m2 x - (2D)(2D) x : stagDP onto the other parity, stagDM back (stagD.nim:434-456)
int op_xx(qexhip_ctx *c, DevField &r, DevField &x, double m2, int par_even, int dot, const int *done, int *ndot) {
  DevField *t;
  CHK(get_work(c, WK_T, &t));
  const int px = par_even ? 0 : 1, py = 1 - px;
  // with deferred partials (the CG loops) the caller's next call is comm_allreduce_parts, which takes the join of the second sweep's
  // boundary launch into its kernel where the sweep is split by sites and the mailboxes carry the sum
  DslashOpts o1, o2;
  o1.done = done;
  o2.cb = 4.0 * m2;
  o2.xs = &x;
  o2.neg = 1;
  o2.dot = (dot && ndot) ? 2 : dot;
  o2.nparts_out = ndot;
  o2.dot_out = &c->cg->pAp;
  o2.done = done;
  o2.defer_join = (dot && ndot) ? 1 : 0;
  o2.pair2 = (t->d != x.d && t->d != r.d) ? 1 : 0;
  if (o2.cb == 0.0 && dot) { qexhip_set_error("op_xx: dot with m2 == 0 unsupported"); return -1; }
  CHK(dslash_sweep(c, *t, x, py, o1));
  CHK(dslash_sweep(c, r, *t, px, o2));
  return 0;
}

// stagD on one parity: r = a*r + m*x + sc*D*x via stagD2(a/(.5sc), m/(.5sc)) then *(.5sc)
static int op_stagD(qexhip_ctx *c, DevField &r, DevField &x, int parity, double m, double sc, double a) {
  DslashOpts o;
  o.ca = a / (0.5 * sc);
  o.cb = m / (0.5 * sc);
  o.rin = &r;
  o.xs = &x;
  o.post = 0.5 * sc;
  return dslash_sweep(c, r, x, parity, o);
}

int op_D(qexhip_ctx *c, DevField &r, DevField &x, double m, double sc, double a) {
  CHK(op_stagD(c, r, x, 0, m, sc, a));
  CHK(op_stagD(c, r, x, 1, m, sc, a));
  return 0;
}

// r.odd = (b.odd - D_oe r.even)/m  (stagD.nim:583-586)
static int op_eo_reconstruct(qexhip_ctx *c, DevField &r, DevField &b, double m) {
  CHK(op_stagD(c, r, r, 1, 0.0, -1.0 / m, 0.0));
  CHK(blas_axpy(c, 1.0 / m, b, r, 1));
  return 0;
}
int op_eo_reconstruct_pub(qexhip_ctx *c, DevField &r, DevField &b, double m) { return op_eo_reconstruct(c, r, b, m); }
int op_stagD_pub(qexhip_ctx *c, DevField &r, DevField &x, int parity, double m, double sc, double a) { return op_stagD(c, r, x, parity, m, sc, a); }
// r.even = (D^+ b).even = (m b - D b).even  (eoReduce, stagD.nim:575-581: one stagD on the even subset with sc = -1)
int op_eo_reduce_pub(qexhip_ctx *c, DevField &r, DevField &b, double m) { return op_stagD(c, r, b, 0, m, -1.0, 0.0); }

static int ensure_hist(qexhip_ctx *c, int cap) {
  if (cap < 1) cap = 1;
  if (c->histcap >= cap) return 0;
  if (c->hist) HIPCHK(hipFree(c->hist));
  c->hist = nullptr; c->histcap = 0;
  HIPCHK(hipMalloc((void **)&c->hist, sizeof(double) * cap));
  c->histcap = cap;
  return 0;
}

static int read_cg(qexhip_ctx *c, CgScal *host) {
  HIPCHK(hipMemcpyAsync(c->pinned, c->cg, sizeof(CgScal), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  memcpy(host, c->pinned, sizeof(CgScal));
  return 0;
}

// The iterations of CgState.solve (cg.nim:174-217) from iteration k on: device state in slot k&1 (`rolled`), r / p / x as the
// previous iteration left them.  Shared by the first call and by the re-entry (cg.nim:133: `if b2<0: # first call`).
static int cg_iterate(qexhip_ctx *c, DevField &x, DevField *r, DevField *p, DevField *Ap, double m2, int par_even, int k,
                      CgScal &st, int *iters, double *r2_over_b2, double *hist, int histcap) {
  const int par = par_even ? 0 : 1;
  const int chunk = 32;
  int rolled = 1;
  bool done = st.dones[k & 1];
  double r2 = st.r2s[k & 1];
  st.itn = st.itns[k & 1];
  // (Round 4 tried forming p = r + beta p inside the first sweep -- every output site builds it for its eight neighbours, one of
  // them stores it -- to drop k_cg_xpay and a launch boundary: the sweep grew by 17 us, the iteration did not move (267.9 vs
  // 267.6 us, profiles/r04_cg_fuse_ab.log), so the separate launch stays.)
  while (!done) {
    int n = std::min(chunk, st.maxits - k);
    if (n <= 0) break;
    for (int i = 0; i < n; i++, k++) {
      CHK(cg_xpay(c, *p, *r, par, k, rolled));                        // cg.nim:186-193 (+ bookkeeping of k-1)
      rolled = 0;
      int ndot = 0;                                                   // <p,Ap> partials are summed inside cg_update
      CHK(op_xx(c, *Ap, *p, m2, par_even, 1, &c->cg->dones[k & 1], &ndot));   // cg.nim:200, qLAp :206
      CHK(cg_update(c, x, *r, *p, *Ap, par, k, ndot));                // cg.nim:208-213
    }
    CHK(cg_close(c, k));
    rolled = 1;
    CHK(read_cg(c, &st));
    CHK(comm_agree_check(c, st));
    done = st.dones[k & 1];
    r2 = st.r2s[k & 1];
    st.itn = st.itns[k & 1];
  }
  st.r2 = r2;
  if (iters) *iters = st.itn;
  if (r2_over_b2) *r2_over_b2 = (st.b2 != 0.0) ? st.r2 / st.b2 : 0.0;
  if (hist && histcap > 0) {
    int n = std::min(std::min(histcap, c->histcap), st.itn + 1);
    HIPCHK(hipMemcpyAsync(hist, c->hist, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  // what a re-entry needs: the same x, the same operator; r, p and the device scalars stay where they are
  c->cg_resume.valid = 1; c->cg_resume.x = x.d; c->cg_resume.par_even = par_even; c->cg_resume.m2 = m2; c->cg_resume.k = st.itn;
  return 0;
}

int solve_xx_dev(qexhip_ctx *c, DevField &x, DevField &b, double mass, double r2req, int maxits,
                 int par_even, int *iters, double *r2_over_b2, double *hist, int histcap) {
  const int par = par_even ? 0 : 1;
  DevField *r, *p, *Ap;
  CHK(get_work(c, WK_R, &r));
  CHK(get_work(c, WK_P, &p));
  CHK(get_work(c, WK_AP, &Ap));
  CHK(ensure_hist(c, std::max(histcap, 1)));
  const double m2 = mass * mass;
  CHK(blas_zero(c, x, 2));                       // threads: r := 0 (stagSolve.nim:63-64)
  CHK(blas_norm2(c, b, par, &c->dscal[0]));      // b2 (cg.nim:134)
  // op.apply(Ap, x) with x = 0 gives Ap = 0 exactly, so r = b - Ap = b and r2 = b2 (cg.nim:145-151)
  CHK(blas_copy(c, *r, b, par));
  CHK(blas_norm2(c, *r, par, &c->dscal[1]));
  CHK(cg_init(c, r2req, maxits));
  CgScal st;
  CHK(read_cg(c, &st));
  return cg_iterate(c, x, r, p, Ap, m2, par_even, 0, st, iters, r2_over_b2, hist, histcap);   // k_cg_init wrote slot 0
}

// Re-entry of CgState.solve with b2 >= 0 (cg.nim:21-27,85,133,155-161,256-261): nothing is set up again; r2stop and maxits are
// taken from the new SolverParams, the iteration count goes on counting, beta of the next iteration uses the kept rzold.
// Valid only directly after a solve_xx_dev / a previous re-entry on the same x and operator.
int solve_xx_continue_dev(qexhip_ctx *c, DevField &x, double r2req, int maxits, int *iters, double *r2_over_b2, double *hist, int histcap) {
  if (!c->cg_resume.valid || c->cg_resume.x != x.d) {
    qexhip_set_error("solve_xx_continue: no resumable CG state for this field (another solver, set_links or a work-vector user ran "
                     "since the last solve_xx on it)");
    return -3;
  }
  const int k = c->cg_resume.k, par_even = c->cg_resume.par_even;
  const double m2 = c->cg_resume.m2;
  DevField *r = &c->fields[c->wk[WK_R]], *p = &c->fields[c->wk[WK_P]], *Ap = &c->fields[c->wk[WK_AP]];
  CHK(cg_resume(c, k, r2req, maxits));
  CgScal st;
  CHK(read_cg(c, &st));
  return cg_iterate(c, x, r, p, Ap, m2, par_even, k, st, iters, r2_over_b2, hist, histcap);
}

// ---- mixed-precision solveXX: CG in fp32 with reliable updates (SolverParams.sloppySolve; QUDA's scheme behind QEX's GPU backend,
// qudaWrapperImpl.nim:194-197, reliable_delta = 0.1 qudaSet.nim:63), the iteration of cg.nim:174-214 ----
// fp64 holds x, b and the true residual r; fp32 holds r_s = r/sigma, p_s, Ap_s and the increment x_s (dslash_f32.hip).  Per fp32
// iteration: p_s = r_s + beta p_s; Ap_s = (4m^2 - D_eo D_oe) p_s (two fp32 sweeps, <p,Ap> in double); x_s += alpha p_s;
// r_s -= alpha Ap_s; |r_s|^2.  A reliable update -- due when |r_s|^2 < delta^2 max|r_s|^2 since the last one, when the fp32 residual
// says converged, or at maxits -- folds x += sigma x_s, recomputes r = b - A x with the fp64 op_xx, and the solve stops only on that
// TRUE residual.  The update's five launches are gated by device flags (k_slp_flush / k_slp_resid / k_slp_rclose test `upd`, the two
// fp64 sweeps read `noupd` as their done word), and the host reads the state once per chunk.  They are posted every
// opt_sloppy_check-th iteration (default 4; always at maxits), so an update waits up to 3 iterations: posted every iteration, the
// gated no-ops (each sweep still dispatches its whole grid, ~4.6 us) cost 7 % of an fp32 iteration at 32^4 -- measured on MI355X,
// 137.9 vs 130.9 us per iteration for every 1st / 4th iteration, 222 vs 224 iterations.
// Sharded: the state every rank just read back decides whether its host posts another chunk, so the ranks must hold the same bits
// (slp_update: the reductions are rank-global, and so are the flags computed from them).  Checked here, with host operands, before
// any rank acts on its copy: {r2t, -r2t, key, -key} max-reduced, max and min must coincide.  stalled: the 16-bit solve's stall flag, which
// decides on every rank whether the fp32 finish -- more collectives -- is entered.
int slp_agree(qexhip_ctx *c, const SlpScal &h, int stalled) {
  if (c->nranks < 2 || !comm_ready(c)) return 0;
  CHK(peer_check(c));
  const double key = (((double)h.k * 2.0 + h.done) * 2.0 + (stalled != 0)) * 65536.0 + (h.nupd & 0xffff);      // (exact in a double)
  double v[4] = {h.r2t, -h.r2t, key, -key};
  CHK(comm_allreduce_max(c, v, 4));
  const bool both_nan = std::isnan(v[0]) && std::isnan(v[1]);
  if ((!both_nan && v[0] != -v[1]) || v[2] != -v[3]) {
    qexhip_set_error("sharded sloppy solve: the ranks disagree on the true residual (%.17g .. %.17g) or on iterations / updates / stop / "
                     "stall (key %g .. %g)", -v[1], v[0], -v[3], v[2]);
    return QEXHIP_ERR_COMM;
  }
  return 0;
}

// ---- SloppyHalf with option "half": the same loop on 16-bit vectors and links (dslash_half.hip) ----
// r_s, p_s, Ap_s are stored in the 16-bit format, the increment x_s stays fp32; the update gating, the chunks and the stop on the
// true fp64 residual are the fp32 solve's, and its fp64 kernels (slp_flush, op_xx, slp_resid) run unchanged.  Stall guard: at a
// light mass cond(A) 2^-15 reaches 1 and the 16-bit recursion can stop improving the true residual; when opt_half_stall reliable
// updates in a row have not lowered it (0: at the first update) the device ends the 16-bit iteration and the solve finishes in
// fp32 -- A e = r with solve_xx_sloppy_dev to r2req |b|^2 / |r|^2, x += e, and the true residual recomputed once.  iters and
// nupdates are the sums.  Sharded: slph_iterate's reductions are rank-global and the stall guard decides from the rank-global true
// residual, so every rank takes the same updates, the same stop and the same stall; the state read back at the end of a chunk, stall
// flag included, is checked with slp_agree before any rank acts on it, and the decision to enter half_finish_f32 (itself sharded
// through solve_xx_sloppy_dev) is taken from that agreed state alone: all ranks enter it or none does.
//
// The one loop of both storages.  HALF: 16-bit storage -- slph_iterate for slp_iterate, the stall guard behind every posted update, its
// flag read back with the state, the fp32 finish, and the report to c->slp_last (the fp32 solve's callers report for it).  The finish
// re-enters this loop as solve_xx_sloppy_dev on the same context, same SlpScal and pinned scratch: what the loop holds on the host
// (h, stalled) is local and final by then.
template <bool HALF>
static int solve_xx_lowp(qexhip_ctx *c, DevField &x, DevField &b, double mass, double r2req, int maxits, int par_even,
                         int *iters, double *r2_over_b2, int *nupdates) {
  const int par = par_even ? 0 : 1;
  const double m2 = mass * mass;
  if (m2 == 0.0) { qexhip_set_error("sloppy solve: mass 0 unsupported (op_xx's <p,Ap> needs 4 m^2 > 0)"); return -1; }
  DevField *r, *Ax;
  CHK(get_work(c, WK_R, &r));
  CHK(get_work(c, WK_AP, &Ax));
  DevFieldF *xs;
  CHK(f32_field(c, F32_X, &xs));
  SlpScal *s;
  CHK(slp_alloc(c, &s));
  CHK(blas_zero(c, x, 2));                       // (as solve_xx_dev)
  CHK(blas_norm2(c, b, par, &c->dscal[0]));
  CHK(blas_copy(c, *r, b, par));
  HIPCHK(hipMemsetAsync(xs->par(par), 0, xs->half * sizeof(float2), c->stream));
  CHK(slp_init(c, s, r2req, maxits));
  if constexpr (HALF) CHK(slph_begin(c, s));     // (sharded: collective where the 16-bit links are rebuilt)
  SlpScal h;
  int stalled = 0;
  int *const pstall = (int *)((char *)c->pinned + 256);     // (behind the SlpScal)
  static_assert(sizeof(SlpScal) <= 256, "pinned scratch layout");
  auto read_state = [&]() -> int {
    HIPCHK(hipMemcpyAsync(c->pinned, s, sizeof(SlpScal), hipMemcpyDeviceToHost, c->stream));
    if constexpr (HALF) CHK(slph_stalled_async(c, pstall));
    HIPCHK(hipStreamSynchronize(c->stream));
    memcpy(&h, c->pinned, sizeof(SlpScal));
    if constexpr (HALF) stalled = *pstall;
    return 0;
  };
  CHK(read_state());
  const int every = std::max(1, c->opt_sloppy_check);
  const int chunk = 32;
  int k = 0;
  while (!h.done && k < maxits) {
    const int n = std::min(chunk, maxits - k);
    for (int i = 0; i < n; i++, k++) {
      CHK((HALF ? slph_iterate : slp_iterate)(c, s, *xs, *r, m2, par_even));
      if ((k + 1) % every == 0 || k + 1 >= maxits) {
        CHK(slp_flush(c, s, x, *xs, par));
        CHK(op_xx(c, *Ax, x, m2, par_even, 0, &s->noupd));
        CHK(slp_resid(c, s, *r, b, *Ax, par));
        if constexpr (HALF) CHK(slph_stall(c, s, c->opt_half_stall));
      }
    }
    CHK(read_state());
    CHK(slp_agree(c, h, stalled));
  }
  int its = h.k, nupd = h.nupd;
  double r2t = h.r2t;
  if constexpr (HALF) {
    int its32 = 0;
    if (stalled && r2t > h.r2stop && its < maxits) {
      // (x holds every increment: the update that tripped the guard flushed x_s; r is its true residual)
      int nu32 = 0;
      CHK(half_finish_f32(c, x, b, *r, *Ax, mass, h.r2stop, maxits - its, par_even, &r2t, &its32, &nu32));
      nupd += nu32;
      c->slp_last.fell_back = 1;
    }
    c->slp_last.precision = 2;
    c->slp_last.half_iters += its;
    c->slp_last.f32_iters += its32;
    its += its32;
  }
  if (iters) *iters = its;
  if (r2_over_b2) *r2_over_b2 = (h.b2 != 0.0) ? r2t / h.b2 : 0.0;
  if (nupdates) *nupdates = nupd;
  return 0;
}

// (the fp32 links before anything else, the mass-0 refusal included, as this entry always had them)
int solve_xx_sloppy_dev(qexhip_ctx *c, DevField &x, DevField &b, double mass, double r2req, int maxits, int par_even,
                        int *iters, double *r2_over_b2, int *nupdates) {
  CHK(f32_links(c, nullptr, nullptr));
  return solve_xx_lowp<false>(c, x, b, mass, r2req, maxits, par_even, iters, r2_over_b2, nupdates);
}
int solve_xx_half_dev(qexhip_ctx *c, DevField &x, DevField &b, double mass, double r2req, int maxits, int par_even,
                      int *iters, double *r2_over_b2, int *nupdates) {
  return solve_xx_lowp<true>(c, x, b, mass, r2req, maxits, par_even, iters, r2_over_b2, nupdates);
}

// the fp32 finish of a 16-bit solve whose stall guard tripped, for solve_xx_half_dev above and for every stalled system of the 16-bit batch
// (batch_half.hip): r is the true residual of x; A e = r with solve_xx_sloppy_dev to r2stop / *r2t, x += e, *r2t recomputed once
int half_finish_f32(qexhip_ctx *c, DevField &x, DevField &b, const DevField &r, DevField &Ax, double mass, double r2stop, int maxits,
                    int par_even, double *r2t, int *its32, int *nupd32) {
  const int par = par_even ? 0 : 1;
  DevField *e, *rc;
  CHK(pool_field(c, POOL_REF, &e));
  CHK(pool_field(c, POOL_REF + 4, &rc));
  CHK(blas_copy(c, *rc, r, par));
  CHK(solve_xx_sloppy_dev(c, *e, *rc, mass, r2stop / *r2t, maxits, par_even, its32, nullptr, nupd32));
  CHK(blas_axpy(c, 1.0, *e, x, par));
  CHK(op_xx(c, Ax, x, mass * mass, par_even, 0, nullptr));
  CHK(blas_axpby(c, 1.0, b, -1.0, Ax, *rc, par));
  CHK(blas_norm2(c, *rc, par, &c->dscal[1]));
  return read_scalars(c, &c->dscal[1], 1, r2t);
}

int solve_xx_sloppy_any(qexhip_ctx *c, int sloppy, DevField &x, DevField &b, double mass, double r2req, int maxits, int par_even,
                        int *iters, double *r2_over_b2, int *nupdates) {
  if (sloppy == 2 && c->opt_half)
    return solve_xx_half_dev(c, x, b, mass, r2req, maxits, par_even, iters, r2_over_b2, nupdates);
  int its = 0;
  CHK(solve_xx_sloppy_dev(c, x, b, mass, r2req, maxits, par_even, &its, r2_over_b2, nupdates));
  if (c->slp_last.precision == 0) c->slp_last.precision = 1;
  c->slp_last.f32_iters += its;
  if (iters) *iters = its;
  return 0;
}

// ---- mixed-precision multi-shift solveXX (QUDA's scheme: fp32 multi-shift iterations, then per-shift refinement) ----
// Phase 1: the multi-shift CG of solve_xx_multi_dev with every iterated vector in fp32 (multishift_f32.hip) and reliable updates on the
// BASE system: gated on device flags and posted every opt_sloppy_check-th iteration and at maxits like the single solve's; one launch
// flushes all shifts, the fp64 op_xx runs on x_0 alone, and the base system's true residual decides the stop.  After a residual
// replacement the shifted residuals are no longer exactly zeta_k r -- expected, and the reason for
// Phase 2: for every k >= 1 the true r_k = b - A_k x_k (fp64 op_xx; A_k = A_0 + sg[k], i.e. op_xx at m_k^2 = m^2 + sg[k]/4); a shift
// with |r_k|^2 > r2req |b|^2 is refined -- A_k d = r_k to r2req |b|^2 / |r_k|^2 with the sloppy CG, x_k += d -- and |r_k|^2 recomputed
// once: the value reported.  One rank without ghost zones: lock-step batches of up to four shifts (solve_xx_batch_sloppy_dev: each
// system returns the bits it returns alone); with ghost zones or more ranks, where the batch is refused, solve_xx_sloppy_dev one
// shift at a time.  Sharded: every reduction is rank-global (msf_iterate, slp_resid, blas_norm2), so every rank takes the same
// updates, the same stop and the same refinement decisions; slp_agree checks it at the end of every 32-iteration chunk.
int multi_sloppy_check(qexhip_ctx *c, int sloppy, const double *vals, int nmass) {
  if (sloppy < 0 || sloppy > 2) {
    qexhip_set_error("sloppy = %d: 0 (SloppyNone, fp64), 1 (SloppySingle) or 2 (SloppyHalf, runs single)", sloppy);
    return QEXHIP_ERR_ARG;
  }
  if (nmass < 1 || nmass > CGM_MAXM) { qexhip_set_error("multishift: 1 <= nmass <= %d (nmass = %d)", CGM_MAXM, nmass); return QEXHIP_ERR_ARG; }
  if (sloppy && vals[0] == 0.0) {
    qexhip_set_error("sloppy multi-shift solve: base mass 0 unsupported (op_xx's <p,Ap> needs 4 m^2 > 0)");
    return QEXHIP_ERR_ARG;
  }
  return 0;
}

int solve_xx_multi_sloppy_dev(qexhip_ctx *c, std::vector<DevField *> &xs, DevField &b, const double *shifts, int nmass, double r2req,
                              int maxits, int par_even, int *iters, double *r2_over_b2, int *nupdates, int *refine_iters) {
  CHK(multi_sloppy_check(c, 1, shifts, nmass));
  const int par = par_even ? 0 : 1;
  DevField *r, *Ax;
  CHK(get_work(c, WK_R, &r));
  CHK(get_work(c, WK_AP, &Ax));
  CHK(f32_links(c, nullptr, nullptr));
  DevFieldF *rs, *aps, *ps0;
  CHK(f32_field(c, F32_R, &rs));
  CHK(f32_field(c, F32_AP, &aps));
  SlpScal *s;
  CHK(slp_alloc(c, &s));
  const double m2 = shifts[0] * shifts[0];
  for (int k = 0; k < nmass; k++) CHK(blas_zero(c, *xs[k], 2));
  CHK(blas_norm2(c, b, par, &c->dscal[0]));
  CHK(blas_copy(c, *r, b, par));
  CHK(slp_init(c, s, r2req, maxits));
  CHK(msf_start(c, s, *rs, b, xs, shifts, nmass, par, &ps0));
  SlpScal h;
  auto read_state = [&]() -> int {
    HIPCHK(hipMemcpyAsync(c->pinned, s, sizeof(SlpScal), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    memcpy(&h, c->pinned, sizeof(SlpScal));
    return 0;
  };
  CHK(read_state());
  const int every = std::max(1, c->opt_sloppy_check);
  int k = 0;
  {
    ScopedTimer tm(c, "multi_phase1", c->stream);       // (timers on: the stream time of the whole phase, host read-backs included)
    while (!h.done && k < maxits) {
      const int n = std::min(32, maxits - k);
      for (int i = 0; i < n; i++, k++) {
        int ndot = 0;
        CHK(f32_op_xx(c, *aps, *ps0, m2, par_even, 1, &s->done, &ndot));
        CHK(msf_iterate(c, s, *rs, *aps, *r, par, ndot));
        if ((k + 1) % every == 0 || k + 1 >= maxits) {
          CHK(msf_flush(c, s, nmass));
          CHK(op_xx(c, *Ax, *xs[0], m2, par_even, 0, &s->noupd));
          CHK(slp_resid(c, s, *r, b, *Ax, par));
        }
      }
      CHK(read_state());
      CHK(slp_agree(c, h));
    }
  }
  if (iters) *iters = h.k;
  if (nupdates) *nupdates = h.nupd;
  if (refine_iters) for (int j = 0; j < nmass; j++) refine_iters[j] = 0;
  const double b2 = h.b2;
  if (r2_over_b2) {
    r2_over_b2[0] = (b2 != 0.0) ? h.r2t / b2 : 0.0;
    for (int j = 1; j < nmass; j++) r2_over_b2[j] = 0.0;
  }
  if (b2 == 0.0 || nmass == 1) return 0;
  // ---- phase 2 ----
  const bool batched = c->nranks == 1 && !c->g.halo;
  double *dr2;
  CHK(msf_r2_buffer(c, &dr2));
  DevField *d[4], *rk[4];
  for (int j = 0; j < 4; j++) {
    CHK(pool_field(c, POOL_REF + j, &d[j]));
    CHK(pool_field(c, POOL_REF + 4 + j, &rk[j]));
  }
  const double r2stop = r2req * b2;
  ScopedTimer tm2(c, "multi_phase2", c->stream);
  auto resid = [&](int kk, double mk, DevField &out, double *dev) -> int {     // out = b - A_k x_k, |out|^2 (rank-global) -> *dev
    CHK(op_xx(c, *Ax, *xs[kk], mk * mk, par_even, 0, nullptr));
    CHK(blas_axpby(c, 1.0, b, -1.0, *Ax, out, par));
    return blas_norm2(c, out, par, dev);
  };
  for (int k0 = 1; k0 < nmass; k0 += 4) {
    const int ng = std::min(4, nmass - k0);
    double mk[4], r2k[4];
    for (int j = 0; j < ng; j++) {
      mk[j] = sqrt(m2 + 0.25 * shifts[k0 + j]);
      CHK(resid(k0 + j, mk[j], *rk[j], &dr2[j]));
    }
    CHK(read_scalars(c, dr2, ng, r2k));
    int sel[4], ns = 0;
    for (int j = 0; j < ng; j++) if (r2k[j] > r2stop) sel[ns++] = j;
    if (ns > 0) {
      DevField *dx[4], *db[4];
      double mm[4], rq[4];
      int its[4] = {0, 0, 0, 0};
      for (int q = 0; q < ns; q++) { dx[q] = d[sel[q]]; db[q] = rk[sel[q]]; mm[q] = mk[sel[q]]; rq[q] = r2stop / r2k[sel[q]]; }
      if (batched) {
        CHK(solve_xx_batch_sloppy_dev(c, ns, dx, db, mm, rq, maxits, par_even, its, nullptr, nullptr));
      } else {
        for (int q = 0; q < ns; q++) CHK(solve_xx_sloppy_dev(c, *dx[q], *db[q], mm[q], rq[q], maxits, par_even, &its[q], nullptr, nullptr));
      }
      for (int q = 0; q < ns; q++) {
        const int j = sel[q];
        CHK(blas_axpy(c, 1.0, *dx[q], *xs[k0 + j], par));
        if (refine_iters) refine_iters[k0 + j] = its[q];
        CHK(resid(k0 + j, mk[j], *rk[j], &dr2[j]));       // (Ax: solve_xx_sloppy_dev's work vector too, free again here)
      }
      CHK(read_scalars(c, dr2, ng, r2k));
    }
    if (r2_over_b2) for (int j = 0; j < ng; j++) r2_over_b2[k0 + j] = r2k[j] / b2;
  }
  return 0;
}

// ---- deflated solveXX (src/eigens/hisqev.nim:653-705, `rsolve` of its main program) ----
// With low modes (v_i, lambda_i) of H = -D_eo D_oe on the even sites, A = 4 (m^2 + H):
//   1. x0 = sum_i v_i <v_i, b> / (4 (lambda_i + m^2))               block dot + block axpy (eig.hip)
//   2. r0 = b - A x0                                                   fp64
//   3. A d = r0 to r2req |b|^2 / |r0|^2                                the EXISTING fp64 / mixed-precision CG
//   4. x = x0 + d;  r2_over_b2 = the true |b - A x|^2 / |b|^2
// nev = 0 is the undeflated solver itself (same bits, same iteration count).
int solve_xx_deflated_dev(qexhip_ctx *c, EigBasis &B, int nev, DevField &x, DevField &b, double mass, double r2req, int maxits,
                          int sloppy, int *iters, double *r2_over_b2) {
  if (nev < 0 || nev > B.nvecs) { qexhip_set_error("deflated solve: nev = %d of a basis of %d vectors", nev, B.nvecs); return QEXHIP_ERR_ARG; }
  if (B.gen != c->links_gen) {
    qexhip_set_error("deflated solve: the basis was computed on other links (the operator's links changed since)");
    return QEXHIP_ERR_STATE;
  }
  if (nev == 0) {
    if (!sloppy) return solve_xx_dev(c, x, b, mass, r2req, maxits, 1, iters, r2_over_b2, nullptr, 0);
    return solve_xx_sloppy_any(c, sloppy, x, b, mass, r2req, maxits, 1, iters, r2_over_b2, nullptr);
  }
  const double m2 = mass * mass;
  CHK(eig_rayleigh(c, B, nev));
  double2 *dots, *coef;
  CHK(eig_coef_buffers(c, &dots, &coef));
  DevField *r0, *d, *Ax;
  CHK(eig_field(c, EIG_R0, &r0));
  CHK(eig_field(c, EIG_D, &d));
  CHK(eig_field(c, EIG_AP, &Ax));
  std::vector<double2> h(nev);
  CHK(eig_block_dot(c, B, 0, nev, b, dots));
  HIPCHK(hipMemcpyAsync(h.data(), dots, sizeof(double2) * nev, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int i = 0; i < nev; i++) {
    const double s = 0.25 / (B.evals[i] + m2);
    h[i].x *= s; h[i].y *= s;
  }
  HIPCHK(hipMemcpyAsync(coef, h.data(), sizeof(double2) * nev, hipMemcpyHostToDevice, c->stream));
  CHK(blas_zero(c, x, 2));
  CHK(eig_block_axpy(c, B, 0, nev, coef, 1.0, x));
  HIPCHK(hipStreamSynchronize(c->stream));              // (h is read by the copy above)
  CHK(op_xx(c, *Ax, x, m2, 1, 0, nullptr));
  CHK(blas_axpby(c, 1.0, b, -1.0, *Ax, *r0, 0));
  CHK(blas_norm2(c, b, 0, &c->dscal[2]));
  CHK(blas_norm2(c, *r0, 0, &c->dscal[3]));
  double n[2];
  CHK(read_scalars(c, &c->dscal[2], 2, n));
  const double b2 = n[0];
  int its = 0;
  if (b2 > 0 && n[1] > r2req * b2) {
    const double rq = r2req * b2 / n[1];
    if (!sloppy) CHK(solve_xx_dev(c, *d, *r0, mass, rq, maxits, 1, &its, nullptr, nullptr, 0));
    else CHK(solve_xx_sloppy_any(c, sloppy, *d, *r0, mass, rq, maxits, 1, &its, nullptr, nullptr));
    CHK(blas_axpy(c, 1.0, *d, x, 0));
    CHK(op_xx(c, *Ax, x, m2, 1, 0, nullptr));
    CHK(blas_axpby(c, 1.0, b, -1.0, *Ax, *r0, 0));
    CHK(blas_norm2(c, *r0, 0, &c->dscal[3]));
    CHK(read_scalars(c, &c->dscal[3], 1, &n[1]));
  }
  if (iters) *iters = its;
  if (r2_over_b2) *r2_over_b2 = b2 != 0.0 ? n[1] / b2 : 0.0;
  return 0;
}

// ---- the deflated lock-step batch: n <= 4 solveXX's with their own masses, of either parity, from the EVEN basis ----
// D is anti-Hermitian, so H_e = -D_eo D_oe = D_oe^+ D_oe and H_o = D_oe D_oe^+: an even pair (v_i, lambda_i), lambda_i > 0, gives the
// odd pair (D_oe v_i / sqrt(lambda_i), lambda_i), and with A_o = 4 (m^2 + H_o)
//   x0.odd = D_oe V diag(1 / (4 lambda_i (lambda_i + m^2))) V^+ (-D_eo b.odd)
// -- two single-parity sweeps per system around the same block dot / block axpy, no second basis.  The steps are those of
// solve_xx_deflated_dev; the projections of all systems are ONE multi-right-hand-side block dot and ONE block axpy (eig.hip), the
// systems that are not finished by the projection run as ONE lock-step batch CG on A d_k = r0_k.
int solve_xx_batch_deflated_dev(qexhip_ctx *c, EigBasis &B, int nev, int n, DevField **x, DevField **b, const double *mass,
                                const double *r2req, int maxits, int par_even, int sloppy, int *iters, double *r2_over_b2, int *nupdates) {
  if (n < 1 || n > EIG_MAXRHS) { qexhip_set_error("batch solve: 1 <= n <= %d", EIG_MAXRHS); return QEXHIP_ERR_ARG; }
  if (nev < 0 || nev > B.nvecs) { qexhip_set_error("deflated solve: nev = %d of a basis of %d vectors", nev, B.nvecs); return QEXHIP_ERR_ARG; }
  if (sloppy) CHK(batch_sloppy_check(c, n, mass));
  for (int k = 0; k < n; k++) if (mass[k] == 0.0) { qexhip_set_error("batch solve: mass must be non-zero"); return QEXHIP_ERR_ARG; }
  if (B.gen != c->links_gen) {
    qexhip_set_error("deflated solve: the basis was computed on other links (the operator's links changed since)");
    return QEXHIP_ERR_STATE;
  }
  if (nupdates) for (int k = 0; k < n; k++) nupdates[k] = 0;
  if (nev == 0) {
    if (!sloppy) return solve_xx_batch_dev(c, n, x, b, mass, r2req, maxits, par_even, iters, r2_over_b2);
    return solve_xx_batch_sloppy_any(c, sloppy, n, x, b, mass, r2req, maxits, par_even, iters, r2_over_b2, nupdates);
  }
  const int par = par_even ? 0 : 1;
  CHK(eig_rayleigh(c, B, nev));
  double2 *dots, *coef;
  CHK(eig_coef_buffers(c, &dots, &coef));
  DevField *Ax, *r0[EIG_MAXRHS], *d[EIG_MAXRHS], *z[EIG_MAXRHS], *w[EIG_MAXRHS];
  CHK(eig_field(c, EIG_AP, &Ax));
  for (int k = 0; k < n; k++) {
    CHK(eig_field(c, EIG_BR0 + k, &r0[k]));
    CHK(eig_field(c, EIG_BD + k, &d[k]));
    if (!par_even) CHK(eig_field(c, EIG_BZ + k, &z[k]));
    w[k] = b[k];
    if (!par_even) {
      CHK(op_stagD_pub(c, *z[k], *b[k], 0, 0.0, -1.0, 0.0));      // z_k.even = -D_eo b_k.odd (the sweep's 2D halved by stagD)
      w[k] = z[k];
    }
  }
  std::vector<double2> h((size_t)n * nev);
  CHK(eig_block_dot_mrhs(c, B, 0, nev, n, w, dots));
  HIPCHK(hipMemcpyAsync(h.data(), dots, sizeof(double2) * h.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int k = 0; k < n; k++) {
    const double m2 = mass[k] * mass[k];
    for (int i = 0; i < nev; i++) {
      const double lam = B.evals[i];
      double s = 0.25 / (lam + m2);
      if (!par_even) s = lam > 0 ? s / lam : 0.0;
      h[(size_t)k * nev + i].x *= s; h[(size_t)k * nev + i].y *= s;
    }
  }
  HIPCHK(hipMemcpyAsync(coef, h.data(), sizeof(double2) * h.size(), hipMemcpyHostToDevice, c->stream));
  for (int k = 0; k < n; k++) {
    CHK(blas_zero(c, *x[k], 2));
    if (!par_even) CHK(blas_zero(c, *z[k], 0));
  }
  CHK(eig_block_axpy_mrhs(c, B, 0, nev, n, coef, 1.0, par_even ? x : z));
  HIPCHK(hipStreamSynchronize(c->stream));              // (h is read by the copy above)
  double b2[EIG_MAXRHS], r2[EIG_MAXRHS];
  auto resid = [&](int k) -> int {                      // r0_k = b_k - A x_k in fp64, |r0_k|^2 -> dscal[3]
    CHK(op_xx(c, *Ax, *x[k], mass[k] * mass[k], par_even, 0, nullptr));
    CHK(blas_axpby(c, 1.0, *b[k], -1.0, *Ax, *r0[k], par));
    return blas_norm2(c, *r0[k], par, &c->dscal[3]);
  };
  for (int k = 0; k < n; k++) {
    if (!par_even) CHK(op_stagD_pub(c, *x[k], *z[k], 1, 0.0, 1.0, 0.0));     // x_k.odd = D_oe z_k
    CHK(blas_norm2(c, *b[k], par, &c->dscal[2]));
    CHK(resid(k));
    double nn[2];
    CHK(read_scalars(c, &c->dscal[2], 2, nn));
    b2[k] = nn[0]; r2[k] = nn[1];
  }
  DevField *dx[EIG_MAXRHS], *db[EIG_MAXRHS];
  double mm[EIG_MAXRHS], rq[EIG_MAXRHS];
  int sel[EIG_MAXRHS], its[EIG_MAXRHS] = {0, 0, 0, 0}, nup[EIG_MAXRHS] = {0, 0, 0, 0}, ns = 0;
  for (int k = 0; k < n; k++)
    if (b2[k] > 0 && r2[k] > r2req[k] * b2[k]) {
      dx[ns] = d[k]; db[ns] = r0[k]; mm[ns] = mass[k]; rq[ns] = r2req[k] * b2[k] / r2[k]; sel[ns] = k;
      ns++;
    }
  if (ns > 0) {
    if (!sloppy) CHK(solve_xx_batch_dev(c, ns, dx, db, mm, rq, maxits, par_even, its, nullptr));
    else {
      int outer[EIG_MAXRHS];
      for (int q = 0; q < EIG_MAXRHS; q++) outer[q] = c->slpb_last.map[q];
      for (int q = 0; q < ns; q++) c->slpb_last.map[q] = outer[sel[q]];
      const int rc = solve_xx_batch_sloppy_any(c, sloppy, ns, dx, db, mm, rq, maxits, par_even, its, nullptr, nup);
      for (int q = 0; q < EIG_MAXRHS; q++) c->slpb_last.map[q] = outer[q];
      CHK(rc);
    }
    for (int q = 0; q < ns; q++) {
      const int k = sel[q];
      CHK(blas_axpy(c, 1.0, *dx[q], *x[k], par));
      CHK(resid(k));
      CHK(read_scalars(c, &c->dscal[3], 1, &r2[k]));
    }
  }
  for (int k = 0; k < n; k++) {
    if (iters) iters[k] = 0;
    if (r2_over_b2) r2_over_b2[k] = b2[k] != 0.0 ? r2[k] / b2[k] : 0.0;
  }
  for (int q = 0; q < ns; q++) {
    if (iters) iters[sel[q]] = its[q];
    if (nupdates) nupdates[sel[q]] = nup[q];
  }
  return 0;
}

// the inner solveXX of the full solve: fp64 CG, or the mixed-precision one (sloppy > 0); even-parity solves deflate with the basis a
// deflated full solve has set
static int inner_xx(qexhip_ctx *c, DevField &x, DevField &b, double m, double r2req, int maxits, int par_even, int *its,
                    int sloppy, int *nupd) {
  if (par_even && c->deflate_nev > 0) {
    EigBasis *B;
    CHK(eig_basis_find(c, c->deflate_basis, &B));
    return solve_xx_deflated_dev(c, *B, c->deflate_nev, x, b, m, r2req, maxits, sloppy, its, nullptr);
  }
  if (!sloppy) return solve_xx_dev(c, x, b, m, r2req, maxits, par_even, its, nullptr, nullptr, 0);
  int nu = 0;
  CHK(solve_xx_sloppy_any(c, sloppy, x, b, m, r2req, maxits, par_even, its, nullptr, &nu));
  *nupd += nu;
  return 0;
}

// ---- full solve (stagSolve.nim:141-294); the decisions are full_solve.h's ----
int norm2_eo(qexhip_ctx *c, DevField &f, double *e, double *o) {
  CHK(blas_norm2(c, f, 0, &c->dscal[2]));
  CHK(blas_norm2(c, f, 1, &c->dscal[3]));
  double h[2];
  CHK(read_scalars(c, &c->dscal[2], 2, h));
  *e = h[0]; *o = h[1];
  return 0;
}
// r = b - D x at mass m with its two parity norms: the true residual every outer loop of a full solve stops on
int resid_eo(qexhip_ctx *c, DevField &r, DevField &b, DevField &x, double m, double *e, double *o) {
  CHK(op_D(c, r, x, m, 1.0));
  CHK(blas_axpby(c, 1.0, b, -1.0, r, r, 2));       // r := b - r
  return norm2_eo(c, r, e, o);
}

static int solve_inner(qexhip_ctx *c, DevField &x, DevField &b, double m, double r2req, int maxits,
                       double b2e, double b2o, int *its, int sloppy, int *nupd) {
  const double b2 = b2e + b2o;
  const EoPlan pl = eo_plan(r2req * b2, b2e, b2o, m);
  *its = 0;
  DevField *w;                                      // ReconR: the inner solution y; ReconL: the inner source d
  CHK(get_work(c, WK_D, &w));
  if (pl.kind == EO_RIGHT) {
    if (pl.par >= 0) {
      CHK(inner_xx(c, *w, b, m, pl.rr, maxits, pl.par, its, sloppy, nupd));
      CHK(blas_scale(c, 4.0, *w, pl.par ? 0 : 1));
      CHK(op_D(c, x, *w, m, -1.0));
    }
  } else {
    CHK(op_D(c, *w, b, m, -1.0));
    CHK(blas_norm2(c, *w, 0, &c->dscal[2]));
    double d2e;
    CHK(read_scalars(c, &c->dscal[2], 1, &d2e));
    CHK(inner_xx(c, x, *w, m, eo_left_target(r2req, b2, m, d2e), maxits, 1, its, sloppy, nupd));
    CHK(blas_scale(c, 4.0, x, 0));
    CHK(op_eo_reconstruct(c, x, b, m));
  }
  return 0;
}

int solve_full_dev(qexhip_ctx *c, DevField &x, DevField &b, double mass, double r2req, int maxits,
                   int *iters, double *r2_final, int use_prev, int sloppy, int *nupdates) {
  DevField *r, *y;
  CHK(get_work(c, WK_R2, &r));
  CHK(get_work(c, WK_Y, &y));
  CHK(blas_norm2(c, b, 2, &c->dscal[2]));
  double b2;
  CHK(read_scalars(c, &c->dscal[2], 1, &b2));
  const double r2stop = r2req * b2;
  double r2e, r2o;
  if (use_prev) {                                  // sp.usePrevSoln (stagSolve.nim:234-238)
    CHK(resid_eo(c, *r, b, x, mass, &r2e, &r2o));
  } else {
    CHK(blas_zero(c, x, 2));
    CHK(blas_copy(c, *r, b, 2));
    CHK(norm2_eo(c, *r, &r2e, &r2o));
  }
  double r2 = r2e + r2o;
  int its = 0, nupd = 0;
  while (r2 > r2stop) {
    int mx = maxits - its;
    if (mx <= 0) break;
    int n = 0;
    CHK(solve_inner(c, *y, *r, mass, r2stop / r2, mx, r2e, r2o, &n, sloppy, &nupd));
    its += n;
    CHK(blas_axpy(c, 1.0, *y, x, 2));
    CHK(resid_eo(c, *r, b, x, mass, &r2e, &r2o));
    r2 = r2e + r2o;
  }
  if (iters) *iters = its;
  if (r2_final) *r2_final = (b2 != 0.0) ? r2 / b2 : 0.0;
  if (nupdates) *nupdates = nupd;
  return 0;
}
