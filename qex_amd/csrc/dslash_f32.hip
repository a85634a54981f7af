// dslash_f32.hip -- the single-precision side of the mixed-precision CG (SolverParams.sloppySolve, solverBase.nim:8-15):
// an fp32 copy of the operator's links, the fp32 Dslash sweep, and the fp32 BLAS / bookkeeping kernels of the reliable-update
// CG whose host control is solve_xx_sloppy_dev (solver.cpp).  Whole lattice on one GPU, or a t-sharded slab with ghost zones (the
// fp64 DevField's layout) filled by the fp32 face exchange; the sweep itself is dslash_lowp.h's, in fp32 storage.
//
// Links: built on the device from the resident fp64 links (c->W: BCs, staggered phases and Naik links already applied), lazily,
// whenever c->links_gen has moved since the last build (every writer of W ends in links_compress, which bumps it).  Per parity
// the copy is [tile][pair][NL][64] float4 with pair pr = (forward link 2pr, backward link 2pr+1): the pair's complex entries
// two to a float4, so every link byte is read with a 16-byte load (MI355X_MICROARCH: narrower loads cost more per byte).
//   format 0 (NL = 9, 72 B/link): 18 reals;
//   format 1 (NL = 6, 48 B/link + 1 bit): rows 0,1 and a sign mask [tile][dir] (bit = lane); row 2 = +-conj(row0 x row1) is
//             rebuilt in registers.  Chosen when every link satisfies that to F32_UNIT_TOL (a few fp32 ulps), and unless
//             QEXHIP_RECON / option "recon" is 0.
// Fields: float2 v[tile][3][64] per parity, the fp64 field's site and tile order (vec_off); with g.halo the ghost tiles follow the
// body as in DevField (ghost_hi, then ghost_lo, room for depth 3 each), without it the body alone.
// Every reduction (<p,Ap>, |r|^2) accumulates in double, as QEX does for fp32 fields (fieldET.nim:609,708).
#include "qexhip_internal.h"
#include "site_index.h"
#include "reduce.h"
#include "cg_device.h"
#include "dslash_lowp.h"
#include <cstring>
#include <cmath>

static constexpr double F32_UNIT_TOL = 1e-6;

struct F32State {
  f4v *W = nullptr; unsigned long long *S = nullptr; size_t cap = 0;   // link copy (capacity in float4)
  int fmt = -1; unsigned long gen = 0; double dev = 0;                  // format in W, links_gen it was built from, unitarity deviation
  DevFieldF f[F32_NF];
  SlpScal *s = nullptr;
};

static F32State *st_of(qexhip_ctx *c) {
  if (!c->f32) c->f32 = new F32State();
  return (F32State *)c->f32;
}

void f32_state_free(qexhip_ctx *c) {
  F32State *S = (F32State *)c->f32;
  if (!S) return;
  if (S->W) (void)hipFree(S->W);
  if (S->S) (void)hipFree(S->S);
  for (auto &f : S->f) if (f.d) (void)hipFree(f.d);
  if (S->s) (void)hipFree(S->s);
  delete S;
  c->f32 = nullptr;
}

static inline size_t body2(const qexhip_ctx *c) { return (size_t)c->g.ntile * 192; }
static inline int grid_for(size_t n) {
  size_t nb = (n + 255) / 256;
  if (nb > 2048) nb = 2048;
  if (nb < 1) nb = 1;
  return (int)nb;
}

// ---- fp32 links ---------------------------------------------------------------------------------------------------
// one wavefront per (parity, tile, pair) row: fp64 rows 2*row (forward) and 2*row+1 (backward) of W
template <int FMT>
__global__ void __launch_bounds__(256) k_links_f32(size_t nrows, const double2 *__restrict__ W, f4v *Wf, unsigned long long *Sf,
                                                   unsigned int *maxdev) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t row = j >> 6;
  if (row >= nrows) return;                     // (whole wavefronts)
  const int l = j & 63;
  constexpr int n = FMT == 1 ? 6 : 9, NL = FMT == 1 ? 6 : 9;
  double2 u[2][9];
#pragma unroll
  for (int h = 0; h < 2; h++)
#pragma unroll
    for (int k = 0; k < 9; k++) u[h][k] = W[(2 * row + h) * 576 + k * 64 + l];
  f4v *o = Wf + row * (NL * 64) + l;
#pragma unroll
  for (int q = 0; q < NL; q++) {
    const double2 a = u[(2 * q) / n][(2 * q) % n], b = u[(2 * q + 1) / n][(2 * q + 1) % n];
    f4v v;
    v.x = (float)a.x; v.y = (float)a.y; v.z = (float)b.x; v.w = (float)b.y;
    o[q * 64] = v;
  }
  if (FMT == 1) {
    double dev = 0;
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const double2 *U = u[h];
      double2 r[3];
      double px = 0;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const int a = (k + 1) % 3, b = (k + 2) % 3;
        r[k].x = (U[a].x * U[3 + b].x - U[a].y * U[3 + b].y) - (U[b].x * U[3 + a].x - U[b].y * U[3 + a].y);
        r[k].y = -((U[a].x * U[3 + b].y + U[a].y * U[3 + b].x) - (U[b].x * U[3 + a].y + U[b].y * U[3 + a].x));
        px += U[6 + k].x * r[k].x + U[6 + k].y * r[k].y;
      }
      const bool neg = px < 0;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const double rx = neg ? -r[k].x : r[k].x, ry = neg ? -r[k].y : r[k].y;
        dev = fmax(dev, fmax(fabs(U[6 + k].x - rx), fabs(U[6 + k].y - ry)));
      }
      const unsigned long long mask = __ballot(neg);
      if (l == 0) Sf[2 * row + h] = mask;
    }
    unsigned int bits = __float_as_uint((float)dev);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned int o2 = __shfl_xor(bits, off, 64);
      bits = o2 > bits ? o2 : bits;
    }
    if (l == 0 && bits > __hip_atomic_load(maxdev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(maxdev, bits);
  }
}

// the fp32 copy of the current links, rebuilt when a writer of W has run since it was made
int f32_links(qexhip_ctx *c, int *fmt_out, double *dev_out) {
  if (!c->W) { qexhip_set_error("staggered links not set (qexhip_stag_set_links)"); return -3; }
  F32State *S = st_of(c);
  if (S->fmt < 0 || S->gen != c->links_gen) {
    const Geom &g = c->g;
    const size_t nrows = (size_t)2 * g.ntile * (c->ndir / 2);
    const size_t need = nrows * 9 * 64;
    if (S->cap < need) {
      if (S->W) HIPCHK(hipFree(S->W));
      if (S->S) HIPCHK(hipFree(S->S));
      S->W = nullptr; S->S = nullptr; S->cap = 0;
      HIPCHK(hipMalloc((void **)&S->W, need * sizeof(f4v)));
      HIPCHK(hipMalloc((void **)&S->S, nrows * 2 * sizeof(unsigned long long)));
      S->cap = need;
    }
    unsigned int *flag = (unsigned int *)&c->dscal[62];
    const unsigned nblk = (unsigned)((nrows * 64 + 255) / 256);
    int fmt = 0;
    double dev = 0;
    if (c->opt_recon) {
      HIPCHK(hipMemsetAsync(flag, 0, sizeof(unsigned int), c->stream));
      k_links_f32<1><<<nblk, 256, 0, c->stream>>>(nrows, c->W, S->W, S->S, flag);
      HIPCHK(hipGetLastError());
      unsigned int bits = 0;
      HIPCHK(hipMemcpyAsync(&bits, flag, sizeof(bits), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
      float d;
      memcpy(&d, &bits, sizeof(d));
      dev = d;
    }
    if (c->nranks > 1 && comm_ready(c)) {
      // t-sharded: the largest deviation over the ranks decides, so that every slab is stored in the format the whole lattice would
      // be (and the sharded operator gives the one-rank operator's bits); a rank with the sign format switched off rules it out
      // everywhere.  Collective: every rank rebuilds its copy at the same point, behind the same (collective) writer of the links.
      double v[1] = {c->opt_recon ? dev : 1e300};
      CHK(comm_allreduce_max(c, v, 1));
      if (c->opt_recon) dev = v[0];
      if (v[0] <= F32_UNIT_TOL) fmt = 1;
    } else if (c->opt_recon && dev <= F32_UNIT_TOL) {
      fmt = 1;
    }
    if (fmt == 0) {
      k_links_f32<0><<<nblk, 256, 0, c->stream>>>(nrows, c->W, S->W, nullptr, nullptr);
      HIPCHK(hipGetLastError());
    }
    S->fmt = fmt; S->dev = dev; S->gen = c->links_gen;
  }
  if (fmt_out) *fmt_out = S->fmt;
  if (dev_out) *dev_out = S->dev;
  return 0;
}

// What a sweep kernel takes for output parity `parity` from the current copy (f32_links has run): the parity's first pair row, its sign
// masks (format 1, else null), the format.  Launches nothing and rebuilds nothing.
int f32_links_dev(qexhip_ctx *c, int parity, const void **W, const unsigned long long **Sm, int *fmt) {
  F32State *S = st_of(c);
  if (S->fmt < 0) { qexhip_set_error("internal: fp32 links not built (f32_links)"); return -3; }
  *fmt = S->fmt;
  const size_t rows = (size_t)parity * c->g.ntile * c->ndir;       // (tile, direction) rows before this parity; a pair holds two
  *W = S->W + rows / 2 * ((S->fmt == 1 ? 6 : 9) * 64);
  *Sm = S->fmt == 1 ? S->S + rows : nullptr;
  return 0;
}

// etile = ntile without a halo: the ghost zones cost nothing on a one-rank context that has none.  A field allocated before the
// geometry changed (qexhip_comm_force_halo) is allocated again.
int f32_field_ensure(qexhip_ctx *c, DevFieldF &F) {
  const size_t half = (size_t)c->g.etile * 192;
  if (F.d && F.half != half) {
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipFree(F.d));
    F.d = nullptr;
  }
  if (!F.d) {
    F.half = half;
    HIPCHK(hipMalloc((void **)&F.d, 2 * F.half * sizeof(float2)));
    HIPCHK(hipMemsetAsync(F.d, 0, 2 * F.half * sizeof(float2), c->stream));   // padding lanes stay zero
  }
  return 0;
}
int f32_field(qexhip_ctx *c, int slot, DevFieldF **f) {
  *f = &st_of(c)->f[slot];
  return f32_field_ensure(c, **f);
}

// ---- fp32 Dslash sweep --------------------------------------------------------------------------------------------
// k_dslash_lowp<StoreF32, ..> behind sweep_lowp<StoreF32> (dslash_lowp.h: the operator, its forms on a slab, the host sweep)
// r[px] = 4 m2 x - (2D)(2D) x in fp32 (op_xx's two sweeps); dot: <x,r> partials in c->partials[0..*nparts)
int f32_op_xx(qexhip_ctx *c, DevFieldF &r, DevFieldF &x, double m2, int par_even, int dot, const int *done, int *nparts) {
  CHK(f32_links(c, nullptr, nullptr));
  DevFieldF *t;
  CHK(f32_field(c, F32_T, &t));
  return op_xx_lowp<StoreF32>(c, r, x, *t, m2, par_even, dot, done, nparts);
}

// ---- precision conversions ----------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_to_f32(float2 *y, const double2 *x, double a, size_t n) {
  for (size_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const double2 v = x[i];
    y[i] = make_float2((float)(a * v.x), (float)(a * v.y));
  }
}
__global__ void __launch_bounds__(256) k_to_f64(double2 *y, const float2 *x, double a, int acc, size_t n) {
  for (size_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float2 v = x[i];
    double2 o = acc ? y[i] : make_double2(0.0, 0.0);
    o.x = fma(a, (double)v.x, o.x); o.y = fma(a, (double)v.y, o.y);
    y[i] = o;
  }
}
int f32_from_f64(qexhip_ctx *c, DevFieldF &y, const DevField &x, int parity, double a) {
  const size_t n = body2(c);
  k_to_f32<<<grid_for(n), 256, 0, c->stream>>>(y.par(parity), x.par(parity), a, n);
  HIPCHK(hipGetLastError());
  return 0;
}
int f32_to_f64(qexhip_ctx *c, DevField &y, const DevFieldF &x, int parity, double a, int accumulate) {
  const size_t n = body2(c);
  k_to_f64<<<grid_for(n), 256, 0, c->stream>>>(y.par(parity), x.par(parity), a, accumulate, n);
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- reliable-update CG: device bookkeeping -----------------------------------------------------------------------
// The fp32 vectors r_s, p_s, x_s hold r / sigma, p / sigma_p and the increment of x / sigma, sigma = |r| at the last reliable
// update: every fp32 residual starts at norm 1, so tight tolerances never reach fp32 denormals.  All scalars are double.
int slp_alloc(qexhip_ctx *c, SlpScal **s) {
  F32State *S = st_of(c);
  if (!S->s) HIPCHK(hipMalloc((void **)&S->s, sizeof(SlpScal)));
  *s = S->s;
  return 0;
}

// b2 in dscal[0]; r = b, x = 0, x_s = 0 already
__global__ void k_slp_init(SlpScal *s, const double *dscal, double r2req, int maxits) {
  SlpScal t = {};
  t.b2 = dscal[0];
  t.r2stop = r2req * t.b2;
  t.r2t = t.b2;
  t.maxits = maxits;
  t.done = !(0 < maxits && t.r2t > t.r2stop);
  t.sigma = t.done ? 1.0 : sqrt(t.r2t);
  t.sigma_p = t.sigma;
  t.r2s = 1.0; t.r2s_old = 1.0; t.maxr2s = 1.0;
  t.conv = 1; t.first = 1; t.upd = 0; t.noupd = 1;
  *s = t;
}

// p_s := r_s (first iteration) | r_s + beta' p_s, beta' = (r2 sigma) / (r2_old sigma_p): QEX's beta = r2/r2old (cg.nim:186-193)
// in the units of the current sigma.  Behind a reliable update (conv) r_s is first rebuilt from the fp64 residual: r_s = r / sigma.
__global__ void __launch_bounds__(256) k_slp_xpay(float2 *p, float2 *rs, const double2 *r, size_t n, const SlpScal *s) {
  if (s->done) return;
  const bool conv = s->conv, first = s->first;
  const double inv = 1.0 / s->sigma;
  const float beta = (float)((s->r2s * s->sigma) / (s->r2s_old * s->sigma_p));
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

// alpha = r2 / <p,Ap>; x_s += alpha p_s; r_s -= alpha Ap_s; |r_s|^2 partials in double  (cg.nim:208-213)
__global__ void __launch_bounds__(256) k_slp_update(float2 *xs, float2 *rs, const float2 *p, const float2 *Ap, size_t n,
                                                    const SlpScal *s, const double *dotp, int ndot, double *partials) {
  if (s->done) return;
  const double pAp = cg_sum_parts(dotp, ndot);
  const float alpha = (float)(s->r2s / pAp);
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
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// end of an fp32 iteration: the new |r_s|^2, and whether a reliable update is due (QUDA's criterion r2 < delta^2 max r2 since the
// last one, or the fp32 residual says converged, or the iteration limit is reached).  A pending update stays pending until it runs.
__global__ void __launch_bounds__(256) k_slp_close(SlpScal *s, const double *parts, int nparts, double delta2) {
  if (s->done) return;
  const double r2 = cg_sum_parts(parts, nparts);
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

// reliable update, part 1: x += sigma x_s, x_s = 0  (no-op unless an update is due)
__global__ void __launch_bounds__(256) k_slp_flush(double2 *x, float2 *xs, size_t n, const SlpScal *s) {
  if (!s->upd || s->done) return;
  const double sg = s->sigma;
  for (size_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float2 v = xs[i];
    double2 o = x[i];
    o.x = fma(sg, (double)v.x, o.x); o.y = fma(sg, (double)v.y, o.y);
    x[i] = o;
    xs[i] = make_float2(0.f, 0.f);
  }
}
// part 2 (behind op_xx's fp64 sweeps into Ax): r = b - Ax, |r|^2 partials
__global__ void __launch_bounds__(256) k_slp_resid(double2 *r, const double2 *b, const double2 *Ax, size_t n, const SlpScal *s,
                                                   double *partials) {
  if (!s->upd || s->done) return;
  double acc = 0;
  for (size_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const double2 bv = b[i], av = Ax[i];
    const double2 rv = make_double2(bv.x - av.x, bv.y - av.y);
    r[i] = rv;
    acc = fma(rv.x, rv.x, fma(rv.y, rv.y, acc));
  }
  const double t = block_sum_256(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}
// part 3: the true residual decides; otherwise the fp32 recursion restarts from it, renormalised (r_s is rebuilt by the next
// k_slp_xpay), and p_s carries on (its units are converted through sigma_p)
__global__ void __launch_bounds__(256) k_slp_rclose(SlpScal *s, const double *parts, int nparts) {
  if (!s->upd || s->done) return;
  const double r2t = cg_sum_parts(parts, nparts);
  if (threadIdx.x == 0) {
    s->r2t = r2t;
    s->nupd += 1;
    s->upd = 0; s->noupd = 1;
    if (!(r2t > s->r2stop) || s->k >= s->maxits) {
      s->done = 1;
    } else {
      const double sg = sqrt(r2t);
      s->r2s = 1.0;                                 // |r / sigma|^2; r2s_old and sigma_p keep the units p_s is in
      s->sigma = sg;
      s->maxr2s = 1.0;
      s->conv = 1;
      if (!(s->r2s_old > 0)) s->first = 1;          // (an fp32 residual of exactly 0 leaves no direction to continue)
    }
  }
}

int slp_init(qexhip_ctx *c, SlpScal *s, double r2req, int maxits) {
  k_slp_init<<<1, 1, 0, c->stream>>>(s, c->dscal, r2req, maxits);
  HIPCHK(hipGetLastError());
  return 0;
}
int slp_xpay(qexhip_ctx *c, SlpScal *s, DevFieldF &p, DevFieldF &rs, const DevField &r, int parity) {
  const size_t n = body2(c);
  k_slp_xpay<<<grid_for(n), 256, 0, c->stream>>>(p.par(parity), rs.par(parity), r.par(parity), n, s);
  HIPCHK(hipGetLastError());
  return 0;
}
// Sharded, every set of partials these kernels sum -- <p,Ap> and |r_s|^2 here, |b - A x|^2 in slp_resid (|b|^2: blas_norm2) -- is first
// summed over the ranks (comm_allreduce_parts, as the fp64 CG does in cg_update), so that k_slp_close / k_slp_rclose see the same
// rank-global values on every rank.  INVARIANT: every rank then sets the same `upd` / `done` flags at the same iteration and takes the
// same reliable updates and the same stop; the host posts the same exchanges and all-reduces everywhere, and solve_xx_sloppy_dev checks
// the agreement at the end of every chunk -- a rank that left the loop or skipped an update its neighbour took would leave the
// neighbour's next exchange without a partner.  (One rank: comm_allreduce_parts changes nothing, the bits are the one-rank solve's.)
int slp_update(qexhip_ctx *c, SlpScal *s, DevFieldF &xs, DevFieldF &rs, const DevFieldF &p, const DevFieldF &Ap, int parity, int ndot) {
  const size_t n = body2(c);
  const int nb = grid_for(n);
  double *r2p = c->partials + c->part2_off;
  if (ndot > 0) CHK(comm_allreduce_parts(c, c->partials, ndot, &ndot));
  CHK(devjoin_flush(c));              // (no-op when the all-reduce has taken the second sweep's join with it)
  k_slp_update<<<nb, 256, 0, c->stream>>>(xs.par(parity), rs.par(parity), p.par(parity), Ap.par(parity), n, s, c->partials, ndot, r2p);
  HIPCHK(hipGetLastError());
  int nr2 = nb;
  CHK(comm_allreduce_parts(c, r2p, nb, &nr2));
  k_slp_close<<<1, 256, 0, c->stream>>>(s, r2p, nr2, SLP_DELTA * SLP_DELTA);
  HIPCHK(hipGetLastError());
  return 0;
}
// one fp32 iteration on the slots F32_R / F32_P / F32_AP: xpay, the two sweeps, the update and its close (slph_iterate's twin)
int slp_iterate(qexhip_ctx *c, SlpScal *s, DevFieldF &xs, const DevField &r, double m2, int par_even) {
  DevFieldF *rs, *ps, *aps;
  CHK(f32_field(c, F32_R, &rs));
  CHK(f32_field(c, F32_P, &ps));
  CHK(f32_field(c, F32_AP, &aps));
  const int par = par_even ? 0 : 1;
  CHK(slp_xpay(c, s, *ps, *rs, r, par));
  int ndot = 0;
  CHK(f32_op_xx(c, *aps, *ps, m2, par_even, 1, &s->done, &ndot));
  return slp_update(c, s, xs, *rs, *ps, *aps, par, ndot);
}
// the close of an iteration whose update kernel is another file's (dslash_half.hip): nparts rank-global |r_s|^2 partials in r2p
int slp_close(qexhip_ctx *c, SlpScal *s, const double *r2p, int nparts) {
  k_slp_close<<<1, 256, 0, c->stream>>>(s, r2p, nparts, SLP_DELTA * SLP_DELTA);
  HIPCHK(hipGetLastError());
  return 0;
}
int slp_flush(qexhip_ctx *c, SlpScal *s, DevField &x, DevFieldF &xs, int parity) {
  const size_t n = body2(c);
  k_slp_flush<<<grid_for(n), 256, 0, c->stream>>>(x.par(parity), xs.par(parity), n, s);
  HIPCHK(hipGetLastError());
  return 0;
}
int slp_resid(qexhip_ctx *c, SlpScal *s, DevField &r, const DevField &b, const DevField &Ax, int parity) {
  const size_t n = body2(c);
  const int nb = grid_for(n);
  double *r2p = c->partials + c->part2_off;
  k_slp_resid<<<nb, 256, 0, c->stream>>>(r.par(parity), b.par(parity), Ax.par(parity), n, s, r2p);
  HIPCHK(hipGetLastError());
  int nr2 = nb;
  CHK(comm_allreduce_parts(c, r2p, nb, &nr2));      // (posted whether or not an update is due: the ranks post the same collectives)
  k_slp_rclose<<<1, 256, 0, c->stream>>>(s, r2p, nr2);
  HIPCHK(hipGetLastError());
  return 0;
}
