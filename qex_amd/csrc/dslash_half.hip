// dslash_half.hip -- 16-bit storage for the mixed-precision CG (SolverParams.sloppySolve = SloppyHalf with option "half" = 1;
// QUDA's half precision behind qudaWrapperImpl.nim:197): a 16-bit copy of the operator's links, the Dslash sweep on 16-bit
// vectors, and the BLAS kernels of the reliable-update CG whose host control is solve_xx_half_dev (solver.cpp).  Whole lattice on
// one GPU, or a t-sharded slab with ghost zones filled by the 16-bit face exchange; one system.  The sweep itself is dslash_lowp.h's,
// in 16-bit storage.  Arithmetic is fp32 (dslash_f32_core.h); only what lies in HBM between kernels is 16-bit.
//
// Vectors: fixed point, not IEEE half.  One site is 16 bytes, six int16 (re, im of the three colours) and one fp32 norm = the
// largest |component| of the site: q = rint(v 32767 / norm), v ~ q norm / 32767; a zero site (norm below FLT_MIN) is all zeros.
// Per parity the field is [tile][64] such elements in the fp64 field's site order: element c of a parity is site c (vec_off's
// tile and lane), a neighbour is one 16-byte load and a wavefront reads 1 KiB contiguously.  With g.halo the ghost zones follow
// the body at the positions nbr_pos<true> gives them (DevFieldH), and a t-face is a contiguous element range: 16 B per site on the
// wire, against 24 B in fp32 and 48 B in fp64, without a pack kernel.  The BLAS kernels run over the body only.  half_pack_host / half_unpack_host
// restate the format on the host in double.
//
// Links: int16, q = rint(u 32767 / s), built on the device from the resident fp64 links (c->W) whenever c->links_gen has moved,
// behind the fp32 copy (f32_links), whose format decision and sign masks they share.  Per parity [tile][pair] rows, pair pr =
// (forward link 2pr, backward link 2pr+1), one 32-bit word per complex entry (re low, im high):
//   format 1 (48 B/pair): rows 0,1 of both links, s = 1, values clamped; [3][64] 16-byte elements per row, row 2 rebuilt in
//             registers with the fp32 copy's sign masks;
//   format 0 (72 B/pair): 18 reals of both links, s = the largest |entry| of the link kind (fat: pairs 0..3, long: pairs 4..7) over
//             the whole lattice (max-reduced over the ranks of a sharded one);
//             a row is [4][64] 16-byte elements followed by [64] 8-byte elements (4608 B).
// Every reduction (<p,Ap>, |r|^2) is formed from the values as stored and accumulates in double.
#include "qexhip_internal.h"
#include "site_index.h"
#include "reduce.h"
#include "cg_device.h"
#include "dslash_lowp.h"
#include <cstring>
#include <cmath>
#include <cfloat>

static HalfState *hs_of(qexhip_ctx *c) {
  if (!c->half) c->half = new HalfState();
  return (HalfState *)c->half;
}

void half_state_free(qexhip_ctx *c) {
  HalfState *S = (HalfState *)c->half;
  if (!S) return;
  if (S->W) (void)hipFree(S->W);
  if (S->mx) (void)hipFree(S->mx);
  for (auto &f : S->f) if (f.d) (void)hipFree(f.d);
  if (S->stall) (void)hipFree(S->stall);
  delete S;
  c->half = nullptr;
}
HalfState *half_state(qexhip_ctx *c) { return hs_of(c); }

// ---- the vector format on the host (double arithmetic) ---------------------------------------------------------------
int half_pack_host(const double *v, size_t nsites, int16_t *q, float *norm) {
  for (size_t i = 0; i < nsites; i++) {
    double m = 0;
    for (int k = 0; k < 6; k++) m = std::fmax(m, std::fabs(v[6 * i + k]));
    const float nf = (float)m;
    if (!(nf >= FLT_MIN) || std::isinf(nf)) {
      if (std::isinf(nf) || std::isnan(nf)) { qexhip_set_error("half_pack_host: site %zu is not finite in fp32", i); return -1; }
      norm[i] = 0.f;
      for (int k = 0; k < 6; k++) q[6 * i + k] = 0;
      continue;
    }
    norm[i] = nf;
    const double s = 32767.0 / (double)nf;
    for (int k = 0; k < 6; k++) {
      double r = std::rint(v[6 * i + k] * s);
      r = r > 32767.0 ? 32767.0 : (r < -32767.0 ? -32767.0 : r);
      q[6 * i + k] = (int16_t)r;
    }
  }
  return 0;
}
int half_unpack_host(const int16_t *q, const float *norm, size_t nsites, double *v) {
  for (size_t i = 0; i < nsites; i++) {
    const double s = (double)norm[i] / 32767.0;
    for (int k = 0; k < 6; k++) v[6 * i + k] = (double)q[6 * i + k] * s;
  }
  return 0;
}

// ---- 16-bit links -----------------------------------------------------------------------------------------------------
// the largest |entry| per link kind, exactly: non-negative doubles order as their bit patterns.  One wavefront per pair row.
__global__ void __launch_bounds__(256) k_links_absmax(size_t nrows, int npair, const double2 *__restrict__ W, unsigned long long *mx) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t row = j >> 6;
  if (row >= nrows) return;                     // (whole wavefronts)
  const int l = j & 63;
  double m = 0;
#pragma unroll
  for (int h = 0; h < 2; h++)
#pragma unroll
    for (int k = 0; k < 9; k++) {
      const double2 u = W[(2 * row + h) * 576 + k * 64 + l];
      m = fmax(m, fmax(fabs(u.x), fabs(u.y)));
    }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
  if (l == 0) {
    unsigned long long *dst = &mx[(int)(row % (size_t)npair) >= 4 ? 1 : 0];
    const unsigned long long bits = (unsigned long long)__double_as_longlong(m);
    if (bits > __hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(dst, bits);
  }
}

__device__ __forceinline__ unsigned qword(const double2 u, const double sc) {
  const double re = fmin(fmax(rint(u.x * sc), -32767.0), 32767.0), im = fmin(fmax(rint(u.y * sc), -32767.0), 32767.0);
  return ((unsigned)(int)re & 0xffffu) | ((unsigned)(int)im << 16);
}

// one wavefront per (parity, tile, pair) row: fp64 rows 2*row (forward) and 2*row+1 (backward) of W
template <int FMT>
__global__ void __launch_bounds__(256) k_links_half(size_t nrows, int npair, const double2 *__restrict__ W, void *out, double sc_fat,
                                                    double sc_long) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t row = j >> 6;
  if (row >= nrows) return;                     // (whole wavefronts)
  const int l = j & 63;
  constexpr int n = FMT == 1 ? 6 : 9;           // entries kept per link
  const double sc = (int)(row % (size_t)npair) >= 4 ? sc_long : sc_fat;
  unsigned w[2 * n];
#pragma unroll
  for (int h = 0; h < 2; h++)
#pragma unroll
    for (int k = 0; k < n; k++) w[h * n + k] = qword(W[(2 * row + h) * 576 + k * 64 + l], sc);
  if (FMT == 1) {
    u4v *o = (u4v *)out + row * (3 * 64) + l;
#pragma unroll
    for (int q = 0; q < 3; q++) {
      u4v v;
      v.x = w[4 * q]; v.y = w[4 * q + 1]; v.z = w[4 * q + 2]; v.w = w[4 * q + 3];
      o[q * 64] = v;
    }
  } else {
    char *base = (char *)out + row * HALF_ROW0;
    u4v *o = (u4v *)base + l;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      u4v v;
      v.x = w[4 * q]; v.y = w[4 * q + 1]; v.z = w[4 * q + 2]; v.w = w[4 * q + 3];
      o[q * 64] = v;
    }
    u2v t;
    t.x = w[16]; t.y = w[17];
    ((u2v *)(base + 4096))[l] = t;
  }
}

// the 16-bit copy of the current links, rebuilt when a writer of W has run since it was made
int half_links(qexhip_ctx *c, int *fmt_out, double *s_fat, double *s_long, double *dev_out) {
  int fmt = 0;
  double dev = 0;
  CHK(f32_links(c, &fmt, &dev));               // the format decision and, in format 1, the sign masks
  HalfState *S = hs_of(c);
  if (S->fmt < 0 || S->gen != c->links_gen || S->fmt != fmt) {
    const int npair = c->ndir / 2;
    const size_t nrows = (size_t)2 * c->g.ntile * npair;
    const size_t need = nrows * HALF_ROW0;
    if (S->cap < need) {
      if (S->W) HIPCHK(hipFree(S->W));
      S->W = nullptr; S->cap = 0;
      HIPCHK(hipMalloc(&S->W, need));
      S->cap = need;
    }
    if (!S->mx) HIPCHK(hipMalloc((void **)&S->mx, 2 * sizeof(unsigned long long)));
    const unsigned nblk = (unsigned)((nrows * 64 + 255) / 256);
    HIPCHK(hipMemsetAsync(S->mx, 0, 2 * sizeof(unsigned long long), c->stream));
    k_links_absmax<<<nblk, 256, 0, c->stream>>>(nrows, npair, c->W, S->mx);
    HIPCHK(hipGetLastError());
    unsigned long long bits[2];
    HIPCHK(hipMemcpyAsync(bits, S->mx, sizeof bits, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    double s[2];
    memcpy(s, bits, sizeof s);
    // t-sharded: format 0 divides by the largest |entry| of the WHOLE lattice, so that a slab's int16 links are the one-rank copy's.
    // c->W holds the body tiles only (backward links arrive shifted and adjointed at set_links), so there are no ghost link tiles to
    // exclude: a slab's rows are exactly the links its sites apply, and the ranks' slabs together are the lattice.  Reduced in
    // format 1 as well (s = 1 there): links_info_half reports rank-global maxima.
    // INVARIANT: this makes the lazily built copy a collective.  Every rank reaches it at the same call -- slph_begin, the operator
    // probe, links_info_half -- behind the same (collective) writer of the links, as with f32_links above.
    if (c->nranks > 1 && comm_ready(c)) CHK(comm_allreduce_max(c, s, 2));
    if (fmt == 1) {
      k_links_half<1><<<nblk, 256, 0, c->stream>>>(nrows, npair, c->W, S->W, 32767.0, 32767.0);
    } else {
      k_links_half<0><<<nblk, 256, 0, c->stream>>>(nrows, npair, c->W, S->W, s[0] > 0 ? 32767.0 / s[0] : 0.0,
                                                   s[1] > 0 ? 32767.0 / s[1] : 0.0);
    }
    HIPCHK(hipGetLastError());
    S->fmt = fmt; S->dev = dev; S->gen = c->links_gen;
    S->s_fat = s[0]; S->s_long = s[1];
  }
  if (fmt_out) *fmt_out = S->fmt;
  if (s_fat) *s_fat = S->s_fat;
  if (s_long) *s_long = S->s_long;
  if (dev_out) *dev_out = S->dev;
  return 0;
}

// etile = ntile without a halo (f32_field_ensure): the lock-step batch, which runs on such contexts only, sees the size it always saw
int half_field_ensure(qexhip_ctx *c, DevFieldH &F) {
  const size_t half = (size_t)c->g.etile * 64;
  if (F.d && F.half != half) {
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipFree(F.d));
    F.d = nullptr;
  }
  if (!F.d) {
    F.half = half;
    HIPCHK(hipMalloc((void **)&F.d, 2 * half * sizeof(u4v)));
    HIPCHK(hipMemsetAsync(F.d, 0, 2 * half * sizeof(u4v), c->stream));   // padding lanes stay zero
  }
  return 0;
}
static int half_field(qexhip_ctx *c, int slot, DevFieldH **f) {
  DevFieldH &F = hs_of(c)->f[slot];
  CHK(half_field_ensure(c, F));
  *f = &F;
  return 0;
}

// ---- 16-bit Dslash sweep ------------------------------------------------------------------------------------------------
// k_dslash_lowp<StoreHalf, ..> behind sweep_lowp<StoreHalf> (dslash_lowp.h: the operator, its one scale per hop, its forms on a slab)
// r[px] = 4 m2 x - (2D)(2D) x on 16-bit fields (slots of HalfState); dot: <x,r> partials in c->partials[0..*nparts)
static int half_op_xx(qexhip_ctx *c, DevFieldH &r, DevFieldH &x, double m2, int par_even, int dot, const int *done, int *nparts) {
  DevFieldH *t;
  CHK(half_field(c, HALF_T, &t));
  return op_xx_lowp<StoreHalf>(c, r, x, *t, m2, par_even, dot, done, nparts);
}

// ---- conversions (the operator probe) ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_to_half(u4v *y, const double2 *x, size_t nsites) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nsites; i += (size_t)gridDim.x * 256) {
    float2 v[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const double2 d = x[vec_off((int)i, k)];
      v[k] = make_float2((float)d.x, (float)d.y);
    }
    y[i] = pack_site(v);
  }
}
__global__ void __launch_bounds__(256) k_from_half(double2 *y, const u4v *x, size_t nsites) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nsites; i += (size_t)gridDim.x * 256) {
    float2 v[3];
    unpack_site(x[i], v, HQ_INV);
#pragma unroll
    for (int k = 0; k < 3; k++) y[vec_off((int)i, k)] = make_double2((double)v[k].x, (double)v[k].y);
  }
}

int half_from_f64(qexhip_ctx *c, u4v *y, const double2 *x) {
  const size_t n = nsite_h(c);
  k_to_half<<<grid_sites(n), 256, 0, c->stream>>>(y, x, n);
  HIPCHK(hipGetLastError());
  return 0;
}
int half_to_f64(qexhip_ctx *c, double2 *y, const u4v *x) {
  const size_t n = nsite_h(c);
  k_from_half<<<grid_sites(n), 256, 0, c->stream>>>(y, x, n);
  HIPCHK(hipGetLastError());
  return 0;
}

// fr[px] = the 16-bit operator on fx[px] rounded to 16 bits, back in fp64 (qexhip_dev_op_xx_half); on a slab, the slab of it
int half_op_xx_probe(qexhip_ctx *c, DevField &fr, const DevField &fx, double m2, int par_even) {
  CHK(half_links(c, nullptr, nullptr, nullptr, nullptr));      // (sharded: collective, see half_links)
  DevFieldH *xi, *ro;
  CHK(half_field(c, HALF_IN, &xi));
  CHK(half_field(c, HALF_AP, &ro));
  const int px = par_even ? 0 : 1;
  const size_t n = nsite_h(c);
  k_to_half<<<grid_sites(n), 256, 0, c->stream>>>(xi->par(px), fx.par(px), n);
  HIPCHK(hipGetLastError());
  CHK(half_op_xx(c, *ro, *xi, m2, par_even, 0, nullptr, nullptr));
  k_from_half<<<grid_sites(n), 256, 0, c->stream>>>(fr.par(px), ro->par(px), n);
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- reliable-update CG on 16-bit vectors -------------------------------------------------------------------------------
// k_slp_xpay on 16-bit r_s, p_s: p_s := r_s (first iteration) | r_s + beta' p_s; behind a reliable update r_s is first rebuilt
// from the fp64 residual, and p_s continues from r_s as stored.  One lane per site.
__global__ void __launch_bounds__(256) k_slph_xpay(u4v *p, u4v *rs, const double2 *r, size_t nsites, const SlpScal *s) {
  if (s->done) return;
  const bool conv = s->conv, first = s->first;
  const double inv = 1.0 / s->sigma;
  const float beta = (float)((s->r2s * s->sigma) / (s->r2s_old * s->sigma_p));
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

// k_slp_update on 16-bit r_s, p_s, Ap_s; the increment x_s stays fp32 (float2 [tile][3][64]).  |r_s|^2 partials from r_s as stored.
__global__ void __launch_bounds__(256) k_slph_update(float2 *xs, u4v *rs, const u4v *p, const u4v *Ap, size_t nsites, const SlpScal *s,
                                                     const double *dotp, int ndot, double *partials) {
  if (s->done) return;
  const double pAp = cg_sum_parts(dotp, ndot);
  const float alpha = (float)(s->r2s / pAp);
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
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// The stall guard, behind a (gated) reliable update: an update that did not lower the true residual below the smallest one seen
// counts as failed; `limit` failures in a row (limit 0: the first update) stop the 16-bit iteration -- the host finishes in fp32.
__global__ void k_slph_stall_init(HalfStall *h, const SlpScal *s) {
  h->best = s->r2t; h->seen = 0; h->nfail = 0; h->stalled = 0; h->pad = 0;
}
__global__ void k_slph_stall(HalfStall *h, SlpScal *s, int limit) {
  if (s->nupd == h->seen) return;
  h->seen = s->nupd;
  if (s->done) return;
  if (s->r2t < h->best) { h->best = s->r2t; h->nfail = 0; }
  else h->nfail += 1;
  if (h->nfail >= limit) { h->stalled = 1; s->done = 1; }
}

int slph_begin(qexhip_ctx *c, SlpScal *s) {
  CHK(half_links(c, nullptr, nullptr, nullptr, nullptr));
  HalfState *S = hs_of(c);
  if (!S->stall) HIPCHK(hipMalloc((void **)&S->stall, sizeof(HalfStall)));
  k_slph_stall_init<<<1, 1, 0, c->stream>>>(S->stall, s);
  HIPCHK(hipGetLastError());
  return 0;
}
// one 16-bit iteration: xpay, the two sweeps, the update and its close (k_slp_close: slp_close).  Sharded, the <p,Ap> partials are
// summed over the ranks before k_slph_update and the |r_s|^2 partials before the close, exactly as slp_update does (its INVARIANT holds
// here too: every rank sets the same `upd` / `done` / `stalled` at the same iteration -- k_slph_stall decides from the rank-global r2t
// and the rank-global counters alone --, and solve_xx_half_dev checks the agreement at the end of every chunk).  One rank:
// comm_allreduce_parts changes nothing, the bits are the one-rank solve's.
int slph_iterate(qexhip_ctx *c, SlpScal *s, DevFieldF &xs, const DevField &r, double m2, int par_even) {
  DevFieldH *rs, *ps, *aps;
  CHK(half_field(c, HALF_R, &rs));
  CHK(half_field(c, HALF_P, &ps));
  CHK(half_field(c, HALF_AP, &aps));
  const int par = par_even ? 0 : 1;
  const size_t n = nsite_h(c);
  const int nb = grid_sites(n);
  k_slph_xpay<<<nb, 256, 0, c->stream>>>(ps->par(par), rs->par(par), r.par(par), n, s);
  HIPCHK(hipGetLastError());
  int ndot = 0;
  CHK(half_op_xx(c, *aps, *ps, m2, par_even, 1, &s->done, &ndot));
  double *r2p = c->partials + c->part2_off;
  if (ndot > 0) CHK(comm_allreduce_parts(c, c->partials, ndot, &ndot));
  CHK(devjoin_flush(c));              // (no-op when the all-reduce has taken the second sweep's join with it)
  k_slph_update<<<nb, 256, 0, c->stream>>>(xs.par(par), rs->par(par), ps->par(par), aps->par(par), n, s, c->partials, ndot, r2p);
  HIPCHK(hipGetLastError());
  int nr2 = nb;
  CHK(comm_allreduce_parts(c, r2p, nb, &nr2));
  return slp_close(c, s, r2p, nr2);
}
int slph_stall(qexhip_ctx *c, SlpScal *s, int limit) {
  k_slph_stall<<<1, 1, 0, c->stream>>>(hs_of(c)->stall, s, limit);
  HIPCHK(hipGetLastError());
  return 0;
}
int slph_stalled_async(qexhip_ctx *c, int *pinned) {     // the guard's flag -> pinned host memory, on the compute stream
  HIPCHK(hipMemcpyAsync(pinned, &hs_of(c)->stall->stalled, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  return 0;
}
