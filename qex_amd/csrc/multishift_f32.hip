// multishift_f32.hip -- the fp32 iteration of the mixed-precision multi-shift CG (host control: solve_xx_multi_sloppy_dev, solver.cpp).
//
// QUDA's scheme for mixed-precision multi-shift on this library's pieces.  fp64 holds b, the true residual r of the BASE system and
// all nmass solutions x_k (the caller's fields); fp32 holds r_s = r/sigma0, Ap_s, the search directions ps_k and the increments xs_k.
// Per iteration: Ap_s = A ps_0 (f32_op_xx, <p,Ap> in double) | k_msf_base: alpha, r_s -= alpha Ap_s, xs_0 += alpha ps_0, |r_s|^2 |
// k_msf_close: one workgroup, the zeta recurrences of cgm.nim:253-266 in double (k_cgm_close's device logic, `pending` included) and
// k_slp_close's decision whether a reliable update is due | k_msf_update: ONE streaming pass over every shift.  A reliable update
// (device-gated, as the single solve's) is k_msf_flush -- x_k += sigma0 xs_k, xs_k = 0 for ALL shifts in one launch --, the fp64
// op_xx on x_0, and k_slp_resid / k_slp_rclose unchanged (slp_resid): the true residual of the base system alone decides the stop.
//
// Units: the VECTORS stay in units of sigma0 = |b| for the whole solve (no renormalisation: the nmass search directions and the
// zeta recurrences never change units; fp32's exponent range carries |r_s| down to 1e-15 |b|, i.e. r2req down to 1e-30, in normal
// numbers, and every reduction accumulates in double).  The SCALARS r2s / maxr2s of SlpScal stay in units of SlpScal.sigma = |r| at
// the last update, which k_slp_rclose maintains -- k_msf_base / k_msf_close convert through sigma^2 / sigma0^2.
// k_slp_rclose also sets SlpScal.first and keeps sigma_p / r2s_old for k_slp_xpay's unit conversion: this iteration has no xpay and
// ignores all three.
// Fields are float2 v[tile][3][64] (a multiple of 128 float2 per parity): every fp32 stream is walked as float4, 16 bytes per lane.
#include "qexhip_internal.h"
#include "reduce.h"
#include "cg_device.h"
#include <cstring>
#include <algorithm>

#define MSF_MAXM CGM_MAXM

// The per-shift field pointers come out of device memory (MsfScal), where the compiler knows no address space: told that they are
// global, it emits global_load / global_store_dwordx4 instead of flat ones.
typedef float f4n __attribute__((ext_vector_type(4)));
typedef double d2n __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) f4n gf4;
typedef __attribute__((address_space(1))) d2n gd2;
__device__ __forceinline__ f4n fma4(float a, f4n x, f4n y) { return f4n{fmaf(a, x.x, y.x), fmaf(a, x.y, y.y), fmaf(a, x.z, y.z), fmaf(a, x.w, y.w)}; }

struct MsfScal {
  int nmass, cont, pending, pad;
  double alphaim1, betaim1;
  double sigma0;                                  // |b|: the unit of every fp32 vector
  double sg[MSF_MAXM], zi[MSF_MAXM], zim1[MSF_MAXM];
  float alpha, beta;                              // of the base system, for the vectors
  float axz[MSF_MAXM], zip1[MSF_MAXM], bzz[MSF_MAXM];
  float4 *ps[MSF_MAXM], *xs[MSF_MAXM];
  double2 *x[MSF_MAXM];
};

struct MsfState {
  DevFieldF ps[MSF_MAXM], xs[MSF_MAXM];           // the pool: lives as long as the fp32 state (qexhip_release_workspace frees both)
  MsfScal *m = nullptr;
  double *r2k = nullptr;                          // MSF_MAXM device scalars: |b - A_k x_k|^2 of phase 2
};

void msf_state_free(qexhip_ctx *c) {
  MsfState *S = (MsfState *)c->msf32;
  if (!S) return;
  for (auto &f : S->ps) if (f.d) (void)hipFree(f.d);
  for (auto &f : S->xs) if (f.d) (void)hipFree(f.d);
  if (S->m) (void)hipFree(S->m);
  if (S->r2k) (void)hipFree(S->r2k);
  delete S;
  c->msf32 = nullptr;
}

static inline size_t body4(const qexhip_ctx *c) { return (size_t)c->g.ntile * 96; }     // float4 per parity body
static inline int grid4(size_t n4) { return (int)std::max<size_t>(1, std::min<size_t>((n4 + 255) / 256, 2048)); }

// r_s := b / sigma0, ps_k := r_s, xs_k := 0 for every shift  (cgm.nim:165-207; r := b and x_k := 0 are the host's fp64 copies)
__global__ void __launch_bounds__(256) k_msf_start(float4 *rs, const double2 *__restrict__ b, size_t n4, const MsfScal *__restrict__ m,
                                                   const SlpScal *__restrict__ s) {
  const double sg = s->sigma;                     // k_slp_init: |b| (1 for a zero source)
  const double inv = 1.0 / sg;
  const int nm = m->nmass;
  for (size_t i = blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const double2 b0 = b[2 * i], b1 = b[2 * i + 1];
    const f4n v = {(float)(inv * b0.x), (float)(inv * b0.y), (float)(inv * b1.x), (float)(inv * b1.y)};
    ((f4n *)rs)[i] = v;
    for (int k = 0; k < nm; k++) {
      ((gf4 *)m->ps[k])[i] = v;
      ((gf4 *)m->xs[k])[i] = f4n{0.f, 0.f, 0.f, 0.f};
    }
  }
}
__global__ void k_msf_init(MsfScal *m, const SlpScal *s) { m->sigma0 = s->sigma; }

// alpha = r2 / <p,Ap>; r_s -= alpha Ap_s; xs_0 += alpha ps_0; |r_s|^2 partials in double (k_slp_update's arithmetic).  Behind a
// reliable update (conv) r_s is first rebuilt from the fp64 residual, r_s = r / sigma0.
__global__ void __launch_bounds__(256) k_msf_base(float4 *xs0, float4 *rs, const float4 *__restrict__ p, const float4 *__restrict__ Ap,
                                                  const double2 *__restrict__ r, size_t n4, const SlpScal *__restrict__ s,
                                                  const MsfScal *__restrict__ m, const double *__restrict__ dotp, int ndot,
                                                  double *partials) {
  if (s->done) return;
  const double pAp = cg_sum_parts(dotp, ndot);
  const double sg0 = m->sigma0, inv = 1.0 / sg0;
  const double r2 = s->r2s * (s->sigma * s->sigma) / (sg0 * sg0);          // |r_s|^2 in the vectors' units
  const float alpha = (pAp != 0.0) ? (float)(r2 / pAp) : 0.f;
  const bool conv = s->conv;
  double acc = 0;
  for (size_t i = blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    float4 rv;
    if (conv) {
      const double2 r0 = r[2 * i], r1 = r[2 * i + 1];
      rv = make_float4((float)(inv * r0.x), (float)(inv * r0.y), (float)(inv * r1.x), (float)(inv * r1.y));
    } else {
      rv = rs[i];
    }
    const float4 pv = p[i], av = Ap[i];
    float4 xv = xs0[i];
    xv.x = fmaf(alpha, pv.x, xv.x); xv.y = fmaf(alpha, pv.y, xv.y); xv.z = fmaf(alpha, pv.z, xv.z); xv.w = fmaf(alpha, pv.w, xv.w);
    rv.x = fmaf(-alpha, av.x, rv.x); rv.y = fmaf(-alpha, av.y, rv.y); rv.z = fmaf(-alpha, av.z, rv.z); rv.w = fmaf(-alpha, av.w, rv.w);
    xs0[i] = xv; rs[i] = rv;
    acc = fma((double)rv.x, (double)rv.x, fma((double)rv.y, (double)rv.y, acc));
    acc = fma((double)rv.z, (double)rv.z, fma((double)rv.w, (double)rv.w, acc));
  }
  const double t = block_sum_256(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// One workgroup closes the iteration.  (1) k_cgm_close: alpha, beta and the zeta recurrences of cgm.nim:253-266 in double, thread k
// owns shift k; `pending` tells the following k_msf_update that this iteration is live -- its xs_k += alpha zr ps_k runs even when
// the loop condition (here: the iteration limit) has turned false, and a later, dead pass through this kernel clears the flag.
// (2) k_slp_close: the new |r_s|^2 and whether a reliable update is due -- r2 < delta^2 max r2 since the last one, or the fp32
// residual says converged, or the iteration limit is reached; a pending update stays pending until it runs.
__global__ void __launch_bounds__(256) k_msf_close(SlpScal *s, MsfScal *m, const double *parts, int nparts, const double *dotp, int ndot,
                                                   double delta2) {
  if (s->done) {
    if (threadIdx.x == 0) m->pending = 0;
    return;
  }
  const double r2n = cg_sum_parts(parts, nparts);                          // |r_s|^2, the vectors' units
  const double pAp = cg_sum_parts(dotp, ndot);
  const double sg0 = m->sigma0, sg = s->sigma;
  const double u = (sg * sg) / (sg0 * sg0);                                // the scalars' unit^2 in the vectors'
  const double r2i = s->r2s * u;
  const double alpha = (pAp != 0.0) ? r2i / pAp : 0.0;
  const double beta = (r2i != 0.0) ? r2n / r2i : 0.0;
  const int itn = s->k + 1;
  const int cont = itn < s->maxits;
  const double alphaim1 = m->alphaim1, betaim1 = m->betaim1;
  const int nm = m->nmass;
  const double r2s_old = s->r2s, maxr2s = s->maxr2s, r2stop = s->r2stop;
  const int upd = s->upd;
  __syncthreads();   // every thread holds the old state before anyone overwrites it
  const int k = threadIdx.x;
  if (k >= 1 && k < nm) {
    double zip1d = alpha * betaim1 * (m->zim1[k] - m->zi[k]);
    zip1d += m->zim1[k] * alphaim1 * (1.0 + m->sg[k] * alpha);
    const double zip1 = (zip1d != 0.0) ? m->zi[k] * m->zim1[k] * alphaim1 / zip1d : 0.0;
    const double zr = (m->zi[k] != 0.0) ? zip1 / m->zi[k] : 0.0;
    m->axz[k] = (float)(alpha * zr);
    m->zip1[k] = (float)zip1;
    m->bzz[k] = (float)(beta * zr * zr);
    if (cont) { m->zim1[k] = m->zi[k]; m->zi[k] = zip1; }
  }
  if (k == 0) {
    m->cont = cont; m->pending = 1;
    m->alpha = (float)alpha; m->beta = (float)beta;
    m->alphaim1 = alpha; m->betaim1 = beta;
    const double r2 = r2n / u;                                             // in units of sigma, as k_slp_close keeps it
    s->k = itn;
    s->r2s_old = r2s_old; s->sigma_p = sg;
    s->r2s = r2;
    const double mx = fmax(maxr2s, r2);
    s->maxr2s = mx;
    const int due = r2 < delta2 * mx || r2 * sg * sg <= r2stop || itn >= s->maxits;
    s->upd = upd || due;
    s->noupd = !(upd || due);
    s->conv = 0; s->first = 0;
  }
}

// The hot kernel: xs_k += axz_k ps_k; ps_k = zip1_k r_s + bzz_k ps_k (k >= 1); ps_0 = r_s + beta ps_0 -- one float4 of r_s per
// lane, read once, then 2 x 16-byte loads and stores per shift.  The coefficients and field pointers are the same for the whole
// grid: they sit behind a const __restrict__ kernel argument at addresses that depend on k alone, i.e. scalar loads, once per
// wavefront and shift.  ps_k / xs_k are re-read by the next iteration (and ps_0 by the sweep): plain loads and stores.
__global__ void __launch_bounds__(256) k_msf_update(const f4n *__restrict__ rs, size_t n4, const MsfScal *__restrict__ m) {
  if (!m->pending) return;
  const int cont = m->cont, nm = m->nmass;
  const float beta = m->beta;
  for (size_t i = blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const f4n rv = rs[i];
    if (cont) {
      gf4 *p0 = (gf4 *)m->ps[0];
      p0[i] = fma4(beta, p0[i], rv);
    }
#pragma unroll 2
    for (int k = 1; k < nm; k++) {
      gf4 *pk = (gf4 *)m->ps[k];
      gf4 *xk = (gf4 *)m->xs[k];
      const float axz = m->axz[k], z = m->zip1[k], b = m->bzz[k];
      const f4n pv = pk[i];
      xk[i] = fma4(axz, pv, xk[i]);
      if (cont) pk[i] = fma4(b, pv, z * rv);
    }
  }
}

// reliable update, part 1, for ALL shifts (blockIdx.y): x_k += sigma0 xs_k, xs_k = 0  (no-op unless an update is due)
__global__ void __launch_bounds__(256) k_msf_flush(size_t n4, const SlpScal *__restrict__ s, const MsfScal *__restrict__ m) {
  if (!s->upd || s->done) return;
  const double sg = m->sigma0;
  gd2 *x = (gd2 *)m->x[blockIdx.y];
  gf4 *xs = (gf4 *)m->xs[blockIdx.y];
  for (size_t i = blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const f4n v = xs[i];
    d2n o0 = x[2 * i], o1 = x[2 * i + 1];
    o0.x = fma(sg, (double)v.x, o0.x); o0.y = fma(sg, (double)v.y, o0.y);
    o1.x = fma(sg, (double)v.z, o1.x); o1.y = fma(sg, (double)v.w, o1.y);
    x[2 * i] = o0; x[2 * i + 1] = o1;
    xs[i] = f4n{0.f, 0.f, 0.f, 0.f};
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------
static MsfState *msf_of(qexhip_ctx *c) {
  if (!c->msf32) c->msf32 = new MsfState();
  return (MsfState *)c->msf32;
}

// nmass device scalars for the per-shift residual norms of phase 2
int msf_r2_buffer(qexhip_ctx *c, double **dev) {
  MsfState *S = msf_of(c);
  if (!S->r2k) HIPCHK(hipMalloc((void **)&S->r2k, sizeof(double) * MSF_MAXM));
  *dev = S->r2k;
  return 0;
}

// Start of phase 1, behind slp_init (SlpScal holds b2 and sigma = |b|): the fp32 pool at the current geometry, the recurrences'
// start values (cgm.nim:176-195), r_s = ps_k = b / sigma0, xs_k = 0.  *ps0 <- the base system's search direction (the sweep's input).
int msf_start(qexhip_ctx *c, SlpScal *s, DevFieldF &rs, const DevField &b, std::vector<DevField *> &xs, const double *shifts, int nmass,
              int parity, DevFieldF **ps0) {
  MsfState *S = msf_of(c);
  if (!S->m) HIPCHK(hipMalloc((void **)&S->m, sizeof(MsfScal)));
  for (int k = 0; k < nmass; k++) {
    CHK(f32_field_ensure(c, S->ps[k]));
    CHK(f32_field_ensure(c, S->xs[k]));
  }
  static_assert(sizeof(MsfScal) <= 4096, "MsfScal must fit the pinned scratch page");
  MsfScal *hm = (MsfScal *)c->pinned;
  memset(hm, 0, sizeof(*hm));
  hm->nmass = nmass; hm->cont = 1; hm->pending = 0;
  hm->alphaim1 = -1.0; hm->betaim1 = 0.0;
  hm->sigma0 = 1.0;
  for (int k = 0; k < nmass; k++) {
    hm->sg[k] = (k == 0) ? 0.0 : shifts[k];
    hm->zi[k] = 1.0; hm->zim1[k] = 1.0;
    hm->ps[k] = (float4 *)S->ps[k].par(parity);
    hm->xs[k] = (float4 *)S->xs[k].par(parity);
    hm->x[k] = xs[k]->par(parity);
  }
  HIPCHK(hipMemcpyAsync(S->m, hm, sizeof(*hm), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));            // the pinned page is reused by the state read-backs
  const size_t n4 = body4(c);
  k_msf_init<<<1, 1, 0, c->stream>>>(S->m, s);
  k_msf_start<<<grid4(n4), 256, 0, c->stream>>>((float4 *)rs.par(parity), b.par(parity), n4, S->m, s);
  HIPCHK(hipGetLastError());
  *ps0 = &S->ps[0];
  return 0;
}

// One fp32 iteration behind the sweep (Ap = A ps_0, ndot <p,Ap> partials in c->partials): base, close, update of all shifts.  Sharded,
// both sets of partials are summed over the ranks first, as slp_update does, so every rank computes the same alpha, beta, zeta_k and
// the same `upd` flag (the INVARIANT above slp_update, dslash_f32.hip).
int msf_iterate(qexhip_ctx *c, SlpScal *s, DevFieldF &rs, const DevFieldF &Ap, const DevField &r, int parity, int ndot) {
  MsfState *S = msf_of(c);
  const size_t n4 = body4(c);
  const int nb = grid4(n4);
  double *r2p = c->partials + c->part2_off;
  if (ndot > 0) CHK(comm_allreduce_parts(c, c->partials, ndot, &ndot));
  CHK(devjoin_flush(c));              // (no-op when the all-reduce has taken the second sweep's join with it)
  {
    ScopedTimer tm(c, "blas", c->stream);
    k_msf_base<<<nb, 256, 0, c->stream>>>((float4 *)S->xs[0].par(parity), (float4 *)rs.par(parity), (const float4 *)S->ps[0].par(parity),
                                          (const float4 *)Ap.par(parity), r.par(parity), n4, s, S->m, c->partials, ndot, r2p);
    HIPCHK(hipGetLastError());
  }
  int nr2 = nb;
  CHK(comm_allreduce_parts(c, r2p, nb, &nr2));
  {
    ScopedTimer tm(c, "reduce", c->stream);
    k_msf_close<<<1, 256, 0, c->stream>>>(s, S->m, r2p, nr2, c->partials, ndot, SLP_DELTA * SLP_DELTA);
    HIPCHK(hipGetLastError());
  }
  ScopedTimer tm(c, "cgm_update_f32", c->stream);
  k_msf_update<<<nb, 256, 0, c->stream>>>((const f4n *)rs.par(parity), n4, S->m);
  HIPCHK(hipGetLastError());
  return 0;
}

// reliable update, part 1: every shift's increment into its fp64 solution (gated on `upd`)
int msf_flush(qexhip_ctx *c, SlpScal *s, int nmass) {
  MsfState *S = msf_of(c);
  const size_t n4 = body4(c);
  k_msf_flush<<<dim3(grid4(n4), nmass), 256, 0, c->stream>>>(n4, s, S->m);
  HIPCHK(hipGetLastError());
  return 0;
}
