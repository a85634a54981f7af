// dslash_lowp.h -- THE reduced-precision Dslash sweep of the mixed-precision CGs: one per-site body for the single-system sweep
// (k_dslash_lowp), one for the lock-step batch (k_dslash_mrhs_lowp), one host sweep each, over a storage description St that says how
// a site vector and a hop pair's links lie in HBM.  Arithmetic is fp32 in both storages (dslash_f32_core.h); the storages are
//   StoreF32   float2 v[tile][3][64] fields and the float4 link copy          (formats: top of dslash_f32.hip)
//   StoreHalf  one 16-byte element per site and the int16 link copy           (formats: top of dslash_half.hip)
// dslash_f32.hip, dslash_half.hip, batch_f32.hip and batch_half.hip instantiate these for their storage and keep what is theirs alone:
// the link encoders, the BLAS and bookkeeping kernels.  The hosts that drive the sweeps are one per form over the same St: the
// lock-step batch in batch_lowp.h, the single-system loop in solver.cpp.
//
// The operator: out = sgn * (sgn*cb*xs + sum_mu [U in(+mu) - U^+ in(-mu)])  (k_dslash's arithmetic with ca = 0, post = 1): one lane per
// site, 64-site tiles, links streamed non-temporally with 16-byte loads, fp32 FMAs -- mv3f<false> on the forward link, then mv3f<true>
// on the backward one, hop pairs in ascending order --, the final *= sgn, the site written in its storage, <xs,out> partials in
// double from the values as stored.  In 16-bit storage the links are integer-valued and one scale s norm_nbr / 32767^2 per hop goes
// on the neighbour's unpacked 3-vector; fp32 storage has no such scale, and none exists in its instantiations.
//   HALO = false  the whole lattice on one GPU (t-hops wrap)
//   HALO = true   a t-sharded slab (or a one-rank context with a halo): t-hops that leave the slab read the ghost zones (nbr_pos<true>),
//                 over the site range [c0,c1) plus [d0,d1) for workgroups >= nb1 (both faces in one launch), as k_dslash<.., HALO, ..>.
//                 Both kernels have it; the lock-step one writes each system's partials from a per-launch offset, and its host sweep
//                 (sweep_mrhs) runs on such a context under option "batch_ranks" only.
// Every site runs the same operations in the same order whatever HALO is and whether it is alone or one of a batch -- only the positions
// its t-hops read differ --, because there is one body: a slab's output is the one-rank operator's bits site for site, and a system
// solved in a batch returns the bits it returns alone.
//
// A neighbour is read in two steps around the link fetch, St::issue before it and St::take behind it, so that each storage keeps the
// statement order it was tuned with: fp32 issues nothing and loads behind the fetch; 16-bit issues its 16-byte loads ahead of the
// fetch and unpacks behind it.  (Moving the fp32 loads ahead of the fetch changed the code of every fp32 instantiation.)
//
// The kernels' gfx950 code is, instruction for instruction, that of the four kernels these bodies replace
// (profiles/lowp_refactor_resources.txt).  What that took, each found by compiling it the other way:
//   - an access (St::read, St::take) is one colour in fp32 storage and the whole site in 16-bit storage, St::NK accesses per site, and
//     the loop over them stands in the kernel body: the fp32 code changes when that loop moves into the storage, the 16-bit code when
//     it unpacks colour by colour;
//   - around the single-system kernel's St::read there is no loop at all where NK = 1 (a loop of one trip there changed 24 of the 32
//     16-bit instantiations; around St::take, inside the hop loop, and in the lock-step kernel it changes none);
//   - St::write takes the sign with it (fp32: multiply and store colour by colour; 16-bit: multiply, then pack), and the 16-bit one
//     takes the output pointer by reference, so that it is loaded behind pack_site as `out[c] = pack_site(..)` does;
//   - the two neighbours of a hop are two St::Nbr, not one record: arrays of a record in the lock-step kernel became loop-carried.
#pragma once
#include "qexhip_internal.h"
#include "site_index.h"
#include "reduce.h"
#include "dslash_half_core.h"
#include <cstring>
#include <type_traits>

// ---- the two storages ------------------------------------------------------------------------------------------------------------
struct StoreF32 {
  using Elem = float2;
  using Field = DevFieldF;
  using LinkBase = f4v;
  template <int NDIR, int RECON> using Cursor = LinkCursorF<NDIR, RECON>;
  static constexpr size_t WIRE = 3 * sizeof(float2);     // bytes per site in a face exchange
  static constexpr const char *T_SWEEP = "dslash_f32", *T_BND = "dslash_f32_bnd", *T_BATCH = "dslash_batch_f32",
                              *T_BATCH_BND = "dslash_batch_f32_bnd";
  static constexpr int NK = 3;                           // an access (read, take) is one colour
  struct Scales {};                                      // no hop scales: nothing in the kernel arguments, nothing in the code
  struct Nbr {};                                         // nothing is in flight across the link fetch
  template <int RECON> static __device__ __forceinline__ Scales hop_scales(const Scales &) { return {}; }
  static __device__ __forceinline__ void read(const float2 *f, const int c, const int k, float2 v[3]) { v[k] = f[vec_off(c, k)]; }
  static __device__ __forceinline__ void write(float2 *f, const int c, float2 v[3], const float sgn) {      // v <- sgn v, stored
#pragma unroll
    for (int k = 0; k < 3; k++) {
      v[k].x *= sgn; v[k].y *= sgn;
      f[vec_off(c, k)] = v[k];
    }
  }
  static __device__ __forceinline__ Nbr issue(const float2 *, const int) { return {}; }
  static __device__ __forceinline__ void take(const float2 *in, const int pf, const int pb, const Nbr &, const Nbr &, const Scales &,
                                              const int, const int k, float2 vf[3], float2 vb[3]) {
    vf[k] = in[vec_off(pf, k)]; vb[k] = in[vec_off(pb, k)];
  }
  // what a sweep on output parity `parity` reads of the current copy (f32_links has run)
  static int links(qexhip_ctx *c, int parity, const f4v **W, const unsigned long long **S, Scales *, int *fmt) {
    const void *Wv = nullptr;
    CHK(f32_links_dev(c, parity, &Wv, S, fmt));
    *W = (const f4v *)Wv;
    return 0;
  }
};

struct StoreHalf {
  using Elem = u4v;
  using Field = DevFieldH;
  using LinkBase = void;
  template <int NDIR, int RECON> using Cursor = LinkCursorH<NDIR, RECON>;
  static constexpr size_t WIRE = sizeof(u4v);
  static constexpr const char *T_SWEEP = "dslash_half", *T_BND = "dslash_half_bnd", *T_BATCH = "dslash_batch_half",
                              *T_BATCH_BND = "dslash_batch_half_bnd";
  static constexpr int NK = 1;                           // an access is the whole site
  struct Scales { float s_fat, s_long; };                // format 0: the largest |entry| of the fat / long links
  using Nbr = u4v;                                       // a neighbour's element, loaded ahead of the link fetch
  // per hop: s / 32767^2 for the fat (pairs 0..3) and the long links, to go on the neighbour's norm
  template <int RECON> static __device__ __forceinline__ Scales hop_scales(const Scales &q) {
    return {(RECON == 1 ? 1.f : q.s_fat) * (HQ_INV * HQ_INV), (RECON == 1 ? 1.f : q.s_long) * (HQ_INV * HQ_INV)};
  }
  static __device__ __forceinline__ void read(const u4v *f, const int c, const int, float2 v[3]) { unpack_site(f[c], v, HQ_INV); }
  static __device__ __forceinline__ void write(u4v *const &f, const int c, float2 v[3], const float sgn) {  // v <- sgn v as stored
#pragma unroll
    for (int k = 0; k < 3; k++) { v[k].x *= sgn; v[k].y *= sgn; }
    f[c] = pack_site(v);
  }
  static __device__ __forceinline__ Nbr issue(const u4v *in, const int p) { return in[p]; }
  static __device__ __forceinline__ void take(const u4v *, const int, const int, const Nbr &hf, const Nbr &hb, const Scales &hs,
                                              const int pr, const int, float2 vf[3], float2 vb[3]) {
    const float sc = pr >= 4 ? hs.s_long : hs.s_fat;
    unpack_site(hf, vf, sc);
    unpack_site(hb, vb, sc);
  }
  // (half_links has run; format 1 shares the fp32 copy's sign masks)
  static int links(qexhip_ctx *c, int parity, const void **W, const unsigned long long **S, Scales *q, int *fmt) {
    const HalfState *H = half_state(c);
    if (H->fmt < 0) { qexhip_set_error("internal: 16-bit sweep without its links"); return -3; }
    *fmt = H->fmt;
    const size_t rows = (size_t)parity * c->g.ntile * (c->ndir / 2);          // pair rows before this parity
    *W = (const char *)H->W + rows * (H->fmt == 1 ? 3 * 64 * 16 : HALF_ROW0);
    *S = nullptr;
    if (H->fmt == 1) {
      const void *Wf = nullptr;
      int f32fmt = 0;
      CHK(f32_links_dev(c, parity, &Wf, S, &f32fmt));
      if (f32fmt != 1 || !*S) { qexhip_set_error("internal: the 16-bit links' sign masks are gone"); return -3; }
    }
    q->s_fat = (float)H->s_fat; q->s_long = (float)H->s_long;
    return 0;
  }
};

// (ndir, fmt) -> f(NDIR, RECON) as compile-time constants: the one place the sweeps' link templates are chosen
template <int N> using IntC = std::integral_constant<int, N>;
template <class F>
static inline void with_ndir_recon(int ndir, int fmt, F &&f) {
  if (ndir == 8) { if (fmt == 1) f(IntC<8>(), IntC<1>()); else f(IntC<8>(), IntC<0>()); }
  else { if (fmt == 1) f(IntC<16>(), IntC<1>()); else f(IntC<16>(), IntC<0>()); }
}

// ---- the single-system sweep -----------------------------------------------------------------------------------------------------
template <class St>
struct SweepArgs {
  Geom g;
  const typename St::LinkBase *W;  // links of the output parity
  const unsigned long long *S;     // RECON: sign masks [tile][dir]
  const typename St::Elem *in;
  typename St::Elem *out;
  const typename St::Elem *xs;
  float cb, sgn;
  [[no_unique_address]] typename St::Scales q;
  int parity;
  double *partials;
  const int *done;
};
template <class St>
struct SweepHaloArgs {             // (a type of its own: the HALO = false kernels keep their kernel arguments and code)
  SweepArgs<St> a;
  SweepRanges r;
};
template <class St, bool HALO> using SweepKernelArgs = std::conditional_t<HALO, SweepHaloArgs<St>, SweepArgs<St>>;
template <class St> __device__ __forceinline__ const SweepArgs<St> &sweep_args(const SweepArgs<St> &P) { return P; }
template <class St> __device__ __forceinline__ const SweepArgs<St> &sweep_args(const SweepHaloArgs<St> &P) { return P.a; }

template <class St, int NDIR, bool HALO, bool INIT, bool DOT, int RECON>
__global__ void __launch_bounds__(256) k_dslash_lowp(SweepKernelArgs<St, HALO> P) {
  const SweepArgs<St> &A = sweep_args(P);
  if (A.done && *A.done) return;
  const Geom &g = A.g;
  int c = blockIdx.x * 256 + threadIdx.x, clim = g.Vh;
  if constexpr (HALO) sweep_site(P.r, blockIdx.x, c, clim);
  const bool active = c < clim;
  double dotv = 0;
  if (active) {
    const SiteXYZT s = site_coord(g, c, A.parity);
    const typename St::template Cursor<NDIR, RECON> L(A.W, A.S, c);
    float2 acc[3], xsv[3];
    if (INIT || DOT) {
      if constexpr (St::NK == 1) St::read(A.xs, c, 0, xsv);
      else {
#pragma unroll
        for (int k = 0; k < St::NK; k++) St::read(A.xs, c, k, xsv);
      }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) acc[k] = INIT ? make_float2((A.sgn * A.cb) * xsv[k].x, (A.sgn * A.cb) * xsv[k].y) : make_float2(0.f, 0.f);
    const typename St::Scales hs = St::template hop_scales<RECON>(A.q);
    constexpr int UNR = NDIR == 8 ? 4 : 2;
#pragma unroll UNR
    for (int pr = 0; pr < NDIR / 2; pr++) {
      const int mu = pr & 3;
      const int hop = pr >= 4 ? 3 : 1;
      const int pf = nbr_pos<HALO>(g, c, s, mu, hop);
      const int pb = nbr_pos<HALO>(g, c, s, mu, -hop);
      const typename St::Nbr hf = St::issue(A.in, pf), hb = St::issue(A.in, pb);
      float2 U[9], W[9], vf[3], vb[3];
      L.fetch(pr, U, W);
#pragma unroll
      for (int k = 0; k < St::NK; k++) St::take(A.in, pf, pb, hf, hb, hs, pr, k, vf, vb);
      mv3f<false>(acc, U, vf);
      mv3f<true>(acc, W, vb);
    }
    St::write(A.out, c, acc, A.sgn);
    if (DOT) {
#pragma unroll
      for (int k = 0; k < 3; k++)
        dotv = fma((double)xsv[k].x, (double)acc[k].x, fma((double)xsv[k].y, (double)acc[k].y, dotv));
    }
  }
  if (DOT) {
    const double r = block_sum_256(dotv);
    if (threadIdx.x == 0) A.partials[blockIdx.x] = r;
  }
}

// One launch on stream st, dot partials from A.partials + part_off.  HALO: over [c0,c1) (+ [d0,d1) behind it), nothing where both are
// empty; else over all sites.
template <class St, bool HALO>
static int launch_sweep(qexhip_ctx *c, int fmt, const SweepArgs<St> &A, int c0, int c1, int d0, int d1, bool init, bool dot, int part_off,
                        const char *tname, hipStream_t st) {
  SweepKernelArgs<St, HALO> P;
  memset(&P, 0, sizeof P);
  int nb = (c->g.Vh + 255) / 256;
  if constexpr (HALO) {
    nb = sweep_ranges(P.r, c0, c1, d0, d1);
    if (!nb) return 0;
    P.a = A;
    P.a.partials = A.partials + part_off;
  } else {
    P = A;
  }
  const dim3 grid(nb), block(256);
  ScopedTimer tm(c, tname, st);
  with_ndir_recon(c->ndir, fmt, [&](auto nd, auto rc) {
    constexpr int ND = decltype(nd)::value, R = decltype(rc)::value;
    if (init && dot) hipLaunchKernelGGL((k_dslash_lowp<St, ND, HALO, true, true, R>), grid, block, 0, st, P);
    else if (init) hipLaunchKernelGGL((k_dslash_lowp<St, ND, HALO, true, false, R>), grid, block, 0, st, P);
    else if (dot) hipLaunchKernelGGL((k_dslash_lowp<St, ND, HALO, false, true, R>), grid, block, 0, st, P);
    else hipLaunchKernelGGL((k_dslash_lowp<St, ND, HALO, false, false, R>), grid, block, 0, st, P);
  });
  HIPCHK(hipGetLastError());
  return 0;
}

// One sweep; *nparts <- how many <xs,out> partials it left in c->partials.  With g.halo, in the forms the fp64 sweep chooses between
// (sweep_plan / sweep_form): exchange-first (the faces, St::WIRE bytes per site, on the compute stream, one launch over all sites with
// the one-rank workgroup partition) or split by sites (exchange + both faces' launch on the comm stream, interior launch on the compute
// stream, device-side join).  The fused (self-pushing) form has no reduced-precision kernel: where sweep_form picks it, the sweep is
// split by sites.  dot: the caller's next operation on the compute stream is comm_allreduce_parts (slp_update, slph_iterate), which
// takes the join of a split sweep with it where the mailboxes carry the sum.
template <class St>
static int sweep_lowp(qexhip_ctx *c, typename St::Field &out, typename St::Field &in, int parity, const typename St::Field *xs, double cb,
                      bool neg, bool dot, const int *done, int *nparts) {
  const Geom &g = c->g;
  SweepArgs<St> A;
  memset(&A, 0, sizeof A);
  A.g = g;
  int fmt = 0;
  CHK(St::links(c, parity, &A.W, &A.S, &A.q, &fmt));
  A.in = in.par(1 - parity);
  A.out = out.par(parity);
  A.xs = xs ? xs->par(parity) : nullptr;
  A.cb = (float)cb;
  A.sgn = neg ? -1.f : 1.f;
  A.parity = parity;
  A.partials = c->partials;
  A.done = done;
  const bool init = cb != 0.0;
  c->bnd_out_on_cstream = nullptr;        // (the fp64 sweep's early-exchange shortcut is for a pair of fp64 sweeps only)
  *nparts = (g.Vh + 255) / 256;
  if (!g.halo) return launch_sweep<St, false>(c, fmt, A, 0, 0, 0, 0, init, dot, 0, St::T_SWEEP, c->stream);
  int lo_end, hi_beg, overlap;
  sweep_plan(c, &lo_end, &hi_beg, &overlap);
  CHK(devjoin_flush(c));
  if (!overlap) {
    CHK(comm_halo_exchange_sites(c, in.par(1 - parity), St::WIRE, 0));
    return launch_sweep<St, true>(c, fmt, A, 0, g.Vh, 0, 0, init, dot, 0, St::T_SWEEP, c->stream);
  }
  // split by sites (also where sweep_form(c, overlap) == 2)
  const int nb_int = (hi_beg - lo_end + 255) / 256, nb_lo = (lo_end + 255) / 256, nb_hi = (g.Vh - hi_beg + 255) / 256;
  HIPCHK(hipEventRecord(c->ev_ready, c->stream));
  CHK(comm_halo_exchange_sites(c, in.par(1 - parity), St::WIRE, 1));
  CHK((launch_sweep<St, true>(c, fmt, A, lo_end, hi_beg, 0, 0, init, dot, 0, St::T_SWEEP, c->stream)));
  CHK((launch_sweep<St, true>(c, fmt, A, 0, lo_end, hi_beg, g.Vh, init, dot, nb_int, St::T_BND, c->cstream)));
  CHK(devjoin_signal(c, c->cstream));
  if (dot && c->peer) CHK(devjoin_defer(c));
  else CHK(devjoin_wait(c, c->stream, c->cstream));
  *nparts = nb_int + nb_lo + nb_hi;
  return 0;
}

// r[px] = 4 m2 x - (2D)(2D) x through the work field t (op_xx's two sweeps); dot: <x,r> partials in c->partials[0..*nparts)
template <class St>
static int op_xx_lowp(qexhip_ctx *c, typename St::Field &r, typename St::Field &x, typename St::Field &t, double m2, int par_even, int dot,
                      const int *done, int *nparts) {
  const int px = par_even ? 0 : 1, py = 1 - px;
  int np = 0;
  CHK(sweep_lowp<St>(c, t, x, py, nullptr, 0.0, false, false, done, &np));
  CHK(sweep_lowp<St>(c, r, t, px, &x, 4.0 * m2, true, dot != 0, done, &np));
  if (nparts) *nparts = np;
  return 0;
}

// ---- the lock-step sweep: up to four systems on the same links -------------------------------------------------------------------
template <class St>
struct MrhsArgs {
  Geom g;
  const typename St::LinkBase *W;  // links of the output parity
  const unsigned long long *S;     // RECON: sign masks [tile][dir]
  const typename St::Elem *in[QX_MAXRHS];
  typename St::Elem *out[QX_MAXRHS];
  const typename St::Elem *xs[QX_MAXRHS];
  float cb[QX_MAXRHS];
  double *partials[QX_MAXRHS];
  const SlpScal *st;               // st[j].done switches system j off
  [[no_unique_address]] typename St::Scales q;
  int parity, nrhs;
};

template <class St>
struct MrhsHaloArgs {              // (a type of its own, as SweepHaloArgs: the HALO = false kernels keep their kernel arguments and code)
  MrhsArgs<St> a;
  SweepRanges r;
  int part_off;                    // this launch's first <xs,out> partial of every system
};
template <class St, bool HALO> using MrhsKernelArgs = std::conditional_t<HALO, MrhsHaloArgs<St>, MrhsArgs<St>>;
template <class St> __device__ __forceinline__ const MrhsArgs<St> &mrhs_args(const MrhsArgs<St> &P) { return P; }
template <class St> __device__ __forceinline__ const MrhsArgs<St> &mrhs_args(const MrhsHaloArgs<St> &P) { return P.a; }

// k_dslash_lowp's body per system, the links of a hop pair fetched once and applied to every live system:
// SECOND = false: out_j = +sum_mu (U in_j(+mu) - U^+ in_j(-mu))              (INIT = false, DOT = false, sgn = +1)
// SECOND = true : out_j = cb_j xs_j - sum_mu (...), partial <xs_j, out_j>   (INIT = true,  DOT = true,  sgn = -1)
// with the single-system workgroup partition and the same fixed-order sums.  All systems' neighbours are issued ahead of the link fetch.
// HALO: k_dslash_lowp's -- the site ranges of sweep_site, t-hops through nbr_pos<true>, every system's partials from part_off on, so that
// a split sweep lays them out per system as sweep_lowp does for one: interior, low face, high face.
template <class St, int NDIR, int RECON, bool SECOND, bool HALO>
__global__ void __launch_bounds__(256) k_dslash_mrhs_lowp(MrhsKernelArgs<St, HALO> P) {
  const MrhsArgs<St> &A = mrhs_args(P);
  bool act[QX_MAXRHS];
  bool any = false;
#pragma unroll
  for (int j = 0; j < QX_MAXRHS; j++) { act[j] = j < A.nrhs && !A.st[j].done; any = any || act[j]; }
  if (!any) return;
  const Geom &g = A.g;
  int c = blockIdx.x * 256 + threadIdx.x, clim = g.Vh;
  if constexpr (HALO) sweep_site(P.r, blockIdx.x, c, clim);
  double dotv[QX_MAXRHS] = {0, 0, 0, 0};
  if (c < clim) {
    const SiteXYZT s = site_coord(g, c, A.parity);
    const typename St::template Cursor<NDIR, RECON> L(A.W, A.S, c);
    const float sgn = SECOND ? -1.f : 1.f;
    float2 acc[QX_MAXRHS][3], xsv[QX_MAXRHS][3];
#pragma unroll
    for (int j = 0; j < QX_MAXRHS; j++) {
      if (!act[j]) continue;
      if (SECOND) {
#pragma unroll
        for (int k = 0; k < St::NK; k++) St::read(A.xs[j], c, k, xsv[j]);
      }
#pragma unroll
      for (int k = 0; k < 3; k++)
        acc[j][k] = SECOND ? make_float2((sgn * A.cb[j]) * xsv[j][k].x, (sgn * A.cb[j]) * xsv[j][k].y) : make_float2(0.f, 0.f);
    }
    const typename St::Scales hs = St::template hop_scales<RECON>(A.q);
#pragma unroll 1
    for (int pr = 0; pr < NDIR / 2; pr++) {
      const int mu = pr & 3;
      const int hop = pr >= 4 ? 3 : 1;
      const int pf = nbr_pos<HALO>(g, c, s, mu, hop);
      const int pb = nbr_pos<HALO>(g, c, s, mu, -hop);
      typename St::Nbr hf[QX_MAXRHS], hb[QX_MAXRHS];
#pragma unroll
      for (int j = 0; j < QX_MAXRHS; j++) {
        if (!act[j]) continue;
        hf[j] = St::issue(A.in[j], pf); hb[j] = St::issue(A.in[j], pb);
      }
      float2 U[9], W[9];
      L.fetch(pr, U, W);
#pragma unroll
      for (int j = 0; j < QX_MAXRHS; j++) {
        if (!act[j]) continue;
        float2 vf[3], vb[3];
#pragma unroll
        for (int k = 0; k < St::NK; k++) St::take(A.in[j], pf, pb, hf[j], hb[j], hs, pr, k, vf, vb);
        mv3f<false>(acc[j], U, vf);
        mv3f<true>(acc[j], W, vb);
      }
    }
#pragma unroll
    for (int j = 0; j < QX_MAXRHS; j++) {
      if (!act[j]) continue;
      St::write(A.out[j], c, acc[j], sgn);
      if (SECOND) {
        // xs_j is read AGAIN here rather than kept: 4 x 3 float2 held across the hop loop put the fp32 kernel at 178-184 VGPRs (2 waves/SIMD);
        // read twice it is at 130-136 (3 waves/SIMD), still without scratch.  The same values, so the same dot.
#pragma unroll
        for (int k = 0; k < St::NK; k++) St::read(A.xs[j], c, k, xsv[j]);
#pragma unroll
        for (int k = 0; k < 3; k++)
          dotv[j] = fma((double)xsv[j][k].x, (double)acc[j][k].x, fma((double)xsv[j][k].y, (double)acc[j][k].y, dotv[j]));
      }
    }
  }
  if (SECOND) {
#pragma unroll
    for (int j = 0; j < QX_MAXRHS; j++) {
      if (!act[j]) continue;             // uniform over the grid
      const double r = block_sum_256(dotv[j]);
      if constexpr (HALO) { if (threadIdx.x == 0) A.partials[j][P.part_off + blockIdx.x] = r; }
      else { if (threadIdx.x == 0) A.partials[j][blockIdx.x] = r; }
    }
  }
}

// the links of both sweeps of op_xx on parity px for n systems with states st (A1: the other parity's links, A2: px's); *fmt <- their format
template <class St>
static int mrhs_links(qexhip_ctx *c, int n, int px, const SlpScal *st, MrhsArgs<St> &A1, MrhsArgs<St> &A2, int *fmt) {
  if (c->g.halo && !c->opt_batch_ranks) { qexhip_set_error("internal: lock-step sweep on a lattice with ghost zones"); return -3; }
  for (MrhsArgs<St> *A : {&A1, &A2}) {
    A->g = c->g; A->st = st; A->nrhs = n; A->parity = (A == &A1) ? 1 - px : px;
    CHK(St::links(c, A->parity, &A->W, &A->S, &A->q, fmt));
  }
  return 0;
}

// One launch on stream st, every system's dot partials from A.partials[j] + part_off.  HALO: over [c0,c1) (+ [d0,d1) behind it), nothing
// where both are empty; else over all sites.
template <class St, bool HALO>
static int launch_mrhs(qexhip_ctx *c, int fmt, const MrhsArgs<St> &A, bool second, int c0, int c1, int d0, int d1, int part_off,
                       const char *tname, hipStream_t st) {
  MrhsKernelArgs<St, HALO> P;
  memset(&P, 0, sizeof P);
  int nb = (c->g.Vh + 255) / 256;
  if constexpr (HALO) {
    nb = sweep_ranges(P.r, c0, c1, d0, d1);
    if (!nb) return 0;
    P.a = A;
    P.part_off = part_off;
  } else {
    P = A;
  }
  const dim3 grid(nb), block(256);
  ScopedTimer tm(c, tname, st);
  with_ndir_recon(c->ndir, fmt, [&](auto nd, auto rc) {
    constexpr int ND = decltype(nd)::value, R = decltype(rc)::value;
    if (second) hipLaunchKernelGGL((k_dslash_mrhs_lowp<St, ND, R, true, HALO>), grid, block, 0, st, P);
    else hipLaunchKernelGGL((k_dslash_mrhs_lowp<St, ND, R, false, HALO>), grid, block, 0, st, P);
  });
  HIPCHK(hipGetLastError());
  return 0;
}

// One lock-step sweep; *nparts <- how many <xs,out> partials it left per system (second).  With g.halo (option "batch_ranks"), in the two
// forms of sweep_lowp, chosen by the same sweep_plan: exchange-first (all systems' faces in ONE exchange on the compute stream, one
// launch over the slab with the one-rank workgroup partition) or split by sites (the exchange and both faces' launch on the comm stream,
// the interior launch on the compute stream, device-side join).  There is no fused form: where sweep_form picks it, the sweep is split by
// sites.  The faces of ALL nrhs systems travel every sweep, done or not: `done` lives on the device and the number of messages a rank
// posts must not depend on it.  second: the caller's next operation on the compute stream is comm_allreduce_parts_multi, which takes the
// join of a split sweep with it where the mailboxes carry the sums.
template <class St>
static int sweep_mrhs(qexhip_ctx *c, const MrhsArgs<St> &A, int fmt, bool second, int *nparts = nullptr) {
  const Geom &g = c->g;
  c->bnd_out_on_cstream = nullptr;
  if (nparts) *nparts = (g.Vh + 255) / 256;
  if (!g.halo) return launch_mrhs<St, false>(c, fmt, A, second, 0, 0, 0, 0, 0, St::T_BATCH, c->stream);
  void *halves[QX_MAXRHS];
  for (int j = 0; j < A.nrhs; j++) halves[j] = const_cast<typename St::Elem *>(A.in[j]);
  int lo_end, hi_beg, overlap;
  sweep_plan(c, &lo_end, &hi_beg, &overlap);
  CHK(devjoin_flush(c));
  if (!overlap) {
    CHK(comm_halo_exchange_sites_multi(c, A.nrhs, halves, St::WIRE, 0));
    return launch_mrhs<St, true>(c, fmt, A, second, 0, g.Vh, 0, 0, 0, St::T_BATCH, c->stream);
  }
  const int nb_int = (hi_beg - lo_end + 255) / 256, nb_lo = (lo_end + 255) / 256, nb_hi = (g.Vh - hi_beg + 255) / 256;
  HIPCHK(hipEventRecord(c->ev_ready, c->stream));
  CHK(comm_halo_exchange_sites_multi(c, A.nrhs, halves, St::WIRE, 1));
  CHK((launch_mrhs<St, true>(c, fmt, A, second, lo_end, hi_beg, 0, 0, 0, St::T_BATCH, c->stream)));
  CHK((launch_mrhs<St, true>(c, fmt, A, second, 0, lo_end, hi_beg, g.Vh, nb_int, St::T_BATCH_BND, c->cstream)));
  CHK(devjoin_signal(c, c->cstream));
  if (second && c->peer) CHK(devjoin_defer(c));
  else CHK(devjoin_wait(c, c->stream, c->cstream));
  if (nparts) *nparts = nb_int + nb_lo + nb_hi;
  return 0;
}
