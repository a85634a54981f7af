// dslash_core.h -- device pieces shared by the fp64 Dslash kernels (dslash.hip, batch.hip) and meson.hip: the matrix-vector
// product, the rebuilds of the compressed link formats (recon_row2; recon_lossless over link_residual.h's traits), and LinkCursor -- the ONE
// place a sweep fetches and rebuilds a hop pair's links
#pragma once
#include <hip/hip_runtime.h>
#include "link_residual.h"

typedef double d2v __attribute__((ext_vector_type(2)));

// acc += U v  (SUB = false)  /  acc -= U v  (SUB = true); every term one v_fma_f64
template <bool SUB>
__device__ __forceinline__ void mv3(double2 acc[3], const double2 U[9], const double2 v[3]) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 3; j++) {
      if (!SUB) {
        acc[i].x += U[3 * i + j].x * v[j].x;
        acc[i].x -= U[3 * i + j].y * v[j].y;
        acc[i].y += U[3 * i + j].x * v[j].y;
        acc[i].y += U[3 * i + j].y * v[j].x;
      } else {
        acc[i].x -= U[3 * i + j].x * v[j].x;
        acc[i].x += U[3 * i + j].y * v[j].y;
        acc[i].y -= U[3 * i + j].x * v[j].y;
        acc[i].y -= U[3 * i + j].y * v[j].x;
      }
    }
  }
}

// rows 0,1 of a link -> full link: row 2 = det * conj(row0 x row1); det = +-1 (format 1) or U[6] (format 2)
template <int FMT>
__device__ __forceinline__ void recon_row2(double2 U[9], bool neg) {
  const double2 ph = U[6];
  double2 r2[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int a = (k + 1) % 3, b = (k + 2) % 3;
    double rx = U[a].x * U[3 + b].x;
    rx -= U[a].y * U[3 + b].y;
    rx -= U[b].x * U[3 + a].x;
    rx += U[b].y * U[3 + a].y;
    double ry = U[b].x * U[3 + a].y;
    ry += U[b].y * U[3 + a].x;
    ry -= U[a].x * U[3 + b].y;
    ry -= U[a].y * U[3 + b].x;
    if (FMT == 1) r2[k] = make_double2(neg ? -rx : rx, neg ? -ry : ry);
    // explicit fma: "a*b - c*d" leaves the compiler two ways to contract, and it chose differently in different kernels
    else r2[k] = make_double2(fma(ph.x, rx, -(ph.y * ry)), fma(ph.x, ry, ph.y * rx));
  }
#pragma unroll
  for (int k = 0; k < 3; k++) U[6 + k] = r2[k];
}

// lossless forms (RECON 3, 4, 5 = LosslessForm<RECON - 2>, link_residual.h): the link whose loaded words are in U[0..NLOAD).  `row` =
// the link's (tile, dir) row, `m` its [sign, escape] masks; an escaped lane re-reads what the form says (row 2, or the whole link)
// from the 18 reals: element `fr` of W's parity half, whose address the header `hdr` of the parity's mask block holds (the
// kernels' argument block stays as it is).  Each mask is read where it is used: hoisted into locals they move registers.
template <int RECON>
__device__ __forceinline__ void recon_lossless(double2 U[9], const double2 *row, const unsigned long long *m, const unsigned long long *hdr,
                                               size_t fr, int lane) {
  typedef LosslessForm<RECON - 2> F;
  LinkExtra x = {0, 0};
  if constexpr (F::LO_OFF >= 0) x.lo = __builtin_nontemporal_load((const uint64_t *)(row + F::LO_OFF) + lane);
  x.hi = __builtin_nontemporal_load((const uint32_t *)(row + F::HI_OFF) + lane);
  // (the whole link: decoded in place; row 2 only: through a temporary that takes the escape too -- written straight into U it moves
  // the RECON 3 kernels' registers)
  constexpr int NOUT = 9 - F::ESC_FIRST;
  double2 tmp[NOUT];
  double2 *o = F::ESC_FIRST ? tmp : U;
  F::decode(U, x, (m[0] >> lane) & 1ull, o);
  if ((m[1] >> lane) & 1ull) {
    const double2 *wf = (const double2 *)(uintptr_t)hdr[0] + fr;
#pragma unroll
    for (int k = 0; k < NOUT; k++) o[k] = wf[(F::ESC_FIRST + k) * 64];
  }
  if constexpr (F::ESC_FIRST > 0) {
#pragma unroll
    for (int k = 0; k < NOUT; k++) U[F::ESC_FIRST + k] = tmp[k];
  }
}

// what a link format stores per link.  RECON 0: 18 reals; 1: rows 0,1 + a sign bit; 2: rows 0,1 + det; 3, 4, 5: the lossless forms
// (link_residual.h).  NLOAD: double2 loaded per lane and link; LROW: double2 per (tile, direction) row (= 4 x the bytes per link)
template <int RECON, bool LOSSLESS = (RECON >= 3)> struct LinkFormat {
  static constexpr int NLOAD = RECON == 1 ? 6 : (RECON == 2 ? 7 : 9);
  static constexpr int LROW = NLOAD * 64;
};
template <int RECON> struct LinkFormat<RECON, true> {
  static constexpr int NLOAD = LosslessForm<RECON - 2>::NLOAD, LROW = LosslessForm<RECON - 2>::ROW;
};

// The links of one output site as a sweep reads them: built once per site from the parity's link base W, its mask base S (RECON 1:
// sign masks [tile][dir], bit = lane; 3, 4, 5: [tile][dir][sign, escape], S[-2] = this parity's 18-real W) and the site c.
// fetch(pr, ..) gives the forward link of hop pair pr (direction 2 pr; fat links: pairs 0..3, 3-hop links: 4..7) in U and the backward
// link (direction 2 pr + 1) in Wb, rebuilt to 3x3: the loads, then rebuild().  The batched sweep (batch.hip) calls it; dslash_body
// (dslash.hip) spells the LOADS out in place, because through the call its RECON 1 / 2 kernels change registers (see there), and calls
// rebuild() itself.
template <int NDIR, int RECON>
struct LinkCursor {
  static constexpr int NLOAD = LinkFormat<RECON>::NLOAD, LROW = LinkFormat<RECON>::LROW;
  const double2 *w;                  // this lane's element of the site's first (tile, direction) row
  const unsigned long long *sm;      // the tile's mask row (RECON 1, 3, 4, 5)
  const unsigned long long *hdr;     // RECON 3, 4, 5: header of the parity's mask block
  int tile, lane;
  __device__ __forceinline__ LinkCursor(const double2 *W, const unsigned long long *S, const int c)
      : w(W + (size_t)(c >> 6) * (NDIR * LROW) + (c & 63)),
        sm(RECON == 1 ? S + (size_t)(c >> 6) * NDIR : (RECON >= 3 ? S + (size_t)(c >> 6) * NDIR * 2 : nullptr)),
        hdr(RECON >= 3 ? S - 2 : nullptr), tile(c >> 6), lane(c & 63) {}
  // do_f / do_b: which of the pair's two links this call takes (literally true on the fast paths)
  __device__ __forceinline__ void fetch(const int pr, const bool do_f, const bool do_b, double2 U[9], double2 Wb[9]) const {
    const double2 *wp = w + (size_t)pr * (2 * LROW);
    // links are read exactly once per sweep: stream them past the caches (non-temporal), which
    // leaves L2 / Infinity Cache to the 8x re-read neighbour vectors.  Measured on MI355X,
    // 32^4: 120 us -> 108 us per sweep (scratch/tune_dslash.py, profiles/r01_tune_dslash.log).
    if (do_f) {
#pragma unroll
      for (int k = 0; k < NLOAD; k++) {
        d2v t = __builtin_nontemporal_load((const d2v *)&wp[k * 64]);
        U[k] = make_double2(t.x, t.y);
      }
    }
    if (do_b) {
#pragma unroll
      for (int k = 0; k < NLOAD; k++) {
        d2v t = __builtin_nontemporal_load((const d2v *)&wp[LROW + k * 64]);
        Wb[k] = make_double2(t.x, t.y);
      }
    }
    rebuild(pr, do_f, do_b, wp, U, Wb);
  }
  // everything after the loads: U / Wb hold the words of the pair's rows at wp / wp + LROW on entry, the 3x3 links on return
  __device__ __forceinline__ void rebuild(const int pr, const bool do_f, const bool do_b, const double2 *wp, double2 U[9], double2 Wb[9]) const {
    if constexpr (RECON == 1) {
      if (do_f) recon_row2<1>(U, (sm[2 * pr] >> lane) & 1ull);
      if (do_b) recon_row2<1>(Wb, (sm[2 * pr + 1] >> lane) & 1ull);
    } else if constexpr (RECON >= 3) {
      // bit for bit the 18-real link; an escaped lane reads it from W
      const size_t fr = ((size_t)tile * NDIR + 2 * pr) * 576 + lane;
      if (do_f) recon_lossless<RECON>(U, wp - lane, sm + 4 * pr, hdr, fr, lane);
      if (do_b) recon_lossless<RECON>(Wb, wp - lane + LROW, sm + 4 * pr + 2, hdr, fr + 576, lane);
    } else if constexpr (RECON == 2) {
      if (do_f) recon_row2<2>(U, false);
      if (do_b) recon_row2<2>(Wb, false);
    }
  }
};

// one link of the operator's storage outside a sweep (meson.hip): `w` points at this lane's element of the (tile, dir) row of W
// (RECON 0: 9 double2) or Wc (RECON 1: rows 0,1; RECON 2: rows 0,1 + det), `sm` at the row's sign mask (RECON 1 only)
template <int RECON>
__device__ __forceinline__ void load_link(double2 U[9], const double2 *w, const unsigned long long *sm, int lane) {
  static_assert(RECON < 3, "the lossless rows are read through LinkCursor only");
#pragma unroll
  for (int k = 0; k < LinkFormat<RECON>::NLOAD; k++) U[k] = w[k * 64];
  if (RECON == 1) recon_row2<1>(U, (*sm >> lane) & 1ull);
  else if (RECON == 2) recon_row2<2>(U, false);
}
