// dslash_f32_core.h -- device pieces of the single-precision Dslash sweeps (dslash_f32.hip, batch_f32.hip): the matrix-vector product,
// the row-2 rebuild of the sign format, and LinkCursorF -- the ONE place an fp32 sweep fetches a hop pair's links.  fp32 counterparts
// only: the fp64 pieces are dslash_core.h's.
#pragma once
#include <hip/hip_runtime.h>

typedef float f4v __attribute__((ext_vector_type(4)));

// acc += U v  (SUB = false)  /  acc -= U v  (SUB = true), fp32 FMAs
template <bool SUB>
__device__ __forceinline__ void mv3f(float2 acc[3], const float2 U[9], const float2 v[3]) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const float2 u = U[3 * i + j];
      if (!SUB) {
        acc[i].x = fmaf(u.x, v[j].x, acc[i].x);
        acc[i].x = fmaf(-u.y, v[j].y, acc[i].x);
        acc[i].y = fmaf(u.x, v[j].y, acc[i].y);
        acc[i].y = fmaf(u.y, v[j].x, acc[i].y);
      } else {
        acc[i].x = fmaf(-u.x, v[j].x, acc[i].x);
        acc[i].x = fmaf(u.y, v[j].y, acc[i].x);
        acc[i].y = fmaf(-u.x, v[j].y, acc[i].y);
        acc[i].y = fmaf(-u.y, v[j].x, acc[i].y);
      }
    }
  }
}

// rows 0,1 -> full link, sign format: row 2 = (+-1) conj(row0 x row1)
__device__ __forceinline__ void recon_row2f(float2 U[9], bool neg) {
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int a = (k + 1) % 3, b = (k + 2) % 3;
    float rx = U[a].x * U[3 + b].x;
    rx = fmaf(-U[a].y, U[3 + b].y, rx);
    rx = fmaf(-U[b].x, U[3 + a].x, rx);
    rx = fmaf(U[b].y, U[3 + a].y, rx);
    float ry = U[b].x * U[3 + a].y;
    ry = fmaf(U[b].y, U[3 + a].x, ry);
    ry = fmaf(-U[a].x, U[3 + b].y, ry);
    ry = fmaf(-U[a].y, U[3 + b].x, ry);
    U[6 + k] = make_float2(neg ? -rx : rx, neg ? -ry : ry);
  }
}

// The fp32 links of one hop pair (forward link, backward link) as NL float4 per lane: the pair's complex entries
// [U_f(0..n-1), U_b(0..n-1)] (n = 9 for 18 reals, 6 for rows 0,1) two to a float4.  Unpack into two 3x3 (rows 0,1 only when n = 6).
template <int NL>
__device__ __forceinline__ void unpack_pair(const f4v t[NL], float2 U[9], float2 W[9]) {
  constexpr int n = NL == 9 ? 9 : 6;
#pragma unroll
  for (int q = 0; q < 2 * n; q++) {
    const f4v v = t[q >> 1];
    const float2 e = (q & 1) ? make_float2(v.z, v.w) : make_float2(v.x, v.y);
    if (q < n) U[q] = e; else W[q - n] = e;
  }
}

// The fp32 links of one output site as a sweep reads them (dslash_core.h's LinkCursor for the fp32 copy): built once per site from
// the parity's link base W ([tile][pair][NL][64] float4), its sign masks S ([tile][dir], bit = lane; RECON 1 only) and the site c.
// fetch(pr, ..): the NL float4 of hop pair pr, streamed non-temporally like the fp64 links, as the forward link U and the backward
// link Wb, rebuilt to 3x3.  The single-system and the lock-step batched fp32 sweep both go through here.
template <int NDIR, int RECON>
struct LinkCursorF {
  static constexpr int NL = RECON == 1 ? 6 : 9;      // float4 per lane and pair
  const f4v *w;                      // this lane's element of the site's first pair
  const unsigned long long *sm;      // the tile's sign-mask row (RECON 1)
  int lane;
  __device__ __forceinline__ LinkCursorF(const f4v *W, const unsigned long long *S, const int c)
      : w(W + (size_t)(c >> 6) * (NDIR / 2 * NL * 64) + (c & 63)), sm(RECON == 1 ? S + (size_t)(c >> 6) * NDIR : nullptr), lane(c & 63) {}
  __device__ __forceinline__ void fetch(const int pr, float2 U[9], float2 Wb[9]) const {
    f4v t[NL];
#pragma unroll
    for (int q = 0; q < NL; q++) t[q] = __builtin_nontemporal_load(&w[(size_t)(pr * NL + q) * 64]);
    unpack_pair<NL>(t, U, Wb);
    if (RECON == 1) {
      recon_row2f(U, (sm[2 * pr] >> lane) & 1ull);
      recon_row2f(Wb, (sm[2 * pr + 1] >> lane) & 1ull);
    }
  }
};
