// dslash_half_core.h -- the pieces of the 16-bit storage that the single-system sweep and BLAS (dslash_half.hip) and the lock-step
// batch (batch_half.hip) share: the site format on the device (pack_site / unpack_site), the 16-bit field and link-copy state
// (DevFieldH, HalfState), and LinkCursorH -- the ONE place a 16-bit sweep fetches a hop pair's links.  Types, constants and
// inline device functions only: no device-side state lives here.  The formats are described at the top of dslash_half.hip.
#pragma once
#include "qexhip_internal.h"
#include "dslash_f32_core.h"
#include <cfloat>

typedef unsigned int u2v __attribute__((ext_vector_type(2)));

static constexpr float HQ = 32767.f;
static constexpr float HQ_INV = 1.f / 32767.f;
static constexpr int HALF_ROW0 = 4608;            // bytes of one format-0 pair row

struct HalfStall {   // the stall guard's device state (k_slph_stall)
  double best;       // the smallest true |r|^2 seen
  int seen, nfail, stalled, pad;
};

struct HalfState {
  void *W = nullptr; size_t cap = 0;                 // link copy (capacity in bytes)
  int fmt = -1; unsigned long gen = 0;
  double dev = 0, s_fat = 0, s_long = 0;
  unsigned long long *mx = nullptr;                  // [2]: bits of the largest |entry| of the fat / long links
  DevFieldH f[HALF_NF];
  HalfStall *stall = nullptr;
};

HalfState *half_state(qexhip_ctx *c);            // the context's 16-bit state, made on first use (dslash_half.hip)
int half_field_ensure(qexhip_ctx *c, DevFieldH &F);   // (re)allocates F, zeroed, at the current geometry's size
// x[px] -> the 16-bit format / back to fp64 (the operator probes): raw parity halves, nsite_h sites
int half_from_f64(qexhip_ctx *c, u4v *y, const double2 *x);
int half_to_f64(qexhip_ctx *c, double2 *y, const u4v *x);

static inline size_t nsite_h(const qexhip_ctx *c) { return (size_t)c->g.ntile * 64; }
static inline int grid_sites(size_t n) {      // one lane per site, grid-stride beyond the CG update's 2048 partials
  const size_t nb = (n + 255) / 256;
  return (int)(nb > 2048 ? 2048 : (nb < 1 ? 1 : nb));
}

// ---- the vector format on the device (fp32 arithmetic) ----------------------------------------------------------------
__device__ __forceinline__ float lo16(const unsigned w) { return (float)(int)(short)(w & 0xffffu); }
__device__ __forceinline__ float hi16(const unsigned w) { return (float)((int)w >> 16); }
__device__ __forceinline__ unsigned word16(const float re, const float im) {       // re, im integral, |.| <= 32767
  return ((unsigned)(int)re & 0xffffu) | ((unsigned)(int)im << 16);
}
// v[k] = mult * (stored value of colour k)
__device__ __forceinline__ void unpack_site(const u4v h, float2 v[3], const float mult) {
  const float sc = __uint_as_float(h.w) * mult;
  v[0] = make_float2(lo16(h.x) * sc, hi16(h.x) * sc);
  v[1] = make_float2(lo16(h.y) * sc, hi16(h.y) * sc);
  v[2] = make_float2(lo16(h.z) * sc, hi16(h.z) * sc);
}
// v -> the stored site; v is replaced by the values as stored
__device__ __forceinline__ u4v pack_site(float2 v[3]) {
  float m = fmaxf(fabsf(v[0].x), fabsf(v[0].y));
  m = fmaxf(m, fmaxf(fabsf(v[1].x), fabsf(v[1].y)));
  m = fmaxf(m, fmaxf(fabsf(v[2].x), fabsf(v[2].y)));
  const bool nz = m >= FLT_MIN;
  const float rcp = nz ? 1.f / m : 0.f;
  const float back = nz ? m * HQ_INV : 0.f;
  float q[6];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    q[2 * k] = fminf(fmaxf(rintf((v[k].x * rcp) * HQ), -HQ), HQ);
    q[2 * k + 1] = fminf(fmaxf(rintf((v[k].y * rcp) * HQ), -HQ), HQ);
    v[k] = make_float2(q[2 * k] * back, q[2 * k + 1] * back);
  }
  u4v h;
  h.x = word16(q[0], q[1]); h.y = word16(q[2], q[3]); h.z = word16(q[4], q[5]);
  h.w = __float_as_uint(nz ? m : 0.f);
  return h;
}

template <int NDIR, int RECON>
struct LinkCursorH {
  const char *w;                     // the tile's first pair row
  const unsigned long long *sm;
  int lane;
  __device__ __forceinline__ LinkCursorH(const void *W, const unsigned long long *S, const int c)
      : w((const char *)W + (size_t)(c >> 6) * (NDIR / 2) * (RECON == 1 ? 3 * 64 * 16 : HALF_ROW0)),
        sm(RECON == 1 ? S + (size_t)(c >> 6) * NDIR : nullptr), lane(c & 63) {}
  // the pair's links as integer-valued floats (units of s / 32767)
  __device__ __forceinline__ void fetch(const int pr, float2 U[9], float2 Wb[9]) const {
    if (RECON == 1) {
      const u4v *p = (const u4v *)(w + (size_t)pr * (3 * 64 * 16)) + lane;
      u4v t[3];
#pragma unroll
      for (int q = 0; q < 3; q++) t[q] = __builtin_nontemporal_load(&p[q * 64]);
#pragma unroll
      for (int q = 0; q < 12; q++) {
        const unsigned wd = t[q >> 2][q & 3];
        const float2 e = make_float2(lo16(wd), hi16(wd));
        if (q < 6) U[q] = e; else Wb[q - 6] = e;
      }
      recon_row2f(U, (sm[2 * pr] >> lane) & 1ull);
      recon_row2f(Wb, (sm[2 * pr + 1] >> lane) & 1ull);
#pragma unroll
      for (int k = 6; k < 9; k++) {                 // the cross product of two rows in units of 1/32767 is in units of 1/32767^2
        U[k].x *= HQ_INV; U[k].y *= HQ_INV;
        Wb[k].x *= HQ_INV; Wb[k].y *= HQ_INV;
      }
    } else {
      const char *base = w + (size_t)pr * HALF_ROW0;
      const u4v *p = (const u4v *)base + lane;
      u4v t[4];
#pragma unroll
      for (int q = 0; q < 4; q++) t[q] = __builtin_nontemporal_load(&p[q * 64]);
      const u2v t2 = __builtin_nontemporal_load((const u2v *)(base + 4096) + lane);
#pragma unroll
      for (int q = 0; q < 18; q++) {
        const unsigned wd = q < 16 ? t[(q >> 2) & 3][q & 3] : t2[q & 1];
        const float2 e = make_float2(lo16(wd), hi16(wd));
        if (q < 9) U[q] = e; else Wb[q - 9] = e;
      }
    }
  }
};
