// link_residual.h -- the lossless 108-byte link format of the 8-link Dslash (layout.hip encodes, dslash.hip decodes, the host
// entry qexhip_link_residual_host runs the same functions on the CPU).
//
// A link that is unitary up to rounding has row 2 = +-conj(row0 x row1) to a few ulp.  Per (parity, tile, dir) row:
//   double2 rows01[6][64]                      rows 0,1 exactly (as format 1)
//   u64     res_lo[64]                         residuals k0..k3 of row 2 (int16 each, k0 in the low bits)
//   u32     res_hi[64]                         residuals k4,k5
// = 432 double2 = 108 B per link, plus two u64 per row in a separate array: the sign mask (bit = lane: row 2 rebuilds with -)
// and the escape mask (bit = lane: row 2 is read from the 18-real copy W instead).  That array is [parity][2 + rows][2]: each
// parity's block starts with a 16-byte header whose first word is the address of the parity's half of W.  Real j of row 2 (re/im of columns 0..2) is
//   row2_j = rec_j + k_j * ulp(rec_j),   ulp(rec_j) = 2^(exponent(rec_j) - 52)
// with rec = +-conj(row0 x row1) computed in ONE fixed order of explicit multiplies and fmas, so that the encoder, the host and
// every sweep produce the same bits; a link is escaped unless decode(encode(U)) == U bit for bit (the encoder checks exactly
// that), so the format reproduces the 18-real operator exactly.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>

#define LR_ROW 432          // double2 per (tile, dir) row
#define LR_RES 384          // double2 offset of res_lo in a row; res_hi follows 512 B later (32 double2)

__host__ __device__ __forceinline__ uint64_t lr_bits(double x) { return __builtin_bit_cast(uint64_t, x); }
__host__ __device__ __forceinline__ double lr_double(uint64_t b) { return __builtin_bit_cast(double, b); }

// +-conj(row0 x row1) from rows 0,1 (u[0..5]): one plain multiply and three fmas per real, in this order on every target
__host__ __device__ __forceinline__ void lr_rebuild(const double2 u[6], bool neg, double rec[6]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int a = (k + 1) % 3, b = (k + 2) % 3;
    double rx = u[a].x * u[3 + b].x;
    rx = fma(-u[a].y, u[3 + b].y, rx);
    rx = fma(-u[b].x, u[3 + a].x, rx);
    rx = fma(u[b].y, u[3 + a].y, rx);
    double ry = u[b].x * u[3 + a].y;
    ry = fma(u[b].y, u[3 + a].x, ry);
    ry = fma(-u[a].x, u[3 + b].y, ry);
    ry = fma(-u[a].y, u[3 + b].x, ry);
    rec[2 * k] = neg ? -rx : rx;
    rec[2 * k + 1] = neg ? -ry : ry;
  }
}

// rec + k * ulp(rec): the scale is rec's exponent bits times 2^-52 (0 for a zero or subnormal rec)
__host__ __device__ __forceinline__ double lr_apply(double rec, int k) {
  const double sc = lr_double(lr_bits(rec) & 0x7ff0000000000000ull) * 0x1p-52;
  return fma((double)k, sc, rec);
}

// row 2 (r2[0..2]) from rows 0,1, the sign and the packed residuals
__host__ __device__ __forceinline__ void lr_decode(const double2 u[6], bool neg, uint64_t lo, uint32_t hi, double2 r2[3]) {
  double rec[6];
  lr_rebuild(u, neg, rec);
  const int k[6] = {(int16_t)lo, (int16_t)(lo >> 16), (int16_t)(lo >> 32), (int16_t)(lo >> 48), (int16_t)hi, (int16_t)(hi >> 16)};
#pragma unroll
  for (int j = 0; j < 3; j++) r2[j] = make_double2(lr_apply(rec[2 * j], k[2 * j]), lr_apply(rec[2 * j + 1], k[2 * j + 1]));
}

// A full link u[9] -> sign and packed residuals.  Returns true when the link decodes back to u bit for bit; false (escaped)
// otherwise -- |k| > 32767, a zero / subnormal / non-finite rebuilt value, an inexact difference: the one check covers them all.
// The sign is that of Re <rec, row2> (the format-1 rule).
__host__ __device__ __forceinline__ bool lr_encode(const double2 u[9], bool *neg, uint64_t *lo, uint32_t *hi) {
  double rec[6];
  lr_rebuild(u, false, rec);
  double px = 0;
#pragma unroll
  for (int j = 0; j < 3; j++) px += u[6 + j].x * rec[2 * j] + u[6 + j].y * rec[2 * j + 1];
  const bool ng = px < 0;
  if (ng) {
#pragma unroll
    for (int j = 0; j < 6; j++) rec[j] = -rec[j];
  }
  const double row2[6] = {u[6].x, u[6].y, u[7].x, u[7].y, u[8].x, u[8].y};
  int k[6];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; j++) {
    const double sc = lr_double(lr_bits(rec[j]) & 0x7ff0000000000000ull) * 0x1p-52;
    const double q = sc > 0 ? (row2[j] - rec[j]) / sc : 0.0;
    k[j] = fabs(q) <= 32767.0 ? (int)rint(q) : 0;  // (false for a NaN q too)
    ok = ok && lr_bits(lr_apply(rec[j], k[j])) == lr_bits(row2[j]);
  }
  if (!ok) {
#pragma unroll
    for (int j = 0; j < 6; j++) k[j] = 0;
  }
  *neg = ng;
  *lo = (uint64_t)(uint16_t)k[0] | (uint64_t)(uint16_t)k[1] << 16 | (uint64_t)(uint16_t)k[2] << 32 | (uint64_t)(uint16_t)k[3] << 48;
  *hi = (uint32_t)(uint16_t)k[4] | (uint32_t)(uint16_t)k[5] << 16;
  return ok;
}
