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

// ---- the packed form (RECON 4): 100 B per link -------------------------------------------------------------------------------
// Every real of a near-unitary matrix lies in (-2, 2) and almost every one above 2^-15: bits 62..56 of such a double (the top
// seven exponent bits) are 0111111 and carry nothing, 84 constant bits in rows 0,1.  The residuals of row 2 live there, 19 bits
// wide (fewer escapes than int16).  Per (parity, tile, dir) row:
//   u64     slot[6][64][2]    rows 0,1 in the order of the rows above (slot 2i = the real, 2i+1 = the imaginary part of element i,
//                             one 16-byte load): the IEEE bits with bits 62..56 replaced by 7 payload bits; the real is
//                             (slot & ~(0x7F << 56)) | (0x3F << 56)
//   u32     extra[64]         at double2 offset 384
// = 400 double2 = 100 B per link.  Residual k_j (signed, |k| <= 262143): bits 0..6 = payload of slot 2j, 7..13 = payload of slot
// 2j+1, 14..18 = extra bits [5j, 5j+5); extra bits 30, 31 are zero.  Row 2 is lr_apply(rec_j, k_j) on the rebuild lr_rebuild of
// the decoded rows 0,1: the residual format's bits.  Masks and header as above (one lossless form is live per context); an
// escaped lane reads the WHOLE link from the 18 reals.
#define LP_ROW 400          // double2 per (tile, dir) row
#define LP_EXTRA 384        // double2 offset of extra in a row
#define LP_KMAX 262143
#define LP_PAY (0x7Full << 56)
#define LP_EXP (0x3Full << 56)

// the real a slot holds / whether a real fits a slot: 2^-15 <= |v| < 2
__host__ __device__ __forceinline__ double lp_real(uint64_t slot) { return lr_double((slot & ~LP_PAY) | LP_EXP); }
__host__ __device__ __forceinline__ bool lp_fits(double v) { return (lr_bits(v) & LP_PAY) == LP_EXP; }

// slots + extra + sign -> the link u[9]
__host__ __device__ __forceinline__ void lp_decode(const uint64_t s[12], uint32_t extra, bool neg, double2 u[9]) {
  int k[6];
#pragma unroll
  for (int j = 0; j < 6; j++) {
    const uint32_t v = (uint32_t)(s[2 * j] >> 56 & 0x7f) | (uint32_t)(s[2 * j + 1] >> 56 & 0x7f) << 7 | (extra >> (5 * j) & 31u) << 14;
    k[j] = (int)(v << 13) >> 13;                      // sign-extend 19 bits
  }
#pragma unroll
  for (int j = 0; j < 6; j++) u[j] = make_double2(lp_real(s[2 * j]), lp_real(s[2 * j + 1]));
  double rec[6];
  lr_rebuild(u, neg, rec);
#pragma unroll
  for (int j = 0; j < 3; j++) u[6 + j] = make_double2(lr_apply(rec[2 * j], k[2 * j]), lr_apply(rec[2 * j + 1], k[2 * j + 1]));
}

// A full link u[9] -> sign, slots and extra.  Returns true when the link decodes back to u bit for bit in all 18 reals; false
// (escaped) otherwise: a real of rows 0,1 outside the window, |k| > 262143, or anything lr_encode escapes.  Sign rule of lr_encode.
__host__ __device__ __forceinline__ bool lp_encode(const double2 u[9], bool *neg, uint64_t s[12], uint32_t *extra) {
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
  bool ok = true;
  uint32_t ex = 0;
#pragma unroll
  for (int j = 0; j < 6; j++) {
    ok = ok && lp_fits(u[j].x) && lp_fits(u[j].y);
    const double sc = lr_double(lr_bits(rec[j]) & 0x7ff0000000000000ull) * 0x1p-52;
    const double q = sc > 0 ? (row2[j] - rec[j]) / sc : 0.0;
    const int k = fabs(q) <= (double)LP_KMAX ? (int)rint(q) : 0;  // (false for a NaN q too)
    const uint32_t v = (uint32_t)k & 0x7ffffu;
    s[2 * j] = (lr_bits(u[j].x) & ~LP_PAY) | (uint64_t)(v & 0x7f) << 56;
    s[2 * j + 1] = (lr_bits(u[j].y) & ~LP_PAY) | (uint64_t)(v >> 7 & 0x7f) << 56;
    ex |= (v >> 14) << (5 * j);
  }
  double2 d[9];
  lp_decode(s, ex, ng, d);
#pragma unroll
  for (int j = 0; j < 9; j++) ok = ok && lr_bits(d[j].x) == lr_bits(u[j].x) && lr_bits(d[j].y) == lr_bits(u[j].y);
  *neg = ng;
  *extra = ex;
  return ok;
}

// ---- the orthogonal form (RECON 5): 92 B per link ----------------------------------------------------------------------------
// Rows 0,1 of a near-unitary link are orthogonal: a0 conj(b0) + a1 conj(b1) + a2 conj(b2) = 0 up to a few ulp, so row 1's last
// element b2 is rebuilt like row 2 -- a fixed-order expression of the stored reals plus a residual in ulp of it -- and only
// a0, a1, a2, b0, b1 are stored.  Per (parity, tile, dir) row:
//   u64     slot[5][64][2]    a0, a1, a2, b0, b1 as in the packed form (slot 2i = the real, 2i+1 = the imaginary part of element i)
//   u64     ex_lo[64]         at double2 offset 320
//   u32     ex_hi[64]         at double2 offset 352
// = 368 double2 = 92 B per link.  166 payload bits: residuals k0..k5 of row 2 (signed 20 bits, |k| <= 524287) and k6, k7 of
// Re b2, Im b2 (signed 23 bits, |k| <= 4194303):
//   k_j, j < 5   bits 0..6 = payload of slot 2j, 7..13 = payload of slot 2j+1, 14..19 = ex_hi bits [6j, 6j+6)
//   k5           bits 0..1 = ex_hi bits 30, 31, bits 2..19 = ex_lo bits 46..63
//   k6, k7       ex_lo bits 0..22 and 23..45
// (b2 needs the slots and ex_lo only.)  Decode order: the ten reals; rec(b2) = conj(-s conj(a2) / |a2|^2), s = a0 conj(b0) + a1 conj(b1),
// in ONE fixed order with two IEEE divisions; b2 = lr_apply(rec(b2), k6 | k7); row 2 = lr_apply on lr_rebuild of the now complete
// rows 0,1: the residual format's bits, so k0..k5 are the packed form's residuals.  Masks, header and escapes as in the packed form.
#define LO_ROW 368          // double2 per (tile, dir) row
#define LO_EXLO 320         // double2 offset of ex_lo in a row
#define LO_EXHI 352         // double2 offset of ex_hi
#define LO_K2MAX 524287     // row 2: 20 bits
#define LO_KBMAX 4194303    // b2: 23 bits

// the rebuild of b2 from a0, a1, a2, b0, b1 (u[0..4]): rec[0] = Re, rec[1] = Im
__host__ __device__ __forceinline__ void lo_rebuild_b2(const double2 u[5], double rec[2]) {
#pragma clang fp contract(off)
  double sx = u[0].x * u[3].x;
  sx = fma(u[0].y, u[3].y, sx);
  sx = fma(u[1].x, u[4].x, sx);
  sx = fma(u[1].y, u[4].y, sx);
  double sy = u[0].y * u[3].x;
  sy = fma(-u[0].x, u[3].y, sy);
  sy = fma(u[1].y, u[4].x, sy);
  sy = fma(-u[1].x, u[4].y, sy);
  double tx = sx * u[2].x;              // t = s conj(a2)
  tx = fma(sy, u[2].y, tx);
  double ty = sy * u[2].x;
  ty = fma(-sx, u[2].y, ty);
  double n = u[2].x * u[2].x;
  n = fma(u[2].y, u[2].y, n);
  rec[0] = -tx / n;                     // conj(b2) = -t / n
  rec[1] = ty / n;
}

// slots + ex_lo + ex_hi + sign -> the link u[9]
__host__ __device__ __forceinline__ void lo_decode(const uint64_t s[10], uint64_t exlo, uint32_t exhi, bool neg, double2 u[9]) {
#pragma unroll
  for (int j = 0; j < 5; j++) u[j] = make_double2(lp_real(s[2 * j]), lp_real(s[2 * j + 1]));
  double rb[2];
  lo_rebuild_b2(u, rb);
  u[5] = make_double2(lr_apply(rb[0], (int)((uint32_t)exlo << 9) >> 9), lr_apply(rb[1], (int)((uint32_t)(exlo >> 23) << 9) >> 9));
  int k[6];
#pragma unroll
  for (int j = 0; j < 5; j++) {
    const uint32_t v = (uint32_t)(s[2 * j] >> 56 & 0x7f) | (uint32_t)(s[2 * j + 1] >> 56 & 0x7f) << 7 | (exhi >> (6 * j) & 63u) << 14;
    k[j] = (int)(v << 12) >> 12;                      // sign-extend 20 bits
  }
  k[5] = (int)((int64_t)exlo >> 46) * 4 + (int)(exhi >> 30);
  double rec[6];
  lr_rebuild(u, neg, rec);
#pragma unroll
  for (int j = 0; j < 3; j++) u[6 + j] = make_double2(lr_apply(rec[2 * j], k[2 * j]), lr_apply(rec[2 * j + 1], k[2 * j + 1]));
}

// the residual of v against rec in ulp(rec), 0 when it does not fit |k| <= kmax (the round trip then fails)
__host__ __device__ __forceinline__ int lo_residual(double v, double rec, int kmax) {
  const double sc = lr_double(lr_bits(rec) & 0x7ff0000000000000ull) * 0x1p-52;
  const double q = sc > 0 ? (v - rec) / sc : 0.0;
  return fabs(q) <= (double)kmax ? (int)rint(q) : 0;  // (false for a NaN q too)
}

// A full link u[9] -> sign, slots, ex_lo and ex_hi.  Returns true when the link decodes back to u bit for bit in all 18 reals;
// false (escaped) otherwise: a stored real outside the window, a residual out of range, a zero / subnormal / non-finite rebuilt
// value (|a2| = 0 among them): the one check covers them all.  Sign rule of lr_encode.
__host__ __device__ __forceinline__ bool lo_encode(const double2 u[9], bool *neg, uint64_t s[10], uint64_t *exlo, uint32_t *exhi) {
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
  double rb[2];
  lo_rebuild_b2(u, rb);
  uint64_t lo = (uint64_t)((uint32_t)lo_residual(u[5].x, rb[0], LO_KBMAX) & 0x7fffffu) |
                (uint64_t)((uint32_t)lo_residual(u[5].y, rb[1], LO_KBMAX) & 0x7fffffu) << 23;
  uint32_t hi = 0;
#pragma unroll
  for (int j = 0; j < 6; j++) {
    const uint32_t v = (uint32_t)lo_residual(row2[j], rec[j], LO_K2MAX) & 0xfffffu;
    if (j < 5) {
      s[2 * j] = (lr_bits(u[j].x) & ~LP_PAY) | (uint64_t)(v & 0x7f) << 56;
      s[2 * j + 1] = (lr_bits(u[j].y) & ~LP_PAY) | (uint64_t)(v >> 7 & 0x7f) << 56;
      hi |= (v >> 14) << (6 * j);
    } else {
      hi |= (v & 3u) << 30;
      lo |= (uint64_t)(v >> 2) << 46;
    }
  }
  double2 d[9];
  lo_decode(s, lo, hi, ng, d);
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 9; j++) ok = ok && lr_bits(d[j].x) == lr_bits(u[j].x) && lr_bits(d[j].y) == lr_bits(u[j].y);
  *neg = ng;
  *exlo = lo;
  *exhi = hi;
  return ok;
}
