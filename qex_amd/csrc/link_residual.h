// link_residual.h -- the three lossless link forms of the 8-link Dslash, each described ONCE by a trait LosslessForm<FORM>
// (FORM = c->lres: 1 residual, 108 B per link; 2 packed, 100 B; 3 orthogonal, 92 B).  layout.hip encodes through the trait,
// dslash_core.h decodes through it, the host entries qexhip_link_{residual,packed,ortho}_host run the same functions on the CPU.
// This header is the definition of the formats' bits: the floating-point statements and their order are fixed.
//
// A link that is unitary up to rounding has row 2 = +-conj(row0 x row1) to a few ulp.  Real j of row 2 (re/im of columns 0..2) is
//   row2_j = rec_j + k_j * ulp(rec_j),   ulp(rec_j) = 2^(exponent(rec_j) - 52)
// with rec = +-conj(row0 x row1) computed in ONE fixed order of explicit multiplies and fmas, so that the encoder, the host and
// every sweep produce the same bits; a link is escaped unless decode(encode(U)) == U bit for bit (the encoder checks exactly
// that), so every form reproduces the 18-real operator exactly.  The forms differ in what else they rebuild and where the
// residuals k_j live.
//
// Every form stores a (parity, tile, dir) row of ROW double2: NLOAD x [64] 16-byte words per lane first, then
// the per-lane extra words (LinkExtra: a u64 at double2 offset LO_OFF where the form has one, a u32 at HI_OFF).  Two u64 per row
// live in a separate array: the sign mask (bit = lane: row 2 rebuilds with -) and the escape mask (bit = lane: elements
// [ESC_FIRST, 9) of the link are read from the 18-real copy W instead).  That array is [parity][2 + rows][2]: each parity's block
// starts with a 16-byte header whose first word is the address of the parity's half of W.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>

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

// the residual of v against rec in ulp(rec), 0 when it does not fit |k| <= kmax (the round trip then fails)
__host__ __device__ __forceinline__ int lr_residual(double v, double rec, int kmax) {
  const double sc = lr_double(lr_bits(rec) & 0x7ff0000000000000ull) * 0x1p-52;
  const double q = sc > 0 ? (v - rec) / sc : 0.0;
  return fabs(q) <= (double)kmax ? (int)rint(q) : 0;  // (false for a NaN q too)
}

// row 2 from its rebuild and the residuals k
__host__ __device__ __forceinline__ void lr_row2(const double rec[6], const int k[6], double2 r2[3]) {
#pragma unroll
  for (int j = 0; j < 3; j++) r2[j] = make_double2(lr_apply(rec[2 * j], k[2 * j]), lr_apply(rec[2 * j + 1], k[2 * j + 1]));
}

// The sign rule of every form (the format-1 rule): the sign of Re <rec, row2>.  Returns it, and rec with that sign applied.
__host__ __device__ __forceinline__ bool lr_sign(const double2 u[9], double rec[6]) {
  lr_rebuild(u, false, rec);
  double px = 0;
#pragma unroll
  for (int j = 0; j < 3; j++) px += u[6 + j].x * rec[2 * j] + u[6 + j].y * rec[2 * j + 1];
  const bool ng = px < 0;
  if (ng) {
#pragma unroll
    for (int j = 0; j < 6; j++) rec[j] = -rec[j];
  }
  return ng;
}

// d == u bit for bit in all 18 reals
__host__ __device__ __forceinline__ bool lr_same(const double2 d[9], const double2 u[9]) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 9; j++) ok = ok && lr_bits(d[j].x) == lr_bits(u[j].x) && lr_bits(d[j].y) == lr_bits(u[j].y);
  return ok;
}

// The exponent window of the packed and orthogonal forms.  Every real of a near-unitary matrix lies in (-2, 2) and almost every
// one above 2^-15: bits 62..56 of such a double (the top seven exponent bits) are 0111111 and carry nothing.  A slot is the IEEE
// bits with bits 62..56 replaced by 7 payload bits; element i of the link takes slots 2i (the real part) and 2i+1 (the
// imaginary part), one 16-byte load, and carries 14 bits: the low 7 in slot 2i, the next 7 in slot 2i+1.
#define LP_PAY (0x7Full << 56)
#define LP_EXP (0x3Full << 56)
// the real a slot holds / whether a real fits a slot: 2^-15 <= |v| < 2
__host__ __device__ __forceinline__ double lp_real(uint64_t slot) { return lr_double((slot & ~LP_PAY) | LP_EXP); }
__host__ __device__ __forceinline__ bool lp_fits(double v) { return (lr_bits(v) & LP_PAY) == LP_EXP; }
__host__ __device__ __forceinline__ double2 lp_slots(double2 v, uint32_t pay) {
  return make_double2(lr_double((lr_bits(v.x) & ~LP_PAY) | (uint64_t)(pay & 0x7f) << 56),
                      lr_double((lr_bits(v.y) & ~LP_PAY) | (uint64_t)(pay >> 7 & 0x7f) << 56));
}
__host__ __device__ __forceinline__ uint32_t lp_payload(const uint64_t s[2]) { return (uint32_t)(s[0] >> 56 & 0x7f) | (uint32_t)(s[1] >> 56 & 0x7f) << 7; }

// the per-lane extra words of a row
struct LinkExtra {
  uint64_t lo;
  uint32_t hi;
};

// The sweep kernels' RECON of a lossless form (dslash_core.h: LinkFormat, LinkCursor)
constexpr int lossless_recon(int form) { return form + 2; }

// What a form is.  Constants: RECON; NLOAD, the double2 loaded per lane; ROW, the double2 per (tile, dir) row; BYTES per link;
// LO_OFF / HI_OFF, the double2 offsets of the row's u64 / u32 extra words (LO_OFF < 0: none); ESC_FIRST, the first element an
// escaped lane re-reads from the 18 reals (6: row 2 only, 0: the whole link).
//   encode: a full link u[9] -> sign, words w[NLOAD] and extra words.  Returns true when the link decodes back to u bit for bit;
//           false (escaped) otherwise.
//   decode: words + extra words + sign -> elements [ESC_FIRST, 9) of the link, what the form does not store as it is.  Where that is
//           the whole link, `out` may be `w` itself (the sweep decodes in place): the words are copied out first.
// (A word is a double2 here as in the sweep's registers; the slots of forms 2, 3 are bit patterns that are only ever moved.)
template <int FORM> struct LosslessForm;

// ---- the residual form: 108 B per link --------------------------------------------------------------------------------------
//   double2 rows01[6][64]     rows 0,1 exactly (as format 1)
//   u64     lo[64]            residuals k0..k3 of row 2 (int16 each, k0 in the low bits)
//   u32     hi[64]            residuals k4,k5, 512 B (32 double2) behind lo
// An escaped lane reads row 2 from the 18 reals.
template <> struct LosslessForm<1> {
  static constexpr int RECON = lossless_recon(1), NLOAD = 6, ROW = 432, BYTES = ROW / 4, LO_OFF = 384, HI_OFF = 416, ESC_FIRST = 6;
  static constexpr int KMAX = 32767;

  __host__ __device__ static __forceinline__ void decode(const double2 w[6], const LinkExtra &x, bool neg, double2 r2[3]) {
    double rec[6];
    lr_rebuild(w, neg, rec);
    const int k[6] = {(int16_t)x.lo, (int16_t)(x.lo >> 16), (int16_t)(x.lo >> 32), (int16_t)(x.lo >> 48), (int16_t)x.hi, (int16_t)(x.hi >> 16)};
    lr_row2(rec, k, r2);
  }

  // escaped: |k| > 32767, a zero / subnormal / non-finite rebuilt value, an inexact difference: the one check covers them all
  __host__ __device__ static __forceinline__ bool encode(const double2 u[9], bool *neg, double2 w[6], LinkExtra *x) {
    double rec[6];
    *neg = lr_sign(u, rec);
    const double row2[6] = {u[6].x, u[6].y, u[7].x, u[7].y, u[8].x, u[8].y};
    int k[6];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; j++) {
      k[j] = lr_residual(row2[j], rec[j], KMAX);
      ok = ok && lr_bits(lr_apply(rec[j], k[j])) == lr_bits(row2[j]);
    }
    if (!ok) {
#pragma unroll
      for (int j = 0; j < 6; j++) k[j] = 0;
    }
#pragma unroll
    for (int j = 0; j < 6; j++) w[j] = u[j];
    x->lo = (uint64_t)(uint16_t)k[0] | (uint64_t)(uint16_t)k[1] << 16 | (uint64_t)(uint16_t)k[2] << 32 | (uint64_t)(uint16_t)k[3] << 48;
    x->hi = (uint32_t)(uint16_t)k[4] | (uint32_t)(uint16_t)k[5] << 16;
    return ok;
  }
};

// ---- the packed form: 100 B per link ----------------------------------------------------------------------------------------
// Rows 0,1 have 84 constant bits in their exponent windows.  The residuals of row 2 live there, 19 bits wide (fewer escapes than int16):
//   u64     slot[6][64][2]    rows 0,1 in the order of the rows above
//   u32     hi[64]            at double2 offset 384
// Residual k_j (signed, |k| <= 262143): bits 0..13 = payload of slot pair j, 14..18 = hi bits [5j, 5j+5); hi bits 30, 31 are zero.
// Row 2 is lr_row2 on the rebuild lr_rebuild of the decoded rows 0,1: the residual form's bits.  An escaped lane reads the WHOLE link from the 18 reals.
template <> struct LosslessForm<2> {
  static constexpr int RECON = lossless_recon(2), NLOAD = 6, ROW = 400, BYTES = ROW / 4, LO_OFF = -1, HI_OFF = 384, ESC_FIRST = 0;
  static constexpr int KMAX = 262143;

  __host__ __device__ static __forceinline__ void decode(const double2 w[6], const LinkExtra &x, bool neg, double2 u[9]) {
    uint64_t s[12];
#pragma unroll
    for (int j = 0; j < 6; j++) { s[2 * j] = lr_bits(w[j].x); s[2 * j + 1] = lr_bits(w[j].y); }
    int k[6];
#pragma unroll
    for (int j = 0; j < 6; j++) {
      const uint32_t v = lp_payload(s + 2 * j) | (x.hi >> (5 * j) & 31u) << 14;
      k[j] = (int)(v << 13) >> 13;                      // sign-extend 19 bits
    }
#pragma unroll
    for (int j = 0; j < 6; j++) u[j] = make_double2(lp_real(s[2 * j]), lp_real(s[2 * j + 1]));
    double rec[6];
    lr_rebuild(u, neg, rec);
    lr_row2(rec, k, u + 6);
  }

  // escaped: a real of rows 0,1 outside the window, |k| > 262143, or anything the residual form escapes
  __host__ __device__ static __forceinline__ bool encode(const double2 u[9], bool *neg, double2 w[6], LinkExtra *x) {
    double rec[6];
    *neg = lr_sign(u, rec);
    const double row2[6] = {u[6].x, u[6].y, u[7].x, u[7].y, u[8].x, u[8].y};
    bool ok = true;
    x->lo = 0;
    x->hi = 0;
#pragma unroll
    for (int j = 0; j < 6; j++) {
      ok = ok && lp_fits(u[j].x) && lp_fits(u[j].y);
      const uint32_t v = (uint32_t)lr_residual(row2[j], rec[j], KMAX) & 0x7ffffu;
      w[j] = lp_slots(u[j], v);
      x->hi |= (v >> 14) << (5 * j);
    }
    double2 d[9];
    decode(w, *x, *neg, d);
    return ok && lr_same(d, u);
  }
};

// ---- the orthogonal form: 92 B per link -------------------------------------------------------------------------------------
// Rows 0,1 of a near-unitary link are orthogonal: a0 conj(b0) + a1 conj(b1) + a2 conj(b2) = 0 up to a few ulp, so row 1's last
// element b2 is rebuilt like row 2 -- a fixed-order expression of the stored reals plus a residual in ulp of it -- and only
// a0, a1, a2, b0, b1 are stored:
//   u64     slot[5][64][2]    a0, a1, a2, b0, b1 as in the packed form
//   u64     lo[64]            at double2 offset 320
//   u32     hi[64]            at double2 offset 352
// 166 payload bits: residuals k0..k5 of row 2 (signed 20 bits, |k| <= 524287) and k6, k7 of Re b2, Im b2 (signed 23 bits,
// |k| <= 4194303):
//   k_j, j < 5   bits 0..13 = payload of slot pair j, 14..19 = hi bits [6j, 6j+6)
//   k5           bits 0..1 = hi bits 30, 31, bits 2..19 = lo bits 46..63
//   k6, k7       lo bits 0..22 and 23..45
// (b2 needs the slots and lo only.)  Decode order: the ten reals; rec(b2) = conj(-s conj(a2) / |a2|^2), s = a0 conj(b0) + a1 conj(b1),
// in ONE fixed order with two IEEE divisions; b2 = lr_apply(rec(b2), k6 | k7); row 2 = lr_row2 on lr_rebuild of the now complete rows 0,1: the
// residual form's bits, so k0..k5 are the packed form's residuals.  Escapes as in the packed form.
template <> struct LosslessForm<3> {
  static constexpr int RECON = lossless_recon(3), NLOAD = 5, ROW = 368, BYTES = ROW / 4, LO_OFF = 320, HI_OFF = 352, ESC_FIRST = 0;
  static constexpr int K2MAX = 524287;     // row 2: 20 bits
  static constexpr int KBMAX = 4194303;    // b2: 23 bits

  // the rebuild of b2 from a0, a1, a2, b0, b1 (u[0..4]): rec[0] = Re, rec[1] = Im
  __host__ __device__ static __forceinline__ void rebuild_b2(const double2 u[5], double rec[2]) {
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

  __host__ __device__ static __forceinline__ void decode(const double2 w[5], const LinkExtra &x, bool neg, double2 u[9]) {
    uint64_t s[10];
#pragma unroll
    for (int j = 0; j < 5; j++) { s[2 * j] = lr_bits(w[j].x); s[2 * j + 1] = lr_bits(w[j].y); }
#pragma unroll
    for (int j = 0; j < 5; j++) u[j] = make_double2(lp_real(s[2 * j]), lp_real(s[2 * j + 1]));
    double rb[2];
    rebuild_b2(u, rb);
    u[5] = make_double2(lr_apply(rb[0], (int)((uint32_t)x.lo << 9) >> 9), lr_apply(rb[1], (int)((uint32_t)(x.lo >> 23) << 9) >> 9));
    int k[6];
#pragma unroll
    for (int j = 0; j < 5; j++) {
      const uint32_t v = lp_payload(s + 2 * j) | (x.hi >> (6 * j) & 63u) << 14;
      k[j] = (int)(v << 12) >> 12;                      // sign-extend 20 bits
    }
    k[5] = (int)((int64_t)x.lo >> 46) * 4 + (int)(x.hi >> 30);
    double rec[6];
    lr_rebuild(u, neg, rec);
    lr_row2(rec, k, u + 6);
  }

  // escaped: a stored real outside the window, a residual out of range, a zero / subnormal / non-finite rebuilt value (|a2| = 0
  // among them): the one check covers them all
  __host__ __device__ static __forceinline__ bool encode(const double2 u[9], bool *neg, double2 w[5], LinkExtra *x) {
    double rec[6];
    *neg = lr_sign(u, rec);
    const double row2[6] = {u[6].x, u[6].y, u[7].x, u[7].y, u[8].x, u[8].y};
    double rb[2];
    rebuild_b2(u, rb);
    x->lo = (uint64_t)((uint32_t)lr_residual(u[5].x, rb[0], KBMAX) & 0x7fffffu) |
            (uint64_t)((uint32_t)lr_residual(u[5].y, rb[1], KBMAX) & 0x7fffffu) << 23;
    x->hi = 0;
#pragma unroll
    for (int j = 0; j < 6; j++) {
      const uint32_t v = (uint32_t)lr_residual(row2[j], rec[j], K2MAX) & 0xfffffu;
      if (j < 5) {
        w[j] = lp_slots(u[j], v);
        x->hi |= (v >> 14) << (6 * j);
      } else {
        x->hi |= (v & 3u) << 30;
        x->lo |= (uint64_t)(v >> 2) << 46;
      }
    }
    double2 d[9];
    decode(w, *x, *neg, d);
    return lr_same(d, u);
  }
};
