// site_index.h -- checkerboard site <-> coordinate arithmetic shared by all kernels, and which sites a sweep's workgroup owns.
//
// Index convention = QEX V=1 layout (src/layout/qlayout.nim:110-131): lex index with x fastest,
// c = lex/2 within a parity, parity = (x+y+z+t)&1.  Neighbour sense follows the shifts:
// the forward hop of direction mu reads the site s + hop*mu (src/layout/shiftX.nim:76-81).
#pragma once
#include "qexhip_internal.h"

struct SiteXYZT {
  int xh, y, z, t, o;  // x = 2*xh + o
};

__host__ __device__ __forceinline__ SiteXYZT site_coord(const Geom &g, int c, int parity) {
  SiteXYZT s;
  unsigned r = (unsigned)c;
  s.xh = r % (unsigned)g.Xh; r /= (unsigned)g.Xh;
  s.y = r % (unsigned)g.X[1]; r /= (unsigned)g.X[1];
  s.z = r % (unsigned)g.X[2];
  s.t = r / (unsigned)g.X[2];
  s.o = (s.y + s.z + s.t + parity) & 1;
  return s;
}

// linear site i in [0, V) = both parities back to back -> (parity, checkerboard index)
__host__ __device__ __forceinline__ void linear_site(const Geom &g, int i, int &p, int &c) {
  p = i >= g.Vh;
  c = i - p * g.Vh;
}

__host__ __device__ __forceinline__ int wrap(int v, int n) { return v >= n ? v - n : (v < 0 ? v + n : v); }

// position, in the field of the OPPOSITE parity, of the site s + hop*mu (hop = +-1, +-3).
// With g.halo, t-hops that leave the local lattice land in the ghost zones.
template <bool HALO>
__host__ __device__ __forceinline__ int nbr_pos(const Geom &g, int c, const SiteXYZT &s, int mu, int hop) {
  if (mu == 0) {
    int x = 2 * s.xh + s.o;
    int xn = wrap(x + hop, g.X[0]);
    return c - s.xh + (xn >> 1);
  } else if (mu == 1) {
    return c + (wrap(s.y + hop, g.X[1]) - s.y) * g.Xh;
  } else if (mu == 2) {
    return c + (wrap(s.z + hop, g.X[2]) - s.z) * g.Xh * g.X[1];
  } else {
    int tn = s.t + hop;
    if (HALO) {
      // The ghost zones continue the slice numbering: ghost_hi holds the virtual slices
      // t = Xt .. Xt+depth-1 (position t*F + cF, no special case), ghost_lo the virtual slices
      // t = -depth .. -1 stored at t + Xt + 2*depth.  One select, no control flow.  (A three-way
      // select / branch formulation made hipcc hoist the loads of all directions and spill:
      // 256 VGPRs + scratch, 1 wave/SIMD.)
      return c + hop * g.F + (tn < 0 ? (g.X[3] + 2 * g.depth) * g.F : 0);
    } else {
      return c + (wrap(tn, g.X[3]) - s.t) * g.F;
    }
  }
}

// The sites of one sweep launch, 256 per workgroup: [c0, c1) for the logical workgroups below nb1, [d0, d1) for the rest (both t-faces of
// a slab in one launch).  The fused sweep's third range and its boundary roles are fused_sweep.h's (fused_site), over the same numbers.
struct SweepRanges { int c0, c1, d0, d1, nb1; };

// host: fills r; an empty first range gives its place to the second.  Returns the number of workgroups, 0 when there is nothing to do
inline int sweep_ranges(SweepRanges &r, int c0, int c1, int d0, int d1) {
  if (c1 <= c0) { c0 = d0; c1 = d1; d0 = d1 = 0; }
  if (c1 <= c0) return 0;
  r.c0 = c0; r.c1 = c1; r.d0 = d0; r.d1 = d1;
  r.nb1 = (c1 - c0 + 255) / 256;
  return r.nb1 + (d1 > d0 ? (d1 - d0 + 255) / 256 : 0);
}

// device: this lane's site c of logical workgroup lb, and the end clim of its range
__device__ __forceinline__ void sweep_site(const SweepRanges &r, const int lb, int &c, int &clim) {
  c = r.c0 + lb * 256 + threadIdx.x;
  clim = r.c1;
  if (lb >= r.nb1) { c = r.d0 + (lb - r.nb1) * 256 + threadIdx.x; clim = r.d1; }
}
