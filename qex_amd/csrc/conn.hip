// conn.hip -- the connected scalar correlator from point sources on resident fields: the point sources, the accumulation of the
// translated |propagator|^2 into a complex site field, and the staggered sign.
//
//   k_point_source  eta_k := 0, then 1 + 0i in colour ic[k] at the GLOBAL coordinate pt[k], k < n <= 4
//                   (`pointSource` of src/observables/conn4d.nim:173-182)
//   k_conn_accum    Re locmes(x) += scal * |phi_k(x (+) pt_k)|^2, one k after the other (conn4d.nim:223-229 with `translate`
//                   :184-195: `newShifter(r, mu, 1)` applied pt[mu] times, and a forward shift reads the site s + mu,
//                   src/layout/shiftX.nim:76-81, so the source point lands on the origin); (+) wraps over the GLOBAL extents
//   k_conn_w / k_conn_add   the same in two steps on a t-sharded lattice: w_k(y) = scal * |phi_k(y)|^2 on the rank's own slab,
//                   then Re locmes(x) += w_k(x (+) pt_k) from the gathered slabs
//   k_stag_sign     locmes(x) *= (-1)^(x0+x1+x2), both components (conn4d.nim:238-245)
//
// locmes is the cfield of trace.hip (its imaginary part is never touched by the accumulation); est[t] of the reference is the Re
// column of cfield_slices.
//
// Gather index: with c = ((t Z + z) Y + y) Xh + xh (site_coord) the site x (+) pt has the parity p ^ (sum pt & 1) -- every global
// extent is even, so a wrap keeps the parity -- and its checkerboard number follows from the four wrapped coordinates; no table.
//
// Order of the arithmetic, the same on every path: n2 = the fma chain of k_trace_accum's a == b branch, w = scal * n2, acc += w,
// the n terms one at a time in ascending k, every operation rounded as written (no contraction).  w passes through memory
// unchanged on the sharded path, so n systems in one launch leave the bits of n launches with one system each, and every rank's
// slab equals the one-rank result bit for bit.
//
// Sharded translation: rank r needs w on the global slices [toff + pt_t, toff + pt_t + Xt) mod NT, which lie on at most two
// consecutive ranks.  The n w-fields of a call (8 B per site each, not the 48 B vector) go through ONE comm_allgather; its cost on
// the peer transport is the N - 1 ring passes a hand-made ring would need, and the gathered copy is 8 n B per GLOBAL site.
#pragma clang fp contract(off)
#include "qexhip_internal.h"
#include "site_index.h"

namespace {

struct PointArgs {
  double2 *dst[2][4];   // [parity][k]
  int pt[4][4], ic[4];  // pt: x, y, z and the LOCAL t (outside [0, Xt) on a rank that does not own the point)
};

// one lane per site (both parities): every body site of every destination is written
__global__ void __launch_bounds__(256) k_point_source(Geom g, PointArgs A, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * g.Vh) return;
  int p, c; linear_site(g, i, p, c);
  const SiteXYZT s = site_coord(g, c, p);
  const int x = 2 * s.xh + s.o;
  for (int k = 0; k < n; k++) {
    const bool on = A.pt[k][0] == x && A.pt[k][1] == s.y && A.pt[k][2] == s.z && A.pt[k][3] == s.t;
#pragma unroll
    for (int col = 0; col < 3; col++) A.dst[p][k][vec_off(c, col)] = make_double2(on && col == A.ic[k] ? 1.0 : 0.0, 0.0);
  }
}

struct ConnArgs {
  const double2 *phi[2][4];   // [parity][k]
  int pt[4][4];               // global coordinates of the source points
};

__device__ __forceinline__ double site_norm2(const double2 *a, int c) {
  double re = 0.0;
#pragma unroll
  for (int col = 0; col < 3; col++) {
    const double2 x = a[vec_off(c, col)];
    re = fma(x.x, x.x, fma(x.y, x.y, re));
  }
  return re;
}

// parity (returned) and number *cs, within the lattice of extents (X0, X1, X2, nt), of the site (s, tg) (+) pt
__device__ __forceinline__ int translated(const Geom &g, const SiteXYZT &s, int p, int tg, int nt, const int *pt, int *cs, int *ts) {
  const int x = wrap(2 * s.xh + s.o + pt[0], g.X[0]), y = wrap(s.y + pt[1], g.X[1]), z = wrap(s.z + pt[2], g.X[2]);
  *ts = wrap(tg + pt[3], nt);
  *cs = (z * g.X[1] + y) * g.Xh + (x >> 1);     // without the slice: the caller adds t F
  return p ^ ((pt[0] + pt[1] + pt[2] + pt[3]) & 1);
}

// one rank: gather straight from the propagators
__global__ void __launch_bounds__(256) k_conn_accum(Geom g, ConnArgs A, int n, double scal, double2 *tr0, double2 *tr1) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * g.Vh) return;
  int p, c; linear_site(g, i, p, c);
  const SiteXYZT s = site_coord(g, c, p);
  double *tr = &((p ? tr1 : tr0) + c)->x;
  double acc = *tr;
  for (int k = 0; k < n; k++) {
    int cs, ts;
    const int ps = translated(g, s, p, s.t, g.X[3], A.pt[k], &cs, &ts);
    const double n2 = site_norm2(A.phi[ps][k], ts * g.F + cs);
    const double w = scal * n2;
    acc += w;
  }
  *tr = acc;
}

// sharded, step 1: w[k][p Vh + c] = scal |phi_k|^2 on the rank's own sites
__global__ void __launch_bounds__(256) k_conn_w(Geom g, ConnArgs A, int n, double scal, double *w) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * g.Vh) return;
  int p, c; linear_site(g, i, p, c);
  for (int k = 0; k < n; k++) {
    const double n2 = site_norm2(A.phi[p][k], c);
    w[(size_t)k * g.V + i] = scal * n2;
  }
}

// sharded, step 2: all[rank][k][p Vh + c] holds every rank's w; toff = the first global t of this rank, nt the global extent
__global__ void __launch_bounds__(256) k_conn_add(Geom g, ConnArgs A, int n, int toff, int nt, const double *all, double2 *tr0, double2 *tr1) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * g.Vh) return;
  int p, c; linear_site(g, i, p, c);
  const SiteXYZT s = site_coord(g, c, p);
  double *tr = &((p ? tr1 : tr0) + c)->x;
  double acc = *tr;
  for (int k = 0; k < n; k++) {
    int cs, ts;
    const int ps = translated(g, s, p, s.t + toff, nt, A.pt[k], &cs, &ts);
    const int r = ts / g.X[3], tl = ts - r * g.X[3];
    const double w = all[((size_t)r * n + k) * g.V + (size_t)ps * g.Vh + tl * g.F + cs];
    acc += w;
  }
  *tr = acc;
}

__global__ void __launch_bounds__(256) k_stag_sign(Geom g, double2 *tr0, double2 *tr1) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * g.Vh) return;
  int p, c; linear_site(g, i, p, c);
  const SiteXYZT s = site_coord(g, c, p);
  if ((s.o + s.y + s.z) & 1) {          // x0 = 2 xh + o
    double2 *d = (p ? tr1 : tr0) + c;
    const double2 e = *d;
    *d = make_double2(-e.x, -e.y);
  }
}

}  // namespace

int conn_point_source(qexhip_ctx *c, int n, DevField *const *dst, const int *pts, const int *ic) {
  const Geom &g = c->g;
  const int toff = g.X[3] * c->rankCoord[3];
  PointArgs A{};
  for (int k = 0; k < n; k++) {
    A.dst[0][k] = dst[k]->par(0);
    A.dst[1][k] = dst[k]->par(1);
    for (int mu = 0; mu < 4; mu++) A.pt[k][mu] = pts[4 * k + mu];
    A.pt[k][3] -= toff;
    A.ic[k] = ic[k];
  }
  ScopedTimer tm(c, "trace", c->stream);
  k_point_source<<<(2 * g.Vh + 255) / 256, 256, 0, c->stream>>>(g, A, n);
  HIPCHK(hipGetLastError());
  return 0;
}

int conn_accum(qexhip_ctx *c, DevCField &tr, int n, DevField *const *phi, const int *pts, double scal) {
  const Geom &g = c->g;
  ConnArgs A{};
  for (int k = 0; k < n; k++) {
    A.phi[0][k] = phi[k]->par(0);
    A.phi[1][k] = phi[k]->par(1);
    for (int mu = 0; mu < 4; mu++) A.pt[k][mu] = pts[4 * k + mu];
  }
  const int nblk = (2 * g.Vh + 255) / 256, N = c->rankGeom[3];
  if (N == 1) {
    ScopedTimer tm(c, "trace", c->stream);
    k_conn_accum<<<nblk, 256, 0, c->stream>>>(g, A, n, scal, tr.par(0), tr.par(1));
    HIPCHK(hipGetLastError());
    return 0;
  }
  const size_t per = (size_t)n * g.V;
  CHK(ensure_stage(c, (1 + (size_t)N) * per * sizeof(double)));
  double *w = (double *)c->stage, *all = w + per;
  {
    ScopedTimer tm(c, "trace", c->stream);
    k_conn_w<<<nblk, 256, 0, c->stream>>>(g, A, n, scal, w);
    HIPCHK(hipGetLastError());
  }
  CHK(comm_allgather(c, w, all, per));
  ScopedTimer tm(c, "trace", c->stream);
  k_conn_add<<<nblk, 256, 0, c->stream>>>(g, A, n, g.X[3] * c->rankCoord[3], g.X[3] * N, all, tr.par(0), tr.par(1));
  HIPCHK(hipGetLastError());
  return 0;
}

int cfield_stag_sign(qexhip_ctx *c, DevCField &f) {
  ScopedTimer tm(c, "trace", c->stream);
  k_stag_sign<<<(2 * c->g.Vh + 255) / 256, 256, 0, c->stream>>>(c->g, f.par(0), f.par(1));
  HIPCHK(hipGetLastError());
  return 0;
}
