// hisq_md.hip -- the two kernels of the resident HISQ molecular dynamics (qexhip_md_hisq_*; the state and the calls are smear.hip's).
//
// Restates fermionForce of the HISQ HMC (src/examples/hisqhmc.nim:496-539) around its smearedForce:
//   :512-526  f1[mu](x) = sum_k s_k p_k(x) (x) p_k(x+mu)^+,  f3[mu](x) the same with x+3mu,  odd sites *= -1     (k_outer13)
//   :531-537  f[mu](x) = projectTAH(ff[mu](x) u[mu](x)^+)   and   updateMomentum (:558-560)  p -= dtau f           (k_projtah_kick)
#include "qexhip_internal.h"
#include "site_index.h"
#include "su3.h"
#include <algorithm>

typedef double hm_d2v __attribute__((ext_vector_type(2)));

struct Outer13Args {
  const double2 *x0[4], *x1[4];   // parity halves of up to four resident vectors
  double se[4], so[4];            // their scales on even / odd sites (so = -se: the odd-site sign)
  int n;
};

// One wavefront per (tile, mu): a workgroup is the four directions of one tile of 64 sites, lane = site, so every store of a matrix
// element is one 1 KiB row of the chain's layout F[parity][tile][mu][9][64].  The hop-1 and the hop-3 products of all the
// vectors are summed in registers and CF, CL are written once (non-temporal: the reverse chain reads them in a later kernel).
// Each term is formed exactly as k_outer (force.hip) forms it and the terms are added in ascending k, the first one assigned
// (accumulate: onto what the fields hold, for the launches after the first four vectors): the bits of 2n k_outer launches.
template <bool HALO>
__global__ void __launch_bounds__(256) k_outer13(Geom g, Outer13Args A, double2 *CF, double2 *CL, int accumulate) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, mu = threadIdx.x >> 6;
  const int p = blockIdx.x >= (unsigned)g.ntile, tile = blockIdx.x - p * g.ntile;
  const int c = tile * 64 + lane;
  if (c >= g.Vh) return;
  const SiteXYZT s = site_coord(g, c, p);
  const int pos1 = nbr_pos<HALO>(g, c, s, mu, 1), pos3 = nbr_pos<HALO>(g, c, s, mu, 3);
  double2 *w1 = CF + (((size_t)p * g.etile + tile) * 4 + mu) * 576 + lane;
  double2 *w3 = CL + (((size_t)p * g.etile + tile) * 4 + mu) * 576 + lane;
  double2 f1[9], f3[9];
  if (accumulate) {
#pragma unroll
    for (int e = 0; e < 9; e++) { f1[e] = w1[e * 64]; f3[e] = w3[e * 64]; }
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (k >= A.n) break;
    const double2 *xs = p ? A.x1[k] : A.x0[k];       // this parity
    const double2 *xn = p ? A.x0[k] : A.x1[k];       // the neighbours' parity
    const double sc = p ? A.so[k] : A.se[k];
    double2 a[3], b1[3], b3[3];
#pragma unroll
    for (int q = 0; q < 3; q++) { a[q] = xs[vec_off(c, q)]; b1[q] = xn[vec_off(pos1, q)]; b3[q] = xn[vec_off(pos3, q)]; }
    const bool first = k == 0 && !accumulate;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int q = 0; q < 3; q++) {
        // k_outer's arithmetic as compiled: re = fma(ax, bx, ay by), im = fma(bx, ay, -(ax by)), one rounding for the scale, one for the sum
        const double2 v1 = make_double2(sc * fma(a[r].x, b1[q].x, a[r].y * b1[q].y), sc * fma(b1[q].x, a[r].y, -(a[r].x * b1[q].y)));
        const double2 v3 = make_double2(sc * fma(a[r].x, b3[q].x, a[r].y * b3[q].y), sc * fma(b3[q].x, a[r].y, -(a[r].x * b3[q].y)));
        const int e = r * 3 + q;
        if (first) { f1[e] = v1; f3[e] = v3; }
        else { f1[e].x = v1.x + f1[e].x; f1[e].y = v1.y + f1[e].y; f3[e].x = v3.x + f3[e].x; f3[e].y = v3.y + f3[e].y; }
      }
  }
#pragma unroll
  for (int e = 0; e < 9; e++) {
    __builtin_nontemporal_store((hm_d2v){f1[e].x, f1[e].y}, (hm_d2v *)&w1[e * 64]);
    __builtin_nontemporal_store((hm_d2v){f3[e].x, f3[e].y}, (hm_d2v *)&w3[e * 64]);
  }
}

// CF (:= | +=) sum_k scale_k x_k (x) x_k(+mu)^+ and CL the same with +3mu, odd sites negated, for n >= 1 resident vectors: launches of
// four (option "hisq_md_fused" bit 0; 0: the 2n stag_outer_dev launches they replace, the A/B of profiles/hisq_md_measure.py)
int hisq_outer13_dev(qexhip_ctx *c, int n, DevField *const *xs, const double *scale, double2 *CF, double2 *CL, int accumulate) {
  const Geom &g = c->g;
  if (!(c->opt_hisq_md_fused & 1)) {
    for (int k = 0; k < n; k++) {
      CHK(stag_outer_dev(c, *xs[k], CF, scale[k], -scale[k], accumulate || k > 0, 1));
      CHK(stag_outer_dev(c, *xs[k], CL, scale[k], -scale[k], accumulate || k > 0, 3));
    }
    return 0;
  }
  if (g.halo) {
    if (g.depth < 3) { qexhip_set_error("outer product with hop 3 on a sharded field needs the Naik operator's ghost depth (set the links first)"); return -3; }
    for (int k = 0; k < n; k++)
      for (int par = 0; par < 2; par++) CHK(comm_halo_exchange(c, *xs[k], par, 0));     // x(s + mu), x(s + 3 mu) across the slab boundary
  }
  ScopedTimer tm(c, "outer", c->stream);
  for (int k0 = 0; k0 < n; k0 += 4) {
    Outer13Args A;
    A.n = std::min(4, n - k0);
    for (int j = 0; j < 4; j++) {
      const int k = k0 + std::min(j, A.n - 1);       // unused slots repeat the last vector: never read
      A.x0[j] = xs[k]->par(0); A.x1[j] = xs[k]->par(1);
      A.se[j] = scale[k]; A.so[j] = -scale[k];
    }
    const int acc = accumulate || k0 > 0;
    if (g.halo) k_outer13<true><<<2 * g.ntile, 256, 0, c->stream>>>(g, A, CF, CL, acc);
    else k_outer13<false><<<2 * g.ntile, 256, 0, c->stream>>>(g, A, CF, CL, acc);
    HIPCHK(hipGetLastError());
  }
  return 0;
}

// f = TAH(F u^+) stored over F (what k_force_projtah stores there) and p += t f in the same pass over the body link tiles:
// one read of F, u and p and one write of f and p instead of k_force_projtah followed by k_links_axpy re-reading f
__global__ void __launch_bounds__(256) k_projtah_kick(size_t nlinks_tiles, double2 *F, const double2 *__restrict__ G, double2 *P, double t,
                                                      size_t ntile4, size_t etile4) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t tile = j >> 6;
  if (tile >= nlinks_tiles) return;
  const size_t o = body_tile_off(tile, ntile4, etile4) + (j & 63);
  const M3 f = m3_tah(m3_mul_na(m3_load(F + o, 64), m3_load(G + o, 64)));
  m3_store(F + o, 64, f);
#pragma unroll
  for (int k = 0; k < 9; k++) {
    double2 a = P[o + k * 64];
    a.x = fma(t, f.e[k].x, a.x); a.y = fma(t, f.e[k].y, a.y);
    P[o + k * 64] = a;
  }
}

// F <- TAH(F G^+), then P += t F on the resident momenta P (option "hisq_md_fused" bit 1; 0: the two launches it replaces)
int hisq_projtah_kick_dev(qexhip_ctx *c, double2 *F, const double2 *G, double2 *P, double t) {
  const Geom &g = c->g;
  ScopedTimer tm(c, "projtah_kick", c->stream);
  if (!(c->opt_hisq_md_fused & 2)) {
    CHK(force_projtah_dev(c, F, G, 0));
    return md_kick_dev(c, F, t);
  }
  const size_t ltiles = (size_t)2 * g.ntile * 4;
  k_projtah_kick<<<(unsigned)((ltiles * 64 + 255) / 256), 256, 0, c->stream>>>(ltiles, F, G, P, t, (size_t)g.ntile * 4, (size_t)g.etile * 4);
  HIPCHK(hipGetLastError());
  return 0;
}
