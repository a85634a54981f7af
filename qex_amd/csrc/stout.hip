// stout.hip -- stout smearing: smear, inverse (Luscher's trivialising map by fixed-point iteration) and the force chain.
//
// Restates (file:line in ctpeterson/qex):
//   smear            src/gauge/stoutsmear.nim:15-34      -- one RK stage of the flow (gauge.hip: gauge_stout_stage)
//   inverse          src/gauge/stoutsmear.nim:36-89      -- k_stout_inv + k_stout_sum + k_stout_decide
//   gaugeForceDeriv  src/gauge/stoutsmear.nim:97-146     -- first half in k_stout_link, second half k_stout_stencil
//   smearDeriv       src/gauge/stoutsmear.nim:148-175    -- k_stout_link + k_stout_stencil
//   expm1Deriv       src/maths/matexp.nim:686-713 (scale 20, expm1Poly4Deriv :100-117; matrixFunctions.nim:471-481)
// Layout: the natural links of gauge.hip, G[parity][tile][mu][9][64] double2, ghost tiles behind the body when t is sharded.
//
// What a level keeps (DESIGN.md "Stout smearing"): its input links gf and v = a f (a = -alpha nc, f = TAH(gf ds^+)), which the flow
// stage writes anyway.  exp(a f) is recomputed per link in the backward pass, the staple sum ds in the stencil kernel, whose
// gathers are the staple's own: with A = gf_nu(x), B = gf_mu(x+nu), C = gf_nu(x+mu) and a, b, c the same links of cg, the three
// inserted terms and the staple of the upper half are A (B c^+ + b C^+) + a (B C^+) and A (B C^+): six products, as many as the
// three inserted terms cost one by one.  The same holds for the lower half.
#include "qexhip_internal.h"
#include "../../include/qexhip.h"
#include "reduce.h"
#include "su3.h"
#include "gauge_index.h"
#include <algorithm>
#include <cmath>
#include <utility>

int gauge_stout_stage(qexhip_ctx *c, double2 *Uin, double2 *V, double2 *Uout, double alpha);        // gauge.hip
int gauge_swap_resident(qexhip_ctx *c, double2 **buf);

// expm1Deriv (matexp.nim:686-713) with scale 20 and expm1Poly4Deriv (:100-117): the reference's recursion, operation by operation
__device__ __forceinline__ void m3_half_sym_acc(M3 &we, const M3 &e) {
  // we += 0.5 (we e^+ + e^+ we)
  M3 t = m3_mul_na(we, e);
  m3_mac_an(t, e, we);
  m3_axpy(we, 0.5, t);
}
__device__ __forceinline__ M3 m3_exp_deriv(const M3 &m, const M3 &w) {
  const double s = 1.0 / (double)(1 << 20);
  M3 ms, a;
#pragma unroll
  for (int k = 0; k < 9; k++) ms.e[k] = make_double2(s * m.e[k].x, s * m.e[k].y);
  // e = expm1Poly4(ms)   (matexp.nim:80-85)
  M3 m2 = m3_mul(ms, ms);
#pragma unroll
  for (int k = 0; k < 9; k++) a.e[k] = make_double2((1.0 / 24.0) * m2.e[k].x, (1.0 / 24.0) * m2.e[k].y);
  m3_axpy(a, 1.0 / 6.0, ms);
  m3_add_diag(a, 0.5);
  M3 e = m3_mul(a, m2);
#pragma unroll
  for (int k = 0; k < 9; k++) { e.e[k].x += ms.e[k].x; e.e[k].y += ms.e[k].y; }
  // we = 0.5 (w e^+ + e^+ w) + w
  M3 we = w;
  m3_half_sym_acc(we, e);
#pragma unroll 1
  for (int i = 2; i <= 20; i++) {
    e = m3_sq_p2(e);                 // e := e (e + 2)
    m3_half_sym_acc(we, e);
  }
  // expm1Poly4Deriv(ms, we), md = ms^+
  const M3 md = m3_adj(ms);
  M3 g, f;
#pragma unroll
  for (int k = 0; k < 9; k++) g.e[k] = make_double2((1.0 / 24.0) * md.e[k].x, (1.0 / 24.0) * md.e[k].y);
  f = g;
  m3_add_diag(f, 1.0 / 6.0);
  const M3 e2 = m3_mul(we, f);       // e = w f
  M3 aa = e2;
  m3_mac(aa, g, we);                 // a = g w + e
  M3 d = m3_mul(e2, md);             // d = e m' + C2 w
  m3_axpy(d, 0.5, we);
  M3 cc = we;
  m3_mac(cc, d, md);                 // c = d m' + w
  M3 h = d;
  m3_mac(h, md, aa);                 // h = m' a + d
  m3_mac(cc, md, h);                 // r = m' h + c
  return cc;
}

// smearDeriv's per-link part (stoutsmear.nim:165-168, 113-119, 171-175), on the body tiles, in place on F (in: chain, out: the
// per-link part of deriv without the t ds term, which k_stout_stencil adds):
//   d1 = a expDeriv(a f, chain gf^+), t = TAH(d1) -> T, cg = t^+ gf -> CG, F = exp(a f)^+ chain
template <bool CLOSED>
__global__ void __launch_bounds__(256) k_stout_link(size_t nlinks_tiles, const double2 *__restrict__ Gf, const double2 *__restrict__ V,
                                                    double2 *F, double2 *T, double2 *CG, double a, size_t ntile4, size_t etile4) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t tile = j >> 6;
  if (tile >= nlinks_tiles) return;
  const size_t p = tile >= ntile4;
  const size_t o = (p * etile4 + (tile - p * ntile4)) * 576 + (j & 63);
  const M3 chain = m3_load(F + o, 64), gf = m3_load(Gf + o, 64), v = m3_load(V + o, 64);
  {
    M3 d1 = m3_exp_deriv(v, m3_mul_na(chain, gf));
#pragma unroll
    for (int k = 0; k < 9; k++) { d1.e[k].x *= a; d1.e[k].y *= a; }
    const M3 t = m3_tah(d1);
    m3_store(T + o, 64, t);
    m3_store(CG + o, 64, m3_mul_an(t, gf));
  }
  const M3 E = CLOSED ? m3_exp_tah(v) : m3_exp(v);
  m3_store(F + o, 64, m3_mul_an(E, chain));
}

// gaugeForceDeriv's stencil part (stoutsmear.nim:127-146) and the t ds term of its first part (:118): one lane per (site, mu), a
// workgroup = one tile x four directions in the blocked visiting order of the force kernels.
//   D_mu(x) += cp [ t_mu(x) S_mu(x) + sum_{nu != mu} ( gf_nu(x) gf_mu(x+nu) cg_nu(x+mu)^+ + gf_nu(x) cg_mu(x+nu) gf_nu(x+mu)^+
//                 + cg_nu(x) gf_mu(x+nu) gf_nu(x+mu)^+ + gf_nu(x-nu)^+ gf_mu(x-nu) cg_nu(x-nu+mu) + gf_nu(x-nu)^+ cg_mu(x-nu) gf_nu(x-nu+mu)
//                 + cg_nu(x-nu)^+ gf_mu(x-nu) gf_nu(x-nu+mu) ) ],   S = the plaquette staple sum (ds = cp S), cp = 1/nc
template <bool HALO>
__global__ void __launch_bounds__(256) k_stout_stencil(Geom g, const double2 *__restrict__ G, const double2 *__restrict__ CG,
                                                       const double2 *__restrict__ T, double2 *D, const int *order, int chunk) {
  const int e = order_block_entry(order, chunk);
  if (e < 0) return;
  const int mu = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int p = e & 1;
  const int c0 = (e >> 1) * 64 + lane;
  const bool live = c0 < g.Vh;
  const int c = live ? c0 : g.Vh - 1;                 // padding lanes of the last tile work on a valid site and store nothing
  int x[4], xpm[4], y[4], z[4];
  coords_of(g, c, p, x);
  shifted_dyn<HALO>(g, x, mu, 1, xpm);
  const size_t o = link_off_t<HALO>(g, x, mu);
  M3 acc = m3_zero(), st = m3_zero();
#pragma unroll 1
  for (int nu = 0; nu < 4; nu++) {
    if (nu == mu) continue;
    {
      shifted_dyn<HALO>(g, x, nu, 1, y);
      const size_t oA = link_off_t<HALO>(g, x, nu), oB = link_off_t<HALO>(g, y, mu), oC = link_off_t<HALO>(g, xpm, nu);
      const M3 B = m3_load(G + oB, 64), C = m3_load(G + oC, 64);
      const M3 bc = m3_mul_na(B, C);
      M3 s = m3_mul_na(B, m3_load(CG + oC, 64));
      m3_mac_na(s, m3_load(CG + oB, 64), C);
      const M3 A = m3_load(G + oA, 64);
      m3_mac(acc, A, s);
      m3_mac(st, A, bc);
      m3_mac(acc, m3_load(CG + oA, 64), bc);
    }
    {
      shifted_dyn<HALO>(g, x, nu, -1, y);
      shifted_dyn<HALO>(g, y, mu, 1, z);
      const size_t oA = link_off_t<HALO>(g, y, nu), oB = link_off_t<HALO>(g, y, mu), oC = link_off_t<HALO>(g, z, nu);
      const M3 B = m3_load(G + oB, 64), C = m3_load(G + oC, 64);
      const M3 bc = m3_mul(B, C);
      M3 s = m3_mul(B, m3_load(CG + oC, 64));
      m3_mac(s, m3_load(CG + oB, 64), C);
      const M3 A = m3_load(G + oA, 64);
      m3_mac_an(acc, A, s);
      m3_mac_an(st, A, bc);
      m3_mac_an(acc, m3_load(CG + oA, 64), bc);
    }
  }
  if (!live) return;
  m3_mac(acc, m3_load_nt(T + o, 64), st);
  M3 d = m3_load_nt(D + o, 64);
  m3_axpy(d, 1.0 / 3.0, acc);
  m3_store_nt(D + o, 64, d);
}

// F <- TAH(G F^+) on the body tiles (contractProjectTAH, gaugeUtils.nim:389-398; tstoutderiv.nim:143)
__global__ void __launch_bounds__(256) k_stout_projtah(size_t nlinks_tiles, double2 *F, const double2 *__restrict__ G, size_t ntile4, size_t etile4) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t tile = j >> 6;
  if (tile >= nlinks_tiles) return;
  const size_t p = tile >= ntile4;
  const size_t o = (p * etile4 + (tile - p * ntile4)) * 576 + (j & 63);
  m3_store(F + o, 64, m3_tah(m3_mul_na(m3_load(G + o, 64), m3_load(F + o, 64))));
}

// device-side loop state of the inverse
struct StoutInv {
  double rdf2, df2o, req;
  int iter, maxits, done, diverging;
};

// One iteration of the inverse (stoutsmear.nim:58-73) for every link at once: f_new = TAH(gf ds(gf)^+), gf' = exp(a f_new) fl into
// the other link buffer, f := f_new, workgroup partials of |f_new - f|^2 and |f_new|^2.  Gated on the loop state.
template <bool HALO>
__global__ void __launch_bounds__(256) k_stout_inv(Geom g, const double2 *__restrict__ G, const double2 *__restrict__ FL, double2 *Gout,
                                                   double2 *Fb, double a, double *partials, const StoutInv *S, const int *order, int chunk) {
  if (S->done) return;
  const int e = order_block_entry(order, chunk);
  double df2 = 0.0, f2 = 0.0;
  if (e >= 0) {                                       // (the whole workgroup together)
    const int mu = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int p = e & 1;
    const int c0 = (e >> 1) * 64 + lane;
    const bool live = c0 < g.Vh;
    const int c = live ? c0 : g.Vh - 1;
    int x[4], xpm[4], y[4], z[4];
    coords_of(g, c, p, x);
    shifted_dyn<HALO>(g, x, mu, 1, xpm);
    const size_t o = link_off_t<HALO>(g, x, mu);
    M3 acc = m3_zero();
#pragma unroll 1
    for (int nu = 0; nu < 4; nu++) {
      if (nu == mu) continue;
      shifted_dyn<HALO>(g, x, nu, 1, y);
      M3 t = m3_mul_na(m3_load(G + link_off_t<HALO>(g, y, mu), 64), m3_load(G + link_off_t<HALO>(g, xpm, nu), 64));
      m3_mac(acc, m3_load(G + link_off_t<HALO>(g, x, nu), 64), t);
      shifted_dyn<HALO>(g, x, nu, -1, y);
      shifted_dyn<HALO>(g, y, mu, 1, z);
      t = m3_mul_an(m3_load(G + link_off_t<HALO>(g, y, nu), 64), m3_load(G + link_off_t<HALO>(g, y, mu), 64));
      m3_mac(acc, t, m3_load(G + link_off_t<HALO>(g, z, nu), 64));
    }
    M3 f = m3_tah(m3_mul_na(m3_load(G + o, 64), acc));
#pragma unroll
    for (int k = 0; k < 9; k++) { f.e[k].x *= 1.0 / 3.0; f.e[k].y *= 1.0 / 3.0; }
    if (live) {
      const M3 fo = m3_load_nt(Fb + o, 64);
#pragma unroll
      for (int k = 0; k < 9; k++) {
        const double dx = f.e[k].x - fo.e[k].x, dy = f.e[k].y - fo.e[k].y;
        df2 += dx * dx + dy * dy;
        f2 += f.e[k].x * f.e[k].x + f.e[k].y * f.e[k].y;
      }
      m3_store_nt(Fb + o, 64, f);
      M3 v;
#pragma unroll
      for (int k = 0; k < 9; k++) v.e[k] = make_double2(a * f.e[k].x, a * f.e[k].y);
      m3_store_nt(Gout + o, 64, m3_mul(m3_exp(v), m3_load_nt(FL + o, 64)));
    }
  }
  double r = block_sum_256(df2);
  if (threadIdx.x == 0) partials[blockIdx.x] = r;
  r = block_sum_256(f2);
  if (threadIdx.x == 0) partials[gridDim.x + blockIdx.x] = r;
}
// the partials in fixed order -> red[0] = df2, red[1] = f2 of this rank
__global__ void __launch_bounds__(256) k_stout_sum(const double *partials, int nb, double *red) {
  for (int k = 0; k < 2; k++) {
    double acc = 0;
    for (int i = threadIdx.x; i < nb; i += 256) acc += partials[(size_t)k * nb + i];
    const double r = block_sum_256(acc);
    if (threadIdx.x == 0) red[k] = r;
  }
}
// loop control (stoutsmear.nim:77-88) on the rank-global sums
__global__ void k_stout_decide(const double *red, StoutInv *S) {
  if (S->done) return;
  const double df2 = red[0], f2 = red[1];
  S->rdf2 = df2 / f2;
  S->iter += 1;
  if (S->df2o >= 0 && S->df2o < df2) S->diverging = 1;      // the reference's "df^2 increased" warning
  S->df2o = df2;
  if (S->rdf2 < S->req || S->iter >= S->maxits) S->done = 1;
}

namespace {
enum { STOUT_MAXLEV = 8 };
struct StoutState {
  size_t n2 = 0;                      // double2 elements of a gauge-shaped field, ghost tiles included
  int nlev = 0, inplace0 = 0;
  double alpha[STOUT_MAXLEV]{};
  double2 *gf[STOUT_MAXLEV + 1]{};    // gf[k]: input of level k; gf[nlev]: the smeared links
  double2 *v[STOUT_MAXLEV]{};         // a f of level k
  double2 *F = nullptr, *T = nullptr, *CG = nullptr;     // chain / deriv, TAH(d1), cg of the level in hand
  double2 *s[4]{};                    // scratch of smear / inverse: link buffers and the inverse's f
  double *part = nullptr; int npart = 0;
  double *red = nullptr; StoutInv *inv = nullptr;
};
StoutState *state(qexhip_ctx *c) { return (StoutState *)c->stout; }
int field(qexhip_ctx *c, StoutState *st, double2 **p) {
  if (*p) return 0;
  HIPCHK(hipMalloc((void **)p, st->n2 * sizeof(double2)));
  HIPCHK(hipMemsetAsync(*p, 0, st->n2 * sizeof(double2), c->stream));
  return 0;
}
int ensure(qexhip_ctx *c, StoutState **out) {
  HIPCHK(hipSetDevice(c->device));
  StoutState *st = state(c);
  if (!st) { st = new StoutState(); c->stout = st; }
  st->n2 = (size_t)2 * c->g.etile * 4 * 576;
  *out = st;
  return 0;
}
int ghosts(qexhip_ctx *c, double2 *field, int depth) { return gauge_field_ghosts(c, field, depth); }
unsigned link_blocks(qexhip_ctx *c) { return (unsigned)(((size_t)2 * c->g.ntile * 4 * 64 + 255) / 256); }

// smearDeriv of level k, in place on st->F
int backward_level(qexhip_ctx *c, StoutState *st, int k) {
  const Geom &g = c->g;
  const size_t ltiles = (size_t)2 * g.ntile * 4;
  const double a = -st->alpha[k] * 3.0;
  {
    ScopedTimer tm(c, "stout_link", c->stream);
    if (c->opt_flow_exp) k_stout_link<true><<<link_blocks(c), 256, 0, c->stream>>>(ltiles, st->gf[k], st->v[k], st->F, st->T, st->CG, a, (size_t)g.ntile * 4, (size_t)g.etile * 4);
    else k_stout_link<false><<<link_blocks(c), 256, 0, c->stream>>>(ltiles, st->gf[k], st->v[k], st->F, st->T, st->CG, a, (size_t)g.ntile * 4, (size_t)g.etile * 4);
    HIPCHK(hipGetLastError());
  }
  CHK(ghosts(c, st->CG, 1));          // cg is gathered at x+mu, x+nu, x-nu, x-nu+mu (gf's ghost slices date from the forward stage)
  const int *order = nullptr; int chunk = 0;
  CHK(tile_order_table(c, &order, &chunk));
  ScopedTimer tm(c, "stout_stencil", c->stream);
  if (g.halo) k_stout_stencil<true><<<8 * chunk, 256, 0, c->stream>>>(g, st->gf[k], st->CG, st->T, st->F, order, chunk);
  else k_stout_stencil<false><<<8 * chunk, 256, 0, c->stream>>>(g, st->gf[k], st->CG, st->T, st->F, order, chunk);
  HIPCHK(hipGetLastError());
  return 0;
}
int chain_ready(qexhip_ctx *c, const char *who) {
  StoutState *st = state(c);
  if (!st || st->nlev < 1) { qexhip_set_error("%s: call qexhip_stout_prepare first", who); return -1; }
  if (st->inplace0) { qexhip_set_error("%s: level 0 was smeared in place, its input links are gone (stoutsmear.nim:22)", who); return -1; }
  return 0;
}
int backward_all(qexhip_ctx *c, StoutState *st) {
  CHK(field(c, st, &st->T)); CHK(field(c, st, &st->CG));
  for (int k = st->nlev - 1; k >= 0; k--) CHK(backward_level(c, st, k));
  c->md_src1_stout = 1;
  return 0;
}
}  // namespace

double2 *stout_force_buffer(qexhip_ctx *c) { StoutState *st = state(c); return st ? st->F : nullptr; }

static void stout_drop_chain(StoutState *st) {
  for (int k = 0; k <= STOUT_MAXLEV; k++) if (st->gf[k]) { (void)hipFree(st->gf[k]); st->gf[k] = nullptr; }
  for (int k = 0; k < STOUT_MAXLEV; k++) if (st->v[k]) { (void)hipFree(st->v[k]); st->v[k] = nullptr; }
  for (double2 **p : {&st->F, &st->T, &st->CG}) if (*p) { (void)hipFree(*p); *p = nullptr; }
  st->nlev = 0; st->inplace0 = 0;
}
// qexhip_stout_release: the chain only;  qexhip_release_workspace / qexhip_finalize: everything
void stout_chain_free(qexhip_ctx *c) {
  if (!c->stout) return;
  stout_drop_chain(state(c));
  c->md_src1_stout = 0;
}
void stout_state_free(qexhip_ctx *c) {
  StoutState *st = state(c);
  if (!st) return;
  stout_drop_chain(st);
  for (int k = 0; k < 4; k++) if (st->s[k]) (void)hipFree(st->s[k]);
  if (st->part) (void)hipFree(st->part);
  if (st->red) (void)hipFree(st->red);
  if (st->inv) (void)hipFree(st->inv);
  delete st;
  c->stout = nullptr;
  c->md_src1_stout = 0;
}

static int stout_check_args(qexhip_ctx *c, const char *who, const double *alphas, int n) {
  for (int k = 0; k < n; k++)
    if (!std::isfinite(alphas[k])) { qexhip_set_error("%s: alpha[%d] is not finite", who, k); return QEXHIP_ERR_ARG; }
  for (int i = 0; i < 4; i++) if (c->g.X[i] < 2) { qexhip_set_error("%s: stout smearing needs local extents >= 2", who); return QEXHIP_ERR_ARG; }
  return 0;
}

// ss.smear(g, fl) without the closure state (stoutsmear.nim:15-34)
int stout_smear(qexhip_ctx *c, const double *g_host, double alpha, double *fl_host) {
  CHK(stout_check_args(c, "stout_smear", &alpha, 1));
  if (!g_host && !gauge_links_dev(c)) { qexhip_set_error("stout_smear(g = NULL) needs a resident gauge field (qexhip_gauge_set / qexhip_md_begin)"); return QEXHIP_ERR_STATE; }
  StoutState *st;
  CHK(ensure(c, &st));
  CHK(field(c, st, &st->s[1])); CHK(field(c, st, &st->s[2]));
  double2 *in = nullptr;                      // nullptr: the resident links
  if (g_host) {
    CHK(field(c, st, &st->s[0]));
    CHK(gauge_upload_nat(c, st->s[0], g_host));
    in = st->s[0];
  }
  CHK(gauge_stout_stage(c, in, st->s[2], st->s[1], alpha));
  if (fl_host) return gauge_download_nat(c, st->s[1], fl_host);
  CHK(gauge_swap_resident(c, &st->s[1]));     // fl = NULL: the result replaces the resident links
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// levels 0..n-1 in order, state kept for stout_force (the n-level closure; one level = newStoutSmear + smear)
int stout_prepare(qexhip_ctx *c, const double *g_host, const double *alphas, int nlevels, double *fl_host) {
  if (!alphas || nlevels < 1 || nlevels > STOUT_MAXLEV) { qexhip_set_error("stout_prepare: 1 <= nlevels <= %d", STOUT_MAXLEV); return QEXHIP_ERR_ARG; }
  CHK(stout_check_args(c, "stout_prepare", alphas, nlevels));
  const double2 *U = gauge_links_dev(c);
  if (!g_host && !U) { qexhip_set_error("stout_prepare(g = NULL) needs a resident gauge field (qexhip_gauge_set / qexhip_md_begin)"); return QEXHIP_ERR_STATE; }
  StoutState *st;
  CHK(ensure(c, &st));
  for (int k = nlevels + 1; k <= STOUT_MAXLEV; k++) if (st->gf[k]) { (void)hipFree(st->gf[k]); st->gf[k] = nullptr; }
  for (int k = nlevels; k < STOUT_MAXLEV; k++) if (st->v[k]) { (void)hipFree(st->v[k]); st->v[k] = nullptr; }
  st->nlev = 0;
  for (int k = 0; k <= nlevels; k++) CHK(field(c, st, &st->gf[k]));
  for (int k = 0; k < nlevels; k++) CHK(field(c, st, &st->v[k]));
  if (g_host) CHK(gauge_upload_nat(c, st->gf[0], g_host));
  else HIPCHK(hipMemcpyAsync(st->gf[0], U, st->n2 * sizeof(double2), hipMemcpyDeviceToDevice, c->stream));
  for (int k = 0; k < nlevels; k++) {
    st->alpha[k] = alphas[k];
    CHK(gauge_stout_stage(c, st->gf[k], st->v[k], st->gf[k + 1], alphas[k]));
  }
  st->nlev = nlevels;
  st->inplace0 = (g_host && (const double *)fl_host == g_host);
  if (fl_host) CHK(gauge_download_nat(c, st->gf[nlevels], fl_host));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// smearDeriv from the last level to the first (tstoutderiv.nim:190-192)
int stout_force(qexhip_ctx *c, double *f_host, const double *chain_host) {
  CHK(chain_ready(c, "stout_force"));
  StoutState *st = state(c);
  HIPCHK(hipSetDevice(c->device));
  CHK(field(c, st, &st->F));
  CHK(gauge_upload_nat(c, st->F, chain_host));
  CHK(backward_all(c, st));
  if (f_host) return gauge_download_nat(c, st->F, f_host);
  return 0;
}
// smearedForce of tstoutderiv.nim:137-143: the action's derivative on the smeared links -> chain -> TAH(g f^+)
int stout_gauge_force(qexhip_ctx *c, double *f_host, double cplaq, double c2, int kind) {
  CHK(chain_ready(c, "stout_gauge_force"));
  StoutState *st = state(c);
  HIPCHK(hipSetDevice(c->device));
  CHK(field(c, st, &st->F));
  CHK(ghosts(c, st->gf[st->nlev], (kind == 0 && c2 != 0.0) ? 2 : 1));
  CHK(gauge_deriv_dev(c, st->gf[st->nlev], st->F, cplaq, c2, kind));
  CHK(backward_all(c, st));
  const size_t ltiles = (size_t)2 * c->g.ntile * 4;
  k_stout_projtah<<<link_blocks(c), 256, 0, c->stream>>>(ltiles, st->F, st->gf[0], (size_t)c->g.ntile * 4, (size_t)c->g.etile * 4);
  HIPCHK(hipGetLastError());
  if (f_host) return gauge_download_nat(c, st->F, f_host);
  return 0;
}

// ss.inverse(gf, fl) (stoutsmear.nim:36-89)
int stout_inverse(qexhip_ctx *c, const double *fl_host, double alpha, double rdf2req, int maxits, double *g_host, int *iters, double *rdf2,
                  int *diverging) {
  CHK(stout_check_args(c, "stout_inverse", &alpha, 1));
  StoutState *st;
  CHK(ensure(c, &st));
  const Geom &g = c->g;
  for (int k = 0; k < 4; k++) CHK(field(c, st, &st->s[k]));
  double2 *buf[2] = {st->s[0], st->s[1]}, *FL = st->s[2], *Fb = st->s[3];
  const int *order = nullptr; int chunk = 0;
  CHK(tile_order_table(c, &order, &chunk));
  const int nb = 8 * chunk;
  if (st->npart < 2 * nb) {
    if (st->part) (void)hipFree(st->part);
    st->part = nullptr; st->npart = 0;
    HIPCHK(hipMalloc((void **)&st->part, sizeof(double) * 2 * nb));
    st->npart = 2 * nb;
  }
  if (!st->red) HIPCHK(hipMalloc((void **)&st->red, sizeof(double) * 2));
  if (!st->inv) HIPCHK(hipMalloc((void **)&st->inv, sizeof(StoutInv)));
  // gf := fl, f := 0 (stoutsmear.nim:50-53)
  CHK(gauge_upload_nat(c, FL, fl_host));
  HIPCHK(hipMemcpyAsync(buf[0], FL, st->n2 * sizeof(double2), hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemsetAsync(Fb, 0, st->n2 * sizeof(double2), c->stream));
  StoutInv h{};
  h.rdf2 = 0.0; h.df2o = -1.0; h.req = rdf2req; h.iter = 0; h.maxits = maxits; h.done = maxits <= 0; h.diverging = 0;
  HIPCHK(hipMemcpyAsync(st->inv, &h, sizeof(h), hipMemcpyHostToDevice, c->stream));
  const double a = alpha * 3.0;               // backward cancels the negative sign of the force (stoutsmear.nim:45)
  const int check = std::max(1, c->opt_stout_check);
  int posted = 0;
  while (!h.done) {
    const int upto = std::min(maxits, posted + check);
    for (; posted < upto; posted++) {
      double2 *in = buf[posted & 1], *out = buf[(posted + 1) & 1];
      CHK(ghosts(c, in, 1));
      {
        ScopedTimer tm(c, "stout_inverse", c->stream);
        if (g.halo) k_stout_inv<true><<<nb, 256, 0, c->stream>>>(g, in, FL, out, Fb, a, st->part, st->inv, order, chunk);
        else k_stout_inv<false><<<nb, 256, 0, c->stream>>>(g, in, FL, out, Fb, a, st->part, st->inv, order, chunk);
      }
      k_stout_sum<<<1, 256, 0, c->stream>>>(st->part, nb, st->red);
      HIPCHK(hipGetLastError());
      if (multi_rank(c)) CHK(comm_allreduce(c, st->red, 2));
      k_stout_decide<<<1, 1, 0, c->stream>>>(st->red, st->inv);
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(&h, st->inv, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  if (iters) *iters = h.iter;
  if (rdf2) *rdf2 = h.rdf2;
  if (diverging) *diverging = h.diverging;
  return gauge_download_nat(c, buf[h.iter & 1], g_host);
}
