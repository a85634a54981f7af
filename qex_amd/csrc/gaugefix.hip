// gaugefix.hip -- Coulomb / Landau gauge fixing on the resident links.
//
// Restates (file:line in ctpeterson/qex, src/gauge/gaugefix.nim):
//   gaugeTransform             :8-20      g_mu(x) <- t(x) g_mu(x) t(x+mu)^+
//   gtGradient                 :22-57     gd(x) = sum_{mu in dirs} [ g_mu(x) t(x+mu)^+ + (t(x-mu) g_mu(x-mu))^+ ]
//   linkTrace / gfMetric       :135-195
//   gfMetrics                  :145-174   m = t gd: met = sf sum Re tr m, gre / gro = sfg sum_{even / odd} |TAH(m)|^2
//   gfLineMin                  :197-227
//   overRelaxSu2, relaxE/O     :241-310
//   getGaugeFixTransform       :312-355
// State: the transform field t, one 3x3 matrix per site, T[parity][tile][9][64] double2 with the ghost tiles of GaugeNat::U
// behind each parity half (gauge_index.h: site_off_t); the polish phase adds a = TAH(t gd) and a copy of t.
//
// One relax iteration of the reference is three passes over the lattice (gradient to memory, metrics, relax of one parity).
// Here gd never leaves the registers: gd(x) needs t at sites of the OTHER parity only, so
//   launch 1 (read only)  the passive parity: gradient, metric partials
//   launch 2 (in place)   the active parity:  gradient, metric partials, the three subgroup steps, store t
// and both see t as it was before the update.  A one-workgroup close kernel (k_gf_close) sums the partials in a fixed order
// and keeps iteration count, polish count and the done flag in a device struct (GfScal); the sweeps of an iteration return at
// once when the flag is set, and the host reads the struct every `gfix_check` iterations.  Because evaluation and update are
// one launch, the update that follows the FIRST evaluation with gdsq <= gstop is still a relax sweep (the reference takes a
// line-minimisation step there); from the next evaluation on the host drives the line-minimisation steps as the reference does.
#include "qexhip_internal.h"
#include "qexhip.h"
#include "reduce.h"
#include "su3.h"
#include "gauge_index.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>

namespace {

struct GfScal {
  double met, gre, gro;      // the last evaluation, rank-global and normalised
  double raw[4];             // the sums {met even, grad even, met odd, grad odd}: a copy of loc[], all-reduced in place when t is sharded
  double loc[4];             // this rank's own sums of the last evaluation
  double gstop, sf, sfg;
  int its, polish, maxits, done;   // done: the relax launches return at once
};

struct GfState {
  double2 *T = nullptr, *A = nullptr, *T0 = nullptr;
  size_t n2 = 0;             // double2 elements per field (both parities, ghost tiles included)
  int etile = 0;             // the geometry the fields were allocated for
  GfScal *s = nullptr;
  double *parts = nullptr; int nparts = 0;
  double *hist = nullptr; int histcap = 0;
};

// r += a^+ b^+ = (b a)^+
__device__ __forceinline__ void m3_mac_aa(M3 &r, const M3 &a, const M3 &b) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      double sx = r.e[3 * i + j].x, sy = r.e[3 * i + j].y;
#pragma unroll
      for (int k = 0; k < 3; k++) M3_MAC(sx, sy, a.e[3 * k + i].x, -a.e[3 * k + i].y, b.e[3 * j + k].x, -b.e[3 * j + k].y);
      r.e[3 * i + j] = make_double2(sx, sy);
    }
}
__device__ __forceinline__ double m3_norm2(const M3 &a) {
  double s = 0;
#pragma unroll
  for (int k = 0; k < 9; k++) s += a.e[k].x * a.e[k].x + a.e[k].y * a.e[k].y;
  return s;
}

// overRelaxSu2 (gaugefix.nim:241-284), operation for operation
template <int I, int J>
__device__ __forceinline__ void over_relax_su2(M3 &r, const M3 &x, double o) {
  double r0 = x.e[4 * I].x + x.e[4 * J].x;
  const double r1 = -x.e[3 * J + I].y - x.e[3 * I + J].y;
  const double r2 = x.e[3 * J + I].x - x.e[3 * I + J].x;
  const double r3 = x.e[4 * J].y - x.e[4 * I].y;
  const double n = sqrt(r0 * r0 + r1 * r1 + r2 * r2 + r3 * r3);
  r0 += n * (1 - o) / o;
  if (fabs(r0) < 1e-12) r0 = r0 < 0 ? -1e-12 : 1e-12;      // moveFromZero (:229-233)
  const double nn = 1.0 / sqrt(r0 * r0 + r1 * r1 + r2 * r2 + r3 * r3);
  const double2 u00 = make_double2(nn * r0, nn * r3), u01 = make_double2(nn * r2, nn * r1);
#pragma unroll
  for (int l = 0; l < 3; l++) {
    const double2 ri = r.e[3 * I + l], rj = r.e[3 * J + l];
    const double2 a = cmul(u00, ri), b = cmul(u01, rj), cc = ccmul(u00, rj), d = ccmul(u01, ri);
    r.e[3 * I + l] = make_double2(a.x + b.x, a.y + b.y);
    r.e[3 * J + l] = make_double2(cc.x - d.x, cc.y - d.y);
  }
}

// Gradient + metric partials of the sites of one parity; RELAX: + relaxE / relaxO in place.  par_arg < 0: an iteration of the device
// loop -- the parity comes from the iteration count (updateType = its mod 2 after `inc its`, :339-340) and the launch returns at
// once when the loop is done.  Aout: a = TAH(t gd) of the polish phase (:201-204).  Visiting order and (tile, parity) table as k_plaq's:
// the wavefronts of the other parity's table slots have nothing to do.
template <bool HALO, bool RELAX>
__global__ void __launch_bounds__(256) k_gf_sweep(Geom g, const double2 *__restrict__ U, double2 *T, double2 *Aout, const GfScal *s,
                                                  double *parts, const int *order, int chunk, int par_arg, int dirmask, double orf) {
  int par = par_arg;
  if (par_arg < 0) {
    if (s->done) return;
    const int active = (s->its + 1) & 1;
    par = RELAX ? active : 1 - active;
  }
  const int e = order_wave_entry(order, chunk);
  const int c = (e >> 1) * 64 + (threadIdx.x & 63);
  double mt = 0, gr = 0;
  if (e >= 0 && (e & 1) == par && c < g.Vh) {
    int x[4], y[4];
    coords_of(g, c, par, x);
    M3 gd = m3_zero();
#pragma unroll
    for (int mu = 0; mu < 4; mu++) {
      if (!((dirmask >> mu) & 1)) continue;
      shifted_t<HALO>(g, x, mu, 1, y);
      {
        const M3 u = m3_load_nt(U + link_off_t<HALO>(g, x, mu), 64);
        const M3 tf = m3_load(T + site_off_t<HALO>(g, y), 64);
        m3_mac_na(gd, u, tf);
      }
      shifted_t<HALO>(g, x, mu, -1, y);
      {
        const M3 u = m3_load_nt(U + link_off_t<HALO>(g, y, mu), 64);
        const M3 tb = m3_load(T + site_off_t<HALO>(g, y), 64);
        m3_mac_aa(gd, u, tb);
      }
    }
    const size_t to = tile_off(g, par, c, 576);
    M3 t = m3_load(T + to, 64);
    M3 m = m3_mul(t, gd);
    mt = m.e[0].x + m.e[4].x + m.e[8].x;
    {
      const M3 a = m3_tah(m);
      gr = m3_norm2(a);
      if (Aout) m3_store(Aout + to, 64, a);
    }
    if (RELAX) {
      over_relax_su2<0, 1>(t, m, orf);
      m = m3_mul(t, gd);
      over_relax_su2<1, 2>(t, m, orf);
      m = m3_mul(t, gd);
      over_relax_su2<0, 2>(t, m, orf);
      m3_store(T + to, 64, t);
    }
  }
  const double r0 = block_sum_256(mt), r1 = block_sum_256(gr);
  if (threadIdx.x == 0) {
    parts[(size_t)(2 * par) * gridDim.x + blockIdx.x] = r0;
    parts[(size_t)(2 * par + 1) * gridDim.x + blockIdx.x] = r1;
  }
}

enum { GF_SUM = 1, GF_FINISH = 2, GF_STEP = 4, GF_GATED = 8 };
// One workgroup.  GF_SUM: the four partial arrays -> loc[] and raw[] in a fixed order; a gated call behind the end of the loop only restores
// raw[] from loc[], so that the all-reduce the host has posted behind it -- a collective cannot be gated -- leaves the true sum again
// instead of multiplying the last one by the rank count.  GF_FINISH: normalise (gfMetrics :147-148,173), record
// the evaluation at hist[3 * (rec < 0 ? its : rec)], leave {gdsq, -gdsq, its, -its} for the ranks' agreement check.  GF_STEP: the loop control of
// :327-342 for a relax iteration -- polish counts consecutive evaluations with gdsq <= gstop; the device loop ends when
// one is seen or maxits is reached.
__global__ void __launch_bounds__(256) k_gf_close(GfScal *s, const double *parts, int nb, int flags, double *hist, int histcap, int rec,
                                                  double *agree) {
  if ((flags & GF_GATED) && s->done) {
    if ((flags & GF_SUM) && threadIdx.x < 4) s->raw[threadIdx.x] = s->loc[threadIdx.x];
    return;
  }
  if (flags & GF_SUM) {
    for (int k = 0; k < 4; k++) {
      double acc = 0;
      for (int i = threadIdx.x; i < nb; i += 256) acc += parts[(size_t)k * nb + i];
      const double r = block_sum_256(acc);
      if (threadIdx.x == 0) { s->loc[k] = r; s->raw[k] = r; }
    }
  }
  if (threadIdx.x != 0 || !(flags & GF_FINISH)) return;
  const double met = s->sf * (s->raw[0] + s->raw[2]), gre = s->sfg * s->raw[1], gro = s->sfg * s->raw[3];
  s->met = met; s->gre = gre; s->gro = gro;
  int its = s->its;
  const int at = rec < 0 ? its : rec;
  if (hist && rec > -2 && at < histcap) { hist[3 * at] = met; hist[3 * at + 1] = gre; hist[3 * at + 2] = gro; }
  if (flags & GF_STEP) {
    const double gdsq = gre + gro;
    const int polish = gdsq <= s->gstop ? s->polish + 1 : 0;
    its++;
    s->polish = polish; s->its = its;
    if (polish > 0 || its >= s->maxits) s->done = 1;
  }
  const double gdsq = gre + gro;
  agree[0] = gdsq; agree[1] = -gdsq; agree[2] = its; agree[3] = -its;
}
// (agree: the first read-back comes before any evaluation -- the ranks then agree on the count alone)
__global__ void k_gf_init(GfScal *s, double gstop, double sf, double sfg, int its, int polish, int maxits, int done, double *agree) {
  s->gstop = gstop; s->sf = sf; s->sfg = sfg;
  s->its = its; s->polish = polish; s->maxits = maxits; s->done = done;
  agree[0] = 0.0; agree[1] = -0.0; agree[2] = its; agree[3] = -its;
}

// gtUpdate (:95-101) with the reference's exp (matexp.nim: Taylor + 20 squarings), optionally followed by projectSU (:224):
// T(x) = exp(-eps a(x)) Tsrc(x) on the body sites
template <bool PROJECT>
__global__ void __launch_bounds__(256) k_gf_update(Geom g, double2 *T, const double2 *__restrict__ Tsrc, const double2 *__restrict__ A, double eps) {
  const int tb = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tb >= 2 * g.ntile) return;
  const int p = tb >= g.ntile, tile = tb - p * g.ntile, c = tile * 64 + (threadIdx.x & 63);
  if (c >= g.Vh) return;
  const size_t o = ((size_t)p * g.etile + tile) * 576 + (threadIdx.x & 63);
  M3 a = m3_load(A + o, 64);
#pragma unroll
  for (int k = 0; k < 9; k++) a.e[k] = make_double2(-eps * a.e[k].x, -eps * a.e[k].y);
  M3 r = m3_mul(m3_exp(a), m3_load(Tsrc + o, 64));
  if (PROJECT) r = m3_projectSU(r);
  m3_store(T + o, 64, r);
}

// gaugeTransform (:8-20): Uout_mu(x) = t(x) U_mu(x) t(x+mu)^+, all four directions
template <bool HALO>
__global__ void __launch_bounds__(256) k_gauge_transform(Geom g, const double2 *__restrict__ U, double2 *Uout, const double2 *__restrict__ T) {
  const int tb = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tb >= 2 * g.ntile) return;
  const int p = tb >= g.ntile, c = (tb - p * g.ntile) * 64 + (threadIdx.x & 63);
  if (c >= g.Vh) return;
  int x[4], y[4];
  coords_of(g, c, p, x);
  const M3 t = m3_load(T + site_off_t<HALO>(g, x), 64);
#pragma unroll
  for (int mu = 0; mu < 4; mu++) {
    shifted_t<HALO>(g, x, mu, 1, y);
    const size_t o = link_off_t<HALO>(g, x, mu);
    const M3 ut = m3_mul_na(m3_load_nt(U + o, 64), m3_load(T + site_off_t<HALO>(g, y), 64));
    m3_store_nt(Uout + o, 64, m3_mul(t, ut));
  }
}

// linkTrace (:135-142): workgroup partials of sum_{mu in dirs} Re tr U_mu(x)
__global__ void __launch_bounds__(256) k_link_trace(Geom g, const double2 *__restrict__ U, int dirmask, double *parts) {
  const int tb = blockIdx.x * 4 + (threadIdx.x >> 6);
  double tr = 0;
  if (tb < 2 * g.ntile) {
    const int p = tb >= g.ntile, tile = tb - p * g.ntile, c = tile * 64 + (threadIdx.x & 63);
    if (c < g.Vh) {
#pragma unroll
      for (int mu = 0; mu < 4; mu++) {
        if (!((dirmask >> mu) & 1)) continue;
        const double2 *u = U + (((size_t)p * g.etile + tile) * 4 + mu) * 576 + (threadIdx.x & 63);
        tr += u[0].x + u[4 * 64].x + u[8 * 64].x;
      }
    }
  }
  const double r = block_sum_256(tr);
  if (threadIdx.x == 0) parts[blockIdx.x] = r;
}
__global__ void __launch_bounds__(256) k_gf_sum1(const double *parts, int nb, double *out) {
  double acc = 0;
  for (int i = threadIdx.x; i < nb; i += 256) acc += parts[i];
  const double r = block_sum_256(acc);
  if (threadIdx.x == 0) out[0] = r;
}

// host [site][3][3] <-> tiles (the body sites; NULL host = identity)
__global__ void __launch_bounds__(256) k_gf_to_tiles(Geom g, const double2 *__restrict__ host, double2 *T) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= g.V) return;
  int p, c; linear_site(g, i, p, c);
  double2 *w = T + tile_off(g, p, c, 576);
  for (int k = 0; k < 9; k++) w[k * 64] = host ? host[(size_t)i * 9 + k] : make_double2((k & 3) == 0 ? 1.0 : 0.0, 0.0);
}
__global__ void __launch_bounds__(256) k_gf_from_tiles(Geom g, double2 *__restrict__ host, const double2 *T) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= g.V) return;
  int p, c; linear_site(g, i, p, c);
  const double2 *w = T + tile_off(g, p, c, 576);
  for (int k = 0; k < 9; k++) host[(size_t)i * 9 + k] = w[k * 64];
}

GfState *state_of(qexhip_ctx *c) { return (GfState *)c->gfix; }
bool state_current(qexhip_ctx *c) { GfState *S = state_of(c); return S && S->T && S->etile == c->g.etile && S->n2 == (size_t)2 * c->g.etile * 576; }

int field_ensure(qexhip_ctx *c, GfState *S, double2 **f) {
  if (*f) return 0;
  HIPCHK(hipMalloc((void **)f, S->n2 * sizeof(double2)));
  HIPCHK(hipMemsetAsync(*f, 0, S->n2 * sizeof(double2), c->stream));
  return 0;
}

// depth-1 t-faces of t into the neighbours' ghost tiles (gauge_ghosts' layout with one matrix per site)
int t_faces(qexhip_ctx *c, GfState *S) {
  const Geom &g = c->g;
  if (!g.halo) return 0;
  double *bottom[2], *top[2], *ghi[2], *glo[2];
  const size_t face = ghost_faces(g, S->T, 576, 1, bottom, top, ghi, glo);
  return comm_faces_exchange(c, 2, bottom, top, ghi, glo, face);
}

struct Sweep {
  qexhip_ctx *c; GfState *S; const int *order; int chunk, nb, dirmask; double orf; bool tdir;
};

int launch_sweep(const Sweep &w, bool relax, int par, double2 *Aout) {
  qexhip_ctx *c = w.c;
#define QX_GF(HL, RL) k_gf_sweep<HL, RL><<<w.nb, 256, 0, c->stream>>>(c->g, c->gn->U, w.S->T, Aout, w.S->s, w.S->parts, w.order, w.chunk, par, w.dirmask, w.orf)
  if (relax) { if (c->g.halo) QX_GF(true, true); else QX_GF(false, true); }
  else { if (c->g.halo) QX_GF(true, false); else QX_GF(false, false); }
#undef QX_GF
  HIPCHK(hipGetLastError());
  return 0;
}
// partials -> rank-global metrics in GfScal (the ranks' sums are all-reduced between the two halves of the close kernel)
int close_eval(const Sweep &w, int flags, int rec) {
  qexhip_ctx *c = w.c;
  GfState *S = w.S;
  const int gate = flags & GF_GATED;
  if (multi_rank(c)) {
    k_gf_close<<<1, 256, 0, c->stream>>>(S->s, S->parts, w.nb, GF_SUM | gate, S->hist, S->histcap, rec, c->cg->agree);
    CHK(comm_allreduce(c, S->s->raw, 4));
    k_gf_close<<<1, 256, 0, c->stream>>>(S->s, S->parts, w.nb, flags & ~GF_SUM, S->hist, S->histcap, rec, c->cg->agree);
  } else {
    k_gf_close<<<1, 256, 0, c->stream>>>(S->s, S->parts, w.nb, flags, S->hist, S->histcap, rec, c->cg->agree);
  }
  HIPCHK(hipGetLastError());
  return 0;
}
// read the device state; sharded: every rank holds the same metrics and count
int read_state(qexhip_ctx *c, GfState *S, GfScal *h) {
  CHK(comm_agree_post(c));
  HIPCHK(hipMemcpyAsync(c->pinned, S->s, sizeof(GfScal), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync((char *)c->pinned + 512, c->cg->agree, 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  memcpy(h, c->pinned, sizeof(GfScal));
  if (multi_rank(c) && comm_ready(c)) {
    CHK(peer_check(c));
    double a[4];
    memcpy(a, (char *)c->pinned + 512, sizeof(a));
    const bool both_nan = std::isnan(a[0]) && std::isnan(a[1]);
    if ((!both_nan && a[0] != -a[1]) || a[2] != -a[3]) {
      qexhip_set_error("gauge_fix: the ranks disagree on gdsq (%.17g .. %.17g) or the iteration count (%g .. %g)", -a[1], a[0], -a[3], a[2]);
      return QEXHIP_ERR_COMM;
    }
  }
  return 0;
}
// gfMetrics of the current t on both parities (ungated); writes a = TAH(t gd) when Aout
int evaluate(const Sweep &w, double2 *Aout, int rec, GfScal *h) {
  CHK(launch_sweep(w, false, 0, Aout));
  CHK(launch_sweep(w, false, 1, Aout));
  CHK(close_eval(w, GF_SUM | GF_FINISH, rec));
  return read_state(w.c, w.S, h);
}
int update_t(const Sweep &w, const double2 *src, double eps, bool project) {
  qexhip_ctx *c = w.c;
  const int nb = (2 * c->g.ntile + 3) / 4;
  if (project) k_gf_update<true><<<nb, 256, 0, c->stream>>>(c->g, w.S->T, src, w.S->A, eps);
  else k_gf_update<false><<<nb, 256, 0, c->stream>>>(c->g, w.S->T, src, w.S->A, eps);
  HIPCHK(hipGetLastError());
  if (w.tdir) CHK(t_faces(c, w.S));
  return 0;
}

}  // namespace

void gfix_state_free(qexhip_ctx *c) {
  GfState *S = state_of(c);
  if (!S) return;
  for (void *p : {(void *)S->T, (void *)S->A, (void *)S->T0, (void *)S->s, (void *)S->parts, (void *)S->hist})
    if (p) (void)hipFree(p);
  delete S;
  c->gfix = nullptr;
}

int gfix_check_args(qexhip_ctx *c, const char *who, const int *dirs, int ndirs, int need_t) {
  if (dirs || ndirs) {
    if (!dirs || ndirs < 1 || ndirs > 4) { qexhip_set_error("%s: dirs must hold 1..4 directions (got %d)", who, ndirs); return QEXHIP_ERR_ARG; }
    int seen = 0;
    for (int i = 0; i < ndirs; i++) {
      if (dirs[i] < 0 || dirs[i] > 3) { qexhip_set_error("%s: dirs[%d] = %d is not a direction 0..3", who, i, dirs[i]); return QEXHIP_ERR_ARG; }
      if (seen & (1 << dirs[i])) { qexhip_set_error("%s: direction %d is repeated in dirs", who, dirs[i]); return QEXHIP_ERR_ARG; }
      seen |= 1 << dirs[i];
    }
  }
  if (!c->gn) { qexhip_set_error("%s: no resident gauge field (qexhip_gauge_set first)", who); return QEXHIP_ERR_ARG; }
  if (need_t && !state_current(c)) { qexhip_set_error("%s: no resident transform (qexhip_gfix_set_transform first)", who); return QEXHIP_ERR_ARG; }
  return 0;
}

int gfix_set_transform(qexhip_ctx *c, const double *t) {
  HIPCHK(hipSetDevice(c->device));
  if (state_of(c) && !state_current(c)) gfix_state_free(c);       // the geometry changed (qexhip_comm_force_halo)
  if (!state_of(c)) {
    GfState *S = new GfState();
    c->gfix = S;
    S->etile = c->g.etile;
    S->n2 = (size_t)2 * c->g.etile * 576;
    CHK(field_ensure(c, S, &S->T));
    HIPCHK(hipMalloc((void **)&S->s, sizeof(GfScal)));
    HIPCHK(hipMemsetAsync(S->s, 0, sizeof(GfScal), c->stream));
  }
  GfState *S = state_of(c);
  const size_t bytes = (size_t)c->g.V * 18 * sizeof(double);
  if (t) {
    CHK(ensure_stage(c, bytes));
    HIPCHK(hipMemcpyAsync(c->stage, t, bytes, hipMemcpyHostToDevice, c->stream));
  }
  k_gf_to_tiles<<<(c->g.V + 255) / 256, 256, 0, c->stream>>>(c->g, t ? (const double2 *)c->stage : nullptr, S->T);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int gfix_get_transform(qexhip_ctx *c, double *t) {
  HIPCHK(hipSetDevice(c->device));
  if (!state_current(c)) { qexhip_set_error("gfix_get_transform: no resident transform (qexhip_gfix_set_transform first)"); return QEXHIP_ERR_ARG; }
  const size_t bytes = (size_t)c->g.V * 18 * sizeof(double);
  CHK(ensure_stage(c, bytes));
  k_gf_from_tiles<<<(c->g.V + 255) / 256, 256, 0, c->stream>>>(c->g, (double2 *)c->stage, state_of(c)->T);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(t, c->stage, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// getGaugeFixTransform (:312-355) on the resident t, plus `maxits`: at most that many updates, then one more evaluation
int gauge_fix(qexhip_ctx *c, const int *dirs, int ndirs, double gstop, double orf, int maxits, int *iters, double metrics[4],
              double *hist, int histcap) {
  CHK(gfix_check_args(c, "gauge_fix", dirs, ndirs, 1));
  if (!dirs) { qexhip_set_error("gauge_fix: dirs is null"); return QEXHIP_ERR_ARG; }
  if (!(orf > 0.0 && orf <= 2.0)) { qexhip_set_error("gauge_fix: over-relaxation factor %g outside (0, 2]", orf); return QEXHIP_ERR_ARG; }
  if (maxits < 0) { qexhip_set_error("gauge_fix: maxits = %d < 0", maxits); return QEXHIP_ERR_ARG; }
  if (hist && histcap < 0) { qexhip_set_error("gauge_fix: histcap = %d < 0", histcap); return QEXHIP_ERR_ARG; }
  HIPCHK(hipSetDevice(c->device));
  GfState *S = state_of(c);
  Sweep w{};
  w.c = c; w.S = S; w.orf = orf;
  for (int i = 0; i < ndirs; i++) w.dirmask |= 1 << dirs[i];
  w.tdir = (w.dirmask & 8) != 0 && c->g.halo;
  CHK(gauge_ghosts(c, 1));
  CHK(tile_order_table(c, &w.order, &w.chunk));
  w.nb = 8 * ((w.chunk + 3) / 4);
  if (S->nparts < 4 * w.nb) {
    if (S->parts) (void)hipFree(S->parts);
    S->parts = nullptr; S->nparts = 0;
    HIPCHK(hipMalloc((void **)&S->parts, sizeof(double) * 4 * w.nb));
    S->nparts = 4 * w.nb;
  }
  const int hcap = hist ? histcap : 0;
  if (S->histcap < hcap) {
    if (S->hist) (void)hipFree(S->hist);
    S->hist = nullptr; S->histcap = 0;
    HIPCHK(hipMalloc((void **)&S->hist, sizeof(double) * 3 * hcap));
    S->histcap = hcap;
  }
  const double vol = (double)c->g.V * (double)c->nranks;
  const double sf = 0.5 / ((double)ndirs * vol * 3.0), sfg = 2.0 * sf * (double)ndirs;
  k_gf_init<<<1, 1, 0, c->stream>>>(S->s, gstop, sf, sfg, 0, 0, maxits, maxits <= 0, c->cg->agree);
  HIPCHK(hipGetLastError());
  if (w.tdir) CHK(t_faces(c, S));
  GfScal h;
  CHK(read_state(c, S, &h));
  const int every = std::max(1, c->opt_gfix_check);
  double eps = 0.1;
  bool final_eval = false;
  for (;;) {
    if (!h.done) {
      // relax iterations, no host round trip: passive parity (read only), active parity (in place), close
      const int n = std::min(every, maxits - h.its);
      for (int i = 0; i < n; i++) {
        CHK(launch_sweep(w, false, -1, nullptr));
        CHK(launch_sweep(w, true, -1, nullptr));
        if (w.tdir) CHK(t_faces(c, S));
        CHK(close_eval(w, GF_SUM | GF_FINISH | GF_STEP | GF_GATED, -1));
      }
      CHK(read_state(c, S, &h));
      continue;
    }
    if (h.its >= maxits) break;
    // an evaluation saw gdsq <= gstop: the host drives (:324-349)
    CHK(field_ensure(c, S, &S->A));
    CHK(field_ensure(c, S, &S->T0));
    const int its = h.its;
    int polish = h.polish;
    CHK(evaluate(w, S->A, its, &h));
    polish = (h.gre + h.gro <= gstop) ? polish + 1 : 0;
    if (polish > 10) { final_eval = true; h.its = its; break; }
    if (polish == 0) {                                   // back to the relax sweeps
      k_gf_init<<<1, 1, 0, c->stream>>>(S->s, gstop, sf, sfg, its, 0, maxits, 0, c->cg->agree);
      HIPCHK(hipGetLastError());
      h.its = its; h.polish = 0; h.done = 0;
      continue;
    }
    // gfLineMin (:197-227)
    const double m0 = h.met;
    HIPCHK(hipMemcpyAsync(S->T0, S->T, S->n2 * sizeof(double2), hipMemcpyDeviceToDevice, c->stream));
    CHK(update_t(w, S->T, eps, false));
    CHK(evaluate(w, nullptr, -2, &h));
    const double m1 = h.met;
    CHK(update_t(w, S->T, eps, false));
    CHK(evaluate(w, nullptr, -2, &h));
    const double m2 = h.met;
    double x = eps * (3 * m0 - 4 * m1 + m2) / (2 * m0 - 4 * m1 + 2 * m2);
    x = (x <= 0) ? 0 : x;
    x = (2 * eps <= x) ? 2 * eps : x;
    eps = x;
    CHK(update_t(w, S->T0, eps, true));
    h.its = its + 1; h.polish = polish; h.done = 1;
  }
  if (!final_eval) {
    const int its = h.its, polish = h.polish;
    CHK(evaluate(w, nullptr, -2, &h));
    h.its = its; h.polish = polish;
  }
  if (iters) *iters = h.its;
  if (metrics) { metrics[0] = h.met; metrics[1] = h.gre; metrics[2] = h.gro; metrics[3] = h.gre + h.gro; }
  const int nh = std::min(h.its, hcap);
  if (nh > 0) {
    HIPCHK(hipMemcpyAsync(hist, S->hist, sizeof(double) * 3 * nh, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return 0;
}

int gauge_transform(qexhip_ctx *c) {
  CHK(gfix_check_args(c, "gauge_transform", nullptr, 0, 1));
  HIPCHK(hipSetDevice(c->device));
  GfState *S = state_of(c);
  if (!c->gn->U2) {
    HIPCHK(hipMalloc((void **)&c->gn->U2, c->gn->n2 * sizeof(double2)));
    HIPCHK(hipMemsetAsync(c->gn->U2, 0, c->gn->n2 * sizeof(double2), c->stream));
  }
  CHK(t_faces(c, S));                                    // t(x + t^) of the top slice: the upper neighbour's bottom slice
  const int nb = (2 * c->g.ntile + 3) / 4;
  if (c->g.halo) k_gauge_transform<true><<<nb, 256, 0, c->stream>>>(c->g, c->gn->U, c->gn->U2, S->T);
  else k_gauge_transform<false><<<nb, 256, 0, c->stream>>>(c->g, c->gn->U, c->gn->U2, S->T);
  HIPCHK(hipGetLastError());
  std::swap(c->gn->U, c->gn->U2);
  c->gn->ghost_valid = 0;
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int gauge_link_trace(qexhip_ctx *c, const int *dirs, int ndirs, double *out) {
  CHK(gfix_check_args(c, "gauge_link_trace", dirs, ndirs, 0));
  if (!dirs) { qexhip_set_error("gauge_link_trace: dirs is null"); return QEXHIP_ERR_ARG; }
  HIPCHK(hipSetDevice(c->device));
  int dirmask = 0;
  for (int i = 0; i < ndirs; i++) dirmask |= 1 << dirs[i];
  const int nb = (2 * c->g.ntile + 3) / 4;
  if (c->gn->npp < nb) {
    if (c->gn->pp) (void)hipFree(c->gn->pp);
    c->gn->pp = nullptr; c->gn->npp = 0;
    HIPCHK(hipMalloc((void **)&c->gn->pp, sizeof(double) * nb));
    c->gn->npp = nb;
  }
  k_link_trace<<<nb, 256, 0, c->stream>>>(c->g, c->gn->U, dirmask, c->gn->pp);
  k_gf_sum1<<<1, 256, 0, c->stream>>>(c->gn->pp, nb, &c->dscal[34]);
  HIPCHK(hipGetLastError());
  double tr;
  CHK(read_global(c, &c->dscal[34], 1, &tr));
  *out = tr / ((double)ndirs * (double)c->g.V * (double)c->nranks * 3.0);
  return 0;
}
