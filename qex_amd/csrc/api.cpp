// api.cpp -- the extern "C" boundary declared in include/qexhip.h.
// Host-pointer entry points upload into work fields, run the device path, download the result:
// the same choreography as qudaSolveXX (src/quda/qudaWrapperImpl.nim:165-261).
#include "qexhip_internal.h"
#include <string>
#include "../../include/qexhip.h"
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <vector>

static thread_local char g_err[1024] = "";

void qexhip_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char *qexhip_last_error(void) { return g_err; }

// ---- timers ----
// levels: 1 everything; 2 only the Dslash sweeps (the dominant kernel), so that the event records perturb a timed region as
// little as possible; 3 the sharded iteration's anatomy: Dslash sweeps (interior "dslash", faces "dslash_bnd"), the face
// exchange ("exchange": events on the stream the RCCL group is posted on) and the all-reduces ("allreduce")
static bool timer_class_on(const qexhip_ctx *c, const char *name) {
  if (!c->timers_on) return false;
  if (c->timers_on == 2) return strncmp(name, "dslash", 6) == 0;
  if (c->timers_on == 3) return strncmp(name, "dslash", 6) == 0 || strcmp(name, "exchange") == 0 || strcmp(name, "allreduce") == 0;
  return true;
}
ScopedTimer::ScopedTimer(qexhip_ctx *c_, const char *name, hipStream_t st_) : c(c_), st(st_) {
  if (!c->timers_on || !name) return;
  if (!timer_class_on(c, name)) return;
  s = &c->timers[name];
  if (s->used + 2 > s->ev.size()) {
    size_t old = s->ev.size();
    s->ev.resize(old + 512);
    for (size_t i = old; i < s->ev.size(); i++) (void)hipEventCreate(&s->ev[i]);
  }
  (void)hipEventRecord(s->ev[s->used], st);
}
ScopedTimer::~ScopedTimer() {
  if (!s) return;
  (void)hipEventRecord(s->ev[s->used + 1], st);
  s->used += 2;
}
bool timer_event_pair(qexhip_ctx *c, const char *name, hipEvent_t *e0, hipEvent_t *e1) {
  if (!timer_class_on(c, name)) return false;
  TimerSlot *s = &c->timers[name];
  if (s->used + 2 > s->ev.size()) {
    size_t old = s->ev.size();
    s->ev.resize(old + 512);
    for (size_t i = old; i < s->ev.size(); i++) (void)hipEventCreate(&s->ev[i]);
  }
  *e0 = s->ev[s->used];
  *e1 = s->ev[s->used + 1];
  s->used += 2;
  return true;
}
int timers_collect(qexhip_ctx *c) {
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipStreamSynchronize(c->cstream));   // "exchange" events of an overlapped sweep live there
  for (auto &kv : c->timers) {
    TimerSlot &s = kv.second;
    for (size_t i = 0; i + 1 < s.used; i += 2) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, s.ev[i], s.ev[i + 1]) == hipSuccess) { s.total_ms += ms; s.count++; }
    }
    s.used = 0;
  }
  return 0;
}

extern "C" int qexhip_timers_enable(qexhip_handle c, int on) { if (!c) return QEXHIP_ERR_ARG; c->timers_on = on; return 0; }
extern "C" int qexhip_timers_reset(qexhip_handle c) {
  if (!c) return QEXHIP_ERR_ARG;
  CHK(timers_collect(c));
  for (auto &kv : c->timers) { kv.second.count = 0; kv.second.total_ms = 0; }
  return 0;
}
extern "C" int qexhip_timers_get(qexhip_handle c, const char *name, long *count, double *total_ms) {
  if (!c || !name) return QEXHIP_ERR_ARG;
  CHK(timers_collect(c));
  auto it = c->timers.find(name);
  if (count) *count = (it == c->timers.end()) ? 0 : it->second.count;
  if (total_ms) *total_ms = (it == c->timers.end()) ? 0.0 : it->second.total_ms;
  return 0;
}

// ---- context ----
static int init_body(qexhip_ctx *c, int device, const int latLocal[4], const int rankGeom[4], const int rankCoord[4]) {
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (ndev <= 0) { qexhip_set_error("no HIP device visible: libqexhip has no CPU fallback"); return QEXHIP_ERR_HIP; }
  if (device < 0 || device >= ndev) { qexhip_set_error("device %d out of range (%d visible)", device, ndev); return QEXHIP_ERR_ARG; }
  c->device = device;
  for (int i = 0; i < 4; i++) {
    c->rankGeom[i] = rankGeom ? rankGeom[i] : 1;
    c->rankCoord[i] = rankCoord ? rankCoord[i] : 0;
  }
  for (int i = 0; i < 3; i++)
    if (c->rankGeom[i] != 1) { qexhip_set_error("only rankGeom = {1,1,1,N} (split along t) is supported"); return QEXHIP_ERR_ARG; }
  const int halo = c->rankGeom[3] > 1;
  if (geom_init(c->g, latLocal, 1, halo)) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  {
    // the comm stream carries the face exchange and the boundary launch that waits for it: at the highest priority, so that the
    // exchange kernel is dispatched at once and not behind the thousands of interior workgroups the compute stream has queued
    // (one-rank rehearsal, where nothing has to be hidden: no difference either way, profiles/r04_prio_ab.log)
    int lo = 0, hi = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && hi != lo) HIPCHK(hipStreamCreateWithPriority(&c->cstream, hipStreamNonBlocking, hi));
    else HIPCHK(hipStreamCreateWithFlags(&c->cstream, hipStreamNonBlocking));
  }
  HIPCHK(hipEventCreateWithFlags(&c->ev_ready, hipEventDisableTiming));
  c->part2_off = std::max(6144, (c->g.Vh + 255) / 256 + 8);   // >= 6*1024 for the plaquette partials
  c->npartials = c->part2_off + 2048 + 64;
  HIPCHK(hipMalloc((void **)&c->partials, sizeof(double) * c->npartials));
  HIPCHK(hipMalloc((void **)&c->dscal, sizeof(double) * 64));
  HIPCHK(hipMemset(c->dscal, 0, sizeof(double) * 64));
  HIPCHK(hipMalloc((void **)&c->cg, sizeof(CgScal)));
  HIPCHK(hipMemset(c->cg, 0, sizeof(CgScal)));
  HIPCHK(hipHostMalloc(&c->pinned, 4096, hipHostMallocDefault));
  CHK(devjoin_init(c));
  if (getenv("QEXHIP_TEST_FAIL_INIT")) {      // test hook (tests/test_gpu_misc_ops.py): fail the way a late HIP error would, everything above built
    qexhip_set_error("QEXHIP_TEST_FAIL_INIT: injected failure");
    return QEXHIP_ERR_HIP;
  }
  // the environment switches of the library (include/qexhip.h "Environment")
  if (const char *e = getenv("QEXHIP_OVERLAP")) c->opt_overlap = atoi(e);
  if (const char *e = getenv("QEXHIP_HOP_SPLIT")) { const int v = atoi(e); c->opt_hop_split = v < 0 ? -1 : (v ? 2 : 0); }
  if (const char *e = getenv("QEXHIP_RECON")) c->opt_recon = atoi(e);
  if (const char *e = getenv("QEXHIP_FLOW_EXP")) c->opt_flow_exp = atoi(e);
  {
    // the gauge kernels stage links through 144 KiB (k_force_lds2) / 72 KiB (k_force_lds, k_flow_obs_clover) of LDS per
    // workgroup: gfx950 offers 160 KiB.  The library is built for that one target (qex_amd/Makefile pins gfx950); anything
    // smaller is refused here rather than at the first flow step.
    int a = 0, b = 0;
    (void)hipDeviceGetAttribute(&a, hipDeviceAttributeMaxSharedMemoryPerBlock, device);
    (void)hipDeviceGetAttribute(&b, hipDeviceAttributeSharedMemPerBlockOptin, device);
    (void)hipGetLastError();
    const int lds = a > b ? a : b;
    if (lds < 147456 + 1024) {      // + the static LDS (reductions) the kernels add on top of the dynamic 144 KiB
      qexhip_set_error("device %d offers %d bytes of LDS per workgroup; libqexhip is built for gfx950 (160 KiB)", device, lds);
      return QEXHIP_ERR_STATE;
    }
  }
  c->nranks = 1;  // until qexhip_comm_init
  c->rank = 0;
  return 0;
}

extern "C" int qexhip_init(qexhip_handle *h, int device, const int latLocal[4], const int rankGeom[4],
                           const int rankCoord[4]) {
  if (!h || !latLocal) return QEXHIP_ERR_ARG;
  qexhip_ctx *c = new qexhip_ctx();
  const int e = init_body(c, device, latLocal, rankGeom, rankCoord);
  if (e) {                      // every failing path releases what was built so far (streams, events, device and pinned memory)
    (void)qexhip_finalize(c);
    return e;
  }
  *h = c;
  return 0;
}

extern "C" int qexhip_device_count(int *n) {
  if (!n) return QEXHIP_ERR_ARG;
  HIPCHK(hipGetDeviceCount(n));
  return 0;
}

extern "C" int qexhip_finalize(qexhip_handle c) {
  if (!c) return QEXHIP_ERR_ARG;
  if (c->stream) {                 // (a context that failed before its first HIP object has nothing on a device)
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
  }
  for (auto &kv : c->fields) (void)hipFree(kv.second.d);
  c->fields.clear();
  for (auto &kv : c->timers) for (auto e : kv.second.ev) (void)hipEventDestroy(e);
  nhyp_state_free(c);
  hisq_state_free(c);
  batch_state_free(c);
  batch_f32_state_free(c);
  batch_half_state_free(c);
  msf_state_free(c);
  gfix_state_free(c);
  stout_state_free(c);
  eig_state_free(c);
  eig_bases_free(c);
  for (auto &kv : c->cfields) (void)hipFree(kv.second.d);
  c->cfields.clear();
  gauge_free(c);
  comm_destroy(c);
  if (c->W) (void)hipFree(c->W);
  f32_state_free(c);
  half_state_free(c);
  if (c->outer_F) (void)hipFree(c->outer_F);
  if (c->obs_table) (void)hipFree(c->obs_table);
  if (c->tile_order) (void)hipFree(c->tile_order);
  for (int *&t : c->tile_order_pl) if (t) { (void)hipFree(t); t = nullptr; }
  if (c->cgm_scal) (void)hipFree(c->cgm_scal);
  if (c->meson_buf) (void)hipFree(c->meson_buf);
  if (c->Wc) (void)hipFree(c->Wc);
  if (c->Ws) (void)hipFree(c->Ws);
  if (c->Wm) (void)hipFree(c->Wm);
  if (c->stage) (void)hipFree(c->stage);
  if (c->partials) (void)hipFree(c->partials);
  if (c->dscal) (void)hipFree(c->dscal);
  if (c->cg) (void)hipFree(c->cg);
  if (c->hist) (void)hipFree(c->hist);
  if (c->pinned) (void)hipHostFree(c->pinned);
  if (c->fz_buf) (void)hipFree(c->fz_buf);
  devjoin_destroy(c);
  if (c->ev_ready) (void)hipEventDestroy(c->ev_ready);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  if (c->cstream) (void)hipStreamDestroy(c->cstream);
  (void)hipGetLastError();
  delete c;
  return 0;
}

extern "C" int qexhip_sync(qexhip_handle c) {
  if (!c) return QEXHIP_ERR_ARG;
  CHK(devjoin_flush(c));
  HIPCHK(hipStreamSynchronize(c->cstream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return devjoin_check(c);
}

extern "C" int qexhip_device_info(qexhip_handle c, char *buf, int buflen) {
  if (!c || !buf) return QEXHIP_ERR_ARG;
  hipDeviceProp_t p;
  HIPCHK(hipGetDeviceProperties(&p, c->device));
  // tile_pairs: -1 until a gather kernel has built the visiting order, then whether its slots pair the two parities of a
  // tile position (k_force_lds2 needs that; otherwise the one-tile kernels run)
  int n = snprintf(buf, buflen, "%s (%s) CUs=%d mem=%.0fGiB local=%dx%dx%dx%d ranks=%d halo=%d tile_pairs=%d", p.name, p.gcnArchName,
                   p.multiProcessorCount, p.totalGlobalMem / 1073741824.0, c->g.X[0], c->g.X[1], c->g.X[2], c->g.X[3],
                   c->rankGeom[3], c->g.halo, c->tile_order ? c->tile_pairs_ok : -1);
  // what set_links measured and decided for the sweeps of a t-sharded slab (qexhip_stag_sweep_tuning has the numbers as numbers):
  // timing-dependent decisions change the grouping of the dot partials, i.e. the last bits of a residual history -- keep them visible
  if (c->g.halo && c->W && n > 0 && n < buflen) {
    double t[8];
    if (qexhip_stag_sweep_tuning(c, t) == 0)
      snprintf(buf + n, buflen - n, "; sweep: overlap=%d form=%s exchange=%.1fus%s boundary_at=%.2f spin=%.0fus tuned[first|sites|fused]=%.0f|%.0f|%.0f us",
               (int)t[7], t[5] == 2 ? "fused" : "by-sites", t[0], c->xchg_us[c->ndir == 16] > 0 ? "(measured)" : "(estimate)", t[1], t[6], t[2], t[3], t[4]);
  }
  return 0;
}

static int drop_fields_for_regeom(qexhip_ctx *c) {
  c->cg_resume.valid = 0;
  // geometry (ghost zones) changed: user fields keep their ids but are re-allocated empty
  HIPCHK(hipStreamSynchronize(c->stream));
  for (auto &kv : c->fields) {
    HIPCHK(hipFree(kv.second.d));
    kv.second.d = nullptr;
    CHK(field_alloc(c, kv.second));
  }
  return 0;
}

extern "C" int qexhip_comm_force_halo(qexhip_handle c, int on) {
  if (!c) return QEXHIP_ERR_ARG;
  if (c->rankGeom[3] > 1) return 0;  // already on
  c->force_halo = on;
  int depth = c->g.depth ? c->g.depth : 1;
  if (geom_init(c->g, c->g.X, depth, on ? 1 : 0)) return QEXHIP_ERR_ARG;
  if (c->W) { HIPCHK(hipFree(c->W)); c->W = nullptr; c->ndir = 0; c->links_gen++; }
  return drop_fields_for_regeom(c);
}

// ---- staggered operator ----
extern "C" int qexhip_stag_set_links(qexhip_handle c, const double *fat, const double *lng) {
  if (!c || !fat) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  if (c->rankGeom[3] > 1 && !comm_ready(c)) { qexhip_set_error("rankGeom[3] = %d but qexhip_comm_init was not called", c->rankGeom[3]); return QEXHIP_ERR_STATE; }
  if (c->g.halo) {
    int depth = lng ? 3 : 1;
    if (c->g.X[3] < depth) { qexhip_set_error("local t extent %d < hop length %d", c->g.X[3], depth); return QEXHIP_ERR_ARG; }
    c->g.depth = depth;  // ghost tiles were allocated for depth 3
  }
  return links_upload(c, fat, lng);
}

static int host_in(qexhip_ctx *c, int slot, const double *host, DevField **f) {
  CHK(get_work(c, slot, f));
  return field_upload(c, **f, host);
}

extern "C" int qexhip_stag_dslash(qexhip_handle c, double *r, const double *x, int parity, double a, double b) {
  if (!c || !r || !x || parity < 0 || parity > 2) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  DevField *fx, *fr;
  CHK(host_in(c, WK_IN, x, &fx));
  CHK(host_in(c, WK_OUT, r, &fr));  // r is read when a != 0, and the untouched parity is preserved
  for (int p = (parity == 2 ? 0 : parity); p <= (parity == 2 ? 1 : parity); p++) {
    DslashOpts o;
    o.ca = a; o.cb = b; o.rin = fr; o.xs = fx;
    CHK(dslash_sweep(c, *fr, *fx, p, o));
  }
  return field_download(c, *fr, r);
}

extern "C" int qexhip_stag_D(qexhip_handle c, double *r, const double *x, double m, double sc) {
  if (!c || !r || !x || sc == 0.0) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  DevField *fx, *fr;
  CHK(host_in(c, WK_IN, x, &fx));
  CHK(get_work(c, WK_OUT, &fr));
  CHK(op_D(c, *fr, *fx, m, sc));
  return field_download(c, *fr, r);
}

extern "C" int qexhip_stag_D_acc(qexhip_handle c, double *r, const double *x, double m, double sc, double a) {
  if (!c || !r || !x || sc == 0.0) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  DevField *fx, *fr;
  CHK(host_in(c, WK_IN, x, &fx));
  CHK(host_in(c, WK_OUT, r, &fr));
  CHK(op_D(c, *fr, *fx, m, sc, a));
  return field_download(c, *fr, r);
}

extern "C" int qexhip_stag_op_xx(qexhip_handle c, double *r, const double *x, double m2, int par_even) {
  if (!c || !r || !x) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  DevField *fx, *fr;
  CHK(host_in(c, WK_IN, x, &fx));
  CHK(host_in(c, WK_OUT, r, &fr));
  CHK(op_xx(c, *fr, *fx, m2, par_even, 0, nullptr));
  return field_download(c, *fr, r);
}

int op_eo_reconstruct_pub(qexhip_ctx *c, DevField &r, DevField &b, double m);
extern "C" int qexhip_stag_eo_reconstruct(qexhip_handle c, double *r, const double *b, double m) {
  if (!c || !r || !b || m == 0.0) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  DevField *fb, *fr;
  CHK(host_in(c, WK_IN, b, &fb));
  CHK(host_in(c, WK_OUT, r, &fr));
  CHK(op_eo_reconstruct_pub(c, *fr, *fb, m));
  return field_download(c, *fr, r);
}

extern "C" int qexhip_stag_sweep_info(qexhip_handle c, int out[8]) {
  if (!c || !out) return QEXHIP_ERR_ARG;
  int lo_end = 0, hi_beg = 0, overlap = 0;
  sweep_plan(c, &lo_end, &hi_beg, &overlap);
  const int slot = c->ndir == 16;
  out[0] = c->g.halo;
  out[1] = overlap;
  out[2] = c->g.halo ? hi_beg - lo_end : c->g.Vh;
  out[3] = c->g.halo ? c->g.depth * c->g.F * 48 : 0;
  out[4] = c->overlap_auto[slot] >= 0;
  out[5] = (int)(c->overlap_tune_us[slot][0] + 0.5);
  out[6] = (int)(std::max(c->overlap_tune_us[slot][1], 0.0) + 0.5);
  out[7] = c->opt_overlap;
  return 0;
}

extern "C" int qexhip_stag_sweep_tuning(qexhip_handle c, double out[8]) {
  if (!c || !out) return QEXHIP_ERR_ARG;
  int lo_end = 0, hi_beg = 0, overlap = 0;
  sweep_plan(c, &lo_end, &hi_beg, &overlap);
  const int slot = c->ndir == 16;
  const double meas = c->xchg_us[slot];
  // (the estimate the placement falls back on where nothing was measured: dslash.hip exchange_estimate_us)
  const double link = (c->emu_link_gbs > 0 ? c->emu_link_gbs : 45.0) * 1e3;
  out[0] = meas > 0 ? meas : (c->g.halo ? 3.0 + (double)c->g.depth * c->g.F * 48.0 / link : 0.0);
  out[1] = c->g.halo && c->ndir ? sweep_push_fraction(c, hi_beg - lo_end) : 0.0;
  for (int k = 0; k < 3; k++) out[2 + k] = c->overlap_tune_us[slot][k];
  out[5] = sweep_form(c, overlap);
  out[6] = c->opt_fused_spin_us == -2 ? -1.0 : (c->opt_fused_spin_us >= 0 ? (double)c->opt_fused_spin_us : std::max(25.0, out[0]));
  out[7] = overlap;
  return 0;
}

extern "C" int qexhip_stag_stagD(qexhip_handle c, double *r, const double *x, int parity, double m, double sc, double a) {
  if (!c || !r || !x || parity < 0 || parity > 2 || sc == 0.0) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  DevField *fx, *fr;
  CHK(host_in(c, WK_IN, x, &fx));
  CHK(host_in(c, WK_OUT, r, &fr));       // r is read when a != 0; the other subset is kept
  for (int p = (parity == 2 ? 0 : parity); p <= (parity == 2 ? 1 : parity); p++) CHK(op_stagD_pub(c, *fr, *fx, p, m, sc, a));
  return field_download(c, *fr, r);
}

extern "C" int qexhip_stag_eo_reduce(qexhip_handle c, double *r, const double *b, double m) {
  if (!c || !r || !b) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  DevField *fb, *fr;
  CHK(host_in(c, WK_IN, b, &fb));
  CHK(host_in(c, WK_OUT, r, &fr));       // the odd half of r is kept
  CHK(op_eo_reduce_pub(c, *fr, *fb, m));
  return field_download(c, *fr, r);
}

extern "C" int qexhip_stag_outer(qexhip_handle c, double *f, const double *x, double scale_even, double scale_odd,
                                 int accumulate) {
  if (!c || !f || !x) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  return stag_outer_host(c, f, x, scale_even, scale_odd, accumulate);
}

// ---- solvers ----
// Host staging of the single-system entries: b into WK_IN; the solution is WK_OUT, holding the caller's x where the solve starts from it
static int stage_in(qexhip_ctx *c, double *x, const double *b, int use_prev, DevField **fx, DevField **fb) {
  if (!c || !x || !b) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  CHK(host_in(c, WK_IN, b, fb));
  return use_prev ? host_in(c, WK_OUT, x, fx) : get_work(c, WK_OUT, fx);
}

extern "C" int qexhip_stag_solve_xx(qexhip_handle c, double *x, const double *b, double mass, double r2req,
                                    int maxits, int par_even, int *iters, double *r2_over_b2, double *hist,
                                    int histcap) {
  DevField *fb, *fx;
  CHK(stage_in(c, x, b, 0, &fx, &fb));
  CHK(solve_xx_dev(c, *fx, *fb, mass, r2req, maxits, par_even, iters, r2_over_b2, hist, histcap));
  return field_download(c, *fx, x);
}

extern "C" int qexhip_stag_solve_prev(qexhip_handle c, double *x, const double *b, double mass, double r2req,
                                      int maxits, int use_prev, int *iters, double *r2_final) {
  DevField *fb, *fx;
  CHK(stage_in(c, x, b, use_prev, &fx, &fb));
  CHK(solve_full_dev(c, *fx, *fb, mass, r2req, maxits, iters, r2_final, use_prev));
  return field_download(c, *fx, x);
}

extern "C" int qexhip_stag_solve(qexhip_handle c, double *x, const double *b, double mass, double r2req,
                                 int maxits, int *iters, double *r2_final) {
  return qexhip_stag_solve_prev(c, x, b, mass, r2req, maxits, 0, iters, r2_final);
}

static int sloppy_check(qexhip_ctx *c, int sloppy) {
  if (sloppy < 0 || sloppy > 2) {
    qexhip_set_error("sloppy = %d: 0 (SloppyNone, fp64), 1 (SloppySingle) or 2 (SloppyHalf, runs single)", sloppy);
    return QEXHIP_ERR_ARG;
  }
  return 0;
}
// the single-system sloppy entries start a new report for qexhip_stag_sloppy_last
static void sloppy_last_reset(qexhip_ctx *c) { c->slp_last.precision = 0; c->slp_last.half_iters = 0; c->slp_last.f32_iters = 0; c->slp_last.fell_back = 0; }
extern "C" int qexhip_stag_sloppy_last(qexhip_handle c, int *precision, int *half_iters, int *f32_iters, int *fell_back) {
  if (!c) return QEXHIP_ERR_ARG;
  if (precision) *precision = c->slp_last.precision;
  if (half_iters) *half_iters = c->slp_last.half_iters;
  if (f32_iters) *f32_iters = c->slp_last.f32_iters;
  if (fell_back) *fell_back = c->slp_last.fell_back;
  return 0;
}

extern "C" int qexhip_stag_solve_xx_sloppy(qexhip_handle c, double *x, const double *b, double mass, double r2req, int maxits,
                                           int par_even, int sloppy, int *iters, double *r2_over_b2, int *nupdates) {
  if (!c || !x || !b) return QEXHIP_ERR_ARG;
  CHK(sloppy_check(c, sloppy));
  if (nupdates) *nupdates = 0;
  if (!sloppy) return qexhip_stag_solve_xx(c, x, b, mass, r2req, maxits, par_even, iters, r2_over_b2, nullptr, 0);
  DevField *fb, *fx;
  CHK(stage_in(c, x, b, 0, &fx, &fb));
  sloppy_last_reset(c);
  CHK(solve_xx_sloppy_any(c, sloppy, *fx, *fb, mass, r2req, maxits, par_even, iters, r2_over_b2, nupdates));
  return field_download(c, *fx, x);
}

extern "C" int qexhip_stag_solve_sloppy(qexhip_handle c, double *x, const double *b, double mass, double r2req, int maxits,
                                        int use_prev, int sloppy, int *iters, double *r2_final, int *nupdates) {
  if (!c || !x || !b) return QEXHIP_ERR_ARG;
  CHK(sloppy_check(c, sloppy));
  if (nupdates) *nupdates = 0;
  if (!sloppy) return qexhip_stag_solve_prev(c, x, b, mass, r2req, maxits, use_prev, iters, r2_final);
  DevField *fb, *fx;
  CHK(stage_in(c, x, b, use_prev, &fx, &fb));
  sloppy_last_reset(c);
  CHK(solve_full_dev(c, *fx, *fb, mass, r2req, maxits, iters, r2_final, use_prev, sloppy, nupdates));
  return field_download(c, *fx, x);
}

// Host staging of the multi-shift entries: b into WK_IN, the solutions in the persistent pool (nothing to free on any path), one of
// the three solvers -- full: Staggered.solve(xs, ...), out = r2_final; else solveXX on one parity, in fp64 (hist) or mixed precision
// (out = r2_over_b2[nmass], refine_iters) -- and the solutions down
static int multi_host(qexhip_ctx *c, double *const *xs, const double *b, const double *vals, int nmass, double r2req, int maxits,
                      int par_even, int full, int sloppy, int *iters, double *out, double *hist, int histcap, int *nupdates,
                      int *refine_iters) {
  if (!c || !xs || !b || !vals || nmass < 1) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  DevField *fb;
  CHK(host_in(c, WK_IN, b, &fb));
  if (nmass > 32) { qexhip_set_error("multishift: nmass <= 32"); return QEXHIP_ERR_ARG; }
  std::vector<DevField *> xp(nmass);
  for (int k = 0; k < nmass; k++) CHK(pool_field(c, POOL_XS + k, &xp[k]));
  if (full) CHK(solve_multi_dev(c, xp, *fb, vals, nmass, r2req, maxits, iters, out, sloppy, nupdates));
  else if (sloppy) CHK(solve_xx_multi_sloppy_dev(c, xp, *fb, vals, nmass, r2req, maxits, par_even, iters, out, nupdates, refine_iters));
  else CHK(solve_xx_multi_dev(c, xp, *fb, vals, nmass, r2req, maxits, par_even, iters, hist, histcap));
  for (int k = 0; k < nmass; k++) CHK(field_download(c, *xp[k], xs[k]));
  return 0;
}

extern "C" int qexhip_stag_solve_xx_multi(qexhip_handle c, double *const *xs, const double *b, const double *shifts,
                                          int nmass, double r2req, int maxits, int par_even, int *iters,
                                          double *hist, int histcap) {
  return multi_host(c, xs, b, shifts, nmass, r2req, maxits, par_even, 0, 0, iters, nullptr, hist, histcap, nullptr, nullptr);
}
extern "C" int qexhip_stag_solve_multi(qexhip_handle c, double *const *xs, const double *b, const double *masses,
                                       int nmass, double r2req, int maxits, int *iters, double *r2_final) {
  return multi_host(c, xs, b, masses, nmass, r2req, maxits, 1, 1, 0, iters, r2_final, nullptr, 0, nullptr, nullptr);
}

// Mixed-precision multi-shift solves.  sloppy = 0 IS the fp64 entry (nupdates = 0, refine_iters all 0); r2_over_b2[k] then is not
// computed by the fp64 solver and comes back as -1.
extern "C" int qexhip_stag_solve_xx_multi_sloppy(qexhip_handle c, double *const *xs, const double *b, const double *shifts, int nmass,
                                                 double r2req, int maxits, int par_even, int sloppy, int *iters, double *r2_over_b2,
                                                 int *nupdates, int *refine_iters) {
  if (!c || !xs || !b || !shifts) return QEXHIP_ERR_ARG;
  CHK(multi_sloppy_check(c, sloppy, shifts, nmass));
  if (nupdates) *nupdates = 0;
  if (refine_iters) for (int k = 0; k < nmass; k++) refine_iters[k] = 0;
  if (!sloppy && r2_over_b2) for (int k = 0; k < nmass; k++) r2_over_b2[k] = -1.0;
  return multi_host(c, xs, b, shifts, nmass, r2req, maxits, par_even, 0, sloppy, iters, r2_over_b2, nullptr, 0, nupdates, refine_iters);
}
extern "C" int qexhip_stag_solve_multi_sloppy(qexhip_handle c, double *const *xs, const double *b, const double *masses, int nmass,
                                              double r2req, int maxits, int sloppy, int *iters, double *r2_final, int *nupdates) {
  if (!c || !xs || !b || !masses) return QEXHIP_ERR_ARG;
  CHK(multi_sloppy_check(c, sloppy, masses, nmass));
  if (nupdates) *nupdates = 0;
  return multi_host(c, xs, b, masses, nmass, r2req, maxits, 1, 1, sloppy, iters, r2_final, nullptr, 0, nupdates, nullptr);
}

// ---- field algebra hooks ----
extern "C" int qexhip_norm2(qexhip_handle c, const double *x, int parity, double *out) {
  if (!c || !x || !out) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  DevField *fx;
  CHK(host_in(c, WK_IN, x, &fx));
  CHK(blas_norm2(c, *fx, parity, &c->dscal[8]));
  return read_scalars(c, &c->dscal[8], 1, out);
}
extern "C" int qexhip_redot(qexhip_handle c, const double *x, const double *y, int parity, double *out) {
  if (!c || !x || !y || !out) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  DevField *fx, *fy;
  CHK(host_in(c, WK_IN, x, &fx));
  CHK(host_in(c, WK_IN2, y, &fy));
  CHK(blas_redot(c, *fx, *fy, parity, &c->dscal[8]));
  return read_scalars(c, &c->dscal[8], 1, out);
}
extern "C" int qexhip_dot(qexhip_handle c, const double *x, const double *y, int parity, double out[2]) {
  if (!c || !x || !y || !out || parity < 0 || parity > 2) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  DevField *fx, *fy;
  CHK(host_in(c, WK_IN, x, &fx));
  CHK(host_in(c, WK_IN2, y, &fy));
  CHK(blas_cdot(c, *fx, *fy, parity, &c->dscal[8]));
  return read_scalars(c, &c->dscal[8], 2, out);
}
extern "C" int qexhip_axpy(qexhip_handle c, double a, const double *x, double *y, int parity) {
  if (!c || !x || !y) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  DevField *fx, *fy;
  CHK(host_in(c, WK_IN, x, &fx));
  CHK(host_in(c, WK_OUT, y, &fy));
  CHK(blas_axpy(c, a, *fx, *fy, parity));
  return field_download(c, *fy, y);
}
extern "C" int qexhip_xpay(qexhip_handle c, const double *x, double a, double *y, int parity) {
  if (!c || !x || !y) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  DevField *fx, *fy;
  CHK(host_in(c, WK_IN, x, &fx));
  CHK(host_in(c, WK_OUT, y, &fy));
  CHK(blas_xpay(c, *fx, a, *fy, parity));
  return field_download(c, *fy, y);
}

// ---- device-resident fields ----
static int find_field(qexhip_ctx *c, int id, DevField **f) {
  auto it = c->fields.find(id);
  if (id <= 0 || it == c->fields.end()) { qexhip_set_error("unknown field id %d", id); return QEXHIP_ERR_ARG; }
  *f = &it->second;
  return 0;
}
// The resident fields of one solve: the solutions x_ids[0..n), then the source.  The solvers zero every solution before they form
// |b|^2, so a solution that is the source, or another solution, would silently give b2 = 0 / one field holding the last shift
// only: refused under the entry's name `who` (by_index: the multi-shift entries, whose messages name the position in x_ids)
static int find_solve_fields(qexhip_ctx *c, const char *who, bool by_index, int n, const int *x_ids, int b_id, DevField **fx, DevField **fb) {
  for (int k = 0; k < n; k++) CHK(find_field(c, x_ids[k], &fx[k]));
  CHK(find_field(c, b_id, fb));
  for (int k = 0; k < n; k++) {
    if (x_ids[k] == b_id) {
      if (by_index) qexhip_set_error("%s: x_ids[%d] is the source field", who, k);
      else qexhip_set_error("%s: the solution field is the source field", who);
      return QEXHIP_ERR_ARG;
    }
    for (int j = 0; j < k; j++)
      if (x_ids[j] == x_ids[k]) { qexhip_set_error("%s: x_ids[%d] == x_ids[%d]", who, j, k); return QEXHIP_ERR_ARG; }
  }
  return 0;
}
// The resident fields of a call of lock-step batches.  Every solution is zeroed while its system is set up, in order: a solution
// field that is also a source (of ANY system of the call) or another system's solution would be destroyed silently -- such aliases
// are refused for the whole call
static int find_batch_fields(qexhip_ctx *c, int n, const int *x_ids, const int *b_ids, DevField **xs, DevField **bs) {
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++)
      if (x_ids[i] == b_ids[j] || (i != j && x_ids[i] == x_ids[j])) {
        qexhip_set_error("dev_solve_batch: solution field %d (system %d) aliases %s of system %d", x_ids[i], i,
                         x_ids[i] == b_ids[j] ? "the source" : "the solution", j);
        return QEXHIP_ERR_ARG;
      }
  for (int j = 0; j < n; j++) {
    CHK(find_field(c, x_ids[j], &xs[j]));
    CHK(find_field(c, b_ids[j], &bs[j]));
  }
  return 0;
}
extern "C" int qexhip_field_new(qexhip_handle c, int *id) {
  if (!c || !id) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  DevField f;
  CHK(field_alloc(c, f));
  *id = c->next_field++;
  c->fields[*id] = f;
  return 0;
}
extern "C" int qexhip_field_free(qexhip_handle c, int id) {
  if (c) c->cg_resume.valid = 0;
  if (!c) return QEXHIP_ERR_ARG;
  DevField *f;
  CHK(find_field(c, id, &f));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipFree(f->d));
  c->fields.erase(id);
  return 0;
}
extern "C" int qexhip_field_upload(qexhip_handle c, int id, const double *host) {
  if (!c || !host) return QEXHIP_ERR_ARG;
  DevField *f;
  CHK(find_field(c, id, &f));
  CHK(field_upload(c, *f, host));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}
extern "C" int qexhip_field_download(qexhip_handle c, int id, double *host) {
  if (!c || !host) return QEXHIP_ERR_ARG;
  DevField *f;
  CHK(find_field(c, id, &f));
  return field_download(c, *f, host);
}
extern "C" int qexhip_field_zero(qexhip_handle c, int id) {
  if (!c) return QEXHIP_ERR_ARG;
  DevField *f;
  CHK(find_field(c, id, &f));
  return blas_zero(c, *f, 2);
}
extern "C" int qexhip_dev_dslash(qexhip_handle c, int r_id, int x_id, int parity, double a, double b) {
  if (!c || parity < 0 || parity > 2) return QEXHIP_ERR_ARG;
  DevField *fr, *fx;
  CHK(find_field(c, r_id, &fr));
  CHK(find_field(c, x_id, &fx));
  for (int p = (parity == 2 ? 0 : parity); p <= (parity == 2 ? 1 : parity); p++) {
    DslashOpts o;
    o.ca = a; o.cb = b; o.rin = fr; o.xs = fx;
    CHK(dslash_sweep(c, *fr, *fx, p, o));
  }
  return 0;
}
extern "C" int qexhip_dev_op_xx(qexhip_handle c, int r_id, int x_id, double m2, int par_even) {
  if (!c) return QEXHIP_ERR_ARG;
  DevField *fr, *fx;
  CHK(find_field(c, r_id, &fr));
  CHK(find_field(c, x_id, &fx));
  return op_xx(c, *fr, *fx, m2, par_even, 0, nullptr);
}
extern "C" int qexhip_dev_solve_xx(qexhip_handle c, int x_id, int b_id, double mass, double r2req, int maxits,
                                   int par_even, int *iters, double *r2_over_b2, double *hist, int histcap) {
  if (!c) return QEXHIP_ERR_ARG;
  DevField *fx, *fb;
  CHK(find_field(c, x_id, &fx));
  CHK(find_field(c, b_id, &fb));
  return solve_xx_dev(c, *fx, *fb, mass, r2req, maxits, par_even, iters, r2_over_b2, hist, histcap);
}

extern "C" int qexhip_dev_solve_xx_sloppy(qexhip_handle c, int x_id, int b_id, double mass, double r2req, int maxits, int par_even,
                                          int sloppy, int *iters, double *r2_over_b2, int *nupdates) {
  if (!c) return QEXHIP_ERR_ARG;
  CHK(sloppy_check(c, sloppy));
  if (nupdates) *nupdates = 0;
  if (!sloppy) return qexhip_dev_solve_xx(c, x_id, b_id, mass, r2req, maxits, par_even, iters, r2_over_b2, nullptr, 0);
  HIPCHK(hipSetDevice(c->device));
  DevField *fx, *fb;
  CHK(find_solve_fields(c, "dev_solve_xx_sloppy", false, 1, &x_id, b_id, &fx, &fb));
  sloppy_last_reset(c);
  return solve_xx_sloppy_any(c, sloppy, *fx, *fb, mass, r2req, maxits, par_even, iters, r2_over_b2, nupdates);
}
extern "C" int qexhip_dev_op_xx_sloppy(qexhip_handle c, int r_id, int x_id, double m2, int par_even) {
  if (!c) return QEXHIP_ERR_ARG;
  CHK(sloppy_check(c, 1));
  HIPCHK(hipSetDevice(c->device));
  DevField *fr, *fx;
  CHK(find_field(c, r_id, &fr));
  CHK(find_field(c, x_id, &fx));
  DevFieldF *xi, *ro;
  CHK(f32_field(c, F32_IN, &xi));
  CHK(f32_field(c, F32_AP, &ro));
  const int px = par_even ? 0 : 1;
  CHK(f32_from_f64(c, *xi, *fx, px, 1.0));
  CHK(f32_op_xx(c, *ro, *xi, m2, par_even, 0, nullptr, nullptr));
  return f32_to_f64(c, *fr, *ro, px, 1.0, 0);
}
// the 16-bit counterpart of qexhip_dev_op_xx_sloppy: x rounded to the 16-bit format, two 16-bit sweeps, the result back in fp64
extern "C" int qexhip_dev_op_xx_half(qexhip_handle c, int r_id, int x_id, double m2, int par_even) {
  if (!c) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  DevField *fr, *fx;
  CHK(find_field(c, r_id, &fr));
  CHK(find_field(c, x_id, &fx));
  return half_op_xx_probe(c, *fr, *fx, m2, par_even);
}
// the batched form of qexhip_dev_op_xx_half: n <= 4 fields rounded to the 16-bit format, ONE batched op_xx (two multi-RHS 16-bit sweeps),
// the results back in fp64
extern "C" int qexhip_dev_op_xx_half_batch(qexhip_handle c, int n, const int *r_ids, const int *x_ids, const double *m2, int par_even) {
  if (!c || !r_ids || !x_ids || !m2) return QEXHIP_ERR_ARG;
  if (n < 1 || n > 4) { qexhip_set_error("dev_op_xx_half_batch: 1 <= n <= 4"); return QEXHIP_ERR_ARG; }
  HIPCHK(hipSetDevice(c->device));
  DevField *fr[4], *fx[4];
  for (int j = 0; j < n; j++) {
    CHK(find_field(c, r_ids[j], &fr[j]));
    CHK(find_field(c, x_ids[j], &fx[j]));
  }
  return half_op_xx_batch_probe(c, n, fr, fx, m2, par_even);
}
// the fp32 twin of qexhip_dev_op_xx_half_batch: n <= 4 fields rounded to fp32, ONE batched op_xx (two multi-RHS fp32 sweeps), back in fp64
extern "C" int qexhip_dev_op_xx_sloppy_batch(qexhip_handle c, int n, const int *r_ids, const int *x_ids, const double *m2, int par_even) {
  if (!c || !r_ids || !x_ids || !m2) return QEXHIP_ERR_ARG;
  if (n < 1 || n > 4) { qexhip_set_error("dev_op_xx_sloppy_batch: 1 <= n <= 4"); return QEXHIP_ERR_ARG; }
  CHK(sloppy_check(c, 1));
  HIPCHK(hipSetDevice(c->device));
  DevField *fr[4], *fx[4];
  for (int j = 0; j < n; j++) {
    CHK(find_field(c, r_ids[j], &fr[j]));
    CHK(find_field(c, x_ids[j], &fx[j]));
  }
  return f32_op_xx_batch_probe(c, n, fr, fx, m2, par_even);
}
// what the last batched sloppy call ran per system: n <- its systems; arrays of n_max entries, the first min(n, n_max) filled
extern "C" int qexhip_stag_sloppy_last_batch(qexhip_handle c, int n_max, int *n, int *precision, int *half_iters, int *f32_iters,
                                             int *fell_back) {
  if (!c || n_max < 0) return QEXHIP_ERR_ARG;
  const auto &l = c->slpb_last;
  if (n) *n = l.n;
  for (int j = 0; j < l.n && j < n_max; j++) {
    if (precision) precision[j] = l.precision[j];
    if (half_iters) half_iters[j] = l.half_iters[j];
    if (f32_iters) f32_iters[j] = l.f32_iters[j];
    if (fell_back) fell_back[j] = l.fell_back[j];
  }
  return 0;
}
extern "C" int qexhip_stag_links_info_half(qexhip_handle c, int *format, double *s_fat, double *s_long, double *max_dev) {
  if (!c) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  return half_links(c, format, s_fat, s_long, max_dev);
}
extern "C" int qexhip_half_pack_host(const double *v, size_t nsites, int16_t *q, float *norm) {
  if (!v || !q || !norm) return QEXHIP_ERR_ARG;
  return half_pack_host(v, nsites, q, norm);
}
extern "C" int qexhip_half_unpack_host(const int16_t *q, const float *norm, size_t nsites, double *v) {
  if (!v || !q || !norm) return QEXHIP_ERR_ARG;
  return half_unpack_host(q, norm, nsites, v);
}
extern "C" int qexhip_stag_links_info_f32(qexhip_handle c, int *format, double *max_dev) {
  if (!c) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  return f32_links(c, format, max_dev);
}

extern "C" int qexhip_dev_solve_xx_continue(qexhip_handle c, int x_id, double r2req, int maxits, int *iters, double *r2_over_b2,
                                            double *hist, int histcap) {
  if (!c) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  DevField *fx;
  CHK(find_field(c, x_id, &fx));
  return solve_xx_continue_dev(c, *fx, r2req, maxits, iters, r2_over_b2, hist, histcap);
}

extern "C" int qexhip_dev_solve_xx_multi(qexhip_handle c, const int *x_ids, int b_id, const double *shifts, int nmass,
                                         double r2req, int maxits, int par_even, int *iters, double *hist, int histcap) {
  if (!c || !x_ids || !shifts || nmass < 1 || nmass > 32) return QEXHIP_ERR_ARG;
  DevField *fb;
  std::vector<DevField *> xp(nmass);
  CHK(find_solve_fields(c, "dev_solve_xx_multi", true, nmass, x_ids, b_id, xp.data(), &fb));
  return solve_xx_multi_dev(c, xp, *fb, shifts, nmass, r2req, maxits, par_even, iters, hist, histcap);
}
// qexhip_stag_solve_xx_multi_sloppy on resident fields
extern "C" int qexhip_dev_solve_xx_multi_sloppy(qexhip_handle c, const int *x_ids, int b_id, const double *shifts, int nmass,
                                                double r2req, int maxits, int par_even, int sloppy, int *iters, double *r2_over_b2,
                                                int *nupdates, int *refine_iters) {
  if (!c || !x_ids || !shifts) return QEXHIP_ERR_ARG;
  CHK(multi_sloppy_check(c, sloppy, shifts, nmass));
  if (nupdates) *nupdates = 0;
  if (refine_iters) for (int k = 0; k < nmass; k++) refine_iters[k] = 0;
  if (!sloppy) {
    if (r2_over_b2) for (int k = 0; k < nmass; k++) r2_over_b2[k] = -1.0;
    return qexhip_dev_solve_xx_multi(c, x_ids, b_id, shifts, nmass, r2req, maxits, par_even, iters, nullptr, 0);
  }
  HIPCHK(hipSetDevice(c->device));
  DevField *fb;
  std::vector<DevField *> xp(nmass);
  CHK(find_solve_fields(c, "dev_solve_xx_multi_sloppy", true, nmass, x_ids, b_id, xp.data(), &fb));
  return solve_xx_multi_sloppy_dev(c, xp, *fb, shifts, nmass, r2req, maxits, par_even, iters, r2_over_b2, nupdates, refine_iters);
}

// out[par] = r(M^+M) b[par], r(x) = f0 + sum_k alpha_k / (x + beta_k), by the accumulating multi-shift solve (multishift.hip).  Every
// refusal comes before anything is launched or staged
extern "C" int qexhip_dev_rational_xx(qexhip_handle c, int out_id, int b_id, double mass, double f0, int nterm, const double *alpha,
                                      const double *beta, double r2req, int maxits, int par_even, int *iters, double *hist, int histcap) {
  if (!c) return QEXHIP_ERR_ARG;
  double shifts[CGM_MAXM];
  int order[CGM_MAXM];
  CHK(rational_map("dev_rational_xx", mass, nterm, alpha, beta, shifts, order));
  if (!std::isfinite(f0)) { qexhip_set_error("dev_rational_xx: f0 is not finite"); return QEXHIP_ERR_ARG; }
  DevField *fo, *fb;
  CHK(find_solve_fields(c, "dev_rational_xx", false, 1, &out_id, b_id, &fo, &fb));
  HIPCHK(hipSetDevice(c->device));
  return rational_xx_dev(c, *fo, *fb, mass, f0, nterm, alpha, beta, r2req, maxits, par_even, iters, hist, histcap);
}
extern "C" int qexhip_stag_rational_xx(qexhip_handle c, double *out, const double *b, double mass, double f0, int nterm, const double *alpha,
                                       const double *beta, double r2req, int maxits, int par_even, int *iters, double *hist, int histcap) {
  if (!c || !out || !b) return QEXHIP_ERR_ARG;
  double shifts[CGM_MAXM];
  int order[CGM_MAXM];
  CHK(rational_map("stag_rational_xx", mass, nterm, alpha, beta, shifts, order));
  if (!std::isfinite(f0)) { qexhip_set_error("stag_rational_xx: f0 is not finite"); return QEXHIP_ERR_ARG; }
  DevField *fb, *fx;
  CHK(stage_in(c, out, b, 0, &fx, &fb));
  CHK(rational_xx_dev(c, *fx, *fb, mass, f0, nterm, alpha, beta, r2req, maxits, par_even, iters, hist, histcap));
  return field_download(c, *fx, out);
}

// The multi-shift solvers keep up to 3 x nmass full fields (search directions, per-parity and host-entry solutions) between
// calls so that a trajectory's repeated solves allocate nothing; a host that is about to need the memory for something
// else (the 52-field nHYP closure, a larger batch) hands it back here.  The next multi-shift solve re-allocates.
extern "C" int qexhip_release_workspace(qexhip_handle c) {
  if (!c) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (auto it = c->fields.begin(); it != c->fields.end();) {
    if (it->first <= -1000) {
      HIPCHK(hipFree(it->second.d));
      it = c->fields.erase(it);
    } else {
      ++it;
    }
  }
  gauge_release_scratch(c);
  f32_state_free(c);                 // the mixed-precision CG's fp32 links and fields: rebuilt by the next sloppy solve
  half_state_free(c);                // and its 16-bit links and fields
  msf_state_free(c);                 // and the mixed multi-shift CG's fp32 search directions / increments
  batch_f32_state_free(c);           // and the batched form's fp32 fields
  batch_half_state_free(c);          // and its 16-bit fields
  gfix_state_free(c);                // and the gauge-fixing transform with its polish scratch (qexhip_gfix_set_transform re-creates it)
  eig_state_free(c);                 // and the eigensolver's Lanczos work fields and buffers (never the user's bases)
  stout_state_free(c);               // and the stout chain with the scratch of smear / inverse (qexhip_stout_prepare re-creates it)
  return 0;
}

// ---- low modes and deflation (eig.hip, eigsolve.cpp, solver.cpp) ----
extern "C" int qexhip_eig_new(qexhip_handle c, int nvecs, int *basis) {
  if (nvecs < 1 || nvecs > EIG_MAX_NVECS) { qexhip_set_error("eig_new: 1 <= nvecs <= %d (nvecs = %d)", EIG_MAX_NVECS, nvecs); return QEXHIP_ERR_ARG; }
  if (!c || !basis) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  return eig_basis_new(c, nvecs, basis);
}
extern "C" int qexhip_eig_free(qexhip_handle c, int basis) {
  if (!c) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  return eig_basis_free(c, basis);
}
extern "C" int qexhip_eig_get_vector(qexhip_handle c, int basis, int i, int field_id) {
  if (!c) return QEXHIP_ERR_ARG;
  EigBasis *B; DevField *f;
  CHK(eig_basis_find(c, basis, &B));
  CHK(find_field(c, field_id, &f));
  HIPCHK(hipSetDevice(c->device));
  return eig_get_vector(c, *B, i, *f);
}
extern "C" int qexhip_eig_set_vector(qexhip_handle c, int basis, int i, int field_id) {
  if (!c) return QEXHIP_ERR_ARG;
  EigBasis *B; DevField *f;
  CHK(eig_basis_find(c, basis, &B));
  CHK(find_field(c, field_id, &f));
  HIPCHK(hipSetDevice(c->device));
  return eig_set_vector(c, *B, i, *f);
}
extern "C" int qexhip_eig_block_dot(qexhip_handle c, int basis, int i0, int n, int w_field_id, double *out) {
  if (!c || !out) return QEXHIP_ERR_ARG;
  EigBasis *B; DevField *f;
  CHK(eig_basis_find(c, basis, &B));
  CHK(find_field(c, w_field_id, &f));
  if (i0 < 0 || n < 1 || i0 > B->nvecs - n) { qexhip_set_error("eig_block_dot: vectors %d..%d of a basis of %d", i0, i0 + n - 1, B->nvecs); return QEXHIP_ERR_ARG; }
  HIPCHK(hipSetDevice(c->device));
  double2 *dots;
  CHK(eig_coef_buffers(c, &dots, nullptr));
  CHK(eig_block_dot(c, *B, i0, n, *f, dots));
  HIPCHK(hipMemcpyAsync(out, dots, sizeof(double) * 2 * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return peer_check(c);
}
extern "C" int qexhip_eig_block_axpy(qexhip_handle c, int basis, int i0, int n, const double *coef, int y_field_id) {
  if (!c || !coef) return QEXHIP_ERR_ARG;
  EigBasis *B; DevField *f;
  CHK(eig_basis_find(c, basis, &B));
  CHK(find_field(c, y_field_id, &f));
  if (i0 < 0 || n < 1 || i0 > B->nvecs - n) { qexhip_set_error("eig_block_axpy: vectors %d..%d of a basis of %d", i0, i0 + n - 1, B->nvecs); return QEXHIP_ERR_ARG; }
  HIPCHK(hipSetDevice(c->device));
  double2 *cf;
  CHK(eig_coef_buffers(c, nullptr, &cf));
  HIPCHK(hipMemcpyAsync(cf, coef, sizeof(double) * 2 * n, hipMemcpyHostToDevice, c->stream));
  CHK(eig_block_axpy(c, *B, i0, n, cf, 1.0, *f));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}
// the multi-right-hand-side forms (the projections of the deflated lock-step batch): out[nrhs][n][2], coef[nrhs][n][2]
static int eig_multi_args(qexhip_ctx *c, int basis, int i0, int n, int nrhs, const int *ids, bool distinct, const char *who, EigBasis **B, DevField **f) {
  CHK(eig_basis_find(c, basis, B));
  if (nrhs < 1 || nrhs > EIG_MAXRHS) { qexhip_set_error("%s: 1 <= nrhs <= %d (nrhs = %d)", who, EIG_MAXRHS, nrhs); return QEXHIP_ERR_ARG; }
  if (i0 < 0 || n < 1 || i0 > (*B)->nvecs - n) { qexhip_set_error("%s: vectors %d..%d of a basis of %d", who, i0, i0 + n - 1, (*B)->nvecs); return QEXHIP_ERR_ARG; }
  for (int k = 0; k < nrhs; k++) {
    CHK(find_field(c, ids[k], &f[k]));
    for (int q = 0; distinct && q < k; q++)
      if (ids[q] == ids[k]) { qexhip_set_error("%s: fields %d and %d are the same (id %d)", who, q, k, ids[k]); return QEXHIP_ERR_ARG; }
  }
  return 0;
}
extern "C" int qexhip_eig_block_dot_multi(qexhip_handle c, int basis, int i0, int n, int nrhs, const int *w_ids, double *out) {
  if (!c || !w_ids || !out) return QEXHIP_ERR_ARG;
  EigBasis *B; DevField *f[EIG_MAXRHS];
  CHK(eig_multi_args(c, basis, i0, n, nrhs, w_ids, false, "eig_block_dot_multi", &B, f));
  HIPCHK(hipSetDevice(c->device));
  double2 *dots;
  CHK(eig_coef_buffers(c, &dots, nullptr));
  CHK(eig_block_dot_mrhs(c, *B, i0, n, nrhs, f, dots));
  HIPCHK(hipMemcpyAsync(out, dots, sizeof(double) * 2 * n * nrhs, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return peer_check(c);
}
extern "C" int qexhip_eig_block_axpy_multi(qexhip_handle c, int basis, int i0, int n, int nrhs, const double *coef, const int *y_ids) {
  if (!c || !coef || !y_ids) return QEXHIP_ERR_ARG;
  EigBasis *B; DevField *f[EIG_MAXRHS];
  CHK(eig_multi_args(c, basis, i0, n, nrhs, y_ids, true, "eig_block_axpy_multi", &B, f));
  HIPCHK(hipSetDevice(c->device));
  double2 *cf;
  CHK(eig_coef_buffers(c, nullptr, &cf));
  HIPCHK(hipMemcpyAsync(cf, coef, sizeof(double) * 2 * n * nrhs, hipMemcpyHostToDevice, c->stream));
  CHK(eig_block_axpy_mrhs(c, *B, i0, n, nrhs, cf, 1.0, f));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}
extern "C" int qexhip_eig_rotate(qexhip_handle c, int basis, int m, int k, const double *Q) {
  if (!c || !Q) return QEXHIP_ERR_ARG;
  EigBasis *B;
  CHK(eig_basis_find(c, basis, &B));
  HIPCHK(hipSetDevice(c->device));
  CHK(eig_rotate(c, *B, m, k, Q));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}
extern "C" int qexhip_stag_eigs(qexhip_handle c, int basis, const qexhip_eig_opts *o, int *nconv, double *evals, double *resid, long stats[4]) {
  CHK(qexhip_eig_check_opts(o));
  if (!c) return QEXHIP_ERR_ARG;
  EigBasis *B;
  CHK(eig_basis_find(c, basis, &B));
  if (o->nvecs > B->nvecs) { qexhip_set_error("eigs: nvecs = %d but the basis holds %d vectors", o->nvecs, B->nvecs); return QEXHIP_ERR_ARG; }
  if (!c->W) { qexhip_set_error("eigs: no links set"); return QEXHIP_ERR_STATE; }
  HIPCHK(hipSetDevice(c->device));
  return eig_solve(c, *B, *o, nconv, evals, resid, stats);
}
extern "C" int qexhip_eig_evals(qexhip_handle c, int basis, int n, double *evals) {
  if (!c || !evals) return QEXHIP_ERR_ARG;
  EigBasis *B;
  CHK(eig_basis_find(c, basis, &B));
  if (n < 0 || n > B->nvecs) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  CHK(eig_rayleigh(c, *B, n));
  for (int i = 0; i < n; i++) evals[i] = B->evals[i];
  return 0;
}
static int deflate_args(qexhip_ctx *c, int basis, int nev, int sloppy, double mass, EigBasis **B) {
  CHK(sloppy_check(c, sloppy));
  CHK(eig_basis_find(c, basis, B));
  if (nev < 0 || nev > (*B)->nvecs) { qexhip_set_error("deflated solve: nev = %d of a basis of %d vectors", nev, (*B)->nvecs); return QEXHIP_ERR_ARG; }
  if (sloppy && mass == 0.0) { qexhip_set_error("sloppy solve: mass 0 unsupported"); return QEXHIP_ERR_ARG; }
  return 0;
}
extern "C" int qexhip_dev_solve_xx_deflated(qexhip_handle c, int basis, int nev, int x_id, int b_id, double mass, double r2req, int maxits,
                                            int sloppy, int *iters, double *r2_over_b2) {
  if (!c) return QEXHIP_ERR_ARG;
  EigBasis *B;
  CHK(deflate_args(c, basis, nev, sloppy, mass, &B));
  DevField *fx, *fb;
  CHK(find_solve_fields(c, "dev_solve_xx_deflated", false, 1, &x_id, b_id, &fx, &fb));
  HIPCHK(hipSetDevice(c->device));
  sloppy_last_reset(c);
  return solve_xx_deflated_dev(c, *B, nev, *fx, *fb, mass, r2req, maxits, sloppy, iters, r2_over_b2);
}
extern "C" int qexhip_stag_solve_xx_deflated(qexhip_handle c, int basis, int nev, double *x, const double *b, double mass, double r2req,
                                             int maxits, int sloppy, int *iters, double *r2_over_b2) {
  if (!c || !x || !b) return QEXHIP_ERR_ARG;
  EigBasis *B;
  CHK(deflate_args(c, basis, nev, sloppy, mass, &B));
  DevField *fb, *fx;
  CHK(stage_in(c, x, b, 0, &fx, &fb));
  sloppy_last_reset(c);
  CHK(solve_xx_deflated_dev(c, *B, nev, *fx, *fb, mass, r2req, maxits, sloppy, iters, r2_over_b2));
  return field_download(c, *fx, x);
}
extern "C" int qexhip_stag_solve_deflated(qexhip_handle c, int basis, int nev, double *x, const double *b, double mass, double r2req,
                                          int maxits, int sloppy, int *iters, double *r2_final) {
  if (!c || !x || !b) return QEXHIP_ERR_ARG;
  EigBasis *B;
  CHK(deflate_args(c, basis, nev, sloppy, mass, &B));
  if (B->gen != c->links_gen) { qexhip_set_error("deflated solve: the basis was computed on other links"); return QEXHIP_ERR_STATE; }
  DevField *fb, *fx;
  CHK(stage_in(c, x, b, 0, &fx, &fb));
  c->deflate_basis = basis; c->deflate_nev = nev;
  sloppy_last_reset(c);
  const int rc = solve_full_dev(c, *fx, *fb, mass, r2req, maxits, iters, r2_final, 0, sloppy, nullptr);
  c->deflate_basis = 0; c->deflate_nev = 0;
  CHK(rc);
  return field_download(c, *fx, x);
}

// norm2 / redot / Staggered.D on resident fields (the host-pointer forms above upload their arguments first)
extern "C" int qexhip_dev_norm2(qexhip_handle c, int x_id, int parity, double *out) {
  if (!c || !out || parity < 0 || parity > 2) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  DevField *fx;
  CHK(find_field(c, x_id, &fx));
  CHK(blas_norm2(c, *fx, parity, &c->dscal[8]));
  return read_scalars(c, &c->dscal[8], 1, out);
}
extern "C" int qexhip_dev_redot(qexhip_handle c, int x_id, int y_id, int parity, double *out) {
  if (!c || !out || parity < 0 || parity > 2) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  DevField *fx, *fy;
  CHK(find_field(c, x_id, &fx));
  CHK(find_field(c, y_id, &fy));
  CHK(blas_redot(c, *fx, *fy, parity, &c->dscal[8]));
  return read_scalars(c, &c->dscal[8], 1, out);
}
extern "C" int qexhip_dev_dot(qexhip_handle c, int x_id, int y_id, int parity, double out[2]) {
  if (!c || !out || parity < 0 || parity > 2) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  DevField *fx, *fy;
  CHK(find_field(c, x_id, &fx));
  CHK(find_field(c, y_id, &fy));
  CHK(blas_cdot(c, *fx, *fy, parity, &c->dscal[8]));
  return read_scalars(c, &c->dscal[8], 2, out);
}
extern "C" int qexhip_dev_D(qexhip_handle c, int r_id, int x_id, double m, double sc) {
  if (!c || r_id == x_id) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  DevField *fr, *fx;
  CHK(find_field(c, r_id, &fr));
  CHK(find_field(c, x_id, &fx));
  return op_D(c, *fr, *fx, m, sc);
}

// ---- meson tables, symmetric shift, slice norms (fpvaMeas.nim:16-61, stagMesonLocal.nim:14-51, sources.nim:10-18) ----
extern "C" int qexhip_dev_meson_corners(qexhip_handle c, int n, const int *x_ids, const int *y_ids, int t0, double *out) {
  if (!c) return QEXHIP_ERR_ARG;
  if (!x_ids || !y_ids || !out) { qexhip_set_error("dev_meson_corners: null argument"); return QEXHIP_ERR_ARG; }
  if (n < 1 || n > 4) { qexhip_set_error("dev_meson_corners: n = %d, must be 1..4", n); return QEXHIP_ERR_ARG; }
  const int ntg = c->g.X[3] * c->rankGeom[3];
  if (t0 < 0 || t0 >= ntg) { qexhip_set_error("dev_meson_corners: t0 = %d outside [0, %d)", t0, ntg); return QEXHIP_ERR_ARG; }
  HIPCHK(hipSetDevice(c->device));
  DevField *xs[4], *ys[4];
  for (int k = 0; k < n; k++) {
    CHK(find_field(c, x_ids[k], &xs[k]));
    CHK(find_field(c, y_ids[k], &ys[k]));
  }
  return meson_corners(c, n, xs, ys, t0, out);
}
extern "C" int qexhip_dev_sym_shift(qexhip_handle c, int r_id, int x_id, int mu) {
  if (!c) return QEXHIP_ERR_ARG;
  if (mu < 0 || mu > 2) { qexhip_set_error("dev_sym_shift: mu = %d, only the spatial directions 0..2 are shifted", mu); return QEXHIP_ERR_ARG; }
  if (r_id == x_id) { qexhip_set_error("dev_sym_shift: r_id == x_id"); return QEXHIP_ERR_ARG; }
  if (!c->W) { qexhip_set_error("dev_sym_shift: no links set (qexhip_stag_set_links first)"); return QEXHIP_ERR_ARG; }
  HIPCHK(hipSetDevice(c->device));
  DevField *fr, *fx;
  CHK(find_field(c, r_id, &fr));
  CHK(find_field(c, x_id, &fx));
  return sym_shift(c, *fr, *fx, mu);
}
extern "C" int qexhip_dev_norm2slice(qexhip_handle c, int id, int dir, double *out) {
  if (!c) return QEXHIP_ERR_ARG;
  if (!out) { qexhip_set_error("dev_norm2slice: null argument"); return QEXHIP_ERR_ARG; }
  if (dir < 0 || dir > 3) { qexhip_set_error("dev_norm2slice: dir = %d, must be 0..3", dir); return QEXHIP_ERR_ARG; }
  HIPCHK(hipSetDevice(c->device));
  DevField *f;
  CHK(find_field(c, id, &f));
  return norm2slice(c, *f, dir, out);
}

// ---- stochastic scalar trace (scalarTrace.nim, dilution.nim): complex site fields, dilution, <a, b> accumulation, slice sums ----
static int find_cfield(qexhip_ctx *c, int id, DevCField **f) {
  auto it = c->cfields.find(id);
  if (id <= 0 || it == c->cfields.end()) { qexhip_set_error("unknown cfield id %d", id); return QEXHIP_ERR_ARG; }
  *f = &it->second;
  return 0;
}
extern "C" int qexhip_cfield_new(qexhip_handle c, int *id) {
  if (!c || !id) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  DevCField f;
  CHK(cfield_alloc(c, f));
  *id = c->next_cfield++;
  c->cfields[*id] = f;
  return 0;
}
extern "C" int qexhip_cfield_free(qexhip_handle c, int id) {
  if (!c) return QEXHIP_ERR_ARG;
  DevCField *f;
  CHK(find_cfield(c, id, &f));
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipFree(f->d));
  c->cfields.erase(id);
  return 0;
}
extern "C" int qexhip_cfield_zero(qexhip_handle c, int id) {
  if (!c) return QEXHIP_ERR_ARG;
  DevCField *f;
  CHK(find_cfield(c, id, &f));
  HIPCHK(hipSetDevice(c->device));
  return cfield_zero(c, *f);
}
extern "C" int qexhip_cfield_scale(qexhip_handle c, int id, double s) {
  if (!c) return QEXHIP_ERR_ARG;
  DevCField *f;
  CHK(find_cfield(c, id, &f));
  HIPCHK(hipSetDevice(c->device));
  return cfield_scale(c, *f, s);
}
extern "C" int qexhip_cfield_axpy(qexhip_handle c, int dst, double a, int src) {
  if (!c) return QEXHIP_ERR_ARG;
  if (!std::isfinite(a)) { qexhip_set_error("cfield_axpy: a is not finite"); return QEXHIP_ERR_ARG; }
  DevCField *fd, *fs;
  CHK(find_cfield(c, dst, &fd));
  CHK(find_cfield(c, src, &fs));
  if (dst == src) { qexhip_set_error("cfield_axpy: dst and src are the same cfield %d", dst); return QEXHIP_ERR_ARG; }
  HIPCHK(hipSetDevice(c->device));
  return cfield_axpy(c, *fd, a, *fs);
}
extern "C" int qexhip_cfield_download(qexhip_handle c, int id, double *host) {
  if (!c) return QEXHIP_ERR_ARG;
  if (!host) { qexhip_set_error("cfield_download: null argument"); return QEXHIP_ERR_ARG; }
  DevCField *f;
  CHK(find_cfield(c, id, &f));
  HIPCHK(hipSetDevice(c->device));
  return cfield_download(c, *f, host);
}
extern "C" int qexhip_dev_dilute(qexhip_handle c, int n, const int *dst_ids, int src_id, int kind, const int *idx, const int *t,
                                 double scale) {
  if (!c) return QEXHIP_ERR_ARG;
  if (!dst_ids || !idx || !t) { qexhip_set_error("dev_dilute: null argument"); return QEXHIP_ERR_ARG; }
  if (n < 1 || n > 4) { qexhip_set_error("dev_dilute: n = %d, must be 1..4", n); return QEXHIP_ERR_ARG; }
  if (kind < 0 || kind > 1) { qexhip_set_error("dev_dilute: kind = %d, must be 0 (EO) or 1 (CORNER)", kind); return QEXHIP_ERR_ARG; }
  const int ntg = c->g.X[3] * c->rankGeom[3], npat = kind == 0 ? 2 : 8;
  DevField *src, *dst[4];
  CHK(find_field(c, src_id, &src));
  for (int k = 0; k < n; k++) {
    if (idx[k] < 0 || idx[k] >= npat) { qexhip_set_error("dev_dilute: idx[%d] = %d outside [0, %d)", k, idx[k], npat); return QEXHIP_ERR_ARG; }
    if (t[k] < 0 || t[k] >= ntg) { qexhip_set_error("dev_dilute: t[%d] = %d outside [0, %d)", k, t[k], ntg); return QEXHIP_ERR_ARG; }
    if (dst_ids[k] == src_id) { qexhip_set_error("dev_dilute: destination %d is the source field %d", k, src_id); return QEXHIP_ERR_ARG; }
    for (int j = 0; j < k; j++)
      if (dst_ids[j] == dst_ids[k]) { qexhip_set_error("dev_dilute: destinations %d and %d are the same field %d", j, k, dst_ids[k]); return QEXHIP_ERR_ARG; }
    CHK(find_field(c, dst_ids[k], &dst[k]));
  }
  HIPCHK(hipSetDevice(c->device));
  return trace_dilute(c, n, dst, *src, kind, idx, t, scale);
}
extern "C" int qexhip_dev_trace_accum(qexhip_handle c, int cfield, int n, const int *a_ids, const int *b_ids, double coef) {
  if (!c) return QEXHIP_ERR_ARG;
  if (!a_ids || !b_ids) { qexhip_set_error("dev_trace_accum: null argument"); return QEXHIP_ERR_ARG; }
  if (n < 1 || n > 4) { qexhip_set_error("dev_trace_accum: n = %d, must be 1..4", n); return QEXHIP_ERR_ARG; }
  DevCField *tr;
  CHK(find_cfield(c, cfield, &tr));
  DevField *a[4], *b[4];
  for (int k = 0; k < n; k++) {
    CHK(find_field(c, a_ids[k], &a[k]));
    CHK(find_field(c, b_ids[k], &b[k]));
  }
  HIPCHK(hipSetDevice(c->device));
  return trace_accum(c, *tr, n, a, b, coef);
}
extern "C" int qexhip_dev_cfield_slices(qexhip_handle c, int cfield, double *out) {
  if (!c) return QEXHIP_ERR_ARG;
  if (!out) { qexhip_set_error("dev_cfield_slices: null argument"); return QEXHIP_ERR_ARG; }
  DevCField *tr;
  CHK(find_cfield(c, cfield, &tr));
  HIPCHK(hipSetDevice(c->device));
  return cfield_slices(c, *tr, out);
}

// ---- low-mode averaging of the scalar trace (eig.hip): the exact low-mode diagonal and phi <- (1 - P) phi ----
extern "C" int qexhip_eig_block_norm2_accum(qexhip_handle c, int basis, int i0, int n, const double *wgt, int cfield) {
  if (!c || !wgt) return QEXHIP_ERR_ARG;
  EigBasis *B; DevCField *cf;
  CHK(eig_basis_find(c, basis, &B));
  CHK(find_cfield(c, cfield, &cf));
  if (i0 < 0 || n < 1 || i0 > B->nvecs - n) { qexhip_set_error("eig_block_norm2_accum: vectors %d..%d of a basis of %d", i0, i0 + n - 1, B->nvecs); return QEXHIP_ERR_ARG; }
  HIPCHK(hipSetDevice(c->device));
  double2 *buf;
  CHK(eig_coef_buffers(c, nullptr, &buf));
  HIPCHK(hipMemcpyAsync(buf, wgt, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  CHK(eig_block_norm2_accum(c, *B, i0, n, (const double *)buf, *cf));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}
// (nev and the basis's links are checked by eig_lowmode_diag / eig_project_out themselves, before they launch anything)
static int lowmode_args(qexhip_ctx *c, int basis, const char *who, EigBasis **B) {
  CHK(eig_basis_find(c, basis, B));
  if (!c->W) { qexhip_set_error("%s: no links set", who); return QEXHIP_ERR_STATE; }
  return 0;
}
extern "C" int qexhip_eig_lowmode_diag(qexhip_handle c, int basis, int nev, double mass, int cfield) {
  if (!c) return QEXHIP_ERR_ARG;
  if (!std::isfinite(mass) || !(mass > 0)) { qexhip_set_error("eig_lowmode_diag: the mass must be finite and positive"); return QEXHIP_ERR_ARG; }
  EigBasis *B; DevCField *cf;
  CHK(find_cfield(c, cfield, &cf));
  CHK(lowmode_args(c, basis, "eig_lowmode_diag", &B));
  HIPCHK(hipSetDevice(c->device));
  CHK(eig_lowmode_diag(c, *B, nev, mass, *cf));
  HIPCHK(hipStreamSynchronize(c->stream));
  return peer_check(c);
}
extern "C" int qexhip_eig_project_out(qexhip_handle c, int basis, int nev, int n, const int *ids) {
  if (!c) return QEXHIP_ERR_ARG;
  if (!ids) { qexhip_set_error("eig_project_out: null argument"); return QEXHIP_ERR_ARG; }
  if (n < 1 || n > EIG_MAXRHS) { qexhip_set_error("eig_project_out: n = %d, must be 1..%d", n, EIG_MAXRHS); return QEXHIP_ERR_ARG; }
  DevField *f[EIG_MAXRHS];
  for (int k = 0; k < n; k++) {
    CHK(find_field(c, ids[k], &f[k]));
    for (int q = 0; q < k; q++)
      if (ids[q] == ids[k]) { qexhip_set_error("eig_project_out: fields %d and %d are the same (id %d)", q, k, ids[k]); return QEXHIP_ERR_ARG; }
  }
  EigBasis *B;
  CHK(lowmode_args(c, basis, "eig_project_out", &B));
  HIPCHK(hipSetDevice(c->device));
  CHK(eig_project_out(c, *B, nev, n, f));
  HIPCHK(hipStreamSynchronize(c->stream));
  return peer_check(c);
}

// ---- connected scalar correlator from point sources (conn4d.nim): point sources, translated |phi|^2 accumulation, staggered sign ----
static int check_points(qexhip_ctx *c, const char *who, int n, const int *pts) {
  for (int k = 0; k < n; k++)
    for (int mu = 0; mu < 4; mu++) {
      const int L = c->g.X[mu] * c->rankGeom[mu];
      if (pts[4 * k + mu] < 0 || pts[4 * k + mu] >= L) {
        qexhip_set_error("%s: pts[%d][%d] = %d outside [0, %d)", who, k, mu, pts[4 * k + mu], L);
        return QEXHIP_ERR_ARG;
      }
    }
  return 0;
}
extern "C" int qexhip_dev_point_source(qexhip_handle c, int n, const int *ids, const int *pts, const int *ic) {
  if (!c) return QEXHIP_ERR_ARG;
  if (!ids || !pts || !ic) { qexhip_set_error("dev_point_source: null argument"); return QEXHIP_ERR_ARG; }
  if (n < 1 || n > 4) { qexhip_set_error("dev_point_source: n = %d, must be 1..4", n); return QEXHIP_ERR_ARG; }
  DevField *dst[4];
  for (int k = 0; k < n; k++) {
    for (int j = 0; j < k; j++)
      if (ids[j] == ids[k]) { qexhip_set_error("dev_point_source: destinations %d and %d are the same field %d", j, k, ids[k]); return QEXHIP_ERR_ARG; }
    CHK(find_field(c, ids[k], &dst[k]));
    if (ic[k] < 0 || ic[k] > 2) { qexhip_set_error("dev_point_source: ic[%d] = %d, must be 0..2", k, ic[k]); return QEXHIP_ERR_ARG; }
  }
  CHK(check_points(c, "dev_point_source", n, pts));
  HIPCHK(hipSetDevice(c->device));
  return conn_point_source(c, n, dst, pts, ic);
}
extern "C" int qexhip_dev_conn_accum(qexhip_handle c, int cfield, int n, const int *phi_ids, const int *pts, double scal) {
  if (!c) return QEXHIP_ERR_ARG;
  if (!phi_ids || !pts) { qexhip_set_error("dev_conn_accum: null argument"); return QEXHIP_ERR_ARG; }
  if (n < 1 || n > 4) { qexhip_set_error("dev_conn_accum: n = %d, must be 1..4", n); return QEXHIP_ERR_ARG; }
  DevCField *tr;
  CHK(find_cfield(c, cfield, &tr));
  DevField *phi[4];
  for (int k = 0; k < n; k++) CHK(find_field(c, phi_ids[k], &phi[k]));
  CHK(check_points(c, "dev_conn_accum", n, pts));
  HIPCHK(hipSetDevice(c->device));
  return conn_accum(c, *tr, n, phi, pts, scal);
}
extern "C" int qexhip_cfield_stag_sign(qexhip_handle c, int cfield) {
  if (!c) return QEXHIP_ERR_ARG;
  DevCField *tr;
  CHK(find_cfield(c, cfield, &tr));
  HIPCHK(hipSetDevice(c->device));
  return cfield_stag_sign(c, *tr);
}

// ---- link smearing ----
extern "C" int qexhip_fat7(qexhip_handle c, const double *g, const double coef[5], double *fl, double *ll, double naik) {
  if (!c || !g || !coef || !fl) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  return smear_fat7_host(c, g, coef, fl, ll, naik);
}
extern "C" int qexhip_hisq_smear(qexhip_handle c, const double *g, double *fl, double *ll) {
  if (!c || !g || !fl || !ll) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  return smear_hisq_host(c, g, fl, ll);
}
extern "C" int qexhip_nhyp_smear(qexhip_handle c, const double *g, double *fl, double a1, double a2, double a3) {
  if (!c || !g || !fl) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  return smear_nhyp_host(c, g, fl, a1, a2, a3);
}

extern "C" int qexhip_set_option(qexhip_handle c, const char *name, int value) {
  if (!c || !name) return QEXHIP_ERR_ARG;
  const std::string n(name);
  if (n == "recon") c->opt_recon = value;            // takes effect at the next set_links
  else if (n == "lossless") c->opt_lossless = value;   // takes effect at the next set_links
  else if (n == "overlap") c->opt_overlap = value;
  else if (n == "transport") {
    if (comm_ready(c)) { qexhip_set_error("option transport must be set before qexhip_comm_init"); return QEXHIP_ERR_STATE; }
    if (value < 0 || value > 3) { qexhip_set_error("option transport: 0 auto, 1 rccl, 2 peer, 3 rccl + mailbox sums"); return QEXHIP_ERR_ARG; }
    c->opt_transport = value;
  }
  else if (n == "batch_multi") c->opt_batch_multi = value;
  else if (n == "multi_reduce") c->opt_multi_reduce = value;
  else if (n == "flow_exp") c->opt_flow_exp = value;
  else if (n == "smear_ca") c->opt_smear_ca = value;
  else if (n == "chain_overlap") c->opt_chain_overlap = value;
  else if (n == "hisq_md_fused") {
    if (value < 0 || value > 3) { qexhip_set_error("option hisq_md_fused: bit 0 k_outer13, bit 1 k_projtah_kick"); return QEXHIP_ERR_ARG; }
    c->opt_hisq_md_fused = value;
  }
  else if (n == "hop_split") {
    if (value != -1 && value != 0 && value != 2) { qexhip_set_error("option hop_split: -1 measured, 0 split by sites, 2 fused (the two-launch form 1 left the library in round 6)"); return QEXHIP_ERR_ARG; }
    c->opt_hop_split = value;
  }
  else if (n == "fused_spin_us") c->opt_fused_spin_us = value;
  else if (n == "emu_exchange_us") c->emu_exchange_us = value;
  else if (n == "emu_allreduce_us") c->emu_allreduce_us = value;
  else if (n == "emu_link_gbs") c->emu_link_gbs = value;
  else if (n == "obs_clover") c->opt_obs_clover = value;
  else if (n == "force_pair") c->opt_force_pair = value;
  else if (n == "sloppy_check") {
    if (value < 1) { qexhip_set_error("option sloppy_check: >= 1 fp32 iterations"); return QEXHIP_ERR_ARG; }
    c->opt_sloppy_check = value;
  }
  else if (n == "half") {
    if (value != 0 && value != 1) { qexhip_set_error("option half: 0 (SloppyHalf runs single) or 1 (16-bit storage)"); return QEXHIP_ERR_ARG; }
    c->opt_half = value;
  }
  else if (n == "half_batch") {
    if (value != 0 && value != 1) { qexhip_set_error("option half_batch: 0 (SloppyHalf batches run single) or 1 (16-bit batches)"); return QEXHIP_ERR_ARG; }
    c->opt_half_batch = value;
  }
  else if (n == "batch_ranks") {
    if (value != 0 && value != 1) { qexhip_set_error("option batch_ranks: 0 (batched sloppy solves refuse t-sharded contexts) or 1 (they run there)"); return QEXHIP_ERR_ARG; }
    c->opt_batch_ranks = value;
  }
  else if (n == "half_stall") {
    if (value < 0) { qexhip_set_error("option half_stall: >= 0 failed reliable updates"); return QEXHIP_ERR_ARG; }
    c->opt_half_stall = value;
  }
  else if (n == "gfix_check") {
    if (value < 1) { qexhip_set_error("option gfix_check: >= 1 relax iterations"); return QEXHIP_ERR_ARG; }
    c->opt_gfix_check = value;
  }
  else if (n == "stout_check") {
    if (value < 1) { qexhip_set_error("option stout_check: >= 1 inverse iterations"); return QEXHIP_ERR_ARG; }
    c->opt_stout_check = value;
  }
  else { qexhip_set_error("unknown option"); return QEXHIP_ERR_ARG; }
  return 0;
}
// Host staging of the lock-step batches, after the entry's own checks: the sources up into the batch state's io fields, ONE batch --
// xx_parity >= 0: solveXX on that parity, else the full solve; in fp64, mixed precision (sloppy > 0) or deflated from basis B (either
// precision) -- and the solutions down.  The sloppy and the deflated entries start a new report for qexhip_stag_sloppy_last_batch.
static int solve_batch_host(qexhip_ctx *c, int n, double *const *x, const double *const *b, const double *mass, const double *r2req,
                            int maxits, int xx_parity, int sloppy, EigBasis *B, int nev, int *iters, double *r2, int *nupdates) {
  HIPCHK(hipSetDevice(c->device));
  if (sloppy && !B) CHK(batch_sloppy_check(c, n, mass));     // (deflate_batch_args has made it for a deflated batch)
  DevField *xs[QX_MAXRHS], *bs[QX_MAXRHS];
  CHK(batch_io_fields(c, n, xs, bs));
  for (int j = 0; j < n; j++) CHK(field_upload(c, *bs[j], b[j]));
  if (sloppy || B) slpb_last_reset(c, n);
  if (B && xx_parity >= 0) CHK(solve_xx_batch_deflated_dev(c, *B, nev, n, xs, bs, mass, r2req, maxits, xx_parity, sloppy, iters, r2, nupdates));
  else if (B) CHK(solve_full_batch_deflated_dev(c, *B, nev, n, xs, bs, mass, r2req, maxits, sloppy, iters, r2, nupdates));
  else if (xx_parity < 0) CHK(solve_full_batch_sloppy_dev(c, n, xs, bs, mass, r2req, maxits, sloppy, iters, r2, nupdates));
  else if (sloppy) CHK(solve_xx_batch_sloppy_any(c, sloppy, n, xs, bs, mass, r2req, maxits, xx_parity, iters, r2, nupdates));
  else CHK(solve_xx_batch_dev(c, n, xs, bs, mass, r2req, maxits, xx_parity, iters, r2));
  for (int j = 0; j < n; j++) CHK(field_download(c, *xs[j], x[j]));
  return 0;
}
extern "C" int qexhip_stag_solve_xx_batch(qexhip_handle c, int n, double *const *x, const double *const *b, const double *mass,
                                          const double *r2req, int maxits, int par_even, int *iters, double *r2_over_b2) {
  if (!c || !x || !b || !mass || !r2req) return QEXHIP_ERR_ARG;
  return solve_batch_host(c, n, x, b, mass, r2req, maxits, par_even ? 1 : 0, 0, nullptr, 0, iters, r2_over_b2, nullptr);
}
extern "C" int qexhip_stag_solve_batch(qexhip_handle c, int n, double *const *x, const double *const *b, const double *mass,
                                       const double *r2req, int maxits, int *iters, double *r2_over_b2) {
  if (!c || !x || !b || !mass || !r2req) return QEXHIP_ERR_ARG;
  return solve_batch_host(c, n, x, b, mass, r2req, maxits, -1, 0, nullptr, 0, iters, r2_over_b2, nullptr);
}
// Mixed-precision lock-step batches.  sloppy = 0 IS the fp64 entry; the batched mixed-precision forms run on one rank, and on t-sharded
// contexts with option "batch_ranks" (batch_sloppy_check).
extern "C" int qexhip_stag_solve_xx_batch_sloppy(qexhip_handle c, int n, double *const *x, const double *const *b, const double *mass,
                                                 const double *r2req, int maxits, int par_even, int sloppy, int *iters,
                                                 double *r2_over_b2, int *nupdates) {
  if (!c || !x || !b || !mass || !r2req) return QEXHIP_ERR_ARG;
  CHK(sloppy_check(c, sloppy));
  if (n < 1 || n > 4) { qexhip_set_error("batch solve: 1 <= n <= 4"); return QEXHIP_ERR_ARG; }
  if (nupdates) for (int j = 0; j < n; j++) nupdates[j] = 0;
  return solve_batch_host(c, n, x, b, mass, r2req, maxits, par_even ? 1 : 0, sloppy, nullptr, 0, iters, r2_over_b2, nupdates);
}
extern "C" int qexhip_stag_solve_batch_sloppy(qexhip_handle c, int n, double *const *x, const double *const *b, const double *mass,
                                              const double *r2req, int maxits, int sloppy, int *iters, double *r2_final, int *nupdates) {
  if (!c || !x || !b || !mass || !r2req) return QEXHIP_ERR_ARG;
  CHK(sloppy_check(c, sloppy));
  if (n < 1 || n > 4) { qexhip_set_error("batch solve: 1 <= n <= 4"); return QEXHIP_ERR_ARG; }
  if (nupdates) for (int j = 0; j < n; j++) nupdates[j] = 0;
  return solve_batch_host(c, n, x, b, mass, r2req, maxits, -1, sloppy, nullptr, 0, iters, r2_final, nupdates);
}
extern "C" int qexhip_stag_links_info(qexhip_handle c, int *nlinks, int *compressed, double *max_dev) {
  if (!c) return QEXHIP_ERR_ARG;
  if (nlinks) *nlinks = c->W ? c->ndir : 0;
  if (compressed) *compressed = c->recon;
  if (max_dev) *max_dev = c->recon_dev;
  return 0;
}
extern "C" int qexhip_stag_links_storage(qexhip_handle c, int *bytes_per_link, long long *escaped) {
  if (!c) return QEXHIP_ERR_ARG;
  if (bytes_per_link) *bytes_per_link = c->W ? stag_link_storage(c).bytes : 0;
  if (escaped) *escaped = c->lres_esc;
  return 0;
}
extern "C" int qexhip_link_residual_host(const double *links, int n, unsigned char *escaped, double *row2) {
  if (!links || n < 0) return QEXHIP_ERR_ARG;
  return link_lossless_host(1, (const double2 *)links, n, escaped, (double2 *)row2);
}
extern "C" int qexhip_link_packed_host(const double *links, int n, unsigned char *escaped, double *decoded) {
  if (!links || n < 0) return QEXHIP_ERR_ARG;
  return link_lossless_host(2, (const double2 *)links, n, escaped, (double2 *)decoded);
}
extern "C" int qexhip_link_ortho_host(const double *links, int n, unsigned char *escaped, double *decoded) {
  if (!links || n < 0) return QEXHIP_ERR_ARG;
  return link_lossless_host(3, (const double2 *)links, n, escaped, (double2 *)decoded);
}
extern "C" int qexhip_hisq_prepare(qexhip_handle c, const double *g, double *fl, double *ll) {
  if (!c || !g) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  return hisq_prepare(c, g, fl, ll);
}
extern "C" int qexhip_hisq_closure_force(qexhip_handle c, const double *dsdsu, const double *dsdsul, double *f) {
  if (!c || !dsdsu || !dsdsul || !f) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  return hisq_closure_force(c, dsdsu, dsdsul, f);
}
extern "C" int qexhip_hisq_fermion_force(qexhip_handle c, double *f, const double *const *psi, const double *scale, int n) {
  if (!c || !f || !psi || !scale) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  return hisq_fermion_force(c, f, psi, scale, n);
}
extern "C" int qexhip_hisq_release(qexhip_handle c) {
  if (!c) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  hisq_state_free(c);
  return 0;
}
extern "C" int qexhip_hisq_force(qexhip_handle c, const double *g, const double *dsdsu, const double *dsdsul, double *f) {
  if (!c || !g || !dsdsu || !dsdsul || !f) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  return smear_hisq_force_host(c, g, dsdsu, dsdsul, f);
}
extern "C" int qexhip_fat7_deriv(qexhip_handle c, const double *g, const double *dfl, const double coef[5], const double *dll,
                                 double naik, double *d) {
  if (!c || !g || !dfl || !coef || !d) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  return smear_fat7_deriv_host(c, g, dfl, coef, dll, naik, d);
}
extern "C" int qexhip_stag_set_links_hisq(qexhip_handle c, const double *g) {
  if (!c) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  return smear_set_links_hisq(c, g);
}
extern "C" int qexhip_stag_set_links_nhyp(qexhip_handle c, const double *g, double a1, double a2, double a3,
                                          const int antiperiodic[4], const int phases[4]) {
  if (!c) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  static const int defph[4] = {8, 9, 11, 0};
  int mask = 0;
  for (int mu = 0; mu < 4; mu++) if (antiperiodic ? antiperiodic[mu] : (mu == 3)) mask |= 1 << mu;
  return smear_set_links_nhyp(c, g, a1, a2, a3, mask, phases ? phases : defph);
}

extern "C" int qexhip_nhyp_prepare(qexhip_handle c, const double *g, double a1, double a2, double a3, double *fl) {
  if (!c) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  return nhyp_prepare(c, g, a1, a2, a3, fl);
}
extern "C" int qexhip_nhyp_force(qexhip_handle c, double *f, const double *chain) {
  if (!c || !f || !chain) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  return nhyp_force_host(c, f, chain);
}
extern "C" int qexhip_nhyp_gauge_force(qexhip_handle c, double *f, double cplaq, double crect, double cadj) {
  if (!c) return QEXHIP_ERR_ARG;
  if (crect != 0.0 && cadj != 0.0) { qexhip_set_error("rect and adjplaq together are not a QEX action"); return QEXHIP_ERR_ARG; }
  HIPCHK(hipSetDevice(c->device));
  return nhyp_gauge_force(c, f, cplaq, cadj != 0.0 ? cadj : crect, cadj != 0.0 ? 1 : 0);
}
// ---- stout smearing (stout.hip) ----
extern "C" int qexhip_stout_smear(qexhip_handle c, const double *g, double alpha, double *fl) {
  if (!c) return QEXHIP_ERR_ARG;
  return stout_smear(c, g, alpha, fl);
}
extern "C" int qexhip_stout_prepare(qexhip_handle c, const double *g, const double *alphas, int nlevels, double *fl) {
  if (!c) return QEXHIP_ERR_ARG;
  return stout_prepare(c, g, alphas, nlevels, fl);
}
extern "C" int qexhip_stout_force(qexhip_handle c, double *f, const double *chain) {
  if (!c) return QEXHIP_ERR_ARG;
  if (!chain) { qexhip_set_error("stout_force: null chain"); return QEXHIP_ERR_ARG; }
  return stout_force(c, f, chain);
}
extern "C" int qexhip_stout_gauge_force(qexhip_handle c, double *f, double cplaq, double crect, double cadj) {
  if (!c) return QEXHIP_ERR_ARG;
  if (crect != 0.0 && cadj != 0.0) { qexhip_set_error("rect and adjplaq together are not a QEX action"); return QEXHIP_ERR_ARG; }
  if (crect != 0.0) for (int d = 0; d < 4; d++) if (c->g.X[d] < 4) { qexhip_set_error("rectangle action needs extents >= 4"); return QEXHIP_ERR_ARG; }
  return stout_gauge_force(c, f, cplaq, cadj != 0.0 ? cadj : crect, cadj != 0.0 ? 1 : 0);
}
extern "C" int qexhip_stout_release(qexhip_handle c) {
  if (!c) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  stout_chain_free(c);
  return 0;
}
extern "C" int qexhip_stout_inverse(qexhip_handle c, const double *fl, double alpha, double rdf2req, int maxits, double *g, int *iters,
                                    double *rdf2, int *diverging) {
  if (!c) return QEXHIP_ERR_ARG;
  if (!fl || !g) { qexhip_set_error("stout_inverse: null field"); return QEXHIP_ERR_ARG; }
  if (g == fl) { qexhip_set_error("stout_inverse: g and fl must be distinct (stoutsmear.nim:37)"); return QEXHIP_ERR_ARG; }
  if (maxits < 0) { qexhip_set_error("stout_inverse: maxits < 0"); return QEXHIP_ERR_ARG; }
  return stout_inverse(c, fl, alpha, rdf2req, maxits, g, iters, rdf2, diverging);
}
extern "C" int qexhip_nhyp_fermion_force(qexhip_handle c, double *f, const double *const *psi, const double *scale, int n,
                                         const int antiperiodic[4], const int phases[4]) {
  if (!c || !psi || !scale) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  static const int defph[4] = {8, 9, 11, 0};
  int mask = 0;
  for (int mu = 0; mu < 4; mu++) if (antiperiodic ? antiperiodic[mu] : (mu == 3)) mask |= 1 << mu;
  return nhyp_fermion_force(c, f, psi, scale, n, mask, phases ? phases : defph);
}
extern "C" int qexhip_nhyp_fforce(qexhip_handle c, double *f, int n, const double *const *phi, const double *mass,
                                  const double *scale, const double *r2req, int maxits, const int antiperiodic[4],
                                  const int phases[4], int *iters) {
  if (!c || !phi || !mass || !scale || !r2req) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  static const int defph[4] = {8, 9, 11, 0};
  int mask = 0;
  for (int mu = 0; mu < 4; mu++) if (antiperiodic ? antiperiodic[mu] : (mu == 3)) mask |= 1 << mu;
  return nhyp_fforce(c, f, n, phi, mass, scale, r2req, maxits, mask, phases ? phases : defph, iters);
}
extern "C" int qexhip_nhyp_fforce_dev(qexhip_handle c, double *f, int n, const int *phi_ids, const double *mass,
                                      const double *scale, const double *r2req, int maxits, const int antiperiodic[4],
                                      const int phases[4], int *iters) {
  if (!c || !phi_ids || !mass || !scale || !r2req || n < 1 || n > 64) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  static const int defph[4] = {8, 9, 11, 0};
  int mask = 0;
  for (int mu = 0; mu < 4; mu++) if (antiperiodic ? antiperiodic[mu] : (mu == 3)) mask |= 1 << mu;
  std::vector<DevField *> pf(n);
  for (int k = 0; k < n; k++) CHK(find_field(c, phi_ids[k], &pf[k]));
  return nhyp_fforce(c, f, n, nullptr, mass, scale, r2req, maxits, mask, phases ? phases : defph, iters, pf.data());
}
// ---- the two ends of a trajectory on resident fields (round 3) ----
struct qexhip_rng;
extern "C" int qexhip_rng_dev_gaussian_vector(qexhip_handle c, qexhip_rng *rng, int field_id) {
  if (!c || !rng) return QEXHIP_ERR_ARG;
  DevField *f;
  CHK(find_field(c, field_id, &f));
  return rng_dev_generate(c, rng, 0, f, nullptr);
}
extern "C" int qexhip_rng_dev_u1_vector(qexhip_handle c, qexhip_rng *rng, int field_id) {
  if (!c || !rng) return QEXHIP_ERR_ARG;
  DevField *f;
  CHK(find_field(c, field_id, &f));
  return rng_dev_generate(c, rng, 1, f, nullptr);
}
extern "C" int qexhip_rng_dev_z4_vector(qexhip_handle c, qexhip_rng *rng, int field_id) {
  if (!c || !rng) return QEXHIP_ERR_ARG;
  DevField *f;
  CHK(find_field(c, field_id, &f));
  return rng_dev_generate(c, rng, 3, f, nullptr);
}
extern "C" int qexhip_rng_dev_z2_vector(qexhip_handle c, qexhip_rng *rng, int field_id) {
  if (!c || !rng) return QEXHIP_ERR_ARG;
  DevField *f;
  CHK(find_field(c, field_id, &f));
  return rng_dev_generate(c, rng, 4, f, nullptr);
}
extern "C" int qexhip_md_refresh_momenta(qexhip_handle c, qexhip_rng *rng) {
  if (!c || !rng) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  double2 *M = nullptr;
  CHK(md_momenta_dev(c, &M));
  return rng_dev_generate(c, rng, 2, nullptr, M);
}
extern "C" int qexhip_dev_zero(qexhip_handle c, int id, int parity) {
  if (!c || parity < 0 || parity > 2) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  DevField *f;
  CHK(find_field(c, id, &f));
  return blas_zero(c, *f, parity);
}
extern "C" int qexhip_dev_solve_batch(qexhip_handle c, int n, const int *x_ids, const int *b_ids, const double *mass,
                                      const double *r2req, int maxits, int *iters, double *r2) {
  if (!c || !x_ids || !b_ids || !mass || !r2req || n < 1 || n > 64) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  DevField *xs[64], *bs[64];
  CHK(find_batch_fields(c, n, x_ids, b_ids, xs, bs));
  for (int k0 = 0; k0 < n; k0 += 4)            // lock-step batches of four, as qexhip_stag_solve_batch
    CHK(solve_full_batch_dev(c, std::min(4, n - k0), xs + k0, bs + k0, mass + k0, r2req + k0, maxits, iters ? iters + k0 : nullptr,
                             r2 ? r2 + k0 : nullptr));
  return 0;
}
// qexhip_stag_solve_batch_sloppy on resident fields: ONE lock-step batch (n <= 4)
extern "C" int qexhip_dev_solve_batch_sloppy(qexhip_handle c, int n, const int *x_ids, const int *b_ids, const double *mass,
                                             const double *r2req, int maxits, int sloppy, int *iters, double *r2, int *nupdates) {
  if (!c || !x_ids || !b_ids || !mass || !r2req) return QEXHIP_ERR_ARG;
  CHK(sloppy_check(c, sloppy));
  if (n < 1 || n > 4) { qexhip_set_error("batch solve: 1 <= n <= 4"); return QEXHIP_ERR_ARG; }
  if (nupdates) for (int j = 0; j < n; j++) nupdates[j] = 0;
  if (!sloppy) return qexhip_dev_solve_batch(c, n, x_ids, b_ids, mass, r2req, maxits, iters, r2);
  HIPCHK(hipSetDevice(c->device));
  CHK(batch_sloppy_check(c, n, mass));
  DevField *xs[4], *bs[4];
  CHK(find_batch_fields(c, n, x_ids, b_ids, xs, bs));
  slpb_last_reset(c, n);
  return solve_full_batch_sloppy_dev(c, n, xs, bs, mass, r2req, maxits, sloppy, iters, r2, nupdates);
}
// ---- the deflated lock-step batch (solver.cpp: solve_xx_batch_deflated_dev; batch.hip: the full solves) ----
// every check before anything is launched: deflate_args per mass, the batch size, the sloppy batch's one-rank condition
static int deflate_batch_args(qexhip_ctx *c, int basis, int nev, int n, const double *mass, int sloppy, EigBasis **B) {
  if (n < 1 || n > 4) { qexhip_set_error("batch solve: 1 <= n <= 4"); return QEXHIP_ERR_ARG; }
  for (int k = 0; k < n; k++) CHK(deflate_args(c, basis, nev, sloppy, mass[k], B));
  for (int k = 0; k < n; k++) if (mass[k] == 0.0) { qexhip_set_error("batch solve: mass must be non-zero"); return QEXHIP_ERR_ARG; }
  if (sloppy) CHK(batch_sloppy_check(c, n, mass));
  if ((*B)->gen != c->links_gen) { qexhip_set_error("deflated solve: the basis was computed on other links"); return QEXHIP_ERR_STATE; }
  return 0;
}
extern "C" int qexhip_dev_solve_xx_batch_deflated(qexhip_handle c, int basis, int nev, int n, const int *x_ids, const int *b_ids,
                                                  const double *mass, const double *r2req, int maxits, int par_even, int sloppy,
                                                  int *iters, double *r2_over_b2, int *nupdates) {
  if (!c || !x_ids || !b_ids || !mass || !r2req) return QEXHIP_ERR_ARG;
  EigBasis *B;
  CHK(deflate_batch_args(c, basis, nev, n, mass, sloppy, &B));
  DevField *xs[4], *bs[4];
  CHK(find_batch_fields(c, n, x_ids, b_ids, xs, bs));
  HIPCHK(hipSetDevice(c->device));
  slpb_last_reset(c, n);
  return solve_xx_batch_deflated_dev(c, *B, nev, n, xs, bs, mass, r2req, maxits, par_even ? 1 : 0, sloppy, iters, r2_over_b2, nupdates);
}
extern "C" int qexhip_dev_solve_batch_deflated(qexhip_handle c, int basis, int nev, int n, const int *x_ids, const int *b_ids,
                                               const double *mass, const double *r2req, int maxits, int sloppy, int *iters,
                                               double *r2_final, int *nupdates) {
  if (!c || !x_ids || !b_ids || !mass || !r2req) return QEXHIP_ERR_ARG;
  EigBasis *B;
  CHK(deflate_batch_args(c, basis, nev, n, mass, sloppy, &B));
  DevField *xs[4], *bs[4];
  CHK(find_batch_fields(c, n, x_ids, b_ids, xs, bs));
  HIPCHK(hipSetDevice(c->device));
  slpb_last_reset(c, n);
  return solve_full_batch_deflated_dev(c, *B, nev, n, xs, bs, mass, r2req, maxits, sloppy, iters, r2_final, nupdates);
}
// the host-field forms: every check of the resident ones, and no null field, before the first upload
static int solve_batch_deflated_host(qexhip_ctx *c, int basis, int nev, int n, double *const *x, const double *const *b, const double *mass,
                                     const double *r2req, int maxits, int xx_parity, int sloppy, int *iters, double *r2, int *nupdates) {
  if (!c || !x || !b || !mass || !r2req) return QEXHIP_ERR_ARG;
  EigBasis *B;
  CHK(deflate_batch_args(c, basis, nev, n, mass, sloppy, &B));
  for (int j = 0; j < n; j++) if (!x[j] || !b[j]) return QEXHIP_ERR_ARG;
  return solve_batch_host(c, n, x, b, mass, r2req, maxits, xx_parity, sloppy, B, nev, iters, r2, nupdates);
}
extern "C" int qexhip_stag_solve_xx_batch_deflated(qexhip_handle c, int basis, int nev, int n, double *const *x, const double *const *b,
                                                   const double *mass, const double *r2req, int maxits, int par_even, int sloppy,
                                                   int *iters, double *r2_over_b2, int *nupdates) {
  return solve_batch_deflated_host(c, basis, nev, n, x, b, mass, r2req, maxits, par_even ? 1 : 0, sloppy, iters, r2_over_b2, nupdates);
}
extern "C" int qexhip_stag_solve_batch_deflated(qexhip_handle c, int basis, int nev, int n, double *const *x, const double *const *b,
                                                const double *mass, const double *r2req, int maxits, int sloppy, int *iters,
                                                double *r2_final, int *nupdates) {
  return solve_batch_deflated_host(c, basis, nev, n, x, b, mass, r2req, maxits, -1, sloppy, iters, r2_final, nupdates);
}
extern "C" int qexhip_nhyp_release(qexhip_handle c) {
  if (!c) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  nhyp_state_free(c);
  return 0;
}

// ---- gauge / flow ----
extern "C" int qexhip_gauge_set(qexhip_handle c, const double *g) { if (!c || !g) return QEXHIP_ERR_ARG; return gauge_set(c, g); }
extern "C" int qexhip_gauge_get(qexhip_handle c, double *g) { if (!c || !g) return QEXHIP_ERR_ARG; return gauge_get(c, g); }
extern "C" int qexhip_plaq(qexhip_handle c, double out[6]) { if (!c || !out) return QEXHIP_ERR_ARG; return gauge_plaq(c, out); }
extern "C" int qexhip_gauge_force(qexhip_handle c, double *f, double cplaq) { if (!c || !f) return QEXHIP_ERR_ARG; return gauge_force(c, f, cplaq); }
extern "C" int qexhip_gauge_force_general(qexhip_handle c, double *f, double cplaq, double c2, int kind) {
  if (!c || !f || kind < 0 || kind > 1) return QEXHIP_ERR_ARG;
  return gauge_force(c, f, cplaq, c2, kind);
}
extern "C" int qexhip_wflow_general(qexhip_handle c, int nsteps, double eps, double cplaq, double c2, int kind) {
  if (!c || nsteps < 0 || kind < 0 || kind > 1) return QEXHIP_ERR_ARG;
  return gauge_wflow(c, nsteps, eps, cplaq, c2, kind);
}
extern "C" int qexhip_flow_EQ(qexhip_handle c, int loop, double out[3]) { if (!c || !out) return QEXHIP_ERR_ARG; return gauge_flow_obs(c, loop, out); }
extern "C" int qexhip_flow_measure(qexhip_handle c, double plaq[6], double EQ[3]) {
  if (!c || !plaq || !EQ) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  // the dedicated kernel when it is available (one pass over the links for all nine numbers), two passes otherwise
  const int rc = gauge_flow_obs(c, 1, EQ, plaq);
  if (rc != -3) return rc;
  CHK(gauge_plaq(c, plaq));
  return gauge_flow_obs(c, 1, EQ);
}
extern "C" int qexhip_gauge_action(qexhip_handle c, double cplaq, double crect, double cadj, double *out) {
  if (!c || !out) return QEXHIP_ERR_ARG;
  if (crect != 0.0 && cadj != 0.0) { qexhip_set_error("rect and adjplaq together are not a QEX action"); return QEXHIP_ERR_ARG; }
  HIPCHK(hipSetDevice(c->device));
  return gauge_action(c, cplaq, cadj != 0.0 ? cadj : crect, cadj != 0.0 ? 1 : 0, out);
}
extern "C" int qexhip_gauge_update(qexhip_handle c, const double *p, double t) {
  if (!c || !p) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  return gauge_md_update(c, p, t);
}
extern "C" int qexhip_gauge_reunit(qexhip_handle c) {
  if (!c) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  return gauge_reunit(c);
}
extern "C" int qexhip_wline(qexhip_handle c, const int *path, int n, double out[2]) {
  if (!c || !path || !out) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  return gauge_wline(c, path, n, out);
}
extern "C" int qexhip_plaq_s4(qexhip_handle c, double out[8]) {
  if (!c || !out) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  return gauge_plaq_s4(c, out);
}
extern "C" int qexhip_polyakov_loops(qexhip_handle c, double out[8]) {
  if (!c || !out) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  return gauge_polyakov(c, out);
}
// gauge fixing (gaugefix.hip): gaugefix.nim:376 `t := 1`, :312-355 getGaugeFixTransform, :8-20 gaugeTransform, :135-142 linkTrace
extern "C" int qexhip_gfix_set_transform(qexhip_handle c, const double *t) { if (!c) return QEXHIP_ERR_ARG; return gfix_set_transform(c, t); }
extern "C" int qexhip_gfix_get_transform(qexhip_handle c, double *t) {
  if (!c) return QEXHIP_ERR_ARG;
  if (!t) { qexhip_set_error("gfix_get_transform: null argument"); return QEXHIP_ERR_ARG; }
  return gfix_get_transform(c, t);
}
extern "C" int qexhip_gauge_fix(qexhip_handle c, const int *dirs, int ndirs, double gstop, double orf, int maxits, int *iters,
                                double metrics[4], double *hist, int histcap) {
  if (!c) return QEXHIP_ERR_ARG;
  return gauge_fix(c, dirs, ndirs, gstop, orf, maxits, iters, metrics, hist, histcap);
}
extern "C" int qexhip_gauge_transform(qexhip_handle c) { if (!c) return QEXHIP_ERR_ARG; return gauge_transform(c); }
extern "C" int qexhip_gauge_link_trace(qexhip_handle c, const int *dirs, int ndirs, double *out) {
  if (!c) return QEXHIP_ERR_ARG;
  if (!out) { qexhip_set_error("gauge_link_trace: null argument"); return QEXHIP_ERR_ARG; }
  return gauge_link_trace(c, dirs, ndirs, out);
}
extern "C" int qexhip_wflow(qexhip_handle c, int nsteps, double eps) { if (!c || nsteps < 0) return QEXHIP_ERR_ARG; return gauge_wflow(c, nsteps, eps); }

// ---- resident molecular dynamics (gauge.hip) ----
extern "C" int qexhip_md_begin(qexhip_handle c, const double *g, const double *p) {
  if (!c) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  return md_begin(c, g, p);
}
extern "C" int qexhip_md_end(qexhip_handle c, double *g, double *p) { if (!c) return QEXHIP_ERR_ARG; HIPCHK(hipSetDevice(c->device)); return md_end(c, g, p); }
extern "C" int qexhip_md_momentum_norm2(qexhip_handle c, double *p2) { if (!c || !p2) return QEXHIP_ERR_ARG; HIPCHK(hipSetDevice(c->device)); return md_momentum_norm2(c, p2); }
extern "C" int qexhip_md_update_links(qexhip_handle c, double t) { if (!c) return QEXHIP_ERR_ARG; HIPCHK(hipSetDevice(c->device)); return md_update_links(c, t); }
extern "C" int qexhip_md_gauge_force(qexhip_handle c, double cplaq, double crect, double cadj) {
  if (!c) return QEXHIP_ERR_ARG;
  if (crect != 0.0 && cadj != 0.0) { qexhip_set_error("rect and adjplaq together are not a QEX action"); return QEXHIP_ERR_ARG; }
  HIPCHK(hipSetDevice(c->device));
  return md_gauge_force(c, cplaq, cadj != 0.0 ? cadj : crect, cadj != 0.0 ? 1 : 0);
}
extern "C" int qexhip_md_kick(qexhip_handle c, int source, double t) { if (!c) return QEXHIP_ERR_ARG; HIPCHK(hipSetDevice(c->device)); return md_kick(c, source, t); }
extern "C" int qexhip_md_shift_links(qexhip_handle c, int source, double t) { if (!c) return QEXHIP_ERR_ARG; HIPCHK(hipSetDevice(c->device)); return md_shift_links(c, source, t); }
// ---- resident HISQ molecular dynamics (smear.hip: md_hisq_*; hisq_md.hip: k_outer13, k_projtah_kick) ----
extern "C" int qexhip_md_hisq_prepare(qexhip_handle c, const int antiperiodic[4], const int phases[4], int set_links) {
  if (!c) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  static const int defph[4] = {8, 9, 11, 0};
  int mask = 0;
  for (int mu = 0; mu < 4; mu++) if (antiperiodic ? antiperiodic[mu] : (mu == 3)) mask |= 1 << mu;
  return md_hisq_prepare(c, mask, phases ? phases : defph, set_links);
}
// every argument and state check of the two force entries, before anything is launched
static int md_hisq_fields(qexhip_ctx *c, const char *who, int n, const int *ids, const double *scale, std::vector<DevField *> &f) {
  if (!ids || !scale) { qexhip_set_error("%s: null argument", who); return QEXHIP_ERR_ARG; }
  if (n < 1) { qexhip_set_error("%s: n < 1", who); return QEXHIP_ERR_ARG; }
  f.resize(n);
  for (int k = 0; k < n; k++) {
    CHK(find_field(c, ids[k], &f[k]));
    for (int j = 0; j < k; j++)
      if (ids[j] == ids[k]) { qexhip_set_error("%s: ids[%d] == ids[%d]", who, j, k); return QEXHIP_ERR_ARG; }
  }
  return md_hisq_check(c, who);
}
extern "C" int qexhip_md_hisq_fforce(qexhip_handle c, int n, const int *psi_ids, const double *scale, double t) {
  if (!c) return QEXHIP_ERR_ARG;
  std::vector<DevField *> f;
  CHK(md_hisq_fields(c, "md_hisq_fforce", n, psi_ids, scale, f));
  HIPCHK(hipSetDevice(c->device));
  return md_hisq_fforce(c, n, f.data(), scale, t);
}
extern "C" int qexhip_md_hisq_fforce_solve(qexhip_handle c, int n, const int *phi_ids, const double *mass, const double *scale,
                                           const double *r2req, int maxits, double t, int *iters) {
  if (!c) return QEXHIP_ERR_ARG;
  if (!mass || !r2req) { qexhip_set_error("md_hisq_fforce_solve: null argument"); return QEXHIP_ERR_ARG; }
  std::vector<DevField *> f;
  CHK(md_hisq_fields(c, "md_hisq_fforce_solve", n, phi_ids, scale, f));
  if (!c->W) { qexhip_set_error("md_hisq_fforce_solve: the operator has no links (qexhip_md_hisq_prepare with set_links)"); return QEXHIP_ERR_STATE; }
  HIPCHK(hipSetDevice(c->device));
  return md_hisq_fforce_solve(c, n, f.data(), mass, scale, r2req, maxits, t, iters);
}
extern "C" int qexhip_md_hisq_fforce_rational(qexhip_handle c, int phi_id, double mass, int nterm, const double *alpha, const double *beta,
                                              double r2req, int maxits, int sloppy, double t, int *iters) {
  if (!c) return QEXHIP_ERR_ARG;
  double shifts[CGM_MAXM];
  int order[CGM_MAXM];
  CHK(rational_map("md_hisq_fforce_rational", mass, nterm, alpha, beta, shifts, order));
  CHK(sloppy_check(c, sloppy));
  DevField *phi;
  CHK(find_field(c, phi_id, &phi));
  CHK(md_hisq_check(c, "md_hisq_fforce_rational"));
  if (!c->W) { qexhip_set_error("md_hisq_fforce_rational: the operator has no links (qexhip_md_hisq_prepare with set_links)"); return QEXHIP_ERR_STATE; }
  HIPCHK(hipSetDevice(c->device));
  return md_hisq_fforce_rational(c, *phi, mass, nterm, alpha, beta, r2req, maxits, sloppy, t, iters);
}
extern "C" int qexhip_md_hisq_force_get(qexhip_handle c, double *f) {
  if (!c || !f) return QEXHIP_ERR_ARG;
  HIPCHK(hipSetDevice(c->device));
  return md_hisq_force_get(c, f);
}
extern "C" int qexhip_md_save_links(qexhip_handle c) { if (!c) return QEXHIP_ERR_ARG; HIPCHK(hipSetDevice(c->device)); return md_save_links(c); }
extern "C" int qexhip_md_restore_links(qexhip_handle c) { if (!c) return QEXHIP_ERR_ARG; HIPCHK(hipSetDevice(c->device)); return md_restore_links(c); }
