// qexhip_internal.h -- shared declarations of libqexhip.so (gfx950 only).
//
// Device data layout (DESIGN.md "Data layout in HBM"):
//   * sites of one parity are numbered by the checkerboard index c = lex/2 of the rank-local
//     lattice (x fastest, t slowest), so a t-slice is the contiguous range [t*F,(t+1)*F);
//   * sites are grouped in TILES of 64 = one wavefront.  A colour vector of one parity is
//       double2 v[tile][3][64]           (re,im packed: one 16-byte load per lane and colour)
//     and the Dslash-ready gauge field of one parity is
//       double2 W[tile][ndir][9][64]     ndir = 8 (fat) or 16 (fat + Naik)
//     with dir d = 2*mu (+8 for the 3-hop links): forward link U_mu(s); d = 2*mu+1: the
//     backward link already shifted and adjointed, U_mu(s-mu)^+.  A wavefront therefore streams
//     one contiguous 72 KiB (144 KiB) block of links per sweep;
//   * with the t dimension sharded, `depth` ghost t-slices follow the body tiles:
//       [ body: Vh sites | ghost_hi: depth*F (upper neighbour's t=0..depth-1) |
//         ghost_lo: depth*F (lower neighbour's t=Xt-depth..Xt-1) ]
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>
#include <map>

#define QEXHIP_TILE 64

struct Geom {
  int X[4];
  int Xh;      // X[0]/2
  int V, Vh;
  int F;       // sites of one parity per t-slice
  int ntile;   // body tiles per parity
  int depth;   // ghost depth in t (0: no ghost zones)
  int gtile;   // ghost tiles per side per parity
  int etile;   // tiles per parity incl. ghosts
  int halo;    // 1: t-hops across the local boundary read the ghost zones
};

// position (site number within one parity, possibly in a ghost zone) -> double2 offset
__host__ __device__ inline size_t vec_off(int pos, int colour) {
  return (size_t)(pos >> 6) * 192 + (size_t)colour * 64 + (size_t)(pos & 63);
}

// body link-tiles of both parity halves of a natural-layout gauge field: linear index -> offset (skips the ghost tiles of a sharded field)
__host__ __device__ inline size_t body_tile_off(size_t tile, size_t ntile4, size_t etile4) {
  const size_t p = tile >= ntile4;
  return (p * etile4 + (tile - p * ntile4)) * 576;
}
// The t-faces of the two parity halves of a tiled field (tstride double2 per tile: 576 one matrix per site, 4*576 gauge-shaped) for
// comm_faces_exchange at ghost depth `depth` (1..3): my bottom and top `depth` slices, the start of ghost_hi, and the last `depth`
// of ghost_lo's three slices.  Fills [0] and [1] of each array; returns the doubles per face.
inline size_t ghost_faces(const Geom &g, const double2 *field, int tstride, int depth, double **bottom, double **top, double **ghi, double **glo) {
  const size_t tile2 = (size_t)tstride * 2, ft = (size_t)g.F / 64;   // doubles per tile, tiles per t-slice
  for (int p = 0; p < 2; p++) {
    double *base = (double *)field + (size_t)p * g.etile * tile2;
    bottom[p] = base;
    top[p] = base + ((size_t)g.ntile - depth * ft) * tile2;
    ghi[p] = base + (size_t)g.ntile * tile2;
    glo[p] = base + ((size_t)g.ntile + 3 * ft + (3 - depth) * ft) * tile2;
  }
  return (size_t)depth * ft * tile2;
}

struct DevField {  // full-volume colour vector: parity halves, each with its ghost tiles
  double2 *d = nullptr;
  size_t half = 0;  // double2 elements per parity half (= etile*192)
  double2 *par(int p) const { return d + (size_t)p * half; }
};

struct DevFieldF {  // fp32 colour vector of the mixed-precision CG: float2 v[tile][3][64] per parity (vec_off), ghost tiles as DevField's
  float2 *d = nullptr;
  size_t half = 0;  // float2 elements per parity half (= etile*192: ntile*192 without a halo)
  float2 *par(int p) const { return d + (size_t)p * half; }
};

// 16-bit colour vector of the SloppyHalf CG (dslash_half.hip): one 16-byte element per site, u4v v[tile][64] per parity, the site at
// position pos is element pos.  With g.halo the ghost zones continue the positions as nbr_pos<true> numbers them: ghost_hi at
// [Vh, Vh + depth F), ghost_lo behind it (room for depth 3 each, as DevField); a t-face is a contiguous element range.
typedef unsigned int u4v __attribute__((ext_vector_type(4)));
struct DevFieldH {
  u4v *d = nullptr;
  size_t half = 0;   // elements per parity (= etile*64: ntile*64 without a halo)
  u4v *par(int p) const { return d + (size_t)p * half; }
};

struct DevCField {  // complex site field (trace.hip): double2 d[parity][ntile*64], site c of a parity at index c; no ghost slices
  double2 *d = nullptr;
  size_t half = 0;  // double2 elements per parity half (= ntile*64)
  double2 *par(int p) const { return d + (size_t)p * half; }
};

// state of the reliable-update CG (dslash_f32.hip, solver.cpp: solve_xx_sloppy_dev), resident on the device
struct SlpScal {
  double b2, r2stop;
  double r2t;                 // |b - A x|^2 of the last reliable update (fp64)
  double sigma, sigma_p;      // r_s = r / sigma; p_s is in units of sigma_p
  double r2s, r2s_old, maxr2s;   // |r_s|^2 now, one iteration back, max since the last update (units of sigma)
  int k, maxits, nupd;
  int done, upd, noupd;       // noupd = !upd: the `done` word the gated fp64 sweeps read
  int conv, first;            // the next k_slp_xpay rebuilds r_s from the fp64 residual / restarts p_s = r_s
};

// CG scalars resident on the device (no host round trip per iteration)
struct CgScal {
  double b2, r2, rzo, pAp, r2stop, tmp;
  int itn, maxits, done, pad;
  // plain CG (blas.hip): state after k iterations in slot k&1, so that the kernel which closes iteration k-1 can
  // write slot k&1 while its other workgroups still read slot (k-1)&1
  double r2s[2];
  int itns[2], dones[2];
  // sharded: {r2, -r2, itn, -itn} of the state the host is about to read, max-reduced over the ranks at the end of a chunk:
  // the ranks decide on `done` each for itself, so their residuals must agree bit for bit (comm_agree)
  double agree[4];
};

struct TimerSlot {
  std::vector<hipEvent_t> ev;  // pairs
  size_t used = 0;
  long count = 0;
  double total_ms = 0;
};

// Device-side stream join and the one error word of every bounded device-side wait (peer.hip).  `signal` raises a counter behind what a
// stream has posted (a one-lane kernel), `wait` makes another stream wait for it (a one-wave kernel with a bounded poll) -- instead of
// the runtime's cross-queue event dependency, which costs ~20-28 us of dead time per join here (profiles/r05_timeline_*.txt).  Both
// transports use it since round 6.
struct DevJoin {
  unsigned long long *ready = nullptr;   // device: word k*16 = joins FROM stream k (0 compute, 1 comm); word 56: start time of the fused sweep's push (emulation)
  unsigned long long *err = nullptr;     // pinned host word: code of the first wait that gave up
  long long ticks = 0;                   // QEXHIP_PEER_TIMEOUT in wall_clock64 ticks
  double timeout_s = 30.0;
  unsigned long long seq[2]{0, 0};
  int deferred = 0;                      // the compute stream still owes a wait for seq[1]: the next mailbox all-reduce of partials polls for it in its
                                         // prologue, anything else posts it first (devjoin_flush)
};

// natural-layout gauge field for plaquette / flow (gauge.hip) and gauge fixing (gaugefix.hip)
struct GaugeNat {
  double2 *U = nullptr, *F = nullptr, *P = nullptr;
  double2 *U2 = nullptr;   // second link buffer: the fused flow stage reads U and writes exp(v) U here, then they swap
  double2 *D2 = nullptr;   // double links U_a(x) U_a(x+a) of the rectangle force (k_double_links / k_force_rect)
  size_t n2 = 0;  // double2 elements per field (incl. ghost tiles when t is sharded)
  int ghost_valid = 0;   // depth to which the ghost slices of U are current
  double *pp = nullptr; int npp = 0;   // per-workgroup plaquette partials of k_plaq
  double2 *M = nullptr;      // resident MD momenta (qexhip_md_*)
  double2 *Usave = nullptr;  // links saved around a force-gradient shift
  int save_ghost_valid = 0;
};
struct PeerComm;  // peer-memory transport (peer.hip)

// A resident basis of half-volume vectors (eig.hip): nvecs vectors of the EVEN parity's body tiles only, each in the vec_off layout
// ([tile][3][64] double2, n2 = ntile*192 elements, spare lanes of a ragged last tile zero), contiguous per vector.
struct EigBasis {
  double2 *v = nullptr;
  int nvecs = 0;
  size_t n2 = 0;
  unsigned long gen = 0;        // c->links_gen its vectors were computed / last set on
  std::vector<double> evals;    // Rayleigh quotients <v_i, H v_i> of the leading nevals vectors (H = -D_eo D_oe)
  int nevals = 0;
};

enum { WK_SLOTS = 16 };   // >= WK_N (below)

struct qexhip_ctx {
  int device = 0;
  Geom g{};
  int rankGeom[4]{1, 1, 1, 1}, rankCoord[4]{0, 0, 0, 0};
  hipStream_t stream = nullptr, cstream = nullptr;
  hipEvent_t ev_ready = nullptr;      // compute -> comm stream: "the producer of the faces is done" (the way back is a device-side join: DevJoin)
  // communicator
  void *comm = nullptr;  // ncclComm_t: everything posted on the compute stream (all-reduces, ghost refreshes, non-overlapped faces)
  void *comm2 = nullptr; // ncclComm_t split off comm: the face exchanges posted on cstream beside the interior sweep
  PeerComm *peer = nullptr; // peer-mapped memory (peer.hip): control block with the mailboxes of the rank sums, and -- when `comm` is null -- the
                            // receive arenas of the faces too.  comm && peer: RCCL faces + mailbox sums (hybrid_sums)
  DevJoin dj;               // device-side stream joins + the error word of the bounded waits (allocated by qexhip_init)
  int opt_transport = -1;   // option "transport" (before comm_init): -1 QEXHIP_TRANSPORT decides, 0 auto, 1 rccl, 2 peer
  int nranks = 1, rank = 0;
  int force_halo = 0;
  // staggered links
  double2 *W = nullptr;  // [parity][tile][ndir][9][64]
  int ndir = 0;
  // device fields
  std::map<int, DevField> fields;
  int next_field = 1;
  // scratch
  double *stage = nullptr; size_t stage_bytes = 0;   // host-format staging on device
  double *partials = nullptr; int npartials = 0;     // block partial sums: [0,part2_off) Dslash / redot, then 2048 for the CG update
  int part2_off = 0;
  double *dscal = nullptr;                           // 64 device scalars (reductions), by owner: [0..4] solvers (b2, r2, norms of
                                                     // the full solve), [8..9] the BLAS entry points, [16..21] plaquettes, [24..32]
                                                     // flow observables / action / line sums, [34] link trace (gaugefix.hip), [40..51]
                                                     // s4 / Polyakov sums, [56..59] comm_allreduce_max, [60] comm_init's agreement,
                                                     // [62] link-compression test
  CgScal *cg = nullptr;                              // device CG state
  struct { int valid = 0; const double2 *x = nullptr; int par_even = 0; double m2 = 0; int k = 0; } cg_resume;   // what solve_xx_continue_dev needs
  int cg_r2parts = 0;                                // values the |r|^2 partial buffer holds after the last cg_update (1 once a peer all-reduce has summed them)
  double *hist = nullptr; int histcap = 0;           // device residual history
  void *pinned = nullptr;                            // pinned host scratch (4 KiB)
  // work vectors (lazily allocated, like the {.global.} temp of stagD.nim:437-442)
  int wk[WK_SLOTS]{0};
  // timers
  int timers_on = 0;
  std::map<std::string, TimerSlot> timers;
  // compressed links (recon = 1: rows 0,1 + sign mask; 2: rows 0,1 + det; row 2 rebuilt in the kernel)
  double2 *Wc = nullptr; unsigned long long *Ws = nullptr; size_t Wc_rows = 0; int recon = 0; double recon_dev = 0;
  // lossless formats (link_residual.h) of 8-link operators that fit neither format: lres = 1 the residual format (rows 0,1 + int16
  // residuals of row 2 in Wc, [sign, escape] masks per row in Wm), 2 its packed form (residuals in the exponent bits of rows 0,1;
  // same masks), 3 its orthogonal form (row 1's last element rebuilt too, 92 B; same masks); recon stays 0 (the values ARE the 18-real links, which W keeps: the escaped lanes,
  // the fp32 builder and every kernel but k_dslash / k_dslash_fused read them there)
  unsigned long long *Wm = nullptr; size_t Wm_rows = 0; int lres = 0; long long lres_esc = 0;
  int opt_lossless = 3;   // option "lossless": 0 keeps the lossless formats off, 1 the residual format only, 2 the packed form first, 3 the orthogonal form first
  int opt_batch_multi = 0; // test hook: take the multi-rank reduction branch of the batched CG on one rank
  int opt_multi_reduce = 0; // test hook: take the multi-rank reduction branches of CG / multi-shift CG / norms on one rank
                            // (with a one-rank RCCL communicator the all-reduces are real collectives)
  int opt_force_pair = 1; // option "force_pair" (test hook): 0 takes k_force_lds, the form lattice shapes without paired tile positions get, on any shape
  int opt_obs_clover = 1; // option "obs_clover" (test hook): 0 takes the generic path walker, the form fmunu loops 3-5 get, for loop 1 as well
  int opt_hop_split = -1;    // option "hop_split" / QEXHIP_HOP_SPLIT: how an OVERLAPPED sweep is laid out on the peer transport.  2 = the fused sweep
                             // (k_dslash_fused: ONE launch on ONE stream pushes the faces, takes the interior, and its boundary workgroups take
                             // the hops that stay inside the slab, wait SHORTLY for the faces, and either finish or park their accumulator for
                             // the cleanup workgroups at the end of the grid), 0 = split by sites (interior launch | exchange + boundary launch
                             // on the comm stream, device-side join; what the RCCL transport always runs), -1 = whichever set_links measured
                             // faster (fused until measured; sweep_autotune)
  int opt_fused_spin_us = -1; // option "fused_spin_us": the short wait of the fused sweep's boundary workgroups; -1 = about the measured (else estimated)
                              // transfer time, >= 0 that many microseconds, -2 = park every boundary block (test hook: cleanup path everywhere)
  int ranks_share_device = 0;   // comm_init's rendezvous saw two ranks of this job on one GPU (informational: no kernel holds more than a few
                                // dozen slots while it waits for another rank any more)
  int hybrid_sums = 0;          // RCCL carries the faces, the mailboxes of the peer control block the CG's rank sums (comm.cpp: comm_init)
  unsigned int *fz_buf = nullptr; int fz_cap = 0;   // FusedCtl words + parked-block list of the fused sweep (dslash.hip)
  const double2 *bnd_out_on_cstream = nullptr;      // the parity half whose t-faces the LAST sweep's boundary launch wrote on the comm stream (split by sites), else null
  double xchg_us[2]{0, 0};      // measured at set_links (collective, max over ranks): one face exchange of the 8- / 16-link operator, us (0: not measured)
  int form_auto[2]{-1, -1};     // measured at set_links: 2 fused / 0 by sites for 8- and 16-link operators (-1: not measured)
  int opt_chain_overlap = 1; // option "chain_overlap" (A/B, test hook): 1 = the nHYP force chain's staple derivatives of a t-sharded field run in two passes,
                          // the ghost-free slices beside the exchange of the level's chain fields, the boundary slices behind it
  int opt_hisq_md_fused = 3;  // option "hisq_md_fused" (A/B, test hook): bit 0 = the outer products of qexhip_md_hisq_fforce* in k_outer13 launches (0: the 2n
                          // k_outer launches they replace), bit 1 = TAH and kick in k_projtah_kick (0: k_force_projtah, then k_links_axpy); same bits either way
  int opt_smear_ca = 1;   // option "smear_ca" (A/B, test hook): 1 = the nHYP levels of a t-sharded field are computed on shrinking ghost slices from
                          // ONE depth-3 thin-link exchange; 0 = every projected level field refreshes its ghost slices (rounds 1-4)
  int opt_flow_exp = 1;   // QEXHIP_FLOW_EXP / option "flow_exp": 1 = closed-form exp(v) in the fused Wilson-flow stage (same function,
                          // another algorithm than the reference's; agrees with it to ~1e-15 per element; the default); 0 = the reference's
                          // Taylor + 20 squarings (matexp.nim), which the MD link updates always use
  int opt_recon = 2;      // QEXHIP_RECON: 0 keeps the 18-real links always, 1 sign format only, 2 also the U(3) format
  int opt_overlap = -1;  // QEXHIP_OVERLAP / option "overlap": 1 always use the comm stream, 0 never, -1 measured once per operator shape when the
                         // communicator has more than one rank (sweep_autotune), by interior / face size otherwise; -2: measure on one rank too
  int emu_link_gbs = 0;                            // option emu_link_gbs: > 0 adds bytes / (GB/s of one xGMI direction) to every emulated exchange
  int emu_exchange_us = 0, emu_allreduce_us = 0;   // options of the same names (test / rehearsal hooks): delay posted in front of every face
                                                   // exchange / all-reduce, as long as the transfer would take between distinct GPUs
  int overlap_auto[2]{-1, -1};          // the measured decision for 8- and 16-link operators (-1: not measured)
  double overlap_tune_us[2][3]{};       // us per sweep the measurement saw: [8 | 16 links][exchange first | overlapped by sites | fused], max over ranks (0: form not available)
  // natural gauge (flow)
  GaugeNat *gn = nullptr;
  void *nhyp = nullptr;   // NhypState (smear.hip): the smearGetForce closure
  void *hisq = nullptr;   // HisqState (smear.hip): HisqCoefs.smearGetForce's closure
  // small per-context device scratch owned by single kernels' host wrappers
  double2 *outer_F = nullptr; size_t outer_Fn = 0;   // force field of stag_outer_host (force.hip)
  int tile_pairs_ok = 0;   // tile_order_table: every even slot holds (tile, 0) and the next one (tile, 1) (or both are padding): k_force_lds2
  int *tile_order = nullptr; int tile_order_n = 0;   // blocked (tile, parity) visiting order of the gather kernels (gauge.hip)
  int *tile_order_pl[16]{};                          // the same for kernels that shift in the (mu, nu) plane only (layout.hip)
  void *obs_table = nullptr;                         // ObsTable of gauge_flow_obs (gauge.hip)
  void *batch = nullptr;                             // BatchState of the lock-step multi-system CG (batch.hip)
  int lds_attr_done = 0;                             // per context (= per device): which kernels had MaxDynamicSharedMemorySize raised (bit 0 k_force_lds, 1 k_flow_obs_clover, 2 k_flow_obs_clover2, 3 k_force_lds2, 4 k_projUderiv_batch)
  void *cgm_scal = nullptr;                          // CgmScal of the multi-shift solver (multishift.hip)
  double *meson_buf = nullptr; size_t meson_cap = 0; // workgroup partials + global table of the meson / slice-norm reductions (meson.hip)
  unsigned long links_gen = 0;                       // bumped by every writer of W / Wc (links_compress ends each of them): the fp32 copy's staleness test
  void *f32 = nullptr;                               // F32State (dslash_f32.hip): fp32 links + fields + SlpScal of the mixed-precision CG
  void *batch_f32 = nullptr;                         // BatchLowpState<StoreF32> (batch_lowp.h): fp32 fields + SlpScal[4] of the mixed-precision batched CG
  void *msf32 = nullptr;                             // MsfState (multishift_f32.hip): fp32 search directions / increments of the mixed-precision multi-shift CG
  void *gfix = nullptr;                              // GfState (gaugefix.hip): transform field t, polish scratch, device loop state
  int opt_gfix_check = 16;                           // option "gfix_check": relax iterations posted between two read-backs of the gauge-fixing state
  std::map<int, EigBasis> bases; int next_basis = 1; // the user's eigenvector bases (qexhip_eig_new)
  void *eig = nullptr;                               // EigWork (eig.hip): Lanczos work fields, coefficient / partial / Q buffers
  int deflate_basis = 0, deflate_nev = 0;            // set around a deflated full solve: its inner solveEE calls deflate with this basis
  std::map<int, DevCField> cfields; int next_cfield = 1;   // the user's complex site fields (qexhip_cfield_new)
  void *stout = nullptr;                             // StoutState (stout.hip): the stout chain's levels, backward scratch, inverse loop state
  int md_src1_stout = 0;                             // MD force source 1 is the stout chain's force (the closure that wrote last), else the nHYP closure's
  int opt_stout_check = 8;                           // option "stout_check": inverse iterations posted between two read-backs of the loop state
  void *half = nullptr;                              // HalfState (dslash_half.hip): 16-bit links + fields + stall guard of the SloppyHalf CG
  int opt_half = 0;                                  // option "half": 1 = sloppy = 2 runs the 16-bit path (single-system solves, sharded or not)
  int opt_half_stall = 2;                            // option "half_stall": failed reliable updates in a row before the 16-bit solve finishes in fp32
  struct { int precision = 0, half_iters = 0, f32_iters = 0, fell_back = 0; } slp_last;   // the last sloppy solve (qexhip_stag_sloppy_last)
  void *batch_half = nullptr;                        // BatchLowpState<StoreHalf> (batch_lowp.h): 16-bit fields, x_s, SlpScal[4] and stall guards of the 16-bit lock-step batch
  int opt_half_batch = 0;                            // option "half_batch": 1 = sloppy = 2 on the batched entries runs the 16-bit batch (one rank, no ghost zones)
  // the last batched sloppy call per system (qexhip_stag_sloppy_last_batch); map: system of the entry <- system of the inner batch
  struct { int n = 0, precision[4] = {0, 0, 0, 0}, half_iters[4] = {0, 0, 0, 0}, f32_iters[4] = {0, 0, 0, 0}, fell_back[4] = {0, 0, 0, 0},
           map[4] = {0, 1, 2, 3}; } slpb_last;
  int opt_batch_ranks = 0;                           // option "batch_ranks": 1 = the batched sloppy entries run on t-sharded contexts (more than one rank, or
                                                     // ghost zones in t); 0 = they refuse there.  Set on every rank
  int opt_sloppy_check = 4;                          // option "sloppy_check": the gated reliable-update launches are posted every this many fp32
                                                     // iterations (solver.cpp: solve_xx_sloppy_dev)
};

// work-field slots (get_work)
enum { WK_T = 0, WK_R, WK_P, WK_AP, WK_Y, WK_D, WK_R2, WK_XT, WK_IN, WK_OUT, WK_IN2, WK_N };

// ---- error handling ----
void qexhip_set_error(const char *fmt, ...);
#define HIPCHK(expr)                                                                     \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess) {                                                              \
      qexhip_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
      return -2;                                                                         \
    }                                                                                    \
  } while (0)
#define CHK(expr) do { int r_ = (expr); if (r_ != 0) return r_; } while (0)

// ---- timers ----
struct ScopedTimer {
  qexhip_ctx *c; TimerSlot *s = nullptr; hipStream_t st;
  ScopedTimer(qexhip_ctx *c_, const char *name, hipStream_t st_);
  ~ScopedTimer();
};
int timers_collect(qexhip_ctx *c);
// reserve an event pair of timer class `name` (false when timing is off for that class)
bool timer_event_pair(qexhip_ctx *c, const char *name, hipEvent_t *e0, hipEvent_t *e1);

// ---- layout.hip ----
int geom_init(Geom &g, const int X[4], int depth, int halo);
int field_alloc(qexhip_ctx *c, DevField &f);
int field_upload(qexhip_ctx *c, DevField &f, const double *host);      // host MILC order -> tiles
int field_download(qexhip_ctx *c, const DevField &f, double *host);
int links_upload(qexhip_ctx *c, const double *fat, const double *lng);
int ensure_stage(qexhip_ctx *c, size_t bytes);
int links_from_natural(qexhip_ctx *c, const double2 *fat, const double2 *lng);
int links_compress(qexhip_ctx *c);
// lossless form `form`'s (1, 2, 3: link_residual.h) encoder + decoder on the host; out: row 2 (form 1) or the whole link, as decoded
int link_lossless_host(int form, const double2 *u, long n, unsigned char *escaped, double2 *out);
int op_eo_reconstruct_pub(qexhip_ctx *c, DevField &r, DevField &b, double m);
int op_eo_reduce_pub(qexhip_ctx *c, DevField &r, DevField &b, double m);
int op_stagD_pub(qexhip_ctx *c, DevField &r, DevField &x, int parity, double m, double sc, double a);   // one subset of stagD
void batch_state_free(qexhip_ctx *c);
int batch_io_fields(qexhip_ctx *c, int n, DevField **xs, DevField **bs);
int solve_full_batch_dev(qexhip_ctx *c, int n, DevField **x, DevField **b, const double *mass, const double *r2req,
                         int maxits, int *iters, double *r2_final);
int batch_work_fields(qexhip_ctx *c, int count, DevField **out);
int solve_xx_batch_dev(qexhip_ctx *c, int n, DevField **x, DevField **b, const double *mass, const double *r2req,
                       int maxits, int par_even, int *iters, double *r2_over_b2);      // n (1..4) solveXX's in lock-step, fp64
// ---- batch_f32.hip: the mixed-precision lock-step batch, fp32 storage (the driver of both storages: batch_lowp.h) ----
void batch_f32_state_free(qexhip_ctx *c);
int batch_sloppy_check(qexhip_ctx *c, int n, const double *mass);     // n in 1..4, not t-sharded unless option batch_ranks, no mass 0 -- before anything is launched
int solve_xx_batch_sloppy_dev(qexhip_ctx *c, int n, DevField **x, DevField **b, const double *mass, const double *r2req,
                              int maxits, int par_even, int *iters, double *r2_over_b2, int *nupdates);
int solve_full_batch_sloppy_dev(qexhip_ctx *c, int n, DevField **x, DevField **b, const double *mass, const double *r2req,
                                int maxits, int sloppy, int *iters, double *r2_final, int *nupdates);     // (batch.hip)
#define QX_MAXRHS 4
struct SlpBatch {
  double2 *x[QX_MAXRHS], *r[QX_MAXRHS];          // fp64: solution, true residual
  const double2 *b[QX_MAXRHS], *Ax[QX_MAXRHS];   // fp64: source, A x of the reliable update
  float2 *rs[QX_MAXRHS], *ps[QX_MAXRHS], *xs[QX_MAXRHS];
  const float2 *aps[QX_MAXRHS];
  double *dotp[QX_MAXRHS], *r2p[QX_MAXRHS];      // <p,Ap> partials of the second sweep; |r_s|^2 / |b - A x|^2 partials
  SlpScal *s;
};
// k_slpb_close / k_slpb_flush / k_slpb_resid + k_slpb_rclose for n systems, for the driver of both storages (nvec, nbb: the fp64 kernels' size and grid)
int slpb_close(qexhip_ctx *c, const SlpBatch &L, int n, int nparts, size_t r2stride);      // (r2stride: doubles between two systems' r2p)
int slpb_flush(qexhip_ctx *c, const SlpBatch &L, int n, size_t nvec, int nbb);
int slpb_resid(qexhip_ctx *c, const SlpBatch &L, int n, size_t nvec, int nbb, size_t r2stride);

// ---- batch_half.hip: the lock-step batch in 16-bit storage (option "half_batch"; the driver: batch_lowp.h) ----
void batch_half_state_free(qexhip_ctx *c);
int solve_xx_batch_half_dev(qexhip_ctx *c, int n, DevField **x, DevField **b, const double *mass, const double *r2req,
                            int maxits, int par_even, int *iters, double *r2_over_b2, int *nupdates);
// the batched sloppy solveXX of either storage: sloppy = 2 takes the 16-bit batch where option "half_batch" is set (one rank, no
// ghost zones), everything else the fp32 batch; both add what they ran to c->slpb_last through its map
int solve_xx_batch_sloppy_any(qexhip_ctx *c, int sloppy, int n, DevField **x, DevField **b, const double *mass, const double *r2req,
                              int maxits, int par_even, int *iters, double *r2_over_b2, int *nupdates);
void slpb_last_reset(qexhip_ctx *c, int n);             // the batched entries start a new report
int half_op_xx_batch_probe(qexhip_ctx *c, int n, DevField **fr, DevField **fx, const double *m2, int par_even);
int f32_op_xx_batch_probe(qexhip_ctx *c, int n, DevField **fr, DevField **fx, const double *m2, int par_even);     // (batch_f32.hip)
int nhyp_fforce(qexhip_ctx *c, double *f_host, int n, const double *const *phi, const double *mass, const double *scale,
                const double *r2req, int maxits, int bcmask, const int ph[4], int *iters, DevField *const *phi_dev = nullptr);

// reductions end in an all-reduce: more than one rank, or the one-rank rehearsal of that code path
inline bool multi_rank(const qexhip_ctx *c) { return c->nranks > 1 || c->opt_multi_reduce; }

// ---- comm.cpp ----
int comm_halo_push_only_multi(qexhip_ctx *c, int n, DevField *const *f, int parity, const double2 **gh_hi, const double2 **gh_lo, struct PeerPush *push);
                                                                              // peer faces, n <= 4 fields: the fused sweep pushes them itself
                                                                              // and reads what arrives in the receive arena
int comm_halo_exchange(qexhip_ctx *c, DevField &f, int parity, int overlap, bool wait_ready = true);  // overlap: on cstream after ev_ready (wait_ready);
                                                                              // the caller joins behind what it posts next
int comm_halo_exchange_sites(qexhip_ctx *c, void *half, size_t site_bytes, int overlap);  // the same for one parity half of an fp32 (24 B per site) or 16-bit (16 B) field
int comm_halo_exchange_multi(qexhip_ctx *c, int n, DevField *const *f, int parity, int overlap);   // n fields, one RCCL group
int comm_halo_exchange_sites_multi(qexhip_ctx *c, int n, void *const *halves, size_t site_bytes, int overlap);   // n (<= 4) reduced-precision parity halves, one group
int comm_allreduce(qexhip_ctx *c, double *dptr, int n);          // on stream
int comm_allreduce_parts(qexhip_ctx *c, double *parts, int n, int *n_out);   // workgroup partials -> *n_out values whose sum is the rank-global dot product
// the same for m (<= 4) systems' partials parts0 + j stride in ONE collective, each system summed as alone; gate: see comm.cpp
int comm_allreduce_parts_multi(qexhip_ctx *c, int m, double *parts0, size_t stride, int n, const SlpScal *st, int gate, int *n_out);
int comm_allreduce_max(qexhip_ctx *c, double *host, int n);      // host values -> max over the ranks, back on the host (n <= 4, synchronous)
int comm_agree_post(qexhip_ctx *c);                               // max-reduce c->cg->agree over the ranks (on stream)
int comm_agree_check(qexhip_ctx *c, const CgScal &host);          // after the state was read back: all ranks hold the same residual and count
int comm_allgather(qexhip_ctx *c, const double *send, double *recv, size_t n);
int comm_faces_exchange(qexhip_ctx *c, int nbuf, double *const bottom[], double *const top[], double *const ghost_hi[],
                        double *const ghost_lo[], size_t ndoubles, int async = 0);   // async: on the comm stream after ev_ready, no join
int comm_exchange_raw(qexhip_ctx *c, const void *send_up, void *recv_from_down, size_t bytes, hipStream_t st);
void comm_destroy(qexhip_ctx *c);
inline bool comm_ready(const qexhip_ctx *c) { return c->comm != nullptr || c->peer != nullptr; }
inline bool peer_faces(const qexhip_ctx *c) { return c->peer != nullptr && c->comm == nullptr; }    // the faces travel through peer-mapped arenas (else RCCL / copies)

// ---- peer.hip: device-side joins, and the peer-memory transport behind the same comm_* entry points ----
int devjoin_init(qexhip_ctx *c);                                                  // qexhip_init
void devjoin_destroy(qexhip_ctx *c);
int devjoin_check(qexhip_ctx *c);                       // a bounded device-side wait gave up since the last check -> QEXHIP_ERR_COMM
int devjoin_signal(qexhip_ctx *c, hipStream_t from);                              // device-side event: record ...
int devjoin_wait(qexhip_ctx *c, hipStream_t waiter, hipStream_t from);            // ... and wait, without the runtime's cross-queue dependency
int devjoin_defer(qexhip_ctx *c);                                                 // the compute stream's wait rides in the next peer_allreduce_parts ...
int devjoin_flush(qexhip_ctx *c);                                                 // ... or is posted now (no-op when nothing is deferred)
struct PeerHost;
int peer_init(qexhip_ctx *c, PeerHost &host);          // after the host rendezvous (collective): control block exported, everybody's mapped
int peer_selftest(qexhip_ctx *c);                       // a few mailbox all-reduces with known answers (collective; bounded): 0 = this rank saw the right sums
void peer_destroy(qexhip_ctx *c);
inline int peer_check(qexhip_ctx *c) { return devjoin_check(c); }
int peer_exchange(qexhip_ctx *c, hipStream_t st, int ns_dn, const void *const *src_dn, int ns_up, const void *const *src_up,
                  void *const *dst_from_up, void *const *dst_from_dn, size_t bytes, double emu_us = 0.0, const void **zc_from_up = nullptr,
                  const void **zc_from_dn = nullptr, struct PeerPush *push_only = nullptr);   // push_only (+ zc_*): nothing is launched, the caller's kernel
                                                                                              // pushes and reads the arena (credits owed: peer_ghost_args)
int peer_allreduce_parts(qexhip_ctx *c, double *parts, int n);       // parts[0] := sum over ranks of (sum of parts[0..n) in cg_sum_parts order)
int peer_allreduce_parts_multi(qexhip_ctx *c, int m, double *parts0, size_t stride, int n, const SlpScal *st, int gate);   // per system j, into parts0[j stride]
int peer_allreduce(qexhip_ctx *c, double *dptr, int n, int op);      // on the compute stream; op 0 sum, 1 max; rank order
int peer_host_reduce(qexhip_ctx *c, double *host, int n, int op);    // host operands (op 0 max, 1 min, 2 sum), synchronous
int peer_allgather(qexhip_ctx *c, const double *send, double *recv, size_t n);
void peer_info(const qexhip_ctx *c, long out[4]);                    // exchanges, all-reduces, arena growths, arena bytes

// ---- dslash.hip ----
// out[parity] = ca*rin + cb*xs + sgn * sum_mu [ U x(+) - U^+ x(-) ]; optional dot = Re<xs,out> partials
struct DslashOpts {
  double ca = 0, cb = 0;
  const DevField *rin = nullptr;   // a-term source (same parity as out)
  const DevField *xs = nullptr;    // b-term source (same parity as out)
  int neg = 0;                     // 1: subtract the hop sum (stagDM)
  double post = 1.0;               // out *= post  (stagD's 0.5*sc)
  int dot = 0;                     // 1: write block partials of Re<xs,out> and reduce into dot_out
                                   // 2: leave the partials in c->partials[0..*nparts_out) (deferred)
  int *nparts_out = nullptr;
  double *dot_out = nullptr;       // device scalar
  const int *done = nullptr;       // device flag: skip when set
  int pair2 = 0;                   // second sweep of a back-to-back pair out2 = D (D in) (op_xx): its input is the first sweep's output and nothing came
                                   // between -- where the first sweep's boundary launch ran on the comm stream, the faces this sweep sends were
                                   // produced THERE: its exchange is posted at once, only its boundary launch waits for the first sweep's interior
  int defer_join = 0;              // the caller's next operation on the compute stream is comm_allreduce_parts (or devjoin_flush): a sweep split by
                                   // sites leaves its join from the comm stream to that kernel's prologue where the mailboxes carry the sum
};
int dslash_sweep(qexhip_ctx *c, DevField &out, DevField &in, int parity, const DslashOpts &o);
// The storage a sweep reads its links from -- what set_links chose; `lossless` false: the 18 reals kept beside a lossless form --:
// the sweep kernels' RECON (dslash_core.h), double2 per (tile, direction) row, bytes per link
struct LinkStorage { int recon, lrow, bytes; };
LinkStorage stag_link_storage(const qexhip_ctx *c, bool lossless = true);
void stag_link_bases(const qexhip_ctx *c, int parity, bool lossless, const double2 **W, const unsigned long long **S);   // a parity's link and mask base
int sweep_autotune(qexhip_ctx *c);      // measure the sweep's forms once per operator shape (collective)
void sweep_plan(const qexhip_ctx *c, int *lo_end, int *hi_beg, int *overlap);   // boundary / interior ranges and the overlap decision
int sweep_form(const qexhip_ctx *c, int overlap);                              // 2 fused / 0 by sites: what an overlapped sweep runs as
double sweep_push_fraction(const qexhip_ctx *c, int interior_sites, int nrhs = 1);   // where in the dispatch order the fused sweep's boundary workgroups go

// ---- dslash_f32.hip (mixed-precision CG; whole lattice or t-sharded slab) ----
enum { F32_T = 0, F32_R, F32_P, F32_AP, F32_X, F32_IN, F32_NF };   // fp32 work fields
#define SLP_DELTA 0.1                                    // reliable-update delta (QEX's reliable_delta, qudaSet.nim:63)
int f32_links(qexhip_ctx *c, int *fmt, double *dev);     // the fp32 copy of the links, rebuilt when links_gen moved
int f32_links_dev(qexhip_ctx *c, int parity, const void **W, const unsigned long long **S, int *fmt);   // behind f32_links: the copy's bases for one output parity (W: float4); pure accessor
int f32_field(qexhip_ctx *c, int slot, DevFieldF **f);
int f32_field_ensure(qexhip_ctx *c, DevFieldF &F);       // (re)allocates F, zeroed, at the current geometry's size
int f32_op_xx(qexhip_ctx *c, DevFieldF &r, DevFieldF &x, double m2, int par_even, int dot, const int *done, int *nparts);
int f32_from_f64(qexhip_ctx *c, DevFieldF &y, const DevField &x, int parity, double a);              // y = f32(a x)
int f32_to_f64(qexhip_ctx *c, DevField &y, const DevFieldF &x, int parity, double a, int accumulate);  // y (+)= a x
void f32_state_free(qexhip_ctx *c);
int slp_alloc(qexhip_ctx *c, SlpScal **s);
int slp_init(qexhip_ctx *c, SlpScal *s, double r2req, int maxits);
int slp_xpay(qexhip_ctx *c, SlpScal *s, DevFieldF &p, DevFieldF &rs, const DevField &r, int parity);
int slp_update(qexhip_ctx *c, SlpScal *s, DevFieldF &xs, DevFieldF &rs, const DevFieldF &p, const DevFieldF &Ap, int parity, int ndot);
int slp_flush(qexhip_ctx *c, SlpScal *s, DevField &x, DevFieldF &xs, int parity);
int slp_resid(qexhip_ctx *c, SlpScal *s, DevField &r, const DevField &b, const DevField &Ax, int parity);
int slp_iterate(qexhip_ctx *c, SlpScal *s, DevFieldF &xs, const DevField &r, double m2, int par_even);   // one fp32 iteration on F32_R / F32_P / F32_AP
int slp_close(qexhip_ctx *c, SlpScal *s, const double *r2p, int nparts);     // k_slp_close alone, on rank-global partials

// ---- dslash_half.hip (16-bit storage for the sloppy CG: whole lattice or t-sharded slab, one system) ----
enum { HALF_T = 0, HALF_R, HALF_P, HALF_AP, HALF_IN, HALF_NF };   // 16-bit work fields
int half_pack_host(const double *v, size_t nsites, int16_t *q, float *norm);       // the vector format on the host
int half_unpack_host(const int16_t *q, const float *norm, size_t nsites, double *v);
int half_links(qexhip_ctx *c, int *fmt, double *s_fat, double *s_long, double *dev);   // the 16-bit copy of the links, rebuilt when links_gen moved
                                                                                       // (sharded: collective; the values are rank-global)
int half_op_xx_probe(qexhip_ctx *c, DevField &fr, const DevField &fx, double m2, int par_even);
int slph_begin(qexhip_ctx *c, SlpScal *s);               // links + the stall guard's state, behind slp_init
int slph_iterate(qexhip_ctx *c, SlpScal *s, DevFieldF &xs, const DevField &r, double m2, int par_even);   // one 16-bit iteration
int slph_stall(qexhip_ctx *c, SlpScal *s, int limit);    // behind a gated reliable update: the stall guard
int slph_stalled_async(qexhip_ctx *c, int *pinned);      // the guard's `stalled` flag -> pinned host memory, on the compute stream
void half_state_free(qexhip_ctx *c);

// ---- multishift_f32.hip: the fp32 iteration of the mixed-precision multi-shift CG ----
#define CGM_MAXM 32                                      // shifts per multi-shift solve (fp64 and mixed)
void msf_state_free(qexhip_ctx *c);
int msf_r2_buffer(qexhip_ctx *c, double **dev);          // 32 device scalars: the per-shift |b - A_k x_k|^2 of the refinement phase
int msf_start(qexhip_ctx *c, SlpScal *s, DevFieldF &rs, const DevField &b, std::vector<DevField *> &xs, const double *shifts, int nmass,
              int parity, DevFieldF **ps0);
int msf_iterate(qexhip_ctx *c, SlpScal *s, DevFieldF &rs, const DevFieldF &Ap, const DevField &r, int parity, int ndot);
int msf_flush(qexhip_ctx *c, SlpScal *s, int nmass);

// ---- blas.hip ----
int blas_zero(qexhip_ctx *c, DevField &f, int parity);
int blas_copy(qexhip_ctx *c, DevField &dst, const DevField &src, int parity);
int blas_axpy(qexhip_ctx *c, double a, const DevField &x, DevField &y, int parity);
int blas_xpay(qexhip_ctx *c, const DevField &x, double a, DevField &y, int parity);
int blas_scale(qexhip_ctx *c, double a, DevField &y, int parity);
int blas_axpby(qexhip_ctx *c, double a, const DevField &x, double b, const DevField &y, DevField &z, int parity);  // z = a x + b y
int blas_norm2(qexhip_ctx *c, const DevField &x, int parity, double *dev_out);   // rank-global
int blas_redot(qexhip_ctx *c, const DevField &x, const DevField &y, int parity, double *dev_out);
int blas_cdot(qexhip_ctx *c, const DevField &x, const DevField &y, int parity, double *dev_out);    // dev_out[0..1] = Re, Im of <x, y>
int tile_order_table(qexhip_ctx *c, const int **tab, int *chunk);   // blocked (tile, parity) visiting order, layout.hip
int tile_order_plane(qexhip_ctx *c, int mu, int nu, const int **tab, int *chunk);   // order for kernels whose gathers stay in the (mu, nu) plane
int reduce_partials(qexhip_ctx *c, int n, double *dev_out);  // sum partials[0..n) -> dev_out (+ allreduce)
int read_scalars(qexhip_ctx *c, const double *dev, int n, double *host);  // sync readback
int blas_grid(const qexhip_ctx *c, int parity_count);
int blas_delay(hipStream_t st, int us);      // transport emulation: a one-lane kernel that waits `us` microseconds on st
// CG fused kernels
int cg_xpay(qexhip_ctx *c, DevField &p, const DevField &r, int parity, int k, int rolled);
int cg_update(qexhip_ctx *c, DevField &x, DevField &r, const DevField &p, const DevField &Ap, int parity, int k, int ndot);
int cg_close(qexhip_ctx *c, int k);
int cg_init(qexhip_ctx *c, double r2req, int maxits);  // after b2 (dscal[0]) and r2 (dscal[1]) are known
int cg_resume(qexhip_ctx *c, int k, double r2req, int maxits);   // CgState re-entry: new stopping criterion on the kept state

// ---- solver.cpp ----
int get_work(qexhip_ctx *c, int slot, DevField **f);
int op_xx(qexhip_ctx *c, DevField &r, DevField &x, double m2, int par_even, int dot, const int *done, int *ndot = nullptr);
int op_D(qexhip_ctx *c, DevField &r, DevField &x, double m, double sc, double a = 0.0);
// the full solves' residual bookkeeping (single, lock-step batch, multi-shift): |f.even|^2 and |f.odd|^2 read back; r = b - D x first
int norm2_eo(qexhip_ctx *c, DevField &f, double *e, double *o);
int resid_eo(qexhip_ctx *c, DevField &r, DevField &b, DevField &x, double m, double *e, double *o);
int solve_xx_dev(qexhip_ctx *c, DevField &x, DevField &b, double mass, double r2req, int maxits,
                 int par_even, int *iters, double *r2_over_b2, double *hist, int histcap);
int solve_xx_continue_dev(qexhip_ctx *c, DevField &x, double r2req, int maxits, int *iters, double *r2_over_b2, double *hist, int histcap);
int solve_full_dev(qexhip_ctx *c, DevField &x, DevField &b, double mass, double r2req, int maxits,
                   int *iters, double *r2_final, int use_prev = 0, int sloppy = 0, int *nupdates = nullptr);
int solve_xx_sloppy_dev(qexhip_ctx *c, DevField &x, DevField &b, double mass, double r2req, int maxits, int par_even,
                        int *iters, double *r2_over_b2, int *nupdates);
// sharded: the state every rank read back at the end of a chunk (and a 16-bit solve's stall flag) is the same on all ranks, checked
// before any rank acts on it; one call per system for a batch
int slp_agree(qexhip_ctx *c, const SlpScal &h, int stalled = 0);
// the 16-bit solve (option "half"), and the single-system sloppy solve of either storage: sloppy = 2 takes the 16-bit one where
// the option is set, on one rank and on t-sharded slabs alike.  Both add what they ran to c->slp_last.
int solve_xx_half_dev(qexhip_ctx *c, DevField &x, DevField &b, double mass, double r2req, int maxits, int par_even,
                      int *iters, double *r2_over_b2, int *nupdates);
// the fp32 finish of a 16-bit solve whose stall guard tripped (single and batched): A e = r to r2stop / *r2t with solve_xx_sloppy_dev,
// x += e, the true residual recomputed once into *r2t (Ax: scratch).  Uses POOL_REF, POOL_REF + 4 and the single sloppy solve's fields.
int half_finish_f32(qexhip_ctx *c, DevField &x, DevField &b, const DevField &r, DevField &Ax, double mass, double r2stop, int maxits,
                    int par_even, double *r2t, int *its32, int *nupd32);
int solve_xx_sloppy_any(qexhip_ctx *c, int sloppy, DevField &x, DevField &b, double mass, double r2req, int maxits, int par_even,
                        int *iters, double *r2_over_b2, int *nupdates);
int solve_xx_multi_dev(qexhip_ctx *c, std::vector<DevField *> &xs, DevField &b, const double *shifts,
                       int nmass, double r2req, int maxits, int par_even, int *iters, double *hist, int histcap);
int solve_multi_dev(qexhip_ctx *c, std::vector<DevField *> &xs, DevField &b, const double *masses,
                    int nmass, double r2req, int maxits, int *iters, double *r2_final, int sloppy = 0, int *nupdates = nullptr);
// mixed-precision multi-shift solveXX: fp32 multi-shift iterations with reliable updates on the base shift, then per-shift refinement
// on the true residual (solver.cpp).  r2_over_b2[k]: |b - A_k x_k|^2 / |b|^2 of the returned x_k; refine_iters, nupdates may be null.
int multi_sloppy_check(qexhip_ctx *c, int sloppy, const double *vals, int nmass);      // QEXHIP_ERR_ARG before anything is launched
int solve_xx_multi_sloppy_dev(qexhip_ctx *c, std::vector<DevField *> &xs, DevField &b, const double *shifts, int nmass, double r2req,
                              int maxits, int par_even, int *iters, double *r2_over_b2, int *nupdates, int *refine_iters);
// persistent multi-shift workspace (multishift.hip): search directions, per-parity solutions, host-entry solutions
enum { POOL_PS = 0, POOL_YS = 32, POOL_XS = 64, POOL_REF = 96 };   // POOL_REF: 4 corrections + 4 residuals of the sloppy solve's refinement
int pool_field(qexhip_ctx *c, int idx, DevField **f);
// rational functions of M^+M (multishift.hip): the terms as the multi-shift solver takes them, and the accumulating solve
int rational_map(const char *who, double mass, int nterm, const double *alpha, const double *beta, double *shifts, int *order);
int rational_xx_dev(qexhip_ctx *c, DevField &out, DevField &b, double mass, double f0, int nterm, const double *alpha, const double *beta,
                    double r2req, int maxits, int par_even, int *iters, double *hist, int histcap);

int solve_xx_deflated_dev(qexhip_ctx *c, EigBasis &B, int nev, DevField &x, DevField &b, double mass, double r2req, int maxits,
                          int sloppy, int *iters, double *r2_over_b2);
// the deflated lock-step batch: n <= 4 solveXX's of either parity deflated from the EVEN basis (solver.cpp); nev = 0 is the
// undeflated batch entry itself.  r2_over_b2: the true residuals; nupdates (may be null): reliable updates of the sloppy batch
int solve_xx_batch_deflated_dev(qexhip_ctx *c, EigBasis &B, int nev, int n, DevField **x, DevField **b, const double *mass,
                                const double *r2req, int maxits, int par_even, int sloppy, int *iters, double *r2_over_b2, int *nupdates);
// n x Staggered.solve whose inner solveXX groups of both parities are the deflated batch (batch.hip)
int solve_full_batch_deflated_dev(qexhip_ctx *c, EigBasis &B, int nev, int n, DevField **x, DevField **b, const double *mass,
                                  const double *r2req, int maxits, int sloppy, int *iters, double *r2_final, int *nupdates);

// ---- eig.hip: basis of half-volume vectors + the three block kernels; eigsolve.cpp: thick-restart Lanczos ----
#define EIG_MAX_NVECS 512       // the in-place rotation keeps m x R site rows in LDS with R >= 16: m <= 512 at 128 KiB
#define EIG_MAXRHS 4            // right-hand sides of the multi-right-hand-side block kernels = systems of a lock-step batch
// EigWork fields; EIG_BR0 / EIG_BD / EIG_BZ + k: residual, correction and odd-projection work field of system k of a deflated batch
enum { EIG_W = 0, EIG_T0, EIG_T1, EIG_AP, EIG_R0, EIG_D, EIG_BR0, EIG_BD = EIG_BR0 + EIG_MAXRHS, EIG_BZ = EIG_BD + EIG_MAXRHS,
       EIG_NF = EIG_BZ + EIG_MAXRHS };
int eig_basis_find(qexhip_ctx *c, int id, EigBasis **B);
int eig_basis_new(qexhip_ctx *c, int nvecs, int *id);
int eig_basis_free(qexhip_ctx *c, int id);
void eig_bases_free(qexhip_ctx *c);                 // qexhip_finalize
void eig_state_free(qexhip_ctx *c);                 // the work fields and buffers only (qexhip_release_workspace)
int eig_field(qexhip_ctx *c, int slot, DevField **f);
int eig_coef_buffers(qexhip_ctx *c, double2 **dots, double2 **coef);      // EIG_MAXRHS x EIG_MAX_NVECS complex numbers each, on the device
int eig_get_vector(qexhip_ctx *c, const EigBasis &B, int i, DevField &f, double scale = 1.0);   // f.even := scale v_i
int eig_set_vector(qexhip_ctx *c, EigBasis &B, int i, const DevField &f, double scale = 1.0);   // v_i := scale f.even
int eig_move_vector(qexhip_ctx *c, EigBasis &B, int dst, int src);
// dots[j] = <v_{i0+j}, w.even>, j < n, rank-global, on the device
int eig_block_dot(qexhip_ctx *c, const EigBasis &B, int i0, int n, const DevField &w, double2 *dots);
// y.even += scale * sum_j coef[j] v_{i0+j}
int eig_block_axpy(qexhip_ctx *c, const EigBasis &B, int i0, int n, const double2 *coef, double scale, DevField &y);
// the two for nrhs <= EIG_MAXRHS fields in one pass over the basis, every number bit for bit the single call's:
// dots[k][j] = <v_{i0+j}, w_k.even> ([nrhs][n]);  y_k.even += scale * sum_j coef[k][j] v_{i0+j} (the y_k distinct)
int eig_block_dot_mrhs(qexhip_ctx *c, const EigBasis &B, int i0, int n, int nrhs, DevField *const *w, double2 *dots);
int eig_block_axpy_mrhs(qexhip_ctx *c, const EigBasis &B, int i0, int n, int nrhs, const double2 *coef, double scale, DevField *const *y);
// V[:, 0:k] <- V[:, 0:m] Q, Q real m x k column-major on the host
int eig_rotate(qexhip_ctx *c, EigBasis &B, int m, int k, const double *Q);
int eig_rayleigh(qexhip_ctx *c, EigBasis &B, int n);     // fills B.evals[0..n) where missing (one operator application each)
// low-mode averaging: cf.even.re += sum_j wgt[j] |v_{i0+j}|^2 (wgt on the device); cf.re += L(x) on both parities; phi_k <- (1 - P) phi_k
int eig_block_norm2_accum(qexhip_ctx *c, const EigBasis &B, int i0, int n, const double *wgt, DevCField &cf);
int eig_lowmode_diag(qexhip_ctx *c, EigBasis &B, int nev, double mass, DevCField &cf);
int eig_project_out(qexhip_ctx *c, EigBasis &B, int nev, int n, DevField *const *phi);
struct qexhip_eig_opts;
int eig_solve(qexhip_ctx *c, EigBasis &B, const qexhip_eig_opts &o, int *nconv, double *evals, double *resid, long stats[4]);

// ---- force.hip ----
int stag_outer_host(qexhip_ctx *c, double *f_host, const double *x_host, double se, double so, int accumulate);

// ---- meson.hip ----
int meson_corners(qexhip_ctx *c, int n, DevField *const *x, DevField *const *y, int t0, double *host_out);   // [nt_global][8], rank-global
int sym_shift(qexhip_ctx *c, DevField &r, const DevField &x, int mu);                                      // mu < 3, links set
int norm2slice(qexhip_ctx *c, const DevField &f, int dir, double *host_out);                                // [L_dir global], rank-global

int meson_scratch(qexhip_ctx *c, size_t npart, size_t nout, double **part, double **out);                      // device scratch [partials | table]
int meson_bins_final(qexhip_ctx *c, const double *partials, int nbin, int nsub, int nchunk, int off, int t0, int nglob, double *out);
                                                                       // k_bins_final: chunk-ordered sums into the rows of the global table
int meson_read_table(qexhip_ctx *c, const double *dev, size_t n, double *host);

// ---- trace.hip: dilution, site-wise trace accumulation and slice sums of the stochastic scalar trace ----
int cfield_alloc(qexhip_ctx *c, DevCField &f);
int cfield_zero(qexhip_ctx *c, DevCField &f);
int cfield_scale(qexhip_ctx *c, DevCField &f, double s);
int cfield_axpy(qexhip_ctx *c, DevCField &dst, double a, const DevCField &src);       // dst += a src, both components
int cfield_download(qexhip_ctx *c, const DevCField &f, double *host);                 // [V][2] in the site order of field_download
int trace_dilute(qexhip_ctx *c, int n, DevField *const *dst, const DevField &src, int kind, const int *idx, const int *t, double scale);
int trace_accum(qexhip_ctx *c, DevCField &tr, int n, DevField *const *a, DevField *const *b, double coef);
int cfield_slices(qexhip_ctx *c, const DevCField &tr, double *host_out);              // [nt_global][2], rank-global

// ---- conn.hip: point sources, translated |phi|^2 accumulation and staggered sign of the connected scalar correlator ----
int conn_point_source(qexhip_ctx *c, int n, DevField *const *dst, const int *pts, const int *ic);            // pts: [n][4], global
int conn_accum(qexhip_ctx *c, DevCField &tr, int n, DevField *const *phi, const int *pts, double scal);
int cfield_stag_sign(qexhip_ctx *c, DevCField &f);

// ---- smear.hip ----
int smear_fat7_host(qexhip_ctx *c, const double *g_host, const double coef[5], double *fl_host, double *ll_host, double naik);
int smear_hisq_host(qexhip_ctx *c, const double *g_host, double *fl_host, double *ll_host);
int smear_nhyp_host(qexhip_ctx *c, const double *g_host, double *fl_host, double a1, double a2, double a3);
int smear_set_links_hisq(qexhip_ctx *c, const double *g_host);
int smear_hisq_force_host(qexhip_ctx *c, const double *g_host, const double *dfl_host, const double *dll_host, double *f_host);
int smear_fat7_deriv_host(qexhip_ctx *c, const double *g_host, const double *dfl_host, const double coef[5], const double *dll_host,
                          double naik, double *d_host);
void nhyp_state_free(qexhip_ctx *c);
void hisq_state_free(qexhip_ctx *c);
int hisq_prepare(qexhip_ctx *c, const double *g_host, double *fl_host, double *ll_host);
int hisq_closure_force(qexhip_ctx *c, const double *dfl_host, const double *dll_host, double *f_host);
int gauge_deriv_dev(qexhip_ctx *c, const double2 *G, double2 *F, double cplaq, double c2, int kind);
int stag_outer_dev(qexhip_ctx *c, DevField &fx, double2 *F, double se, double so, int accumulate, int hop = 1);
int hisq_fermion_force(qexhip_ctx *c, double *f_host, const double *const *psi, const double *scale, int n);
int force_projtah_dev(qexhip_ctx *c, double2 *F, const double2 *G, int adj);             // F <- TAH(F G^+) (adj: TAH(G F^+)), ghost tiles included
// resident HISQ molecular dynamics (qexhip_md_hisq_*): the state is the HISQ closure's, the two kernels are hisq_md.hip's
int md_hisq_prepare(qexhip_ctx *c, int bcmask, const int ph[4], int set_links);
int md_hisq_check(qexhip_ctx *c, const char *who);                                       // QEXHIP_ERR_STATE before anything is launched
int md_hisq_fforce(qexhip_ctx *c, int n, DevField *const *psi, const double *scale, double t);
int md_hisq_fforce_solve(qexhip_ctx *c, int n, DevField *const *phi, const double *mass, const double *scale, const double *r2req, int maxits,
                         double t, int *iters);
int md_hisq_fforce_rational(qexhip_ctx *c, DevField &phi, double mass, int nterm, const double *alpha, const double *beta, double r2req,
                            int maxits, int sloppy, double t, int *iters);
int md_hisq_force_get(qexhip_ctx *c, double *f_host);
int hisq_outer13_dev(qexhip_ctx *c, int n, DevField *const *xs, const double *scale, double2 *CF, double2 *CL, int accumulate);
int hisq_projtah_kick_dev(qexhip_ctx *c, double2 *F, const double2 *G, double2 *P, double t);
int nhyp_gauge_force(qexhip_ctx *c, double *f_host, double cplaq, double c2, int kind);
int nhyp_fermion_force(qexhip_ctx *c, double *f_host, const double *const *psi, const double *scale, int n, int bcmask, const int ph[4]);
int nhyp_prepare(qexhip_ctx *c, const double *g_host, double a1, double a2, double a3, double *fl_host);
int nhyp_force_host(qexhip_ctx *c, double *f_host, const double *chain_host);
int smear_set_links_nhyp(qexhip_ctx *c, const double *g_host, double a1, double a2, double a3, int bcmask, const int ph[4]);

// ---- gauge.hip ----
int gauge_set(qexhip_ctx *c, const double *g);
int gauge_get(qexhip_ctx *c, double *g);
int gauge_plaq(qexhip_ctx *c, double out[6]);
int gauge_force(qexhip_ctx *c, double *f_host, double cplaq, double c2 = 0.0, int kind = 0);
int gauge_wflow(qexhip_ctx *c, int nsteps, double eps, double cplaq = 1.0, double c2 = 0.0, int kind = 0);
int gauge_flow_obs(qexhip_ctx *c, int loop, double out[3], double *plaq6 = nullptr);
int gauge_action(qexhip_ctx *c, double cplaq, double c2, int kind, double *out);
int gauge_md_update(qexhip_ctx *c, const double *p_host, double t);
int gauge_reunit(qexhip_ctx *c);
int md_begin(qexhip_ctx *c, const double *g, const double *p);
int md_end(qexhip_ctx *c, double *g, double *p);
int md_momentum_norm2(qexhip_ctx *c, double *out);
int md_update_links(qexhip_ctx *c, double t);
int md_gauge_force(qexhip_ctx *c, double cplaq, double c2, int kind);
int md_kick(qexhip_ctx *c, int source, double t);
int md_kick_dev(qexhip_ctx *c, const double2 *F, double t);      // p += t F for a device force field in the links' layout
int md_shift_links(qexhip_ctx *c, int source, double t);
int md_save_links(qexhip_ctx *c);
int md_restore_links(qexhip_ctx *c);
int gauge_wline(qexhip_ctx *c, const int *path, int n, double out[2]);
int gauge_polyakov(qexhip_ctx *c, double out[8]);
int gauge_plaq_s4(qexhip_ctx *c, double out[8]);
void gauge_free(qexhip_ctx *c);
void gauge_release_scratch(qexhip_ctx *c);
const double2 *gauge_links_dev(qexhip_ctx *c);   // resident natural-layout links (nullptr before qexhip_gauge_set)
// host [idx][mu][9] <-> any gauge-shaped device field, through the staging buffer.  The download waits for the stream; the upload does with
// sync (the caller may reuse `host` at once), else `host` must stay untouched until the stream has passed the copy
int gauge_upload_nat(qexhip_ctx *c, double2 *G, const double *host, bool sync = true);
int gauge_download_nat(qexhip_ctx *c, const double2 *G, double *host);
int gauge_field_ghosts(qexhip_ctx *c, double2 *field, int depth);   // refresh the depth-`depth` ghost slices of any gauge-shaped device field
int gauge_ghosts(qexhip_ctx *c, int depth);      // refresh the ghost slices of the resident links to at least `depth` (no-op unless t is sharded)
int read_global(qexhip_ctx *c, double *dev, int n, double *host);   // rank-sum of n device scalars, then read back
// ---- gaugefix.hip (src/gauge/gaugefix.nim) ----
int gfix_set_transform(qexhip_ctx *c, const double *t);
int gfix_get_transform(qexhip_ctx *c, double *t);
int gfix_check_args(qexhip_ctx *c, const char *who, const int *dirs, int ndirs, int need_t);   // QEXHIP_ERR_ARG before anything is launched
int gauge_fix(qexhip_ctx *c, const int *dirs, int ndirs, double gstop, double orf, int maxits, int *iters, double metrics[4],
              double *hist, int histcap);
int gauge_transform(qexhip_ctx *c);
int gauge_link_trace(qexhip_ctx *c, const int *dirs, int ndirs, double *out);
void gfix_state_free(qexhip_ctx *c);
// ---- stout.hip (src/gauge/stoutsmear.nim) ----
int stout_smear(qexhip_ctx *c, const double *g_host, double alpha, double *fl_host);
int stout_prepare(qexhip_ctx *c, const double *g_host, const double *alphas, int nlevels, double *fl_host);
int stout_force(qexhip_ctx *c, double *f_host, const double *chain_host);
int stout_gauge_force(qexhip_ctx *c, double *f_host, double cplaq, double c2, int kind);
int stout_inverse(qexhip_ctx *c, const double *fl_host, double alpha, double rdf2req, int maxits, double *g_host, int *iters, double *rdf2,
                  int *diverging);
void stout_chain_free(qexhip_ctx *c);    // the levels of the chain (qexhip_stout_release)
void stout_state_free(qexhip_ctx *c);    // and the scratch of smear / inverse (qexhip_release_workspace, qexhip_finalize)
// ---- rng.hip (device-side generation) ----
struct qexhip_rng;
int rng_dev_generate(qexhip_ctx *c, qexhip_rng *R, int what, DevField *f, double2 *P);   // what: 0 gaussian vector, 1 u1 vector, 2 randomTAH -> P,
                                                                                         // 3 z4 vector, 4 z2 vector
int md_momenta_dev(qexhip_ctx *c, double2 **M);                                          // resident MD momenta (allocated on demand)
