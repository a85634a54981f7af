// dslash.hip -- one-parity staggered Dslash sweep (kernels K1/K2/K3 of SURVEY.md 2.3).
//
// Restates stagD2 (src/physics/stagD.nim:349-395), stagDP (:200-237) and stagDM (:278-313):
//   out(s) = ca*rin(s) + cb*xs(s) +/- sum_mu [ U_mu(s) in(s+mu) - U_mu(s-mu)^+ in(s-mu) ]
// (+ the 3-hop terms with 16 links, initStagD3T :38-49).  One lane per output site, one
// wavefront per 64-site tile: the wavefront streams its contiguous block of links (72 KiB /
// 144 KiB) with 16-byte loads, neighbour vectors come from the opposite-parity field with
// unit-stride (x), row-stride (y), plane-stride (z) or slice-stride (t) access, all coalesced.
// HBM-bound: 1248 B and 570 flop per site (1-hop; 960 B on the lossless 108-byte links, 898 B on their packed form, 834 B on the orthogonal form, link_residual.h), no MFMA on purpose.
//
// Two kernels with disjoint roles (round 6; rounds 4-5 had one kernel with seven template parameters) around one dslash_body; the link
// fetch is LinkCursor's (dslash_core.h), the workgroup -> site mapping sweep_site's (site_index.h), shared with the batched and fp32 sweeps:
//   k_dslash<NDIR, HALO, INIT, DOT, RECON>     every sweep that reads its t-neighbours from the FIELD: the whole lattice on one GPU, and on a
//                                              t-sharded slab the launches around an exchange into the ghost tiles (RCCL, or the peer
//                                              transport's unpacking exchange): one launch behind it, or interior | both faces
//   k_dslash_fused<NDIR, INIT, DOT, RECON>     the overlapped sweep of a t-sharded slab on the peer transport as ONE launch on ONE stream
//                                              (shifts.nim:67-94,254-285: local terms while the faces travel, boundary terms when they
//                                              are in): push | interior | boundary | cleanup workgroups, fused_sweep.h
#include "qexhip_internal.h"
#include "site_index.h"
#include "reduce.h"
#include "fused_sweep.h"
#include <hip/hip_ext.h>
#include <cstring>
#include <algorithm>
#include <chrono>

static double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct DslashArgs {
  Geom g;
  const double2 *W;      // links of the output parity (RECON 1, 2: rows 0,1 (+ det) only, [tile][dir][6|7][64]; 3, 4, 5: link_residual.h rows)
  const unsigned long long *S;   // RECON 1: sign masks [tile][dir], bit = lane; 3, 4, 5: [tile][dir][sign, escape] (S[-2]: this parity's W)
  const double2 *in;     // hop source (opposite parity half)
  double2 *out;          // output parity half
  const double2 *rin;    // a-term
  const double2 *xs;     // b-term / dot partner
  double ca, cb;
  double sgn;            // +1 (stagDP / stagD2) or -1 (stagDM)
  double post;           // final scale, the `r := (0.5*sc)*r` of stagD (stagD.nim:409)
  int parity;
  SweepRanges r;         // [c0,c1), and [d0,d1) for workgroups >= nb1 (both t-faces in one launch; fused: interior, low face)
  const double2 *gh_hi, *gh_lo;   // fused: where ghost POSITIONS are read from: the transport's receive arena (pre-offset: gh[vec_off(pos, k)])
  double *partials;
  const int *done;
  int swz;               // number of workgroups if XCD swizzle is on, else 0
  int ntstore;           // 1: non-temporal stores of the output
  FusedSweep fs;         // fused only: third range, push, ghost words, bookkeeping
};

#include "dslash_core.h"

// The fused sweep's workgroup roles (push | interior | boundary | cleanup) are fused_sweep.h's, the site ranges site_index.h's
// (sweep_site), the link fetch dslash_core.h's (LinkCursor); this is only the per-site arithmetic.
template <int NDIR, bool HALO, bool INIT, bool DOT, int RECON, bool FUSED>
__device__ __forceinline__ void dslash_body(const DslashArgs &A) {
  const bool skip = A.done && *A.done;
  // a finished solve turns the rest of its chunk into no-ops -- except that a fused launch still returns the credits it owes
  if (skip && !FUSED) return;
  if (FUSED && fused_push(A.fs, skip)) return;
  FusedRole R;
  R.bid = blockIdx.x; R.cleanup = false; R.bnd = false; R.parked = false;
  if (FUSED) fused_enter(A.fs, A.r.nb1, R);
  const bool cleanup = FUSED && R.cleanup;
  for (;;) {                               // one pass; a cleanup workgroup takes every fz.ncl-th parked block
    int lb = R.bid;                        // logical workgroup: [0, nb1) first range, [nb1, nb2) second, [nb2, ..) third
    if (FUSED && !fused_next_block(A.fs, R, lb)) break;
    const bool bnd = FUSED && R.bnd;
    if (A.swz && !bnd) {
      // XCD-aware remap: workgroups are dealt round-robin over the 8 XCDs; give every XCD a
      // contiguous run of tiles (= a contiguous t-range) so that y/z/t neighbours share its L2.
      int per = A.swz >> 3;
      lb = (lb & 7) * per + (lb >> 3);
    }
    int c, clim;
    if (FUSED) c = fused_site(A.fs, R, lb, A.r, clim);
    else sweep_site(A.r, lb, c, clim);
    double dotv = 0;
    const bool active = c < clim && !skip;
    const Geom &g = A.g;
    const SiteXYZT s = site_coord(g, c, A.parity);     // (arithmetic only: harmless beyond clim)
    // a tile lies in one t-slice (64 | F on sharded handles): t is wavefront-uniform
    const int tu = FUSED ? __builtin_amdgcn_readfirstlane(s.t) : 0;
    double2 acc[3];
    double2 xsv[3];
    const LinkCursor<NDIR, RECON> L(A.W, A.S, c);
    // fused: hops that leave the slab read the neighbours' faces where the neighbours WROTE them -- the transport's receive arena --
    // instead of the field's ghost tiles: which base a t-hop reads from is wavefront-uniform, four scalar selects, nothing per lane
    const double2 *in_f1 = A.in, *in_b1 = A.in, *in_f3 = A.in, *in_b3 = A.in;
    if (FUSED) {
      in_f1 = tu + 1 >= g.X[3] ? A.gh_hi : A.in;
      in_b1 = tu - 1 < 0 ? A.gh_lo : A.in;
      in_f3 = tu + 3 >= g.X[3] ? A.gh_hi : A.in;
      in_b3 = tu - 3 < 0 ? A.gh_lo : A.in;
    }
    // One pair = the forward and the backward hop of one direction (fat links: pairs 0..3, 3-hop links: pairs 4..7);
    // do_f / do_b: which of the two this call takes (literally true on the fast path).
    auto pair = [&](const int pr, const bool do_f, const bool do_b) __attribute__((always_inline)) {
      const int mu = pr & 3;
      const int hop = pr >= 4 ? 3 : 1;
      const int pf = nbr_pos<HALO>(g, c, s, mu, hop);
      const int pb = nbr_pos<HALO>(g, c, s, mu, -hop);
      double2 U[9], W[9], vf[3], vb[3];
      // The loads of L.fetch(pr, do_f, do_b, U, W), spelled out: through the call the compiler orders the loop differently (every load
      // first, the rebuild behind the neighbour loads) and the RECON 1 / 2 instantiations of k_dslash move by -14 .. +6 VGPRs
      // (profiles/sweep_refactor_resources.txt).  The rebuild behind them is the cursor's.
      constexpr int NLOAD = LinkFormat<RECON>::NLOAD, LROW = LinkFormat<RECON>::LROW;
      const double2 *wp = L.w + (size_t)pr * (2 * LROW);
      if (do_f) {
#pragma unroll
        for (int k = 0; k < NLOAD; k++) {
          d2v t = __builtin_nontemporal_load((const d2v *)&wp[k * 64]);
          U[k] = make_double2(t.x, t.y);
        }
      }
      if (do_b) {
#pragma unroll
        for (int k = 0; k < NLOAD; k++) {
          d2v t = __builtin_nontemporal_load((const d2v *)&wp[LROW + k * 64]);
          W[k] = make_double2(t.x, t.y);
        }
      }
      L.rebuild(pr, do_f, do_b, wp, U, W);
      const double2 *srcf = (FUSED && mu == 3) ? (hop == 3 ? in_f3 : in_f1) : A.in;
      const double2 *srcb = (FUSED && mu == 3) ? (hop == 3 ? in_b3 : in_b1) : A.in;
      if (do_f) {
#pragma unroll
        for (int k = 0; k < 3; k++) vf[k] = srcf[vec_off(pf, k)];
      }
      if (do_b) {
#pragma unroll
        for (int k = 0; k < 3; k++) vb[k] = srcb[vec_off(pb, k)];
      }
      // forward hops add, backward hops subtract (compile-time sign: no per-direction multiply).
      // stagDM's overall minus sign is carried by the initial value and the final scale: negation is
      // exact, so init - sum == -((-init) + sum) bit for bit.
      if (do_f) mv3<false>(acc, U, vf);
      if (do_b) mv3<true>(acc, W, vb);
    };
    // the outermost slices of the fused sweep (wavefront-uniform branch): `crossing` false takes every hop but the t-hops that
    // leave the slab -- the spatial pairs in the fast loop's form, then the t pairs hop by hop --, true exactly those t-hops.
    auto edge_pairs = [&](const bool crossing) __attribute__((always_inline)) {
      if (!crossing) {
        constexpr int NSP = NDIR / 2 - NDIR / 8;       // spatial pairs: 0,1,2 (and 4,5,6)
        constexpr int UNS = NDIR == 8 ? 1 : 2;      // (8 links: rolled -- unrolled x3 the function takes 255 VGPRs, one workgroup per SIMD pair)
#pragma unroll UNS
        for (int q = 0; q < NSP; q++) pair(q + q / 3, true, true);
      }
#pragma unroll 1
      for (int pr = 3; pr < NDIR / 2; pr += 4) {
        const int hop = pr >= 4 ? 3 : 1;
        const bool xf = tu + hop >= g.X[3], xb = tu - hop < 0;
        pair(pr, crossing ? xf : !xf, crossing ? xb : !xb);
      }
    };
    const bool edge = FUSED && bnd;          // (every site of a boundary block has a hop that leaves the slab)
    if (active) {
      if ((INIT && !cleanup) || DOT) {
#pragma unroll
        for (int k = 0; k < 3; k++) xsv[k] = A.xs[vec_off(c, k)];
      }
      if (FUSED && cleanup) {
#pragma unroll
        for (int k = 0; k < 3; k++) acc[k] = A.out[vec_off(c, k)];          // the raw accumulator its boundary workgroup parked here
      } else if (INIT) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
          acc[k].x = (A.sgn * A.cb) * xsv[k].x;
          acc[k].y = (A.sgn * A.cb) * xsv[k].y;
        }
        if (A.ca != 0.0) {
#pragma unroll
          for (int k = 0; k < 3; k++) {
            double2 r = A.rin[vec_off(c, k)];
            acc[k].x += (A.sgn * A.ca) * r.x;
            acc[k].y += (A.sgn * A.ca) * r.y;
          }
        }
      } else {
#pragma unroll
        for (int k = 0; k < 3; k++) acc[k] = make_double2(0.0, 0.0);
      }
      // How far the loop is unrolled decides how many link loads a wave keeps in flight.  Measured inside CG on 32^4
      // (scratch A/B builds, 2 rounds):
      //   1-hop: rolled 117 us, x2 120 us, fully unrolled 113.6 us (all 96 loads in flight, 256 VGPRs)
      //   Naik : rolled 215 us, x2 210 us, x4 222 us; FULLY unrolled hipcc hoists all 192 loads and
      //          spills to scratch (290-330 us) -- never unroll the 16-link loop completely.
      // mu/hop are wave-uniform, so the neighbour arithmetic of the rolled loop branches on scalars.
      // compressed 8-link kernel (rows 0,1 + sign, 864 B/site): rolled 80.2 us, x2 81.9, x4 83.5 (32^4, in CG)
      // lossless 8-link kernel (108 B/link, 960 B/site): x2 83.8 us, rolled 88.5 (32^4, bench.py); the fused sweep stays rolled
      // packed lossless 8-link kernel (100 B/link, 898 B/site): rolled 77.2 + 80.4 us per sweep pair (134-150 VGPRs, 3 waves per SIMD),
      //   x2 76.5 + 80.1 us (217-231 VGPRs, 2 waves); 0.2126-0.2140 against 0.2117-0.2126 ms per iteration over six alternating bench.py
      //   runs, but one x2 run at 0.2212: rolled, the steadier one (profiles/packed_bench_32x4.log)
      // orthogonal lossless 8-link kernel (92 B/link, 834 B/site): rolled 74.2 + 74.2 us per sweep pair (135-159 VGPRs, 3 waves per SIMD);
      //   x2 239-254 VGPRs, 2 waves, 0.2089-0.2178 against 0.2027-0.2096 ms per iteration over six alternating bench.py runs, slower
      //   in every pair: rolled (profiles/ortho_bench_32x4.log)
      constexpr int UNR = (NDIR == 8) ? (RECON >= 4 ? 1 : RECON == 3 ? (FUSED ? 1 : 2) : (RECON ? 1 : 4)) : 2;
      if (!edge) {
        // every hop of the site: the loop of the one-launch kernel
#pragma unroll UNR
        for (int pr = 0; pr < NDIR / 2; pr++) pair(pr, true, true);
      } else if (!cleanup) {
        edge_pairs(false);
      }
    }
    if (edge && !skip) {
      fused_wait_faces(A.fs, R);
      if (active && !R.parked) edge_pairs(true);
    }
    const bool parked = FUSED && R.parked;
    if (active) {
      if (parked) {
        // the raw accumulator waits in `out` for a cleanup workgroup (which re-reads it soon: plain stores)
#pragma unroll
        for (int k = 0; k < 3; k++) A.out[vec_off(c, k)] = acc[k];
      } else {
#pragma unroll
        for (int k = 0; k < 3; k++) {
          acc[k].x *= (A.sgn * A.post); acc[k].y *= (A.sgn * A.post);
          if (A.ntstore) {
            d2v t; t.x = acc[k].x; t.y = acc[k].y;
            __builtin_nontemporal_store(t, (d2v *)&A.out[vec_off(c, k)]);
          } else {
            A.out[vec_off(c, k)] = acc[k];
          }
        }
        if (DOT) {
#pragma unroll
          for (int k = 0; k < 3; k++) dotv = fma(xsv[k].x, acc[k].x, fma(xsv[k].y, acc[k].y, dotv));
        }
      }
    }
    if (DOT && !skip && !parked) {
      // (RECON 3, 4, 5: the slot of the logical block, which the XCD swizzle leaves where the unswizzled launch puts it -- the partials are
      // summed in slot order, and this format computes the 18-real operator's bits, the residual history included)
      const int pidx = !FUSED ? (RECON >= 3 ? lb : (int)blockIdx.x) : fused_partial_slot(A.fs, R, lb);
      double r = block_sum_256(dotv);
      if (threadIdx.x == 0) A.partials[pidx] = r;
    }
    if (!cleanup) break;
  }
  if (FUSED) fused_finish(A.fs, R);
}

template <int NDIR, bool HALO, bool INIT, bool DOT, int RECON>
__global__ void __launch_bounds__(256) k_dslash(DslashArgs A) { dslash_body<NDIR, HALO, INIT, DOT, RECON, false>(A); }
template <int NDIR, bool INIT, bool DOT, int RECON>
__global__ void __launch_bounds__(256) k_dslash_fused(DslashArgs A) { dslash_body<NDIR, true, INIT, DOT, RECON, true>(A); }

// Launch with the HIP extension that attaches a start and a stop event to the kernel itself
// (hipExtLaunchKernelGGL): the pair brackets exactly the kernel's execution, like the duration
// rocprofv3 reports, instead of the record-to-record interval of two stream markers.
template <class K>
static void launch_timed(qexhip_ctx *c, const char *tname, K kernel, dim3 grid, dim3 block, DslashArgs &A, hipStream_t st) {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (timer_event_pair(c, tname, &e0, &e1)) hipExtLaunchKernelGGL(kernel, grid, block, 0, st, e0, e1, 0, A);
  else hipLaunchKernelGGL(kernel, grid, block, 0, st, A);
}

// ranges [c0,c1) (+ [d0,d1) behind it); fused_grid > 0: the fused launch of that many workgroups that fused_sweep_setup prepared in A.fs
template <int NDIR, bool HALO>
static int launch(qexhip_ctx *c, DslashArgs &A, int c0, int c1, bool init, bool dot, int part_off,
                  int d0 = 0, int d1 = 0, const char *tname = "dslash", hipStream_t st = nullptr, int fused_grid = 0) {
  if (!st) st = c->stream;
  const bool fused = fused_grid > 0;
  const int nb = sweep_ranges(A.r, c0, c1, d0, d1);
  if (!nb) return 0;
  // XCD swizzle: measured on for compressed links, off for 18-real links (profiles/r01_tune_dslash.log); output stores are
  // non-temporal (the result is read by the NEXT kernel, after 0.6 GB of links went through the caches).  The lossless format
  // takes it in the one-launch kernel only: the fused kernel's dot partials go by dispatch slot, which the remap would reorder
  const int nsw = fused ? A.r.nb1 : nb;          // (the fused launch remaps its interior workgroups only)
  A.swz = ((c->recon != 0 || (c->lres && !fused)) && nsw >= 64 && (nsw & 7) == 0) ? nsw : 0;
  A.ntstore = 1;
  double *psave = A.partials;
  A.partials = psave ? psave + part_off : nullptr;
  dim3 grid(fused ? fused_grid : nb), block(256);
#define QX_LAUNCH(R) \
  do { \
    if (HALO && fused) { \
      if (init && dot) launch_timed(c, tname, k_dslash_fused<NDIR, true, true, R>, grid, block, A, st); \
      else if (init) launch_timed(c, tname, k_dslash_fused<NDIR, true, false, R>, grid, block, A, st); \
      else if (dot) launch_timed(c, tname, k_dslash_fused<NDIR, false, true, R>, grid, block, A, st); \
      else launch_timed(c, tname, k_dslash_fused<NDIR, false, false, R>, grid, block, A, st); \
    } else if (init && dot) launch_timed(c, tname, k_dslash<NDIR, HALO, true, true, R>, grid, block, A, st); \
    else if (init) launch_timed(c, tname, k_dslash<NDIR, HALO, true, false, R>, grid, block, A, st); \
    else if (dot) launch_timed(c, tname, k_dslash<NDIR, HALO, false, true, R>, grid, block, A, st); \
    else launch_timed(c, tname, k_dslash<NDIR, HALO, false, false, R>, grid, block, A, st); \
  } while (0)
  const int recon = stag_link_storage(c).recon;
  if (recon == 1) QX_LAUNCH(1);
  else if (recon == 2) QX_LAUNCH(2);
  else if constexpr (NDIR == 8) {              // (the lossless forms are 8-link operators' only)
    if (recon == 5) QX_LAUNCH(5);
    else if (recon == 4) QX_LAUNCH(4);
    else if (recon == 3) QX_LAUNCH(3);
    else QX_LAUNCH(0);
  } else QX_LAUNCH(0);
#undef QX_LAUNCH
  A.partials = psave;
  HIPCHK(hipGetLastError());
  return 0;
}

// How a sweep over a t-sharded field is laid out: boundary sites [0, lo_end) and [hi_beg, Vh), interior between them, and
// whether the face exchange overlaps the interior at all.
// Overlap only when the interior is long enough to hide the exchange (measured on one MI355X with a one-rank communicator:
// the two cross-stream dependencies cost ~20 us per sweep; an interior of 128k sites runs ~30 us) and a face is big enough
// for its transfer to cost more than the split does: in the one-rank rehearsal (no transport time at all) the interior /
// boundary split with its two cross-stream events costs ~15 us per sweep (48^3 x 12: 417 vs 388 us per iteration; 32^3 x 16:
// 253 vs 218); a 48^3 face is 2.65 MB per direction (tens of microseconds on an xGMI link), a 32^3 face 0.79 MB.
void sweep_plan(const qexhip_ctx *c, int *lo_end_out, int *hi_beg_out, int *overlap_out) {
  const Geom &g = c->g;
  int lo_end = g.depth * g.F; if (lo_end > g.Vh) lo_end = g.Vh;
  int hi_beg = g.Vh - g.depth * g.F; if (hi_beg < lo_end) hi_beg = lo_end;
  const size_t face_bytes = (size_t)g.depth * g.F * 48;
  *lo_end_out = lo_end; *hi_beg_out = hi_beg;
  const int tuned = c->overlap_auto[c->ndir == 16];
  *overlap_out = !g.halo || hi_beg <= lo_end ? 0
                 : (c->opt_overlap >= 0 ? (c->opt_overlap != 0)
                    : (tuned >= 0 ? tuned : ((hi_beg - lo_end) >= 131072 && face_bytes >= ((size_t)1 << 20))));
}

// What an overlapped sweep runs as: 2 = the fused launch (peer transport carrying the faces: the only transport a kernel of ours can push
// through), 0 = split by sites.  Option hop_split pins it; at -1 it is what set_links measured, fused until then.
int sweep_form(const qexhip_ctx *c, int overlap) {
  if (!overlap || !peer_faces(c)) return 0;
  if (c->opt_hop_split >= 0) return c->opt_hop_split ? 2 : 0;
  const int m = c->form_auto[c->ndir == 16];
  return m >= 0 ? m : 2;
}

// One face exchange of this operator in microseconds: measured at set_links where a communicator exists (sweep_autotune), else -- and
// in rehearsals that emulate a link -- the estimate 3 us + face bytes at 45 GB/s per xGMI direction (option emu_link_gbs replaces the rate).
static double exchange_estimate_us(const qexhip_ctx *c) {
  const double meas = c->xchg_us[c->ndir == 16];
  if (meas > 0) return meas;
  const double link = (c->emu_link_gbs > 0 ? c->emu_link_gbs : 45.0) * 1e3;      // bytes per us
  return 3.0 + (double)c->g.depth * c->g.F * 48.0 / link;
}
// Where the fused sweep's boundary workgroups go in the dispatch order.  They should start about when the faces arrive: exchange time
// over estimated interior time (its bytes at 5.5 TB/s); never before 65 % (their rolled edge loops should not be the tail either),
// last of all when the exchange is the longer of the two.  A wrong guess costs little since round 6 (a boundary workgroup waits
// about one exchange time, then parks), but the waiting ones do hold slots meanwhile.
// nrhs > 1 (the lock-step batch): the links once, the vectors and the faces nrhs times.
double sweep_push_fraction(const qexhip_ctx *c, int interior_sites, int nrhs) {
  const double bsite = c->ndir * (double)stag_link_storage(c).bytes + 120.0 * nrhs;
  const double t_int = (double)interior_sites * bsite / 5.5e6;       // us
  return t_int > 0 ? std::min(1.0, std::max(0.65, nrhs * exchange_estimate_us(c) / t_int)) : 1.0;
}

// FusedCtl of the next fused launch: five words on lines of their own + the parked-block list
static int sweep_fused_ctl(qexhip_ctx *c, int nbnd, FusedCtl *F, int nrhs) {
  if (c->fz_cap < nbnd) {
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->fz_buf) HIPCHK(hipFree(c->fz_buf));
    c->fz_buf = nullptr; c->fz_cap = 0;
    const int cap = std::max(2 * nbnd, 4096);
    HIPCHK(hipMalloc((void **)&c->fz_buf, (size_t)(256 + cap) * sizeof(unsigned int)));
    HIPCHK(hipMemsetAsync(c->fz_buf, 0, (size_t)(256 + cap) * sizeof(unsigned int), c->stream));     // (ordered before the launch that uses it)
    c->fz_cap = cap;
  }
  F->dec = c->fz_buf; F->ndef = c->fz_buf + 32; F->cl_done = c->fz_buf + 64; F->late = c->fz_buf + 96;
  F->list = c->fz_buf + 256;
  // the cleanup workgroups hold their slots through the LONG wait when the faces are late: few, so that a neighbour that shares the chip
  // always finds room; enough to take a whole face's parked blocks in ~100 us when it comes to that.  Measured (48^3 x 12 / 32^3 x 4
  // slabs, profiles/r06_fused_ab.log): 8 | 16 | 32 | 64 of them cost 91 | 92.5 | 95 | 97.6 us per iteration on the thin slab's normal
  // path (they poll while the whole launch is resident) and 663 | 513 | 450 | 438 us with EVERY block parked on the 48^3 one:
  // one per eight boundary workgroups (a parked face then costs each of them the same ~8-14 blocks whatever the face), at most 32
  F->ncl = std::max(std::min(nbnd, 4), std::min(nbnd / 8, 32));       // one per eight boundary workgroups, 4 .. 32
  const double tick_per_us = (double)c->dj.ticks / (c->dj.timeout_s * 1e6);
  if (c->opt_fused_spin_us == -2) F->spin_ticks = -1;
  else {
    const double us = c->opt_fused_spin_us >= 0 ? (double)c->opt_fused_spin_us : std::max(25.0, nrhs * exchange_estimate_us(c));
    F->spin_ticks = (long long)(us * tick_per_us);
  }
  return 0;
}

int fused_sweep_setup(qexhip_ctx *c, int nrhs, DevField *const *f, int parity, int lo_end, int hi_beg, FusedSweep *F,
                      const double2 **gh_hi, const double2 **gh_lo, int *grid, int *nparts) {
  const int nb_int = (hi_beg - lo_end + 255) / 256, nb_lo = (lo_end + 255) / 256, nb_hi = (c->g.Vh - hi_beg + 255) / 256;
  CHK(comm_halo_push_only_multi(c, nrhs, f, parity, gh_hi, gh_lo, &F->push));
  CHK(peer_ghost_args(c, &F->pg));
  CHK(sweep_fused_ctl(c, nb_lo + nb_hi, &F->fz, nrhs));
  F->e0 = hi_beg; F->e1 = c->g.Vh; F->nb2 = nb_int + nb_lo;
  F->nbA = (int)(sweep_push_fraction(c, hi_beg - lo_end, nrhs) * nb_int);
  *grid = F->push.nblocks + nb_int + nb_lo + nb_hi + F->fz.ncl;
  *nparts = nb_int + nb_lo + nb_hi;
  return 0;
}

// The static rule in sweep_plan was set from one-rank rehearsals, where an exchange costs one kernel and no transport.  With a real
// communicator (nranks > 1) the decisions are MEASURED once per operator shape, right after the links are in place: the face
// exchange alone (what the fused sweep's placement and its short wait go by), then a few pairs of sweeps in every form -- exchange
// first, overlapped and split by sites, fused -- on scratch fields; the slower rank's time decides (max-all-reduce, so every rank
// takes the same branch).  Collective over the communicator, like set_links itself (ghost links).  Options overlap = 0 / 1 and
// hop_split = 0 / 2 switch the respective measurement off and pin form and bits; overlap = -2 asks for it on one rank too (test hook).
int sweep_autotune(qexhip_ctx *c) {
  const Geom &g = c->g;
  const int slot = c->ndir == 16;
  if (!g.halo || !c->W) return 0;
  const bool multi = c->nranks > 1 && comm_ready(c);
  if (multi) {
    // The forms select the stream (and, on RCCL, the communicator) an exchange is posted on: ranks that disagreed would never match.
    // set_links is collective, so this is the place to find out.
    const double code = 64.0 * c->opt_overlap + 1024.0 * (c->opt_hop_split + 1) + 65536.0 * (c->opt_fused_spin_us + 2);
    double v[2] = {code, -code};
    CHK(comm_allreduce_max(c, v, 2));
    if (v[0] != -v[1]) {
      qexhip_set_error("options overlap (QEXHIP_OVERLAP) / hop_split / fused_spin_us differ between the ranks (65536 (fused_spin_us + 2) + 1024 (hop_split + 1) "
                       "+ 64 overlap = %g .. %g): they must be the same everywhere", -v[1], v[0]);
      return -3;
    }
  }
  if (c->form_auto[slot] >= 0) return 0;           // measured already for this operator shape
  const bool measure = c->opt_overlap == -2 || multi;
  if (!measure) return 0;
  int lo_end, hi_beg, dummy;
  sweep_plan(c, &lo_end, &hi_beg, &dummy);
  if (hi_beg <= lo_end) { c->overlap_auto[slot] = 0; c->form_auto[slot] = 0; return 0; }        // no interior to overlap with
  DevField f[3];
  int rc = 0;
  for (int k = 0; k < 3 && !rc; k++) rc = field_alloc(c, f[k]);
  const int saved = c->opt_overlap, saved_form = c->opt_hop_split, saved_timers = c->timers_on;
  c->timers_on = 0;
  // (1) the exchange alone, on the compute stream: 2 to warm up (arena growth is collective and synchronous), 8 timed
  double tx = 0;
  for (int k = 0; k < 10 && !rc; k++) {
    if (k == 2) { rc = hipStreamSynchronize(c->stream) != hipSuccess ? -2 : 0; tx = -now_us(); }
    if (!rc) rc = comm_halo_exchange(c, f[0], 0, 0);
  }
  if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = -2;
  tx = (tx + now_us()) / 8.0;
  if (!rc && multi) {
    double v[2] = {tx, 0};
    rc = comm_allreduce_max(c, v, 1);
    tx = v[0];
  }
  if (!rc) c->xchg_us[slot] = tx;
  // (2) pairs of sweeps a -> b -> c (what the normal operator runs) in the forms this context can take
  const bool try_fused = peer_faces(c) && (c->opt_hop_split < 0 || c->opt_hop_split == 2);
  const bool try_sites = !(peer_faces(c) && c->opt_hop_split == 2);
  double t[3] = {0, 0, 0};
  for (int mode = 0; mode < 3 && !rc; mode++) {
    if ((mode == 1 && !try_sites) || (mode == 2 && !try_fused)) continue;
    if ((mode && saved == 0) || (!mode && saved == 1)) continue;           // overlap pinned: only the forms it leaves
    c->opt_overlap = mode ? 1 : 0;
    c->opt_hop_split = mode == 2 ? 2 : 0;
    for (int k = 0; k < 6 && !rc; k++) {
      if (k == 1) { rc = hipStreamSynchronize(c->stream) != hipSuccess ? -2 : 0; t[mode] = -now_us(); }
      DslashOpts o1, o2;
      DevField &in0 = f[(k & 1) ? 2 : 0], &out2 = f[(k & 1) ? 0 : 2];
      if (!rc) rc = dslash_sweep(c, f[1], in0, 1, o1);
      if (!rc) rc = dslash_sweep(c, out2, f[1], 0, o2);
    }
    if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = -2;
    t[mode] += now_us();
  }
  c->opt_overlap = saved;
  c->opt_hop_split = saved_form;
  c->timers_on = saved_timers;
  for (int k = 0; k < 3; k++) if (f[k].d) (void)hipFree(f[k].d);
  // every rank reaches the collective, a failed one with a sentinel, so that all fail together instead of one hanging the others
  double v[4] = {t[0], t[1], t[2], rc ? 1.0 : 0.0};
  if (multi) {
    const int e = comm_allreduce_max(c, v, 4);
    if (e && !rc) rc = e;
  }
  if (rc) return rc;
  if (v[3] != 0.0) { qexhip_set_error("sweep_autotune: another rank failed while measuring"); return -4; }
  // The fused form unless the split by sites is clearly (> 3 %) faster; overlap at all only on a clear win (> 5 %) over exchange-first:
  // the forms group the dot partials differently (and the fused one sums a boundary site's local hops first), so a decision that flips
  // between runs on timing noise would cost run-to-run bit-reproducibility of the residual history for nothing.
  const bool have1 = v[1] > 0, have2 = v[2] > 0;
  const int form = have2 && !(have1 && v[1] < 0.97 * v[2]) ? 2 : 0;
  const double best = form == 2 ? v[2] : v[1];
  c->form_auto[slot] = form;
  if (saved < 0) c->overlap_auto[slot] = (best > 0 && v[0] > 0 && best < 0.95 * v[0]) ? 1 : 0;
  for (int k = 0; k < 3; k++) c->overlap_tune_us[slot][k] = v[k] / 10.0;
  return 0;
}

// The links of output parity `parity` as a sweep kernel takes them: W = the parity's first (tile, direction) row in the format
// set_links chose (rows 0,1 (+ det) in Wc with recon 1 / 2; the lossless rows where `lossless` -- c->lres for the single-system
// sweep, whose kernel reads them; false for the batch, which reads the 18 reals beside them; else the 18 reals), S = its masks
void stag_link_bases(const qexhip_ctx *c, int parity, bool lossless, const double2 **W, const unsigned long long **S) {
  const size_t rows = (size_t)parity * c->g.ntile * c->ndir;         // (tile, direction) rows before this parity
  const LinkStorage ls = stag_link_storage(c, lossless);
  *W = (ls.recon ? c->Wc : c->W) + rows * ls.lrow;
  if (ls.recon >= 3) *S = c->Wm + (size_t)parity * (2 + c->g.ntile * c->ndir * 2) + 2;
  else *S = ls.recon ? c->Ws + rows : nullptr;
}

// The one answer to "which kernel, which stride, how many bytes": c->recon (formats 1, 2) or the lossless form c->lres
LinkStorage stag_link_storage(const qexhip_ctx *c, bool lossless) {
  static constexpr int lrow[6] = {LinkFormat<0>::LROW, LinkFormat<1>::LROW, LinkFormat<2>::LROW, LinkFormat<3>::LROW, LinkFormat<4>::LROW, LinkFormat<5>::LROW};
  const int recon = c->recon ? c->recon : (lossless && c->lres ? lossless_recon(c->lres) : 0);
  return {recon, lrow[recon], lrow[recon] * (int)sizeof(double2) / 64};
}

int dslash_sweep(qexhip_ctx *c, DevField &out, DevField &in, int parity, const DslashOpts &o) {
  const Geom &g = c->g;
  if (!c->W) { qexhip_set_error("staggered links not set (qexhip_stag_set_links)"); return -3; }
  DslashArgs A;
  memset(&A, 0, sizeof A);
  A.g = g;
  stag_link_bases(c, parity, c->lres != 0, &A.W, &A.S);
  A.in = in.par(1 - parity);
  A.out = out.par(parity);
  A.rin = o.rin ? o.rin->par(parity) : nullptr;
  A.xs = o.xs ? o.xs->par(parity) : nullptr;
  A.ca = o.ca; A.cb = o.cb;
  A.sgn = o.neg ? -1.0 : 1.0;
  A.post = o.post;
  A.parity = parity;
  A.partials = c->partials;
  A.done = o.done;
  const bool init = (o.ca != 0.0 || o.cb != 0.0);
  if ((init || o.dot) && !A.xs) { qexhip_set_error("dslash_sweep: b-term/dot needs xs"); return -1; }
  if (o.ca != 0.0 && !A.rin) { qexhip_set_error("dslash_sweep: a-term needs rin"); return -1; }
  int nparts = 0;
  const double2 *faces_on_cstream = nullptr;
  if (!g.halo) {
    if (c->ndir == 8) CHK((launch<8, false>(c, A, 0, g.Vh, init, o.dot, 0)));
    else CHK((launch<16, false>(c, A, 0, g.Vh, init, o.dot, 0)));
    nparts = (g.Vh + 255) / 256;
  } else {
    int lo_end, hi_beg, overlap;
    sweep_plan(c, &lo_end, &hi_beg, &overlap);
    CHK(devjoin_flush(c));
    const int nb_int = (hi_beg - lo_end + 255) / 256, nb_lo = (lo_end + 255) / 256, nb_hi = (g.Vh - hi_beg + 255) / 256;
    if (sweep_form(c, overlap) == 2) {
      // The fused sweep: the exchange is INSIDE the launch -- its first workgroups push the faces, its boundary workgroups poll the inbound
      // data words, park when those are late, its last workgroups clean up -- and neither the comm stream nor an event is involved.
      DevField *inp = &in;
      int grid;
      CHK(fused_sweep_setup(c, 1, &inp, 1 - parity, lo_end, hi_beg, &A.fs, &A.gh_hi, &A.gh_lo, &grid, &nparts));
      if (c->ndir == 8) CHK((launch<8, true>(c, A, lo_end, hi_beg, init, o.dot, 0, 0, lo_end, "dslash", nullptr, grid)));
      else CHK((launch<16, true>(c, A, lo_end, hi_beg, init, o.dot, 0, 0, lo_end, "dslash", nullptr, grid)));
    } else if (!overlap) {
      // the exchange is ordered before us on the compute stream: one launch over all sites
      // (small local volumes are launch-latency-bound; this drops two launches per CG iteration)
      CHK(comm_halo_exchange(c, in, 1 - parity, 0));
      if (c->ndir == 8) CHK((launch<8, true>(c, A, 0, g.Vh, init, o.dot, 0)));
      else CHK((launch<16, true>(c, A, 0, g.Vh, init, o.dot, 0)));
      nparts = (g.Vh + 255) / 256;
    } else {
      // Split by sites: the face exchange on the comm stream (behind ev_ready: the producer of `in`), the interior launch on the
      // compute stream meanwhile, both t-faces in ONE launch on the COMM stream right behind the exchange -- it needs the ghost zones
      // and nothing of the interior launch, so it starts the moment the faces have arrived and runs beside the interior's tail
      // (round 4: 1-6 % of an iteration on thin slabs).  The join back is a device-side counter on BOTH transports since round 6 (a
      // one-lane signal kernel behind the boundary launch, a one-wave wait on the compute stream -- or, with o.defer_join, in the
      // prologue of the mailbox all-reduce that comes next): the runtime's cross-queue event dependency was ~28 us of dead time per
      // sweep (profiles/r05_timeline_*.txt).
      // Second sweep of a pair (op_xx) behind a first one of this form: the faces it sends ARE the output of the first sweep's boundary
      // launch, the comm stream's own previous kernel -- the exchange is posted at once (~28 us earlier: it no longer waits for the first
      // sweep's interior launch and the join), and only the boundary launch, which also reads the slices next to the faces, waits for
      // ev_ready.  (Round 5's "chained pair" did this and more -- it also dropped the join by narrowing the second interior -- and never
      // won; this keeps every launch as it is.)
      const bool early = o.pair2 && c->bnd_out_on_cstream == in.par(1 - parity);
      HIPCHK(hipEventRecord(c->ev_ready, c->stream));
      CHK(comm_halo_exchange(c, in, 1 - parity, 1, !early));
      if (early) HIPCHK(hipStreamWaitEvent(c->cstream, c->ev_ready, 0));
      if (c->ndir == 8) CHK((launch<8, true>(c, A, lo_end, hi_beg, init, o.dot, 0)));
      else CHK((launch<16, true>(c, A, lo_end, hi_beg, init, o.dot, 0)));
      if (c->ndir == 8) CHK((launch<8, true>(c, A, 0, lo_end, init, o.dot, nb_int, hi_beg, g.Vh, "dslash_bnd", c->cstream)));
      else CHK((launch<16, true>(c, A, 0, lo_end, init, o.dot, nb_int, hi_beg, g.Vh, "dslash_bnd", c->cstream)));
      CHK(devjoin_signal(c, c->cstream));
      if (o.defer_join && c->peer) CHK(devjoin_defer(c));
      else CHK(devjoin_wait(c, c->stream, c->cstream));
      nparts = nb_int + nb_lo + nb_hi;
      faces_on_cstream = out.par(parity);
    }
  }
  c->bnd_out_on_cstream = faces_on_cstream;
  if (o.dot) {
    if (nparts > c->part2_off) { qexhip_set_error("internal: partial buffer too small"); return -3; }
    // deferred final sum (inside k_cg_update) only while every workgroup can afford to re-sum the
    // partials itself; big local volumes take the separate one-block reduction
    if (o.dot == 2 && o.nparts_out && nparts <= 4096) *o.nparts_out = nparts;
    else {
      if (o.nparts_out) *o.nparts_out = 0;
      CHK(devjoin_flush(c));                 // (the reduction reads the boundary launch's partials)
      CHK(reduce_partials(c, nparts, o.dot_out));
    }
  }
  return 0;
}
