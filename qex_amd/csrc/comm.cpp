// comm.cpp -- the communicator: t-face halo exchange and scalar all-reduce, over RCCL (xGMI) or over peer-mapped memory (peer.hip).
//
// Replaces (a) the persistent QMP send/recv pairs behind startSB/boundarySB2
// (src/layout/shifts.nim:67-94,254-285; src/layout/qshifts.nim:51-131) and (b) the
// QMP_sum_double_array at the end of threadRankSum (src/comms/commsUtils.nim:195-204,
// src/comms/commsQmp.nim:127-128).  The lattice is split along t only (rankGeom {1,1,1,N}),
// so every rank talks to two ring neighbours; faces are contiguous tile ranges of the field
// (qexhip_internal.h), so there is no pack or unpack kernel: RCCL sends straight out of the
// field and receives straight into the ghost tiles.
#include "qexhip_internal.h"
#include "peer_shm.h"
#include "../../include/qexhip.h"
#include <rccl/rccl.h>
#include <cstring>
#include <cmath>
#include <cstdlib>

#define NCCLCHK(expr)                                                                      \
  do {                                                                                     \
    ncclResult_t r_ = (expr);                                                              \
    if (r_ != ncclSuccess) {                                                               \
      qexhip_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, ncclGetErrorString(r_)); \
      return QEXHIP_ERR_COMM;                                                              \
    }                                                                                      \
  } while (0)

extern "C" int qexhip_comm_unique_id(char id[QEXHIP_UNIQUE_ID_BYTES]) {
  static_assert(sizeof(ncclUniqueId) <= QEXHIP_UNIQUE_ID_BYTES, "id size");
  ncclUniqueId u;
  NCCLCHK(ncclGetUniqueId(&u));
  memset(id, 0, QEXHIP_UNIQUE_ID_BYTES);
  memcpy(id, &u, sizeof(u));
  return 0;
}

// QEXHIP_TRANSPORT / option "transport": which transport a communicator uses.  One decision for the whole job:
//   rccl (1)  RCCL for everything, the north star's transport; no rendezvous, works across nodes
//   peer (2)  peer-mapped memory for faces and sums (peer.hip); one node; the only choice when ranks share a device
//   mbox (3)  RCCL for the faces, the peer control block's mailboxes for the CG's rank sums (4 us instead of 15-20 per sum); one node
//   auto (0, default)  the ranks of a ONE-NODE job meet in a shared-memory segment named after the id and compare devices: `peer` if
//             any two of them share one (RCCL refuses that), else `mbox` if the mailboxes pass a self-test between the devices, else
//             `rccl`.  A job that spans nodes (LOCAL_WORLD_SIZE and friends say so, or the rendezvous times out) takes `rccl`.
static int transport_wish(const qexhip_ctx *c) {
  if (c->opt_transport >= 0) return c->opt_transport;
  const char *e = getenv("QEXHIP_TRANSPORT");
  if (!e || !*e) return 0;
  if (!strcmp(e, "rccl") || !strcmp(e, "1")) return 1;
  if (!strcmp(e, "peer") || !strcmp(e, "2")) return 2;
  if (!strcmp(e, "mbox") || !strcmp(e, "rccl+mbox") || !strcmp(e, "3")) return 3;
  return 0;
}

// Decide the transport (collective over the node's ranks unless the wish is rccl): peer_shm.cpp has the decision itself (pure host code,
// CPU-tested with forked ranks incl. the multi-node cases).  *mode: 0 rccl, 2 peer, 3 rccl + mailbox sums; for 2 and 3 `host` stays open
// for peer_init.
static int choose_transport(qexhip_ctx *c, const char *id, int nranks, int rank, PeerHost *host, int *mode) {
  char bus[32];
  bus[0] = 0;
  if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, c->device) != hipSuccess) { (void)hipGetLastError(); snprintf(bus, sizeof bus, "dev%d", c->device); }
  double tmo = 120.0;
  if (const char *e = getenv("QEXHIP_RENDEZVOUS_TIMEOUT")) { const double v = atof(e); if (v > 0) tmo = v; }
  int shared = 0;
  CHK(peer_host_choose(host, (const unsigned char *)id, nranks, rank, transport_wish(c), c->device, bus, tmo, mode, &shared));
  c->ranks_share_device = shared;
  return 0;
}

static int rccl_init(qexhip_ctx *c, const char *id, int nranks, int rank);

extern "C" int qexhip_comm_init(qexhip_handle c, const char id[QEXHIP_UNIQUE_ID_BYTES], int nranks, int rank) {
  if (!c || !id) return QEXHIP_ERR_ARG;
  if (nranks != c->rankGeom[3] || rank != c->rankCoord[3]) {
    qexhip_set_error("comm_init: nranks/rank (%d/%d) must equal rankGeom[3]/rankCoord[3] (%d/%d)", nranks, rank,
                     c->rankGeom[3], c->rankCoord[3]);
    return QEXHIP_ERR_ARG;
  }
  if (comm_ready(c)) { qexhip_set_error("communicator already initialised"); return QEXHIP_ERR_STATE; }
  HIPCHK(hipSetDevice(c->device));
  PeerHost host;
  int mode = 0;
  CHK(choose_transport(c, id, nranks, rank, &host, &mode));
  if (mode == 2) {
    c->nranks = nranks;
    c->rank = rank;
    if (int e = peer_init(c, host)) { peer_destroy(c); c->nranks = 1; c->rank = 0; return e; }
    return 0;
  }
  if (mode == 3) {
    // RCCL for the faces, the mailboxes for the sums.  The control blocks are mapped between DISTINCT devices here, and a granule that
    // crosses xGMI is what no box of rounds 1-6 could try: the mapping, a self-test of the all-reduce with known answers, and the
    // agreement on both are all allowed to fail -- every rank then drops the control block together and RCCL carries the sums as
    // well (QEXHIP_TRANSPORT=mbox insists instead).
    c->nranks = nranks;
    c->rank = rank;
    // QEXHIP_TEST_FAIL_MBOX (test hook, tests/test_gpu_misc_ops.py): 1 = the self-test reports a failure; 2 = the same, and an explicit
    // `mbox` wish is treated like `auto` -- the fall-back to RCCL alone, which no one-GPU box reaches otherwise (auto never picks mbox there)
    const char *hook = getenv("QEXHIP_TEST_FAIL_MBOX");
    const int fail_hook = hook ? atoi(hook) : 0;
    const bool insist = transport_wish(c) == 3 && fail_hook != 2;
    int e = peer_init(c, host);
    double bad[1] = {0.0};
    if (!e) {
      bad[0] = (peer_selftest(c) || fail_hook) ? 1.0 : 0.0;
      e = peer_host_reduce(c, bad, 1, 0);               // max over the ranks, through the segment: one outcome for the whole job
    }
    if (e || bad[0] != 0.0) {
      if (!e) qexhip_set_error("mailbox self-test between the devices failed on some rank");
      if (insist) { peer_destroy(c); c->nranks = 1; c->rank = 0; return e ? e : QEXHIP_ERR_COMM; }
      fprintf(stderr, "libqexhip: rank %d: no mailbox sums between the devices (%s): RCCL carries the rank sums too\n", rank, qexhip_last_error());
      peer_destroy(c);
      *c->dj.err = 0;                                    // (a self-test wait that ran out is not an error of the job)
    } else c->hybrid_sums = 1;
    c->nranks = 1; c->rank = 0;
  }
  if (int e = rccl_init(c, id, nranks, rank)) {
    if (c->peer) peer_destroy(c);
    c->hybrid_sums = 0;
    return e;
  }
  return 0;
}

static int rccl_init(qexhip_ctx *c, const char *id, int nranks, int rank) {
  HIPCHK(hipSetDevice(c->device));
  ncclUniqueId u;
  memcpy(&u, id, sizeof(u));
  ncclComm_t comm;
  NCCLCHK(ncclCommInitRank(&comm, nranks, u, rank));
  c->comm = comm;
  c->nranks = nranks;
  c->rank = rank;
  // The face exchange that overlaps the interior sweep is posted on the comm stream while the compute stream posts the
  // all-reduces of the CG scalars.  RCCL serialises the operations of ONE communicator in host issue order whatever
  // stream they are on, i.e. an exchange queued behind an all-reduce that waits for a long kernel would wait too; with a
  // communicator of its own the exchange depends on ev_ready only.  ncclCommSplit is collective over the parent: every
  // rank is here.  QEXHIP_COMM2=0 keeps the single communicator (A/B).
  // Whether the second communicator is used must be ONE decision for the whole job: ranks that disagreed would post the
  // overlapped exchange on different communicators and never match.  So every step is agreed by a min-all-reduce over the
  // parent: (1) the wish (QEXHIP_COMM2=0 on any rank keeps the single communicator everywhere -- no rank may skip the
  // collective split on its own), (2) the outcome of the split (a rank-local failure drops comm2 on every rank).
  auto agree_min = [&](int mine, int *all) -> int {
    double *d = &c->dscal[60];
    double h = (double)mine;
    HIPCHK(hipMemcpyAsync(d, &h, sizeof(double), hipMemcpyHostToDevice, c->stream));
    NCCLCHK(ncclAllReduce(d, d, 1, ncclDouble, ncclMin, comm, c->stream));
    HIPCHK(hipMemcpyAsync(&h, d, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *all = (int)h;
    return 0;
  };
  const char *e2 = getenv("QEXHIP_COMM2");
  int want = (!e2 || atoi(e2) != 0) ? 1 : 0, want_all = 0;
  CHK(agree_min(want, &want_all));
  if (want_all) {
    ncclComm_t comm2 = nullptr;
    ncclResult_t r2 = ncclCommSplit(comm, 0, rank, &comm2, nullptr);
    int n2 = 0, k2 = -1;
    if (r2 == ncclSuccess && comm2) {
      if (ncclCommCount(comm2, &n2) != ncclSuccess || ncclCommUserRank(comm2, &k2) != ncclSuccess || n2 != nranks || k2 != rank) r2 = ncclInternalError;
    }
    int ok = (r2 == ncclSuccess && comm2) ? 1 : 0, ok_all = 0;
    CHK(agree_min(ok, &ok_all));
    if (ok_all) {
      c->comm2 = comm2;
    } else {
      // not fatal: the context keeps the one communicator for both streams, which is what rounds 1-2 ran with
      fprintf(stderr, "libqexhip: rank %d: no second communicator for the comm stream (%s); every rank uses one communicator for both streams\n",
              rank, ok ? "another rank could not split" : (r2 == ncclSuccess ? "split returned none" : ncclGetErrorString(r2)));
      if (comm2) (void)ncclCommDestroy(comm2);
    }
  } else if (want) {
    fprintf(stderr, "libqexhip: rank %d: QEXHIP_COMM2=0 on another rank: one communicator for both streams everywhere\n", rank);
  }
  return 0;
}

void comm_destroy(qexhip_ctx *c) {
  peer_destroy(c);
  if (c->comm2) { ncclCommDestroy((ncclComm_t)c->comm2); c->comm2 = nullptr; }
  if (c->comm) { ncclCommDestroy((ncclComm_t)c->comm); c->comm = nullptr; }
}

extern "C" int qexhip_comm_count(qexhip_handle c, int *ncomms) {
  if (!c || !ncomms) return QEXHIP_ERR_ARG;
  *ncomms = peer_faces(c) ? 2 : (c->comm ? 1 : 0) + (c->comm2 ? 1 : 0);      // peer transport: the two stream classes are independent channels
  return 0;
}

// A context created with rankGeom[3] > 1 holds one slab of a larger lattice: without a communicator the only thing
// the copy fallbacks below could do is wrap that slab onto itself, i.e. silently compute the physics of a different
// (periodic, smaller) lattice.  Every exchange / reduction entry refuses instead.
static int need_comm(const qexhip_ctx *c) {
  if (!comm_ready(c) && c->rankGeom[3] > 1) {
    qexhip_set_error("rankGeom[3] = %d but qexhip_comm_init was not called: refusing to wrap the local slab periodically",
                     c->rankGeom[3]);
    return QEXHIP_ERR_STATE;
  }
  return 0;
}

extern "C" int qexhip_comm_transport(qexhip_handle c, char *name, int len, long stats[4]) {
  if (!c) return QEXHIP_ERR_ARG;
  // "rccl+mbox": RCCL carries the faces, the peer control block's mailboxes the CG's rank sums (one node, distinct devices)
  if (name && len > 0) snprintf(name, len, "%s", peer_faces(c) ? "peer" : (c->comm ? (c->peer ? "rccl+mbox" : "rccl") : "none"));
  if (stats) peer_info(c, stats);
  return 0;
}

// what RCCL itself says about the communicator (bench.py reports it so that "N ranks" is RCCL's count, not ours)
extern "C" int qexhip_comm_info(qexhip_handle c, int *nranks, int *rank, int *device, char *busid, int buslen) {
  if (!c) return QEXHIP_ERR_ARG;
  int n = 0, r = -1, d = c->device;
  if (peer_faces(c)) { n = c->nranks; r = c->rank; }
  if (c->comm) {
    NCCLCHK(ncclCommCount((ncclComm_t)c->comm, &n));
    NCCLCHK(ncclCommUserRank((ncclComm_t)c->comm, &r));
    NCCLCHK(ncclCommCuDevice((ncclComm_t)c->comm, &d));
  }
  if (nranks) *nranks = n;
  if (rank) *rank = r;
  if (device) *device = d;
  if (busid && buslen > 0) {
    busid[0] = 0;
    HIPCHK(hipDeviceGetPCIBusId(busid, buslen, c->device));
  }
  return 0;
}

// transport emulation (one-GPU rehearsals): what an exchange of `bytes` per direction would cost between distinct GPUs --
// a fixed latency (option emu_exchange_us) plus, with option emu_link_gbs > 0, bytes / bandwidth of one xGMI direction
static double emu_exchange_time(const qexhip_ctx *c, size_t bytes) {
  double us = c->emu_exchange_us;
  if (c->emu_link_gbs > 0) us += (double)bytes / (1e3 * c->emu_link_gbs);
  return us;
}
// RCCL arm: a wait in front of the group (the one-rank self-copy that follows stands in for nothing: it is extra).
// Peer arm: the time goes INTO the exchange kernel (peer.hip): data counts as arrived no earlier than that long after the
// kernel started, the local copy that stands in for the remote push runs inside the window -- as the real push would.
static int emu_exchange(qexhip_ctx *c, hipStream_t st, size_t bytes) {
  if (peer_faces(c)) return 0;
  return blas_delay(st, (int)(emu_exchange_time(c, bytes) + 0.5));
}

static inline int upper(const qexhip_ctx *c) { return (c->rank + 1) % c->nranks; }
static inline int lower(const qexhip_ctx *c) { return (c->rank - 1 + c->nranks) % c->nranks; }

// Exchange the t-faces of one parity half of a field that stores a site in `site_bytes` bytes (48: DevField, 24: DevFieldF, 16: DevFieldH)
// and whose ghost zones begin `ghost_off` bytes behind `base` (the body's ntile * 64 sites): a face is the contiguous byte range of
// depth * F sites in all three layouts, and the emulated transport delay sees the true byte count.  Runs on the comm stream after ev_ready (the producer of the field on the compute stream); the caller joins (devjoin_signal / devjoin_wait) behind
// whatever it posts after the exchange.  Message order is the same on every rank -- sends {bottom->lower, top->upper}, receives
// {ghost_hi<-upper, ghost_lo<-lower} -- so that with two ranks (upper == lower) or one rank (self) the k-th send pairs with the k-th recv.
static int halo_exchange(qexhip_ctx *c, char *base, size_t site_bytes, size_t ghost_off, int overlap, bool wait_ready) {
  // overlap == 0: post the exchange on the compute stream itself (no cross-stream events).  Used
  // when the interior sweep is too short to hide the exchange: two cross-stream dependencies
  // cost more than they buy there.
  CHK(need_comm(c));
  hipStream_t cs = overlap ? c->cstream : c->stream;
  const Geom &g = c->g;
  const size_t bytes = (size_t)g.depth * g.F * site_bytes;       // per face
  // RCCL's element: the field's own real type, or 32-bit words for the 16-bit sites (six int16 and an fp32 norm)
  const ncclDataType_t type = site_bytes == 48 ? ncclDouble : (site_bytes == 24 ? ncclFloat : ncclUint32);
  const size_t nd = bytes / (site_bytes == 48 ? 8 : 4);          // elements per face
  char *bottom = base;                                           // t = 0 .. depth-1
  char *top = base + ghost_off - bytes;                          // t = Xt-depth .. Xt-1
  char *ghost_hi = base + ghost_off;
  char *ghost_lo = ghost_hi + bytes;
  if (overlap && wait_ready) HIPCHK(hipStreamWaitEvent(c->cstream, c->ev_ready, 0));     // (not when the comm stream produced the faces itself)
  ScopedTimer tm(c, "exchange", cs);            // on the stream the group is posted on: transport + waiting for the neighbours
  CHK(emu_exchange(c, cs, bytes));
  if (peer_faces(c)) {
    const void *dn = bottom, *up = top;
    void *from_up = ghost_hi, *from_dn = ghost_lo;
    CHK(peer_exchange(c, cs, 1, &dn, 1, &up, &from_up, &from_dn, bytes, emu_exchange_time(c, bytes)));
  } else if (c->comm) {
    // the overlapped exchange has the second communicator to itself (comm_init)
    ncclComm_t comm = (ncclComm_t)((overlap && c->comm2) ? c->comm2 : c->comm);
    NCCLCHK(ncclGroupStart());
    NCCLCHK(ncclSend(bottom, nd, type, lower(c), comm, cs));
    NCCLCHK(ncclSend(top, nd, type, upper(c), comm, cs));
    NCCLCHK(ncclRecv(ghost_hi, nd, type, upper(c), comm, cs));
    NCCLCHK(ncclRecv(ghost_lo, nd, type, lower(c), comm, cs));
    NCCLCHK(ncclGroupEnd());
  } else {
    // single rank, no communicator: periodic wrap by device-to-device copies
    HIPCHK(hipMemcpyAsync(ghost_hi, bottom, bytes, hipMemcpyDeviceToDevice, cs));
    HIPCHK(hipMemcpyAsync(ghost_lo, top, bytes, hipMemcpyDeviceToDevice, cs));
  }
  // overlap: the caller (dslash_sweep) posts its boundary launch behind the group on cstream and the join signal after it
  return 0;
}
int comm_halo_exchange(qexhip_ctx *c, DevField &f, int parity, int overlap, bool wait_ready) {
  return halo_exchange(c, (char *)f.par(parity), 3 * sizeof(double2), (size_t)c->g.ntile * 192 * sizeof(double2), overlap, wait_ready);
}
// the reduced-precision fields of the mixed-precision CGs (dslash_lowp.h), one parity half at `half`: the same messages in the same order
// at site_bytes = 24 (DevFieldF) or 16 (DevFieldH: a site is one 16-byte element at its position, so the faces are the ranges
// [0, depth F) and [Vh - depth F, Vh) of the half); in both the ghost zones follow the body's ntile * 64 sites
int comm_halo_exchange_sites(qexhip_ctx *c, void *half, size_t site_bytes, int overlap) {
  return halo_exchange(c, (char *)half, site_bytes, (size_t)c->g.ntile * 64 * site_bytes, overlap, true);
}

// Peer transport, the fused sweeps: the faces of one parity half of n fields (fused_sweep_setup: n = 1 for dslash_sweep, up to 4 for the lock-step batch) will be
// pushed by the caller's OWN kernel (`push` is filled for its first workgroups) and what arrives STAYS in the receive arena.
// gh_hi[j] / gh_lo[j] come back pre-offset so that gh[vec_off(pos, colour)] addresses the ghost POSITION pos of field j (ghost_hi: pos in
// [Vh, Vh + depth F), ghost_lo: the depth F positions behind it) -- the kernel reads them instead of the fields' ghost tiles and returns
// the credits (peer_ghost_args).  Nothing is launched here.
int comm_halo_push_only_multi(qexhip_ctx *c, int n, DevField *const *f, int parity, const double2 **gh_hi, const double2 **gh_lo, PeerPush *push) {
  CHK(need_comm(c));
  if (!peer_faces(c)) { qexhip_set_error("internal: fused sweep without the peer transport's arenas"); return QEXHIP_ERR_STATE; }
  if (n < 1 || n > 4) { qexhip_set_error("internal: fused sweep over %d fields", n); return QEXHIP_ERR_ARG; }
  const Geom &g = c->g;
  const size_t face2 = (size_t)g.depth * g.F * 3;
  const size_t nd = face2 * 2;
  const void *dn[4], *up[4];
  for (int j = 0; j < n; j++) {
    double2 *base = f[j]->par(parity);
    dn[j] = base; up[j] = base + (size_t)(g.ntile) * 192 - face2;
  }
  const void *from_up = nullptr, *from_dn = nullptr;
  CHK(peer_exchange(c, c->cstream, n, dn, n, up, nullptr, nullptr, nd * sizeof(double), emu_exchange_time(c, (size_t)n * nd * sizeof(double)), &from_up, &from_dn, push));
  // tile-aligned zones (64 | F): vec_off(pos, k) - vec_off(zone start, 0) = vec_off(pos - zone start, k)
  for (int j = 0; j < n; j++) {
    gh_hi[j] = (const double2 *)from_up + (size_t)j * face2 - (size_t)(g.Vh >> 6) * 192;
    gh_lo[j] = (const double2 *)from_dn + (size_t)j * face2 - (size_t)((g.Vh + g.depth * g.F) >> 6) * 192;
  }
  return 0;
}

// The same for the input fields of the n systems of a lock-step batch in ONE RCCL group (one kernel instead of n): per field
// the message order of comm_halo_exchange, fields in ascending order on every rank.
int comm_halo_exchange_multi(qexhip_ctx *c, int n, DevField *const *f, int parity, int overlap) {
  CHK(need_comm(c));
  hipStream_t cs = overlap ? c->cstream : c->stream;
  const Geom &g = c->g;
  const size_t face2 = (size_t)g.depth * g.F * 3;
  const size_t nd = face2 * 2;
  if (overlap) HIPCHK(hipStreamWaitEvent(c->cstream, c->ev_ready, 0));
  ScopedTimer tm(c, "exchange", cs);
  CHK(emu_exchange(c, cs, (size_t)n * nd * sizeof(double)));
  if (peer_faces(c)) {
    std::vector<const void *> dn(n), up(n);
    std::vector<void *> from_up(n), from_dn(n);
    for (int j = 0; j < n; j++) {
      double2 *base = f[j]->par(parity);
      dn[j] = base; up[j] = base + (size_t)(g.ntile) * 192 - face2;
      from_up[j] = base + (size_t)g.ntile * 192; from_dn[j] = base + (size_t)g.ntile * 192 + face2;
    }
    CHK(peer_exchange(c, cs, n, dn.data(), n, up.data(), from_up.data(), from_dn.data(), nd * sizeof(double),
                      emu_exchange_time(c, (size_t)n * nd * sizeof(double))));
  } else if (c->comm) {
    ncclComm_t comm = (ncclComm_t)((overlap && c->comm2) ? c->comm2 : c->comm);
    NCCLCHK(ncclGroupStart());
    for (int j = 0; j < n; j++) {
      double2 *base = f[j]->par(parity);
      NCCLCHK(ncclSend(base, nd, ncclDouble, lower(c), comm, cs));
      NCCLCHK(ncclSend(base + (size_t)(g.ntile) * 192 - face2, nd, ncclDouble, upper(c), comm, cs));
    }
    for (int j = 0; j < n; j++) {
      double2 *ghost_hi = f[j]->par(parity) + (size_t)g.ntile * 192;
      NCCLCHK(ncclRecv(ghost_hi, nd, ncclDouble, upper(c), comm, cs));
      NCCLCHK(ncclRecv(ghost_hi + face2, nd, ncclDouble, lower(c), comm, cs));
    }
    NCCLCHK(ncclGroupEnd());
  } else {
    for (int j = 0; j < n; j++) {
      double2 *base = f[j]->par(parity), *ghost_hi = base + (size_t)g.ntile * 192;
      HIPCHK(hipMemcpyAsync(ghost_hi, base, nd * sizeof(double), hipMemcpyDeviceToDevice, cs));
      HIPCHK(hipMemcpyAsync(ghost_hi + face2, base + (size_t)(g.ntile) * 192 - face2, nd * sizeof(double), hipMemcpyDeviceToDevice, cs));
    }
  }
  return 0;
}

// The reduced-precision parity halves of the n systems of a mixed-precision lock-step batch (dslash_lowp.h: sweep_mrhs) in ONE RCCL group
// or ONE peer exchange with n buffers per direction (no communicator: n pairs of wrap copies): per half the messages of
// comm_halo_exchange_sites, halves in ascending order on every rank -- the message order of comm_halo_exchange_multi.  The emulated
// transport delay sees the true byte count n depth F site_bytes.  n is the batch's nrhs on every rank, whatever its systems' `done` words say.
int comm_halo_exchange_sites_multi(qexhip_ctx *c, int n, void *const *halves, size_t site_bytes, int overlap) {
  CHK(need_comm(c));
  if (n < 1 || n > 4) { qexhip_set_error("internal: face exchange of %d reduced-precision halves", n); return QEXHIP_ERR_ARG; }
  hipStream_t cs = overlap ? c->cstream : c->stream;
  const Geom &g = c->g;
  const size_t bytes = (size_t)g.depth * g.F * site_bytes;       // per face
  const size_t ghost_off = (size_t)g.ntile * 64 * site_bytes;
  const ncclDataType_t type = site_bytes == 24 ? ncclFloat : ncclUint32;
  const size_t nd = bytes / 4;
  if (overlap) HIPCHK(hipStreamWaitEvent(c->cstream, c->ev_ready, 0));
  ScopedTimer tm(c, "exchange", cs);
  CHK(emu_exchange(c, cs, (size_t)n * bytes));
  if (peer_faces(c)) {
    const void *dn[4], *up[4];
    void *from_up[4], *from_dn[4];
    for (int j = 0; j < n; j++) {
      char *base = (char *)halves[j];
      dn[j] = base; up[j] = base + ghost_off - bytes;
      from_up[j] = base + ghost_off; from_dn[j] = base + ghost_off + bytes;
    }
    CHK(peer_exchange(c, cs, n, dn, n, up, from_up, from_dn, bytes, emu_exchange_time(c, (size_t)n * bytes)));
  } else if (c->comm) {
    ncclComm_t comm = (ncclComm_t)((overlap && c->comm2) ? c->comm2 : c->comm);
    NCCLCHK(ncclGroupStart());
    for (int j = 0; j < n; j++) {
      char *base = (char *)halves[j];
      NCCLCHK(ncclSend(base, nd, type, lower(c), comm, cs));
      NCCLCHK(ncclSend(base + ghost_off - bytes, nd, type, upper(c), comm, cs));
    }
    for (int j = 0; j < n; j++) {
      char *ghost_hi = (char *)halves[j] + ghost_off;
      NCCLCHK(ncclRecv(ghost_hi, nd, type, upper(c), comm, cs));
      NCCLCHK(ncclRecv(ghost_hi + bytes, nd, type, lower(c), comm, cs));
    }
    NCCLCHK(ncclGroupEnd());
  } else {
    for (int j = 0; j < n; j++) {
      char *base = (char *)halves[j], *ghost_hi = base + ghost_off;
      HIPCHK(hipMemcpyAsync(ghost_hi, base, bytes, hipMemcpyDeviceToDevice, cs));
      HIPCHK(hipMemcpyAsync(ghost_hi + bytes, base + ghost_off - bytes, bytes, hipMemcpyDeviceToDevice, cs));
    }
  }
  return 0;
}

// send `bytes` to the upper neighbour, receive the same amount from the lower one (stream-ordered)
int comm_exchange_raw(qexhip_ctx *c, const void *send_up, void *recv_from_down, size_t bytes, hipStream_t st) {
  CHK(need_comm(c));
  CHK(emu_exchange(c, st, bytes));
  if (peer_faces(c)) {
    CHK(peer_exchange(c, st, 0, nullptr, 1, &send_up, nullptr, &recv_from_down, bytes, emu_exchange_time(c, bytes)));
  } else if (c->comm) {
    ncclComm_t comm = (ncclComm_t)c->comm;
    NCCLCHK(ncclGroupStart());
    NCCLCHK(ncclSend(send_up, bytes, ncclChar, upper(c), comm, st));
    NCCLCHK(ncclRecv(recv_from_down, bytes, ncclChar, lower(c), comm, st));
    NCCLCHK(ncclGroupEnd());
  } else {
    HIPCHK(hipMemcpyAsync(recv_from_down, send_up, bytes, hipMemcpyDeviceToDevice, st));
  }
  return 0;
}

// faces of several buffers (the two parity halves of one or more matrix fields) in ONE group, both directions:
// bottom[k] -> lower neighbour's ghost_hi, top[k] -> upper neighbour's ghost_lo   (same message order as above).
// async: on the comm stream (second communicator) after ev_ready, which the caller recorded behind the producer of the
// buffers; nothing waits for it here -- the caller joins (devjoin_signal on the comm stream, devjoin_wait on the compute stream)
// before the first kernel that reads the ghosts.
int comm_faces_exchange(qexhip_ctx *c, int nbuf, double *const bottom[], double *const top[], double *const ghost_hi[],
                        double *const ghost_lo[], size_t ndoubles, int async) {
  CHK(need_comm(c));
  hipStream_t st = async ? c->cstream : c->stream;
  if (async) HIPCHK(hipStreamWaitEvent(c->cstream, c->ev_ready, 0));
  ScopedTimer tm(c, "faces", st);               // after the wait for the producer: transport only (the same span as "exchange" above)
  CHK(emu_exchange(c, st, (size_t)nbuf * ndoubles * sizeof(double)));
  if (peer_faces(c)) {
    CHK(peer_exchange(c, st, nbuf, (const void *const *)bottom, nbuf, (const void *const *)top, (void *const *)ghost_hi, (void *const *)ghost_lo,
                      ndoubles * sizeof(double), emu_exchange_time(c, (size_t)nbuf * ndoubles * sizeof(double))));
  } else if (c->comm) {
    ncclComm_t comm = (ncclComm_t)((async && c->comm2) ? c->comm2 : c->comm);
    NCCLCHK(ncclGroupStart());
    for (int k = 0; k < nbuf; k++) {
      NCCLCHK(ncclSend(bottom[k], ndoubles, ncclDouble, lower(c), comm, st));
      NCCLCHK(ncclSend(top[k], ndoubles, ncclDouble, upper(c), comm, st));
    }
    for (int k = 0; k < nbuf; k++) {
      NCCLCHK(ncclRecv(ghost_hi[k], ndoubles, ncclDouble, upper(c), comm, st));
      NCCLCHK(ncclRecv(ghost_lo[k], ndoubles, ncclDouble, lower(c), comm, st));
    }
    NCCLCHK(ncclGroupEnd());
  } else {
    for (int k = 0; k < nbuf; k++) {
      HIPCHK(hipMemcpyAsync(ghost_hi[k], bottom[k], ndoubles * sizeof(double), hipMemcpyDeviceToDevice, st));
      HIPCHK(hipMemcpyAsync(ghost_lo[k], top[k], ndoubles * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
  }
  return 0;
}

// rank-ordered concatenation of `n` doubles per rank (one rank / no communicator: a copy)
int comm_allgather(qexhip_ctx *c, const double *send, double *recv, size_t n) {
  CHK(need_comm(c));
  if (peer_faces(c) && c->nranks > 1) return peer_allgather(c, send, recv, n);
  if (c->comm && c->nranks > 1) {
    NCCLCHK(ncclAllGather(send, recv, n, ncclDouble, (ncclComm_t)c->comm, c->stream));
  } else {
    HIPCHK(hipMemcpyAsync(recv, send, n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  }
  return 0;
}

int comm_allreduce(qexhip_ctx *c, double *dptr, int n) {
  CHK(need_comm(c));
  if (!multi_rank(c) || !comm_ready(c)) return 0;    // one rank without the rehearsal hook, or no communicator: nothing to sum
  ScopedTimer tm(c, "allreduce", c->stream);
  if (c->peer) return peer_allreduce(c, dptr, n, 0);       // (emulated latency: inside the kernel)
  CHK(blas_delay(c->stream, c->emu_allreduce_us));
  NCCLCHK(ncclAllReduce(dptr, dptr, n, ncclDouble, ncclSum, (ncclComm_t)c->comm, c->stream));
  return 0;
}

// The workgroup partials parts[0..n) of a dot product, summed over the ranks, for a consumer that sums *n_out values itself:
//   RCCL  the partial VECTOR is all-reduced in place (a few KB: the latency of one double), *n_out = n
//   peer  one single-workgroup launch sums the vector in the consumers' own order (cg_sum_parts), passes the scalar through
//         the mailboxes and leaves the rank-ordered total in parts[0], *n_out = 1
// commsUtils.nim:195-204 (threadRankSum) is what both replace.
int comm_allreduce_parts(qexhip_ctx *c, double *parts, int n, int *n_out) {
  *n_out = n;
  CHK(need_comm(c));
  if (!multi_rank(c) || !comm_ready(c) || n <= 0) return devjoin_flush(c);     // (a join deferred to this call still has to happen)
  if (!c->peer) { CHK(devjoin_flush(c)); return comm_allreduce(c, parts, n); }
  ScopedTimer tm(c, "allreduce", c->stream);
  *n_out = 1;
  return peer_allreduce_parts(c, parts, n);
}

// comm_allreduce_parts for the m systems of a lock-step batch in ONE collective: system j's partials are parts[j][0..n), and the ranges
// lie `stride` doubles apart (parts[j] = parts[0] + j stride).  Every system's sum is formed exactly as comm_allreduce_parts forms it for
// that system alone, so the consumer sees the bits of the single-system solve:
//   RCCL  the partial vectors are all-reduced elementwise in place, one all-reduce over [parts[0], parts[m-1] + n), *n_out = n
//   peer  one single-workgroup launch sums every system's vector in cg_sum_parts order to one operand, the m operands cross the mailboxes
//         in one set of tagged words and the rank-ordered totals land in parts[j][0], *n_out = 1; the deferred join of a split sweep
//         rides in its prologue
// gate (peer): 1 leaves out the systems that are done, 2 those without a pending reliable update (what their consumers skip) -- a system's
// stale partials never enter a sum.  RCCL reduces stale ranges in place with the rest; they grow by the factor nranks per collective and
// NOTHING reads them: every consumer (k_slpb_update, k_slpb_close, k_slpb_rclose and their 16-bit forms) tests the same flags first, and
// a live system's producer rewrites its whole range ahead of the collective.  Posted whatever the flags say: same collectives on every rank.
int comm_allreduce_parts_multi(qexhip_ctx *c, int m, double *parts0, size_t stride, int n, const SlpScal *st, int gate, int *n_out) {
  *n_out = n;
  CHK(need_comm(c));
  if (!multi_rank(c) || !comm_ready(c) || n <= 0) return devjoin_flush(c);
  if (!c->peer) { CHK(devjoin_flush(c)); return comm_allreduce(c, parts0, (int)(stride * (size_t)(m - 1)) + n); }
  ScopedTimer tm(c, "allreduce", c->stream);
  *n_out = 1;
  return peer_allreduce_parts_multi(c, m, parts0, stride, n, st, gate);
}

int comm_allreduce_max(qexhip_ctx *c, double *host, int n) {
  if (n > 4) return QEXHIP_ERR_ARG;
  if (!comm_ready(c) || c->nranks < 2) return 0;
  if (c->peer) return peer_host_reduce(c, host, n, 0);     // host operands: through the rendezvous segment, no GPU involved (hybrid too)
  double *d = &c->dscal[56];
  HIPCHK(hipMemcpyAsync(d, host, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  NCCLCHK(ncclAllReduce(d, d, n, ncclDouble, ncclMax, (ncclComm_t)c->comm, c->stream));
  HIPCHK(hipMemcpyAsync(host, d, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// The CG loops run their control flow on every rank separately (loop condition on the rank's own copy of the all-reduced
// residual, as the reference does after its QMP sum, cg.nim:174): if two ranks ever held different bits they would leave
// the loop at different iterations and the next collective would never complete.  At the end of every chunk of iterations
// the state the host is about to read is therefore max-reduced as {r2, -r2, itn, -itn}; max and min must coincide.
int comm_agree_post(qexhip_ctx *c) {
  CHK(need_comm(c));
  if (!multi_rank(c) || !comm_ready(c)) return 0;
  if (c->peer) return peer_allreduce(c, c->cg->agree, 4, 1);
  NCCLCHK(ncclAllReduce(c->cg->agree, c->cg->agree, 4, ncclDouble, ncclMax, (ncclComm_t)c->comm, c->stream));
  return 0;
}
int comm_agree_check(qexhip_ctx *c, const CgScal &h) {
  if (!multi_rank(c) || !comm_ready(c)) return 0;
  CHK(peer_check(c));
  const bool both_nan = std::isnan(h.agree[0]) && std::isnan(h.agree[1]);     // a NaN residual ends the loop on every rank alike
  if ((!both_nan && h.agree[0] != -h.agree[1]) || h.agree[2] != -h.agree[3]) {
    qexhip_set_error("sharded CG: the ranks disagree on the residual (%.17g .. %.17g) or the iteration count (%g .. %g) -- "
                     "the all-reduce did not return the same bits on every rank", -h.agree[1], h.agree[0], -h.agree[3], h.agree[2]);
    return QEXHIP_ERR_COMM;
  }
  return 0;
}
