/* qexhip.h -- C ABI of libqexhip.so: MI355X-native staggered Dslash + CG (+ Wilson flow)
 * behind QEX's stagD / stagSolve operator API.
 *
 * This is the drop-in boundary.  Every entry point names the reference interface it
 * replaces (file:line relative to ctpeterson/qex @ 2025-02-23).  The precedent for the
 * whole boundary is QEX's own QUDA bridge, src/quda/qudaWrapperImpl.nim:165-261
 * (qudaSolveXX): host fields are handed over site-major in the V=1 layout, one C call
 * does the solve, the solution is copied back.  INTEGRATION.md shows the Nim binding.
 *
 * Conventions
 *   - all pointers are HOST pointers to fp64 data unless a name says `dev`;
 *   - site order: V=1 MILC even-odd order of the rank-local lattice
 *       lex = x0 + L0*(x1 + L1*(x2 + L2*x3)); idx = lex/2 + ((x0+x1+x2+x3)&1)*vol/2
 *     (src/layout/qlayout.nim:110-131 with innerGeom = 1);
 *   - colour vector: double[vol][3][2]; gauge field: double[vol][4][3][3][2]
 *     ([site][mu][row][col][re,im], QUDA_MILC_GAUGE_ORDER as in qudaWrapperImpl.nim:216-240);
 *   - links passed to qexhip_stag_set_links already carry boundary conditions and
 *     staggered phases (Staggered.g, src/physics/stagD.nim:19-22,72-80); they are general
 *     3x3 complex matrices (smeared links are not unitary);
 *   - parity: 0 = "even", 1 = "odd", 2 = "all" (src/layout/layoutX.nim:285-295);
 *   - return value: 0 = ok, <0 = error, message from qexhip_last_error().  Not converging
 *     within maxits is NOT an error (src/solvers/cg.nim:174): iters == maxits is returned.
 *   - threading: entry points are called from one host thread (the master thread outside
 *     any `threads:` block, src/physics/stagSolve.nim:63,78); one context per GPU/rank.
 */
#ifndef QEXHIP_H
#define QEXHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qexhip_ctx *qexhip_handle;

#define QEXHIP_OK 0
#define QEXHIP_ERR_ARG (-1)
#define QEXHIP_ERR_HIP (-2)
#define QEXHIP_ERR_STATE (-3)
#define QEXHIP_ERR_COMM (-4)
#define QEXHIP_ERR_IO (-5)

#define QEXHIP_EVEN 0
#define QEXHIP_ODD 1
#define QEXHIP_ALL 2

/* ---------------- context ----------------
 * Replaces qudaInit/qudaSetup (src/quda/qudaWrapperImpl.nim:70-123): bind one GPU, record the
 * rank-local lattice and the rank grid (src/layout/layoutX.nim:70-125).  Only a split of the
 * outermost dimension is supported: rankGeom = {1,1,1,N} (BASELINE.json north_star).
 * Preconditions on latLocal (checked here and at set_links; QEXHIP_ERR_ARG otherwise) -- narrower than QEX's "any even
 * lattice, any rankGeom" (src/layout/layoutX.nim:46-68,81-95):
 *   * every extent even (the even/odd layout);
 *   * sharded (rankGeom[3] > 1 or qexhip_comm_force_halo): X*Y*Z/2 a multiple of 64, so that a t-slice of one parity is a whole
 *     number of 64-site wavefront tiles and the faces are contiguous tile ranges (no pack kernels); local t even; local t
 *     >= 1 for the one-hop operator, >= 3 for Naik links (ghost depth 3);
 *   * unsharded: X*Y*Z*T/2 need not be a multiple of 64 (the last tile is ragged).
 * On any failure after the context was allocated everything built so far is released; *h is written only on success. */
int qexhip_init(qexhip_handle *h, int device, const int latLocal[4],
                const int rankGeom[4], const int rankCoord[4]);
int qexhip_finalize(qexhip_handle h);
/* number of HIP devices this process can bind (qudaInit takes the device from the caller too,
 * src/quda/qudaWrapperImpl.nim:70-83): a host picks device = (rank on its node) mod this count */
int qexhip_device_count(int *n);
const char *qexhip_last_error(void);
/* wait for all work queued on the context's streams */
int qexhip_sync(qexhip_handle h);
/* library / device description, for logs */
int qexhip_device_info(qexhip_handle h, char *buf, int buflen);

/* ---------------- communicator (RCCL over xGMI, or peer-mapped memory) ----------------
 * Replaces the QMP send/recv pairs of the shifts (src/layout/qshifts.nim:51-131) and
 * threadRankSum's QMP_sum (src/comms/commsUtils.nim:195-204, commsQmp.nim:127-128).
 * Rank 0 obtains an id, the host broadcasts it (QMP_broadcast in QEX), every rank calls init (collective; an id serves ONE
 * comm_init).  Two transports sit behind the same entry points (QEXHIP_TRANSPORT / option "transport", one value for the
 * whole job):
 *   rccl   ncclSend/ncclRecv groups and ncclAllReduce between DISTINCT devices; no rendezvous; works across nodes
 *   peer   every rank maps its neighbours' receive arenas and every rank's mailbox through hipIpc; a face exchange is a push into
 *          the neighbour's HBM (from inside the sweep kernel itself where sweeps overlap: option "hop_split"), an all-reduce one
 *          single-workgroup kernel that sums the ranks' mailboxes in rank order (bit-identical on every rank).  One node only
 *          (<= 16 ranks).  It is the only transport that lets several ranks share ONE device, which RCCL refuses
 *   mbox   RCCL for the faces, the mailboxes of `peer` for the scalar rank sums of the solvers (one single-workgroup kernel of ~4 us
 *          instead of an ncclAllReduce of 15-20 us, two per CG iteration; cg.nim:206-214); one node; reported as "rccl+mbox"
 *   auto   (default) the ranks of a ONE-NODE job meet in a POSIX shared-memory segment named after the id and take `peer` if any
 *          two of them are bound to the same device, else `mbox` -- provided the control blocks map between the devices and a
 *          self-test of the mailbox all-reduce (known answers, 5 s bound) passes on every rank; if not, all ranks drop to `rccl`
 *          together.  A job that SPANS NODES takes `rccl`: by what the launcher says (QEXHIP_LOCAL_RANKS, LOCAL_WORLD_SIZE,
 *          OMPI_COMM_WORLD_LOCAL_SIZE, MPI_LOCALNRANKS, SLURM_NTASKS_PER_NODE: fewer local ranks than nranks -> no rendezvous at
 *          all) or, with no such variable, when the node-local rendezvous does not complete within QEXHIP_RENDEZVOUS_TIMEOUT
 *          (s, default 120) -- every node's ranks time out alike, so the decision stays one for the whole job; only an explicit
 *          `peer` / `mbox` turns that timeout into QEXHIP_ERR_COMM.  QEXHIP_PEER_TIMEOUT (s, default 30) bounds every device-side
 *          wait: a rank that never arrives becomes QEXHIP_ERR_COMM on the others, never a hang. */
#define QEXHIP_UNIQUE_ID_BYTES 128
int qexhip_comm_unique_id(char id[QEXHIP_UNIQUE_ID_BYTES]);
int qexhip_comm_init(qexhip_handle h, const char id[QEXHIP_UNIQUE_ID_BYTES], int nranks, int rank);
/* What RCCL reports for the communicator (ncclCommCount / ncclCommUserRank / ncclCommCuDevice) and the PCI bus id of
 * the bound GPU -- QEX prints the same facts from QMP at start-up (src/comms/commsQmp.nim:14-33: rank, size).
 * Without a communicator nranks = 0, rank = -1.  Any output pointer may be NULL.
 * A context with rankGeom[3] > 1 refuses every exchange / reduction until qexhip_comm_init has run (QEXHIP_ERR_STATE). */
int qexhip_comm_info(qexhip_handle h, int *nranks, int *rank, int *device, char *busid, int buslen);
/* which transport the communicator runs on: name = "none" | "rccl" | "rccl+mbox" | "peer"; stats (may be NULL) = peer-transport counters
 * {face exchanges posted, all-reduces posted, arena (re)allocations, bytes of receive arena}, zeros otherwise */
int qexhip_comm_transport(qexhip_handle h, char *name, int len, long stats[4]);
/* number of RCCL communicators the context holds: 0 before comm_init, 2 afterwards (one for the compute stream's all-reduces
 * and ghost refreshes, one -- ncclCommSplit of the first -- for the face exchanges posted on the second stream beside the
 * interior sweep, so that neither queues behind the other), 1 with QEXHIP_COMM2=0.  Peer transport: 2 (the two streams'
 * channels are independent by construction). */
int qexhip_comm_count(qexhip_handle h, int *ncomms);
/* How a one-parity sweep runs on this context's (t-sharded) field: out[0] = 1 if t-hops across the slab boundary go through
 * ghost zones, out[1] = 1 if the face exchange runs beside interior work (second stream, or inside the fused launch), out[2] = interior
 * sites of one parity, out[3] = bytes of one face message, out[4] = 1 if out[1] was MEASURED: with a communicator of more
 * than one rank, set_links times a few sweeps in every form (collective; the slowest rank decides, so all ranks agree) --
 * out[5], out[6] = microseconds per sweep it saw exchange-first / overlapped and split by sites (0: that form was not timed;
 * qexhip_stag_sweep_tuning has all three forms); otherwise out[1] follows option "overlap" or, at -1, the rule of the one-rank
 * rehearsals (overlap when the interior is >= 131072 sites and a face >= 1 MiB); out[7] = the option's value.  bench.py prints it
 * so that a scaling run explains its own launch structure. */
int qexhip_stag_sweep_info(qexhip_handle h, int out[8]);
/* ... and what set_links MEASURED for them (collective, max over ranks; qexhip_device_info prints the same):
 *   out[0] one face exchange of this operator, microseconds (measured where the communicator has more than one rank or option
 *          "overlap" = -2 asked for it; otherwise the estimate 3 us + face bytes at 45 GB/s per xGMI direction)
 *   out[1] where in its dispatch order the fused sweep puts its boundary workgroups (0.65 .. 1: out[0] over the estimated interior time)
 *   out[2..4] microseconds per sweep in the three forms: exchange first | overlapped, split by sites | fused (0: not measured / not available)
 *   out[5] the form an overlapped sweep takes: 2 fused, 0 split by sites        out[6] the fused sweep's short wait, us (-1: parks always)
 *   out[7] 1 if sweeps overlap at all
 * The decisions are timing-dependent and regroup the dot-product partials (the fused form also sums a boundary site's local hops
 * first): a job that needs its residual history bit-reproducible from run to run pins "overlap" and "hop_split". */
int qexhip_stag_sweep_tuning(qexhip_handle h, double out[8]);
/* test hook: with one rank, route the t-direction hops through the halo path
 * (pack -> RCCL self send/recv -> boundary sweep) instead of the periodic wrap. */
int qexhip_comm_force_halo(qexhip_handle h, int on);

/* ---------------- QEX's SIMD field memory <-> the host format of this header ----------------
 * A QEX Field[V,T] is double[outer][...T...][re|im][V lanes] with site i = outer*V + lane (src/field/fieldET.nim:18-22,123-128);
 * which lattice site that is follows LayoutQ (src/layout/qlayout.nim:10-66 set-up, :110-131 index, :133-185 coordinates).
 * Everything below takes the RANK-LOCAL geometry and the inner (SIMD) geometry of the Layout[V] (l.localGeom, l.innerGeom) and
 * the field's own memory, and produces / consumes the V = 1 even-odd site-major arrays every other entry point of this header
 * takes ([site][3][2], [site][4][3][3][2]) -- the per-site copy loops of the QUDA bridge (src/quda/qudaWrapperImpl.nim:198-260:
 * r.l.coord -> lo1.rankIndex) as one call.  Pure host code, no GPU needed. */
/* the inner geometry newLayoutX picks for V lanes when none is given (src/layout/layoutX.nim:19-42,98-111); {1,2,2,2} for V = 8
 * on lattices whose y, z, t extents are multiples of 4; QEXHIP_ERR_ARG where QEX itself gives up ("can't lay out inner geom") */
int qexhip_layout_default_inner(const int localGeom[4], int V, int innerGeom[4]);
/* v1_of_simd[outer*V + lane] = index of that site in the V = 1 even-odd order (Layout[1].rankIndex(Layout[V].coord(i))) */
/* (all of these refuse an ODD local extent: the even/odd split of a QEX field then depends on the rank origin, which they are not given) */
int qexhip_layout_simd_map(const int localGeom[4], const int innerGeom[4], int *v1_of_simd);
/* colour vector: simd = double[outer][3][2][V] */
int qexhip_layout_vec_simd_to_v1(const int localGeom[4], const int innerGeom[4], const double *simd, double *v1);
int qexhip_layout_vec_v1_to_simd(const int localGeom[4], const int innerGeom[4], const double *v1, double *simd);
/* gauge field: g[mu] = double[outer][3][3][2][V], one QEX field per direction (s.g[mu]; s.g[2 mu] / s.g[2 mu + 1] for the fat /
 * long links of a Naik operator, stagD.nim:552-564: the caller picks the four pointers) */
int qexhip_layout_gauge_simd_to_v1(const int localGeom[4], const int innerGeom[4], const double *const g[4], double *v1);
int qexhip_layout_gauge_v1_to_simd(const int localGeom[4], const int innerGeom[4], const double *v1, double *const g[4]);

/* ---------------- staggered operator ----------------
 * Staggered.g  (src/physics/stagD.nim:19-22; newStag :522-541, newStag3 :543-564).
 * fat: 4 links per site; lng: NULL (plain) or 4 three-hop links per site (Naik). */
int qexhip_stag_set_links(qexhip_handle h, const double *fat, const double *lng);

/* stagD2 (src/physics/stagD.nim:349-395):
 *   r[parity] = a*r + b*x + sum_mu [ U_mu(s) x(s+mu) - U_mu^+(s-mu) x(s-mu) ]  (= a r + b x + 2D x) */
int qexhip_stag_dslash(qexhip_handle h, double *r, const double *x, int parity, double a, double b);

/* stagD (src/physics/stagD.nim:406-409) on both parities = Staggered.D (sc=+1, :566-568) and
 * Staggered.Ddag (sc=-1, :569-571):  r = m*x + sc*D*x */
int qexhip_stag_D(qexhip_handle h, double *r, const double *x, double m, double sc);

/* stagD itself (src/physics/stagD.nim:406-409) on ONE subset (parity QEXHIP_EVEN / ODD / ALL): r[subset] = a*r + m*x + sc*D*x,
 * the rest of r kept.  stagDb (:425-427, no final scale) is qexhip_stag_dslash(h, r, x, parity, 0, m / (0.5 sc)). */
int qexhip_stag_stagD(qexhip_handle h, double *r, const double *x, int parity, double m, double sc, double a);

/* stagD with the accumulate coefficient: r = a*r + m*x + sc*D*x on both parities; a = 1, sc = -1 is
 * Staggered.peqDdag (src/physics/stagD.nim:572-574) */
int qexhip_stag_D_acc(qexhip_handle h, double *r, const double *x, double m, double sc, double a);

/* stagD2ee / stagD2oo (src/physics/stagD.nim:434-469): r[par] = 4 m2 x - (2D_eo)(2D_oe) x */
int qexhip_stag_op_xx(qexhip_handle h, double *r, const double *x, double m2, int par_even);

/* eoReconstruct (src/physics/stagD.nim:583-586): r.odd = (b.odd - D_oe r.even)/m, r.even kept */
int qexhip_stag_eo_reconstruct(qexhip_handle h, double *r, const double *b, double m);

/* eoReduce (src/physics/stagD.nim:575-581): r.even = (D^+ b).even = (m b - D b).even, r.odd kept */
int qexhip_stag_eo_reduce(qexhip_handle h, double *r, const double *b, double m);

/* Shifted outer product of the fermion force:
 *   f[mu](s) (+)= scale(parity of s) * x(s) (x) x(s+mu)^+     f: double[vol][4][3][3][2]
 * stagDeriv (src/physics/stagD.nim:634-664) is scale_even = +1, scale_odd = -1, accumulate = 1 (the
 * caller then rephases f); the loop of fforce (src/stagg_pv_hmc/staghmc_spv.nim:831-854) is
 * scale_even = scale_odd = scale with accumulate = 0 for the first field and 1 afterwards. */
int qexhip_stag_outer(qexhip_handle h, double *f, const double *x, double scale_even, double scale_odd,
                      int accumulate);

/* ---------------- solvers ----------------
 * solveEE / solveOO = solveXX (src/physics/stagSolve.nim:57-138), the backend seam next to
 * sbQuda (:105-118 -> qudaSolveEE/OO, src/quda/qudaWrapperImpl.nim:263-267).
 * On `par_even ? even : odd` sites solve  4(m^2 - D_eo D_oe) x = b  from x = 0 with the CG of
 * src/solvers/cg.nim:55-272; stop when |r|^2 <= r2req*|b_par|^2 or after maxits iterations.
 * x is zeroed on both parities first (stagSolve.nim:63-64).
 *   iters          <- sp.iterations (cg.nim:271)
 *   r2_over_b2     <- final recursive |r|^2/|b|^2
 *   hist[k]        <- |r|^2/|b|^2 after iteration k (k = 0 initial), the values of the
 *                     "CG iteration: k  r2/b2:" log lines (cg.nim:172,215-217); at most histcap. */
int qexhip_stag_solve_xx(qexhip_handle h, double *x, const double *b, double mass, double r2req,
                         int maxits, int par_even, int *iters, double *r2_over_b2,
                         double *hist, int histcap);

/* Staggered.solve (src/physics/stagSolve.nim:224-294): full-lattice D x = b by even-odd
 * preconditioning with the outer true-residual restart loop, x starts from 0.
 *   iters <- total CG iterations, r2_final <- |b - D x|^2/|b|^2 (sp.r2) */
int qexhip_stag_solve(qexhip_handle h, double *x, const double *b, double mass, double r2req,
                      int maxits, int *iters, double *r2_final);

/* the same with sp.usePrevSoln (src/physics/stagSolve.nim:234-243): with use_prev != 0 the solve
 * starts from the x handed in (r = b - D x) instead of x = 0 */
int qexhip_stag_solve_prev(qexhip_handle h, double *x, const double *b, double mass, double r2req,
                           int maxits, int use_prev, int *iters, double *r2_final);

/* Mixed-precision solves: SolverParams.sloppySolve (src/solvers/solverBase.nim:8-15), what QEX's GPU backend turns into a
 * QUDA solve with reliable updates (src/quda/qudaWrapperImpl.nim:194-197, reliable_delta = 0.1).
 *   sloppy = 0 (SloppyNone)   the fp64 CG: exactly qexhip_stag_solve_xx / qexhip_stag_solve_prev / qexhip_dev_solve_xx
 *   sloppy = 1 (SloppySingle) CG iterations in fp32 (fp32 links and fields, fp32 Dslash sweeps, reductions in double), with
 *                             reliable updates: x, b and the true residual b - A x in fp64 whenever |r_s|^2 has fallen by
 *                             delta^2 = 0.01 since the last one, when the fp32 residual says converged, and at maxits
 *   sloppy = 2 (SloppyHalf)   with option "half" = 0 (the default) runs single, bit for bit.  With "half" = 1 the single-system
 *                             entries below, qexhip_dev_solve_xx_sloppy and the single-system deflated entries iterate on 16-bit
 *                             storage: r_s, p_s, Ap_s as six int16 + one fp32 norm per site (qexhip_half_pack_host), the links
 *                             as int16 (qexhip_stag_links_info_half), fp32 arithmetic, the increment of x in fp32, the same
 *                             reliable updates and the same stop on the true fp64 residual.  If "half_stall" reliable updates in
 *                             a row do not lower the true residual the solve finishes in fp32 (qexhip_stag_sloppy_last says so;
 *                             iters and nupdates are then the sums).  With option "half_batch" = 1 (default 0, independent of
 *                             "half") the lock-step batched entries -- qexhip_stag_solve_xx_batch_sloppy,
 *                             qexhip_stag_solve_batch_sloppy, qexhip_dev_solve_batch_sloppy and the deflated batches -- run the
 *                             same 16-bit solve for up to four systems in lock-step on one stream of the int16 links: every
 *                             system returns the bits of its single-system 16-bit solve, stall guard and fp32 finish included
 *                             (qexhip_stag_sloppy_last_batch).  With "half_batch" = 0 the batches run single for sloppy = 2;
 *                             multi-shift solves run single for sloppy = 2 whatever the options say.  t-sharded contexts (or
 *                             ghost zones forced on one rank): the single-system 16-bit solve runs there as on one rank -- the
 *                             faces travel in the 16-bit format, 16 B per site; the int16 links are scaled by the largest
 *                             |entry| of the whole lattice; every rank takes the same updates, the same stall decision and the
 *                             same fp32 finish --; the sloppy batches are refused there unless option "batch_ranks" is 1
 *                             (qexhip_stag_solve_xx_batch_sloppy below)
 * The solve stops on the TRUE (fp64) residual: r2_over_b2 is |b - A x|^2/|b|^2 of the returned x (solveXX); iters counts fp32
 * iterations; nupdates (may be NULL) receives the number of reliable updates, the last one that confirmed convergence included
 * (0 for sloppy = 0).  iters == maxits is not an error.  QEXHIP_ERR_ARG for sloppy outside 0..2.
 * t-sharded contexts: each rank passes its slab, as with the fp64 entries, and the call is collective.  The fp32 faces travel on the
 * context's transport (half the bytes of the fp64 ones), every reduction is rank-global, and every rank returns the same iters,
 * r2 and nupdates; the sharded fp32 operator gives the one-rank operator's bits site for site.  The fp32 copy of the links is
 * built on first use and rebuilt whenever the operator's links have changed since (any set_links variant, t-sharding by
 * qexhip_comm_force_halo); its storage format is the one the whole lattice would get (largest deviation over the ranks);
 * qexhip_release_workspace frees it. */
int qexhip_stag_solve_xx_sloppy(qexhip_handle h, double *x, const double *b, double mass, double r2req, int maxits,
                                int par_even, int sloppy, int *iters, double *r2_over_b2, int *nupdates);
int qexhip_stag_solve_sloppy(qexhip_handle h, double *x, const double *b, double mass, double r2req, int maxits,
                             int use_prev, int sloppy, int *iters, double *r2_final, int *nupdates);
/* What the last single-system sloppy solve (the two entries above, qexhip_dev_solve_xx_sloppy, the single-system deflated entries)
 * ran: precision = 1 single, 2 16-bit storage (0: none yet); the iterations it spent on 16-bit storage and in fp32, summed over the
 * inner solves of a full solve (half_iters + f32_iters = iters); fell_back = 1 if the stall guard of a 16-bit solve handed over
 * to fp32.  Any pointer may be NULL. */
int qexhip_stag_sloppy_last(qexhip_handle h, int *precision, int *half_iters, int *f32_iters, int *fell_back);
/* The same per system for the last BATCHED sloppy call (the lock-step batched entries with sloppy > 0, the deflated batches): *n <- the
 * number of systems of that call; the arrays hold n_max entries, of which the first min(*n, n_max) are written; sums over the inner
 * batches of a full solve.  precision[j] = 0: system j ran no sloppy iteration (finished by the start or by the deflation).  The
 * batched entries do not touch qexhip_stag_sloppy_last's report, nor the single-system entries this one.  Any pointer may be NULL. */
int qexhip_stag_sloppy_last_batch(qexhip_handle h, int n_max, int *n, int *precision, int *half_iters, int *f32_iters, int *fell_back);
/* The 16-bit vector format on the host, for nsites sites of 6 doubles (re, im of three colours): norm[i] = fp32 of the largest
 * |component| of site i, q[6 i + k] = rint(v 32767 / norm[i]) formed in double; a site whose norm is below the smallest normal
 * fp32 number is all zeros.  unpack: v = q norm / 32767.  Needs no device.  QEXHIP_ERR_ARG for a site that is not finite in fp32. */
int qexhip_half_pack_host(const double *v, size_t nsites, int16_t *q, float *norm);
int qexhip_half_unpack_host(const int16_t *q, const float *norm, size_t nsites, double *v);

/* multi-shift solveXX (src/physics/stagSolve.nim:296-345 + src/solvers/cgm.nim:84-315).
 * shifts[0] = base mass, shifts[k>0] = sigma_k added to the base operator 4 m0^2 - (2D)(2D) (i.e. shift k is that operator at
 * m_k^2 = m0^2 + sigma_k / 4); xs[k] full-volume vectors.  fp64 throughout; the stop is the BASE system's iterated residual, the
 * shifted systems follow it through the zeta recurrences and their residuals are not checked.  The mixed-precision form, which
 * checks every shift's true residual, is qexhip_stag_solve_xx_multi_sloppy below. */
int qexhip_stag_solve_xx_multi(qexhip_handle h, double *const *xs, const double *b,
                               const double *shifts, int nmass, double r2req, int maxits,
                               int par_even, int *iters, double *hist, int histcap);
/* Staggered.solve(xs, b, ms, sp) (src/physics/stagSolve.nim:347-446) */
int qexhip_stag_solve_multi(qexhip_handle h, double *const *xs, const double *b,
                            const double *masses, int nmass, double r2req, int maxits,
                            int *iters, double *r2_final);
/* Mixed-precision multi-shift solves (QUDA's scheme).  sloppy as qexhip_stag_solve_xx_sloppy: 0 IS the fp64 entry above (nupdates = 0,
 * refine_iters all 0, r2_over_b2 all -1: the fp64 solver does not compute them), 1 single, 2 runs single.  QEXHIP_ERR_ARG before
 * anything is launched for sloppy outside 0..2, for base mass 0 with sloppy > 0, and for nmass outside 1..32.
 * Phase 1: the multi-shift CG with r, Ap, all nmass search directions and solution increments in fp32 (vectors in units of |b| for
 * the whole solve), the zeta recurrences in double, and reliable updates on the base system as in the single solve (all shifts'
 * increments flushed into the fp64 x_k in one launch, r = b - A_0 x_0 recomputed in fp64); it ends when the base system's TRUE
 * residual is <= r2req |b|^2, or at maxits.  Phase 2: for every k >= 1 the true r_k = b - A_k x_k is computed in fp64; a shift with
 * |r_k|^2 > r2req |b|^2 is refined by a sloppy CG on A_k d = r_k (own maxits; one rank without ghost zones: lock-step batches of up
 * to 4 shifts, else one shift at a time) and |r_k|^2 recomputed once.
 *   iters          fp32 iterations of phase 1
 *   r2_over_b2[k]  the true |b - A_k x_k|^2 / |b|^2 of the returned x_k (nmass values)
 *   nupdates       reliable updates of phase 1 (may be NULL)
 *   refine_iters   nmass values (may be NULL): fp32 iterations spent refining shift k (0: not refined; [0] is always 0)
 * t-sharded: collective, every rank returns the same values.  qexhip_release_workspace frees the fp32 fields. */
int qexhip_stag_solve_xx_multi_sloppy(qexhip_handle h, double *const *xs, const double *b, const double *shifts, int nmass,
                                      double r2req, int maxits, int par_even, int sloppy, int *iters, double *r2_over_b2,
                                      int *nupdates, int *refine_iters);
/* qexhip_stag_solve_multi with the inner multi-shift solveXX in mixed precision (every shift of every inner solve refined to the
 * inner target); the outer loop and the return values are the fp64 entry's; nupdates: the updates of all inner solves. */
int qexhip_stag_solve_multi_sloppy(qexhip_handle h, double *const *xs, const double *b, const double *masses, int nmass,
                                   double r2req, int maxits, int sloppy, int *iters, double *r2_final, int *nupdates);

/* ---------------- field algebra hooks ----------------
 * norm2 / redot with fp64 accumulation (src/field/fieldET.nim:605-625,704-724) and the
 * elementwise updates CG uses (fieldET.nim:547-598).  On host vectors; for tests. */
int qexhip_norm2(qexhip_handle h, const double *x, int parity, double *out);
int qexhip_redot(qexhip_handle h, const double *x, const double *y, int parity, double *out);
/* dotP (src/field/fieldET.nim:677-693): the complex inner product sum_s x(s)^+ y(s); out[0] = Re, out[1] = Im */
int qexhip_dot(qexhip_handle h, const double *x, const double *y, int parity, double out[2]);
/* y[parity] += a*x */
int qexhip_axpy(qexhip_handle h, double a, const double *x, double *y, int parity);
/* y[parity] = x + a*y */
int qexhip_xpay(qexhip_handle h, const double *x, double a, double *y, int parity);

/* ---------------- device-resident fields ----------------
 * QEX re-uploads per call through the QUDA seam; these keep vectors in HBM between calls
 * (the "set once per trajectory" extension of SURVEY.md 8b "Ownership"). Fields are
 * full-volume colour vectors identified by small integer ids. */
int qexhip_field_new(qexhip_handle h, int *id);
int qexhip_field_free(qexhip_handle h, int id);
int qexhip_field_upload(qexhip_handle h, int id, const double *host);
int qexhip_field_download(qexhip_handle h, int id, double *host);
int qexhip_field_zero(qexhip_handle h, int id);
/* asynchronous on the context stream; qexhip_sync() to wait */
int qexhip_dev_dslash(qexhip_handle h, int r_id, int x_id, int parity, double a, double b);
int qexhip_dev_op_xx(qexhip_handle h, int r_id, int x_id, double m2, int par_even);
/* solveXX on resident fields; blocks until finished. */
int qexhip_dev_solve_xx(qexhip_handle h, int x_id, int b_id, double mass, double r2req,
                        int maxits, int par_even, int *iters, double *r2_over_b2,
                        double *hist, int histcap);
/* qexhip_stag_solve_xx_sloppy on resident fields */
int qexhip_dev_solve_xx_sloppy(qexhip_handle h, int x_id, int b_id, double mass, double r2req, int maxits, int par_even,
                               int sloppy, int *iters, double *r2_over_b2, int *nupdates);
/* the fp32 operator of the sloppy solve on resident fp64 fields: r[par] = f64(4 m2 x32 - (2D)(2D) x32), x32 = f32(x[par]), with
 * the fp32 links and the fp32 sweep the sloppy CG iterates with; t-sharded: collective, on each rank's slab */
int qexhip_dev_op_xx_sloppy(qexhip_handle h, int r_id, int x_id, double m2, int par_even);
/* format of the fp32 link copy (building it if stale): 0 = 18 reals, 1 = rows 0,1 + sign (every link +-SU(3) to 1e-6); max_dev =
 * the largest deviation of a stored row 2 from the sign-format rebuild (0 when the sign format is capped off by "recon" = 0); t-sharded:
 * the maximum over the ranks, and collective when the copy is rebuilt */
int qexhip_stag_links_info_f32(qexhip_handle h, int *format, double *max_dev);
/* the 16-bit counterpart of qexhip_dev_op_xx_sloppy: x[par] rounded to the 16-bit vector format, the two 16-bit sweeps (their
 * intermediate and result stored in the format), the result back in fp64.  t-sharded: collective, each rank's slab of the one-rank
 * result bit for bit */
int qexhip_dev_op_xx_half(qexhip_handle h, int r_id, int x_id, double m2, int par_even);
/* the batched form: n <= 4 fields x_ids[j][par] rounded to the format, ONE batched operator (two multi-right-hand-side 16-bit sweeps that
 * stream the links once for all systems) at m2[j], the results back in fp64 in r_ids[j][par]; per system the bits of qexhip_dev_op_xx_half */
int qexhip_dev_op_xx_half_batch(qexhip_handle h, int n, const int *r_ids, const int *x_ids, const double *m2, int par_even);
/* the fp32 twin: n <= 4 fields rounded to fp32, ONE batched fp32 operator (two multi-right-hand-side fp32 sweeps) at m2[j], the
 * results back in fp64; per system the bits of qexhip_dev_op_xx_sloppy.  Both batched probes run on one rank without ghost zones,
 * and refuse t-sharded contexts (QEXHIP_ERR_ARG) unless option "batch_ranks" is 1: then they are collective, all systems' faces
 * travel in one exchange per sweep, and every system's slab is the slab of the one-rank single-system result, bit for bit */
int qexhip_dev_op_xx_sloppy_batch(qexhip_handle h, int n, const int *r_ids, const int *x_ids, const double *m2, int par_even);
/* the 16-bit link copy (building it if stale, behind the fp32 copy whose format decision it shares): format 1 = rows 0,1 as int16
 * of u 32767 (clamped) + the fp32 copy's sign masks, 48 B per forward/backward pair; format 0 = 18 reals as int16 of u 32767 / s,
 * 72 B per pair, s = *s_fat for the one-hop links and *s_long for the Naik links: the largest |entry| of each kind (reported in
 * either format; 0 without Naik links).  max_dev as qexhip_stag_links_info_f32.  t-sharded: format, *s_fat and *s_long are those of
 * the whole lattice (maxima over the ranks), and the call is collective when the copy is rebuilt */
int qexhip_stag_links_info_half(qexhip_handle h, int *format, double *s_fat, double *s_long, double *max_dev);
/* Re-entry of the CG on the state the last qexhip_dev_solve_xx (or re-entry) on x_id left behind -- CgState.solve called
 * again with b2 >= 0 (src/solvers/cg.nim:21-27,85,133,155-161,256-261): no set-up, r / p / rzold kept, the stopping
 * criterion comes from the new r2req / maxits, `iters` goes on counting from where the last call stopped (maxits is the
 * cumulative limit, as sp.maxits is there).  QEXHIP_ERR_STATE if anything that uses the CG's work vectors or changes the
 * operator ran in between.  hist (may be NULL) receives the whole history from iteration 0. */
int qexhip_dev_solve_xx_continue(qexhip_handle h, int x_id, double r2req, int maxits, int *iters, double *r2_over_b2,
                                 double *hist, int histcap);
/* multi-shift solveXX (Staggered.solveXX(xs, b, ms, sp), src/physics/stagSolve.nim:296-345) on resident fields:
 * x_ids[k] receives the solution of shift k; shifts as qexhip_stag_solve_xx_multi.  Blocks until finished. */
int qexhip_dev_solve_xx_multi(qexhip_handle h, const int *x_ids, int b_id, const double *shifts, int nmass,
                              double r2req, int maxits, int par_even, int *iters, double *hist, int histcap);
/* qexhip_stag_solve_xx_multi_sloppy on resident fields (x_ids distinct, none of them b_id) */
int qexhip_dev_solve_xx_multi_sloppy(qexhip_handle h, const int *x_ids, int b_id, const double *shifts, int nmass, double r2req,
                                     int maxits, int par_even, int sloppy, int *iters, double *r2_over_b2, int *nupdates,
                                     int *refine_iters);
/* Rational functions of the one-parity operator (the rooted staggered action; restates the rooted field of
 * src/mcmc/fields/staggeredFields.nim:58-95,191-230 on M^+M, see DESIGN.md "Rooted HISQ").
 *   M^+M = m^2 - D_eo D_oe on the even sites (par_even; parities swapped otherwise) = A(m)/4, A the operator of qexhip_dev_op_xx.
 *   r(x) = f0 + sum_{k<nterm} alpha[k] / (x + beta[k]).
 * out[par] = r(M^+M) b[par]; the other parity of out is zeroed.  ONE multi-shift solve: the terms are sorted by beta, the base
 * mass is m_0 = sqrt(mass^2 + beta_min), the shifts are sigma_k = 4 (beta_k - beta_min) in the convention of
 * qexhip_dev_solve_xx_multi ((A(m_0) + sigma_k) y_k = b), and out = f0 b + sum_k 4 alpha[k] y_k.  No y_k is ever stored: the update
 * kernel accumulates the sum (2 vector streams per shift instead of 4) and the workspace is nterm search directions plus work
 * fields.  fp64 only.  Stop criterion: the BASE system's iterated residual |r_0|^2 <= r2req |b|^2, as in the fp64 multi-shift
 * solve; iters and hist are bit for bit those of qexhip_dev_solve_xx_multi with shifts [m_0, sigma_1, ...].
 * QEXHIP_ERR_ARG before anything is launched: nterm outside 1..32, mass^2 + beta_min <= 0, non-finite mass / f0 / alpha / beta,
 * out_id == b_id, unknown ids, NULL arrays.  beta[k] = 0 and repeated beta are legal.  t-sharded: collective.
 * qexhip_stag_rational_xx is the host-pointer twin (b up, out down; out != b). */
int qexhip_dev_rational_xx(qexhip_handle h, int out_id, int b_id, double mass, double f0, int nterm, const double *alpha,
                           const double *beta, double r2req, int maxits, int par_even, int *iters, double *hist, int histcap);
int qexhip_stag_rational_xx(qexhip_handle h, double *out, const double *b, double mass, double f0, int nterm, const double *alpha,
                            const double *beta, double r2req, int maxits, int par_even, int *iters, double *hist, int histcap);

/* Free the multi-shift solvers' persistent workspace (up to 3 x nmass full fields kept between solves; QEX allocates its
 * ps / ys per call with newOneOf and leaves them to the GC, src/solvers/cgm.nim:120-131, src/physics/stagSolve.nim:376-381).
 * The next multi-shift solve allocates it again.  Also frees the double-link field of the rectangle force / Symanzik flow
 * (one more field the size of the links, rebuilt at the next such call). */
int qexhip_release_workspace(qexhip_handle h);
/* norm2 / redot (src/field/fieldET.nim:605-625,704-724; rank-global sums) and Staggered.D / Ddag (r = m x + sc D x, r_id != x_id)
 * on resident fields: what a caller that keeps its vectors in HBM uses for true residuals and solution norms. */
int qexhip_dev_norm2(qexhip_handle h, int x_id, int parity, double *out);
int qexhip_dev_redot(qexhip_handle h, int x_id, int y_id, int parity, double *out);
int qexhip_dev_dot(qexhip_handle h, int x_id, int y_id, int parity, double out[2]);     /* dotP on resident fields */
int qexhip_dev_D(qexhip_handle h, int r_id, int x_id, double m, double sc);
/* r[parity] := 0 (the `phi.odd := 0` of the pseudofermion refresh, staghmc_sh.nim:748-755) */
int qexhip_dev_zero(qexhip_handle h, int id, int parity);
/* n x Staggered.solve (qexhip_stag_solve semantics per system) on resident fields, lock-step batches of four on the
 * operator's current links: faction / pbp of the HMC drivers without moving a vector (staghmc_sh.nim:260-272,339-364) */
int qexhip_dev_solve_batch(qexhip_handle h, int n, const int *x_ids, const int *b_ids, const double *mass,
                           const double *r2req, int maxits, int *iters, double *r2);
/* qexhip_stag_solve_batch_sloppy (below) on resident fields: ONE lock-step batch, n in 1..4 (t-sharded with sloppy > 0: option
 * "batch_ranks", as there) */
int qexhip_dev_solve_batch_sloppy(qexhip_handle h, int n, const int *x_ids, const int *b_ids, const double *mass,
                                  const double *r2req, int maxits, int sloppy, int *iters, double *r2_final, int *nupdates);

/* ---------------- meson correlators on resident fields ----------------
 * Local staggered mesons from point-source propagators (src/observables/fpvaMeas.nim, tests/examples/testStagProp.nim).
 * Tables are rank-global and returned on the host; on a t-sharded context every rank receives the whole table.
 *
 * stagLocalMesons (fpvaMeas.nim:33-61) summed over n <= 4 field pairs in one launch, both parities:
 *   out[tt*8 + s] = sum_k sum_{x: (t(x) - t0) mod nt = tt, corner(x) = s} Re<x_k(x), y_k(x)>,  corner = (x0&1) | (x1&1)<<1 | (x2&1)<<2
 * with t the global time coordinate and nt the global t extent; out holds nt*8 doubles.  stagMesons(v)
 * (src/physics/stagMesonLocal.nim:14-51) is x = y = v, t0 = 0.  The summation order is fixed and every entry is computed on the
 * rank that owns its time slice: the table is bit-identical run to run and for any number of ranks. */
int qexhip_dev_meson_corners(qexhip_handle h, int n, const int *x_ids, const int *y_ids, int t0, double *out);
/* symShift (fpvaMeas.nim:16-31): r(x) = U_mu(x) x(x+mu) + U_mu(x-mu)^+ x(x-mu) for mu = 0, 1, 2 on both parities, r_id != x_id.
 * U are the operator's one-hop links as qexhip_stag_set_links* left them (with boundary conditions and staggered phases: for
 * newStag(g) the rephased g that fpvaMeas shifts with; for HISQ or nHYP operators the SMEARED one-hop links).  mu = 3 is refused:
 * the reference shifts spatially only. */
int qexhip_dev_sym_shift(qexhip_handle h, int r_id, int x_id, int mu);
/* norm2slice (src/observables/sources.nim:10-18): out[v] = sum_{x: x_dir = v} |f(x)|^2 over the global extent of dir (dir 0..3) */
int qexhip_dev_norm2slice(qexhip_handle h, int id, int dir, double *out);

/* ---------------- stochastic scalar trace on resident fields ----------------
 * The pieces of src/observables/scalarTrace.nim (disconnected pbp: Tr (D+m)^-1(x,x) from diluted noise sources) between the noise
 * fill (qexhip_rng_dev_*_vector) and the batched solves (qexhip_dev_solve_batch*).
 *
 * A "cfield" is a resident complex site field (lo.Complex, 16 B per site), identified by small positive ids of its own.  It is
 * created zeroed; scale multiplies every site by the real s; download returns [site][2] (re, im) in the site order of
 * qexhip_field_download (V=1 even-odd order of the rank-local lattice).  qexhip_finalize frees what is left. */
int qexhip_cfield_new(qexhip_handle h, int *id);
int qexhip_cfield_free(qexhip_handle h, int id);
int qexhip_cfield_zero(qexhip_handle h, int id);
int qexhip_cfield_scale(qexhip_handle h, int id, double s);
int qexhip_cfield_download(qexhip_handle h, int id, double *host);
/* dst += a * src on every site, both components (product and sum rounded as written); dst != src, a finite */
int qexhip_cfield_axpy(qexhip_handle h, int dst, double a, int src);
/* Time + pattern dilution (src/algorithms/dilution.nim, scalarTrace.nim:169-185) of src into n <= 4 colour vectors in one launch:
 *   dst_k(x) = scale * src(x)  where the GLOBAL time of x is t[k] and x belongs to pattern idx[k];  +0.0 elsewhere
 * kind 0 (EO):     idx in 0..1, the global parity (x0+x1+x2+t)&1
 * kind 1 (CORNER): idx in 0..7, (x0&1) | (x1&1)<<1 | (x2&1)<<2
 * The destinations are distinct fields, none of them src.  On a t-sharded context a rank that does not own t[k] zeroes dst_k. */
int qexhip_dev_dilute(qexhip_handle h, int n, const int *dst_ids, int src_id, int kind, const int *idx, const int *t, double scale);
/* trce(x) += coef * sum_colour conj(a_k(x)) b_k(x) for k = 0..n-1 (n <= 4) in one launch; the n terms are added one at a time in
 * ascending k, so the result is bit for bit that of n calls with one pair each.  a_ids[k] == b_ids[k] (the improved trace
 * mass * phi.dot phi, scalarTrace.nim:195-198) loads the vector once and adds an imaginary part of exactly 0. */
int qexhip_dev_trace_accum(qexhip_handle h, int cfield, int n, const int *a_ids, const int *b_ids, double coef);
/* out[2*t], out[2*t+1] = Re, Im of the sum of the cfield over the global time slice t; out holds 2 * (global t extent) doubles.
 * Rank-global; the summation order is fixed and every entry is computed on the rank that owns its slice, so the table is
 * bit-identical run to run and for any number of ranks. */
int qexhip_dev_cfield_slices(qexhip_handle h, int cfield, double *out);

/* ---------------- connected scalar correlator from point sources on resident fields ----------------
 * The pieces of src/observables/conn4d.nim (the connected part of the flavour-singlet scalar) around the batched solves
 * (qexhip_dev_solve_batch*); `locmes` is a cfield of the section above, est[t] the Re column of qexhip_dev_cfield_slices.
 * Coordinates are GLOBAL (x, y, z, t), pts[4*k + mu]; a coordinate outside the global lattice, a colour outside 0..2, n outside
 * 1..4 or an unknown id is QEXHIP_ERR_ARG before anything is written.
 *
 * pointSource (conn4d.nim:173-182) for n <= 4 distinct colour vectors in one launch: field ids[k] := 0 on every site, then 1 + 0i
 * in colour ic[k] at pts[k].  On a t-sharded context only the rank that owns pts[k][3] stores the one. */
int qexhip_dev_point_source(qexhip_handle h, int n, const int *ids, const int *pts /* n x 4, global */, const int *ic);
/* Re cfield(x) += scal * |phi_k(x (+) pts_k)|^2 for k = 0..n-1 (n <= 4), (+) the coordinate-wise sum wrapped over the global
 * extents: conn4d.nim:223-229, whose `translate` (:184-195) shifts forward pts[mu] times, so the source point lands on the origin.
 * |phi|^2 is the fma chain of qexhip_dev_trace_accum with a == b, then w = scal * n2, then acc += w, the n terms one at a time in
 * ascending k: the result is bit for bit that of n calls with one system each.  The imaginary part is not touched.  Odd
 * coordinates are allowed.  On a t-sharded context w (8 B per site) travels through one all-gather and every rank's slab equals
 * the one-rank result bit for bit. */
int qexhip_dev_conn_accum(qexhip_handle h, int cfield, int n, const int *phi_ids, const int *pts /* n x 4, global */, double scal);
/* cfield(x) *= (-1)^(x0+x1+x2), both components, in place (conn4d.nim:238-245) */
int qexhip_cfield_stag_sign(qexhip_handle h, int cfield);

/* ---------------- low modes of the even/odd operator and deflated solves ----------------
 * src/eigens/hisqev.nim: the lowest singular pairs (sv_i, v_i) of D_oe on the even sites (`hisqev` with EigOpts, hisqev.nim:380-560,
 * block Lanczos of src/eigens/svdLanczos.nim + Rayleigh-Ritz passes), and the deflated solveEE of its main program (:653-705).
 * Everything here lives on the EVEN sites (the deflated batch below also deflates odd-parity solves, from the same even basis).  The operator is H = -D_eo D_oe in this header's normalisation: qexhip_dev_op_xx(r, x, m2, 1)
 * is 4 (m2 + H) x.  Eigenvalues are lambda_i = sv_i^2.  Whatever links the operator currently holds define H (newStag, newStag3, HISQ,
 * nHYP).
 *
 * A BASIS is a resident set of nvecs half-volume vectors (even body sites only: half the memory of a field), identified by a small
 * id like fields.  It remembers the links it was computed (or last written) on: using it after any set_links variant is
 * QEXHIP_ERR_STATE in the deflated solves.  nvecs <= QEXHIP_EIG_MAX_NVECS (the largest m of the in-place rotation), else
 * QEXHIP_ERR_ARG.  qexhip_release_workspace frees the eigensolver's work fields, never a basis; qexhip_finalize frees the bases.
 *   get_vector / set_vector   field_id.even := v_i  /  v_i := field_id.even (the odd half of the field is not touched / not read)
 * The three block kernels, as hooks for tests (the linear algebra of src/eigens/linalgFuncs.nim on sets of vectors):
 *   block_dot    out[2 j], out[2 j + 1] = Re, Im of <v_{i0+j}, w.even>, j < n: one pass over the n vectors, w read once per 128 of them;
 *                fp64 accumulation in a fixed order (bit-identical run to run); t-sharded: ONE rank sum of 2 n doubles
 *   block_axpy   y.even += sum_j (coef[2 j] + i coef[2 j + 1]) v_{i0+j}: one pass over the n vectors, y read and written once
 *   rotate       V[:, 0:k] <- V[:, 0:m] Q in place, Q real m x k column-major (Q[j + m c]), 1 <= k <= m <= nvecs.  Vectors k .. m-1
 *                are LEFT AS THEY WERE (not zeroed, not orthogonal to the new ones): they are scratch afterwards.
 *   block_dot_multi   out[(k n + j) 2 + re|im] = <v_{i0+j}, w_k.even> for the nrhs (1..4) fields w_ids[k] in ONE pass over the n vectors
 *                (every basis element loaded once for all of them).  Each number is BIT FOR BIT what block_dot returns for w_k alone;
 *                t-sharded: ONE rank sum of 2 n nrhs doubles
 *   block_axpy_multi  y_k.even += sum_j (coef[(k n + j) 2] + i coef[(k n + j) 2 + 1]) v_{i0+j} for the nrhs distinct fields y_ids[k], one
 *                pass; each y_k is BIT FOR BIT what block_axpy gives with its own coefficients
 *   Bad vector ranges, nrhs outside 1..4 and repeated y_ids: QEXHIP_ERR_ARG before anything is launched. */
#define QEXHIP_EIG_MAX_NVECS 512
int qexhip_eig_new(qexhip_handle h, int nvecs, int *basis);
int qexhip_eig_free(qexhip_handle h, int basis);
int qexhip_eig_get_vector(qexhip_handle h, int basis, int i, int field_id);
int qexhip_eig_set_vector(qexhip_handle h, int basis, int i, int field_id);
int qexhip_eig_block_dot(qexhip_handle h, int basis, int i0, int n, int w_field_id, double *out);
int qexhip_eig_block_axpy(qexhip_handle h, int basis, int i0, int n, const double *coef, int y_field_id);
int qexhip_eig_rotate(qexhip_handle h, int basis, int m, int k, const double *Q);
int qexhip_eig_block_dot_multi(qexhip_handle h, int basis, int i0, int n, int nrhs, const int *w_ids, double *out /* [nrhs][n][2] */);
int qexhip_eig_block_axpy_multi(qexhip_handle h, int basis, int i0, int n, int nrhs, const double *coef /* [nrhs][n][2] */, const int *y_ids);
/* EigOpts (src/eigens/hisqev.nim: nev, nvecs, relerr, abserr, maxup) for the thick-restart Lanczos with Chebyshev acceleration:
 *   nev, nvecs     pairs wanted / size of the Krylov basis (= vectors of the basis object used), 1 <= nev <= nvecs <= QEXHIP_EIG_MAX_NVECS
 *   relerr, abserr a pair counts as converged when its residual |H v - lambda v| <= max(abserr, relerr * lambda)
 *   max_restarts   thick restarts allowed (maxup); reaching it is not an error
 *   cheb_degree    0: plain Lanczos on H; p > 0: Lanczos on T_p(s(H)), s mapping [cheb_lo, cheb_hi] onto [-1, 1]: cheb_lo is put
 *                  just above the wanted eigenvalues, cheb_hi at or above the top of the spectrum; cheb_hi = 0: estimated as 1.1 x the
 *                  largest Ritz value of 20 plain Lanczos steps
 *   seed           of the start vector (the device Gaussian generator, one stream per GLOBAL site: runs repeat, for any rank count) */
typedef struct qexhip_eig_opts {
  int nev, nvecs;
  double relerr, abserr;
  int max_restarts, cheb_degree;
  double cheb_lo, cheb_hi;
  unsigned long long seed;
} qexhip_eig_opts;
/* the option checks of qexhip_stag_eigs alone: QEXHIP_ERR_ARG or 0.  Host only, no handle. */
int qexhip_eig_check_opts(const qexhip_eig_opts *opts);
/* hisqev (src/eigens/hisqev.nim): the nev lowest eigenpairs of H into vectors 0 .. nev-1 of `basis` (nvecs <= the basis's size; the
 * other vectors are scratch), sorted ascending, each with |v_i| = 1.
 *   nconv      pairs with resid_i <= max(abserr, relerr * evals_i)
 *   evals[nev] Rayleigh quotients <v_i, H v_i>;  resid[nev] the TRUE residuals |H v_i - evals_i v_i|, recomputed with the fp64 operator
 *   stats[4]   (may be NULL) operator applications, restarts, Lanczos steps, true-residual checks
 * nconv < nev after max_restarts is not an error.  Bad options: QEXHIP_ERR_ARG before anything is launched.  t-sharded: collective,
 * every reduction rank-global, every rank returns the same numbers and holds its slab of every vector. */
int qexhip_stag_eigs(qexhip_handle h, int basis, const qexhip_eig_opts *opts, int *nconv, double *evals, double *resid, long stats[4]);
/* the Rayleigh quotients the basis holds for its leading n vectors (computing those it lacks: vectors written by set_vector) */
int qexhip_eig_evals(qexhip_handle h, int basis, int n, double *evals);
/* The deflated solveEE of hisqev.nim:653-705 (`rsolve`): x0 = sum_{i<nev} v_i <v_i, b> / (4 (lambda_i + m^2)); r0 = b - A x0 in fp64;
 * the EXISTING CG (sloppy = 0: qexhip_dev_solve_xx; 1: the mixed-precision one) on A d = r0 to r2req |b|^2 / |r0|^2; x = x0 + d.
 * iters = the CG's iterations; r2_over_b2 = the true |b - A x|^2 / |b|^2.  nev = 0 gives exactly the bits and the iteration count of
 * the undeflated entry.  Basis vectors are taken as orthonormal.  QEXHIP_ERR_STATE when the operator's links changed since the basis
 * was computed.  dev_: resident fields (x_id != b_id); stag_: host fields.  solve_deflated: Staggered.solve (qexhip_stag_solve_sloppy
 * semantics, use_prev = 0) whose inner solveEE calls deflate. */
int qexhip_dev_solve_xx_deflated(qexhip_handle h, int basis, int nev, int x_id, int b_id, double mass, double r2req, int maxits,
                                 int sloppy, int *iters, double *r2_over_b2);
int qexhip_stag_solve_xx_deflated(qexhip_handle h, int basis, int nev, double *x, const double *b, double mass, double r2req,
                                  int maxits, int sloppy, int *iters, double *r2_over_b2);
int qexhip_stag_solve_deflated(qexhip_handle h, int basis, int nev, double *x, const double *b, double mass, double r2req, int maxits,
                               int sloppy, int *iters, double *r2_final);
/* The deflated LOCK-STEP BATCH: the steps above for n (1..4) systems with their own masses, on EITHER parity, from the even basis.
 * D is anti-Hermitian, so H_e = -D_eo D_oe = D_oe^+ D_oe and H_o = D_oe D_oe^+: an even pair (v_i, lambda_i) with lambda_i > 0 gives the
 * odd pair (D_oe v_i / sqrt(lambda_i), lambda_i), and with A_o = 4 (m^2 + H_o) the odd projection is
 *   x0.odd = D_oe V diag(1 / (4 lambda_i (lambda_i + m^2))) V^+ (-D_eo b.odd)
 * (a mode with lambda_i <= 0 gets coefficient 0): two single-parity sweeps per system, no second basis.  The projections of all
 * systems are ONE block_dot_multi and ONE block_axpy_multi, so a system's starting guess is bit for bit the single deflated solve's;
 * a system with |b_k - A x0_k|^2 <= r2req_k |b_k|^2 is finished with 0 iterations, the others run as ONE lock-step batch CG (sloppy = 0:
 * the fp64 batch; > 0: the mixed-precision one, refused with QEXHIP_ERR_ARG on t-sharded contexts before anything is launched unless
 * option "batch_ranks" is 1, with which it runs there as qexhip_stag_solve_xx_batch_sloppy describes) on
 * A d_k = r0_k, then x_k = x0_k + d_k.  iters, r2_over_b2 (the TRUE residuals) and nupdates (may be NULL) are arrays of n; maxits is
 * shared.  nev = 0 is the undeflated batch entry itself: same bits, same iteration counts.  solve_batch_deflated: n x Staggered.solve
 * (qexhip_stag_solve_batch semantics: same ReconR / ReconL decisions, outer loop and maxits sharing) whose inner solveXX groups of BOTH
 * parities are this batch.  dev_: resident fields, no solution aliasing a source or another solution; stag_: host fields.
 * QEXHIP_ERR_STATE for a basis of other links.  The single-system deflated entries above are unchanged: their odd sources stay
 * undeflated. */
int qexhip_dev_solve_xx_batch_deflated(qexhip_handle h, int basis, int nev, int n, const int *x_ids, const int *b_ids, const double *mass,
                                       const double *r2req, int maxits, int par_even, int sloppy, int *iters, double *r2_over_b2,
                                       int *nupdates);
int qexhip_stag_solve_xx_batch_deflated(qexhip_handle h, int basis, int nev, int n, double *const *x, const double *const *b,
                                        const double *mass, const double *r2req, int maxits, int par_even, int sloppy, int *iters,
                                        double *r2_over_b2, int *nupdates);
int qexhip_dev_solve_batch_deflated(qexhip_handle h, int basis, int nev, int n, const int *x_ids, const int *b_ids, const double *mass,
                                    const double *r2req, int maxits, int sloppy, int *iters, double *r2_final, int *nupdates);
int qexhip_stag_solve_batch_deflated(qexhip_handle h, int basis, int nev, int n, double *const *x, const double *const *b,
                                     const double *mass, const double *r2req, int maxits, int sloppy, int *iters, double *r2_final,
                                     int *nupdates);
/* LOW-MODE AVERAGING of the scalar trace (no counterpart in src/observables/scalarTrace.nim: an opt-in extension).  With the pairs
 * (lambda_i, v_i) of a basis, i < nev, and w_i = D_oe v_i / sqrt(lambda_i) for lambda_i > 0, P is the orthogonal projector onto
 * span{(v_i, 0), (0, w_i)}: P = V V^+ on the even sites, P phi_o = -D_oe V diag(1/lambda) V^+ D_eo phi_o on the odd sites (a mode with
 * lambda_i <= 0 has no odd partner).  For exact pairs P commutes with D, and P (D+m)^-1 has the real site diagonal
 *   L(x) = sum_i m/(m^2 + lambda_i) |v_i(x)|^2  (x even),   sum_i m/(m^2 + lambda_i) |(D_oe v_i)(x)|^2 / lambda_i  (x odd),
 * |.|^2 summed over colour; sum_{x even} L = sum_{x odd} L = sum_i m/(m^2 + lambda_i).  With Q = 1 - P and phi_d = (D+m)^-1 eta_d,
 *   L(x) + sum_d m |(Q phi_d)(x)|^2      and      L(x) + sum_d conj(eta_d(x)) (Q phi_d)(x)
 * estimate m (M^+ M)^-1(x,x) with the low modes' part exact.  With eigenvectors of finite residual P is still an orthogonal projector
 * but no longer commutes with D: the estimators then carry a bias of the order of the eigenvector residuals.  lambda_i are the basis's
 * Rayleigh quotients (qexhip_eig_evals).
 *   block_norm2_accum  (test hook) cfield.even(c).re += sum_{j<n} wgt[j] sum_col |v_{i0+j}(c,col)|^2 in one pass over the n vectors, the
 *                cfield read and written once.  Vector after vector in ascending j: n2 by the fma chain of qexhip_dev_trace_accum with
 *                a == b, then re += wgt[j] * n2 (product and sum rounded as written), so the even sites are BIT FOR BIT those of
 *                get_vector(i0+j, f) + dev_trace_accum(cfield, f, f, wgt[j]) for j = 0..n-1.  Imaginary part and odd sites: untouched.
 *   lowmode_diag cfield.re += L(x) on both parities for the leading nev vectors: the even sites are block_norm2_accum with
 *                wgt_i = m/(m^2 + lambda_i); the odd sites take one D_oe sweep per vector with lambda_i > 0 and add
 *                wgt_i/lambda_i |D_oe v_i|^2 in ascending i.  t-sharded: collective (the sweeps' halo).
 *   project_out  phi_k <- (1 - P) phi_k in place on both parities for the n (1..4) distinct resident fields ids[k]: per parity ONE
 *                block_dot_multi and ONE block_axpy_multi, on the odd sites between a D_eo and a D_oe sweep per system; each field's
 *                result is bit for bit what it is alone.  t-sharded: collective.
 * Refused before anything is launched: mass not finite or <= 0, nev outside 0..nvecs, n outside 1..4, repeated or unknown ids
 * (QEXHIP_ERR_ARG); a basis of other links (QEXHIP_ERR_STATE).  nev = 0 changes nothing. */
int qexhip_eig_block_norm2_accum(qexhip_handle h, int basis, int i0, int n, const double *wgt, int cfield);
int qexhip_eig_lowmode_diag(qexhip_handle h, int basis, int nev, double mass, int cfield);
int qexhip_eig_project_out(qexhip_handle h, int basis, int nev, int n, const int *ids);
/* Dense real symmetric eigensolver on the host (cyclic Jacobi, no external library): what the eigensolver diagonalises at every
 * restart (the reference calls LAPACK there, src/eigens/lapack.nim).  a: n x n symmetric; w[n]: eigenvalues ascending; z (may be
 * NULL): n x n column-major, column i the unit eigenvector of w[i].  Needs no device. */
int qexhip_symeig_host(const double *a, int n, double *w, double *z);

/* ---------------- gauge field, plaquette, Wilson flow ----------------
 * qexhip_gauge_set/get: the `g` of src/gauge/wflow.nim:21 (unphased links, periodic). */
int qexhip_gauge_set(qexhip_handle h, const double *g);
int qexhip_gauge_get(qexhip_handle h, double *g);
/* plaq (src/gauge/gaugeUtils.nim:213-282): six values, index mu(mu-1)/2+nu, each /(V*6*nc) */
int qexhip_plaq(qexhip_handle h, double out[6]);
/* gaugeForce with GaugeActionCoeffs(plaq: cplaq) (src/gauge/gaugeAction.nim:334-350):
 * f_mu(x) = TAH( U_mu(x) * [ (cplaq/nc) sum_staples ]^+ ), written to host f */
int qexhip_gauge_force(qexhip_handle h, double *f, double cplaq);
/* gaugeFlow(steps, eps) (src/gauge/wflow.nim:21-67): RK3 Wilson flow of the resident gauge field */
int qexhip_wflow(qexhip_handle h, int nsteps, double eps);
/* The action-selectable variants used by the fork's flow driver (src/flow/flow.nim:22-90):
 *   kind 0 ("Wilson" | "rect"): GaugeActionCoeffs(plaq: cplaq, rect: c2), gaugeForce / gaugeActionDeriv
 *           incl. the rectangle part (src/gauge/gaugeAction.nim:148-350);
 *   kind 1 ("adj"):             GaugeActionCoeffs(plaq: cplaq, adjplaq: c2), forceA / gaugeADeriv (:683-747). */
int qexhip_gauge_force_general(qexhip_handle h, double *f, double cplaq, double c2, int kind);
int qexhip_wflow_general(qexhip_handle h, int nsteps, double eps, double cplaq, double c2, int kind);
/* EQ of the flow drivers (src/flow/gauge_flow.nim:360-379, tests/base/twflow_topo.nim:4-10):
 * out = {E_s, E_t, Q} from f = g.fmunu(loop), f.densityE, f.topoQ
 * (src/gauge/gaugeUtils.nim:1162-1271); loop in {1,3,4,5} selects the clover improvement
 * (1x1 | +2x2+3x3 | +2x2+1x2+1x3 | all five loop shapes, coefficients of :1128-1146). */
int qexhip_flow_EQ(qexhip_handle h, int loop, double out[3]);
/* What a flow loop measures after every step (src/flow/gauge_flow.nim:139-156,360-379; tests/base/twflow_topo.nim:4-10:
 * `g.plaq` and `EQ` = fmunu(1) -> densityE, topoQ) in ONE pass over the resident links: the plaquette of a plane is the
 * trace of one of the four clover leaves of that plane, so plaq[6] (as qexhip_plaq) and EQ[3] (as qexhip_flow_EQ with
 * loop = 1) come out of the same kernel. */
int qexhip_flow_measure(qexhip_handle h, double plaq[6], double EQ[3]);
/* The remaining gauge-sector pieces an HMC trajectory needs, on the resident field (set with qexhip_gauge_set):
 *   action: gc.gaugeAction1(g) (crect) / gc.actionA(g) (cadjplaq) (src/gauge/gaugeAction.nim:61-142,614-681),
 *           coefficients as GaugeActionCoeffs(plaq, rect | adjplaq); at most one of crect, cadjplaq non-zero
 *   update: mdt, g[mu][s] := exp(t p[mu][s]) g[mu][s] (src/examples/staghmc_sh.nim:429-435); p host, [vol][4][3][3][2]
 *   reunit: g.projectSU (src/gauge/gaugeUtils.nim:1333-1334; `reunit` of the HMC examples, staghmc_sh.nim:247-258)
 *   wline:  g.wline(path) (gaugeUtils.nim:1079-1112): volume- and colour-averaged trace, out = {re, im}; path entries
 *           +-(mu+1); the Polyakov loops of `ploop` are path = [mu+1] * L_mu (staghmc_sh.nim:281-291).  On a t-sharded
 *           field: paths that stray at most 3 slices in t, or the straight line [+-4] * L_t (global) */
int qexhip_gauge_action(qexhip_handle h, double cplaq, double crect, double cadjplaq, double *out);
int qexhip_gauge_update(qexhip_handle h, const double *p, double t);
int qexhip_gauge_reunit(qexhip_handle h);
int qexhip_wline(qexhip_handle h, const int *path, int n, double out[2]);
/* the four Polyakov loops wline([mu+1] * L_mu), mu = 0..3, of the resident field in one call: what `meas_ploop`
 * (src/flow/gauge_flow.nim:137-156) and `ploop` (src/examples/staghmc_sh.nim:281-291) compute with four g.wline calls;
 * out[2 mu], out[2 mu + 1] = Re, Im (normalised like qexhip_wline: trace / 3, lattice average) */
int qexhip_polyakov_loops(qexhip_handle h, double out[8]);
/* `s4_gauge` of the fork's measurements (src/stagg_pv_hmc/staghmc_spv_meas.nim:25-65; the pure-gauge S4 order parameter of
 * arXiv:1111.2317, printed as "MEASplaq <dir>-dir even/odd"): the plaquette of plane (mu, nu) at x is added to peo[mu][x_mu mod 2]
 * and peo[nu][x_nu mod 2]; out[2 d + eo] = peo[d][eo] / (physVol * 0.5 * (nd - 1) * nc), of the resident field */
int qexhip_plaq_s4(qexhip_handle h, double out[8]);

/* ---------------- gauge fixing (src/gauge/gaugefix.nim) ----------------
 * Coulomb (dirs = {0,1,2}) or Landau (dirs = {0,1,2,3}) gauge fixing of the resident links (qexhip_gauge_set) by a resident
 * transform field t, one SU(3) matrix per site, host format [vol][3][3][2] in the V = 1 even-odd site order.  `dirs` is any
 * subset of {0,1,2,3} without repeats.  QEXHIP_ERR_ARG, before anything is launched and with nothing written, for bad dirs,
 * orf outside (0,2], maxits < 0, and when the gauge field or the transform is not resident.
 *   set_transform   t := the given field, NULL = the identity (`t := 1`, gaugefix.nim:376); get_transform downloads it
 *   gauge_fix       getGaugeFixTransform (gaugefix.nim:312-355): even/odd SU(2)-subgroup over-relaxation (relaxE / relaxO :286-310,
 *                   overRelaxSu2 :241-284) until gdsq = gre + gro <= gstop, then line-minimisation steps (gfLineMin :197-227)
 *                   while it stays there; stops after 11 consecutive evaluations with gdsq <= gstop, or after maxits updates
 *                   (which the reference lacks; reaching it is not an error).  An evaluation and the relax sweep behind it are
 *                   one pass here, so the first update after gdsq has fallen to gstop is still a relax sweep.  iters = updates
 *                   done; metrics = {met, gre, gro, gdsq} of the last evaluation (gfMetrics :145-174), which is t's as returned;
 *                   hist (may be NULL) receives met, gre, gro of the evaluation before update k at hist[3 k], k < min(iters, histcap).
 *                   Option "gfix_check" (default 16): relax iterations between two read-backs of the device-side loop state;
 *                   the result does not depend on it.
 *   gauge_transform gaugeTransform (gaugefix.nim:8-20): g_mu(x) <- t(x) g_mu(x) t(x+mu)^+ on the resident links, all four mu
 *   link_trace      linkTrace (gaugefix.nim:135-142): sum_{mu in dirs} Re tr g_mu / (ndirs * physVol * 3) of the resident links
 * t-sharded contexts: collective; t is the rank's slab, sums are rank-global.  qexhip_release_workspace frees the transform. */
int qexhip_gfix_set_transform(qexhip_handle h, const double *t);
int qexhip_gfix_get_transform(qexhip_handle h, double *t);
int qexhip_gauge_fix(qexhip_handle h, const int *dirs, int ndirs, double gstop, double orf, int maxits, int *iters, double metrics[4],
                     double *hist, int histcap);
int qexhip_gauge_transform(qexhip_handle h);
int qexhip_gauge_link_trace(qexhip_handle h, const int *dirs, int ndirs, double *out);

/* ---------------- link construction upstream of the solver ----------------
 * g, fl, ll: double[vol][4][3][3][2].
 * qexhip_fat7: makeImpLinks (src/gauge/fat7l.nim:77-161), coef = {oneLink, threeStaple, fiveStaple,
 *   sevenStaple, lepage} (Fat7lCoefs :5-10); ll (nullable) <- naik * U U U.
 * qexhip_hisq_smear: HisqCoefs.init + smear (src/physics/hisqLinks.nim:9-43): fat7 -> projectU ->
 *   fat7 + Naik; the input already carries BC + staggered phases (tests/examples/testStagProp.nim:24-33).
 * qexhip_nhyp_smear: the forward part of HypCoefs.smear (src/gauge/hypsmear.nim:49-144,260-275). */
int qexhip_fat7(qexhip_handle h, const double *g, const double coef[5], double *fl, double *ll, double naik);
int qexhip_hisq_smear(qexhip_handle h, const double *g, double *fl, double *ll);
int qexhip_nhyp_smear(qexhip_handle h, const double *g, double *fl, double alpha1, double alpha2, double alpha3);
/* The chain rule through those link constructions (HISQ molecular dynamics):
 *   fat7_deriv: fat7lDeriv (src/gauge/fat7lderiv.nim): d = d/dU^+ of sum Re tr(dfl^+ fl(g)) + sum Re tr(dll^+ ll(g)) for
 *               (fl, ll) = makeImpLinks(g, coef, naik); dll NULL = no long links
 *   hisq_force: HisqCoefs.smearGetForce's smearedForce(dsdu, dsdsu, dsdsul) (src/gauge/hisqsmear.nim:55-90): second fat7 +
 *               Naik, projectUderiv, first fat7, in reverse; dsdsu / dsdsul = the action's derivative w.r.t. the fat / long links */
int qexhip_fat7_deriv(qexhip_handle h, const double *g, const double *dfl, const double coef[5], const double *dll, double naik, double *d);
int qexhip_hisq_force(qexhip_handle h, const double *g, const double *dsdsu, const double *dsdsul, double *f);
/* the same as the closure the reference returns (hisqsmear.nim:55-90: it retains u and the intermediate v, w):
 *   prepare: smear g, keep u, v = fat7_1(u), w = projectU(v) and the smeared su, sul on the device; fl / ll (nullable) receive
 *            su / sul; qexhip_stag_set_links_hisq(h, NULL) afterwards hands su, sul to the operator without another smearing
 *   closure_force: smearedForce(dsdu, dsdsu, dsdsul), the reverse pass only;  release: drop the state */
int qexhip_hisq_prepare(qexhip_handle h, const double *g, double *fl, double *ll);
int qexhip_hisq_closure_force(qexhip_handle h, const double *dsdsu, const double *dsdsul, double *f);
int qexhip_hisq_release(qexhip_handle h);
/* fermionForce of the HISQ HMC (src/examples/hisqhmc.nim:496-541) through the closure (prepared with the PHASED links, as
 * smearRephase does, :407-412): f1 = sum_k scale[k] p_k(x) (x) p_k(x+mu)^+, f3 the same with x+3mu, odd sites *= -1,
 * smearedForce(ff, f1, f3), f = TAH(ff u^+) */
int qexhip_hisq_fermion_force(qexhip_handle h, double *f, const double *const *psi, const double *scale, int n);

/* n (1..4) independent systems on the SAME links solved in lock-step, the links streamed once per sweep for all of
 * them (the Dslash is HBM-bound and 89 % of its bytes are links).  This is how the back-to-back solves of QEX's HMC
 * are meant to be issued: the Hasenbusch chain of faction / fforce (src/examples/staghmc_sh.nim:339-364,394-404), the
 * pbp repetitions (:260-272), the fork's fforce loop (src/stagg_pv_hmc/staghmc_spv.nim:758-830).
 *   solve_xx_batch: n x solveXX (qexhip_stag_solve_xx semantics per system: own mass, r2req, iteration count)
 *   solve_batch:    n x Staggered.solve (qexhip_stag_solve semantics per system)
 * Each system's arithmetic is that of the single-system call, so solutions and iteration counts are the same.
 * x, b: arrays of n host fields [vol][3][2].  Works t-sharded as well (faces of all systems exchanged per sweep, one
 * all-reduce for the n scalars of a reduction). */
int qexhip_stag_solve_xx_batch(qexhip_handle h, int n, double *const *x, const double *const *b, const double *mass,
                               const double *r2req, int maxits, int par_even, int *iters, double *r2_over_b2);
int qexhip_stag_solve_batch(qexhip_handle h, int n, double *const *x, const double *const *b, const double *mass,
                            const double *r2req, int maxits, int *iters, double *r2_over_b2);

/* The lock-step batch in mixed precision (sloppy as in qexhip_stag_solve_xx_sloppy): the fp32 iterations of all n (1..4) systems
 * share ONE sweep over the fp32 link copy; every system keeps its own reliable-update state, takes its fp64 true-residual updates
 * on its own, and stops on its own TRUE residual.  Per system the arithmetic is that of the single-system sloppy call on that
 * system, so x, iters (fp32 iterations), the residual and nupdates are bit for bit what qexhip_stag_solve_xx_sloppy /
 * qexhip_stag_solve_sloppy return for it alone; maxits is shared, as in the fp64 batch.  iters, r2_* and nupdates (may be NULL) are
 * arrays of n.  sloppy = 0 is qexhip_stag_solve_xx_batch / qexhip_stag_solve_batch itself (nupdates 0).
 * QEXHIP_ERR_ARG for sloppy outside 0..2, n outside 1..4, mass 0 (with sloppy > 0), and -- with sloppy > 0 and option "batch_ranks"
 * = 0, the default -- for t-sharded contexts (more than one rank, or qexhip_comm_force_halo); nothing is launched.
 * With option "batch_ranks" = 1 (set on every rank) the batches run t-sharded, collectively: each rank passes its slabs; the
 * reduced-precision faces of ALL n systems travel in one exchange per sweep (fp32: 24 B per site, 16-bit with "half_batch" = 1: 16 B),
 * whether or not a system has finished; every system's <p,Ap>, |r_s|^2 and |b - A x|^2 are rank-global, summed for all systems in
 * one collective per reduction point exactly as the single-system sharded solve sums them; the reliable updates run the sharded fp64
 * operator per system.  Every system returns the bits of its single-system sloppy solve on the SAME sharded context (same sweep
 * form -- option "overlap" --, same transport), every rank returns the same iters, residuals, nupdates and
 * qexhip_stag_sloppy_last_batch, and the n states are checked for agreement across the ranks every 32 iterations (QEXHIP_ERR_COMM).
 * The refinement phase of the sharded mixed-precision multi-shift solve stays one shift at a time. */
int qexhip_stag_solve_xx_batch_sloppy(qexhip_handle h, int n, double *const *x, const double *const *b, const double *mass,
                                      const double *r2req, int maxits, int par_even, int sloppy, int *iters, double *r2_over_b2,
                                      int *nupdates);
int qexhip_stag_solve_batch_sloppy(qexhip_handle h, int n, double *const *x, const double *const *b, const double *mass,
                                   const double *r2req, int maxits, int sloppy, int *iters, double *r2_final, int *nupdates);

/* Storage format the library chose for the operator's links at the last set_links call.  A unitary link is fixed
 * by rows 0,1 and its determinant (row2 = det * conj(row0 x row1)), and the sweep is HBM-bound, so:
 *   1: every link is SU(3) up to a sign (thin links with BC + staggered phases): rows 0,1 + a sign bit, 96 B/link
 *   2: every link is U(3) (nHYP-smeared links): rows 0,1 + det, 112 B/link
 *   0: otherwise (HISQ fat links; QEX's `random` start, 1.3 % of whose links are further than 5e-14 from unitary, the
 *      worst 2.5e-9): all 18 reals, 144 B/link
 * chosen only if ALL links reproduce their stored row 2 to 5e-14 (a few hundred ulp: exactly unitary links of a 48^3x96 lattice peak at ~2e-14); max_dev = the largest deviation found for the
 * chosen format.  Row 2 is rebuilt in registers.  QEXHIP_RECON=0|1|2 caps the format.  No counterpart in QEX (its
 * CPU Dslash always reads full links, stagD.nim:349-395); QUDA's reconstruct-12/13 is the precedent. */
int qexhip_stag_links_info(qexhip_handle h, int *nlinks, int *compressed, double *max_dev);
/* Bytes the 8- or 16-link sweep streams per link at the last set_links: 96 / 112 for formats 1 / 2, 144 for 18 reals, and 108 for
 * the lossless residual format.  That one is taken by 8-link operators that fit neither format 1 nor 2 (QEX's `random` start):
 * rows 0,1 are stored exactly, row 2 as int16 multiples of one ulp of its rebuild +-conj(row0 x row1), and a link whose row 2 this
 * does not reproduce bit for bit is "escaped" (its row 2 is read from the 18 reals).  The operator is the 18-real one bit for bit,
 * so qexhip_stag_links_info reports format 0.  Taken when at most 1 % of the links escape; option "lossless" = 0 (or "recon"
 * = 0) keeps it off.  100 for the packed form of the same (option "lossless" = 2): the residuals, 19 bits wide, sit in
 * bits 62..56 of the 12 reals of rows 0,1, which are constant for 2^-15 <= |v| < 2, and in one extra 4-byte word; a link with a real
 * outside that window is escaped too, and an escaped link is read whole from the 18 reals.  Above 1 % escaped the choice falls to
 * the 108-byte format under its own rule, then to 18 reals.  92 for the orthogonal form (option "lossless" = 3, the default): row 1's
 * last element is rebuilt as well, from the orthogonality of rows 0 and 1 (two IEEE divisions by |a2|^2), so ten slots are stored;
 * the residuals -- 20 bits for row 2, 23 for that element -- sit in the ten slots' payload bits and in an 8- and a 4-byte word.  Above
 * 1 % escaped the choice falls to the packed form.  escaped = the links the last encoding escaped (0 if it did not run). */
int qexhip_stag_links_storage(qexhip_handle h, int *bytes_per_link, long long *escaped);
/* The residual format's encoder and decoder on the host, for n links of 18 doubles (3x3 complex, row-major, re/im): escaped[i] =
 * link i is escaped; row2[6 i ..] = its row 2 as decoded (the rebuild for an escaped link).  Either output may be null.  Needs no
 * device. */
int qexhip_link_residual_host(const double *links, int n, unsigned char *escaped, double *row2);
/* The same for the packed form: decoded[18 i ..] = link i as decoded, all 18 reals. */
int qexhip_link_packed_host(const double *links, int n, unsigned char *escaped, double *decoded);
/* The same for the orthogonal form. */
int qexhip_link_ortho_host(const double *links, int n, unsigned char *escaped, double *decoded);
/* Options of a context.  Unknown names are an error (QEXHIP_ERR_ARG).
 *   "recon"        cap on the link compression (0 keep all 18 reals, 1 sign format only, 2 also the U(3) format; default 2),
 *                  effective at the next set_links (the fp32 copy of the sloppy solves: 0 keeps 18 reals, else the sign format
 *                  where it applies); 0 also keeps the lossless format off
 *   "lossless"     8-link operators that fit neither compressed format take a lossless format (qexhip_stag_links_storage) if at most
 *                  1 % of their links escape it.  3 (default): the orthogonal 92-byte form, else as 2; 2: the packed 100-byte form, else
 *                  the 108-byte residual format, else 18 reals; 1: the 108-byte format, else 18 reals; 0: 18 reals.  Effective at the
 *                  next set_links
 *   "sloppy_check" the sloppy solves post their (device-gated) reliable-update launches every this many fp32 iterations, and
 *                  at maxits (default 4; 1: in the iteration that calls for an update)
 *   "half"         1: sloppy = 2 (SloppyHalf) iterates on 16-bit storage in the single-system solves, on one rank and on t-sharded
 *                  contexts (set it on every rank); 0 (default): it runs single.  Other values are refused
 *   "half_batch"   1: sloppy = 2 on the lock-step batched entries (the deflated batches included) iterates on 16-bit storage, up to
 *                  four systems per stream of the int16 links (t-sharded contexts: with "batch_ranks" = 1); 0 (default): those
 *                  batches run single.  Independent of "half".  Other values are refused
 *   "batch_ranks"  1: the mixed-precision lock-step batched entries (sloppy > 0; the deflated batches and both batched operator probes
 *                  included) run on t-sharded contexts -- more than one rank, or qexhip_comm_force_halo; set it on every rank; 0
 *                  (default): they refuse there, as before the option existed.  Precision follows "half_batch".  Other values are refused
 *   "half_stall"   successive reliable updates of a 16-bit solve that may fail to lower the true residual before the solve
 *                  finishes in fp32 (default 2; 0: hand over at the first update, a test hook)
 *   "stout_check"  inverse iterations of qexhip_stout_inverse posted between two read-backs of its device-side loop state
 *                  (default 8); the result does not depend on it
 *   "overlap"      face exchange on the second stream beside the interior sweep: 0 never, 1 always, -1 (default) measured at
 *                  set_links when the communicator has more than one rank (qexhip_stag_sweep_info), else by interior / face
 *                  size; -2: measure on one rank too (test hook)
 *                  0 / 1 also pin the launch structure, and with it the bits of a sharded residual history, from run to run
 *                  (the measurement takes the overlapped form only on a > 5 % win).  Must be the same on every rank (checked
 *                  at set_links)
 *   "transport"    before qexhip_comm_init: 0 auto, 1 rccl, 2 peer, 3 mbox (see "communicator"); the same on every rank
 *   "flow_exp"     1: closed-form exp(v) in the Wilson-flow stage (default; agrees with the reference's to ~1e-15 per element),
 *                  0: the reference's algorithm, order-4 Taylor + 20 squarings (matexp.nim:80-85,634-649)
 *   test hooks -- each selects, on any lattice, the code path that some lattices / ranks take by necessity:
 *   "multi_reduce" 1: the sharded reduction branches (all-reduce of the partial vectors) on one rank
 *   "batch_multi"  1: the same for the lock-step multi-system CG
 *   "smear_ca"     0: the nHYP levels of a t-sharded field refresh the ghost slices of every projected level field (rounds 1-4) instead of
 *                  computing them on shrinking ghost slices from one depth-3 thin-link exchange (default 1)
 *   "hop_split"    how an OVERLAPPED sweep of a t-sharded field is laid out on the peer transport (RCCL always runs 0).
 *                  2: the FUSED sweep, one kernel on one stream (shifts.nim:67-94,254-285: local terms while the faces travel, boundary
 *                  terms when they are in): its first workgroups push the faces into the neighbours' receive arenas, the interior
 *                  workgroups take every hop of their sites, the boundary workgroups take the hops inside the slab, wait SHORTLY (about
 *                  one measured exchange time) for the inbound data words and then either take the 1-2 hops per site that leave the slab
 *                  straight from the arena, or -- faces late -- park their raw accumulator and give up their slot; the last <= 32
 *                  workgroups of the grid finish the parked blocks behind the one LONG bounded wait (QEXHIP_PEER_TIMEOUT: a lost
 *                  neighbour).  No kernel holds more than those 32 slots hostage to another rank's progress -- ranks may share a chip.
 *                  0: by SITES (interior launch beside the exchange, boundary launch on the second stream behind it, device-side join).
 *                  -1 (default): whichever set_links measured faster (qexhip_stag_sweep_tuning), fused until measured.  Boundary sites
 *                  sum their local hops first under 2, parked or not: equal to 0 to rounding, and to itself to the bit.
 *   "fused_spin_us" the fused sweep's short wait: -1 (default) max(25 us, one exchange time), >= 0 microseconds, -2 park every boundary
 *                  block (test hook: the cleanup path everywhere)
 *   "chain_overlap" 0: the nHYP force chain of a t-sharded field exchanges a level's chain fields first and runs the next staple
 *                  derivative in one pass, instead of running its ghost-free slices beside the exchange (default 1; bit-identical)
 *   "hisq_md_fused" the two kernels of qexhip_md_hisq_fforce / _fforce_solve (default 3): bit 0 = k_outer13 (0: the 2n outer-product launches
 *                  it replaces), bit 1 = k_projtah_kick (0: TAH, then the kick, in two launches); bit-identical, A/B and test hook
 *   "force_pair"   0: k_force_lds (one tile and parity per workgroup), what shapes without paired tile positions run
 *   "obs_clover"   0: the generic path walker, what fmunu loops 3-5 run, for the clover loop as well
 *   "emu_exchange_us", "emu_allreduce_us"   transport emulation for one-GPU rehearsals: every face exchange / all-reduce is preceded,
 *                  on its stream, by a wait of that many microseconds -- the time the transfer would take between distinct
 *                  GPUs.  Results must not depend on it (a consumer that does not wait for its ghosts would show); iteration
 *                  times under it are what bench.py --halo --emulate-transport reports
 *
 * Environment (read once, at qexhip_init / qexhip_comm_init) -- the complete list:
 *   QEXHIP_RECON, QEXHIP_OVERLAP, QEXHIP_HOP_SPLIT, QEXHIP_FLOW_EXP   initial values of the options of the same (lower-case) name
 *   QEXHIP_TRANSPORT=auto|rccl|peer|mbox, QEXHIP_RENDEZVOUS_TIMEOUT, QEXHIP_PEER_TIMEOUT, QEXHIP_LOCAL_RANKS   see "communicator"
 *   QEXHIP_TEST_FAIL_INIT, QEXHIP_TEST_FAIL_MBOX   test hooks: inject a late failure into qexhip_init / into comm_init's mailbox self-test
 *                    (1: it fails; 2: and an explicit `mbox` wish falls back to rccl like `auto`), so that the clean-up and fall-back
 *                    paths run on a one-GPU box (tests/test_gpu_misc_ops.py)
 *   QEXHIP_COMM2=0   keep ONE RCCL communicator for both streams (default: the overlapped face exchange gets a communicator
 *                    of its own); the ranks agree on this by a min-all-reduce, any rank's 0 wins
 * Every other choice the kernels make (visiting orders, non-temporal accesses, LDS staging, launch shapes) is fixed to the
 * variant that won its A/B measurement on MI355X (profiles/); the losers are not in the library. */
int qexhip_set_option(qexhip_handle h, const char *name, int value);

/* Smear on the device and hand the result straight to the operator (replaces smear -> rephase ->
 * set_links without moving the smeared links over PCIe):
 *   hisq: Staggered.g <- HisqCoefs.smear(g) (fat + long); g carries BC + phases already
 *         (tests/examples/testStagProp.nim:24-40: g.setBC; g.stagPhase; hc.smear(g, fl, ll); newStag3(fl, ll))
 *   nhyp: Staggered.g <- rephase(HypCoefs.smear(g)) with the fork's per-direction boundary flags
 *         (src/stagg_pv_hmc/staghmc_spv.nim:367-401,601-604): antiperiodic[mu] != 0 flips U_mu on the last
 *         slice of direction mu (NULL: t only, as gaugeUtils.nim:124-131); phases NULL = {8,9,11,0}.
 *         g == NULL: take the links the closure of qexhip_nhyp_prepare already smeared (the alphas are
 *         ignored), which is what smearRephase does (src/examples/staghmc_sh.nim:303-312). */
int qexhip_stag_set_links_hisq(qexhip_handle h, const double *g);
int qexhip_stag_set_links_nhyp(qexhip_handle h, const double *g, double alpha1, double alpha2, double alpha3,
                               const int antiperiodic[4], const int phases[4]);

/* nHYP smeared-force chain = the closure smearGetForce returns (src/gauge/hypsmear.nim:49-247):
 *   prepare: smear g (alphas as HypCoefs) and keep the 12+12+12+12+4 intermediate link fields on the
 *            device; fl (nullable) receives the smeared links.  Replaces `coef.smearGetForce(gf, fl, info)`
 *            (src/stagg_pv_hmc/staghmc_spv.nim:989-993).  The state refers to THIS g.
 *   force:   smearedForce(f, chain): chain = dS/dV^+ w.r.t. the smeared links ([vol][4][3][3][2]),
 *            f = dS/dU^+ w.r.t. the thin links, through projectUderiv + symStapleDeriv
 *            (src/maths/matrixFunctions.nim:329-357, src/gauge/smearutil.nim:22-50); f may alias chain
 *            (the fork calls f.smeared_force(f), staghmc_spv.nim:740).
 *   release: drop the closure (QEX: GC of the closure, hypsmear.nim:249-263).
 *   prepare with g == NULL smears the links resident on the device (qexhip_gauge_set / qexhip_md_begin); the three MD
 *   forces below with f == NULL leave their result on the device for qexhip_md_kick / qexhip_md_shift_links (source 1). */
int qexhip_nhyp_prepare(qexhip_handle h, const double *g, double alpha1, double alpha2, double alpha3, double *fl);
int qexhip_nhyp_force(qexhip_handle h, double *f, const double *chain);
int qexhip_nhyp_release(qexhip_handle h);
/* The two MD forces of the fork's HMC that run through the closure, start to finish on the device:
 *   gauge:   gforce(act, g, sg, f, smear_force) (src/stagg_pv_hmc/staghmc_spv.nim:217-228): derivative of the
 *            gauge action on the SMEARED links (gaugeForceCust / forceACust, staghmc_spv_gforce.nim:17-253;
 *            coefficients as qexhip_gauge_force_general), smearedForce, projTAH(g, "adj") = TAH(g f^+).
 *   fermion: fforce + smeared_one_link_force (staghmc_spv.nim:716-865): f = sum_k scale[k] psi_k(s) (x) psi_k(s+mu)^+
 *            (psi_k full-volume vectors, host), f.rephase (setBC_cust + stagPhase), odd sites *= -1,
 *            smearedForce, projTAH(gf) = TAH(f g^+).  antiperiodic / phases as qexhip_stag_set_links_nhyp. */
int qexhip_nhyp_gauge_force(qexhip_handle h, double *f, double cplaq, double crect, double cadjplaq);
/*   fforce, solves included (src/examples/staghmc_sh.nim:387-427): psi_k = D(mass[k])^-1 phi_k for the n pseudofermion
 *            fields (Staggered.solve semantics, lock-step batches of four on the operator's CURRENT links -- set them
 *            from this closure first: qexhip_stag_set_links_nhyp(h, NULL, ...)), then the fermion force above with
 *            scale[k] = fscale(k, i, t).  Solutions never leave the GPU; iters[k] (nullable) = iterations of system k. */
int qexhip_nhyp_fforce(qexhip_handle h, double *f, int n, const double *const *phi, const double *mass, const double *scale,
                       const double *r2req, int maxits, const int antiperiodic[4], const int phases[4], int *iters);
int qexhip_nhyp_fermion_force(qexhip_handle h, double *f, const double *const *psi, const double *scale, int n,
                              const int antiperiodic[4], const int phases[4]);
/*   the same with the pseudofermion fields already resident (field ids): nothing but scalars crosses PCIe when f == NULL */
int qexhip_nhyp_fforce_dev(qexhip_handle h, double *f, int n, const int *phi_ids, const double *mass, const double *scale,
                           const double *r2req, int maxits, const int antiperiodic[4], const int phases[4], int *iters);

/* ---------------- stout smearing (src/gauge/stoutsmear.nim) ----------------
 * One step is fl = exp(-alpha nc TAH(g ds^+)) g with ds the derivative of the plaquette action (plaq: 1.0): one stage of the flow
 * integrator, and it honours option "flow_exp" as the flow does.  Fields are double[vol][4][3][3][2].
 *   smear        StoutSmear.smear (stoutsmear.nim:15-34), one step, nothing kept.  g NULL = the resident links (qexhip_gauge_set /
 *                qexhip_md_begin); fl NULL = the result replaces the resident links; g == fl is allowed (tstoutderiv.nim:22-23).
 *   prepare      levels 0..nlevels-1 (alphas[k]) applied in order, 1 <= nlevels <= 8, and what smearDeriv needs of every level kept
 *                on the device: its input links and alpha nc f (the reference keeps gf, f, expaf, ds, stoutsmear.nim:5-13;
 *                exp(a f) and ds are recomputed here).  g NULL = the resident links, fl (nullable) receives the smeared links.
 *                The state refers to THIS g: with fl == g ("in place", level 0's input overwritten, :22) the force entry points
 *                refuse, as smearDeriv is undefined then.
 *   force        smearDeriv (stoutsmear.nim:148-175; gaugeForceDeriv :97-146, expDeriv = expm1Deriv with scale 20, order 4,
 *                src/maths/matexp.nim:686-713, matrixFunctions.nim:471-481) from the last level to the first
 *                (tstoutderiv.nim:190-192): chain = dS/dV^+ w.r.t. the smeared links, f = dS/dU^+ w.r.t. the input links.  f may
 *                alias chain; f NULL leaves the result on the device as MD force source 1 (qexhip_md_kick).
 *   gauge_force  smearedForce of tests/base/tstoutderiv.nim:137-143: gaugeActionDeriv on the smeared links (coefficients as
 *                qexhip_nhyp_gauge_force), the chain, contractProjectTAH(g, f) = TAH(g f^+).  f NULL as in force.
 *   release      drop the chain.  force / gauge_force without a prepared chain, after release, or after an in-place level 0
 *                fail with QEXHIP_ERR_ARG and the message "call qexhip_stout_prepare first" / "smeared in place".
 *   inverse      StoutSmear.inverse (stoutsmear.nim:36-89): g with smear(g) = fl by the fixed-point iteration of Luescher's
 *                trivialising map (all links move at once), from g = fl.  iters = the first iteration whose rdf2 = |f_k - f_{k-1}|^2 /
 *                |f_k|^2 < rdf2req, or maxits (not an error); rdf2 belongs to the returned field; diverging = 1 if |f_k - f_{k-1}|^2
 *                ever grew (the reference's "df^2 increased" warning, :81-83).  iters, rdf2, diverging may be NULL.  The loop state
 *                stays on the device; option "stout_check" (default 8) = iterations posted between two read-backs of it, and the
 *                result does not depend on it.  g != fl.
 * QEXHIP_ERR_ARG, before anything is launched and with nothing written: a non-finite alpha, nlevels outside 1..8, maxits < 0,
 * g == fl in inverse.  t-sharded contexts: collective, fields are the rank's slab.  qexhip_release_workspace drops the chain and
 * the scratch fields of smear / inverse. */
int qexhip_stout_smear(qexhip_handle h, const double *g, double alpha, double *fl);
int qexhip_stout_prepare(qexhip_handle h, const double *g, const double *alphas, int nlevels, double *fl);
int qexhip_stout_force(qexhip_handle h, double *f, const double *chain);
int qexhip_stout_gauge_force(qexhip_handle h, double *f, double cplaq, double crect, double cadjplaq);
int qexhip_stout_release(qexhip_handle h);
int qexhip_stout_inverse(qexhip_handle h, const double *fl, double alpha, double rdf2req, int maxits, double *g, int *iters,
                         double *rdf2, int *diverging);

/* ---------------- random number fields and configuration generation (host only, no handle) ----------------
 * newRNGField (src/rng/distributionUtils.nim:306-331): one generator per site of the LOCAL lattice, seeded with
 * (seed, global lexicographic site index, x fastest); kind 0 = RngMilc6 (src/rng/milcrng.nim), 1 = MRG32k3a
 * (src/rng/mrg32k3a.nim).  glat NULL = lat, t_offset = first global t of this rank's slab.  The deviates are produced
 * with the host's libm so that they are bit-identical to QEX's.  Fields in the library's host format:
 *   uniform:          x.uniform r, ncomp reals per site           (distributionUtils.nim:23-44)
 *   gaussian_vector:  v.gaussian r, colour vector                  (:64-97)
 *   u1_vector:        v.u1 r                                       (:182-211)
 *   random_tah:       p.randomTAH r (randTah3)                     (src/gauge/gaugeUtils.nim:1356-1383)
 *   gauge_random:     g.random r = gaussian + projectSU            (:1348-1354,1424-1429)
 *   gauge_warm:       g.warm s, r = exp(s randTah3)                (:1384-1388,1431-1441) */
typedef struct qexhip_rng qexhip_rng;
int qexhip_rng_new(qexhip_rng **rng, int kind, unsigned long long seed, const int lat[4], const int glat[4], int t_offset);
int qexhip_rng_free(qexhip_rng *rng);
int qexhip_rng_uniform(qexhip_rng *rng, int ncomp, double *v);
int qexhip_rng_gaussian_vector(qexhip_rng *rng, double *v);
int qexhip_rng_u1_vector(qexhip_rng *rng, double *v);
/* v.z4 r / v.z2 r (distributionUtils.nim:102-180, without FUELCompat): one uniform u per colour component;
 * z4: u < 0.25 -> 1, < 0.5 -> i, < 0.75 -> -1, else -i;  z2: u < 0.5 -> 1, else -1 */
int qexhip_rng_z4_vector(qexhip_rng *rng, double *v);
int qexhip_rng_z2_vector(qexhip_rng *rng, double *v);
int qexhip_rng_random_tah(qexhip_rng *rng, double *p);
int qexhip_rng_gauge_random(qexhip_rng *rng, double *g);
int qexhip_rng_gauge_warm(qexhip_rng *rng, double s, double *g);
/* generator state per site (RngMilc6: 9 uint32 = r0..r6, icState, multiplier, src/rng/milcrng.nim:12-14; MRG32k3a: 6),
 * the payload of the fork's RNG checkpoints (src/stagg_pv_hmc/staghmc_spv_rng.nim:135-182) */
int qexhip_rng_state_words(qexhip_rng *rng);
int qexhip_rng_get_state(qexhip_rng *rng, unsigned *out);
int qexhip_rng_set_state(qexhip_rng *rng, const unsigned *in);

/* The same generators writing into HBM, for the two ends of an HMC trajectory (refresh / measure of the drivers:
 * src/examples/staghmc_sh.nim:716-757,774-789, src/stagg_pv_hmc/staghmc_spv.nim:1180-1250) -- RngMilc6 fields only.  The
 * generator states go to the device (36 B per site), one lane per site advances its stream, the states come back: the field's
 * state afterwards is bit for bit the one the host call of the same name leaves (qexhip_rng_get_state), and host and device
 * calls can be mixed freely.  Deviates: formed with the device's fp64 log / cos / sqrt; after RngMilc6.gaussian's float32
 * rounding they equal the host's except where the double falls within ~1e-16 of a float32 rounding boundary (about one
 * deviate in 1e8, by one float32 ulp); u1 phases agree to 1e-16.
 *   dev_gaussian_vector: v.gaussian r into the resident colour vector `field_id`      (distributionUtils.nim:64-97)
 *   dev_u1_vector:       v.u1 r                                                       (:182-211)
 *   md_refresh_momenta:  p.randomTAH r into the resident MD momenta (gaugeUtils.nim:1356-1383); qexhip_md_begin(h, g, NULL)
 *                        keeps them, qexhip_md_momentum_norm2 gives 2 T + const. */
int qexhip_rng_dev_gaussian_vector(qexhip_handle h, qexhip_rng *rng, int field_id);
int qexhip_rng_dev_u1_vector(qexhip_handle h, qexhip_rng *rng, int field_id);
/* z4 / z2 noise: the values are exact, so field and generator state equal the host fill's bit for bit */
int qexhip_rng_dev_z4_vector(qexhip_handle h, qexhip_rng *rng, int field_id);
int qexhip_rng_dev_z2_vector(qexhip_handle h, qexhip_rng *rng, int field_id);
int qexhip_md_refresh_momenta(qexhip_handle h, qexhip_rng *rng);

/* ---------------- resident molecular dynamics ----------------
 * The MD loop of QEX's HMC drivers -- mdt (U <- exp(t p) U), mdv (p -= t f), mdvAllfga with its force-gradient shifts
 * (src/examples/staghmc_sh.nim:429-640, src/stagg_pv_hmc/staghmc_spv.nim:873-1061) -- with links and momenta left on the
 * device between the updates.  Forces stay in a device buffer, the "source" of a later kick or shift:
 *   source 0: qexhip_md_gauge_force (gc.forceA / gaugeForce of the resident thin links)
 *   source 1: the last force of the nHYP closure: qexhip_nhyp_gauge_force / _fermion_force / _fforce called with f = NULL
 * and qexhip_nhyp_prepare(g = NULL) smears the resident links.  begin uploads (g NULL: keep the resident links of
 * qexhip_gauge_set; p NULL: keep the resident momenta, e.g. of qexhip_md_refresh_momenta), end downloads (either pointer may be NULL).  kick: p += t * f.  shift_links: U <- exp(t f) U
 * (fgv / fgvf of the force-gradient update); save / restore bracket it (fgsave / fgload). */
int qexhip_md_begin(qexhip_handle h, const double *g, const double *p);
int qexhip_md_end(qexhip_handle h, double *g, double *p);
int qexhip_md_momentum_norm2(qexhip_handle h, double *p2);
int qexhip_md_update_links(qexhip_handle h, double t);
int qexhip_md_gauge_force(qexhip_handle h, double cplaq, double crect, double cadj);
int qexhip_md_kick(qexhip_handle h, int source, double t);
int qexhip_md_shift_links(qexhip_handle h, int source, double t);
int qexhip_md_save_links(qexhip_handle h);
int qexhip_md_restore_links(qexhip_handle h);
/* HISQ molecular dynamics on the resident fields: the force side of src/examples/hisqhmc.nim with nothing but the arguments
 * crossing PCIe.  The state is the HISQ closure's (qexhip_hisq_prepare / qexhip_hisq_release), built from the resident links.
 *   md_hisq_prepare: smearRephase (hisqhmc.nim:405-414) on the resident thin links of qexhip_md_begin / qexhip_gauge_set: a phased
 *       copy (setBC + stagPhase; antiperiodic / phases NULL = the defaults of qexhip_stag_set_links_nhyp: t antiperiodic, QEX's
 *       staggered phases), then u, v, w, su, sul exactly as qexhip_hisq_prepare builds them from that field.  The resident links
 *       are not written (the reference rephases them back).  set_links != 0 also hands su, sul to the operator
 *       (qexhip_stag_set_links_hisq(h, NULL); the reference's stag = newStag3(su, sul), :332).
 *   md_hisq_fforce: fermionForce (:496-539) for n >= 1 resident full-volume vectors: f1 = sum_k scale[k] psi_k(x) (x) psi_k(x+mu)^+,
 *       f3 the same with x+3mu, odd sites *= -1 (one launch per four vectors for both), smearedForce(ff, f1, f3),
 *       f = TAH(ff u^+) with the phased u, and updateMomentum (:558-560) p += t f in the pass that stores f.
 *   md_hisq_fforce_solve: the same with psi_k = D(mass[k])^-1 phi_k (Staggered.solve, :541-545) solved first, in lock-step
 *       batches of at most four on the operator's current links; iters (nullable) receives the iteration counts.
 *   md_hisq_fforce_rational: the force of S = 1/2 Re<phi, r(M^+M) phi>_even with r as in qexhip_dev_rational_xx (the rooted branch
 *       of stagForce, mcmc/fields/staggeredFields.nim:434-467): ONE multi-shift solve on phi.even (mapping as there; sloppy = 1:
 *       the mixed-precision multi-shift solve, 2 runs single), m_k = sqrt(mass^2 + beta[k]), psi_k = D(m_k)^-1 phi with phi.odd = 0,
 *       i.e. psi_k.even = 4 m_k y_k, psi_k.odd = -D_oe psi_k.even / m_k, then md_hisq_fforce with scale_k = alpha[k] / m_k.  f0
 *       contributes nothing.  iters (nullable): the iterations of the one solve.  QEXHIP_ERR_ARG as qexhip_dev_rational_xx.
 *   md_hisq_force_get: the last f of those three, [vol][4][3][3][2] (tests, host integrators); QEXHIP_ERR_STATE if there is none.
 * QEXHIP_ERR_ARG (n < 1, unknown or repeated field ids, NULL arrays) and QEXHIP_ERR_STATE (no resident links, no momenta, no
 * prepare) are returned before anything is launched.  t-sharded: collective. */
int qexhip_md_hisq_prepare(qexhip_handle h, const int antiperiodic[4], const int phases[4], int set_links);
int qexhip_md_hisq_fforce(qexhip_handle h, int n, const int *psi_ids, const double *scale, double t);
int qexhip_md_hisq_fforce_solve(qexhip_handle h, int n, const int *phi_ids, const double *mass, const double *scale, const double *r2req,
                                int maxits, double t, int *iters);
int qexhip_md_hisq_fforce_rational(qexhip_handle h, int phi_id, double mass, int nterm, const double *alpha, const double *beta,
                                   double r2req, int maxits, int sloppy, double t, int *iters);
int qexhip_md_hisq_force_get(qexhip_handle h, double *f);

/* ---------------- SciDAC/LIME gauge files (host only, no handle) ----------------
 * loadGauge / saveGauge (src/gauge/gaugeUtils.nim:87-122) via Reader / Writer (src/io/readerQiolite.nim:37-239,
 * src/io/writerQiolite.nim:28-187): one record of 4 x QDP_{F,D}3_ColorMatrix per site, sites x-fastest, big-endian,
 * with the SciDAC checksum pair.  g is the library's host format (V=1 even-odd, [vol][4][3][3][2] doubles).
 *   info:  lattice, record precision ('F' | 'D') and whether the file carries checksums (getFileLattice, readerQiolite.nim:11-17)
 *   read:  fills g, returns the checksums it computed; QEXHIP_ERR_IO if they differ from the file's
 *   write: precision 'F' | 'D' (saveGauge's prec); file_md / record_md NULL = QEX's defaults (gaugeUtils.nim:108-109) */
int qexhip_io_gauge_info(const char *path, int lat[4], char *precision, int *checksums_present);
int qexhip_io_read_gauge(const char *path, const int lat[4], double *g, unsigned *suma, unsigned *sumb);
/* the slab t0 <= t < t0 + nt (both even) of a file with the GLOBAL lattice lat, into a rank-local field */
int qexhip_io_read_gauge_slab(const char *path, const int lat[4], int t0, int nt, double *g);
int qexhip_io_write_gauge(const char *path, const int lat[4], const double *g, char precision, const char *file_md,
                          const char *record_md);
/* any other field, as Writer.write / Reader.read handle it (src/io/writerQiolite.nim:96-166): site_bytes per site
 * (library's even-odd order in memory, x-fastest in the file), every word_bytes-wide word big-endian in the file;
 * datatype / precision / colors / datacount go into the record header (typesize = site_bytes / datacount).
 * The fork's RNG checkpoint (staghmc_spv_rng.nim:135-182) is write_field(state, 36, 4, "QDP_RngMilc6", 'F', 0, 1, ...). */
int qexhip_io_write_field(const char *path, const int lat[4], const void *data, int site_bytes, int word_bytes, const char *datatype,
                          char precision, int colors, int datacount, const char *file_md, const char *record_md);
int qexhip_io_read_field(const char *path, const int lat[4], void *data, int site_bytes, int word_bytes, char datatype[64]);
/* Reader.fileMetadata / Reader.recordMetadata (src/io/readerQiolite.nim:37-68,120-135; checked by tests/base/tfieldio.nim:
 * 44-62): the user strings of the file and of its first record, 0-terminated, truncated to the capacities given;
 * *file_len / *record_len = the sizes needed (incl. the 0). */
int qexhip_io_metadata(const char *path, char *file_md, int file_cap, char *record_md, int record_cap, int *file_len,
                       int *record_len);
/* crc32 of src/io/crc32.nim:35-37 (reflected 0xedb88320, start and final complement 0xffffffff): what the SciDAC checksum pair
 * is built from, suma ^= rotl(crc32(site), rank % 29), sumb ^= rotl(crc32(site), rank % 31).  The reference's own known
 * answer: crc32("The quick brown fox jumps over the lazy dog") == 0x414FA339 (crc32.nim:103-106). */
int qexhip_io_crc32(const void *data, size_t nbytes, unsigned *crc);

/* ---------------- kernel timers ----------------
 * hipEvent pairs around launches of the named kernel class on the context stream
 * (the tic/toc hooks of src/physics/stagD.nim:354-395, src/solvers/cg.nim:175-241).
 * names: "dslash" (one-parity sweep; the faces of an overlapped sweep are "dslash_bnd"), "blas", "reduce", "staple",
 * "expupdate", "plaq", "exchange" (the RCCL face exchange, on the stream it is posted on), "allreduce".
 * on = 1: every class; 2: the Dslash sweeps only (least perturbation of a timed region); 3: the anatomy of a sharded
 * iteration -- Dslash sweeps, exchange, allreduce; 0: off. */
int qexhip_timers_enable(qexhip_handle h, int on);
int qexhip_timers_reset(qexhip_handle h);
int qexhip_timers_get(qexhip_handle h, const char *name, long *count, double *total_ms);

/* ---------------- index-arithmetic test hooks (pure host functions, no GPU) ----------------
 * The site order / neighbour sense / ghost-zone positions the kernels use, evaluated on the host
 * (same inline code): layoutIndexQ with V=1 (src/layout/qlayout.nim:110-131) and the shift sense of
 * src/layout/shiftX.nim:76-81.  out[8] = {Vh, F, ntile, ghost tiles/side, tiles/parity, depth, halo, X0/2}. */
int qexhip_debug_geom(const int latLocal[4], int depth, int halo, int out[8]);
/* position, in the opposite-parity field, of site (c,parity) + hop*mu; ghost positions when halo */
int qexhip_debug_nbr_pos(const int latLocal[4], int depth, int halo, int c, int parity, int mu, int hop);
int qexhip_debug_site_coord(const int latLocal[4], int c, int parity, int x[4]);
/* the (tile, parity) visiting order of the staple kernels for gathers in the (mu, nu) plane: out[k] = 2 tile + parity or
 * -1 (empty slot); returns the number of entries, or minus the capacity needed.  Must be a permutation. */
int qexhip_debug_tile_order(const int latLocal[4], int mu, int nu, int *out, int cap);

#ifdef __cplusplus
}
#endif
#endif
