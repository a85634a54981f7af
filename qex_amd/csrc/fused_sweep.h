// fused_sweep.h -- the workgroup roles of a fused sweep: push, interior, boundary, cleanup.  k_dslash_fused (dslash.hip) and the
// lock-step k_dslash_mrhs_fused (batch.hip) both run this protocol around their own per-site arithmetic.
//
// The fused sweep, by workgroup number:
//   [0, npush)            push this rank's two faces into the neighbours' receive arenas (credits, release, data words: peer_device.h)
//   interior workgroups   every hop of their sites: the loop of the plain kernel
//   boundary workgroups   (the `depth` outermost slices either side; placed at nbA of the dispatch order, interior workgroups before AND behind
//                         them) the hops that stay inside the slab, then a SHORT wait for the inbound data words (about the transfer time):
//                         faces in -> the 1-2 hops per site that leave the slab straight from the arena, accumulator in registers throughout;
//                         faces late -> the raw accumulator is PARKED in `out`, the block appended to the parked list, the slot given up
//   cleanup workgroups    (the last fz.ncl of the grid) once every boundary workgroup has decided: nothing parked -> exit; else the LONG
//                         bounded wait for the faces (the only place a lost neighbour is noticed), then the parked blocks' remaining hops
//                         on top of their raw accumulators, final scale, store and dot partial -- in the parked block's own partial slot
// Whoever reads the arena last returns the credits.  The sum of a boundary site runs local hops first, then the others, parked or not:
// a parked block gives the same bits as an unparked one (tests/test_gpu_parity.py), and the plain kernel's to rounding.
// Why park (round 6): a boundary workgroup that spins until the faces are in holds its slot hostage to ANOTHER kernel's progress.  With
// 16 links a 48^3 face has 6 x 216 = 1296 boundary workgroups, the chip 768 slots for this kernel: on a chip shared by two ranks'
// processes the spinning ones kept the neighbour's push from ever becoming resident (profiles/r06_notes.md section 1).
// A kernel calls fused_push and fused_enter once, then per pass (one; a cleanup workgroup takes every fz.ncl-th parked block)
// fused_next_block, fused_site, fused_wait_faces (boundary blocks) and fused_partial_slot, and fused_finish at the end.
#pragma once
#include "peer_device.h"
#include "site_index.h"

// What a fused launch carries beside its kernel's own arguments (the ghost base pointers stay with the kernel: one pair per system).
// Site ranges: interior [c0,c1) for logical workgroups [0, nb1), low face [d0,d1) from nb1, high face [e0,e1) from nb2.
struct FusedSweep {
  int e0, e1, nb2;       // the third site range and its first logical workgroup
  int nbA;               // position of the boundary workgroups in the dispatch order (interior workgroups before and behind them)
  PeerGhost pg;          // the inbound data words, the credits owed to the two senders
  PeerPush push;         // the launch's FIRST push.nblocks workgroups send the faces
  FusedCtl fz;           // who has decided, who has parked
};

// One workgroup's part in the launch (workgroup-uniform)
struct FusedRole {
  int bid;               // workgroup number among those that own sites (push workgroups not counted); cleanup workgroups: >= ngrid
  int nb1;               // first boundary block (logical workgroup numbers)
  int nbnd;              // boundary workgroups
  int npark, jpark;      // cleanup: parked blocks (< 0: a wait gave up), the next list entry this workgroup takes
  bool cleanup;
  bool bnd;              // the current block is a boundary block
  bool parked;           // this boundary workgroup gave its block to the cleanup workgroups
};

// the one LDS word the workgroup's lane 0 hands its decisions down by (faces arrived / parked blocks to take)
__device__ __forceinline__ int &fused_sh_word() {
  __shared__ int sh_n;
  return sh_n;
}

// true: one of the launch's first push.nblocks workgroups, which has pushed its share of the faces (nothing when the solve is done) and
// has nothing else to do.  (A helper of its own: folded into fused_enter, this early exit costs the batched kernel 20-50 VGPRs.)
__device__ __forceinline__ bool fused_push(const FusedSweep &F, const bool skip) {
  if ((int)blockIdx.x >= F.push.nblocks) return false;
  if (!skip) peer_push_block(F.push, blockIdx.x);
  return true;
}

// Every other workgroup: its role.  Cleanup workgroups wait here until every boundary workgroup has decided.
__device__ __forceinline__ void fused_enter(const FusedSweep &F, const int nb1, FusedRole &R) {
  const int bid = (int)blockIdx.x - F.push.nblocks;
  const int ngrid = (int)gridDim.x - F.push.nblocks - F.fz.ncl;     // workgroups that own sites
  R.bid = bid; R.nb1 = nb1; R.nbnd = ngrid - nb1;
  R.npark = 0; R.jpark = 0;
  R.cleanup = bid >= ngrid; R.bnd = false; R.parked = false;
  if (R.cleanup) {
    int &sh_n = fused_sh_word();
    if (threadIdx.x == 0) {
      int n = 0;
      if (peer_poll_u32(F.fz.dec, (unsigned)R.nbnd, F.pg.err, F.pg.ticks, 0x520)) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");          // the parked accumulators, the list
        n = (int)__hip_atomic_load(F.fz.ndef, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n > 0) {
          if (!peer_ghost_wait(F.pg)) n = -1;                       // the neighbour is gone: error word set, nothing more to do here
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");             // what other devices wrote into the arena
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
      } else n = -1;
      sh_n = n;
    }
    __syncthreads();
    R.npark = sh_n;
    R.jpark = bid - ngrid;
  }
}

// The logical workgroup lb of this pass: [0, nb1) interior, [nb1, ..) boundary; sets R.bnd.  False: a cleanup workgroup is out of
// parked blocks.
__device__ __forceinline__ bool fused_next_block(const FusedSweep &F, FusedRole &R, int &lb) {
  if (R.cleanup) {
    if (R.jpark >= R.npark) return false;
    lb = (int)F.fz.list[R.jpark];
    R.jpark += F.fz.ncl;
    R.bnd = true;
  } else {
    R.bnd = R.bid >= F.nbA && R.bid < F.nbA + R.nbnd;
    lb = R.bnd ? R.nb1 + (R.bid - F.nbA) : (R.bid < F.nbA ? R.bid : R.bid - R.nbnd);
  }
  return true;
}

// this lane's site of logical workgroup lb, and the end of its range
__device__ __forceinline__ int fused_site(const FusedSweep &F, const FusedRole &R, const int lb, const SweepRanges &r, int &clim) {
  int c = r.c0 + lb * 256 + threadIdx.x;
  clim = r.c1;
  if (R.bnd) {
    c = r.d0 + (lb - R.nb1) * 256 + threadIdx.x; clim = r.d1;
    if (lb >= F.nb2) { c = F.e0 + (lb - F.nb2) * 256 + threadIdx.x; clim = F.e1; }
  }
  return c;
}

// A boundary workgroup between its local and its slab-leaving hops: the SHORT wait for the faces (one lane), then the acquire for what
// other devices wrote.  Sets R.parked when they are late.  A cleanup workgroup has waited in fused_enter already.
__device__ __forceinline__ void fused_wait_faces(const FusedSweep &F, FusedRole &R) {
  if (R.cleanup) return;
  int &sh_n = fused_sh_word();
  if (threadIdx.x == 0) {
    const bool in = F.fz.spin_ticks >= 0 && peer_ghost_try(F.pg, F.fz.spin_ticks, F.fz.late);
    if (in) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    sh_n = in ? 1 : 0;
  }
  __syncthreads();
  R.parked = sh_n == 0;
}

// where the dot partial of block lb goes: the pushing workgroups have none; a parked block's goes where its boundary workgroup's would have
// gone
__device__ __forceinline__ int fused_partial_slot(const FusedSweep &F, const FusedRole &R, const int lb) {
  return R.cleanup ? F.nbA + (lb - R.nb1) : R.bid;
}

// After the last pass: a boundary workgroup appends its block to the parked list if it parked and counts itself in `dec`; the last to decide
// returns the credits if nobody parked.  The last cleanup workgroup resets the words for the next launch and returns the credits if
// anything was parked.  Interior workgroups have nothing to do here.
__device__ __forceinline__ void fused_finish(const FusedSweep &F, const FusedRole &R) {
  if (!(R.bnd || R.cleanup)) return;
  // every wave's loads of the arena have returned / its parked accumulators are on their way before the workgroup counts itself
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x != 0) return;
  bool credits = false;
  if (!R.cleanup) {
    if (R.parked) {
      const unsigned idx = __hip_atomic_fetch_add(F.fz.ndef, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&F.fz.list[idx], (unsigned)(R.nb1 + (R.bid - F.nbA)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");     // accumulators and list entry before the count (the cleanup workgroup may sit on another XCD)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    const unsigned a = __hip_atomic_fetch_add(F.fz.dec, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (a == (unsigned)R.nbnd - 1) {
      // the last to decide: if nobody parked, every reader of the arena is through -- the halves go back to the two senders
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      credits = __hip_atomic_load(F.fz.ndef, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u;
    }
  } else {
    const unsigned a = __hip_atomic_fetch_add(F.fz.cl_done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (a == (unsigned)F.fz.ncl - 1) {
      credits = R.npark > 0;             // (npark < 0: a wait gave up -- the error word is set, the job is over)
      __hip_atomic_store(F.fz.ndef, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(F.fz.dec, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(F.fz.late, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(F.fz.cl_done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (credits) {
    __hip_atomic_store(F.pg.credit[0], F.pg.credit_val[0], __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(F.pg.credit[1], F.pg.credit_val[1], __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// Host: sets up the next fused sweep over the slab of nrhs t-sharded fields (parity half `parity` of f[j] is the hop source): interior
// [lo_end, hi_beg), low face [0, lo_end), high face [hi_beg, Vh).  Posts the push-only exchange, fills F (e0, e1, nb2 and nbA included)
// and the systems' ghost bases, and gives the grid size and the number of dot partials the launch writes.  dslash.hip.
int fused_sweep_setup(qexhip_ctx *c, int nrhs, DevField *const *f, int parity, int lo_end, int hi_beg, FusedSweep *F,
                      const double2 **gh_hi, const double2 **gh_lo, int *grid, int *nparts);
