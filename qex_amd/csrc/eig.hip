// eig.hip -- a resident basis of half-volume vectors and the three block kernels of the low-mode eigensolver / deflation.
//
// The reference's counterpart is src/eigens/hisqev.nim (block Lanczos + Rayleigh-Ritz on the even sites) with the vector algebra
// of src/eigens/linalgFuncs.nim / svdLanczos.nim: orthogonalisation against a set of vectors, the projection x0 = sum_i v_i <v_i,b> c_i
// of its deflated solve (hisqev.nim:653-705), and the rotation of a set of vectors by a small dense matrix (the `rotate` / merge steps
// of its Rayleigh-Ritz passes).  With a few hundred basis vectors these move more bytes than the operator does, so they are block
// forms here, not loops over blas_cdot / blas_axpy:
//   k_block_dot    c_j = <v_j, w>, j < n: a wavefront takes one 64-site tile, keeps the tile of w in registers and streams the n basis
//                  vectors' tiles past it -- w is read once (per 128 vectors), every basis vector once
//   k_block_axpy   y += scale * sum_j coef_j v_j: one pass over the basis, y read and written once
//   k_block_dot_mrhs / k_block_axpy_mrhs   the two for up to four right-hand sides in one pass over the basis (the deflated lock-step batch),
//                  every number bit for bit the single kernel's
//   k_rotate       V[:, 0:k] <- V[:, 0:m] Q in place: a workgroup stages all m inputs of its block of rows in LDS, then writes its k outputs
// A basis holds the body tiles of the EVEN parity only ([tile][3][64] double2 per vector: vec_off), half the memory of a field; vectors
// are copied to / from the even half of an ordinary field when the operator has to run on them.
#include "qexhip_internal.h"
#include "../../include/qexhip.h"
#include "reduce.h"
#include <algorithm>
#include <cstring>

#define EIG_NJ 128          // basis vectors per k_block_dot launch (its LDS accumulators: 4 waves x EIG_NJ complex)
#define EIG_DOT_WG 1024     // at most this many workgroups (= partial sums per vector) per k_block_dot launch

struct EigWork {
  DevField f[EIG_NF];
  bool have[EIG_NF]{};
  double2 *dots = nullptr, *coef = nullptr;   // EIG_MAX_NVECS each
  double *parts = nullptr;                    // 2 * EIG_NJ * EIG_DOT_WG
  double *parts_mrhs = nullptr;               // EIG_MAXRHS times as much, allocated by the first multi-right-hand-side block dot
  double *Q = nullptr;                        // EIG_MAX_NVECS^2
  int lds_attr = 0;                           // k_rotate instantiations whose dynamic LDS limit was raised
};

static int eig_work(qexhip_ctx *c, EigWork **w) {
  if (!c->eig) {
    EigWork *e = new EigWork;
    c->eig = e;
    HIPCHK(hipMalloc((void **)&e->dots, sizeof(double2) * EIG_MAX_NVECS * EIG_MAXRHS));    // [rhs][vector] in the multi-right-hand-side forms
    HIPCHK(hipMalloc((void **)&e->coef, sizeof(double2) * EIG_MAX_NVECS * EIG_MAXRHS));
    HIPCHK(hipMalloc((void **)&e->parts, sizeof(double) * 2 * EIG_NJ * EIG_DOT_WG));
    HIPCHK(hipMalloc((void **)&e->Q, sizeof(double) * EIG_MAX_NVECS * EIG_MAX_NVECS));
  }
  *w = (EigWork *)c->eig;
  return 0;
}
void eig_state_free(qexhip_ctx *c) {
  EigWork *e = (EigWork *)c->eig;
  if (!e) return;
  for (int i = 0; i < EIG_NF; i++) if (e->have[i] && e->f[i].d) (void)hipFree(e->f[i].d);
  if (e->dots) (void)hipFree(e->dots);
  if (e->coef) (void)hipFree(e->coef);
  if (e->parts) (void)hipFree(e->parts);
  if (e->parts_mrhs) (void)hipFree(e->parts_mrhs);
  if (e->Q) (void)hipFree(e->Q);
  delete e;
  c->eig = nullptr;
}
int eig_field(qexhip_ctx *c, int slot, DevField **f) {
  EigWork *e;
  CHK(eig_work(c, &e));
  if (e->have[slot] && e->f[slot].half != (size_t)c->g.etile * 192) {     // the geometry changed (qexhip_comm_force_halo)
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipFree(e->f[slot].d));
    e->f[slot].d = nullptr;
    e->have[slot] = false;
  }
  if (!e->have[slot]) {
    CHK(field_alloc(c, e->f[slot]));
    e->have[slot] = true;
  }
  *f = &e->f[slot];
  return 0;
}
int eig_coef_buffers(qexhip_ctx *c, double2 **dots, double2 **coef) {
  EigWork *e;
  CHK(eig_work(c, &e));
  if (dots) *dots = e->dots;
  if (coef) *coef = e->coef;
  return 0;
}

// ---------------- the basis object ----------------
int eig_basis_find(qexhip_ctx *c, int id, EigBasis **B) {
  auto it = c->bases.find(id);
  if (id <= 0 || it == c->bases.end()) { qexhip_set_error("unknown eigenvector basis id %d", id); return QEXHIP_ERR_ARG; }
  *B = &it->second;
  return 0;
}
int eig_basis_new(qexhip_ctx *c, int nvecs, int *id) {
  if (nvecs < 1 || nvecs > EIG_MAX_NVECS) {
    qexhip_set_error("eig_new: 1 <= nvecs <= %d (nvecs = %d)", EIG_MAX_NVECS, nvecs);
    return QEXHIP_ERR_ARG;
  }
  EigBasis B;
  B.nvecs = nvecs;
  B.n2 = (size_t)c->g.ntile * 192;
  B.gen = c->links_gen;
  B.evals.assign(nvecs, 0.0);
  const size_t bytes = B.n2 * nvecs * sizeof(double2);
  HIPCHK(hipMalloc((void **)&B.v, bytes));
  HIPCHK(hipMemsetAsync(B.v, 0, bytes, c->stream));
  *id = c->next_basis++;
  c->bases[*id] = B;
  return 0;
}
int eig_basis_free(qexhip_ctx *c, int id) {
  EigBasis *B;
  CHK(eig_basis_find(c, id, &B));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipFree(B->v));
  c->bases.erase(id);
  return 0;
}
void eig_bases_free(qexhip_ctx *c) {
  for (auto &kv : c->bases) if (kv.second.v) (void)hipFree(kv.second.v);
  c->bases.clear();
}

__global__ void __launch_bounds__(256) k_eig_copy_scale(double2 *dst, const double2 *src, double a, size_t n) {
  for (size_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const double2 v = src[i];
    dst[i] = make_double2(a * v.x, a * v.y);
  }
}
static inline int grid_for(size_t n2) { return (int)std::min<size_t>(2048, std::max<size_t>(1, (n2 + 255) / 256)); }

static int basis_index_check(const EigBasis &B, int i0, int n, const char *who) {
  if (i0 < 0 || n < 1 || i0 > B.nvecs - n) { qexhip_set_error("%s: vectors %d..%d of a basis of %d", who, i0, i0 + n - 1, B.nvecs); return QEXHIP_ERR_ARG; }
  return 0;
}
static int basis_geom_check(const qexhip_ctx *c, const EigBasis &B) {
  if (B.n2 != (size_t)c->g.ntile * 192) { qexhip_set_error("the basis was allocated for another lattice"); return QEXHIP_ERR_STATE; }
  return 0;
}
int eig_get_vector(qexhip_ctx *c, const EigBasis &B, int i, DevField &f, double scale) {
  CHK(basis_index_check(B, i, 1, "eig_get_vector"));
  CHK(basis_geom_check(c, B));
  k_eig_copy_scale<<<grid_for(B.n2), 256, 0, c->stream>>>(f.par(0), B.v + (size_t)i * B.n2, scale, B.n2);
  HIPCHK(hipGetLastError());
  return 0;
}
int eig_set_vector(qexhip_ctx *c, EigBasis &B, int i, const DevField &f, double scale) {
  CHK(basis_index_check(B, i, 1, "eig_set_vector"));
  CHK(basis_geom_check(c, B));
  k_eig_copy_scale<<<grid_for(B.n2), 256, 0, c->stream>>>(B.v + (size_t)i * B.n2, f.par(0), scale, B.n2);
  HIPCHK(hipGetLastError());
  B.nevals = std::min(B.nevals, i);
  B.gen = c->links_gen;
  return 0;
}
int eig_move_vector(qexhip_ctx *c, EigBasis &B, int dst, int src) {
  CHK(basis_index_check(B, dst, 1, "eig_move_vector"));
  CHK(basis_index_check(B, src, 1, "eig_move_vector"));
  if (dst == src) return 0;
  HIPCHK(hipMemcpyAsync(B.v + (size_t)dst * B.n2, B.v + (size_t)src * B.n2, B.n2 * sizeof(double2), hipMemcpyDeviceToDevice, c->stream));
  return 0;
}

// ---------------- block dot ----------------
// One wavefront per 64-site tile (grid-stride over the tiles): the three colours of w's tile stay in registers, the tiles of the n
// basis vectors stream past.  Per vector: wave_sum (reduce.h), lane 0 adds the tile's value to the wave's accumulator in LDS -- tiles
// in ascending order, so the order is fixed -- then the four waves are combined in a fixed order and one partial per workgroup and
// vector is written: parts[(2 j + re|im) * nwg + workgroup].  k_block_dot_final sums the workgroups in a fixed order.  Bit-identical
// run to run.  Lanes past the last site of a ragged last tile load nothing and contribute exact zeros.
__global__ void __launch_bounds__(256) k_block_dot(const double2 *__restrict__ V, size_t n2, int n, const double2 *__restrict__ w,
                                                   int ntile, int Vh, double *__restrict__ parts) {
  __shared__ double2 acc[4][EIG_NJ];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int j = lane; j < n; j += 64) acc[wave][j] = make_double2(0, 0);
  __syncthreads();
  for (int tile = blockIdx.x * 4 + wave; tile < ntile; tile += gridDim.x * 4) {
    const bool valid = tile * 64 + lane < Vh;
    const size_t base = (size_t)tile * 192 + lane;
    const double2 z = make_double2(0, 0);
    const double2 w0 = valid ? w[base] : z, w1 = valid ? w[base + 64] : z, w2 = valid ? w[base + 128] : z;
    for (int j0 = 0; j0 < n; j0 += 4) {          // four vectors' loads in flight before the first reduction
      double2 a[4], b[4], d[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int j = j0 + u < n ? j0 + u : n - 1;
        const double2 *v = V + (size_t)j * n2 + base;
        a[u] = valid ? v[0] : z; b[u] = valid ? v[64] : z; d[u] = valid ? v[128] : z;
      }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        if (j0 + u >= n) break;
        // conj(v) w: the fma chains of k_cdot, colour by colour
        double ar = fma(a[u].x, w0.x, a[u].y * w0.y), ai = fma(a[u].x, w0.y, -a[u].y * w0.x);
        ar = fma(b[u].x, w1.x, fma(b[u].y, w1.y, ar)); ai = fma(b[u].x, w1.y, fma(-b[u].y, w1.x, ai));
        ar = fma(d[u].x, w2.x, fma(d[u].y, w2.y, ar)); ai = fma(d[u].x, w2.y, fma(-d[u].y, w2.x, ai));
        ar = wave_sum(ar);
        ai = wave_sum(ai);
        if (lane == 0) { acc[wave][j0 + u].x += ar; acc[wave][j0 + u].y += ai; }
      }
    }
  }
  __syncthreads();
  const int nwg = gridDim.x;
  for (int j = threadIdx.x; j < n; j += 256) {
    parts[(size_t)(2 * j) * nwg + blockIdx.x] = (acc[0][j].x + acc[1][j].x) + (acc[2][j].x + acc[3][j].x);
    parts[(size_t)(2 * j + 1) * nwg + blockIdx.x] = (acc[0][j].y + acc[1][j].y) + (acc[2][j].y + acc[3][j].y);
  }
}
// out[b] = sum over the workgroups of parts[b * nwg + g], b = 2 j + re|im
__global__ void __launch_bounds__(256) k_block_dot_final(const double *__restrict__ parts, int nwg, double *__restrict__ out) {
  const double *p = parts + (size_t)blockIdx.x * nwg;
  double a = 0;
  for (int g = threadIdx.x; g < nwg; g += 256) a += p[g];
  const double r = block_sum_256(a);
  if (threadIdx.x == 0) out[blockIdx.x] = r;
}
int eig_block_dot(qexhip_ctx *c, const EigBasis &B, int i0, int n, const DevField &w, double2 *dots) {
  CHK(basis_index_check(B, i0, n, "eig_block_dot"));
  CHK(basis_geom_check(c, B));
  EigWork *e;
  CHK(eig_work(c, &e));
  const int nwg = std::min(EIG_DOT_WG, (c->g.ntile + 3) / 4);
  {
    ScopedTimer tm(c, "eig_dot", c->stream);
    for (int j0 = 0; j0 < n; j0 += EIG_NJ) {
      const int nj = std::min(EIG_NJ, n - j0);
      k_block_dot<<<nwg, 256, 0, c->stream>>>(B.v + (size_t)(i0 + j0) * B.n2, B.n2, nj, w.par(0), c->g.ntile, c->g.Vh, e->parts);
      k_block_dot_final<<<2 * nj, 256, 0, c->stream>>>(e->parts, nwg, (double *)(dots + j0));
    }
    HIPCHK(hipGetLastError());
  }
  if (multi_rank(c)) CHK(comm_allreduce(c, (double *)dots, 2 * n));      // ONE rank sum of 2 n doubles
  return 0;
}

// The same for nrhs (<= 4) vectors w_k at once: a wavefront keeps the three colours of ALL w_k tiles in registers (12 double2 at most)
// and every basis element is loaded once for all of them.  Tile -> wave -> workgroup mapping, nwg, the fma chains, wave_sum and
// every summation order are those of k_block_dot / k_block_dot_final, so the number (k, j) is bit for bit what eig_block_dot returns
// for w_k alone.  parts[((k n + j) 2 + re|im) * nwg + workgroup]; LDS acc[4][NRHS][EIG_NJ] = 32 KiB at NRHS = 4.
struct EigMrhsPtrs { const double2 *w[EIG_MAXRHS]; double2 *y[EIG_MAXRHS]; };
template <int NRHS>
__global__ void __launch_bounds__(256) k_block_dot_mrhs(const double2 *__restrict__ V, size_t n2, int n, EigMrhsPtrs P, int ntile, int Vh,
                                                        double *__restrict__ parts) {
  __shared__ double2 acc[4][NRHS][EIG_NJ];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < NRHS; k++)
    for (int j = lane; j < n; j += 64) acc[wave][k][j] = make_double2(0, 0);
  __syncthreads();
  for (int tile = blockIdx.x * 4 + wave; tile < ntile; tile += gridDim.x * 4) {
    const bool valid = tile * 64 + lane < Vh;
    const size_t base = (size_t)tile * 192 + lane;
    const double2 z = make_double2(0, 0);
    double2 w0[NRHS], w1[NRHS], w2[NRHS];
#pragma unroll
    for (int k = 0; k < NRHS; k++) {
      const double2 *w = P.w[k];
      w0[k] = valid ? w[base] : z; w1[k] = valid ? w[base + 64] : z; w2[k] = valid ? w[base + 128] : z;
    }
    for (int j0 = 0; j0 < n; j0 += 4) {          // four vectors' loads in flight before the first reduction
      double2 a[4], b[4], d[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int j = j0 + u < n ? j0 + u : n - 1;
        const double2 *v = V + (size_t)j * n2 + base;
        a[u] = valid ? v[0] : z; b[u] = valid ? v[64] : z; d[u] = valid ? v[128] : z;
      }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        if (j0 + u >= n) break;
#pragma unroll
        for (int k = 0; k < NRHS; k++) {
          double ar = fma(a[u].x, w0[k].x, a[u].y * w0[k].y), ai = fma(a[u].x, w0[k].y, -a[u].y * w0[k].x);
          ar = fma(b[u].x, w1[k].x, fma(b[u].y, w1[k].y, ar)); ai = fma(b[u].x, w1[k].y, fma(-b[u].y, w1[k].x, ai));
          ar = fma(d[u].x, w2[k].x, fma(d[u].y, w2[k].y, ar)); ai = fma(d[u].x, w2[k].y, fma(-d[u].y, w2[k].x, ai));
          ar = wave_sum(ar);
          ai = wave_sum(ai);
          if (lane == 0) { acc[wave][k][j0 + u].x += ar; acc[wave][k][j0 + u].y += ai; }
        }
      }
    }
  }
  __syncthreads();
  const int nwg = gridDim.x;
  for (int i = threadIdx.x; i < NRHS * n; i += 256) {
    const int k = i / n, j = i - k * n;
    parts[(size_t)(2 * i) * nwg + blockIdx.x] = (acc[0][k][j].x + acc[1][k][j].x) + (acc[2][k][j].x + acc[3][k][j].x);
    parts[(size_t)(2 * i + 1) * nwg + blockIdx.x] = (acc[0][k][j].y + acc[1][k][j].y) + (acc[2][k][j].y + acc[3][k][j].y);
  }
}
// k_block_dot_final's sum for right-hand side blockIdx.y: out[k][j0 + j] of an [nrhs][ntot] array (ntot2 = 2 ntot doubles per row)
__global__ void __launch_bounds__(256) k_block_dot_final_mrhs(const double *__restrict__ parts, int nwg, int nj2, double *__restrict__ out, int ntot2) {
  const double *p = parts + ((size_t)blockIdx.y * nj2 + blockIdx.x) * nwg;
  double a = 0;
  for (int g = threadIdx.x; g < nwg; g += 256) a += p[g];
  const double r = block_sum_256(a);
  if (threadIdx.x == 0) out[(size_t)blockIdx.y * ntot2 + blockIdx.x] = r;
}
int eig_block_dot_mrhs(qexhip_ctx *c, const EigBasis &B, int i0, int n, int nrhs, DevField *const *w, double2 *dots) {
  CHK(basis_index_check(B, i0, n, "eig_block_dot_mrhs"));
  CHK(basis_geom_check(c, B));
  if (nrhs < 1 || nrhs > EIG_MAXRHS) { qexhip_set_error("eig_block_dot_mrhs: 1 <= nrhs <= %d", EIG_MAXRHS); return QEXHIP_ERR_ARG; }
  EigWork *e;
  CHK(eig_work(c, &e));
  if (!e->parts_mrhs) HIPCHK(hipMalloc((void **)&e->parts_mrhs, sizeof(double) * 2 * EIG_NJ * EIG_DOT_WG * EIG_MAXRHS));
  const int nwg = std::min(EIG_DOT_WG, (c->g.ntile + 3) / 4);
  EigMrhsPtrs P;
  memset(&P, 0, sizeof P);
  for (int k = 0; k < nrhs; k++) P.w[k] = w[k]->par(0);
  {
    ScopedTimer tm(c, "eig_dot", c->stream);
    for (int j0 = 0; j0 < n; j0 += EIG_NJ) {
      const int nj = std::min(EIG_NJ, n - j0);
      const double2 *V = B.v + (size_t)(i0 + j0) * B.n2;
      switch (nrhs) {
        case 1: k_block_dot_mrhs<1><<<nwg, 256, 0, c->stream>>>(V, B.n2, nj, P, c->g.ntile, c->g.Vh, e->parts_mrhs); break;
        case 2: k_block_dot_mrhs<2><<<nwg, 256, 0, c->stream>>>(V, B.n2, nj, P, c->g.ntile, c->g.Vh, e->parts_mrhs); break;
        case 3: k_block_dot_mrhs<3><<<nwg, 256, 0, c->stream>>>(V, B.n2, nj, P, c->g.ntile, c->g.Vh, e->parts_mrhs); break;
        default: k_block_dot_mrhs<4><<<nwg, 256, 0, c->stream>>>(V, B.n2, nj, P, c->g.ntile, c->g.Vh, e->parts_mrhs); break;
      }
      k_block_dot_final_mrhs<<<dim3(2 * nj, nrhs), 256, 0, c->stream>>>(e->parts_mrhs, nwg, 2 * nj, (double *)(dots + j0), 2 * n);
    }
    HIPCHK(hipGetLastError());
  }
  if (multi_rank(c)) CHK(comm_allreduce(c, (double *)dots, 2 * n * nrhs));      // ONE rank sum of 2 n nrhs doubles
  return 0;
}

// ---------------- block axpy ----------------
// y_i += scale * sum_j coef_j v_j,i: a lane owns element i, the coefficients are wave-uniform loads, eight basis loads in flight.
__global__ void __launch_bounds__(256) k_block_axpy(const double2 *__restrict__ V, size_t n2, int n, const double2 *__restrict__ coef,
                                                    double scale, double2 *y) {
  for (size_t i = blockIdx.x * 256 + threadIdx.x; i < n2; i += (size_t)gridDim.x * 256) {
    double sr = 0, si = 0;
    const double2 *v = V + i;
#pragma unroll 8
    for (int j = 0; j < n; j++) {
      const double2 cf = coef[j], x = v[(size_t)j * n2];
      sr = fma(cf.x, x.x, fma(-cf.y, x.y, sr));
      si = fma(cf.x, x.y, fma(cf.y, x.x, si));
    }
    double2 yv = y[i];
    yv.x = fma(scale, sr, yv.x);
    yv.y = fma(scale, si, yv.y);
    y[i] = yv;
  }
}
int eig_block_axpy(qexhip_ctx *c, const EigBasis &B, int i0, int n, const double2 *coef, double scale, DevField &y) {
  CHK(basis_index_check(B, i0, n, "eig_block_axpy"));
  CHK(basis_geom_check(c, B));
  ScopedTimer tm(c, "eig_axpy", c->stream);
  k_block_axpy<<<grid_for(B.n2), 256, 0, c->stream>>>(B.v + (size_t)i0 * B.n2, B.n2, n, coef, scale, y.par(0));
  HIPCHK(hipGetLastError());
  return 0;
}

// y_k += scale * sum_j coef[k][j] v_j for nrhs (<= 4) fields at once: every basis element is loaded once, and the fma order over j is
// k_block_axpy's, so each y_k is bit for bit what eig_block_axpy gives with its own coefficients.
template <int NRHS>
__global__ void __launch_bounds__(256) k_block_axpy_mrhs(const double2 *__restrict__ V, size_t n2, int n, const double2 *__restrict__ coef,
                                                         double scale, EigMrhsPtrs P) {
  for (size_t i = blockIdx.x * 256 + threadIdx.x; i < n2; i += (size_t)gridDim.x * 256) {
    double sr[NRHS], si[NRHS];
#pragma unroll
    for (int k = 0; k < NRHS; k++) sr[k] = si[k] = 0;
    const double2 *v = V + i;
#pragma unroll 8
    for (int j = 0; j < n; j++) {
      const double2 x = v[(size_t)j * n2];
#pragma unroll
      for (int k = 0; k < NRHS; k++) {
        const double2 cf = coef[k * n + j];
        sr[k] = fma(cf.x, x.x, fma(-cf.y, x.y, sr[k]));
        si[k] = fma(cf.x, x.y, fma(cf.y, x.x, si[k]));
      }
    }
#pragma unroll
    for (int k = 0; k < NRHS; k++) {
      double2 yv = P.y[k][i];
      yv.x = fma(scale, sr[k], yv.x);
      yv.y = fma(scale, si[k], yv.y);
      P.y[k][i] = yv;
    }
  }
}
// coef: [nrhs][n] on the device; the y_k are distinct fields
int eig_block_axpy_mrhs(qexhip_ctx *c, const EigBasis &B, int i0, int n, int nrhs, const double2 *coef, double scale, DevField *const *y) {
  CHK(basis_index_check(B, i0, n, "eig_block_axpy_mrhs"));
  CHK(basis_geom_check(c, B));
  if (nrhs < 1 || nrhs > EIG_MAXRHS) { qexhip_set_error("eig_block_axpy_mrhs: 1 <= nrhs <= %d", EIG_MAXRHS); return QEXHIP_ERR_ARG; }
  for (int k = 0; k < nrhs; k++)
    for (int q = 0; q < k; q++)
      if (y[k]->d == y[q]->d) { qexhip_set_error("eig_block_axpy_mrhs: outputs %d and %d are the same field", q, k); return QEXHIP_ERR_ARG; }
  EigMrhsPtrs P;
  memset(&P, 0, sizeof P);
  for (int k = 0; k < nrhs; k++) P.y[k] = y[k]->par(0);
  ScopedTimer tm(c, "eig_axpy", c->stream);
  const double2 *V = B.v + (size_t)i0 * B.n2;
  const int grid = grid_for(B.n2);
  switch (nrhs) {
    case 1: k_block_axpy_mrhs<1><<<grid, 256, 0, c->stream>>>(V, B.n2, n, coef, scale, P); break;
    case 2: k_block_axpy_mrhs<2><<<grid, 256, 0, c->stream>>>(V, B.n2, n, coef, scale, P); break;
    case 3: k_block_axpy_mrhs<3><<<grid, 256, 0, c->stream>>>(V, B.n2, n, coef, scale, P); break;
    default: k_block_axpy_mrhs<4><<<grid, 256, 0, c->stream>>>(V, B.n2, n, coef, scale, P); break;
  }
  HIPCHK(hipGetLastError());
  return 0;
}

// ---------------- block norm2 accumulate (low-mode averaging) ----------------
// cf.even(c).re += sum_j wgt_j sum_col |v_j(c, col)|^2: a lane owns site c of the even parity, the three colours of a vector are three
// lane-contiguous 16-byte loads, the weights are wave-uniform loads, eight vectors' loads in flight.  The arithmetic is k_trace_accum's
// with a == b (trace.hip), vector after vector in ascending j: n2 by its fma chain over the colours, then acc += wgt_j * n2 with the
// product and the sum rounded as written -- the bits of n times get_vector + trace_accum.  The imaginary part, the odd parity and the
// spare lanes of a ragged last tile are not written.
__global__ void __launch_bounds__(256) k_block_norm2_accum(const double2 *__restrict__ V, size_t n2, int n, const double *__restrict__ wgt,
                                                           int Vh, double2 *cf) {
#pragma clang fp contract(off)
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= Vh) return;
  const double2 *v = V + (size_t)(c >> 6) * 192 + (c & 63);
  double acc = cf[c].x;
#pragma unroll 8
  for (int j = 0; j < n; j++) {
    const double2 *vj = v + (size_t)j * n2;
    const double2 x0 = vj[0], x1 = vj[64], x2 = vj[128];
    double s = 0.0;
    s = fma(x0.x, x0.x, fma(x0.y, x0.y, s));
    s = fma(x1.x, x1.x, fma(x1.y, x1.y, s));
    s = fma(x2.x, x2.x, fma(x2.y, x2.y, s));
    acc += wgt[j] * s;
  }
  cf[c].x = acc;
}
// wgt: n doubles on the device
int eig_block_norm2_accum(qexhip_ctx *c, const EigBasis &B, int i0, int n, const double *wgt, DevCField &cf) {
  CHK(basis_index_check(B, i0, n, "eig_block_norm2_accum"));
  CHK(basis_geom_check(c, B));
  if (cf.half != (size_t)c->g.ntile * 64) { qexhip_set_error("eig_block_norm2_accum: the cfield was allocated for another lattice"); return QEXHIP_ERR_STATE; }
  ScopedTimer tm(c, "eig_norm2", c->stream);
  k_block_norm2_accum<<<(c->g.Vh + 255) / 256, 256, 0, c->stream>>>(B.v + (size_t)i0 * B.n2, B.n2, n, wgt, c->g.Vh, cf.par(0));
  HIPCHK(hipGetLastError());
  return 0;
}

// ---------------- low-mode averaging of the scalar trace: L(x) and phi <- (1 - P) phi ----------------
// P projects onto span{(v_i, 0), (0, D_oe v_i / sqrt(lambda_i)) : i < nev} (lambda_i <= 0: no odd partner).  Both need the Rayleigh
// quotients and a basis of the operator's present links.
static int lowmode_check(qexhip_ctx *c, EigBasis &B, int nev, const char *who) {
  if (nev < 0 || nev > B.nvecs) { qexhip_set_error("%s: nev = %d of a basis of %d vectors", who, nev, B.nvecs); return QEXHIP_ERR_ARG; }
  CHK(basis_geom_check(c, B));
  if (B.gen != c->links_gen) { qexhip_set_error("%s: the basis was computed on other links (the operator's links changed since)", who); return QEXHIP_ERR_STATE; }
  return 0;
}
// cf.re += L(x) = sum_i m/(m^2 + lambda_i) |v_i(x)|^2 (x even), ... |(D_oe v_i)(x)|^2 / lambda_i (x odd)
int eig_lowmode_diag(qexhip_ctx *c, EigBasis &B, int nev, double mass, DevCField &cf) {
  CHK(lowmode_check(c, B, nev, "eig_lowmode_diag"));
  if (nev == 0) return 0;
  CHK(eig_rayleigh(c, B, nev));
  EigWork *e;
  CHK(eig_work(c, &e));
  std::vector<double> w(nev);
  for (int i = 0; i < nev; i++) w[i] = mass / (mass * mass + B.evals[i]);
  double *dw = (double *)e->coef;
  HIPCHK(hipMemcpyAsync(dw, w.data(), sizeof(double) * nev, hipMemcpyHostToDevice, c->stream));
  CHK(eig_block_norm2_accum(c, B, 0, nev, dw, cf));
  HIPCHK(hipStreamSynchronize(c->stream));              // (w is read by the copy above)
  // odd sites, one vector after the other: g.odd = D_oe v_i; g.even = 0 and stays 0 (the odd sweep writes the odd half only).  Every
  // launch is on the one stream and the accumulation takes one vector at a time, so more work fields would buy nothing.
  DevField *v, *g;
  CHK(eig_field(c, EIG_T0, &v));
  CHK(eig_field(c, EIG_BZ, &g));
  CHK(blas_zero(c, *g, 0));
  for (int i = 0; i < nev; i++) {
    if (!(B.evals[i] > 0)) continue;
    CHK(eig_get_vector(c, B, i, *v));
    CHK(op_stagD_pub(c, *g, *v, 1, 0.0, 1.0, 0.0));
    CHK(trace_accum(c, cf, 1, &g, &g, w[i] / B.evals[i]));
  }
  return 0;
}

// phi_k <- (1 - P) phi_k in place on both parities, k < n <= 4 distinct fields:
//   even   phi_e -= V V^+ phi_e
//   odd    phi_o += D_oe V diag(1/lambda) V^+ D_eo phi_o
// one block_dot_mrhs and one block_axpy_mrhs per parity for all systems, two single-parity sweeps per system.
int eig_project_out(qexhip_ctx *c, EigBasis &B, int nev, int n, DevField *const *phi) {
  CHK(lowmode_check(c, B, nev, "eig_project_out"));
  if (nev == 0) return 0;
  CHK(eig_rayleigh(c, B, nev));
  double2 *dots, *coef;
  CHK(eig_coef_buffers(c, &dots, &coef));
  DevField *z[EIG_MAXRHS];
  for (int k = 0; k < n; k++) CHK(eig_field(c, EIG_BZ + k, &z[k]));
  std::vector<double2> h((size_t)n * nev);
  // even sites
  CHK(eig_block_dot_mrhs(c, B, 0, nev, n, phi, dots));
  HIPCHK(hipMemcpyAsync(h.data(), dots, sizeof(double2) * h.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (size_t q = 0; q < h.size(); q++) { h[q].x = -h[q].x; h[q].y = -h[q].y; }
  HIPCHK(hipMemcpyAsync(coef, h.data(), sizeof(double2) * h.size(), hipMemcpyHostToDevice, c->stream));
  CHK(eig_block_axpy_mrhs(c, B, 0, nev, n, coef, 1.0, phi));
  HIPCHK(hipStreamSynchronize(c->stream));              // (h is read by the copy above)
  // odd sites
  for (int k = 0; k < n; k++) CHK(op_stagD_pub(c, *z[k], *phi[k], 0, 0.0, 1.0, 0.0));        // z_k.even = D_eo phi_k.odd
  CHK(eig_block_dot_mrhs(c, B, 0, nev, n, z, dots));
  HIPCHK(hipMemcpyAsync(h.data(), dots, sizeof(double2) * h.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int k = 0; k < n; k++)
    for (int i = 0; i < nev; i++) {
      const double lam = B.evals[i], s = lam > 0 ? 1.0 / lam : 0.0;
      h[(size_t)k * nev + i].x *= s; h[(size_t)k * nev + i].y *= s;
    }
  HIPCHK(hipMemcpyAsync(coef, h.data(), sizeof(double2) * h.size(), hipMemcpyHostToDevice, c->stream));
  for (int k = 0; k < n; k++) CHK(blas_zero(c, *z[k], 0));
  CHK(eig_block_axpy_mrhs(c, B, 0, nev, n, coef, 1.0, z));
  HIPCHK(hipStreamSynchronize(c->stream));              // (h is read by the copy above)
  for (int k = 0; k < n; k++) {
    CHK(op_stagD_pub(c, *z[k], *z[k], 1, 0.0, 1.0, 0.0));                                     // z_k.odd = D_oe z_k.even
    CHK(blas_axpy(c, 1.0, *z[k], *phi[k], 1));
  }
  return 0;
}

// ---------------- in-place rotation ----------------
// V[:, c] <- sum_j V[:, j] Q[j, c], c < k, j < m, with no second copy of the basis.  A workgroup owns blocks of R consecutive rows
// (double2 elements): it loads the R x m inputs of a block into LDS ([j][R], 16-byte reads conflict-free), and only after the
// barrier writes the block's k outputs -- no other workgroup touches those rows.  A thread computes four output columns of one row
// at a time from one LDS read per j (vector FMA; v_mfma_f64_16x16x4_f64 fits the shape and was not needed to reach the streaming
// rate -- DESIGN.md section 4); Q comes through the cache, and with R = 64 its address is wave-uniform.  Columns k .. m-1 are left as
// they were.  R = 64 for m <= 128, 32 for m <= 256, 16 for m <= 512: m * R * 16 bytes <= 128 KiB of LDS.
template <int R>
__global__ void __launch_bounds__(256) k_rotate(double2 *V, size_t n2, int m, int k, const double *__restrict__ Q, size_t nblk) {
  extern __shared__ __attribute__((aligned(16))) char eig_smem[];
  double2 *s = (double2 *)eig_smem;
  constexpr int G = 256 / R;
  const int r = threadIdx.x % R;
  int c0 = threadIdx.x / R;
  if (R == 64) c0 = __builtin_amdgcn_readfirstlane(c0);
  for (size_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const size_t i0 = blk * R;
    for (int idx = threadIdx.x; idx < m * R; idx += 256) {
      const int j = idx / R, rr = idx % R;
      const size_t i = i0 + rr;
      s[idx] = i < n2 ? V[(size_t)j * n2 + i] : make_double2(0, 0);
    }
    __syncthreads();
    const size_t i = i0 + r;
    for (int c = c0; c < k; c += 4 * G) {
      const int ca = c, cb = c + G < k ? c + G : k - 1, cc = c + 2 * G < k ? c + 2 * G : k - 1, cd = c + 3 * G < k ? c + 3 * G : k - 1;
      const double *qa = Q + (size_t)ca * m, *qb = Q + (size_t)cb * m, *qc = Q + (size_t)cc * m, *qd = Q + (size_t)cd * m;
      double2 a = make_double2(0, 0), b = a, d = a, e = a;
#pragma unroll 4
      for (int j = 0; j < m; j++) {
        const double2 x = s[j * R + r];
        const double q0 = qa[j], q1 = qb[j], q2 = qc[j], q3 = qd[j];
        a.x = fma(q0, x.x, a.x); a.y = fma(q0, x.y, a.y);
        b.x = fma(q1, x.x, b.x); b.y = fma(q1, x.y, b.y);
        d.x = fma(q2, x.x, d.x); d.y = fma(q2, x.y, d.y);
        e.x = fma(q3, x.x, e.x); e.y = fma(q3, x.y, e.y);
      }
      if (i < n2) {
        V[(size_t)ca * n2 + i] = a;
        if (c + G < k) V[(size_t)cb * n2 + i] = b;
        if (c + 2 * G < k) V[(size_t)cc * n2 + i] = d;
        if (c + 3 * G < k) V[(size_t)cd * n2 + i] = e;
      }
    }
    __syncthreads();
  }
}
template <int R>
static int rotate_launch(qexhip_ctx *c, EigWork *e, int bit, EigBasis &B, int m, int k) {
  const size_t lds = (size_t)m * R * sizeof(double2);
  if (lds > 65536 && !(e->lds_attr & (1 << bit))) {
    HIPCHK(hipFuncSetAttribute((const void *)k_rotate<R>, hipFuncAttributeMaxDynamicSharedMemorySize, 131072));
    e->lds_attr |= 1 << bit;
  }
  const size_t nblk = (B.n2 + R - 1) / R;
  const int grid = (int)std::min<size_t>(nblk, 4096);
  k_rotate<R><<<grid, 256, lds, c->stream>>>(B.v, B.n2, m, k, e->Q, nblk);
  HIPCHK(hipGetLastError());
  return 0;
}
int eig_rotate(qexhip_ctx *c, EigBasis &B, int m, int k, const double *Q) {
  if (!Q || k < 1 || k > m || m > B.nvecs) { qexhip_set_error("eig_rotate: 1 <= k <= m <= nvecs (k = %d, m = %d, nvecs = %d)", k, m, B.nvecs); return QEXHIP_ERR_ARG; }
  CHK(basis_geom_check(c, B));
  EigWork *e;
  CHK(eig_work(c, &e));
  HIPCHK(hipMemcpyAsync(e->Q, Q, sizeof(double) * (size_t)m * k, hipMemcpyHostToDevice, c->stream));
  ScopedTimer tm(c, "eig_rotate", c->stream);
  B.nevals = 0;
  if (m <= 128) return rotate_launch<64>(c, e, 0, B, m, k);
  if (m <= 256) return rotate_launch<32>(c, e, 1, B, m, k);
  return rotate_launch<16>(c, e, 2, B, m, k);
}

// Rayleigh quotients of the leading n vectors where the basis does not hold them yet (vectors set by the caller)
int eig_rayleigh(qexhip_ctx *c, EigBasis &B, int n) {
  if (n > B.nvecs) return QEXHIP_ERR_ARG;
  DevField *t0, *ap;
  CHK(eig_field(c, EIG_T0, &t0));
  CHK(eig_field(c, EIG_AP, &ap));
  for (int i = B.nevals; i < n; i++) {
    CHK(eig_get_vector(c, B, i, *t0));
    CHK(op_xx(c, *ap, *t0, 0.0, 1, 0, nullptr));
    CHK(blas_redot(c, *t0, *ap, 0, &c->dscal[8]));
    CHK(blas_norm2(c, *t0, 0, &c->dscal[9]));
    double h[2];
    CHK(read_scalars(c, &c->dscal[8], 2, h));
    if (!(h[1] > 0)) { qexhip_set_error("basis vector %d is zero", i); return QEXHIP_ERR_STATE; }
    B.evals[i] = 0.25 * h[0] / h[1];
  }
  B.nevals = std::max(B.nevals, n);
  return 0;
}
