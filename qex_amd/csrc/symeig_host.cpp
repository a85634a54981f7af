// symeig_host.cpp -- dense real symmetric eigensolver on the host: cyclic Jacobi, no external library.
//
// What the thick-restart Lanczos (eigsolve.cpp) diagonalises at every restart: the projected matrix of the Krylov basis, an
// m x m real symmetric matrix (diagonal of kept Ritz values + the arrow row of their residual couplings + the tridiagonal of
// the new steps), m <= a few hundred.  The reference does the same job with its own svdbi / LAPACK calls
// (src/eigens/svdLanczos.nim, src/eigens/lapack.nim); here it is plain C++ so that the library needs nothing beyond ROCm, and
// a file without any HIP in it so that a host sanitizer build links it directly (tests/cpp/test_symeig_san.cpp).
//
// Cyclic Jacobi (Golub & Van Loan 8.5, the rotation of Rutishauser): every sweep annihilates each off-diagonal element once
// with a plane rotation.  It converges quadratically, its eigenvalues have small RELATIVE error on graded matrices, and the
// eigenvector matrix is a product of rotations -- orthogonal to rounding by construction.  O(n^3) per sweep, 6-10 sweeps:
// instant for the m <= 256 of a restart, seconds at n = 1024.
#include "../../include/qexhip.h"
#include <cmath>
#include <vector>
#include <algorithm>
#include <numeric>

// a: n x n, symmetric (column-major = row-major; only read).  w[n]: eigenvalues ascending.  z (may be null): n x n column-major,
// column i = the unit eigenvector of w[i].
extern "C" int qexhip_symeig_host(const double *a, int n, double *w, double *z) {
  if (n < 0 || (n > 0 && (!a || !w))) return QEXHIP_ERR_ARG;
  if (n == 0) return 0;
  const size_t N = (size_t)n;
  std::vector<double> A(a, a + N * N), V(N * N, 0.0);
  for (size_t i = 0; i < N; i++) V[i * N + i] = 1.0;
  // work on the symmetrised matrix: what an almost symmetric input (rounding) means
  double fro2 = 0;
  for (size_t i = 0; i < N; i++)
    for (size_t j = 0; j < i; j++) {
      const double s = 0.5 * (A[i * N + j] + A[j * N + i]);
      A[i * N + j] = A[j * N + i] = s;
    }
  for (size_t i = 0; i < N * N; i++) {
    if (!std::isfinite(A[i])) return QEXHIP_ERR_ARG;
    fro2 += A[i] * A[i];
  }
  const double tiny = 1e-290;
  for (int sweep = 0; sweep < 64; sweep++) {
    double off2 = 0;
    for (size_t p = 0; p < N; p++)
      for (size_t q = p + 1; q < N; q++) off2 += A[p * N + q] * A[p * N + q];
    if (2 * off2 <= 1e-34 * fro2 || off2 < tiny) break;      // |off|_F <= 1e-17 |A|_F: below the rounding of the diagonal
    for (size_t p = 0; p + 1 < N; p++) {
      for (size_t q = p + 1; q < N; q++) {
        const double apq = A[p * N + q];
        if (apq == 0.0) continue;
        const double app = A[p * N + p], aqq = A[q * N + q];
        // an element that no longer changes either diagonal entry is dropped (after the first sweeps, as Rutishauser does)
        if (sweep > 3 && std::fabs(app) + 100.0 * std::fabs(apq) == std::fabs(app) && std::fabs(aqq) + 100.0 * std::fabs(apq) == std::fabs(aqq)) {
          A[p * N + q] = A[q * N + p] = 0.0;
          continue;
        }
        const double theta = 0.5 * (aqq - app) / apq;
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));   // the smaller root: |angle| <= pi/4
        const double cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;
        A[p * N + p] = app - t * apq;
        A[q * N + q] = aqq + t * apq;
        A[p * N + q] = A[q * N + p] = 0.0;
        for (size_t k = 0; k < N; k++) {
          if (k == p || k == q) continue;
          const double akp = A[k * N + p], akq = A[k * N + q];
          const double np_ = cs * akp - sn * akq, nq_ = sn * akp + cs * akq;
          A[k * N + p] = A[p * N + k] = np_;
          A[k * N + q] = A[q * N + k] = nq_;
        }
        double *vp = &V[p * N], *vq = &V[q * N];     // V kept column-major: column p is contiguous
        for (size_t k = 0; k < N; k++) {
          const double a0 = vp[k], b0 = vq[k];
          vp[k] = cs * a0 - sn * b0;
          vq[k] = sn * a0 + cs * b0;
        }
      }
    }
  }
  if (z && N > 1) {
    // the product of ~5 n^2 rotations has lost orthogonality at the level sqrt(5 n) eps per column pair (1e-13 at n = 200): one
    // Newton-Schulz step V <- V (3 - V^T V) / 2 squares that error; what remains is the rounding of the step itself
    std::vector<double> M(N * N), Vn(N * N, 0.0);
    for (size_t p = 0; p < N; p++)
      for (size_t q = 0; q <= p; q++) {
        double g = 0;
        for (size_t k = 0; k < N; k++) g += V[p * N + k] * V[q * N + k];
        M[p * N + q] = M[q * N + p] = (p == q ? 1.5 : 0.0) - 0.5 * g;
      }
    for (size_t q = 0; q < N; q++)
      for (size_t p = 0; p < N; p++) {
        const double mpq = M[p * N + q];
        const double *vp = &V[p * N];
        double *vq = &Vn[q * N];
        for (size_t k = 0; k < N; k++) vq[k] += vp[k] * mpq;
      }
    V.swap(Vn);
  }
  std::vector<int> idx(N);
  std::iota(idx.begin(), idx.end(), 0);
  std::stable_sort(idx.begin(), idx.end(), [&](int i, int j) { return A[(size_t)i * N + i] < A[(size_t)j * N + j]; });
  for (size_t i = 0; i < N; i++) {
    w[i] = A[(size_t)idx[i] * N + idx[i]];
    if (z) std::copy(&V[(size_t)idx[i] * N], &V[(size_t)idx[i] * N] + N, z + i * N);
  }
  return 0;
}
