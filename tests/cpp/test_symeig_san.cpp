// Stand-alone driver of qexhip_symeig_host (qex_amd/csrc/symeig_host.cpp) for a host AddressSanitizer + UBSan build: the file is
// compiled and linked directly, no library, no device, no Python.  Matrices: random real symmetric and arrow-plus-tridiagonal (the
// shape a thick restart leaves: diagonal of kept Ritz values, one coupling row, tridiagonal tail) for n in {0, 1, 2, 7, 40, 200},
// a matrix with repeated eigenvalues, the zero matrix, and the argument errors.  Checked without a reference solver:
//   |A z_i - w_i z_i| <= 1e-13 |A|_F,   |Z^T Z - 1| <= 1e-13,   w ascending,   sum w = trace A to 1e-13 |A|_F.
#include "qexhip.h"
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <vector>

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static double rnd() {       // xorshift64*, uniform in (-1, 1)
  g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
  return (double)((g_state * 0x2545F4914F6CDD1Dull) >> 11) / 4503599627370496.0 - 1.0;
}

static int check(const char *name, const std::vector<double> &A, int n) {
  std::vector<double> w(n > 0 ? n : 1), z((size_t)(n > 0 ? n : 1) * (n > 0 ? n : 1));
  int rc = qexhip_symeig_host(n ? A.data() : nullptr, n, w.data(), z.data());
  if (rc != 0) { printf("%s n=%d: rc %d\n", name, n, rc); return 1; }
  double fro = 0, tr = 0, sw = 0;
  for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) fro += A[(size_t)i * n + j] * A[(size_t)i * n + j];
  fro = std::sqrt(fro);
  const double bound = 1e-13 * (fro > 0 ? fro : 1.0);
  double worst_r = 0, worst_o = 0;
  int bad = 0;
  for (int i = 0; i < n; i++) {
    tr += A[(size_t)i * n + i]; sw += w[i];
    if (i && !(w[i] >= w[i - 1])) bad++;
    const double *zi = &z[(size_t)i * n];
    double r2 = 0;
    for (int r = 0; r < n; r++) {
      double s = 0;
      for (int k = 0; k < n; k++) s += A[(size_t)r * n + k] * zi[k];
      s -= w[i] * zi[r];
      r2 += s * s;
    }
    worst_r = std::fmax(worst_r, std::sqrt(r2));
    for (int j = 0; j <= i; j++) {
      const double *zj = &z[(size_t)j * n];
      double d = 0;
      for (int k = 0; k < n; k++) d += zi[k] * zj[k];
      worst_o = std::fmax(worst_o, std::fabs(d - (i == j ? 1.0 : 0.0)));
    }
  }
  const bool ok = !bad && worst_r <= bound && worst_o <= 1e-13 && std::fabs(tr - sw) <= bound * (n > 0 ? std::sqrt((double)n) : 1.0);
  printf("%-10s n=%3d  resid %.2e (bound %.2e)  orth %.2e  trace dev %.2e  %s\n", name, n, worst_r, bound, worst_o, std::fabs(tr - sw), ok ? "ok" : "FAILED");
  return ok ? 0 : 1;
}

int main() {
  int fails = 0;
  const int sizes[] = {0, 1, 2, 7, 40, 200};
  for (int n : sizes) {
    std::vector<double> A((size_t)n * n, 0.0);
    for (int i = 0; i < n; i++) for (int j = 0; j <= i; j++) A[(size_t)i * n + j] = A[(size_t)j * n + i] = rnd();
    fails += check("random", A, n);
    // arrow + tridiagonal: k kept values, their couplings to column k, a tridiagonal tail
    std::fill(A.begin(), A.end(), 0.0);
    const int k = n / 2;
    for (int i = 0; i < n; i++) A[(size_t)i * n + i] = 2.0 + rnd();
    for (int i = 0; i < k; i++) A[(size_t)i * n + k] = A[(size_t)k * n + i] = 1e-3 * rnd();
    for (int i = k; i + 1 < n; i++) A[(size_t)i * n + i + 1] = A[(size_t)(i + 1) * n + i] = 0.5 + 0.5 * std::fabs(rnd());
    fails += check("arrow", A, n);
  }
  {  // repeated eigenvalues: Householder-rotated diag(1, 1, 1, 2, 2, 5, 5, 5, 5, -3)
    const int n = 10;
    const double d[n] = {1, 1, 1, 2, 2, 5, 5, 5, 5, -3};
    std::vector<double> u(n), A((size_t)n * n);
    double un = 0;
    for (auto &x : u) { x = rnd(); un += x * x; }
    for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) {
      double s = 0;
      for (int k = 0; k < n; k++) s += ((i == k) - 2 * u[i] * u[k] / un) * d[k] * ((k == j) - 2 * u[k] * u[j] / un);
      A[(size_t)i * n + j] = s;
    }
    fails += check("repeated", A, n);
    std::vector<double> w(n);
    qexhip_symeig_host(A.data(), n, w.data(), nullptr);      // eigenvalues only
    const double expect[n] = {-3, 1, 1, 1, 2, 2, 5, 5, 5, 5};
    for (int i = 0; i < n; i++) if (std::fabs(w[i] - expect[i]) > 1e-13 * 12) { printf("repeated: w[%d] = %.17g\n", i, w[i]); fails++; }
    std::vector<double> Z((size_t)n * n, 0.0);
    fails += check("zero", Z, n);
  }
  {  // argument errors
    double a[4] = {1, 0, 0, 1}, w[2];
    if (qexhip_symeig_host(a, -1, w, nullptr) != QEXHIP_ERR_ARG) { printf("n = -1 accepted\n"); fails++; }
    if (qexhip_symeig_host(nullptr, 2, w, nullptr) != QEXHIP_ERR_ARG) { printf("a = NULL accepted\n"); fails++; }
    if (qexhip_symeig_host(a, 2, nullptr, nullptr) != QEXHIP_ERR_ARG) { printf("w = NULL accepted\n"); fails++; }
    a[1] = a[2] = NAN;
    if (qexhip_symeig_host(a, 2, w, nullptr) != QEXHIP_ERR_ARG) { printf("NaN accepted\n"); fails++; }
    if (qexhip_symeig_host(nullptr, 0, nullptr, nullptr) != 0) { printf("n = 0 refused\n"); fails++; }
  }
  printf(fails ? "symeig sanitizer run: %d FAILED\n" : "symeig sanitizer run: Passed\n", fails);
  return fails ? 1 : 0;
}
