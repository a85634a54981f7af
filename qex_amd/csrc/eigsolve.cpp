// eigsolve.cpp -- host loop of the low-mode eigensolver: thick-restart Lanczos with Chebyshev acceleration on the even sites.
//
// The reference's src/eigens/hisqev.nim computes the lowest singular pairs of D_oe (sv_i, with sv_i^2 the eigenvalues of
// H = -D_eo D_oe on the even sites) by block Lanczos (svdLanczos.nim) and Rayleigh-Ritz passes, options EigOpts{nev, nvecs, relerr,
// abserr, maxup}.  The contract kept here is the eigenpairs, not its iteration path: the algorithm is the thick-restart Lanczos of
// Wu & Simon (SIAM J. Matrix Anal. Appl. 22 (2000) 602) on B = T_p(s(H)), s mapping [cheb_lo, cheb_hi] onto [1, -1], so that the
// wanted eigenvalues lambda < cheb_lo of H are the LARGEST of B (T_p grows like cosh(p acosh s) outside [-1, 1]); p = 0 is plain
// Lanczos on H, wanted = smallest.
//   step j     w = B v_j (p operator applications, each with one fused vector update: t_{n+1} = (a/2) A(m2) t_n - t_{n-1} where
//              A(m2) = 4 (m2 + H) is op_xx and 2 s(H) = (a/2) A(b/a)); classical Gram-Schmidt twice against v_0..v_j (block dot +
//              block axpy, eig.hip); alpha_j = <v_j, w>, beta_j = |w|, v_{j+1} = w / beta_j
//   restart    at j = m = nvecs the projected matrix (diagonal of kept Ritz values + arrow + tridiagonal) is diagonalised on the
//              host (qexhip_symeig_host), the k wanted Ritz vectors are formed in place (eig_rotate), v_k = the last residual vector
// Convergence is judged on the Lanczos estimate |beta_m y_mi| (for p > 0 divided by |dB/dlambda| at the Ritz value); when the
// estimate says converged the TRUE residuals |H v - lambda v| are computed with the fp64 operator, and only they end the solve
// (an estimate that was too optimistic tightens the estimate's threshold tenfold and the iteration goes on).
#include "qexhip_internal.h"
#include "../../include/qexhip.h"
#include <cmath>
#include <vector>
#include <algorithm>
#include <numeric>

extern "C" int qexhip_eig_check_opts(const qexhip_eig_opts *o) {
  if (!o) return QEXHIP_ERR_ARG;
  auto bad = [](const char *what) { qexhip_set_error("eig options: %s", what); return QEXHIP_ERR_ARG; };
  if (o->nev < 1) return bad("nev < 1");
  if (o->nvecs < 1 || o->nvecs > EIG_MAX_NVECS) return bad("nvecs outside 1..512 (QEXHIP_EIG_MAX_NVECS)");
  if (o->nev > o->nvecs) return bad("nev > nvecs");
  if (!(o->relerr >= 0) || !(o->abserr >= 0) || !std::isfinite(o->relerr) || !std::isfinite(o->abserr)) return bad("relerr / abserr negative or not finite");
  if (o->max_restarts < 0) return bad("max_restarts < 0");
  if (o->cheb_degree < 0) return bad("cheb_degree < 0");
  if (o->cheb_degree > 0) {
    if (!(o->cheb_lo > 0) || !std::isfinite(o->cheb_lo)) return bad("cheb_lo must be > 0 with cheb_degree > 0");
    if (!(o->cheb_hi >= 0) || !std::isfinite(o->cheb_hi)) return bad("cheb_hi must be 0 (estimate it) or > cheb_lo");
    if (o->cheb_hi != 0 && !(o->cheb_hi > o->cheb_lo)) return bad("cheb_hi <= cheb_lo");
  }
  return 0;
}

namespace {
struct Lanczos {
  qexhip_ctx *c;
  EigBasis &B;
  DevField *F[2], *ap, *tw;      // tw: scratch of true_pair -- F[0] / F[1] may hold the residual vector a restart still needs
  int p = 0;
  double lo = 0, hi = 0;
  long ops = 0;

  // res = B in: returns the field that holds it (in or other; both are clobbered)
  int apply(DevField *in, DevField *other, DevField **res) {
    if (p == 0) {
      CHK(op_xx(c, *ap, *in, 0.0, 1, 0, nullptr));
      CHK(blas_axpby(c, 0.25, *ap, 0.0, *ap, *other, 0));
      ops++;
      *res = other;
      return 0;
    }
    const double a = -2.0 / (hi - lo), m2 = -0.5 * (hi + lo);      // s(H) = a H + b, b / a = m2
    DevField *P = in, *C = other;
    CHK(op_xx(c, *ap, *P, m2, 1, 0, nullptr));
    CHK(blas_axpby(c, 0.25 * a, *ap, 0.0, *ap, *C, 0));             // T_1 = s(H) v
    ops++;
    for (int n = 2; n <= p; n++) {
      CHK(op_xx(c, *ap, *C, m2, 1, 0, nullptr));
      CHK(blas_axpby(c, 0.5 * a, *ap, -1.0, *P, *P, 0));            // T_n = 2 s(H) T_{n-1} - T_{n-2}, over T_{n-2}
      ops++;
      std::swap(P, C);
    }
    *res = C;
    return 0;
  }
  // eigenvalue of H and |dB/dlambda| behind a Ritz value theta of B
  void unmap(double theta, double *lambda, double *slope) const {
    if (p == 0) { *lambda = theta; *slope = 1.0; return; }
    double s, d;
    if (theta > 1.0) {
      const double A = std::acosh(theta) / p;
      s = std::cosh(A);
      d = A > 1e-8 ? p * std::sinh(p * A) / std::sinh(A) : (double)p * p;
    } else {
      s = std::cos(std::acos(std::max(theta, -1.0)) / p);
      d = 1.0;
    }
    *lambda = 0.5 * (hi + lo - s * (hi - lo));
    *slope = d * 2.0 / (hi - lo);
  }
  // Rayleigh quotient and true residual of basis vector i
  int true_pair(int i, double *lambda, double *resid) {
    DevField *t0 = tw;
    CHK(eig_get_vector(c, B, i, *t0));
    CHK(op_xx(c, *ap, *t0, 0.0, 1, 0, nullptr));
    ops++;
    CHK(blas_redot(c, *t0, *ap, 0, &c->dscal[8]));
    CHK(blas_norm2(c, *t0, 0, &c->dscal[9]));
    double h[2];
    CHK(read_scalars(c, &c->dscal[8], 2, h));
    if (!(h[1] > 0)) { qexhip_set_error("eigs: Ritz vector %d is zero", i); return QEXHIP_ERR_STATE; }
    const double lam = 0.25 * h[0] / h[1];
    CHK(blas_axpby(c, 0.25, *ap, -lam, *t0, *ap, 0));
    CHK(blas_norm2(c, *ap, 0, &c->dscal[8]));
    double r2;
    CHK(read_scalars(c, &c->dscal[8], 1, &r2));
    *lambda = lam;
    *resid = std::sqrt(r2 / h[1]);
    return 0;
  }
};
}  // namespace

int eig_solve(qexhip_ctx *c, EigBasis &B, const qexhip_eig_opts &o, int *nconv_out, double *evals, double *resid, long stats[4]) {
  const int m = o.nvecs, nev = o.nev;
  DevField *f0, *f1, *ap, *tw;
  CHK(eig_field(c, EIG_W, &tw));
  CHK(eig_field(c, EIG_T0, &f0));
  CHK(eig_field(c, EIG_T1, &f1));
  CHK(eig_field(c, EIG_AP, &ap));
  double2 *d1, *d2;
  CHK(eig_coef_buffers(c, &d1, &d2));
  Lanczos L{c, B, {f0, f1}, ap, tw};
  L.p = o.cheb_degree; L.lo = o.cheb_lo; L.hi = o.cheb_hi;

  // start vector: the device Gaussian generator, seeded per GLOBAL site -- the same vector for any number of ranks
  {
    int glat[4] = {c->g.X[0], c->g.X[1], c->g.X[2], c->g.X[3] * c->rankGeom[3]};
    qexhip_rng *R = nullptr;
    CHK(qexhip_rng_new(&R, 0, o.seed, c->g.X, glat, c->rankCoord[3] * c->g.X[3]));
    int rc = rng_dev_generate(c, R, 0, f0, nullptr);
    qexhip_rng_free(R);
    CHK(rc);
    CHK(blas_norm2(c, *f0, 0, &c->dscal[8]));
    double n2;
    CHK(read_scalars(c, &c->dscal[8], 1, &n2));
    CHK(eig_set_vector(c, B, 0, *f0, 1.0 / std::sqrt(n2)));
  }
  // cheb_hi = 0: 1.1 x the largest Ritz value of 20 plain Lanczos steps (no re-orthogonalisation needed for the top of the spectrum)
  if (L.p > 0 && L.hi == 0.0) {
    const int ns = 20;
    std::vector<double> T((size_t)ns * ns, 0.0), w(ns);
    DevField *v = f0, *vp = f1;
    CHK(eig_get_vector(c, B, 0, *v));
    CHK(blas_zero(c, *vp, 0));
    double beta = 0;
    int done = 0;
    for (int s = 0; s < ns; s++) {
      CHK(op_xx(c, *ap, *v, 0.0, 1, 0, nullptr));
      L.ops++;
      CHK(blas_redot(c, *v, *ap, 0, &c->dscal[8]));
      double h;
      CHK(read_scalars(c, &c->dscal[8], 1, &h));
      const double alpha = 0.25 * h;
      CHK(blas_axpby(c, 0.25, *ap, -alpha, *v, *ap, 0));
      CHK(blas_axpy(c, -beta, *vp, *ap, 0));
      CHK(blas_norm2(c, *ap, 0, &c->dscal[8]));
      CHK(read_scalars(c, &c->dscal[8], 1, &h));
      T[(size_t)s * ns + s] = alpha;
      done = s + 1;
      beta = std::sqrt(h);
      if (!(beta > 1e-12 * std::fabs(alpha)) || s + 1 == ns) break;
      T[(size_t)s * ns + s + 1] = T[(size_t)(s + 1) * ns + s] = beta;
      CHK(blas_axpby(c, 1.0 / beta, *ap, 0.0, *ap, *vp, 0));
      std::swap(v, vp);
    }
    std::vector<double> Td((size_t)done * done);
    for (int i = 0; i < done; i++) for (int j = 0; j < done; j++) Td[(size_t)i * done + j] = T[(size_t)i * ns + j];
    CHK(qexhip_symeig_host(Td.data(), done, w.data(), nullptr));
    L.hi = 1.1 * w[done - 1];
    if (!(L.hi > L.lo)) { qexhip_set_error("eigs: cheb_lo = %g is not below the estimated top of the spectrum %g", L.lo, L.hi); return QEXHIP_ERR_ARG; }
  }

  std::vector<double> T((size_t)m * m, 0.0), theta(m), Y((size_t)m * m), Q((size_t)m * m);
  std::vector<double> lam(nev, 0.0), res(nev, 0.0);
  std::vector<double2> h1(m), h2(m);
  const bool largest = L.p > 0;
  int k0 = 0, restarts = 0;
  long steps = 0, checks = 0;
  double safety = 1.0;
  auto tol = [&](double l) { return std::max(o.abserr, o.relerr * std::fabs(l)); };
  for (;;) {
    DevField *r = nullptr;
    double betam = 0;
    for (int j = k0; j < m; j++, steps++) {
      CHK(eig_get_vector(c, B, j, *f0));
      CHK(L.apply(f0, f1, &r));
      CHK(eig_block_dot(c, B, 0, j + 1, *r, d1));
      CHK(eig_block_axpy(c, B, 0, j + 1, d1, -1.0, *r));
      CHK(eig_block_dot(c, B, 0, j + 1, *r, d2));
      CHK(eig_block_axpy(c, B, 0, j + 1, d2, -1.0, *r));
      CHK(blas_norm2(c, *r, 0, &c->dscal[8]));
      HIPCHK(hipMemcpyAsync(&h1[j], d1 + j, sizeof(double2), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipMemcpyAsync(&h2[j], d2 + j, sizeof(double2), hipMemcpyDeviceToHost, c->stream));
      double n2;
      CHK(read_scalars(c, &c->dscal[8], 1, &n2));
      const double alpha = h1[j].x + h2[j].x, beta = std::sqrt(n2);
      T[(size_t)j * m + j] = alpha;
      if (!std::isfinite(beta) || !(beta > 0)) { qexhip_set_error("eigs: Lanczos breakdown at step %d (|w| = %g)", j, beta); return QEXHIP_ERR_STATE; }
      if (j + 1 < m) {
        T[(size_t)j * m + j + 1] = T[(size_t)(j + 1) * m + j] = beta;
        CHK(eig_set_vector(c, B, j + 1, *r, 1.0 / beta));
      } else {
        betam = beta;
      }
    }
    CHK(qexhip_symeig_host(T.data(), m, theta.data(), Y.data()));
    std::vector<int> idx(m);
    for (int i = 0; i < m; i++) idx[i] = largest ? m - 1 - i : i;
    bool est_ok = true;
    for (int i = 0; i < nev; i++) {
      double l, slope;
      L.unmap(theta[idx[i]], &l, &slope);
      const double est = std::fabs(betam * Y[(size_t)idx[i] * m + m - 1]) / slope;
      if (!(est <= safety * tol(l)) || (largest && theta[idx[i]] <= 1.0)) est_ok = false;
    }
    const bool last = restarts >= o.max_restarts;
    int kk = std::min(nev + (m - nev) / 2, m - 1);
    const bool cannot_go_on = kk < nev;                  // nev == nvecs: the Ritz vectors fill the basis
    if ((est_ok || last) && cannot_go_on) kk = nev;
    if (kk > 0) {
      for (int i = 0; i < kk; i++) std::copy(&Y[(size_t)idx[i] * m], &Y[(size_t)idx[i] * m] + m, &Q[(size_t)i * m]);
      CHK(eig_rotate(c, B, m, kk, Q.data()));
    }
    if (est_ok || last) {
      checks++;
      bool all = true;
      for (int i = 0; i < nev; i++) {
        CHK(L.true_pair(i, &lam[i], &res[i]));
        if (!(res[i] <= tol(lam[i]))) all = false;
      }
      if (all || last || cannot_go_on) break;
      safety *= 0.1;
    }
    // thick restart: T = diag(kept Ritz values) + arrow of their couplings to v_k = the last residual vector
    std::fill(T.begin(), T.end(), 0.0);
    for (int i = 0; i < kk; i++) {
      T[(size_t)i * m + i] = theta[idx[i]];
      T[(size_t)i * m + kk] = T[(size_t)kk * m + i] = betam * Y[(size_t)idx[i] * m + m - 1];
    }
    CHK(eig_set_vector(c, B, kk, *r, 1.0 / betam));
    k0 = kk;
    restarts++;
  }
  // ascending Rayleigh quotients (the Ritz order is the eigenvalue order except among pairs closer than their errors)
  std::vector<int> perm(nev);
  std::iota(perm.begin(), perm.end(), 0);
  std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return lam[a] < lam[b]; });
  bool ident = true;
  for (int i = 0; i < nev; i++) ident = ident && perm[i] == i;
  if (!ident) {
    std::vector<double> P((size_t)nev * nev, 0.0);
    for (int i = 0; i < nev; i++) P[(size_t)i * nev + perm[i]] = 1.0;
    CHK(eig_rotate(c, B, nev, nev, P.data()));
  }
  int nconv = 0;
  for (int i = 0; i < nev; i++) {
    const double l = lam[perm[i]], rr = res[perm[i]];
    if (evals) evals[i] = l;
    if (resid) resid[i] = rr;
    B.evals[i] = l;
    if (rr <= tol(l)) nconv++;
  }
  B.nevals = nev;
  B.gen = c->links_gen;
  if (nconv_out) *nconv_out = nconv;
  if (stats) { stats[0] = L.ops; stats[1] = restarts; stats[2] = steps; stats[3] = checks; }
  return 0;
}
