// qexhip.hpp -- C++ host-side mirror of QEX's staggered operator / solver interface over the C ABI.
//
// QEX's host code is Nim compiled to C; the toolchain is not available in this build image, so
// this header is the compiled-language host layer above include/qexhip.h: same names, argument
// meaning and error behaviour as the reference, so a test written against it reads like the
// reference's own (tests/examples/testStagProp.nim, src/physics/stagSolve.nim:516-680):
//
//   Layout, ColorVector(), newGauge()         src/layout/layoutX.nim:70, src/physics/qcdTypes.nim
//   setBC / stagPhase / rephase               src/gauge/gaugeUtils.nim:124-131, src/physics/stagD.nim:72-80,509-520
//   newStag(g) / newStag3(g, g3)              src/physics/stagD.nim:522-564
//   Staggered::D / Ddag / eoReconstruct       src/physics/stagD.nim:566-586
//   Staggered::solveEE / solveOO / solve      src/physics/stagSolve.nim:134-138,224-294,347-446
//   SolverParams                              src/solvers/solverBase.nim:10-58
//   plaq / gaugeFlow                          src/gauge/gaugeUtils.nim:213-282, src/gauge/wflow.nim:21-67
//
// Header-only; link with -lqexhip.  Fields are std::vector<double> in the V=1 even-odd host format
// (colour vector [vol][3][2], gauge [vol][4][3][3][2]).  Errors throw qex::Error (QEX aborts with
// qexError, src/base/qexInternal.nim:37-45); not converging within maxits is not an error.
#pragma once
#include "qexhip.h"
#include <array>
#include <chrono>
#include <complex>
#include <stdexcept>
#include <string>
#include <vector>

namespace qex {

struct Error : std::runtime_error {
  using std::runtime_error::runtime_error;
};
inline void check(int rc) {
  if (rc != 0) throw Error(std::string("libqexhip error ") + std::to_string(rc) + ": " + qexhip_last_error());
}

using Field = std::vector<double>;

// V=1 even-odd layout of the rank-local lattice (src/layout/qlayout.nim:110-131)
struct Layout {
  std::array<int, 4> physGeom;
  int nSites, nEven;
  std::vector<std::array<int, 4>> coords;  // coords[idx]
  explicit Layout(const std::array<int, 4> &lat) : physGeom(lat) {
    nSites = lat[0] * lat[1] * lat[2] * lat[3];
    nEven = nSites / 2;
    coords.resize(nSites);
    std::array<int, 4> x;
    for (x[3] = 0; x[3] < lat[3]; x[3]++)
      for (x[2] = 0; x[2] < lat[2]; x[2]++)
        for (x[1] = 0; x[1] < lat[1]; x[1]++)
          for (x[0] = 0; x[0] < lat[0]; x[0]++) coords[index(x)] = x;
  }
  int index(const std::array<int, 4> &x) const {
    int lex = 0, p = 0;
    for (int i = 3; i >= 0; i--) lex = lex * physGeom[i] + x[i];
    for (int i = 0; i < 4; i++) p += x[i];
    return (p & 1) ? (lex + nSites) / 2 : lex / 2;
  }
  Field ColorVector() const { return Field((size_t)nSites * 6, 0.0); }
  Field newGauge() const { return Field((size_t)nSites * 72, 0.0); }
};

// U_3 *= -1 on the last t slice (gaugeUtils.nim:124-131)
inline void setBC(const Layout &lo, Field &g) {
  for (int s = 0; s < lo.nSites; s++)
    if (lo.coords[s][3] == lo.physGeom[3] - 1)
      for (int k = 0; k < 18; k++) g[((size_t)s * 4 + 3) * 18 + k] *= -1.0;
}
// eta_mu from the bit masks [8,9,11,0] (stagD.nim:509-520)
inline void stagPhase(const Layout &lo, Field &g, const std::array<int, 4> &phases = {8, 9, 11, 0}) {
  for (int mu = 0; mu < 4; mu++)
    for (int i = 0; i < lo.nSites; i++) {
      int s = 0;
      for (int k = 0; k < 4; k++) s += (phases[mu] >> k) & lo.coords[i][k];
      if (s & 1)
        for (int k = 0; k < 18; k++) g[((size_t)i * 4 + mu) * 18 + k] *= -1.0;
    }
}
inline void rephase(const Layout &lo, Field &g) { setBC(lo, g); stagPhase(lo, g); }

// solverBase.nim:10-58
struct SolverParams {
  double r2req = 1e-6;
  int maxits = 50000;
  int verbosity = 1;
  int sloppySolve = 0;         // SloppyNone / SloppySingle / SloppyHalf (solverBase.nim:8-15): > 0 = mixed-precision single-mass solves
  // outputs
  int calls = 0, iterations = 0, iterationsMax = 0;
  double seconds = 0, flops = 0, r2 = 0;
  int reliableUpdates = 0;     // sloppySolve > 0: fp64 true-residual updates
  std::vector<double> r2hist;  // "CG iteration: k  r2/b2:" values when histcap > 0 (fp64 solves only)
  void resetStats() { calls = iterations = iterationsMax = reliableUpdates = 0; seconds = flops = r2 = 0; r2hist.clear(); }
  int finalIterations() const { return iterations; }
};

class Context {
 public:
  qexhip_handle h = nullptr;
  Layout lo;
  explicit Context(const std::array<int, 4> &latLocal, int device = 0,
                   const std::array<int, 4> &rankGeom = {1, 1, 1, 1}, const std::array<int, 4> &rankCoord = {0, 0, 0, 0})
      : lo(latLocal) {
    check(qexhip_init(&h, device, latLocal.data(), rankGeom.data(), rankCoord.data()));
  }
  ~Context() { if (h) qexhip_finalize(h); }
  Context(const Context &) = delete;
  Context &operator=(const Context &) = delete;
  std::string info() const { char b[512]; check(qexhip_device_info(h, b, 512)); return b; }
  // multi-rank set-up as hipSetup of qexhip.nim: rank 0 calls uniqueId(), the host broadcasts it, every rank calls commInit
  static std::array<char, QEXHIP_UNIQUE_ID_BYTES> uniqueId() {
    std::array<char, QEXHIP_UNIQUE_ID_BYTES> id{};
    check(qexhip_comm_unique_id(id.data()));
    return id;
  }
  void commInit(const std::array<char, QEXHIP_UNIQUE_ID_BYTES> &id, int nranks, int rank) { check(qexhip_comm_init(h, id.data(), nranks, rank)); }
  // what RCCL reports for the communicator + the PCI bus id of the bound GPU
  struct CommInfo { int nranks, rank, device; std::string busId; };
  CommInfo commInfo() const {
    CommInfo ci{0, -1, 0, ""};
    char bus[64] = "";
    check(qexhip_comm_info(h, &ci.nranks, &ci.rank, &ci.device, bus, 64));
    ci.busId = bus;
    return ci;
  }
  void setOption(const char *name, int value) { check(qexhip_set_option(h, name, value)); }   // e.g. "flow_exp", 0
  // per system what the last batched sloppy call ran (qexhip_stag_sloppy_last_batch)
  struct SloppyLast { int precision = 0, halfIters = 0, f32Iters = 0, fellBack = 0; };
  std::vector<SloppyLast> sloppyLastBatch() const {
    int n = 0, p[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0}, fi[4] = {0, 0, 0, 0}, fb[4] = {0, 0, 0, 0};
    check(qexhip_stag_sloppy_last_batch(h, 4, &n, p, hi, fi, fb));
    std::vector<SloppyLast> out(n < 4 ? n : 4);
    for (size_t j = 0; j < out.size(); j++) out[j] = SloppyLast{p[j], hi[j], fi[j], fb[j]};
    return out;
  }
  // the batched 16-bit operator probe on resident fields (qexhip_dev_op_xx_half_batch)
  void devOpXXHalfBatch(const std::vector<int> &rIds, const std::vector<int> &xIds, const std::vector<double> &m2, bool parEven = true) {
    if (rIds.size() != xIds.size() || rIds.size() != m2.size()) throw std::invalid_argument("devOpXXHalfBatch: sizes differ");
    check(qexhip_dev_op_xx_half_batch(h, (int)rIds.size(), rIds.data(), xIds.data(), m2.data(), parEven ? 1 : 0));
  }
  // its fp32 twin (qexhip_dev_op_xx_sloppy_batch); both run t-sharded with setOption("batch_ranks", 1) on every rank
  void devOpXXSloppyBatch(const std::vector<int> &rIds, const std::vector<int> &xIds, const std::vector<double> &m2, bool parEven = true) {
    if (rIds.size() != xIds.size() || rIds.size() != m2.size()) throw std::invalid_argument("devOpXXSloppyBatch: sizes differ");
    check(qexhip_dev_op_xx_sloppy_batch(h, (int)rIds.size(), rIds.data(), xIds.data(), m2.data(), parEven ? 1 : 0));
  }
  // out[par] = r(M^+M) b[par] on resident fields, r(x) = f0 + sum_k alpha_k / (x + beta_k): one accumulating multi-shift solve
  // (qexhip_dev_rational_xx); returns the iterations of the base system
  int devRationalXX(int outId, int bId, double mass, double f0, const std::vector<double> &alpha, const std::vector<double> &beta,
                    double r2req, int maxits, bool parEven = true) {
    if (alpha.size() != beta.size()) throw std::invalid_argument("devRationalXX: sizes differ");
    int its = 0;
    check(qexhip_dev_rational_xx(h, outId, bId, mass, f0, (int)alpha.size(), alpha.data(), beta.data(), r2req, maxits, parEven ? 1 : 0,
                                 &its, nullptr, 0));
    return its;
  }
  static int deviceCount() { int n = 0; check(qexhip_device_count(&n)); return n; }
};

class Staggered {
  Context &c_;
  int nlinks_;
  double flops(int its) const { return double(nlinks_ * 4 * 72 + 60) * c_.lo.nEven * its; }  // stagSolve.nim:92
  template <class F> void timed(SolverParams &sp, int &its, F &&f) {
    auto t0 = std::chrono::steady_clock::now();
    f();
    sp.seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    sp.calls += 1; sp.iterations += its; sp.iterationsMax = std::max(sp.iterationsMax, its); sp.flops += flops(its);
  }

 public:
  Staggered(Context &c, const Field &g) : c_(c), nlinks_(4) { check(qexhip_stag_set_links(c.h, g.data(), nullptr)); }
  Staggered(Context &c, const Field &g, const Field &g3) : c_(c), nlinks_(8) { check(qexhip_stag_set_links(c.h, g.data(), g3.data())); }
  struct FromHisq {};   // links = HisqCoefs.smear(g) built on the device (hisqLinks.nim:32-43)
  struct FromNhyp { double alpha1, alpha2, alpha3; std::array<int, 4> antiperiodic{0, 0, 0, 1}; };   // rephase(nHYP(g))
  Staggered(Context &c, const Field &g, FromHisq) : c_(c), nlinks_(8) { check(qexhip_stag_set_links_hisq(c.h, g.data())); }
  Staggered(Context &c, const Field &g, const FromNhyp &h) : c_(c), nlinks_(4) {
    check(qexhip_stag_set_links_nhyp(c.h, g.data(), h.alpha1, h.alpha2, h.alpha3, h.antiperiodic.data(), nullptr));
  }
  // storage format chosen for the links: 0 = 18 reals, 1 = 2 rows + sign, 2 = 2 rows + determinant
  int linkFormat() const { int n = 0, f = 0; double d = 0; check(qexhip_stag_links_info(c_.h, &n, &f, &d)); return f; }
  void D(Field &r, const Field &x, double m) { check(qexhip_stag_D(c_.h, r.data(), x.data(), m, 1.0)); }
  void Ddag(Field &r, const Field &x, double m) { check(qexhip_stag_D(c_.h, r.data(), x.data(), m, -1.0)); }
  void stagD(Field &r, const Field &x, int subset, double m, double sc = 1.0, double a = 0.0) { check(qexhip_stag_stagD(c_.h, r.data(), x.data(), subset, m, sc, a)); }
  void eoReduce(Field &r, const Field &b, double m) { check(qexhip_stag_eo_reduce(c_.h, r.data(), b.data(), m)); }
  void eoReconstruct(Field &r, const Field &b, double m) { check(qexhip_stag_eo_reconstruct(c_.h, r.data(), b.data(), m)); }
  void stagD2(Field &r, const Field &x, int subset, double a, double b) { check(qexhip_stag_dslash(c_.h, r.data(), x.data(), subset, a, b)); }
  void stagD2ee(Field &r, const Field &x, double m2) { check(qexhip_stag_op_xx(c_.h, r.data(), x.data(), m2, 1)); }
  void stagD2oo(Field &r, const Field &x, double m2) { check(qexhip_stag_op_xx(c_.h, r.data(), x.data(), m2, 0)); }
  // solveXX(s, r, x, m, sp, parEven): r <- solution, x = rhs (stagSolve.nim:57-132)
  void solveXX(Field &r, const Field &x, double m, SolverParams &sp, bool parEven = true, int histcap = 0) {
    int its = 0; double fin = 0;
    if (sp.sloppySolve) {
      int nup = 0;
      timed(sp, its, [&] {
        check(qexhip_stag_solve_xx_sloppy(c_.h, r.data(), x.data(), m, sp.r2req, sp.maxits, parEven ? 1 : 0, sp.sloppySolve, &its, &fin, &nup));
      });
      sp.r2 = fin; sp.reliableUpdates += nup; sp.r2hist.clear();
      return;
    }
    std::vector<double> hist(histcap > 0 ? histcap : 1);
    timed(sp, its, [&] {
      check(qexhip_stag_solve_xx(c_.h, r.data(), x.data(), m, sp.r2req, sp.maxits, parEven ? 1 : 0, &its, &fin, hist.data(), histcap));
    });
    sp.r2 = fin;
    sp.r2hist.assign(hist.begin(), hist.begin() + (histcap > 0 ? std::min(histcap, its + 1) : 0));
  }
  // r <- r(M^+M) x on one parity for host fields (qexhip_stag_rational_xx; fp64 whatever sp.sloppySolve says)
  void rationalXX(Field &r, const Field &x, double m, double f0, const std::vector<double> &alpha, const std::vector<double> &beta,
                  SolverParams &sp, bool parEven = true, int histcap = 0) {
    if (alpha.size() != beta.size()) throw std::invalid_argument("rationalXX: sizes differ");
    int its = 0;
    std::vector<double> hist(histcap > 0 ? histcap : 1);
    timed(sp, its, [&] {
      check(qexhip_stag_rational_xx(c_.h, r.data(), x.data(), m, f0, (int)alpha.size(), alpha.data(), beta.data(), sp.r2req, sp.maxits,
                                    parEven ? 1 : 0, &its, hist.data(), histcap));
    });
    sp.r2hist.assign(hist.begin(), hist.begin() + (histcap > 0 ? std::min(histcap, its + 1) : 0));
  }
  void solveEE(Field &r, const Field &x, double m, SolverParams &sp, int histcap = 0) { solveXX(r, x, m, sp, true, histcap); }
  void solveOO(Field &r, const Field &x, double m, SolverParams &sp, int histcap = 0) { solveXX(r, x, m, sp, false, histcap); }
  // Staggered.solve(x, b, m, sp): full lattice, even-odd preconditioned, true-residual restarts
  void solve(Field &x, const Field &b, double m, SolverParams &sp) {
    int its = 0; double fin = 0;
    if (sp.sloppySolve) {
      int nup = 0;
      timed(sp, its, [&] { check(qexhip_stag_solve_sloppy(c_.h, x.data(), b.data(), m, sp.r2req, sp.maxits, 0, sp.sloppySolve, &its, &fin, &nup)); });
      sp.r2 = fin; sp.reliableUpdates += nup;
      return;
    }
    timed(sp, its, [&] { check(qexhip_stag_solve(c_.h, x.data(), b.data(), m, sp.r2req, sp.maxits, &its, &fin)); });
    sp.r2 = fin;
  }
  // convenience form used by the reference's tests: s.solve(v2, v1, m, 1e-8) (stagSolve.nim:462-472)
  void solve(Field &x, const Field &b, double m, double res) {
    SolverParams sp; sp.r2req = res * res; sp.maxits = 100000;
    solve(x, b, m, sp);
  }
  // hisqev (src/eigens/hisqev.nim): the nev lowest eigenpairs of H = -D_eo D_oe on the even sites (eigenvalues = sv^2) in a resident
  // basis of half-volume vectors; opts as EigOpts + the Chebyshev acceleration (qexhip_eig_opts).  The basis is freed with the object.
  struct EigBasis {
    Context &c; int id = 0, nconv = 0;
    std::vector<double> evals, resid;
    long stats[4] = {0, 0, 0, 0};        // operator applications, restarts, Lanczos steps, true-residual checks
    EigBasis(Context &c_, int nvecs) : c(c_) { check(qexhip_eig_new(c.h, nvecs, &id)); }
    ~EigBasis() { if (id) qexhip_eig_free(c.h, id); }
    EigBasis(const EigBasis &) = delete;
    EigBasis &operator=(const EigBasis &) = delete;
    // v_i as a full-volume host field (odd sites zero) / v_i := the even half of a host field
    void vector(int i, Field &out) const {
      int f = 0; check(qexhip_field_new(c.h, &f));
      int rc = qexhip_eig_get_vector(c.h, id, i, f);
      if (rc == 0) rc = qexhip_field_download(c.h, f, out.data());
      qexhip_field_free(c.h, f); check(rc);
    }
    void setVector(int i, const Field &in) {
      int f = 0; check(qexhip_field_new(c.h, &f));
      int rc = qexhip_field_upload(c.h, f, in.data());
      if (rc == 0) rc = qexhip_eig_set_vector(c.h, id, i, f);
      qexhip_field_free(c.h, f); check(rc);
    }
    // the three block kernels on a resident field (hooks): <v_j, w>, y += sum_j coef_j v_j, V[:, 0:k] <- V[:, 0:m] Q (column-major Q)
    void blockDot(int i0, int n, int wField, double *out) const { check(qexhip_eig_block_dot(c.h, id, i0, n, wField, out)); }
    void blockAxpy(int i0, int n, const double *coef, int yField) { check(qexhip_eig_block_axpy(c.h, id, i0, n, coef, yField)); }
    void rotate(int m, int k, const double *Q) { check(qexhip_eig_rotate(c.h, id, m, k, Q)); }
    // the two for nrhs <= 4 fields in one pass over the basis, bit for bit the single calls: out / coef [nrhs][n][2]
    void blockDotMulti(int i0, int n, const std::vector<int> &wFields, double *out) const {
      check(qexhip_eig_block_dot_multi(c.h, id, i0, n, (int)wFields.size(), wFields.data(), out));
    }
    void blockAxpyMulti(int i0, int n, const double *coef, const std::vector<int> &yFields) {
      check(qexhip_eig_block_axpy_multi(c.h, id, i0, n, (int)yFields.size(), coef, yFields.data()));
    }
    // low-mode averaging (cfield = TraceField::id): cfield.even.re += sum_j wgt[j] |v_{i0+j}|^2 (hook); cfield.re += L(x) of the leading
    // nev modes at mass m; phi_k <- (1 - P) phi_k in place for at most four resident fields
    void blockNorm2Accum(int i0, int n, const double *wgt, int cfield) const { check(qexhip_eig_block_norm2_accum(c.h, id, i0, n, wgt, cfield)); }
    void lowmodeDiag(int nev, double m, int cfield) const { check(qexhip_eig_lowmode_diag(c.h, id, nev, m, cfield)); }
    void projectOut(int nev, const std::vector<int> &fields) const {
      check(qexhip_eig_project_out(c.h, id, nev, (int)fields.size(), fields.data()));
    }
  };
  void eigs(EigBasis &B, const qexhip_eig_opts &o) {
    B.evals.assign(o.nev > 0 ? o.nev : 0, 0.0); B.resid = B.evals;
    check(qexhip_stag_eigs(c_.h, B.id, &o, &B.nconv, B.evals.data(), B.resid.data(), B.stats));
  }
  // the deflated solveEE of hisqev.nim:653-705 with the leading nev vectors of B; sp.r2 = the TRUE residual
  void solveEE(Field &r, const Field &x, double m, SolverParams &sp, const EigBasis &B, int nev) {
    int its = 0; double fin = 0;
    timed(sp, its, [&] { check(qexhip_stag_solve_xx_deflated(c_.h, B.id, nev, r.data(), x.data(), m, sp.r2req, sp.maxits, sp.sloppySolve, &its, &fin)); });
    sp.r2 = fin; sp.r2hist.clear();
  }
  // Staggered.solve whose inner solveEE calls deflate
  void solve(Field &x, const Field &b, double m, SolverParams &sp, const EigBasis &B, int nev) {
    int its = 0; double fin = 0;
    timed(sp, its, [&] { check(qexhip_stag_solve_deflated(c_.h, B.id, nev, x.data(), b.data(), m, sp.r2req, sp.maxits, sp.sloppySolve, &its, &fin)); });
    sp.r2 = fin;
  }
  // n <= 4 independent solves on these links in lock-step (one stream of the links per sweep for all of them);
  // per system the result of solve(x[j], b[j], m[j], sps[j]).  sloppy = -1: fp64, and a sloppy SolverParams is refused (as before);
  // 0, 1, 2: the precision of the batch, chosen explicitly (qexhip_stag_solve_batch_sloppy; when > 0: one rank, or t-sharded with option "batch_ranks" = 1), overriding
  // sps[j].sloppySolve; sps[j].reliableUpdates gets system j's updates
  void solveBatch(std::vector<Field> &xs, const std::vector<Field> &bs, const std::vector<double> &ms, std::vector<SolverParams> &sps,
                  int sloppy = -1) {
    const int n = (int)xs.size();
    if (sloppy < -1 || sloppy > 2) throw std::invalid_argument("solveBatch: sloppy = -1 (unset), 0, 1 or 2");
    if (sloppy < 0)
      for (auto &sp : sps)
        if (sp.sloppySolve) throw std::invalid_argument("sloppySolve: single-system solves only (pass sloppy = 1 to solveBatch for the mixed-precision batch)");
    std::vector<double *> xp; std::vector<const double *> bp; std::vector<double> rq, fin(n); std::vector<int> its(n), nup(n);
    int maxits = sps.at(0).maxits;
    for (int j = 0; j < n; j++) { xp.push_back(xs[j].data()); bp.push_back(bs.at(j).data()); rq.push_back(sps.at(j).r2req); maxits = std::min(maxits, sps[j].maxits); }
    auto t0 = std::chrono::steady_clock::now();
    if (sloppy < 0) check(qexhip_stag_solve_batch(c_.h, n, xp.data(), bp.data(), ms.data(), rq.data(), maxits, its.data(), fin.data()));
    else check(qexhip_stag_solve_batch_sloppy(c_.h, n, xp.data(), bp.data(), ms.data(), rq.data(), maxits, sloppy, its.data(), fin.data(), nup.data()));
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / n;
    for (int j = 0; j < n; j++) {
      SolverParams &sp = sps[j];
      sp.seconds += dt; sp.calls += 1; sp.iterations += its[j]; sp.iterationsMax = std::max(sp.iterationsMax, its[j]);
      sp.flops += flops(its[j]); sp.r2 = fin[j]; sp.reliableUpdates += nup[j];
    }
  }
  // the deflated lock-step batch (qexhip_stag_solve_batch_deflated / _xx_batch_deflated): n <= 4 systems, both parities deflated from
  // the even basis B with its leading nev vectors; sloppy = 0, 1 or 2 is the precision of the batched CG.  solveBatch: n x solve;
  // solveXXBatch: n x solveEE / solveOO, returning the true |b - A x|^2 / |b|^2 per system
  std::vector<double> deflatedBatch(std::vector<Field> &xs, const std::vector<Field> &bs, const std::vector<double> &ms,
                                    std::vector<SolverParams> &sps, const EigBasis &B, int nev, int sloppy, int xxParity) {
    const int n = (int)xs.size();
    if (sloppy < 0 || sloppy > 2) throw std::invalid_argument("deflated batch: sloppy = 0, 1 or 2");
    std::vector<double *> xp; std::vector<const double *> bp; std::vector<double> rq, fin(n); std::vector<int> its(n), nup(n);
    int maxits = sps.at(0).maxits;
    for (int j = 0; j < n; j++) { xp.push_back(xs[j].data()); bp.push_back(bs.at(j).data()); rq.push_back(sps.at(j).r2req); maxits = std::min(maxits, sps[j].maxits); }
    auto t0 = std::chrono::steady_clock::now();
    if (xxParity < 0) check(qexhip_stag_solve_batch_deflated(c_.h, B.id, nev, n, xp.data(), bp.data(), ms.data(), rq.data(), maxits, sloppy, its.data(), fin.data(), nup.data()));
    else check(qexhip_stag_solve_xx_batch_deflated(c_.h, B.id, nev, n, xp.data(), bp.data(), ms.data(), rq.data(), maxits, xxParity, sloppy, its.data(), fin.data(), nup.data()));
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / n;
    for (int j = 0; j < n; j++) {
      SolverParams &sp = sps[j];
      sp.seconds += dt; sp.calls += 1; sp.iterations += its[j]; sp.iterationsMax = std::max(sp.iterationsMax, its[j]);
      sp.flops += flops(its[j]); sp.r2 = fin[j]; sp.reliableUpdates += nup[j];
    }
    return fin;
  }
  void solveBatch(std::vector<Field> &xs, const std::vector<Field> &bs, const std::vector<double> &ms, std::vector<SolverParams> &sps,
                  const EigBasis &B, int nev, int sloppy = 0) {
    deflatedBatch(xs, bs, ms, sps, B, nev, sloppy, -1);
  }
  std::vector<double> solveXXBatch(std::vector<Field> &xs, const std::vector<Field> &bs, const std::vector<double> &ms,
                                   std::vector<SolverParams> &sps, const EigBasis &B, int nev, bool parEven = true, int sloppy = 0) {
    return deflatedBatch(xs, bs, ms, sps, B, nev, sloppy, parEven ? 1 : 0);
  }
  // multi-mass Staggered.solve(xs, b, ms, sp) (stagSolve.nim:347-446).  sloppy = -1: fp64, and a sloppy SolverParams is refused (as
  // before); 0, 1, 2: the precision of the inner multi-shift CG, chosen explicitly (qexhip_stag_solve_multi_sloppy), overriding
  // sp.sloppySolve; sp.reliableUpdates gets the updates
  void solve(std::vector<Field> &xs, const Field &b, const std::vector<double> &ms, SolverParams &sp, int sloppy = -1) {
    if (sloppy < -1 || sloppy > 2) throw std::invalid_argument("solve: sloppy = -1 (unset), 0, 1 or 2");
    if (sloppy < 0 && sp.sloppySolve)
      throw std::invalid_argument("sloppySolve: single-mass solves only (pass sloppy = 1 to solve for the mixed-precision multi-shift solve)");
    std::vector<double *> p;
    for (auto &x : xs) p.push_back(x.data());
    int its = 0, nup = 0; double fin = 0;
    if (sloppy < 0) timed(sp, its, [&] { check(qexhip_stag_solve_multi(c_.h, p.data(), b.data(), ms.data(), (int)ms.size(), sp.r2req, sp.maxits, &its, &fin)); });
    else timed(sp, its, [&] { check(qexhip_stag_solve_multi_sloppy(c_.h, p.data(), b.data(), ms.data(), (int)ms.size(), sp.r2req, sp.maxits, sloppy, &its, &fin, &nup)); });
    sp.r2 = fin; sp.reliableUpdates += nup;
  }
  // mixed-precision multi-shift solveXX (qexhip_stag_solve_xx_multi_sloppy): shifts[0] = base mass; returns the true
  // |b - A_k x_k|^2 / |b|^2 per shift; sp.iterations gets the fp32 iterations of phase 1, refineIterations (if given) those of phase 2
  std::vector<double> solveXXMulti(std::vector<Field> &xs, const Field &b, const std::vector<double> &shifts, SolverParams &sp,
                                   bool parEven = true, int sloppy = 1, std::vector<int> *refineIterations = nullptr) {
    std::vector<double *> p;
    for (auto &x : xs) p.push_back(x.data());
    const int n = (int)shifts.size();
    std::vector<double> r2(n);
    std::vector<int> ref(n);
    int its = 0, nup = 0;
    timed(sp, its, [&] {
      check(qexhip_stag_solve_xx_multi_sloppy(c_.h, p.data(), b.data(), shifts.data(), n, sp.r2req, sp.maxits, parEven ? 1 : 0, sloppy, &its,
                                              r2.data(), &nup, ref.data()));
    });
    sp.reliableUpdates += nup;
    sp.r2 = 0;
    for (double v : r2) sp.r2 = std::max(sp.r2, v);
    if (refineIterations) *refineIterations = ref;
    return r2;
  }
};
inline Staggered newStag(Context &c, const Field &g) { return Staggered(c, g); }
inline Staggered newStag3(Context &c, const Field &g, const Field &g3) { return Staggered(c, g, g3); }

// plaq(g) (gaugeUtils.nim:213-282)
inline std::array<double, 6> plaq(Context &c, const Field &g) {
  std::array<double, 6> p;
  check(qexhip_gauge_set(c.h, g.data()));
  check(qexhip_plaq(c.h, p.data()));
  return p;
}
// getGaugeFixTransform(t, g, dirs, gstop, orf) (gaugefix.nim:312-355) on the resident links, starting from t (resized to
// vol * 18 and set to the identity when empty); t stays resident for gaugeTransform.  Returns the iterations; metrics (may be
// null) receives met, gre, gro, gdsq of the last evaluation.
inline int getGaugeFixTransform(Context &c, Field &t, const std::vector<int> &dirs, double gstop = 1e-5, double orf = 1.8,
                                int maxits = 100000, double *metrics = nullptr) {
  if (!t.empty() && t.size() != (size_t)c.lo.nSites * 18) throw Error("getGaugeFixTransform: t must be empty or hold nSites * 18 doubles");
  check(qexhip_gfix_set_transform(c.h, t.empty() ? nullptr : t.data()));
  int its = 0;
  double m[4];
  check(qexhip_gauge_fix(c.h, dirs.data(), (int)dirs.size(), gstop, orf, maxits, &its, m, nullptr, 0));
  if (metrics) std::copy(m, m + 4, metrics);
  t.resize((size_t)c.lo.nSites * 18);
  check(qexhip_gfix_get_transform(c.h, t.data()));
  return its;
}
// gaugeTransform (gaugefix.nim:8-20) of the resident links by the resident t; linkTrace (gaugefix.nim:135-142)
inline void gaugeTransform(Context &c) { check(qexhip_gauge_transform(c.h)); }
inline double linkTrace(Context &c, const std::vector<int> &dirs) {
  double r = 0;
  check(qexhip_gauge_link_trace(c.h, dirs.data(), (int)dirs.size(), &r));
  return r;
}
// Stout smearing (src/gauge/stoutsmear.nim).  stoutSmear: ss.smear(g, fl) (:15-34), one step, nothing kept; fl may be g.
inline void stoutSmear(Context &c, const Field &g, double alpha, Field &fl) {
  fl.resize(g.size());
  check(qexhip_stout_smear(c.h, g.data(), alpha, fl.data()));
}
// ss.inverse(gf, fl) (:36-89): returns the iterations; rdf2 / diverging (may be null) as qexhip_stout_inverse
inline int stoutInverse(Context &c, Field &g, const Field &fl, double alpha, double rdf2req = 1e-24, int maxIter = 1000,
                        double *rdf2 = nullptr, bool *diverging = nullptr) {
  int its = 0, dv = 0;
  double r2 = 0;
  g.resize(fl.size());
  check(qexhip_stout_inverse(c.h, fl.data(), alpha, rdf2req, maxIter, g.data(), &its, &r2, &dv));
  if (rdf2) *rdf2 = r2;
  if (diverging) *diverging = dv != 0;
  return its;
}
// the n-level chain kept on the device: smearDeriv (:148-175) from the last level to the first, and smearedForce of
// tests/base/tstoutderiv.nim:137-143
class StoutSmearedForce {
  Context &c_;
 public:
  StoutSmearedForce(Context &c, const Field &g, const std::vector<double> &alphas, Field *fl) : c_(c) {
    if (fl) fl->resize(g.size());
    check(qexhip_stout_prepare(c.h, g.data(), alphas.data(), (int)alphas.size(), fl ? fl->data() : nullptr));
  }
  StoutSmearedForce(Context &c, const std::vector<double> &alphas) : c_(c) {      // the links resident on the device
    check(qexhip_stout_prepare(c.h, nullptr, alphas.data(), (int)alphas.size(), nullptr));
  }
  ~StoutSmearedForce() { qexhip_stout_release(c_.h); }
  StoutSmearedForce(const StoutSmearedForce &) = delete;
  void operator()(Field &f, const Field &chain) { check(qexhip_stout_force(c_.h, f.data(), chain.data())); }      // f may be chain
  void gaugeForce(Field &f, double plaq, double rect = 0, double adjplaq = 0) { check(qexhip_stout_gauge_force(c_.h, f.data(), plaq, rect, adjplaq)); }
  void gaugeForceResident(double plaq, double rect = 0, double adjplaq = 0) { check(qexhip_stout_gauge_force(c_.h, nullptr, plaq, rect, adjplaq)); }
};
// The complex site field `trce` of scalarTrace.nim, resident on the device, with the accumulation and slice sums on it; field
// arguments are ids of resident colour vectors (qexhip_field_new).
class TraceField {
  Context &c_;
 public:
  int id = 0;
  explicit TraceField(Context &c) : c_(c) { check(qexhip_cfield_new(c.h, &id)); }
  ~TraceField() { if (id) qexhip_cfield_free(c_.h, id); }
  TraceField(const TraceField &) = delete;
  void zero() { check(qexhip_cfield_zero(c_.h, id)); }
  void scale(double s) { check(qexhip_cfield_scale(c_.h, id, s)); }
  void axpy(double a, const TraceField &src) { check(qexhip_cfield_axpy(c_.h, id, a, src.id)); }     // this += a * src
  // trce += coef * a_k.dot b_k, k ascending (at most four pairs a call)
  void accum(const std::vector<int> &a, const std::vector<int> &b, double coef = 1.0) {
    if (a.size() != b.size()) throw Error("TraceField::accum: a and b differ in length");
    check(qexhip_dev_trace_accum(c_.h, id, (int)a.size(), a.data(), b.data(), coef));
  }
  std::vector<std::complex<double>> slices(int ntGlobal) {
    std::vector<double> o(2 * (size_t)ntGlobal);
    check(qexhip_dev_cfield_slices(c_.h, id, o.data()));
    std::vector<std::complex<double>> r(ntGlobal);
    for (int t = 0; t < ntGlobal; t++) r[t] = {o[2 * t], o[2 * t + 1]};
    return r;
  }
  void download(Field &out) {
    out.resize((size_t)c_.lo.nSites * 2);
    check(qexhip_cfield_download(c_.h, id, out.data()));
  }
  // conn4d.nim:223-229: Re trce(x) += scal |phi_k(x (+) pts[k])|^2, k ascending (at most four propagators a call; global points)
  void connAccum(const std::vector<int> &phi, const std::vector<std::array<int, 4>> &pts, double scal) {
    if (phi.size() != pts.size()) throw Error("TraceField::connAccum: phi and pts differ in length");
    check(qexhip_dev_conn_accum(c_.h, id, (int)phi.size(), phi.data(), pts.empty() ? nullptr : pts[0].data(), scal));
  }
  void stagSign() { check(qexhip_cfield_stag_sign(c_.h, id)); }     // trce(x) *= (-1)^(x0+x1+x2)  (conn4d.nim:238-245)
};
// pointSource (conn4d.nim:173-182): field ids[k] := 0, then 1 in colour ic[k] at the global point pts[k] (at most four a call)
inline void pointSource(Context &c, const std::vector<int> &ids, const std::vector<std::array<int, 4>> &pts, const std::vector<int> &ic) {
  if (ids.size() != pts.size() || ids.size() != ic.size()) throw Error("pointSource: ids, pts and ic differ in length");
  check(qexhip_dev_point_source(c.h, (int)ids.size(), ids.data(), pts.empty() ? nullptr : pts[0].data(), ic.data()));
}
enum DilutionKind { dkEvenOdd = 0, dkCorners3D = 1 };     // src/algorithms/dilution.nim
// dst_k = scale * src on the sites of global time t[k] in pattern idx[k], zero elsewhere (at most four destinations a call)
inline void dilute(Context &c, const std::vector<int> &dst, int src, DilutionKind kind, const std::vector<int> &idx, const std::vector<int> &t,
                   double scale = 1.0) {
  if (dst.size() != idx.size() || dst.size() != t.size()) throw Error("dilute: dst, idx and t differ in length");
  check(qexhip_dev_dilute(c.h, (int)dst.size(), dst.data(), src, (int)kind, idx.data(), t.data(), scale));
}
// g.gaugeFlow(steps, eps): measure(wflowT)  (wflow.nim:21-67); g is modified in place
template <class Measure>
inline void gaugeFlow(Context &c, Field &g, int steps, double eps, Measure &&measure) {
  check(qexhip_gauge_set(c.h, g.data()));
  for (int n = 1; n <= steps; n++) {
    check(qexhip_wflow(c.h, 1, eps));
    measure(n * eps);
  }
  check(qexhip_gauge_get(c.h, g.data()));
}
inline void gaugeFlow(Context &c, Field &g, int steps, double eps) {
  check(qexhip_gauge_set(c.h, g.data()));
  check(qexhip_wflow(c.h, steps, eps));
  check(qexhip_gauge_get(c.h, g.data()));
}

// HypCoefs (hypsmear.nim:15-18): smear, and smearGetForce as an object holding the device-resident closure
struct HypCoefs {
  double alpha1 = 0.4, alpha2 = 0.5, alpha3 = 0.5;
  void smear(Context &c, const Field &g, Field &fl) const { check(qexhip_nhyp_smear(c.h, g.data(), fl.data(), alpha1, alpha2, alpha3)); }
  class SmearedForce {
    Context &c_;
   public:
    SmearedForce(Context &c, const HypCoefs &h, const Field &g, Field *fl) : c_(c) {
      check(qexhip_nhyp_prepare(c.h, g.data(), h.alpha1, h.alpha2, h.alpha3, fl ? fl->data() : nullptr));
    }
    // smear the links resident on the device (ResidentMD below); forces are then left there too: gforceResident / fforceResident
    SmearedForce(Context &c, const HypCoefs &h) : c_(c) { check(qexhip_nhyp_prepare(c.h, nullptr, h.alpha1, h.alpha2, h.alpha3, nullptr)); }
    void gforceResident(double plaq, double rect = 0, double adjplaq = 0) { check(qexhip_nhyp_gauge_force(c_.h, nullptr, plaq, rect, adjplaq)); }
    std::vector<int> fforceResident(const std::vector<Field> &phi, const std::vector<double> &mass, const std::vector<double> &scale, double r2req,
                                    int maxits = 1000000, const std::array<int, 4> &antiperiodic = {0, 0, 0, 1}) {
      std::vector<const double *> p;
      for (auto &v : phi) p.push_back(v.data());
      std::vector<double> rq(p.size(), r2req);
      std::vector<int> its(p.size(), 0);
      check(qexhip_nhyp_fforce(c_.h, nullptr, (int)p.size(), p.data(), mass.data(), scale.data(), rq.data(), maxits, antiperiodic.data(), nullptr, its.data()));
      return its;
    }
    ~SmearedForce() { qexhip_nhyp_release(c_.h); }
    SmearedForce(const SmearedForce &) = delete;
    void operator()(Field &f, const Field &chain) { check(qexhip_nhyp_force(c_.h, f.data(), chain.data())); }   // smearedForce(f, chain)
    void gforce(Field &f, double plaq, double rect = 0, double adjplaq = 0) { check(qexhip_nhyp_gauge_force(c_.h, f.data(), plaq, rect, adjplaq)); }
    void fforce(Field &f, const std::vector<Field> &psi, const std::vector<double> &scale, const std::array<int, 4> &antiperiodic = {0, 0, 0, 1}) {
      std::vector<const double *> p;
      for (auto &v : psi) p.push_back(v.data());
      check(qexhip_nhyp_fermion_force(c_.h, f.data(), p.data(), scale.data(), (int)p.size(), antiperiodic.data(), nullptr));
    }
  };
};
// mdt / mdv / force-gradient shifts on device-resident links and momenta (staghmc_sh.nim:429-640; qexhip_md_*)
class ResidentMD {
  Context &c_;
 public:
  enum Source { Gauge = 0, Nhyp = 1 };                      // which device force buffer a kick / shift applies
  ResidentMD(Context &c, const Field &g, const Field &p) : c_(c) { check(qexhip_md_begin(c.h, g.data(), p.data())); }
  void end(Field *g, Field *p) { check(qexhip_md_end(c_.h, g ? g->data() : nullptr, p ? p->data() : nullptr)); }
  double momentumNorm2() { double r = 0; check(qexhip_md_momentum_norm2(c_.h, &r)); return r; }
  void updateLinks(double t) { check(qexhip_md_update_links(c_.h, t)); }                       // mdt
  void gaugeForce(double plaq, double rect = 0, double adjplaq = 0) { check(qexhip_md_gauge_force(c_.h, plaq, rect, adjplaq)); }
  void kick(Source s, double t) { check(qexhip_md_kick(c_.h, (int)s, t)); }                     // mdv: p += t f
  void shiftLinks(Source s, double t) { check(qexhip_md_shift_links(c_.h, (int)s, t)); }        // fgv / fgvf
  void saveLinks() { check(qexhip_md_save_links(c_.h)); }
  void restoreLinks() { check(qexhip_md_restore_links(c_.h)); }
  // HISQ molecular dynamics (hisqhmc.nim:405-414,496-545) on the resident fields: qexhip_md_hisq_*
  void hisqPrepare(bool setLinks = true, const std::array<int, 4> &antiperiodic = {0, 0, 0, 1}) {
    check(qexhip_md_hisq_prepare(c_.h, antiperiodic.data(), nullptr, setLinks ? 1 : 0));
  }
  void hisqFforce(const std::vector<int> &psiIds, const std::vector<double> &scale, double t) {
    check(qexhip_md_hisq_fforce(c_.h, (int)psiIds.size(), psiIds.data(), scale.data(), t));
  }
  std::vector<int> hisqFforceSolve(const std::vector<int> &phiIds, const std::vector<double> &mass, const std::vector<double> &scale,
                                   const std::vector<double> &r2req, int maxits, double t) {
    std::vector<int> its(phiIds.size(), 0);
    check(qexhip_md_hisq_fforce_solve(c_.h, (int)phiIds.size(), phiIds.data(), mass.data(), scale.data(), r2req.data(), maxits, t, its.data()));
    return its;
  }
  // the rooted force: r(x) = f0 + sum_k alpha_k / (x + beta_k) of M^+M, every pole's vector from one multi-shift solve
  int hisqFforceRational(int phiId, double mass, const std::vector<double> &alpha, const std::vector<double> &beta, double r2req,
                         int maxits, double t, int sloppy = 0) {
    int its = 0;
    check(qexhip_md_hisq_fforce_rational(c_.h, phiId, mass, (int)alpha.size(), alpha.data(), beta.data(), r2req, maxits, sloppy, t, &its));
    return its;
  }
  void hisqForce(Field &f) { check(qexhip_md_hisq_force_get(c_.h, f.data())); }
};
// HisqCoefs.smear(g, fl, ll) (hisqLinks.nim:32-43)
inline void hisqSmear(Context &c, const Field &g, Field &fl, Field &ll) { check(qexhip_hisq_smear(c.h, g.data(), fl.data(), ll.data())); }
// loadGauge / saveGauge (gaugeUtils.nim:87-122)
inline void saveGauge(const Layout &lo, const Field &g, const std::string &fn, char prec = 'D') {
  check(qexhip_io_write_gauge(fn.c_str(), lo.physGeom.data(), g.data(), prec, nullptr, nullptr));
}
inline void loadGauge(const Layout &lo, Field &g, const std::string &fn) {
  unsigned a = 0, b = 0;
  check(qexhip_io_read_gauge(fn.c_str(), lo.physGeom.data(), g.data(), &a, &b));
}

// field algebra used by the reference's tests (fieldET.nim:605-625)
inline double norm2(Context &c, const Field &x, int subset = QEXHIP_ALL) {
  double r = 0;
  check(qexhip_norm2(c.h, x.data(), subset, &r));
  return r;
}
inline double redot(Context &c, const Field &x, const Field &y, int subset = QEXHIP_ALL) {      // fieldET.nim:704-724
  double r = 0;
  check(qexhip_redot(c.h, x.data(), y.data(), subset, &r));
  return r;
}
inline std::complex<double> dot(Context &c, const Field &x, const Field &y, int subset = QEXHIP_ALL) {   // fieldET.nim:677-693
  double r[2] = {0, 0};
  check(qexhip_dot(c.h, x.data(), y.data(), subset, r));
  return {r[0], r[1]};
}

}  // namespace qex
