// test_stag_prop.cpp -- C++ host-side parity test through include/qexhip.hpp.
//
// Mirrors the reference's own programs:
//   tests/examples/testStagProp.nim:16-60   point source, s.D, s.solve(v2, v1, m, 1e-8), true residual
//   tests/reprod/trandgauge.nim:4-27        plaquettes of g.random            (golden set G1)
//   src/gauge/wflow.nim:92-149              plaquettes after gaugeFlow(6,.01) (golden set G2)
// with the CPU oracle (oracle/qex_oracle.h, test infrastructure) as the checker.
// Build + run: tests/test_cpp_host.py (g++ -Iinclude -Ioracle ... -lqexhip -lqexoracle).
// argv[1]: directory for the SciDAC round-trip file (default /tmp).
#include "qexhip.hpp"
extern "C" {
#include "qex_oracle.h"
}
#include <cmath>
#include <cstdio>
#include <cstdlib>

static int fails = 0;
#define CHECK(cond, ...)                                                   \
  do {                                                                     \
    if (!(cond)) { fails++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
  } while (0)

static double relerr(const qex::Field &a, const qex::Field &b) {
  double n = 0, d = 0;
  for (size_t i = 0; i < a.size(); i++) { d += (a[i] - b[i]) * (a[i] - b[i]); n += b[i] * b[i]; }
  return std::sqrt(d / n);
}

int main(int argc, char **argv) {
  using namespace qex;
  const std::array<int, 4> lat = {8, 8, 8, 8};
  Context ctx(lat);
  printf("%s\n", ctx.info().c_str());
  const Layout &lo = ctx.lo;

  // oracle side: same layout, RngMilc6 configuration (default seed 17^7, as trandgauge.nim)
  qo_layout *olo = qo_layout_new(lat.data());
  qo_rngfield *rf = qo_rngfield_new(olo, QO_RNG_MILC6, 410338673ull);
  Field g = lo.newGauge();
  qo_gauge_random(olo, rf, g.data());

  // --- trandgauge.nim: plaquettes of the random field (G1) through the HIP plaquette kernel
  const double P[6] = {0.0006005738094166639, 0.0007744149733359666, 0.000491692592364555,
                       -0.0002244585371871249, -0.000700363878755635, -4.121898341926528e-05};
  auto pl = plaq(ctx, g);
  double d2 = 0;
  for (int i = 0; i < 6; i++) d2 += (pl[i] - P[i]) * (pl[i] - P[i]);
  printf("diff2: %g\n", d2);
  CHECK(d2 <= 1e-30, "random-gauge plaquettes differ from the reference's golden values");

  // --- wflow.nim self-test: gaugeFlow(6, 0.01) then plaquettes (G2)
  {
    Field gf = g;
    gaugeFlow(ctx, gf, 6, 0.01, [&](double t) { (void)t; });
    const double p0[6] = {0.01960725848281519, 0.01982378149813489, 0.01938877647467847,
                          0.0185899778070918, 0.0180821938831715, 0.01876842496122964};
    auto p = plaq(ctx, gf);
    double d = 0, s = 0;
    for (int i = 0; i < 6; i++) { d += std::fabs(p[i] - p0[i]); s += p0[i]; }
    printf("wflow relative diff: %g\n", d / s);
    CHECK(d / s <= 2e-14, "flowed plaquettes differ from the reference's golden values");
  }

  // --- testStagProp.nim: g.setBC; g.stagPhase; point source; D; solve; true residual
  rephase(lo, g);
  {
    Field go = g;  // the oracle's own rephase must agree with the C++ host one
    qo_gauge_random(olo, qo_rngfield_new(olo, QO_RNG_MILC6, 410338673ull), go.data());
    qo_setBC(olo, go.data());
    const int ph[4] = {8, 9, 11, 0};
    qo_stagPhase(olo, go.data(), ph);
    CHECK(go == g, "host-side rephase differs from the oracle's");
  }
  Field v1 = lo.ColorVector(), v2 = lo.ColorVector(), r = lo.ColorVector(), ref = lo.ColorVector();
  v1[0] = 1.0;  // v1{0}[0] := 1
  auto s = newStag(ctx, g);
  const double m = 0.1;
  s.D(v2, v1, m);
  qo_D(olo, g.data(), nullptr, ref.data(), v1.data(), m);
  printf("D: rel err vs oracle %g, norm2 %g\n", relerr(v2, ref), norm2(ctx, v2));
  CHECK(relerr(v2, ref) < 1e-13, "D");

  SolverParams sp;
  sp.r2req = 1e-16;  // res = 1e-8
  sp.maxits = 100000;
  s.solve(v2, v1, m, sp);
  printf("solve: its %d  secs %g  Gf/s %g  r2 %g\n", sp.iterations, sp.seconds, 1e-9 * sp.flops / sp.seconds, sp.r2);
  s.D(r, v2, m);
  double r2 = 0;
  for (size_t i = 0; i < r.size(); i++) r2 += (r[i] - v1[i]) * (r[i] - v1[i]);
  printf("true residual^2: %g\n", r2);
  CHECK(r2 <= 1e-16, "true residual after solve");
  double fin = 0;
  int oits = qo_solve(olo, g.data(), nullptr, ref.data(), v1.data(), m, 1e-16, 100000, &fin);
  printf("oracle: its %d  rel diff of solutions %g\n", oits, relerr(v2, ref));
  CHECK(std::abs(oits - sp.iterations) <= 2, "iteration count vs oracle");
  CHECK(relerr(v2, ref) < 1e-6, "solution vs oracle");

  // --- solveEE with the residual history (the `CG iteration:` lines of cg.nim:215-217)
  {
    Field b = lo.ColorVector(), x = lo.ColorVector(), xo = lo.ColorVector();
    qo_vector_gaussian(olo, rf, b.data());
    SolverParams spe;
    spe.r2req = 1e-12;
    spe.maxits = 2000;
    s.solveEE(x, b, m, spe, 512);
    std::vector<double> hist(512);
    double f2 = 0;
    int its = qo_solveXX(olo, g.data(), nullptr, xo.data(), b.data(), m, 1e-12, 2000, 1, hist.data(), 512, &f2);
    // CG amplifies rounding differences between equivalent summation orders: on this system the
    // CPU path deviates from ITSELF by 2e-2 at iteration 187 when only its thread count changes
    // (1 vs 8), while the first 100 iterations agree to 1e-15 (see tests/test_gpu_parity.py,
    // history_tolerance).  Hence: early history tight, tail loose, iteration count exact +-1.
    double dev100 = 0, dev = 0;
    for (int k = 0; k < (int)spe.r2hist.size() && k <= its; k++) {
      double d = std::fabs(spe.r2hist[k] / hist[k] - 1);
      dev = std::fmax(dev, d);
      if (k < 100) dev100 = std::fmax(dev100, d);
    }
    printf("solveEE: its %d (oracle %d), history deviation: first 100 its %g, whole %g\n", spe.iterations, its, dev100, dev);
    CHECK(std::abs(its - spe.iterations) <= 1 && dev100 < 1e-10 && dev < 0.1, "CG residual history vs CPU path");
  }

  // --- the HMC-side pieces: nHYP closure (hypsmear.nim:49-247), links from smeared fields, batched solves, file I/O
  {
    Field gw = lo.newGauge(), sg = lo.newGauge(), sgo = lo.newGauge(), f = lo.newGauge(), fo = lo.newGauge(), chain = lo.newGauge();
    qo_rngfield *rf2 = qo_rngfield_new(olo, QO_RNG_MILC6, 77ull);
    qo_gauge_warm(olo, rf2, 0.5, gw.data());
    qo_gauge_random_tah(olo, rf2, chain.data());
    HypCoefs hc;                                          // 0.4, 0.5, 0.5
    {
      HypCoefs::SmearedForce sf(ctx, hc, gw, &sg);
      sf(f, chain);
    }
    qo_nhyp_force(olo, gw.data(), sgo.data(), fo.data(), chain.data(), 0.4, 0.5, 0.5);
    printf("nHYP: smeared links rel err %g, force chain rel err %g\n", relerr(sg, sgo), relerr(f, fo));
    CHECK(relerr(sg, sgo) < 1e-12 && relerr(f, fo) < 1e-11, "nHYP smearing / force chain vs oracle");
    // operator on device-smeared links; thin warm links are stored compressed, the U(3) ones with their determinant
    Staggered sn(ctx, gw, Staggered::FromNhyp{0.4, 0.5, 0.5});
    CHECK(sn.linkFormat() == 2, "nHYP links use the 2 rows + determinant format");
    qo_setBC(olo, sgo.data());
    const int ph2[4] = {8, 9, 11, 0};
    qo_stagPhase(olo, sgo.data(), ph2);
    Field b1 = lo.ColorVector(), b2 = lo.ColorVector(), y = lo.ColorVector(), yo = lo.ColorVector();
    qo_vector_gaussian(olo, rf2, b1.data());
    qo_vector_gaussian(olo, rf2, b2.data());
    sn.D(y, b1, 0.05);
    qo_D(olo, sgo.data(), nullptr, yo.data(), b1.data(), 0.05);
    CHECK(relerr(y, yo) < 1e-12, "D on device-smeared links");
    // two systems in lock-step == the same two solved one after the other
    std::vector<Field> xs(2, lo.ColorVector()), bs{b1, b2};
    std::vector<SolverParams> sps(2);
    for (auto &p : sps) { p.r2req = 1e-20; p.maxits = 100000; }
    sn.solveBatch(xs, bs, {0.1, 0.2}, sps);
    for (int j = 0; j < 2; j++) {
      SolverParams s1; s1.r2req = 1e-20; s1.maxits = 100000;
      Field x1 = lo.ColorVector();
      sn.solve(x1, bs[j], j ? 0.2 : 0.1, s1);
      CHECK(s1.iterations == sps[j].iterations && relerr(xs[j], x1) < 1e-13, "batched solve equals the single solve");
    }
    // MD loop on resident fields (qexhip_md_*): smeared gauge force through the closure, kick, link update -- against
    // the oracle's force chain and exp update
    {
      Field pm = lo.newGauge(), g2 = lo.newGauge(), p2 = lo.newGauge(), fg = lo.newGauge(), go = gw, po = lo.newGauge();
      qo_gauge_random_tah(olo, rf2, pm.data());
      ResidentMD md(ctx, gw, pm);
      const double p2dev = md.momentumNorm2();
      double p2host = 0;
      for (double v : pm) p2host += v * v;
      CHECK(std::abs(p2dev - p2host) <= 1e-10 * p2host, "momentum norm on the device");   // the host loop above sums naively
      {
        HypCoefs::SmearedForce sfr(ctx, hc);             // smears the resident links
        sfr.gforceResident(1.3);                         // Wilson action of the smeared links, force left on the device
        md.kick(ResidentMD::Nhyp, -0.2);
      }
      md.updateLinks(0.05);
      md.end(&g2, &p2);
      // oracle: chain = dS/dV of the Wilson action on the smeared links, smearedForce, TAH(g f^+), p -= 0.2 f, g = exp(0.05 p) g
      Field ch2 = lo.newGauge(), sg2 = lo.newGauge();
      qo_nhyp_smear(olo, gw.data(), sg2.data(), 0.4, 0.5, 0.5);
      qo_gauge_deriv_rect(olo, sg2.data(), ch2.data(), 1.3, 0.0);
      qo_nhyp_force(olo, gw.data(), sg2.data(), fg.data(), ch2.data(), 0.4, 0.5, 0.5);
      qo_force_projTAH(olo, fg.data(), gw.data(), 1);
      po = pm;
      for (size_t i = 0; i < po.size(); i++) po[i] -= 0.2 * fg[i];
      qo_gauge_exp_update(olo, go.data(), po.data(), 0.05);
      printf("resident MD: momenta rel err %g, links rel err %g\n", relerr(p2, po), relerr(g2, go));
      CHECK(relerr(p2, po) < 1e-11 && relerr(g2, go) < 1e-12, "resident MD step vs oracle");
    }
    // SciDAC file round trip
    const std::string fn = std::string(argc > 1 ? argv[1] : "/tmp") + "/qexhip_cpp_test.lime";
    saveGauge(lo, gw, fn);
    Field gr = lo.newGauge();
    loadGauge(lo, gr, fn);
    CHECK(gr == gw, "saveGauge / loadGauge round trip");
    std::remove(fn.c_str());
    qo_rngfield_free(rf2);
  }

  // --- error behaviour: bad arguments raise, non-convergence does not
  {
    SolverParams sp2;
    sp2.r2req = 1e-30;
    sp2.maxits = 5;
    s.solveEE(v2, v1, m, sp2);
    CHECK(sp2.iterations == 5, "maxits reached is not an error");
    bool threw = false;
    try { std::array<int, 4> bad = {8, 8, 7, 8}; Context c2(bad); } catch (const Error &) { threw = true; }
    CHECK(threw, "odd lattice extent must raise");
  }

  qo_layout_free(olo);
  printf(fails ? "FAILED (%d)\n" : "Passed\n", fails);
  return fails ? 1 : 0;
}
