// The decisions of the even/odd full solve (qex_amd/csrc/full_solve.h) against the rule of stagSolve.nim:141-218, spelled out per case:
//   stop2 = 0.5 stop;  stope = r2o <= stop2 ? stop - r2o : stop2;  stopo = r2e <= stop2 ? stop - r2e : stop2
//   right when r2e <= stope || r2o <= stopo || m == 0, else left
//   right: r2e > stope -> (even, stope / r2e); else r2o > stopo -> (odd, stopo / r2o); else nothing to solve
//   left:  even, target 0.99 * rq * r2 * m * m / d2e (multiplied from the left; stop = rq * r2)
// Every comparison is == on doubles: the three callers must keep the bits they computed before they shared this header.
#include "full_solve.h"
#include <cstdio>

static int fails = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); fails++; } } while (0)

static void expect_plan(int line, const EoPlan &p, int kind, int par, double rr) {
  if (p.kind != kind || p.par != par || !(p.rr == rr)) {
    printf("FAILED line %d: plan {%d, %d, %.17g}, expected {%d, %d, %.17g}\n", line, p.kind, p.par, p.rr, kind, par, rr);
    fails++;
  }
}
#define EXPECT_PLAN(p, kind, par, rr) expect_plan(__LINE__, p, kind, par, rr)

int main() {
  const double stop = 3e-7;
  double se, so;

  // even-only source: the even solve gets the whole target
  eo_stops(stop, 2.0, 0.0, &se, &so);
  EXPECT(se == stop && so == 0.5 * stop);
  EXPECT_PLAN(eo_plan(stop, 2.0, 0.0, 0.1), EO_RIGHT, 1, stop / 2.0);
  // odd-only source
  eo_stops(stop, 0.0, 3.0, &se, &so);
  EXPECT(se == 0.5 * stop && so == stop);
  EXPECT_PLAN(eo_plan(stop, 0.0, 3.0, 0.1), EO_RIGHT, 0, stop / 3.0);
  // equal parities: left; rr is eo_left_target's to fill
  eo_stops(stop, 1.0, 1.0, &se, &so);
  EXPECT(se == 0.5 * stop && so == 0.5 * stop);
  EXPECT_PLAN(eo_plan(stop, 1.0, 1.0, 0.1), EO_LEFT, 1, 0.0);
  // the same at mass 0: the left form would divide by m, so right on the even sites with half the target
  EXPECT_PLAN(eo_plan(stop, 1.0, 1.0, 0.0), EO_RIGHT, 1, 0.5 * stop / 1.0);
  // the even part below its target, the odd part above: the odd solve gets what the even part leaves
  eo_stops(1.0, 0.1, 5.0, &se, &so);
  EXPECT(se == 0.5 && so == 1.0 - 0.1);
  EXPECT_PLAN(eo_plan(1.0, 0.1, 5.0, 0.1), EO_RIGHT, 0, (1.0 - 0.1) / 5.0);
  // r2e + r2o <= stop: nothing to solve
  EXPECT_PLAN(eo_plan(1.0, 0.3, 0.2, 0.1), EO_RIGHT, -1, 0.0);
  // r2o exactly 0.5 stop: `<=` makes it right (stopo = 0.5 stop = r2o); `<` would send it left
  eo_stops(4.0, 10.0, 2.0, &se, &so);
  EXPECT(se == 4.0 - 2.0 && so == 2.0);
  EXPECT_PLAN(eo_plan(4.0, 10.0, 2.0, 0.1), EO_RIGHT, 1, (4.0 - 2.0) / 10.0);
  // ... and just above it: left
  EXPECT_PLAN(eo_plan(4.0, 10.0, 2.0000000000000004, 0.1), EO_LEFT, 1, 0.0);

  // the left target, multiplied from the left.  The second set is one where (0.99 * rq) * r2 and 0.99 * (rq * r2) differ in the last
  // bit and the difference survives to the result: the order is part of the contract.
  EXPECT(eo_left_target(1e-12, 2.0, 0.1, 3.0) == 0.99 * 1e-12 * 2.0 * 0.1 * 0.1 / 3.0);
  const double rq = 3e-13, r2 = 3805.0512621179655, m = 0.05, d2e = 7.25;
  EXPECT(eo_left_target(rq, r2, m, d2e) == ((((0.99 * rq) * r2) * m) * m) / d2e);
  EXPECT(eo_left_target(rq, r2, m, d2e) == 3.896897327065641e-13);
  EXPECT(eo_left_target(rq, r2, m, d2e) != 0.99 * (rq * r2) * m * m / d2e);

  if (fails) { printf("full solve plan: %d check(s) FAILED\n", fails); return 1; }
  printf("full solve plan: Passed\n");
  return 0;
}
