// full_solve.h -- the decisions of the even/odd full solve (Staggered.solve, stagSolve.nim:141-294 and :347-446), host only.
// One statement for solve_inner (solver.cpp), the lock-step batch (batch.hip: solve_full_batch_impl) and the multi-shift full solve
// (multishift.hip: solve_multi_dev).  `stop` is the absolute target |r|^2 <= stop of this pass; every caller computes it in its own
// way (r2req * (b2e + b2o) / (r2stop / r2) * r2 / r2stop), which can differ by a rounding, and hands it in.
#pragma once

// the target of each parity's solveXX: all of `stop` that the other parity does not use up already, else half of it (:144-147,162 and :213-217)
inline void eo_stops(double stop, double r2e, double r2o, double *stope, double *stopo) {
  const double stop2 = 0.5 * stop;
  *stope = (r2o <= stop2) ? stop - r2o : stop2;
  *stopo = (r2e <= stop2) ? stop - r2e : stop2;
}

enum { EO_RIGHT = 0, EO_LEFT = 1 };
// kind EO_RIGHT (solveReconR :141-176): solveXX on parity `par` (1 even, 0 odd, -1 nothing to solve) to the relative target rr, then
// x = D^+ (4 y).  kind EO_LEFT (solveReconL :179-208): solveXX on the even sites with source (D^+ b).even, then the odd sites
// reconstructed; its rr needs |(D^+ b).even|^2 and comes from eo_left_target.
struct EoPlan {
  int kind, par;
  double rr;
};
// right where one parity is below its target already, and at mass 0 where the reconstruction of the left form divides by m (:218)
inline EoPlan eo_plan(double stop, double r2e, double r2o, double m) {
  double stope, stopo;
  eo_stops(stop, r2e, r2o, &stope, &stopo);
  if (r2e <= stope || r2o <= stopo || m == 0.0) {
    if (r2e > stope) return {EO_RIGHT, 1, stope / r2e};
    if (r2o > stopo) return {EO_RIGHT, 0, stopo / r2o};
    return {EO_RIGHT, -1, 0.0};
  }
  return {EO_LEFT, 1, 0.0};
}

// 0.99 stop m^2 / |d_e|^2 with stop = rq * r2 (:196).  The factors come in separately because both callers have always multiplied
// from the left, (0.99 * rq) * r2, which is not 0.99 * (rq * r2) in the last bit.
inline double eo_left_target(double rq, double r2, double m, double d2e) { return 0.99 * rq * r2 * m * m / d2e; }
