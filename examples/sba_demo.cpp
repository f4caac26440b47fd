// Bundle adjustment through include/vslam_filter_hip.hpp's SysSbaHip: two cameras one unit apart look at a small
// cloud; the second camera and every point start perturbed, doSBA brings the RMS down.  Prints "ok" on success.
// With --pcg the handle uses the block-Jacobi PCG solver and doSBA is called with useCSparse = 3.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "vslam_filter_hip.hpp"

int main(int argc, char** argv) {
  const bool pcg = argc > 1 && std::strcmp(argv[1], "--pcg") == 0;
  if (argc > 1 && !pcg) {
    std::fprintf(stderr, "usage: %s [--pcg]\n", argv[0]);
    return 64;
  }
  const double fx = 500, fy = 500, cx = 320, cy = 240;
  SysSbaHip sba(fx, fy, cx, cy, 4, 64, 256, 0, pcg ? EKF_SBA_SOLVER_BPCG : EKF_SBA_SOLVER_CHOLESKY);
  const double cam[2][7] = {{0, 0, 0, 1, 0, 0, 0}, {1, 0, 0, 1, 0, 0, 0}};
  const double start1[7] = {1.02, -0.01, 0.015, 0.9999, 0.005, -0.004, 0.003};
  sba.addNode(cam[0]);
  sba.addNode(start1);
  for (int j = 0; j < 40; ++j) {
    const double X[3] = {-1.0 + 0.07 * j, 0.5 * std::sin(0.9 * j), 4.0 + 0.05 * (j % 7)};
    const double Xs[3] = {X[0] + 0.01 * std::cos(1.3 * j), X[1] - 0.01, X[2] + 0.02 * std::sin(0.7 * j)};
    const int p = sba.addPoint(Xs);
    for (int c = 0; c < 2; ++c) {
      const double xc = X[0] - cam[c][0], yc = X[1] - cam[c][1], zc = X[2] - cam[c][2];
      const double uv[2] = {fx * xc / zc + cx, fy * yc / zc + cy};
      if (!sba.addMonoProj(c, p, uv)) return 1;
    }
    const double again[2] = {0.0, 0.0};
    if (sba.addMonoProj(0, p, again)) return 2;       // a repeat of the pair keeps the first keypoint
  }
  const double rms0 = sba.calcRMSCost();
  const int it = pcg ? sba.doSBA(20, 1e-4, 3, 1e-8, 100) : sba.doSBA(20, 1e-4);
  if (pcg) {
    const std::vector<int> cg = sba.cgIterations();
    if ((int)cg.size() < it || cg.empty()) return 4;
    std::printf("pcg: %d CG iterations in the first solve\n", cg[0]);
    bool refused = false;
    try {
      sba.doSBA(1, 1e-4, 2);                            // SBA_GRADIENT
    } catch (const std::runtime_error&) {
      refused = true;
    }
    if (!refused) return 5;
  }
  const double rms1 = sba.calcRMSCost();
  std::printf("nodes %d points %d projections %d: rms %.4g -> %.4g in %d iterations\n", sba.numNodes(), sba.numPoints(),
              sba.numProjections(), rms0, rms1, it);
  if (!(it > 0 && rms1 < 0.1 * rms0 && sba.nodes()[0] == 0.0)) return 3;
  std::printf("ok\n");
  return 0;
}
