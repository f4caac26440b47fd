// Dense plane sweep through include/vslam_filter_hip.hpp's DenseStereoHip: three cameras half a unit apart look at a
// textured fronto-parallel wall that lies exactly on plane 5 of 12; the middle view is swept against the other two, the
// three maps are filtered against each other and the wall's points come back.  Prints "ok" on success.
#include <cmath>
#include <cstdio>
#include <vector>

#include "vslam_filter_hip.hpp"

static const int W = 96, H = 64, D = 12, TRUE_PLANE = 5;
static const double K[4] = {64.0, 64.0, 48.0, 32.0};
static const double W_MIN = 0.15, W_MAX = 0.40;

static double texture(double X, double Y) {
  return 127.5 + 23.0 * (std::sin(7.3 * X + 1.1 * Y) + std::sin(2.9 * X - 6.1 * Y + 0.7) + std::sin(11.7 * X + 4.3 * Y + 2.1) +
                         std::sin(-4.7 * X + 9.9 * Y + 0.3) + 0.7 * std::sin(17.1 * X - 2.3 * Y) + 0.7 * std::sin(1.3 * X + 15.7 * Y + 1.9));
}

// the wall z = Z seen from a camera at (cx, 0, 0) with no rotation
static std::vector<unsigned char> render(double cx, double Z) {
  std::vector<unsigned char> g((size_t)W * H);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const double v = std::floor(texture(cx + Z * (x - K[2]) / K[0], Z * (y - K[3]) / K[1]) + 0.5);
      g[(size_t)y * W + x] = (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
    }
  return g;
}

int main() {
  const double step = (W_MAX - W_MIN) / (D - 1), Z = 1.0 / (W_MIN + TRUE_PLANE * step);
  const double cams[3] = {0.0, 0.5, -0.5};
  DenseStereoHip ds(W, H, 3);
  for (int s = 0; s < 3; ++s) {
    const double pose[7] = {cams[s], 0, 0, 1, 0, 0, 0};
    ds.setView(s, render(cams[s], Z).data(), K, pose);
  }
  ds.profile(true);
  for (int s = 0; s < 3; ++s) ds.sweep(s, {(s + 1) % 3, (s + 2) % 3}, W_MIN, W_MAX, D, 2, 255);
  ds.filter(0, {1, 2}, 0.02, 2);
  const DenseStereoHip::Depth d = ds.depth(0, true);
  const std::vector<double> xyz = ds.points(0, true);
  // interior: the window radius plus the largest disparity (64 * 0.5 * 0.40 = 12.8 px) away from the border
  const int m = 15;
  int inside = 0, right = 0, kept = 0;
  double worst = 0.0;
  for (int y = m; y < H - m; ++y)
    for (int x = m; x < W - m; ++x) {
      const size_t i = (size_t)y * W + x;
      ++inside;
      if (d.plane[i] == TRUE_PLANE) ++right;
      if (d.depth[i] > 0.f) {
        ++kept;
        worst = std::fmax(worst, std::fabs(xyz[3 * i + 2] - Z));
      }
    }
  double ms[2];
  long long n[2];
  ds.getProfile(ms, n);
  std::printf("interior %d: plane %d on %d, kept %d, worst |z - Z| = %.3g (Z = %.4f); sweep %.3f ms x %lld, filter %.3f ms x %lld\n",
              inside, TRUE_PLANE, right, kept, worst, Z, ms[0], n[0], ms[1], n[1]);
  bool refused = false;
  try {
    ds.sweep(0, {0, 1}, W_MIN, W_MAX, D, 2, 255);       // the reference among the sources
  } catch (const std::runtime_error&) {
    refused = true;
  }
  if (!refused) return 2;
  if (!(right == inside && kept == inside && worst < 0.05 * Z && n[0] == 3 && n[1] == 2)) return 1;
  std::printf("ok\n");
  return 0;
}
