// The dense sweep with the sum over all sources and with best-K source selection through include/vslam_filter_hip.hpp's
// DenseStereoHip: three cameras half a unit apart look at a textured two-level step (near for world
// x < 0.2, far beyond).  Near the left and right border of the reference image one of the two sources does not see the
// surface; its warp is invalid there and costs the truncation, 255, so the sum over both sources prefers the planes on
// which both warps are valid over the plane on which the other source matches.  Keeping the cheaper of the two sources per
// pixel and plane (n_best = 1) leaves the blind source out.  The same views are swept both ways, also with semi-global
// aggregation, and the pixels of the WHOLE image within one plane step of the truth are counted.  Prints "ok" on success.
#include <cmath>
#include <cstdio>
#include <vector>

#include "vslam_filter_hip.hpp"

static const int W = 96, H = 64, D = 12, NEAR_PLANE = 8, FAR_PLANE = 3;
static const double K[4] = {64.0, 64.0, 48.0, 32.0};
static const double W_MIN = 0.15, W_MAX = 0.40, STEP_EDGE = 0.2;

static double texture(double X, double Y) {
  return 127.5 + 23.0 * (std::sin(7.3 * X + 1.1 * Y) + std::sin(2.9 * X - 6.1 * Y + 0.7) + std::sin(11.7 * X + 4.3 * Y + 2.1) +
                         std::sin(-4.7 * X + 9.9 * Y + 0.3) + 0.7 * std::sin(17.1 * X - 2.3 * Y) + 0.7 * std::sin(1.3 * X + 15.7 * Y + 1.9));
}

static unsigned char to_byte(double v) {
  v = std::floor(v + 0.5);
  return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// the step seen from a camera at (cx, 0, 0) with no rotation; depth: its true depth per pixel
static std::vector<unsigned char> render(double cx, double z_near, double z_far, std::vector<double>* depth) {
  std::vector<unsigned char> g((size_t)W * H);
  if (depth) depth->resize(g.size());
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const double rx = (x - K[2]) / K[0], ry = (y - K[3]) / K[1];
      const double Z = cx + z_near * rx < STEP_EDGE ? z_near : z_far;
      g[(size_t)y * W + x] = to_byte(texture(cx + Z * rx, Z * ry));
      if (depth) (*depth)[(size_t)y * W + x] = Z;
    }
  return g;
}

// pixels of the swept map of view 0 within one plane step of the truth, over the whole image
static int count(DenseStereoHip& ds, const std::vector<double>& truth) {
  const DenseStereoHip::Depth swept = ds.depth(0, false);
  const double step = (W_MAX - W_MIN) / (D - 1);
  int right = 0;
  for (size_t i = 0; i < truth.size(); ++i)
    if (swept.depth[i] > 0.f && std::fabs(1.0 / (double)swept.depth[i] - 1.0 / truth[i]) <= step) ++right;
  return right;
}

int main() {
  const double step = (W_MAX - W_MIN) / (D - 1), z_near = 1.0 / (W_MIN + NEAR_PLANE * step), z_far = 1.0 / (W_MIN + FAR_PLANE * step);
  const double cams[3] = {0.0, 0.5, -0.5};
  std::vector<double> truth;
  DenseStereoHip ds(W, H, 3);
  for (int s = 0; s < 3; ++s) {
    const double pose[7] = {cams[s], 0, 0, 1, 0, 0, 0};
    ds.setView(s, render(cams[s], z_near, z_far, s == 0 ? &truth : nullptr).data(), K, pose);
  }
  const int all = W * H;
  ds.sweep(0, {1, 2}, W_MIN, W_MAX, D, 1, 255);
  const int sum_all = count(ds, truth);
  const std::vector<unsigned> cost_all = ds.depth(0, false).cost;
  ds.profile(true);
  ds.sweepBest(0, {1, 2}, 2, W_MIN, W_MAX, D, 1, 255);               // n_best = n_src: the sum again, through the new kernel
  const bool identical = ds.depth(0, false).cost == cost_all && count(ds, truth) == sum_all;
  ds.sweepBest(0, {1, 2}, 1, W_MIN, W_MAX, D, 1, 255);
  const int best_one = count(ds, truth);
  ds.sweepBest(0, {1, 2}, 1, W_MIN, W_MAX, D, 1, 255, false, 8);      // ... and with 8 aggregation paths, default penalties
  const int best_one_sgm = count(ds, truth);
  const bool has_volume = ds.volume(0, true).size() == (size_t)D * W * H;
  ds.sweepBest(0, {1, 2}, 1, W_MIN, W_MAX, D, 2, 62, true);           // ... and with the census cost
  const int best_one_census = count(ds, truth);
  double ms[4];
  long long n[4];
  ds.getBestProfile(ms, n);
  std::printf("of %d pixels within a plane step of the truth: sum of both sources %d (%.1f %%), best 1 of 2 %d (%.1f %%), "
              "aggregated %d, census %d\n", all, sum_all, 100.0 * sum_all / all, best_one, 100.0 * best_one / all, best_one_sgm,
              best_one_census);
  std::printf("k_plane_sweep_best %.3f ms x %lld, k_plane_sweep_best_census %.3f ms x %lld, k_sweep_volume_best %.3f ms x %lld\n",
              ms[0], n[0], ms[1], n[1], ms[2], n[2]);
  if (!identical || !has_volume) return 2;
  // the oracle's counts on this scene are 5275 (85.9 %) and 6095 (99.2 %)
  if (!(100 * best_one >= 95 * all && 100 * sum_all < 90 * all && 100 * best_one_sgm >= 95 * all && 100 * best_one_census >= 90 * all &&
        n[0] == 2 && n[1] == 1 && n[2] == 1 && n[3] == 0))
    return 1;
  std::printf("ok\n");
  return 0;
}
