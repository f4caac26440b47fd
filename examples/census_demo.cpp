// The dense sweep with the absolute-difference and with the census matching cost through include/vslam_filter_hip.hpp's
// DenseStereoHip: three cameras half a unit apart look at a textured two-level step (near for world
// x < 0.2, far beyond), and the two source views are re-exposed as a camera with automatic exposure and gain would have
// taken them: 1.25 I + 15 and 0.8 I - 10.  The absolute difference of grey values then finds no plane; the census
// descriptor keeps only the order of the grey values in a 9 x 7 window, which a change of exposure leaves alone.  The same
// views are swept both ways and filtered, and the interior pixels within one plane step of the truth are counted.
// Prints "ok" on success.
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

// the step seen from a camera at (cx, 0, 0) with no rotation, re-exposed as gain I + bias; depth: its true depth per pixel
static std::vector<unsigned char> render(double cx, double z_near, double z_far, double gain, double bias, std::vector<double>* depth) {
  std::vector<unsigned char> g((size_t)W * H);
  if (depth) depth->resize(g.size());
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const double rx = (x - K[2]) / K[0], ry = (y - K[3]) / K[1];
      const double Z = cx + z_near * rx < STEP_EDGE ? z_near : z_far;
      g[(size_t)y * W + x] = to_byte(gain * (double)to_byte(texture(cx + Z * rx, Z * ry)) + bias);
      if (depth) (*depth)[(size_t)y * W + x] = Z;
    }
  return g;
}

// interior pixels of the filtered map of view 0 with a depth, and those within one plane step of the truth (swept map)
static void count(DenseStereoHip& ds, const std::vector<double>& truth, int* kept, int* right, int* inside) {
  ds.filter(0, {1, 2}, 0.05, 1);
  const DenseStereoHip::Depth swept = ds.depth(0, false), filtered = ds.depth(0, true);
  const double step = (W_MAX - W_MIN) / (D - 1);
  const int m = 18;                                                  // the window and census radii plus the largest disparity, 12.8 px
  *kept = *right = *inside = 0;
  for (int y = m; y < H - m; ++y)
    for (int x = m; x < W - m; ++x) {
      const size_t i = (size_t)y * W + x;
      ++*inside;
      if (filtered.depth[i] > 0.f) ++*kept;
      if (swept.depth[i] > 0.f && std::fabs(1.0 / (double)swept.depth[i] - 1.0 / truth[i]) <= step) ++*right;
    }
}

int main() {
  const double step = (W_MAX - W_MIN) / (D - 1), z_near = 1.0 / (W_MIN + NEAR_PLANE * step), z_far = 1.0 / (W_MIN + FAR_PLANE * step);
  const double cams[3] = {0.0, 0.5, -0.5}, gain[3] = {1.0, 1.25, 0.8}, bias[3] = {0.0, 15.0, -10.0};
  std::vector<double> truth;
  DenseStereoHip ds(W, H, 3);
  for (int s = 0; s < 3; ++s) {
    const double pose[7] = {cams[s], 0, 0, 1, 0, 0, 0};
    ds.setView(s, render(cams[s], z_near, z_far, gain[s], bias[s], s == 0 ? &truth : nullptr).data(), K, pose);
  }
  int kept[2], right[2], inside = 0;
  for (int s = 0; s < 3; ++s) ds.sweep(s, {(s + 1) % 3, (s + 2) % 3}, W_MIN, W_MAX, D, 1, 20);
  count(ds, truth, &kept[0], &right[0], &inside);
  ds.profile(true);
  for (int s = 0; s < 3; ++s) ds.sweepCensus(s, {(s + 1) % 3, (s + 2) % 3}, W_MIN, W_MAX, D, 1, 255);
  count(ds, truth, &kept[1], &right[1], &inside);
  double ms[3];
  long long n[3];
  ds.getCensusProfile(ms, n);
  std::printf("interior %d pixels within a plane step of the truth: absolute differences %d (%d kept by the filter), census %d (%d kept)\n",
              inside, right[0], kept[0], right[1], kept[1]);
  std::printf("k_census %.3f ms x %lld, k_plane_sweep_census %.3f ms x %lld\n", ms[0], n[0], ms[1], n[1]);
  const std::vector<unsigned long long> T = ds.census(0);
  unsigned long long high = 0;
  for (unsigned long long t : T) high |= t >> 62;
  if (T.size() != (size_t)W * H || high != 0) return 2;
  // three descriptors for three sweeps: each view's is computed once
  if (!(10 * right[1] >= 9 * inside && 10 * right[0] < inside && n[0] == 3 && n[1] == 3 && n[2] == 0)) return 1;
  std::printf("ok\n");
  return 0;
}
