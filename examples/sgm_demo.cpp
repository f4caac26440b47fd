// The dense sweep with and without semi-global cost aggregation through include/vslam_filter_hip.hpp's DenseStereoHip
// (DESIGN.md section 19): three cameras half a unit apart look at a fronto-parallel wall on plane 5 of 12 whose middle is
// painted flat grey.  There every plane costs the same and the pixel-wise winner is plane 0 in every view, which the
// geometric filter deletes or, where the views agree on it, lets through; the aggregated sweep carries the wall's plane
// across the patch.  The same views are swept both ways and the pixels that received a depth are counted.  Prints "ok" on
// success.
#include <cmath>
#include <cstdio>
#include <vector>

#include "vslam_filter_hip.hpp"

static const int W = 96, H = 64, D = 12, TRUE_PLANE = 5;
static const double K[4] = {64.0, 64.0, 48.0, 32.0};
static const double W_MIN = 0.15, W_MAX = 0.40;

static double texture(double X, double Y) {
  if (X > -1.5 && X < 1.5 && Y > -1.0 && Y < 1.0) return 128.0;      // the patch without texture
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

// interior pixels of the filtered map of view 0 with a depth, and those of them on the wall's plane
static void count(DenseStereoHip& ds, int* kept, int* right, int* inside) {
  ds.filter(0, {1, 2}, 0.02, 2);
  const DenseStereoHip::Depth d = ds.depth(0, true);
  const int m = 14;                                                  // the window radius plus the largest disparity, 12.8 px
  *kept = *right = *inside = 0;
  for (int y = m; y < H - m; ++y)
    for (int x = m; x < W - m; ++x) {
      const size_t i = (size_t)y * W + x;
      ++*inside;
      if (d.depth[i] > 0.f) ++*kept;
      if (d.plane[i] == TRUE_PLANE) ++*right;
    }
}

int main() {
  const double step = (W_MAX - W_MIN) / (D - 1), Z = 1.0 / (W_MIN + TRUE_PLANE * step);
  const double cams[3] = {0.0, 0.5, -0.5};
  DenseStereoHip ds(W, H, 3);
  for (int s = 0; s < 3; ++s) {
    const double pose[7] = {cams[s], 0, 0, 1, 0, 0, 0};
    ds.setView(s, render(cams[s], Z).data(), K, pose);
  }
  int kept[2], right[2], inside = 0;
  for (int s = 0; s < 3; ++s) ds.sweep(s, {(s + 1) % 3, (s + 2) % 3}, W_MIN, W_MAX, D, 1, 20);
  count(ds, &kept[0], &right[0], &inside);
  ds.profile(true);
  for (int s = 0; s < 3; ++s) ds.sweepSgm(s, {(s + 1) % 3, (s + 2) % 3}, W_MIN, W_MAX, D, 1, 20);
  count(ds, &kept[1], &right[1], &inside);
  double ms[10];
  long long n[10];
  ds.getSgmProfile(ms, n);
  double paths_ms = 0.0;
  for (int i = 1; i <= 8; ++i) paths_ms += ms[i];
  std::printf("interior %d pixels: winner-take-all gave %d a depth (%d on plane %d), aggregated %d (%d on plane %d)\n", inside, kept[0],
              right[0], TRUE_PLANE, kept[1], right[1], TRUE_PLANE);
  std::printf("volume sweep %.3f ms x %lld, 8 directions %.3f ms, winner %.3f ms x %lld\n", ms[0], n[0], paths_ms, ms[9], n[9]);
  const std::vector<unsigned int> S = ds.volume(2);                 // the last swept slot owns the volumes
  bool refused = false;
  try {
    ds.volume(0);
  } catch (const std::runtime_error&) {
    refused = true;
  }
  if (!refused || S.size() != (size_t)D * W * H) return 2;
  if (!(right[1] == kept[1] && right[1] > 2 * right[0] && 10 * right[1] >= 9 * inside && n[0] == 3 && n[1] == 3 && n[8] == 3 && n[9] == 3)) return 1;
  std::printf("ok\n");
  return 0;
}
