// The geometric filter with and without the uniqueness test through include/vslam_filter_hip.hpp's DenseStereoHip
// (DESIGN.md section 22): three cameras half a unit apart look at a textured plane that carries a patch without texture,
// grey 128 inside a world rectangle.  Inside the patch every plane of the sweep costs the same, the winner is arbitrary, and
// the two sources make the same arbitrary choice: the geometric filter finds the views in agreement and keeps depths of a
// surface that is not there.  The sweeps record the runner-up cost (keepRunnerUp), and filterUnique at 5 per cent drops
// the pixels whose runner-up is no dearer than the winner.  Prints the two counts of kept pixels, and "ok" on success.
#include <cmath>
#include <cstdio>
#include <vector>

#include "vslam_filter_hip.hpp"

static const int W = 96, H = 64, D = 12, TRUE_PLANE = 5;
static const double K[4] = {64.0, 64.0, 48.0, 32.0};
static const double W_MIN = 0.15, W_MAX = 0.40;
static const double RECT[4] = {-1.0, -0.2, -0.6, 0.6};              // x0 < X < x1, y0 < Y < y1 in the world: no texture

static double texture(double X, double Y) {
  return 127.5 + 23.0 * (std::sin(7.3 * X + 1.1 * Y) + std::sin(2.9 * X - 6.1 * Y + 0.7) + std::sin(11.7 * X + 4.3 * Y + 2.1) +
                         std::sin(-4.7 * X + 9.9 * Y + 0.3) + 0.7 * std::sin(17.1 * X - 2.3 * Y) + 0.7 * std::sin(1.3 * X + 15.7 * Y + 1.9));
}

static unsigned char to_byte(double v) {
  v = std::floor(v + 0.5);
  return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// the plane z = Z seen from a camera at (cx, 0, 0) with no rotation
static std::vector<unsigned char> render(double cx, double Z) {
  std::vector<unsigned char> g((size_t)W * H);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const double X = cx + Z * (x - K[2]) / K[0], Y = Z * (y - K[3]) / K[1];
      const bool flat = X > RECT[0] && X < RECT[1] && Y > RECT[2] && Y < RECT[3];
      g[(size_t)y * W + x] = to_byte(flat ? 128.0 : texture(X, Y));
    }
  return g;
}

struct Count { int kept, wrong; };

// pixels of the filtered map of view 0 with a depth, and those of them more than one plane step from the truth
static Count count(const DenseStereoHip::Depth& f, double Z) {
  const double step = (W_MAX - W_MIN) / (D - 1);
  Count c = {0, 0};
  for (size_t i = 0; i < f.depth.size(); ++i)
    if (f.depth[i] > 0.f) {
      ++c.kept;
      if (std::fabs(1.0 / (double)f.depth[i] - 1.0 / Z) > step) ++c.wrong;
    }
  return c;
}

int main() {
  const double Z = 1.0 / (W_MIN + TRUE_PLANE * (W_MAX - W_MIN) / (D - 1));
  const double cams[3] = {0.0, 0.5, -0.5};
  DenseStereoHip ds(W, H, 3);
  for (int s = 0; s < 3; ++s) {
    const double pose[7] = {cams[s], 0, 0, 1, 0, 0, 0};
    ds.setView(s, render(cams[s], Z).data(), K, pose);
  }
  ds.profile(true);
  ds.keepRunnerUp(true);
  for (int s = 0; s < 3; ++s) ds.sweep(s, {(s + 1) % 3, (s + 2) % 3}, W_MIN, W_MAX, D, 1, 20);
  const std::vector<unsigned int> runner = ds.runnerUp(0), cost = ds.depth(0, false).cost;
  int flat = 0;
  for (size_t i = 0; i < runner.size(); ++i) flat += runner[i] == cost[i];
  ds.filter(0, {1, 2});
  const DenseStereoHip::Depth plain = ds.depth(0, true);
  ds.filterUnique(0, {1, 2}, 0);                                   // 0 per cent: the geometric filter itself
  const DenseStereoHip::Depth zero = ds.depth(0, true);
  const bool identical = zero.depth == plain.depth && zero.plane == plain.plane;
  ds.filterUnique(0, {1, 2}, 5);
  const Count a = count(plain, Z), b = count(ds.depth(0, true), Z);
  double ms[6], ms2[2];
  long long n[6], n2[2];
  ds.getUniqueProfile(ms, n);
  ds.getProfile(ms2, n2);
  std::printf("of %d pixels, %d with a flat cost curve: kept by the geometric filter %d (%d of them wrong), with uniqueness 5 %d (%d wrong)\n",
              W * H, flat, a.kept, a.wrong, b.kept, b.wrong);
  std::printf("k_plane_sweep_unique %.3f ms x %lld, k_depth_filter_unique %.3f ms x %lld, k_depth_filter_points x %lld\n", ms[0], n[0],
              ms[5], n[5], n2[1]);
  if (!identical) return 2;
  // the oracle's counts on this scene are 5057 kept (106 wrong) and 4923 kept (1 wrong)
  if (!(a.wrong >= 25 && 5 * b.wrong <= a.wrong && b.kept < a.kept && 100 * b.kept >= 95 * a.kept && n[0] == 3 && n[5] == 1 &&
        n2[0] == 0 && n2[1] == 2))
    return 1;
  std::printf("ok\n");
  return 0;
}
