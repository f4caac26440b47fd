// Depth-map fusion through include/vslam_filter_hip.hpp's TsdfVolumeHip: three cameras half a unit apart look at a textured
// fronto-parallel wall that lies exactly on plane 5 of 12 (the scene of dense_demo.cpp); two of the views are swept and
// filtered, their filtered maps are integrated straight from the dense slots into a volume round the wall, and the mesh
// comes back.  Prints the triangle count and "ok" on success.
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
  for (int s = 0; s < 3; ++s) ds.sweep(s, {(s + 1) % 3, (s + 2) % 3}, W_MIN, W_MAX, D, 2, 255);
  ds.filter(0, {1, 2}, 0.02, 2);
  ds.filter(1, {0, 2}, 0.02, 1);

  // a slab of 0.1-unit voxels round the wall: 41 x 25 x 13, truncation 4 voxels
  const double voxel = 0.1, trunc = 0.4, origin[3] = {-2.0, -1.2, Z - 0.65};
  TsdfVolumeHip vol(41, 25, 13, origin, voxel, trunc);
  bool refused = false;
  try {
    vol.integrate(ds, 2, true);                         // slot 2 was never filtered
  } catch (const std::runtime_error&) {
    refused = true;
  }
  if (!refused) return 2;
  vol.profile(true);
  vol.integrate(ds, 0, true);
  vol.integrate(ds, 1, true);
  const TsdfVolumeHip::Mesh once = vol.extract(1), both = vol.extract(2);
  double ms[4];
  long long n[4];
  vol.getProfile(ms, n);
  // where both views saw the wall the surface lies on it
  double worst = 0.0;
  for (size_t i = 0; i < both.triangles() * 3; ++i) worst = std::fmax(worst, std::fabs(both.xyz[3 * i + 2] - Z));
  std::printf("triangles: %zu seen once, %zu seen twice, worst |z - Z| = %.3g (Z = %.4f); integrate %.3f ms x %lld, "
              "count %.3f, scan %.3f, emit %.3f ms\n",
              once.triangles(), both.triangles(), worst, Z, ms[0], n[0], ms[1], ms[2], ms[3]);
  if (!(both.triangles() > 100 && once.triangles() >= both.triangles() && worst < voxel && vol.volume().maps == 2 && n[0] == 2 && n[1] == 2))
    return 1;
  std::printf("ok\n");
  return 0;
}
