// Ray casting through include/vslam_filter_hip.hpp's TsdfVolumeHip: the true depth maps of a textured fronto-parallel wall
// z = Z from three cameras half a unit apart are integrated into a volume round the wall; the volume is then rendered from
// the first camera (raycast) and from a fourth pose held by a dense slot (raycastView).  Where all three maps saw the wall
// the rendered depth is the wall's, the normal points back at the cameras and the grey value is the texture's.  Prints the
// hit counts and "ok" on success.
#include <cmath>
#include <cstdio>
#include <vector>

#include "vslam_filter_hip.hpp"

static const int W = 96, H = 64;
static const double K[4] = {64.0, 64.0, 48.0, 32.0};
static const double Z = 3.5;

static double texture(double X, double Y) {
  return 127.5 + 40.0 * (std::sin(1.3 * X + 0.4 * Y) + std::sin(0.9 * X - 1.1 * Y + 0.7));
}

// the wall z = Z seen from a camera at (cx, 0, 0) with no rotation
static std::vector<unsigned char> image(double cx) {
  std::vector<unsigned char> g((size_t)W * H);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const double v = std::floor(texture(cx + Z * (x - K[2]) / K[0], Z * (y - K[3]) / K[1]) + 0.5);
      g[(size_t)y * W + x] = (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
    }
  return g;
}

int main() {
  // a slab of 0.1-unit voxels round the wall: 61 x 41 x 13, truncation 4 voxels
  const double voxel = 0.1, trunc = 0.4, origin[3] = {-3.0, -2.0, Z - 0.62};
  TsdfVolumeHip vol(61, 41, 13, origin, voxel, trunc);
  const std::vector<float> depth((size_t)W * H, (float)Z);
  const double cams[3] = {0.0, 0.5, -0.5};
  for (int s = 0; s < 3; ++s) {
    const double pose[7] = {cams[s], 0, 0, 1, 0, 0, 0};
    vol.integrateHost(depth.data(), image(cams[s]).data(), W, H, K, pose);
  }
  const TsdfVolumeHip::Mesh mesh = vol.extract(3);
  bool refused = false;
  try {
    const double pose[7] = {0, 0, 0, 1, 0, 0, 0};
    vol.raycast(W, H, K, pose, Z - 1.0, Z + 1.0, 0.0);      // a step of 0
  } catch (const std::runtime_error&) {
    refused = true;
  }
  if (!refused) return 2;

  vol.profile(true);
  const double pose0[7] = {0, 0, 0, 1, 0, 0, 0};
  const TsdfVolumeHip::Render a = vol.raycast(W, H, K, pose0, Z - 1.0, Z + 1.0, voxel / 2, 3);
  DenseStereoHip ds(W, H, 1);
  const double pose3[7] = {0.2, -0.1, 0.3, 1, 0, 0, 0};
  ds.setView(0, image(0.2).data(), K, pose3);
  const TsdfVolumeHip::Render b = vol.raycastView(ds, 0, Z - 1.3, Z + 0.7, voxel / 2, 3);
  double ms[2];
  long long n[2];
  vol.getRaycastProfile(ms, n);

  size_t hits_a = 0, hits_b = 0;
  double worst_z = 0.0, worst_n = 0.0, grey_err = 0.0;
  const std::vector<unsigned char> img0 = image(0.0);
  for (size_t i = 0; i < a.depth.size(); ++i) {
    if (a.depth[i] > 0.f) {
      ++hits_a;
      worst_z = std::fmax(worst_z, std::fabs((double)a.depth[i] - Z));
      worst_n = std::fmax(worst_n, std::fabs((double)a.normal[3 * i + 2] + 1.0));
      grey_err += std::fabs((double)a.grey[i] - (double)img0[i]);
    }
    if (b.depth[i] > 0.f) {
      ++hits_b;
      worst_z = std::fmax(worst_z, std::fabs((double)b.depth[i] - (Z - 0.3)));
    }
  }
  grey_err /= hits_a ? (double)hits_a : 1.0;
  std::printf("hits: %zu and %zu of %d, worst |z - Z| = %.3g, worst |n_z + 1| = %.3g, mean |grey - image| = %.3g; mean %.3f ms x %lld, "
              "raycast %.3f ms x %lld; mesh %zu triangles\n",
              hits_a, hits_b, W * H, worst_z, worst_n, grey_err, ms[0], n[0], ms[1], n[1], mesh.triangles());
  if (!(a.width == W && a.height == H && hits_a > 1000 && hits_b > 1000 && worst_z < 0.1 * voxel && worst_n < 1e-3 && grey_err < 8.0 &&
        n[0] == 1 && n[1] == 2 && vol.extract(3).triangles() == mesh.triangles()))
    return 1;
  std::printf("ok\n");
  return 0;
}
