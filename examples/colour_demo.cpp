// Colour through include/vslam_filter_hip.hpp's DenseStereoHip and TsdfVolumeHip: a fronto-parallel
// wall z = Z with a different texture in each of B, G and R is seen by three cameras half a unit apart.  The colour views go
// into dense slots (their grey conversion is made on the device), the true depth maps with the colour images into a colour
// volume; the mesh is extracted with its vertex colours and written as a coloured PLY, and the volume is rendered from the
// first camera.  Where all three maps saw the wall the rendered colour is the image's.  Usage: colour_demo [out.ply].
// Prints the counts and "ok" on success.
#include <cmath>
#include <cstdio>
#include <map>
#include <vector>

#include "vslam_filter_hip.hpp"

static const int W = 96, H = 64;
static const double K[4] = {64.0, 64.0, 48.0, 32.0};
static const double Z = 3.5;

static double texture(int c, double X, double Y) {
  return 127.5 + 40.0 * (std::sin((1.3 - 0.3 * c) * X + 0.4 * Y + c) + std::sin(0.9 * X - (1.1 + 0.2 * c) * Y + 0.7));
}

// the wall z = Z seen from a camera at (cx, 0, 0) with no rotation: H rows of W x 3 bytes, B G R
static std::vector<unsigned char> image(double cx) {
  std::vector<unsigned char> bgr((size_t)W * H * 3);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x)
      for (int c = 0; c < 3; ++c) {
        const double v = std::floor(texture(c, cx + Z * (x - K[2]) / K[0], Z * (y - K[3]) / K[1]) + 0.5);
        bgr[((size_t)y * W + x) * 3 + c] = (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
      }
  return bgr;
}

int main(int argc, char** argv) {
  const double cams[3] = {0.0, 0.5, -0.5};
  // the views: a colour slot keeps its image and holds the grey conversion the sweep reads
  DenseStereoHip ds(W, H, 3);
  const std::vector<unsigned char> img0 = image(cams[0]);
  for (int s = 0; s < 3; ++s) {
    const double pose[7] = {cams[s], 0, 0, 1, 0, 0, 0};
    ds.setViewColour(s, image(cams[s]).data(), K, pose);
  }
  const std::vector<unsigned char> grey0 = ds.viewImage(0);
  size_t grey_bad = 0;
  for (size_t i = 0; i < grey0.size(); ++i) {
    const unsigned b = img0[3 * i], g = img0[3 * i + 1], r = img0[3 * i + 2];
    grey_bad += grey0[i] != (unsigned char)((b * 1868u + g * 9617u + r * 4899u + 8192u) >> 14);
  }
  if (!ds.hasColour(0) || ds.viewColour(0) != img0 || grey_bad) return 2;

  // a slab of 0.1-unit voxels round the wall: 61 x 41 x 13, truncation 4 voxels, with colour
  const double voxel = 0.1, trunc = 0.4, origin[3] = {-3.0, -2.0, Z - 0.62};
  TsdfVolumeHip vol(61, 41, 13, origin, voxel, trunc, 0, true);
  const std::vector<float> depth((size_t)W * H, (float)Z);
  for (int s = 0; s < 3; ++s) {
    const double pose[7] = {cams[s], 0, 0, 1, 0, 0, 0};
    vol.integrateHostColour(depth.data(), image(cams[s]).data(), W, H, K, pose);
  }
  TsdfVolumeHip plain(61, 41, 13, origin, voxel, trunc);
  bool refused = false;
  try {
    const double pose[7] = {0, 0, 0, 1, 0, 0, 0};
    plain.integrateHostColour(depth.data(), img0.data(), W, H, K, pose);      // a plain volume takes no colour
  } catch (const std::runtime_error&) {
    refused = true;
  }
  if (!refused || plain.hasColour() || !vol.hasColour()) return 2;

  const TsdfVolumeHip::Mesh mesh = vol.extract(3);
  const double pose0[7] = {0, 0, 0, 1, 0, 0, 0};
  const TsdfVolumeHip::Render a = vol.raycast(W, H, K, pose0, Z - 1.0, Z + 1.0, voxel / 2, 3);
  size_t hits = 0;
  double err[3] = {0, 0, 0};
  for (size_t i = 0; i < a.depth.size(); ++i)
    if (a.depth[i] > 0.f) {
      ++hits;
      for (int c = 0; c < 3; ++c) err[c] += std::fabs((double)a.colour[3 * i + c] - (double)img0[3 * i + c]);
    }
  for (int c = 0; c < 3; ++c) err[c] /= hits ? (double)hits : 1.0;

  // weld by key (equal keys: bit-equal vertices, equal colours) and write x y z intensity red green blue
  std::map<unsigned long long, int> index;
  std::vector<size_t> first;
  std::vector<int> face(mesh.key.size());
  for (size_t v = 0; v < mesh.key.size(); ++v) {
    auto it = index.find(mesh.key[v]);
    if (it == index.end()) {
      it = index.emplace(mesh.key[v], (int)first.size()).first;
      first.push_back(v);
    }
    face[v] = it->second;
  }
  if (argc > 1) {
    FILE* f = std::fopen(argv[1], "w");
    if (!f) return 3;
    std::fprintf(f, "ply\nformat ascii 1.0\nelement vertex %zu\nproperty double x\nproperty double y\nproperty double z\n"
                    "property uchar intensity\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nelement face %zu\n"
                    "property list uchar int vertex_indices\nend_header\n", first.size(), mesh.triangles());
    for (size_t v : first)
      std::fprintf(f, "%.17g %.17g %.17g %d %d %d %d\n", mesh.xyz[3 * v], mesh.xyz[3 * v + 1], mesh.xyz[3 * v + 2], mesh.grey[v],
                   mesh.colour[3 * v + 2], mesh.colour[3 * v + 1], mesh.colour[3 * v]);
    for (size_t t = 0; t < mesh.triangles(); ++t) std::fprintf(f, "3 %d %d %d\n", face[3 * t], face[3 * t + 1], face[3 * t + 2]);
    std::fclose(f);
  }
  std::printf("triangles: %zu, vertices %zu; coloured hits: %zu of %d, mean |colour - image| = %.3g %.3g %.3g (B G R)\n",
              mesh.triangles(), first.size(), hits, W * H, err[0], err[1], err[2]);
  if (!(mesh.triangles() > 1000 && mesh.colour.size() == mesh.key.size() * 3 && a.colour.size() == a.depth.size() * 3 &&
        hits > 1000 && err[0] < 8.0 && err[1] < 8.0 && err[2] < 8.0))
    return 1;
  std::printf("ok\n");
  return 0;
}
