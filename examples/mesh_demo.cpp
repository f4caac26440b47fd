// The indexed mesh of a fused volume through include/vslam_filter_hip.hpp's TsdfVolumeHip::weld: two
// cameras look at a tilted wall, their exact depth maps are integrated from the host, and the mesh comes back welded on the
// device with vertex normals.  The demo welds the triangle soup of extract() once more on the host, by sorting its keys, and
// holds the two against each other bit for bit; the normals must point from the wall to the cameras.  Prints the counts and
// "ok" on success.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "vslam_filter_hip.hpp"

static const int W = 96, H = 64;
static const double K[4] = {64.0, 64.0, 48.0, 32.0};
static const double Z0 = 2.0, SLOPE = 0.15;              // the wall z = Z0 + SLOPE x

// the depth of the wall along the ray of pixel (x, y) from a camera at (cx, 0, 0) with no rotation
static std::vector<float> depth_map(double cx) {
  std::vector<float> d((size_t)W * H);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const double rx = (x - K[2]) / K[0];               // X = cx + z rx, and z = Z0 + SLOPE X
      d[(size_t)y * W + x] = (float)((Z0 + SLOPE * cx) / (1.0 - SLOPE * rx));
    }
  return d;
}

int main() {
  const double voxel = 0.1, trunc = 0.4, origin[3] = {-2.0, -1.2, Z0 - 1.0};
  TsdfVolumeHip vol(41, 25, 21, origin, voxel, trunc);
  std::vector<unsigned char> grey((size_t)W * H);
  for (size_t i = 0; i < grey.size(); ++i) grey[i] = (unsigned char)(i * 7 % 251);
  const double cams[2] = {0.25, -0.25};
  for (double cx : cams) {
    const double pose[7] = {cx, 0, 0, 1, 0, 0, 0};
    vol.integrateHost(depth_map(cx).data(), grey.data(), W, H, K, pose);
  }
  vol.profile(true);
  const TsdfVolumeHip::Mesh soup = vol.extract(2);
  const TsdfVolumeHip::IndexedMesh plain = vol.weld(2), mesh = vol.weld(2, true), again = vol.mesh();

  // the host weld: the distinct keys in ascending order, each with the values of its first occurrence
  std::vector<unsigned long long> keys(soup.key);
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  bool same = keys == mesh.key && keys == plain.key && mesh.triangles() == soup.triangles() && plain.normal.empty() &&
              plain.xyz == mesh.xyz && plain.faces == mesh.faces && again.normal == mesh.normal && again.faces == mesh.faces;
  for (size_t c = 0; same && c < soup.key.size(); ++c) {
    const size_t v = (size_t)(std::lower_bound(keys.begin(), keys.end(), soup.key[c]) - keys.begin());
    same = mesh.faces[c] == v && std::memcmp(&mesh.xyz[3 * v], &soup.xyz[3 * c], 3 * sizeof(double)) == 0 && mesh.grey[v] == soup.grey[c];
  }

  // the wall's normal towards the cameras is (SLOPE, 0, -1) / |.|
  const double len = std::sqrt(1.0 + SLOPE * SLOPE), want[3] = {SLOPE / len, 0.0, -1.0 / len};
  double worst = 1.0;
  size_t with_normal = 0;
  for (size_t v = 0; v < mesh.vertices(); ++v) {
    const float* n = &mesh.normal[3 * v];
    if (n[0] == 0.f && n[1] == 0.f && n[2] == 0.f) continue;
    ++with_normal;
    worst = std::fmin(worst, n[0] * want[0] + n[1] * want[1] + n[2] * want[2]);
  }
  double ms[5], fms[4];
  long long n[5], fn[4];
  vol.getMeshProfile(ms, n);
  vol.getProfile(fms, fn);
  std::printf("weld(2, normals): %zu vertices for %zu triangles (%zu soup corners), %zu with a normal, least n . wall = %.4f; host weld %s\n",
              mesh.vertices(), mesh.triangles(), soup.key.size(), with_normal, worst, same ? "equal" : "DIFFERS");
  std::printf("cells %.3f, edges %.3f, scan %.3f, vertices %.3f, faces %.3f ms over %lld welds; %lld extract\n", ms[0], ms[1], ms[2], ms[3],
              ms[4], n[0], fn[3]);
  if (!(same && mesh.triangles() > 100 && mesh.vertices() * 3 < soup.key.size() && with_normal == mesh.vertices() && worst > 0.9 &&
        n[0] == 2 && n[4] == 2 && fn[1] == 1 && fn[3] == 1))
    return 1;
  std::printf("ok\n");
  return 0;
}
