// Taubin smoothing of a welded mesh through include/vslam_filter_hip.hpp's TsdfVolumeHip::smooth.
// The volume is written directly: the analytic sphere of radius 1.25 round the world origin on a 17 x 15 x 13 grid.  The demo
// welds, smooths with the defaults and with normals, prints the vertices, the triangles and the number of boundary vertices,
// and holds a few invariants: a closed surface has no boundary vertex, the incident counts add up to three a triangle, faces,
// grey and key are the weld's, the mean radius stays within half a per cent, the mean distance of a vertex from the centroid
// of its neighbours falls to less than half, every normal is within cosine 0.99 of the radial direction, and the weld is what
// it was.  Prints "ok" on success.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <set>
#include <vector>

#include "vslam_filter_hip.hpp"

typedef TsdfVolumeHip::IndexedMesh Mesh;

static double mean_radius(const Mesh& m) {
  double s = 0.0;
  for (size_t v = 0; v < m.vertices(); ++v)
    s += std::sqrt(m.xyz[3 * v] * m.xyz[3 * v] + m.xyz[3 * v + 1] * m.xyz[3 * v + 1] + m.xyz[3 * v + 2] * m.xyz[3 * v + 2]);
  return s / (double)m.vertices();
}

// the mean distance of a vertex from the centroid of its neighbours
static double roughness(const Mesh& m) {
  std::vector<std::set<unsigned int> > nb(m.vertices());
  for (size_t t = 0; t < m.triangles(); ++t)
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b)
        if (a != b) nb[m.faces[3 * t + a]].insert(m.faces[3 * t + b]);
  double total = 0.0;
  for (size_t v = 0; v < m.vertices(); ++v) {
    double c[3] = {0.0, 0.0, 0.0};
    for (unsigned int w : nb[v])
      for (int k = 0; k < 3; ++k) c[k] += m.xyz[3 * w + k];
    double d = 0.0;
    for (int k = 0; k < 3; ++k) {
      const double e = c[k] / (double)nb[v].size() - m.xyz[3 * v + k];
      d += e * e;
    }
    total += std::sqrt(d);
  }
  return total / (double)m.vertices();
}

int main() {
  const int nx = 17, ny = 15, nz = 13;
  const double origin[3] = {-2.0, -1.75, -1.5}, voxel = 0.25, trunc = 0.5, radius = 1.25;
  TsdfVolumeHip vol(nx, ny, nz, origin, voxel, trunc);
  const size_t n = (size_t)nx * ny * nz;
  std::vector<float> sum(n);
  std::vector<unsigned short> cnt(n, 1);
  std::vector<unsigned int> gsum(n, 128);
  for (int k = 0; k < nz; ++k)
    for (int j = 0; j < ny; ++j)
      for (int i = 0; i < nx; ++i) {
        const double x = origin[0] + i * voxel, y = origin[1] + j * voxel, z = origin[2] + k * voxel;
        const double d = (std::sqrt(x * x + y * y + z * z) - radius) / trunc;
        sum[(size_t)i + (size_t)nx * ((size_t)j + (size_t)ny * (size_t)k)] = (float)std::max(-1.0, std::min(1.0, d));
      }
  if (ekf_fusion_set_volume(vol.handle(), sum.data(), cnt.data(), gsum.data(), 1) != EKF_OK) return 2;

  vol.profile(true);
  const Mesh weld = vol.weld(1);
  const Mesh smooth = vol.smooth(10, 0.5, -0.53, false, true), again = vol.smoothed(), after = vol.mesh();
  const TsdfVolumeHip::Adjacency adj = vol.adjacency();
  size_t boundary = 0, incident = 0;
  bool ok = adj.inc.size() == weld.vertices();
  for (size_t v = 0; ok && v < weld.vertices(); ++v) {
    boundary += adj.boundary[v];
    incident += adj.inc[v];
    ok = adj.deg[v] >= 2;
  }
  std::printf("%zu vertices, %zu triangles, %zu boundary vertices\n", smooth.vertices(), smooth.triangles(), boundary);
  ok = ok && boundary == 0 && incident == 3 * weld.triangles();
  ok = ok && smooth.faces == weld.faces && smooth.key == weld.key && smooth.grey == weld.grey && smooth.xyz != weld.xyz;
  ok = ok && again.xyz == smooth.xyz && again.normal == smooth.normal && smooth.normal.size() == 3 * weld.vertices();
  ok = ok && after.xyz == weld.xyz && after.faces == weld.faces && after.key == weld.key;                  // the weld stays
  const double r0 = mean_radius(weld), r1 = mean_radius(smooth), q0 = roughness(weld), q1 = roughness(smooth);
  double least = 1.0;
  for (size_t v = 0; v < smooth.vertices(); ++v) {
    const double* p = &smooth.xyz[3 * v];
    const float* nr = &smooth.normal[3 * v];
    least = std::min(least, (p[0] * nr[0] + p[1] * nr[1] + p[2] * nr[2]) / std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]));
  }
  std::printf("mean radius %.4f -> %.4f, roughness %.4f -> %.4f, least cosine of a normal with the radial direction %.4f\n", r0, r1,
              q0, q1, least);
  ok = ok && std::fabs(r1 / r0 - 1.0) < 0.005 && q1 < 0.5 * q0 && least > 0.99;
  double ms[7];
  long long cnt_[7];
  vol.getSmoothProfile(ms, cnt_);
  std::printf("count %.3f, offsets %.3f, scan %.3f, fill %.3f, lists %.3f, 20 steps %.3f, normals %.3f ms\n", ms[0], ms[1], ms[2],
              ms[3], ms[4], ms[5], ms[6]);
  ok = ok && cnt_[0] == 1 && cnt_[1] == 1 && cnt_[2] == 1 && cnt_[3] == 1 && cnt_[4] == 1 && cnt_[5] == 20 && cnt_[6] == 1;
  const Mesh plain = vol.smooth(2, 0.5, 0.0);                                      // the adjacency is held: two steps and nothing else
  vol.getSmoothProfile(ms, cnt_);
  ok = ok && plain.normal.empty() && cnt_[0] == 1 && cnt_[4] == 1 && cnt_[5] == 22 && cnt_[6] == 1;
  if (!ok) {
    std::printf("FAILED\n");
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
