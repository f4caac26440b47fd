// Vertex-clustering simplification of a welded mesh through include/vslam_filter_hip.hpp's TsdfVolumeHip::simplify (DESIGN.md
// section 28).  The volume is written directly: the analytic sphere of radius 1.25 round the world origin on a 17 x 15 x 13
// grid.  The demo welds with normals, simplifies at cells of 1 and 2 voxels, and the smoothed mesh at 2, prints the triangles and
// vertices before and after, and holds a few invariants: the counts add up, a face has three distinct vertices and no two faces
// share their three, every vertex is referenced, keys ascend, the map sends every source vertex of a used cell to the vertex
// with that cell's key, the mean radius falls, and by less than the sagitta of a chord as long as a cell's diagonal (the mean of
// a cell's members lies slightly inside a convex surface: 1.5 per cent of the radius at 1 voxel, 6.3 at 2), every normal is
// within cosine 0.8 of the radial direction (a cell's diagonal spans 0.7 rad), and the weld is what it was.  Prints "ok" on
// success.
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

// what holds for every result, given its source, its map and its stats
static bool sound(const Mesh& src, const Mesh& m, const std::vector<unsigned int>& map, const TsdfVolumeHip::SimplifyStats& st) {
  bool ok = m.triangles() + st.degenerate + st.duplicate == src.triangles() && map.size() == src.vertices() && m.vertices() > 0;
  std::set<std::vector<unsigned int> > triples;
  std::vector<char> referenced(m.vertices(), 0);
  for (size_t t = 0; ok && t < m.triangles(); ++t) {
    std::vector<unsigned int> f(m.faces.begin() + 3 * t, m.faces.begin() + 3 * t + 3);
    ok = f[0] < m.vertices() && f[1] < m.vertices() && f[2] < m.vertices() && f[0] != f[1] && f[0] != f[2] && f[1] != f[2];
    if (!ok) break;
    for (int c = 0; c < 3; ++c) referenced[f[c]] = 1;
    std::sort(f.begin(), f.end());
    ok = triples.insert(f).second;
  }
  for (size_t v = 0; ok && v < m.vertices(); ++v) ok = referenced[v] && (v == 0 || m.key[v - 1] < m.key[v]);
  size_t mapped = 0;
  for (size_t v = 0; ok && v < map.size(); ++v) {
    if (map[v] == 0xffffffffu) continue;
    ok = map[v] < m.vertices();
    ++mapped;
  }
  return ok && mapped >= m.vertices();
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
  const Mesh weld = vol.weld(1, true);
  TsdfVolumeHip::SimplifyStats st1, st2, st3;
  const Mesh fine = vol.simplify(voxel, 0, &st1), again = vol.simplified();
  const std::vector<unsigned int> map1 = vol.simplifyMap();
  std::printf("cell 1 voxel: %zu -> %zu triangles, %zu -> %zu vertices, %llu degenerate, %llu duplicate\n", weld.triangles(),
              fine.triangles(), weld.vertices(), fine.vertices(), st1.degenerate, st1.duplicate);
  bool ok = sound(weld, fine, map1, st1) && fine.triangles() < weld.triangles() && fine.vertices() < weld.vertices();
  ok = ok && again.xyz == fine.xyz && again.faces == fine.faces && again.key == fine.key && again.grey == fine.grey && again.normal == fine.normal;
  ok = ok && fine.normal.size() == 3 * fine.vertices();
  double ms[10];
  long long cnt_[10];
  vol.getSimplifyProfile(ms, cnt_);
  std::printf("cells %.3f, count %.3f, offsets %.3f, 5 scans %.3f, fill %.3f, lists %.3f, flags %.3f, vertices %.3f, faces %.3f, map %.3f ms\n",
              ms[0], ms[1], ms[2], ms[3], ms[4], ms[5], ms[6], ms[7], ms[8], ms[9]);
  for (int k = 0; k < 10; ++k) ok = ok && cnt_[k] == (k == 3 ? 5 : 1);

  const Mesh coarse = vol.simplify(2.0 * voxel, 0, &st2);
  const std::vector<unsigned int> map2 = vol.simplifyMap();
  std::printf("cell 2 voxels: %zu -> %zu triangles, %zu -> %zu vertices, %llu degenerate, %llu duplicate\n", weld.triangles(),
              coarse.triangles(), weld.vertices(), coarse.vertices(), st2.degenerate, st2.duplicate);
  ok = ok && sound(weld, coarse, map2, st2) && coarse.triangles() < fine.triangles();

  const Mesh smooth = vol.smooth(10, 0.5, -0.53, false, true);
  const Mesh both = vol.simplify(2.0 * voxel, 2, &st3);
  const std::vector<unsigned int> map3 = vol.simplifyMap();
  std::printf("the smoothed mesh at 2 voxels: %zu -> %zu triangles, %zu -> %zu vertices\n", smooth.triangles(), both.triangles(),
              smooth.vertices(), both.vertices());
  ok = ok && sound(smooth, both, map3, st3);

  const Mesh after = vol.mesh(), smoothed = vol.smoothed();
  ok = ok && after.xyz == weld.xyz && after.faces == weld.faces && after.key == weld.key && after.normal == weld.normal;   // the weld stays
  ok = ok && smoothed.xyz == smooth.xyz && smoothed.normal == smooth.normal;                                                // and the smoothed mesh
  const double r0 = mean_radius(weld), r1 = mean_radius(fine), r2 = mean_radius(coarse);
  double least = 1.0;
  for (size_t v = 0; v < coarse.vertices(); ++v) {
    const double* p = &coarse.xyz[3 * v];
    const float* nr = &coarse.normal[3 * v];
    least = std::min(least, (p[0] * nr[0] + p[1] * nr[1] + p[2] * nr[2]) / std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]));
  }
  std::printf("mean radius %.4f -> %.4f -> %.4f, least cosine of a normal with the radial direction %.4f\n", r0, r1, r2, least);
  ok = ok && r1 <= r0 && r1 > 0.98 * r0 && r2 <= r0 && r2 > 0.93 * r0 && least > 0.8;
  if (!ok) {
    std::printf("FAILED\n");
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
