// How far a simplified mesh lies from the mesh it was made from, through include/vslam_filter_hip.hpp's TsdfVolumeHip::distance
// (DESIGN.md section 31).  The volume is written directly: the analytic sphere of radius 1.25 round the world origin on a
// 17 x 15 x 13 grid.  The demo welds, simplifies the weld at a cell of 2 voxels, measures the simplified vertices against the weld
// and the weld's vertices against the simplified mesh, prints both one-sided maxima (the Hausdorff distances over vertices) and
// holds a few invariants: a mesh is at distance 0 from itself, every closest point lies within dist of its query, most simplified
// vertices lie on the inner side of the weld (clustering shrinks a convex surface), the weld given back through setDistanceMesh
// gives the same distances, the result does not depend on the grid, and the weld is what it was.  Prints "ok" on success.
#include <cmath>
#include <cstdio>
#include <vector>

#include "vslam_filter_hip.hpp"

typedef TsdfVolumeHip::IndexedMesh Mesh;
typedef TsdfVolumeHip::MeshDistance Dist;

static bool same(const Dist& a, const Dist& b) { return a.dist == b.dist && a.tri == b.tri && a.closest == b.closest && a.side == b.side; }

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

  const Mesh weld = vol.weld(1);
  const Mesh simp = vol.simplify(2.0 * voxel);
  vol.profile(true);
  const Dist to_weld = vol.distance(0, 3);                   // the simplified vertices against the weld
  const TsdfVolumeHip::DistanceStats a = vol.distanceStats(voxel / 4);
  const Dist to_simp = vol.distance(3, 0);                   // the weld's vertices against the simplified mesh
  const TsdfVolumeHip::DistanceStats b = vol.distanceStats(voxel / 4);
  std::printf("%zu triangles, simplified to %zu\n", weld.triangles(), simp.triangles());
  std::printf("simplified -> weld: max %.6f mean %.6f rms %.6f, %llu of %llu within %.4f\n", a.max, a.mean, a.rms, a.within, a.n, voxel / 4);
  std::printf("weld -> simplified: max %.6f mean %.6f rms %.6f, %llu of %llu within %.4f\n", b.max, b.mean, b.rms, b.within, b.n, voxel / 4);
  bool ok = to_weld.points() == simp.vertices() && to_simp.points() == weld.vertices() && a.n == simp.vertices() && b.n == weld.vertices() &&
            a.n_bad == 0 && b.n_bad == 0;
  ok = ok && a.max > 0.0 && a.max < voxel && b.max > a.max && b.max < 2.0 * voxel && a.mean < a.rms && a.rms < a.max && b.mean > a.mean;
  ok = ok && to_weld.dist[(size_t)a.argmax] == a.max && to_simp.dist[(size_t)b.argmax] == b.max;
  size_t inner = 0;
  for (size_t i = 0; ok && i < to_weld.points(); ++i) {
    const double* c = &to_weld.closest[i * 3];
    const double* p = &simp.xyz[i * 3];
    const double d = std::sqrt((p[0] - c[0]) * (p[0] - c[0]) + (p[1] - c[1]) * (p[1] - c[1]) + (p[2] - c[2]) * (p[2] - c[2]));
    ok = std::fabs(d - to_weld.dist[i]) <= 1e-12 && to_weld.tri[i] < weld.triangles();
    inner += to_weld.side[i] < 0;
  }
  ok = ok && inner * 2 > to_weld.points();

  double ms[9];
  long long launches[9];
  vol.getDistanceProfile(ms, launches);
  std::printf("box %.3f grid %.3f count %.3f offsets %.3f scan %.3f fill %.3f query %.3f stats %.3f reduce %.3f ms\n", ms[0], ms[1], ms[2], ms[3],
              ms[4], ms[5], ms[6], ms[7], ms[8]);
  for (int k = 0; k < 7; ++k) ok = ok && launches[k] == 2;
  ok = ok && launches[7] == 2 && launches[8] == 2;

  // a mesh against itself: every vertex of a valid triangle is at distance 0
  const Dist self = vol.distance(3, 3);
  ok = ok && vol.distanceStats().max == 0.0 && self.points() == simp.vertices();
  // brute force and a fine grid: the same arrays
  for (int g : {1, 64}) {
    vol.setDistanceGrid(g);
    ok = ok && same(vol.distance(0, 3), to_weld) && same(vol.distance(3, 0), to_simp);
  }
  vol.setDistanceGrid(0);
  // the weld given back by the caller, and the simplified vertices as points
  vol.setDistanceMesh(weld.xyz, weld.faces);
  ok = ok && same(vol.distance(4, 3), to_weld) && same(vol.distancePoints(4, simp.xyz), to_weld) && same(vol.distancePoints(0, simp.xyz), to_weld);
  const Mesh after = vol.mesh();
  ok = ok && after.xyz == weld.xyz && after.faces == weld.faces && after.grey == weld.grey;                  // the source stays
  if (!ok) {
    std::printf("FAILED\n");
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
