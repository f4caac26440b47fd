// The connected components of a welded mesh through include/vslam_filter_hip.hpp's TsdfVolumeHip::components and ::prune
// (DESIGN.md section 25).  The volume is written directly: a flat wall between two layers, and two single voxels of the
// other sign, one on each side of it, each of which makes a small closed fragment.  The demo welds, prints the component
// sizes, prunes, and holds a few invariants: the sizes add up to the triangles, the wall is the largest component, prune(1)
// is the identity, a pruned mesh keeps ascending keys and in-range faces, and the weld is what it was.  Prints "ok" on
// success.
#include <algorithm>
#include <cstdio>
#include <map>
#include <vector>

#include "vslam_filter_hip.hpp"

static bool well_formed(const TsdfVolumeHip::IndexedMesh& m) {
  bool ok = m.xyz.size() == 3 * m.vertices() && m.grey.size() == m.vertices() && m.faces.size() % 3 == 0;
  for (size_t v = 1; ok && v < m.vertices(); ++v) ok = m.key[v - 1] < m.key[v];
  for (size_t c = 0; ok && c < m.faces.size(); ++c) ok = m.faces[c] < m.vertices();
  return ok;
}

int main() {
  const int nx = 24, ny = 20, nz = 12;
  const double origin[3] = {-1.2, -1.0, 1.0};
  TsdfVolumeHip vol(nx, ny, nz, origin, 0.1, 0.4);
  const size_t n = (size_t)nx * ny * nz;
  std::vector<float> sum(n);
  std::vector<unsigned short> cnt(n, 2);
  std::vector<unsigned int> gsum(n, 200);
  auto at = [&](int i, int j, int k) -> float& { return sum[(size_t)i + (size_t)nx * ((size_t)j + (size_t)ny * (size_t)k)]; };
  for (int k = 0; k < nz; ++k)
    for (int j = 0; j < ny; ++j)
      for (int i = 0; i < nx; ++i) at(i, j, k) = k < 6 ? 1.f : -1.f;             // free space in front of the wall
  at(4, 4, 2) = -1.f;                                                            // a speck in front of it
  at(15, 10, 9) = 1.f;                                                           // and a hole behind it
  if (ekf_fusion_set_volume(vol.handle(), sum.data(), cnt.data(), gsum.data(), 2) != EKF_OK) return 2;

  vol.profile(true);
  const TsdfVolumeHip::IndexedMesh weld = vol.weld(1);
  const TsdfVolumeHip::Components comp = vol.components();
  std::map<unsigned int, unsigned int> sizes;                                    // label -> triangles
  bool ok = comp.label.size() == weld.vertices();
  for (size_t v = 0; ok && v < weld.vertices(); ++v) {
    ok = comp.label[v] <= v && comp.label[comp.label[v]] == comp.label[v];
    sizes[comp.label[v]] = comp.size[v];
  }
  size_t total = 0, wall = 0;
  std::printf("%zu vertices, %zu triangles, %llu components:", weld.vertices(), weld.triangles(), comp.count);
  for (const auto& s : sizes) {
    std::printf(" %u (label %u)", s.second, s.first);
    total += s.second;
    wall = std::max<size_t>(wall, s.second);
  }
  std::printf("\n");
  ok = ok && sizes.size() == comp.count && comp.count == 3 && total == weld.triangles() && wall == (size_t)(nx - 1) * (ny - 1) * 8;

  unsigned long long kept = 0;
  const TsdfVolumeHip::IndexedMesh all = vol.prune(1), big = vol.prune((unsigned int)wall, false, &kept), again = vol.pruned();
  const TsdfVolumeHip::IndexedMesh one = vol.prune(1, true), none = vol.prune((unsigned int)wall + 1), after = vol.mesh();
  ok = ok && all.key == weld.key && all.faces == weld.faces && all.xyz == weld.xyz && all.grey == weld.grey;      // the identity
  ok = ok && kept == 1 && big.triangles() == wall && big.vertices() < weld.vertices() && well_formed(big);
  ok = ok && again.key == big.key && again.faces == big.faces && one.key == big.key && one.faces == big.faces && one.xyz == big.xyz;
  ok = ok && none.vertices() == 0 && none.triangles() == 0;
  ok = ok && after.key == weld.key && after.faces == weld.faces && after.xyz == weld.xyz;                         // the weld stays
  double ms[8];
  long long cnt_[8];
  vol.getComponentProfile(ms, cnt_);
  std::printf("pruned to the wall: %zu vertices, %zu triangles; init %.3f, union %.3f, count %.3f, largest %.3f, flags %.3f, scan %.3f, "
              "vertices %.3f, faces %.3f ms\n", big.vertices(), big.triangles(), ms[0], ms[1], ms[2], ms[3], ms[4], ms[5], ms[6], ms[7]);
  ok = ok && cnt_[0] == 1 && cnt_[1] == 1 && cnt_[2] == 1 && cnt_[3] == 1 && cnt_[4] == 5 && cnt_[5] == 12 && cnt_[6] == 3 && cnt_[7] == 3;
  if (!ok) {
    std::printf("FAILED\n");
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
