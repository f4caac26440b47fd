// The launches of the TSDF kernels that more than one host check makes (fusion, raycast, colour): the extraction of a mesh and
// the arguments of a ray cast.  It includes host_kernels.hpp and then the csrc headers, in the order they need.
#pragma once
#include "host_kernels.hpp"

#include "../ekf-monoslam_for_3d-reconstruction_amd/csrc/ekf_dense_stereo.hpp"
#include "../ekf-monoslam_for_3d-reconstruction_amd/csrc/ekf_raycast.hpp"

struct HostMesh {
  size_t n_tri;
  std::vector<double> xyz;
  std::vector<unsigned long long> key;
  std::vector<unsigned char> grey;
};

// k_tsdf_count -> k_tsdf_scan -> k_tsdf_emit (no emit for an empty mesh), into buffers of exactly the mesh's size.
static HostMesh host_extract(const std::vector<float>& sum, const std::vector<unsigned short>& cnt, const std::vector<unsigned>& gsum,
                             const ekf::TsdfGrid& g, int min_count) {
  const unsigned ncell = (unsigned)((size_t)(g.nx - 1) * (g.ny - 1) * (g.nz - 1)), nblk = (ncell + 255) / 256;
  std::vector<unsigned> tot(nblk);
  std::vector<unsigned long long> off((size_t)nblk + 1);
  ekf::ExtractArgs e{};
  e.sum = sum.data(); e.cnt = cnt.data(); e.gsum = gsum.data(); e.g = g; e.min_count = min_count; e.ncell = ncell;
  e.blk_tot = tot.data(); e.blk_off = off.data();
  launch({nblk, 1, 1}, [&] { ekf::k_tsdf_count(e); });
  launch({1, 1, 1}, [&] { ekf::k_tsdf_scan(tot.data(), off.data(), nblk); });
  const size_t n_tri = (size_t)off[nblk];
  HostMesh m{n_tri, std::vector<double>(n_tri * 9), std::vector<unsigned long long>(n_tri * 3), std::vector<unsigned char>(n_tri * 3)};
  e.xyz = m.xyz.data(); e.key = m.key.data(); e.grey = m.grey.data();
  if (n_tri) launch({nblk, 1, 1}, [&] { ekf::k_tsdf_emit(e); });
  return m;
}

// The arguments of a ray cast of a W x H view into depth, normal and grey.  view: fx, fy, cx, cy, pose7, z_near, step, as the
// case files keep them.  false = pose7 is no pose.
static bool host_raycast_args(ekf::RaycastArgs& a, const float* mean, const unsigned short* cnt, const unsigned* gsum, float* depth,
                              float* normal, unsigned char* grey, const ekf::TsdfGrid& g, int W, int H, int N, const double* view) {
  a = ekf::RaycastArgs{};
  a.mean = mean; a.cnt = cnt; a.gsum = gsum;
  a.depth = depth; a.normal = normal; a.grey = grey;
  a.W = W; a.H = H; a.g = g; a.inv = 1.0 / g.voxel;
  a.fx = view[0]; a.fy = view[1]; a.cx = view[2]; a.cy = view[3];
  double q[4];
  if (!ekf::dense_pose(view + 4, a.t, a.R, q)) return false;
  a.z_near = view[11]; a.step = view[12]; a.N = N;
  return true;
}
