// The four kernels of csrc/ekf_fusion.hpp run lane by lane on the host by host_kernels.hpp, which
// says how to build and run this.  It reads the case files tools/fusion_host_check.py writes (inputs in buffers of exactly
// the device's sizes, and the numpy oracle's outputs) and compares bit for bit.
#include "host_tsdf.hpp"

static int run(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::perror(path); return 2; }
  const auto hdr = take<int>(f, 5);
  const auto par = take<double>(f, 5);
  ekf::TsdfGrid g{hdr[0], hdr[1], hdr[2], {par[0], par[1], par[2]}, par[3]};
  const int n_maps = hdr[3], min_count = hdr[4];
  const size_t nvox = (size_t)g.nx * g.ny * g.nz;
  struct Map { int W, H; std::vector<double> K, pose; std::vector<float> depth; std::vector<unsigned char> img; };
  std::vector<Map> maps;
  for (int m = 0; m < n_maps; ++m) {
    const auto wh = take<int>(f, 2);
    Map mp{wh[0], wh[1], take<double>(f, 4), take<double>(f, 7), {}, {}};
    mp.depth = take<float>(f, (size_t)wh[0] * wh[1]);
    mp.img = take<unsigned char>(f, (size_t)wh[0] * wh[1]);
    maps.push_back(std::move(mp));
  }
  auto sum = take<float>(f, nvox);
  auto cnt = take<unsigned short>(f, nvox);
  auto gsum = take<unsigned>(f, nvox);
  const auto w_sum = take<float>(f, nvox);
  const auto w_cnt = take<unsigned short>(f, nvox);
  const auto w_gsum = take<unsigned>(f, nvox);
  const size_t n_want = (size_t)take<unsigned long long>(f, 1)[0];
  const auto w_xyz = take<double>(f, n_want * 9);
  const auto w_key = take<unsigned long long>(f, n_want * 3);
  const auto w_grey = take<unsigned char>(f, n_want * 3);
  std::fclose(f);

  for (const Map& mp : maps) {
    ekf::IntegrateArgs a{};
    a.sum = sum.data(); a.cnt = cnt.data(); a.gsum = gsum.data();
    a.depth = mp.depth.data(); a.img = mp.img.data(); a.W = mp.W; a.H = mp.H;
    a.g = g; a.trunc = par[4];
    a.fx = mp.K[0]; a.fy = mp.K[1]; a.cx = mp.K[2]; a.cy = mp.K[3];
    double q[4];
    if (!ekf::dense_pose(mp.pose.data(), a.t, a.R, q)) return 2;
    launch({(unsigned)((nvox + 255) / 256), 1, 1}, [&] { ekf::k_tsdf_integrate(a); });
  }

  const HostMesh m = host_extract(sum, cnt, gsum, g, min_count);

  const int bad = differs("sum", sum, w_sum) + differs("cnt", cnt, w_cnt) + differs("gsum", gsum, w_gsum) +
                  differs("xyz", m.xyz, w_xyz) + differs("key", m.key, w_key) + differs("grey", m.grey, w_grey);
  std::printf("%s: %d x %d x %d, %d maps, min_count %d, %zu triangles (oracle %zu): %s\n", path, g.nx, g.ny, g.nz, n_maps,
              min_count, m.n_tri, n_want, bad ? "DIFFERS" : "equal");
  return bad ? 1 : 0;
}
