// The two kernels of csrc/ekf_raycast.hpp run lane by lane on the host by host_kernels.hpp, which
// says how to build and run this.  It reads the case files tools/raycast_host_check.py writes (inputs in buffers of exactly
// the device's sizes, and the numpy oracle's outputs) and compares bit for bit.
#include "host_tsdf.hpp"

static int run(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::perror(path); return 2; }
  const auto hdr = take<int>(f, 7);
  const auto par = take<double>(f, 17);
  ekf::TsdfGrid g{hdr[0], hdr[1], hdr[2], {par[0], par[1], par[2]}, par[3]};
  const int W = hdr[3], H = hdr[4], N = hdr[5], min_count = hdr[6];
  const size_t nvox = (size_t)g.nx * g.ny * g.nz, npix = (size_t)W * H;
  const auto sum = take<float>(f, nvox);
  const auto cnt = take<unsigned short>(f, nvox);
  const auto gsum = take<unsigned>(f, nvox);
  const auto w_mean = take<float>(f, nvox);
  const auto w_depth = take<float>(f, npix);
  const auto w_normal = take<float>(f, npix * 3);
  const auto w_grey = take<unsigned char>(f, npix);
  std::fclose(f);

  std::vector<float> mean(nvox, 1.f), depth(npix, -1.f), normal(npix * 3, -1.f);
  std::vector<unsigned char> grey(npix, 0xA5);
  const ekf::MeanArgs m{sum.data(), cnt.data(), mean.data(), (unsigned)nvox, min_count};
  launch({(unsigned)((nvox + 255) / 256), 1, 1}, [&] { ekf::k_tsdf_mean(m); });

  ekf::RaycastArgs a;
  if (!host_raycast_args(a, mean.data(), cnt.data(), gsum.data(), depth.data(), normal.data(), grey.data(), g, W, H, N, &par[4])) return 2;
  launch({(unsigned)((W + 15) / 16), (unsigned)((H + 15) / 16), 1}, [&] { ekf::k_tsdf_raycast(a); });

  size_t hits = 0;
  for (float d : depth) hits += d > 0.f;
  const int bad = differs("mean", mean, w_mean) + differs("depth", depth, w_depth) + differs("normal", normal, w_normal) +
                  differs("grey", grey, w_grey);
  std::printf("%s: %d x %d x %d, view %d x %d, %d samples, min_count %d, %zu hits: %s\n", path, g.nx, g.ny, g.nz, W, H, N, min_count,
              hits, bad ? "DIFFERS" : "equal");
  return bad ? 1 : 0;
}
