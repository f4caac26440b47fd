// The four kernels of the speckle filter (csrc/ekf_dense_speckle.hpp: k_speckle_label, k_speckle_merge, k_speckle_count,
// k_speckle_apply) run on the host by host_kernels.hpp, which says how to build and run this: the 256
// lanes of a workgroup are 256 real threads, so the union-find of a tile in LDS and the unions of a workgroup of
// k_speckle_merge run concurrently (the workgroups follow one another).  It reads the case files tools/speckle_host_check.py
// writes (the maps in buffers of exactly the device's sizes, and the oracle's outputs), makes the launches of
// DenseSpeckle::run and compares label, size, depth and plane bit for bit.
#include "host_kernels.hpp"

// the header's accessors of the forest and of the LDS counters, with the compiler's atomics
#define EKF_SPECKLE_HOST_ATOMICS
// (fetch_min as a compare-and-swap loop: not every host compiler has the builtin)
static inline unsigned seg_global_load(const unsigned* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
static inline unsigned seg_global_min(unsigned* p, unsigned v) {
  unsigned old = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (old > v && !__atomic_compare_exchange_n(p, &old, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
  return old;
}
static inline unsigned seg_global_add(unsigned* p, unsigned v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
static inline unsigned seg_lds_load(const unsigned* p) { return seg_global_load(p); }
static inline unsigned seg_lds_min(unsigned* p, unsigned v) { return seg_global_min(p, v); }
static inline unsigned seg_lds_add(unsigned* p, unsigned v) { return seg_global_add(p, v); }

#include "../ekf-monoslam_for_3d-reconstruction_amd/csrc/ekf_dense_speckle.hpp"

// a case: ints W H min_size max_diff; the depth and the plane map; then the oracle's depth, plane, label and size.
static int run(const char* path_) {
  FILE* f = std::fopen(path_, "rb");
  if (!f) { std::perror(path_); return 2; }
  const auto hdr = take<int>(f, 4);
  const int W = hdr[0], H = hdr[1], min_size = hdr[2], max_diff = hdr[3];
  const size_t n = (size_t)W * H;
  auto depth = take<float>(f, n);
  auto plane = take<int>(f, n);
  const auto w_depth = take<float>(f, n);
  const auto w_plane = take<int>(f, n);
  const auto w_label = take<unsigned>(f, n);
  const auto w_size = take<unsigned>(f, n);
  std::fclose(f);
  std::vector<unsigned> L(n, 0xdeadbeefu), R(n, 0xdeadbeefu), S(n, 0xdeadbeefu);
  const ekf::SpeckleArgs a{depth.data(), plane.data(), L.data(), R.data(), S.data(), W, H, min_size, max_diff};
  // DenseSpeckle::run's grids
  const Idx3 tiles{(unsigned)((W + ekf::kDenseTW - 1) / ekf::kDenseTW), (unsigned)((H + ekf::kDenseTH - 1) / ekf::kDenseTH), 1};
  const size_t border = (size_t)((W - 1) / ekf::kDenseTW) * H + (size_t)((H - 1) / ekf::kDenseTH) * W;
  const unsigned wg_m = (unsigned)std::max<size_t>(1, (border + 255) / 256), wg_n = (unsigned)((n + 255) / 256);
  launch(tiles, [&] { ekf::k_speckle_label(a); });
  launch({wg_m, 1, 1}, [&] { ekf::k_speckle_merge(a); });
  launch(tiles, [&] { ekf::k_speckle_count(a); });
  launch({wg_n, 1, 1}, [&] { ekf::k_speckle_apply(a); });
  const int bad = differs("label", R, w_label) + differs("size", L, w_size) + differs("depth", depth, w_depth) +
                  differs("plane", plane, w_plane);
  size_t kept = 0, roots = 0;
  for (size_t i = 0; i < n; ++i) { kept += plane[i] >= 0; roots += R[i] == (unsigned)i; }
  std::printf("%s: %d x %d, min_size %d, max_diff %d, %zu segments, %zu kept, %zu border links examined: %s\n", path_, W, H, min_size,
              max_diff, roots, kept, border, bad ? "DIFFERS" : "equal");
  return bad ? 1 : 0;
}
