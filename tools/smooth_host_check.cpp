// The six kernels of csrc/ekf_mesh_smooth.hpp (and k_tsdf_scan between them) run on the host by
// host_kernels.hpp, which says how to build and run this: the 256 lanes of a workgroup are 256 real threads, so the corners of
// a workgroup of k_smooth_fill reach their cursors in an order that differs from run to run (the workgroups follow one
// another).  It reads the case files tools/smooth_host_check.py writes (a mesh in buffers of exactly the device's sizes, and the
// oracle's adjacency, positions and normals of several runs), makes the launches of TsdfSmooth::adjacency and ::run and
// compares bit for bit.
#include "host_kernels.hpp"

// the counters, with the compiler's atomics (the forest's accessors too: ekf_union_find.hpp is on the way in)
#define EKF_SPECKLE_HOST_ATOMICS
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
static inline void comp_global_max(unsigned long long* p, unsigned long long v) {
  unsigned long long old = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (old < v && !__atomic_compare_exchange_n(p, &old, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
}

#include "host_tsdf.hpp"

#include "../ekf-monoslam_for_3d-reconstruction_amd/csrc/ekf_mesh_smooth.hpp"

static int run(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::perror(path); return 2; }
  const auto hdr = take<int>(f, 3);
  const size_t nv = (size_t)hdr[0], nt = (size_t)hdr[1];
  const auto xyz = take<double>(f, nv * 3);
  const auto faces = take<unsigned>(f, nt * 3);
  const auto w_inc = take<unsigned>(f, nv);
  const auto w_deg = take<unsigned>(f, nv);
  const auto w_boundary = take<unsigned char>(f, nv);

  // TsdfSmooth::adjacency's buffers and launches
  const unsigned vblk = (unsigned)((nv + 255) / 256), tblk = (unsigned)((nt + 255) / 256);
  std::vector<unsigned> inc(nv, 0xdeadbeefu), pre(nv, 0xdeadbeefu), deg(nv, 0xdeadbeefu), tot(vblk, 0xdeadbeefu);
  std::vector<unsigned> tri(nt * 3, 0xdeadbeefu), nbr(nt * 6, 0xdeadbeefu);
  std::vector<unsigned char> boundary(nv, 0xee);
  std::vector<unsigned long long> off((size_t)vblk + 1, 0xdeadbeefull);
  ekf::SmoothArgs a{};
  a.faces = faces.data();
  a.inc = inc.data(); a.pre = pre.data(); a.deg = deg.data(); a.boundary = boundary.data(); a.blk_tot = tot.data();
  a.off = off.data(); a.tri = tri.data(); a.nbr = nbr.data();
  a.n_vert = (unsigned)nv; a.n_tri = nt;
  if (nt) {
    std::fill(inc.begin(), inc.end(), 0u);                                    // the hipMemsetAsync
    launch({tblk, 1, 1}, [&] { ekf::k_smooth_count(a); });
    launch({vblk, 1, 1}, [&] { ekf::k_smooth_offsets(a); });
    launch({1, 1, 1}, [&] { ekf::k_tsdf_scan(tot.data(), off.data(), vblk); });
    launch({tblk, 1, 1}, [&] { ekf::k_smooth_fill(a); });
    launch({vblk, 1, 1}, [&] { ekf::k_smooth_lists(a); });
  }
  int bad = differs("inc", inc, w_inc) + differs("deg", deg, w_deg) + differs("boundary", boundary, w_boundary);
  if (nt && off[vblk] != 3ull * nt) { std::printf("  the lists hold %llu entries, not %zu\n", off[vblk], 3 * nt); ++bad; }

  // TsdfSmooth::run's, once per run of the case
  for (int r = 0; r < hdr[2]; ++r) {
    const auto par = take<int>(f, 3);                                         // iterations, pin_boundary, normals
    const auto fac = take<double>(f, 2);                                      // lambda, mu
    const auto want = take<double>(f, nv * 3);
    const auto want_n = take<float>(f, par[2] ? nv * 3 : 0);
    const int steps = fac[1] != 0.0 ? 2 * par[0] : par[0];
    std::vector<double> pos[2] = {std::vector<double>(nv * 3, -7.0), std::vector<double>(steps > 1 ? nv * 3 : 0, -7.0)};
    std::vector<float> normal(par[2] ? nv * 3 : 0, -7.f);
    int last = 0;
    if (nt) {
      a.pin = par[1];
      for (int k = 0; k < steps; ++k) {
        a.src = k == 0 ? xyz.data() : pos[(k - 1) & 1].data();
        a.dst = pos[k & 1].data();
        a.f = (fac[1] != 0.0 && (k & 1)) ? fac[1] : fac[0];
        launch({vblk, 1, 1}, [&] { ekf::k_smooth_step(a); });
      }
      last = (steps - 1) & 1;
      if (par[2]) {
        a.src = pos[last].data();
        a.normal = normal.data();
        launch({vblk, 1, 1}, [&] { ekf::k_smooth_normals(a); });
      }
    }
    const int d = differs("xyz", pos[last], want) + differs("normal", normal, want_n) + differs("inc after the run", inc, w_inc) +
                  differs("deg after the run", deg, w_deg);
    if (d) std::printf("  run(iterations %d, pin %d, normals %d, lambda %g, mu %g)\n", par[0], par[1], par[2], fac[0], fac[1]);
    bad += d;
  }
  std::fclose(f);
  unsigned most = 0;
  for (unsigned x : inc) most = std::max(most, x);
  std::printf("%s: %zu vertices, %zu triangles, longest list %u, %d runs: %s\n", path, nv, nt, most, hdr[2], bad ? "DIFFERS" : "equal");
  return bad ? 1 : 0;
}
