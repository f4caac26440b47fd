// The kernels of csrc/ekf_mesh_distance.hpp run on the host by host_kernels.hpp, which says how to build
// and run this: the 256 lanes of a workgroup are 256 real threads, so the adds of the cell counts and the cursors meet real
// concurrency.  It reads the case files tools/distance_host_check.py writes (a target mesh, query points and the oracle's result
// and statistics), makes the launches of TsdfDistance::run and ::stats into buffers of exactly the device's sizes at g = 1, 5 and
// automatic, and compares bit for bit each time.
#include "host_kernels.hpp"

// the atomics, with the compiler's (the forest's accessors too: ekf_union_find.hpp is on the way in)
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
#define EKF_RASTER_HOST_ATOMICS
static inline void rast_key_min(unsigned long long* p, unsigned long long v) {
  unsigned long long old = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (old > v && !__atomic_compare_exchange_n(p, &old, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
}

#include "host_tsdf.hpp"

#include "../ekf-monoslam_for_3d-reconstruction_amd/csrc/ekf_mesh_distance.hpp"

static int run(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::perror(path); return 2; }
  const auto hdr = take<unsigned>(f, 3);                                      // n_vert n_tri n_pts
  const size_t nv = hdr[0], nt = hdr[1], np = hdr[2];
  const auto xyz = take<double>(f, nv * 3);
  const auto faces = take<unsigned>(f, nt * 3);
  const auto pts = take<double>(f, np * 3);
  const auto w_dist = take<double>(f, np);
  const auto w_tri = take<unsigned>(f, np);
  const auto w_closest = take<double>(f, np * 3);
  const auto w_side = take<signed char>(f, np);
  const auto w_real = take<double>(f, 4);                                     // thr, sum, sum2, max
  const auto w_int = take<unsigned>(f, 3);                                    // argmax, within, bad
  std::fclose(f);

  int bad = 0;
  unsigned cells[3] = {0, 0, 0};
  unsigned long long entries[3] = {0, 0, 0};
  const unsigned gs[3] = {1u, 5u, 0u};
  const unsigned tblk = (unsigned)((nt + 255) / 256), pblk = (unsigned)((np + 255) / 256);
  for (int l = 0; l < 3; ++l) {
    // TsdfDistance::run's buffers, of exactly its sizes, filled with what a launch must overwrite
    std::vector<double> part((size_t)tblk * 6, -7.0), head(7, -7.0);
    std::vector<unsigned> part_n(tblk, 0xdeadbeefu);
    ekf::DistArgs a{};
    a.xyz = xyz.data(); a.faces = faces.data(); a.n_tri = (unsigned)nt; a.tblk = tblk;
    a.pts = pts.data(); a.n_pts = (unsigned)np; a.pblk = pblk;
    a.part = part.data(); a.part_n = part_n.data(); a.head = head.data();
    launch({tblk, 1, 1}, [&] { ekf::k_dist_box(a); });
    launch({1, 1, 1}, [&] { ekf::k_dist_grid(a); });
    if (!(head[6] >= 1.0)) { std::printf("  no valid triangle\n"); return 1; }
    a.g = ekf::dist_make_grid(head.data(), gs[l] ? gs[l] : ekf::dist_auto_g(head[6]));
    a.ncell = (unsigned)a.g.G[0] * (unsigned)a.g.G[1] * (unsigned)a.g.G[2];
    const unsigned cblk = (a.ncell + 255) / 256;
    std::vector<unsigned> cnt(a.ncell, 0u), cur(a.ncell, 0u), pre(a.ncell, 0xdeadbeefu), tot(cblk, 0xdeadbeefu);   // (the two memsets)
    std::vector<unsigned long long> off((size_t)cblk + 1, ~0ull);
    a.cnt = cnt.data(); a.cur = cur.data(); a.pre = pre.data(); a.tot = tot.data(); a.off = off.data();
    launch({tblk, 1, 1}, [&] { ekf::k_dist_count(a); });
    launch({cblk, 1, 1}, [&] { ekf::k_dist_offsets(a); });
    launch({1, 1, 1}, [&] { ekf::k_tsdf_scan(tot.data(), off.data(), cblk); });
    const unsigned long long total = off[cblk];
    std::vector<unsigned> list((size_t)total, 0xdeadbeefu);
    std::vector<double> dist(np, -7.0), closest(np * 3, -7.0), s_part((size_t)pblk * 3, -7.0);
    std::vector<unsigned> tri(np, 0x5a5a5a5au), s_ipart((size_t)pblk * 3, 0x5a5a5a5au);
    std::vector<signed char> side(np, 0x5a);
    ekf::DistSums sums;
    std::memset(&sums, 0xee, sizeof sums);
    a.list = list.data(); a.dist = dist.data(); a.tri = tri.data(); a.closest = closest.data(); a.side = side.data();
    launch({tblk, 1, 1}, [&] { ekf::k_dist_fill(a); });
    for (unsigned c = 0; c < a.ncell; ++c)
      if (cur[c] != cnt[c]) { std::printf("  g %u: the cursor of cell %u is %u of %u\n", gs[l], c, cur[c], cnt[c]); ++bad; break; }
    for (unsigned t : list)
      if (t >= nt) { std::printf("  g %u: a list entry was not written\n", gs[l]); ++bad; break; }
    launch({pblk, 1, 1}, [&] { ekf::k_dist_query(a); });
    a.thr = w_real[0]; a.s_part = s_part.data(); a.s_ipart = s_ipart.data(); a.sums = &sums;
    launch({pblk, 1, 1}, [&] { ekf::k_dist_stats(a); });
    launch({1, 1, 1}, [&] { ekf::k_dist_reduce(a); });
    cells[l] = a.ncell; entries[l] = total;
    const std::vector<double> g_real = {w_real[0], sums.sum, sums.sum2, sums.max};
    const std::vector<unsigned> g_int = {sums.argmax, sums.within, sums.bad};
    bad += differs("dist", dist, w_dist) + differs("tri", tri, w_tri) + differs("closest", closest, w_closest) + differs("side", side, w_side) +
           differs("sums", g_real, w_real) + differs("counts", g_int, w_int);
  }
  std::printf("%s: %zu triangles, %zu points, cells %u %u %u, entries %llu %llu %llu: %s\n", path, nt, np, cells[0], cells[1], cells[2], entries[0],
              entries[1], entries[2], bad ? "DIFFERS" : "equal");
  return bad ? 1 : 0;
}
