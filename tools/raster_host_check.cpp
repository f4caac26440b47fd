// The four kernels of csrc/ekf_mesh_raster.hpp run on the host by host_kernels.hpp, which says how to
// build and run this: the 256 lanes of a workgroup are 256 real threads, so the minimum of the keys, the adds of the cover image
// and the cursor of the deferred list meet real concurrency.  It reads the case files tools/raster_host_check.py writes (a mesh,
// a view, perhaps an atlas, and the oracle's images), makes the launches of TsdfRaster::render into buffers of exactly the
// device's sizes at small_limit 0, 64 and 65536, and compares bit for bit each time.
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

#include "../ekf-monoslam_for_3d-reconstruction_amd/csrc/ekf_mesh_raster.hpp"

static int run(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::perror(path); return 2; }
  const auto hdr = take<int>(f, 11);                                          // n_vert n_tri has_bgr W H cull shading P C A colour
  const size_t nv = (size_t)hdr[0], nt = (size_t)hdr[1];
  const bool has_bgr = hdr[2] != 0, shading = hdr[6] != 0, colour = hdr[10] != 0;
  const int W = hdr[3], H = hdr[4], P = hdr[7], C = hdr[8], A = hdr[9];
  const size_t npix = (size_t)W * (size_t)H;
  const auto cam = take<double>(f, 12);                                       // K[4] pose7 z_near
  const auto xyz = take<double>(f, nv * 3);
  const auto faces = take<unsigned>(f, nt * 3);
  const auto grey = take<unsigned char>(f, nv);
  const auto bgr = take<unsigned char>(f, has_bgr ? nv * 3 : 0);
  const auto atlas = take<unsigned char>(f, shading ? (size_t)A * (size_t)A * (size_t)C : 0);
  const auto w_depth = take<float>(f, npix);
  const auto w_normal = take<float>(f, npix * 3);
  const auto w_grey = take<unsigned char>(f, npix);
  const auto w_bgr = take<unsigned char>(f, colour ? npix * 3 : 0);
  const auto w_tri = take<int>(f, npix);
  const auto w_bary = take<float>(f, npix * 2);
  const auto w_cover = take<unsigned>(f, npix);
  std::fclose(f);

  int bad = 0;
  unsigned deferred[3] = {0, 0, 0};
  const unsigned limits[3] = {0u, 64u, 65536u};
  for (int l = 0; l < 3; ++l) {
    // TsdfRaster::render's buffers, of exactly its sizes, filled with what a launch must overwrite
    std::vector<unsigned long long> keys(npix, 0x1234567812345678ull);
    std::vector<float> depth(npix, -7.f), normal(npix * 3, -7.f), bary(npix * 2, -7.f);
    std::vector<int> tri(npix, 0x5a5a5a5a);
    std::vector<unsigned char> out_grey(npix, 0xee), out_bgr(colour ? npix * 3 : 0, 0xee), usable(nv, 0xee);
    std::vector<unsigned> cover(npix, 0xdeadbeefu), list(nt, 0xdeadbeefu);
    std::vector<double> proj(nv * 3, -7.0);
    unsigned cursor = 0xdeadbeefu;
    ekf::RastArgs a{};
    a.xyz = xyz.data(); a.faces = faces.data(); a.grey = grey.data(); a.bgr = has_bgr ? bgr.data() : nullptr;
    a.n_vert = (unsigned)nv; a.n_tri = (unsigned)nt;
    a.W = W; a.H = H; a.z_near = cam[11]; a.cull = hdr[5]; a.shading = shading ? 1 : 0; a.want_cover = 1;
    a.small_limit = limits[l]; a.large_grid = (unsigned)std::min<size_t>(nt, ekf::kRastLargeGrid);
    a.fx = cam[0]; a.fy = cam[1]; a.cx = cam[2]; a.cy = cam[3];
    double q[4];
    if (!ekf::dense_pose(cam.data() + 4, a.t, a.R, q)) { std::printf("  no pose\n"); return 1; }
    a.proj = proj.data(); a.usable = usable.data(); a.list = list.data(); a.cursor = &cursor; a.keys = keys.data(); a.cover = cover.data();
    a.depth = depth.data(); a.normal = normal.data(); a.bary = bary.data(); a.tri = tri.data(); a.out_grey = out_grey.data();
    a.out_bgr = colour ? out_bgr.data() : nullptr;
    if (shading) { a.atlas = atlas.data(); a.P = P; a.B = P + 2; a.Q = A / (P + 2); a.A = A; a.C = C; }
    std::memset(keys.data(), 0xff, npix * sizeof(unsigned long long));        // the three hipMemsetAsync
    std::memset(cover.data(), 0, npix * sizeof(unsigned));
    cursor = 0u;
    launch({(unsigned)((nv + 255) / 256), 1, 1}, [&] { ekf::k_rast_project(a); });
    launch({(unsigned)((nt + 255) / 256), 1, 1}, [&] { ekf::k_rast_small(a); });
    if ((size_t)limits[l] < npix) launch({a.large_grid, 1, 1}, [&] { ekf::k_rast_large(a); });
    launch({(unsigned)((W + 15) / 16), (unsigned)((H + 15) / 16), 1}, [&] { ekf::k_rast_resolve(a); });
    deferred[l] = cursor;
    if (cursor > nt) { std::printf("  limit %u: the cursor is %u of %zu triangles\n", limits[l], cursor, nt); ++bad; }
    bad += differs("depth", depth, w_depth) + differs("normal", normal, w_normal) + differs("grey", out_grey, w_grey) +
           differs("bgr", out_bgr, w_bgr) + differs("tri", tri, w_tri) + differs("bary", bary, w_bary) + differs("cover", cover, w_cover);
  }
  size_t hit = 0;
  for (int t : w_tri) hit += t >= 0;
  std::printf("%s: %zu vertices, %zu triangles, %d x %d, %zu hit, deferred %u %u %u: %s\n", path, nv, nt, W, H, hit, deferred[0], deferred[1],
              deferred[2], bad ? "DIFFERS" : "equal");
  return bad ? 1 : 0;
}
