// The four kernels of csrc/ekf_mesh_texture.hpp run on the host by host_kernels.hpp, which says how to
// build and run this: the 256 lanes of a workgroup are 256 real threads.  It reads the case files tools/texture_host_check.py
// writes (a mesh, its views and the oracle's result), makes the launches of TsdfTexture::begin, add_view and finish into buffers
// of exactly the device's sizes and compares bit for bit.
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

#include "../ekf-monoslam_for_3d-reconstruction_amd/csrc/ekf_mesh_texture.hpp"

static int run(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::perror(path); return 2; }
  const auto hdr = take<int>(f, 6);                                           // n_vert n_tri has_bgr P C n_views
  const size_t nv = (size_t)hdr[0], nt = (size_t)hdr[1];
  const bool has_bgr = hdr[2] != 0;
  const int P = hdr[3], C = hdr[4];
  const auto xyz = take<double>(f, nv * 3);
  const auto faces = take<unsigned>(f, nt * 3);
  const auto grey = take<unsigned char>(f, nv);
  const auto bgr = take<unsigned char>(f, has_bgr ? nv * 3 : 0);

  // TsdfTexture::begin's buffers, cleared as it clears them
  int B;
  long long Q, A;
  ekf::tex_layout(nt, P, B, Q, A);
  const size_t na = (size_t)A * (size_t)A * (size_t)C;
  std::vector<unsigned char> atlas(na, 0), won(nt, 0), vis(nv, 0xee);
  std::vector<double> best_score(nt, 0.0), sxy(nv * 2, -7.0);
  std::vector<int> best_view(nt, -1);
  unsigned counts[2] = {0xdeadbeefu, 0xdeadbeefu};
  ekf::TexArgs a{};
  a.xyz = xyz.data(); a.faces = faces.data(); a.grey = grey.data(); a.bgr = (has_bgr && C == 3) ? bgr.data() : nullptr;
  a.n_vert = (unsigned)nv; a.n_tri = (unsigned)nt;
  a.P = P; a.B = B; a.Q = (int)Q; a.A = (int)A; a.C = C;
  const unsigned long long n_sq = (nt + 1) >> 1, rows = (n_sq + (unsigned long long)Q - 1) / (unsigned long long)Q;
  a.n_texel = (unsigned)(rows * (unsigned long long)B * (unsigned long long)A);
  a.atlas = atlas.data(); a.best_score = best_score.data(); a.best_view = best_view.data(); a.won = won.data();
  a.sxy = sxy.data(); a.vis = vis.data(); a.counts = counts;
  const unsigned vblk = (unsigned)((nv + 255) / 256), tblk = (unsigned)((nt + 255) / 256), ablk = (a.n_texel + 255u) / 256u;
  int bad = 0, fills = 0;
  unsigned long long n_textured = 0;

  for (int n = 0; n < hdr[5]; ++n) {
    const auto vh = take<int>(f, 5);                                          // W H vch has_zbuf n_won
    const auto cam = take<double>(f, 13);                                     // K[4] pose7 tol min_area2
    const size_t npix = (size_t)vh[0] * (size_t)vh[1];
    const auto img = take<unsigned char>(f, npix * (size_t)vh[2]);
    const auto zbuf = take<float>(f, vh[3] ? npix : 0);
    a.img = img.data(); a.vch = vh[2]; a.W = vh[0]; a.H = vh[1]; a.view = n; a.zbuf = vh[3] ? zbuf.data() : nullptr;
    a.fx = cam[0]; a.fy = cam[1]; a.cx = cam[2]; a.cy = cam[3]; a.tol = cam[11]; a.min_area2 = cam[12];
    double q[4];
    if (!ekf::dense_pose(cam.data() + 4, a.t, a.R, q)) { std::printf("  view %d: no pose\n", n); ++bad; continue; }
    counts[0] = counts[1] = 0u;                                               // the hipMemsetAsync
    launch({vblk, 1, 1}, [&] { ekf::k_tex_project(a); });
    launch({tblk, 1, 1}, [&] { ekf::k_tex_select(a); });
    n_textured += counts[1];
    if (counts[0] > 0) {
      launch({ablk, 1, 1}, [&] { ekf::k_tex_fill(a); });
      ++fills;
    }
    if ((int)counts[0] != vh[4]) { std::printf("  view %d won %u triangles, not %d\n", n, counts[0], vh[4]); ++bad; }
  }
  launch({ablk, 1, 1}, [&] { ekf::k_tex_fallback(a); });

  const auto w_atlas = take<unsigned char>(f, na);
  const auto w_view = take<int>(f, nt);
  const auto w_score = take<double>(f, nt);
  const auto w_uv = take<double>(f, nt * 6);
  const auto w_textured = take<int>(f, 1);
  std::fclose(f);
  std::vector<double> uv(nt * 6);
  for (size_t t = 0; t < nt; ++t) ekf::tex_uv(t, P, B, Q, A, uv.data() + 6 * t);
  bad += differs("atlas", atlas, w_atlas) + differs("view", best_view, w_view) + differs("score", best_score, w_score) + differs("uv", uv, w_uv);
  if ((int)n_textured != w_textured[0]) { std::printf("  %llu triangles textured, not %d\n", n_textured, w_textured[0]); ++bad; }
  std::printf("%s: %zu vertices, %zu triangles, atlas %lld x %d, %d views, %d fills, %llu textured: %s\n", path, nv, nt, A, C, hdr[5], fills,
              n_textured, bad ? "DIFFERS" : "equal");
  return bad ? 1 : 0;
}
