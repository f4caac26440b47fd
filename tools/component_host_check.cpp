// The seven kernels of csrc/ekf_mesh_components.hpp (and k_tsdf_scan between them) run on the host by
// host_kernels.hpp, which says how to build and run this: the 256 lanes of a workgroup are 256 real threads, so the unions of
// a workgroup of k_comp_union run concurrently (the workgroups follow one another).  It reads the case files
// tools/component_host_check.py writes (a welded mesh in buffers of exactly the device's sizes, and the oracle's labels, sizes
// and pruned meshes), makes the launches of TsdfComponents::components and ::prune and compares bit for bit.
#include "host_kernels.hpp"

// the accessors of the forest and of the counters, with the compiler's atomics
#define EKF_SPECKLE_HOST_ATOMICS
// (fetch_min and fetch_max as compare-and-swap loops: not every host compiler has the builtins)
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

#include "../ekf-monoslam_for_3d-reconstruction_amd/csrc/ekf_mesh_components.hpp"

struct Rows {
  std::vector<double> xyz;
  std::vector<unsigned long long> key;
  std::vector<unsigned char> grey, bgr;
  std::vector<float> normal;
  std::vector<unsigned> faces;
  Rows(size_t nv, size_t nt, bool colour) : xyz(nv * 3), key(nv), grey(nv), bgr(colour ? nv * 3 : 0), normal(nv * 3), faces(nt * 3) {}
};

static Rows take_rows(FILE* f, size_t nv, size_t nt, bool colour) {
  Rows r(0, 0, false);
  r.xyz = take<double>(f, nv * 3);
  r.key = take<unsigned long long>(f, nv);
  r.grey = take<unsigned char>(f, nv);
  r.bgr = take<unsigned char>(f, colour ? nv * 3 : 0);
  r.normal = take<float>(f, nv * 3);
  r.faces = take<unsigned>(f, nt * 3);
  return r;
}

static int run(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::perror(path); return 2; }
  const auto hdr = take<int>(f, 4);
  const size_t nv = (size_t)hdr[0], nt = (size_t)hdr[1];
  const bool colour = hdr[2] != 0;
  const Rows weld = take_rows(f, nv, nt, colour);
  const auto w_label = take<unsigned>(f, nv);
  const auto w_size = take<unsigned>(f, nv);
  const auto w_count = take<unsigned long long>(f, 1);

  // TsdfComponents::components's buffers and launches
  const unsigned vblk = (unsigned)((nv + 255) / 256), tblk = (unsigned)((nt + 255) / 256);
  const size_t P = (size_t)std::max(vblk, tblk) + 1;
  std::vector<unsigned> L(nv, 0xdeadbeefu), R(nv, 0xdeadbeefu), S(nv, 0xdeadbeefu), V(nv, 0xdeadbeefu), T(nt, 0xdeadbeefu);
  std::vector<unsigned> tot((size_t)vblk * 2 + tblk, 0xdeadbeefu), n_roots(1, 0xdeadbeefu);
  std::vector<unsigned long long> off(3 * P, 0xdeadbeefull), best(1, 0xdeadbeefull);
  ekf::CompArgs a{};
  a.faces = weld.faces.data();
  a.L = L.data(); a.R = R.data(); a.S = S.data(); a.V = V.data(); a.T = T.data(); a.blk_tot = tot.data();
  a.best = best.data(); a.n_roots = n_roots.data();
  a.n_vert = (unsigned)nv; a.vblk = vblk; a.n_tri = nt;
  a.off_v = off.data() + (P - 1 - vblk);
  a.off_t = off.data() + P + (P - 1 - tblk);
  unsigned long long* off_r = off.data() + 2 * P + (P - 1 - vblk);
  a.min_triangles = 1; a.largest = 0;
  a.xyz = weld.xyz.data(); a.key = weld.key.data(); a.grey = weld.grey.data();
  a.bgr = colour ? weld.bgr.data() : nullptr;
  a.normal = weld.normal.data();
  unsigned long long n_comp = 0;
  if (nt) {
    launch({vblk, 1, 1}, [&] { ekf::k_comp_init(a); });
    launch({tblk, 1, 1}, [&] { ekf::k_comp_union(a); });
    launch({vblk + tblk, 1, 1}, [&] { ekf::k_comp_count(a); });
    launch({vblk + tblk, 1, 1}, [&] { ekf::k_comp_flags(a); });
    n_comp = n_roots[0];
  }
  int bad = differs("label", R, w_label) + differs("size", L, w_size) + (n_comp != w_count[0]);

  // TsdfComponents::prune's, once per prune of the case
  for (int p = 0; p < hdr[3]; ++p) {
    const auto par = take<unsigned>(f, 2);
    const auto n = take<unsigned long long>(f, 3);
    const Rows want = take_rows(f, (size_t)n[0], (size_t)n[1], colour);
    unsigned long long totals[3] = {0, 0, 0};
    Rows got(0, 0, false);
    if (nt) {
      a.min_triangles = par[0];
      a.largest = (int)par[1];
      if (a.largest) launch({vblk, 1, 1}, [&] { ekf::k_comp_largest(a); });
      launch({vblk + tblk, 1, 1}, [&] { ekf::k_comp_flags(a); });
      launch({1, 1, 1}, [&] { ekf::k_tsdf_scan(tot.data(), (unsigned long long*)a.off_v, vblk); });
      launch({1, 1, 1}, [&] { ekf::k_tsdf_scan(tot.data() + vblk, (unsigned long long*)a.off_t, tblk); });
      launch({1, 1, 1}, [&] { ekf::k_tsdf_scan(tot.data() + vblk + tblk, off_r, vblk); });
      for (int i = 0; i < 3; ++i) totals[i] = off[(size_t)i * P + P - 1];
      got = Rows((size_t)totals[0], (size_t)totals[1], colour);
      a.p_xyz = got.xyz.data(); a.p_key = got.key.data(); a.p_grey = got.grey.data(); a.p_bgr = got.bgr.data();
      a.p_normal = got.normal.data(); a.p_faces = got.faces.data();
      if (totals[0]) launch({vblk, 1, 1}, [&] { ekf::k_comp_vertices(a); });
      if (totals[1]) launch({tblk, 1, 1}, [&] { ekf::k_comp_faces(a); });
    }
    const int d = (totals[0] != n[0]) + (totals[1] != n[1]) + (totals[2] != n[2]) + differs("xyz", got.xyz, want.xyz) +
                  differs("key", got.key, want.key) + differs("grey", got.grey, want.grey) + differs("bgr", got.bgr, want.bgr) +
                  differs("normal", got.normal, want.normal) + differs("faces", got.faces, want.faces) +
                  differs("size after the prune", L, w_size) + differs("label after the prune", R, w_label);
    if (d) std::printf("  prune(%u, %u): %llu vertices, %llu triangles, %llu kept (oracle %llu, %llu, %llu)\n", par[0], par[1],
                       totals[0], totals[1], totals[2], n[0], n[1], n[2]);
    bad += d;
  }
  std::fclose(f);
  std::printf("%s: %zu vertices, %zu triangles, %s, %llu components, %d prunes: %s\n", path, nv, nt, colour ? "colour" : "grey",
              n_comp, hdr[3], bad ? "DIFFERS" : "equal");
  return bad ? 1 : 0;
}
