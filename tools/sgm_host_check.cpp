// The kernels of csrc/ekf_dense_sgm.hpp run lane by lane on the host by host_kernels.hpp, which says
// how to build and run this and emulates the one cross-lane read of k_sgm_path.  It reads the case files
// tools/sgm_host_check.py writes (inputs in buffers of exactly the device's sizes, and the numpy oracle's outputs), makes
// the launches of DenseSgm::sweep by the launch plan it calls (ekf::sweep_launches: its grids and instantiations), and compares
// bit for bit.
#include "host_kernels.hpp"

#include "../ekf-monoslam_for_3d-reconstruction_amd/csrc/ekf_dense_sgm.hpp"

// case file: ints W H D radius trunc n_src p1 p2 paths; doubles w_min w_max; per view (0 = reference, then the sources)
// 4 + 7 doubles (K, pose) and W H bytes; then the oracle: C and S (D H W unsigned each), depth plane cost views.
static int run(const char* path_) {
  FILE* f = std::fopen(path_, "rb");
  if (!f) { std::perror(path_); return 2; }
  const auto hdr = take<int>(f, 9);
  const int W = hdr[0], H = hdr[1], D = hdr[2], radius = hdr[3], trunc = hdr[4], n_src = hdr[5], p1 = hdr[6], p2 = hdr[7], paths = hdr[8];
  const auto par = take<double>(f, 2);
  const size_t n = (size_t)W * H, elems = n * (size_t)D;
  std::vector<std::vector<double>> K, pose;
  std::vector<std::vector<unsigned char>> img;
  for (int v = 0; v <= n_src; ++v) {
    K.push_back(take<double>(f, 4));
    pose.push_back(take<double>(f, 7));
    img.push_back(take<unsigned char>(f, n));
  }
  const auto w_C = take<unsigned>(f, elems);
  const auto w_S = take<unsigned>(f, elems);
  const auto w_depth = take<float>(f, n);
  const auto w_plane = take<int>(f, n);
  const auto w_cost = take<unsigned>(f, n);
  const auto w_views = take<unsigned char>(f, n);
  std::fclose(f);

  // K, t and R of every view, as the library holds them
  std::vector<double> t(3 * (n_src + 1)), R(9 * (n_src + 1));
  std::vector<ekf::DenseCam> cam;
  for (int v = 0; v <= n_src; ++v) {
    double q[4];
    if (!ekf::dense_pose(pose[v].data(), &t[3 * v], &R[9 * v], q)) return 2;
    cam.push_back({K[v].data(), &t[3 * v], &R[9 * v]});
  }
  std::vector<float> depth(n);
  std::vector<int> plane(n);
  std::vector<unsigned> cost(n), C(elems), S(elems);
  std::vector<unsigned char> views(n), V(elems);
  ekf::SweepArgs a = ekf::sweep_args(cam.data(), n_src, W, H, D, radius, trunc, par[0], par[1]);
  a.ref = img[0].data(); a.depth = depth.data(); a.plane = plane.data(); a.cost = cost.data(); a.views = views.data();
  for (int v = 1; v <= n_src; ++v) a.s[v - 1].img = img[v].data();
  ekf::sweep_launches(a, {C.data(), V.data()}, S.data(), {false, 0, nullptr, paths, p1, p2}, HostGo{});

  std::vector<unsigned> planes(elems);                    // as ekf_dense_get_volume delivers a volume
  ekf::sgm_volume_to_planes(C.data(), planes.data(), n, D);
  const int raw_bad = differs("raw volume", planes, w_C);
  ekf::sgm_volume_to_planes(S.data(), planes.data(), n, D);
  const int bad = raw_bad + differs("aggregated volume", planes, w_S) + differs("depth", depth, w_depth) + differs("plane", plane, w_plane) +
                  differs("cost", cost, w_cost) + differs("views", views, w_views);
  std::printf("%s: %d x %d, D %d, radius %d, trunc %d, %d sources, p1 %d, p2 %d, %d paths: %s\n", path_, W, H, D, radius, trunc, n_src,
              p1, p2, paths, bad ? "DIFFERS" : "equal");
  return bad ? 1 : 0;
}
