// The two kernels of csrc/ekf_dense_stereo.hpp run lane by lane on the host by host_kernels.hpp,
// which says how to build and run this.  It reads the case files tools/dense_host_check.py writes (inputs in buffers of
// exactly the device's sizes, and the numpy oracle's outputs), makes the library's launches of a pixel-wise sweep
// (ekf::sweep_launches, csrc/ekf_dense_sgm.hpp) and of the filter, and compares bit for bit.
#include "host_kernels.hpp"

#include "../ekf-monoslam_for_3d-reconstruction_amd/csrc/ekf_dense_sgm.hpp"

// case file: ints W H D radius trunc n_src min_agree; doubles w_min w_max rel_tol; per view (0 = reference, then the
// sources) 4 + 7 doubles (K, pose) and W H bytes; the sources' swept depths; then the oracle: depth plane cost views of the
// sweep, filtered depth and plane, points of the swept and of the filtered map.
static int run(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::perror(path); return 2; }
  const auto hdr = take<int>(f, 7);
  const int W = hdr[0], H = hdr[1], D = hdr[2], radius = hdr[3], trunc = hdr[4], n_src = hdr[5], min_agree = hdr[6];
  const auto par = take<double>(f, 3);
  const size_t n = (size_t)W * H;
  std::vector<std::vector<double>> K, pose;
  std::vector<std::vector<unsigned char>> img;
  for (int v = 0; v <= n_src; ++v) {
    K.push_back(take<double>(f, 4));
    pose.push_back(take<double>(f, 7));
    img.push_back(take<unsigned char>(f, n));
  }
  std::vector<std::vector<float>> src_depth;
  for (int v = 0; v < n_src; ++v) src_depth.push_back(take<float>(f, n));
  const auto w_depth = take<float>(f, n);
  const auto w_plane = take<int>(f, n);
  const auto w_cost = take<unsigned>(f, n);
  const auto w_views = take<unsigned char>(f, n);
  const auto w_fdepth = take<float>(f, n);
  const auto w_fplane = take<int>(f, n);
  const auto w_pts = take<double>(f, 3 * n);
  const auto w_fpts = take<double>(f, 3 * n);
  std::fclose(f);

  // K, t and R of every view, as the library holds them
  std::vector<double> t(3 * (n_src + 1)), R(9 * (n_src + 1));
  std::vector<ekf::DenseCam> cam;
  for (int v = 0; v <= n_src; ++v) {
    double q[4];
    if (!ekf::dense_pose(pose[v].data(), &t[3 * v], &R[9 * v], q)) return 2;
    cam.push_back({K[v].data(), &t[3 * v], &R[9 * v]});
  }

  std::vector<float> depth(n), fdepth(n);
  std::vector<int> plane(n), fplane(n);
  std::vector<unsigned> cost(n);
  std::vector<unsigned char> views(n);
  std::vector<double> pts(3 * n), fpts(3 * n);
  ekf::SweepArgs a = ekf::sweep_args(cam.data(), n_src, W, H, D, radius, trunc, par[0], par[1]);
  a.ref = img[0].data(); a.depth = depth.data(); a.plane = plane.data(); a.cost = cost.data(); a.views = views.data();
  for (int v = 1; v <= n_src; ++v) a.s[v - 1].img = img[v].data();
  ekf::sweep_launches(a, {}, nullptr, {false, 0, nullptr, 0, 0, 0}, HostGo{});

  ekf::FilterArgs fa{};
  fa.depth = depth.data(); fa.plane = plane.data(); fa.out_depth = fdepth.data(); fa.out_plane = fplane.data(); fa.xyz = nullptr;
  fa.W = W; fa.H = H; fa.n_src = n_src; fa.min_agree = min_agree; fa.rel_tol = par[2];
  fa.fx = K[0][0]; fa.fy = K[0][1]; fa.cx = K[0][2]; fa.cy = K[0][3];
  std::copy(&R[0], &R[9], fa.R);
  std::copy(&t[0], &t[3], fa.t);
  for (int v = 1; v <= n_src; ++v) {
    ekf::dense_relative(cam[0], cam[v], fa.s[v - 1]);
    fa.s[v - 1].depth = src_depth[v - 1].data();
  }
  const Idx3 grid1 = {(unsigned)((n + 255) / 256), 1, 1};
  launch(grid1, [&] { ekf::k_depth_filter_points(fa); });
  fa.n_src = 0; fa.out_depth = nullptr; fa.out_plane = nullptr;
  fa.xyz = pts.data();
  launch(grid1, [&] { ekf::k_depth_filter_points(fa); });
  fa.depth = fdepth.data(); fa.plane = fplane.data(); fa.xyz = fpts.data();
  launch(grid1, [&] { ekf::k_depth_filter_points(fa); });

  const int bad = differs("depth", depth, w_depth) + differs("plane", plane, w_plane) + differs("cost", cost, w_cost) +
                  differs("views", views, w_views) + differs("filtered depth", fdepth, w_fdepth) +
                  differs("filtered plane", fplane, w_fplane) + differs("points", pts, w_pts) + differs("filtered points", fpts, w_fpts);
  std::printf("%s: %d x %d, D %d, radius %d, trunc %d, %d sources: %s\n", path, W, H, D, radius, trunc, n_src, bad ? "DIFFERS" : "equal");
  return bad ? 1 : 0;
}
