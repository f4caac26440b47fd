// The kernels of the runner-up cost and the uniqueness test (csrc/ekf_dense_stereo.hpp: k_plane_sweep_unique,
// k_plane_sweep_census_unique, k_plane_sweep_best_unique, k_plane_sweep_best_census_unique, k_depth_filter_unique;
// csrc/ekf_dense_sgm.hpp: k_sgm_winner_unique behind the unchanged volume and path kernels) run lane by lane on the host
//  by host_kernels.hpp, which says how to build and run this.  It reads the case files
// tools/unique_host_check.py writes (inputs in buffers of exactly the device's sizes, and the numpy oracle's outputs), makes
// the launches of DenseSgm::sweep (by the launch plan it calls, ekf::sweep_launches) and DenseStereo::filter_points with the
// switch on, and compares bit for bit: the four existing maps and the runner-up of a sweep, the filtered depth and plane of a filter.
#include "host_kernels.hpp"

#include "../ekf-monoslam_for_3d-reconstruction_amd/csrc/ekf_dense_sgm.hpp"

// K, t and R of every view, as the library holds them (t and R live in tR: 12 doubles a view); false: not a pose
static bool cams(const std::vector<std::vector<double>>& K, const std::vector<std::vector<double>>& pose, std::vector<double>& tR,
                 std::vector<ekf::DenseCam>& cam) {
  tR.resize(12 * pose.size());
  for (size_t v = 0; v < pose.size(); ++v) {
    double q[4];
    if (!ekf::dense_pose(pose[v].data(), &tR[12 * v], &tR[12 * v + 3], q)) return false;
    cam.push_back({K[v].data(), &tR[12 * v], &tR[12 * v + 3]});
  }
  return true;
}

// a sweep case: ints W H D radius trunc n_src n_best census paths p1 p2; doubles w_min w_max; per view (0 = reference, then
// the sources) 4 + 7 doubles (K, pose) and W H bytes; then the oracle's depth plane cost views runner.
static int run_sweep(FILE* f, const char* path_) {
  const auto hdr = take<int>(f, 11);
  const int W = hdr[0], H = hdr[1], D = hdr[2], radius = hdr[3], trunc = hdr[4], n_src = hdr[5], n_best = hdr[6], census = hdr[7],
            paths = hdr[8], p1 = hdr[9], p2 = hdr[10];
  const auto par = take<double>(f, 2);
  const size_t n = (size_t)W * H, elems = paths ? n * (size_t)D : 0;
  std::vector<std::vector<double>> K, pose;
  std::vector<std::vector<unsigned char>> img;
  for (int v = 0; v <= n_src; ++v) {
    K.push_back(take<double>(f, 4));
    pose.push_back(take<double>(f, 7));
    img.push_back(take<unsigned char>(f, n));
  }
  const auto w_depth = take<float>(f, n);
  const auto w_plane = take<int>(f, n);
  const auto w_cost = take<unsigned>(f, n);
  const auto w_views = take<unsigned char>(f, n);
  const auto w_runner = take<unsigned>(f, n);

  const Idx3 tiles{(unsigned)((W + ekf::kDenseTW - 1) / ekf::kDenseTW), (unsigned)((H + ekf::kDenseTH - 1) / ekf::kDenseTH), 1};
  std::vector<std::vector<unsigned long long>> T;
  for (int v = 0; census && v <= n_src; ++v) {
    T.emplace_back(n);
    const ekf::CensusArgs c{img[v].data(), T[v].data(), W, H};
    launch(tiles, [&] { ekf::k_census(c); });
  }
  std::vector<double> tR;
  std::vector<ekf::DenseCam> cam;
  if (!cams(K, pose, tR, cam)) return 2;
  std::vector<float> depth(n);
  std::vector<int> plane(n);
  std::vector<unsigned> cost(n), runner(n), C(elems), S(elems);
  std::vector<unsigned char> views(n), V(elems);
  ekf::SweepArgs a = ekf::sweep_args(cam.data(), n_src, W, H, D, radius, trunc, par[0], par[1]);
  a.depth = depth.data(); a.plane = plane.data(); a.cost = cost.data(); a.views = views.data();
  if (census) {                                           // each cost gets its own inputs alone
    a.ref_census = T[0].data();
    for (int v = 1; v <= n_src; ++v) a.s[v - 1].census = T[v].data();
  } else {
    a.ref = img[0].data();
    for (int v = 1; v <= n_src; ++v) a.s[v - 1].img = img[v].data();
  }
  ekf::sweep_launches(a, {C.data(), V.data()}, S.data(), {census != 0, n_best, runner.data(), paths, p1, p2}, HostGo{});
  const int bad = differs("depth", depth, w_depth) + differs("plane", plane, w_plane) + differs("cost", cost, w_cost) +
                  differs("views", views, w_views) + differs("runner-up", runner, w_runner);
  size_t absent = 0;
  for (unsigned r : runner) absent += r == ekf::kRunnerAbsent;
  std::printf("%s: %d x %d, D %d, radius %d, trunc %d, %d sources, best %d, %s%s, %zu absent: %s\n", path_, W, H, D, radius, trunc,
              n_src, n_best, census ? "census" : "absolute differences", paths ? ", aggregated" : "", absent, bad ? "DIFFERS" : "equal");
  return bad ? 1 : 0;
}

// a filter case: ints W H n_src min_agree uniqueness; double rel_tol; per view (0 = reference, then the sources) 4 + 7 doubles
// (K, pose); the reference's swept depth, plane, cost and runner-up; per source its swept depth; then the oracle's filtered
// depth and plane.
static int run_filter(FILE* f, const char* path_) {
  const auto hdr = take<int>(f, 5);
  const int W = hdr[0], H = hdr[1], n_src = hdr[2], min_agree = hdr[3], u = hdr[4];
  const double rel_tol = take<double>(f, 1)[0];
  const size_t n = (size_t)W * H;
  std::vector<std::vector<double>> K, pose;
  for (int v = 0; v <= n_src; ++v) {
    K.push_back(take<double>(f, 4));
    pose.push_back(take<double>(f, 7));
  }
  const auto depth = take<float>(f, n);
  const auto plane = take<int>(f, n);
  const auto cost = take<unsigned>(f, n);
  const auto runner = take<unsigned>(f, n);
  std::vector<std::vector<float>> sdepth;
  for (int v = 1; v <= n_src; ++v) sdepth.push_back(take<float>(f, n));
  const auto w_depth = take<float>(f, n);
  const auto w_plane = take<int>(f, n);
  std::vector<float> fdepth(n);
  std::vector<int> fplane(n);
  ekf::FilterArgs a{};
  a.depth = depth.data(); a.plane = plane.data(); a.out_depth = fdepth.data(); a.out_plane = fplane.data(); a.xyz = nullptr;
  a.W = W; a.H = H; a.n_src = n_src; a.min_agree = min_agree; a.rel_tol = rel_tol;
  a.fx = K[0][0]; a.fy = K[0][1]; a.cx = K[0][2]; a.cy = K[0][3];
  std::vector<double> tR;
  std::vector<ekf::DenseCam> cam;
  if (!cams(K, pose, tR, cam)) return 2;
  for (int v = 1; v <= n_src; ++v) {
    ekf::dense_relative(cam[0], cam[v], a.s[v - 1]);
    a.s[v - 1].depth = sdepth[v - 1].data();
  }
  const unsigned *c1 = cost.data(), *c2 = runner.data();
  launch({(unsigned)((n + 255) / 256), 1, 1}, [&] { ekf::k_depth_filter_unique(a, c1, c2, u); });
  const int bad = differs("filtered depth", fdepth, w_depth) + differs("filtered plane", fplane, w_plane);
  size_t kept = 0;
  for (float z : fdepth) kept += z > 0.f;
  std::printf("%s: %d x %d, filter against %d sources, uniqueness %d, %zu kept: %s\n", path_, W, H, n_src, u, kept, bad ? "DIFFERS" : "equal");
  return bad ? 1 : 0;
}

// every case file starts with one int: 0 = a sweep, 1 = a filter
static int run(const char* path_) {
  FILE* f = std::fopen(path_, "rb");
  if (!f) { std::perror(path_); return 2; }
  const int kind = take<int>(f, 1)[0];
  const int rc = kind == 0 ? run_sweep(f, path_) : run_filter(f, path_);
  std::fclose(f);
  return rc;
}
