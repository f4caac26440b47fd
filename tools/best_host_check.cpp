// The kernels of the best-K source selection (csrc/ekf_dense_stereo.hpp: k_plane_sweep_best, k_plane_sweep_best_census,
// k_sweep_volume_best, k_sweep_volume_best_census, the latter two followed by the unchanged k_sgm_path and k_sgm_winner of
// csrc/ekf_dense_sgm.hpp) run lane by lane on the host by host_kernels.hpp, which says how to build
// and run this.  It reads the case files tools/best_host_check.py writes (inputs in buffers of exactly the device's sizes,
// and the numpy oracle's outputs), makes the launches of DenseStereo::sweep and DenseSgm::sweep with n_best > 0 -- k_census of
// the reference and of every source first where the cost is census -- and compares bit for bit.
#include "host_kernels.hpp"

#include "../ekf-monoslam_for_3d-reconstruction_amd/csrc/ekf_dense_sgm.hpp"

template <int G, int NP>
static void path(const ekf::SgmPathArgs& p, bool first, unsigned wg) {
  if (first)
    launch({wg, 1, 1}, [&] { ekf::k_sgm_path<G, NP, true>(p); });
  else
    launch({wg, 1, 1}, [&] { ekf::k_sgm_path<G, NP, false>(p); });
}

// case file: ints W H D radius trunc n_src n_best census paths p1 p2; doubles w_min w_max; per view (0 = reference, then the
// sources) 4 + 7 doubles (K, pose) and W H bytes; then the oracle: for paths > 0 C and S (D H W unsigned each), and depth
// plane cost views.
static int run(const char* path_) {
  FILE* f = std::fopen(path_, "rb");
  if (!f) { std::perror(path_); return 2; }
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
  const auto w_C = take<unsigned>(f, elems);
  const auto w_S = take<unsigned>(f, elems);
  const auto w_depth = take<float>(f, n);
  const auto w_plane = take<int>(f, n);
  const auto w_cost = take<unsigned>(f, n);
  const auto w_views = take<unsigned char>(f, n);
  std::fclose(f);

  // DenseStereo::census_update of every view (the census cost only: an absolute-difference sweep has no descriptors)
  const Idx3 tiles{(unsigned)((W + ekf::kDenseTW - 1) / ekf::kDenseTW), (unsigned)((H + ekf::kDenseTH - 1) / ekf::kDenseTH), 1};
  std::vector<std::vector<unsigned long long>> T;
  for (int v = 0; census && v <= n_src; ++v) {
    T.emplace_back(n);
    const ekf::CensusArgs c{img[v].data(), T[v].data(), W, H};
    launch(tiles, [&] { ekf::k_census(c); });
  }

  // the host side of DenseStereo::relative, from the same dense_pose
  std::vector<double> t(3 * (n_src + 1)), R(9 * (n_src + 1));
  for (int v = 0; v <= n_src; ++v) {
    double q[4];
    if (!ekf::dense_pose(pose[v].data(), &t[3 * v], &R[9 * v], q)) return 2;
  }
  std::vector<float> depth(n);
  std::vector<int> plane(n);
  std::vector<unsigned> cost(n), C(elems), S(elems);
  std::vector<unsigned char> views(n), V(elems);
  ekf::SweepArgs a{};
  a.ref = census ? nullptr : img[0].data();               // each cost reads its own inputs alone
  a.ref_census = census ? T[0].data() : nullptr;
  a.depth = depth.data(); a.plane = plane.data(); a.cost = cost.data(); a.views = views.data();
  a.W = W; a.H = H; a.D = D; a.radius = radius; a.trunc = trunc; a.n_src = n_src;
  a.fx = K[0][0]; a.fy = K[0][1]; a.cx = K[0][2]; a.cy = K[0][3];
  a.w_min = par[0];
  a.step = (par[1] - par[0]) / (double)(D - 1);
  for (int v = 1; v <= n_src; ++v) {
    ekf::DenseSrc& o = a.s[v - 1];
    const double *Rr = &R[0], *Rs = &R[9 * v];
    const double d[3] = {t[0] - t[3 * v], t[1] - t[3 * v + 1], t[2] - t[3 * v + 2]};
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) o.A[3 * i + j] = Rs[i] * Rr[j] + Rs[3 + i] * Rr[3 + j] + Rs[6 + i] * Rr[6 + j];
      o.b[i] = Rs[i] * d[0] + Rs[3 + i] * d[1] + Rs[6 + i] * d[2];
    }
    o.fx = K[v][0]; o.fy = K[v][1]; o.cx = K[v][2]; o.cy = K[v][3];
    o.img = census ? nullptr : img[v].data();
    o.census = census ? T[v].data() : nullptr;
    o.depth = nullptr;
  }
  int bad = 0;
  if (paths == 0) {
    if (census) launch(tiles, [&] { ekf::k_plane_sweep_best_census(a, n_best); });
    else launch(tiles, [&] { ekf::k_plane_sweep_best(a, n_best); });
  } else {
    const ekf::SweepVolume vol{C.data(), V.data()};
    if (census) launch(tiles, [&] { ekf::k_sweep_volume_best_census(a, vol, n_best); });
    else launch(tiles, [&] { ekf::k_sweep_volume_best(a, vol, n_best); });
    std::vector<unsigned> planes(elems);                  // as ekf_dense_get_volume delivers a volume
    ekf::sgm_volume_to_planes(C.data(), planes.data(), n, D);
    bad += differs("raw volume", planes, w_C);
    for (int i = 0; i < paths; ++i) {                     // DenseSgm::sweep's choice of grid and instantiation
      const ekf::SgmPathArgs p{C.data(), S.data(), W, H, D, p1, p2, ekf::kSgmDir[i][0], ekf::kSgmDir[i][1]};
      const bool diag = p.dx != 0 && p.dy != 0;
      const int nlines = diag ? W + H - 1 : (p.dy == 0 ? H : W);
      const int G = D <= 16 ? 16 : 64;
      const unsigned wg = (unsigned)((nlines + 256 / G - 1) / (256 / G));
      const int np = (D + 63) / 64;
      if (G == 16) path<16, 1>(p, i == 0, wg);
      else if (np <= 1) path<64, 1>(p, i == 0, wg);
      else if (np <= 2) path<64, 2>(p, i == 0, wg);
      else if (np <= 4) path<64, 4>(p, i == 0, wg);
      else if (np <= 8) path<64, 8>(p, i == 0, wg);
      else path<64, 16>(p, i == 0, wg);
    }
    const ekf::SgmWinnerArgs w{S.data(), V.data(), a};
    launch({(unsigned)((n + 255) / 256), 1, 1}, [&] { ekf::k_sgm_winner(w); });
    ekf::sgm_volume_to_planes(S.data(), planes.data(), n, D);
    bad += differs("aggregated volume", planes, w_S);
  }
  bad += differs("depth", depth, w_depth) + differs("plane", plane, w_plane) + differs("cost", cost, w_cost) + differs("views", views, w_views);
  std::printf("%s: %d x %d, D %d, radius %d, trunc %d, %d of %d sources, %s%s: %s\n", path_, W, H, D, radius, trunc, n_best, n_src,
              census ? "census" : "absolute differences", paths ? ", aggregated" : "", bad ? "DIFFERS" : "equal");
  return bad ? 1 : 0;
}
