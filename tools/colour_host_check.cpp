// The four colour kernels of csrc/ekf_dense_stereo.hpp, ekf_fusion.hpp and ekf_raycast.hpp run lane by lane on the host
//  by host_kernels.hpp, which says how to build and run this.  It reads the case files
// tools/colour_host_check.py writes (inputs in buffers of exactly the device's sizes, and the numpy oracle's outputs) and
// compares bit for bit.  The keys the vertex colours are made from come from the grey extraction kernels, run here as well.
#include "host_tsdf.hpp"

static int run(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::perror(path); return 2; }
  const auto hdr = take<int>(f, 7);
  const auto par = take<double>(f, 5);
  ekf::TsdfGrid g{hdr[0], hdr[1], hdr[2], {par[0], par[1], par[2]}, par[3]};
  const int n_maps = hdr[3], min_count = hdr[4], n_views = hdr[5], n_images = hdr[6];
  const size_t nvox = (size_t)g.nx * g.ny * g.nz;
  struct Map { int W, H, C; std::vector<double> K, pose; std::vector<float> depth; std::vector<unsigned char> img; };
  std::vector<Map> maps;
  for (int m = 0; m < n_maps; ++m) {
    const auto whc = take<int>(f, 3);
    Map mp{whc[0], whc[1], whc[2], take<double>(f, 4), take<double>(f, 7), {}, {}};
    mp.depth = take<float>(f, (size_t)mp.W * mp.H);
    mp.img = take<unsigned char>(f, (size_t)mp.W * mp.H * mp.C);
    maps.push_back(std::move(mp));
  }
  auto sum = take<float>(f, nvox);
  auto cnt = take<unsigned short>(f, nvox);
  auto gsum = take<unsigned>(f, nvox);
  auto csum = take<unsigned>(f, 3 * nvox);
  const auto w_sum = take<float>(f, nvox);
  const auto w_cnt = take<unsigned short>(f, nvox);
  const auto w_gsum = take<unsigned>(f, nvox);
  const auto w_csum = take<unsigned>(f, 3 * nvox);
  const size_t n_want = (size_t)take<unsigned long long>(f, 1)[0];
  const auto w_vcol = take<unsigned char>(f, n_want * 9);

  int bad = 0;
  // k_tsdf_integrate_colour
  for (const Map& mp : maps) {
    ekf::IntegrateColourArgs c{};
    ekf::IntegrateArgs& a = c.g;
    a.sum = sum.data(); a.cnt = cnt.data(); a.gsum = gsum.data();
    a.depth = mp.depth.data(); a.img = mp.C == 1 ? mp.img.data() : nullptr; a.W = mp.W; a.H = mp.H;
    a.g = g; a.trunc = par[4];
    a.fx = mp.K[0]; a.fy = mp.K[1]; a.cx = mp.K[2]; a.cy = mp.K[3];
    double q[4];
    if (!ekf::dense_pose(mp.pose.data(), a.t, a.R, q)) return 2;
    c.bgr = mp.C == 3 ? mp.img.data() : nullptr;
    c.csum = csum.data();
    c.nvox = nvox;
    launch({(unsigned)((nvox + 255) / 256), 1, 1}, [&] { ekf::k_tsdf_integrate_colour(c); });
  }
  bad += differs("sum", sum, w_sum) + differs("cnt", cnt, w_cnt) + differs("gsum", gsum, w_gsum) + differs("csum", csum, w_csum);

  // the grey extraction for its keys, then k_tsdf_colour_vertices
  const HostMesh mesh = host_extract(sum, cnt, gsum, g, min_count);
  const size_t n_tri = mesh.n_tri, nv = n_tri * 3;
  std::vector<unsigned char> vcol(nv * 3, 0xA5);
  if (n_tri) {
    const ekf::ColourVertexArgs c{sum.data(), cnt.data(), csum.data(), mesh.key.data(), vcol.data(), (unsigned long long)nv, nvox,
                                  (unsigned)g.nx, (unsigned)g.ny};
    launch({(unsigned)((nv + 255) / 256), 1, 1}, [&] { ekf::k_tsdf_colour_vertices(c); });
  }
  bad += differs("vertex colours", vcol, w_vcol);

  // k_tsdf_raycast_colour
  size_t hits = 0;
  std::vector<float> mean(nvox, 1.f);
  const ekf::MeanArgs m{sum.data(), cnt.data(), mean.data(), (unsigned)nvox, min_count};
  if (n_views) launch({(unsigned)((nvox + 255) / 256), 1, 1}, [&] { ekf::k_tsdf_mean(m); });
  for (int v = 0; v < n_views; ++v) {
    const auto whn = take<int>(f, 3);
    const auto vp = take<double>(f, 13);
    const int W = whn[0], H = whn[1];
    const size_t npix = (size_t)W * H;
    const auto w_depth = take<float>(f, npix);
    const auto w_normal = take<float>(f, npix * 3);
    const auto w_grey = take<unsigned char>(f, npix);
    const auto w_col = take<unsigned char>(f, npix * 3);
    std::vector<float> depth(npix, -1.f), normal(npix * 3, -1.f);
    std::vector<unsigned char> rgrey(npix, 0xA5), col(npix * 3, 0xA5);
    ekf::RaycastArgs a;
    if (!host_raycast_args(a, mean.data(), cnt.data(), gsum.data(), depth.data(), normal.data(), rgrey.data(), g, W, H, whn[2], vp.data()))
      return 2;
    const ekf::RaycastColour k{csum.data(), col.data(), nvox};
    launch({(unsigned)((W + 15) / 16), (unsigned)((H + 15) / 16), 1}, [&] { ekf::k_tsdf_raycast_colour(a, k); });
    for (float d : depth) hits += d > 0.f;
    bad += differs("depth", depth, w_depth) + differs("normal", normal, w_normal) + differs("grey", rgrey, w_grey) +
           differs("colour", col, w_col);
  }

  // k_bgr_to_grey
  for (int i = 0; i < n_images; ++i) {
    const unsigned npix = (unsigned)take<int>(f, 1)[0];
    const auto bgr = take<unsigned char>(f, (size_t)npix * 3);
    const auto w_g = take<unsigned char>(f, npix);
    std::vector<unsigned char> out(npix, 0xA5);
    const ekf::GreyArgs a{bgr.data(), out.data(), npix};
    launch({(npix / 4u + 1u + 255u) / 256u, 1, 1}, [&] { ekf::k_bgr_to_grey(a); });
    bad += differs("grey image", out, w_g);
  }
  std::fclose(f);

  std::printf("%s: %d x %d x %d, %d maps, min_count %d, %zu triangles (oracle %zu), %d views with %zu hits, %d images: %s\n", path,
              g.nx, g.ny, g.nz, n_maps, min_count, n_tri, n_want, n_views, hits, n_images, bad ? "DIFFERS" : "equal");
  return bad ? 1 : 0;
}
