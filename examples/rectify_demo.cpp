// Key frames for a pinhole consumer through include/vslam_filter_hip.hpp: the frames of
// raw_frame_demo.cpp go through a filter whose lens is distorted (the default config's k1 k2 p1 p2), and for every emitted
// key frame the demo asks for what a bundle adjuster or a dense step needs: the rectified raw and grey image, the
// undistorted projection rows and the one K they belong to.  It checks that the selector's rectified image is the
// rectified frame the filter held for that id, that K of the two resolutions describe the same rays, and that the
// principal point is a fixed point of the undistortion.  Prints `id action emitted-id rows` per frame, both K and "ok".
#include <cmath>
#include <cstdio>
#include <map>
#include <vector>

#include "vslam_filter_hip.hpp"

static const int W = 64, H = 48, C = 3, S = 2;

static std::vector<unsigned char> frame_of(int id) {
  std::vector<unsigned char> p((size_t)W * H * C);
  unsigned v = 12345u + 977u * (unsigned)id;
  for (unsigned char& b : p) { v = v * 1664525u + 1013904223u; b = (unsigned char)(v >> 24); }
  return p;
}

int main() {
  ekf_config cfg;
  ekf_config_default(&cfg);
  cfg.scale = S;
  cfg.image_width = W / S;
  cfg.image_height = H / S;
  cfg.window_size = 5;
  cfg.fx = cfg.fy = 30.f;                                  // a lens for a 32 x 24 frame; the default distortion stays
  cfg.u0 = 15.5f;
  cfg.v0 = 11.5f;
  VSlamFilterHip filter(cfg, 16);
  KeyframeSelectorHip sel(filter, W, H, C, 18.f, true);
  std::map<int, std::vector<unsigned char>> rect_raw, rect_gray;
  int emits = 0;
  for (int k = 0; k < 24; ++k) {
    const int id = k + 1;
    const std::vector<unsigned char> raw = frame_of(id);
    filter.captureNewFrame(raw.data(), W, H, C, W * C, 1.0 + k / 30.0);
    rect_raw[id] = filter.getFrameRectified(W, H, C, true);
    rect_gray[id] = filter.getFrameRectified(W / S, H / S);
    if (rect_raw[id] == raw) return 2;                     // the lens is distorted: the remap must move pixels
    float pose[7] = {1.3f * k, 0, 0, 1, 0, 0, 0};
    float cov[49] = {};
    const float c = 0.5f - 0.01f * (k % 5) + 0.02f * (k % 3);
    for (int i = 0; i < 7; ++i) cov[8 * i] = c / 7.f;
    if (ekf_set_state(filter.handle(), pose, 0, 7) != EKF_OK) return 1;
    if (ekf_set_sigma_block(filter.handle(), cov, 0, 0, 7, 7) != EKF_OK) return 1;
    const KeyframeSelectorHip::Result r = sel.observe(id);
    int kid = -1, rows = 0;
    if (r.emitted()) {
      kid = sel.emitted().id;
      ++emits;
      if (sel.emittedImageRectified(W, H, C, true) != rect_raw[kid]) return 3;
      if (sel.emittedImageRectified(W / S, H / S) != rect_gray[kid]) return 4;
      rows = (int)sel.emittedRowsRectified(true).size() / 2;
    }
    std::printf("%d %d %d %d\n", id, r.action, kid, rows);
  }
  if (emits < 3) return 5;
  const ekf_sba_camera K0 = filter.rectifiedCamera(false), K1 = filter.rectifiedCamera(true);
  std::printf("K matcher %.17g %.17g %.17g %.17g\nK raw %.17g %.17g %.17g %.17g\n", K0.fx, K0.fy, K0.cx, K0.cy, K1.fx, K1.fy,
              K1.cx, K1.cy);
  // raw pixel X and matcher pixel u = (X + 0.5) / S - 0.5 are the same ray under the two K
  const double X = 40.0, u = (X + 0.5) / S - 0.5;
  if (std::fabs((X - K1.cx) / K1.fx - (u - K0.cx) / K0.fx) > 1e-12) return 6;
  // the principal point is where the lens model moves nothing
  const std::vector<double> pp = filter.undistortPixels({K1.cx, K1.cy}, true);
  if (std::fabs(pp[0] - K1.cx) > 1e-9 || std::fabs(pp[1] - K1.cy) > 1e-9) return 7;
  std::printf("ok\n");
  return 0;
}
