// From the camera's own frame to a key frame through include/vslam_filter_hip.hpp: synthetic 64 x 48 B, G, R frames go into
// VSlamFilterHip::captureNewFrame (resize by scale = 2 and grey conversion on the device), the camera
// walks along x, and a raw KeyframeSelectorHip keeps the full-resolution colour frame of every key frame beside the
// matcher's grey one.  Each emitted key frame is checked against the frame that was given for its id; the grey frame is
// checked against the pinned arithmetic worked out here on the host.  Prints `id action emitted-id` per frame and "ok".
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

// section 13 at an exact factor of 2: the rounded 2 x 2 mean per channel, then Y = (1868 B + 9617 G + 4899 R + 8192) >> 14
static std::vector<unsigned char> gray_of(const std::vector<unsigned char>& raw) {
  std::vector<unsigned char> g((size_t)(W / S) * (H / S));
  for (int y = 0; y < H / S; ++y)
    for (int x = 0; x < W / S; ++x) {
      int ch[3];
      for (int c = 0; c < 3; ++c) {
        auto at = [&](int yy, int xx) { return (int)raw[((size_t)yy * W + xx) * C + c]; };
        ch[c] = (at(2 * y, 2 * x) + at(2 * y, 2 * x + 1) + at(2 * y + 1, 2 * x) + at(2 * y + 1, 2 * x + 1) + 2) >> 2;
      }
      g[(size_t)y * (W / S) + x] = (unsigned char)((ch[0] * 1868 + ch[1] * 9617 + ch[2] * 4899 + 8192) >> 14);
    }
  return g;
}

int main() {
  ekf_config cfg;
  ekf_config_default(&cfg);
  cfg.scale = S;
  cfg.image_width = W / S;
  cfg.image_height = H / S;
  cfg.window_size = 5;
  VSlamFilterHip filter(cfg, 16);
  KeyframeSelectorHip sel(filter, W, H, C);
  std::map<int, std::vector<unsigned char>> shown;
  int emits = 0;
  for (int k = 0; k < 24; ++k) {
    const int id = k + 1;
    shown[id] = frame_of(id);
    filter.captureNewFrame(shown[id].data(), W, H, C, W * C, 1.0 + k / 30.0);
    if (filter.getFrame(W / S, H / S) != gray_of(shown[id])) return 2;
    float pose[7] = {1.3f * k, 0, 0, 1, 0, 0, 0};          // 3.33 * 1.3 = 4.3 per frame
    float cov[49] = {};
    const float c = 0.5f - 0.01f * (k % 5) + 0.02f * (k % 3);
    for (int i = 0; i < 7; ++i) cov[8 * i] = c / 7.f;
    if (ekf_set_state(filter.handle(), pose, 0, 7) != EKF_OK) return 1;
    if (ekf_set_sigma_block(filter.handle(), cov, 0, 0, 7, 7) != EKF_OK) return 1;
    const KeyframeSelectorHip::Result r = sel.observe(id);
    int kid = -1;
    if (r.emitted()) {
      kid = sel.emitted().id;
      ++emits;
      if (sel.emittedRawImage(W, H, C) != shown[kid]) return 3;
      if (sel.emittedImage(W / S, H / S) != gray_of(shown[kid])) return 4;
    }
    std::printf("%d %d %d\n", id, r.action, kid);
  }
  if (emits < 3) return 5;
  std::printf("ok\n");
  return 0;
}
