// Key-frame selection through include/vslam_filter_hip.hpp's KeyframeSelectorHip: a scripted stream of camera poses and
// 7 x 7 covariance blocks is written into a filter frame by frame and observed.  Without an argument the stream is a walk
// along x whose covariance figure falls inside each window; with a file, each record is `id`, 7 pose values and 49
// values of the block (row-major).  Prints one line `id action emitted-id` per frame and "ok" at the end.
#include <cmath>
#include <cstdio>
#include <vector>

#include "vslam_filter_hip.hpp"

struct Frame {
  int id;
  float pose[7];
  float cov[49];
};

static std::vector<Frame> builtin() {
  std::vector<Frame> out;
  for (int k = 0; k < 24; ++k) {
    Frame f = {};
    f.id = k + 1;
    f.pose[0] = 1.3f * k;                                // 3.33 * 1.3 = 4.3 per frame
    f.pose[3] = 1.f;
    const float c = 0.5f - 0.01f * (k % 5) + 0.02f * (k % 3);
    for (int i = 0; i < 7; ++i) f.cov[8 * i] = c / 7.f;
    out.push_back(f);
  }
  return out;
}

static bool load(const char* path, std::vector<Frame>& out) {
  std::FILE* fh = std::fopen(path, "r");
  if (!fh) return false;
  Frame f;
  while (std::fscanf(fh, "%d", &f.id) == 1) {
    for (float& v : f.pose) if (std::fscanf(fh, "%f", &v) != 1) { std::fclose(fh); return false; }
    for (float& v : f.cov) if (std::fscanf(fh, "%f", &v) != 1) { std::fclose(fh); return false; }
    out.push_back(f);
  }
  std::fclose(fh);
  return true;
}

int main(int argc, char** argv) {
  std::vector<Frame> frames;
  if (argc > 1) {
    if (!load(argv[1], frames)) {
      std::fprintf(stderr, "cannot read %s\n", argv[1]);
      return 64;
    }
  } else {
    frames = builtin();
  }
  ekf_config cfg;
  ekf_config_default(&cfg);
  VSlamFilterHip filter(cfg, 16);
  KeyframeSelectorHip sel(filter);
  int emits = 0;
  for (const Frame& f : frames) {
    float colmajor[49];
    for (int r = 0; r < 7; ++r) for (int c = 0; c < 7; ++c) colmajor[c * 7 + r] = f.cov[r * 7 + c];
    if (ekf_set_state(filter.handle(), f.pose, 0, 7) != EKF_OK) return 1;
    if (ekf_set_sigma_block(filter.handle(), colmajor, 0, 0, 7, 7) != EKF_OK) return 1;
    const KeyframeSelectorHip::Result r = sel.observe(f.id);
    int id = -1;
    if (r.emitted()) {
      const KeyframeSelectorHip::Emitted e = sel.emitted();
      id = e.id;
      ++emits;
      if (e.projections.size() != 3 || e.projections[0] != 0) return 2;     // no features: the "0 0 0" row
    }
    std::printf("%d %d %d\n", f.id, r.action, id);
  }
  if (argc == 1 && emits < 3) return 3;
  std::printf("ok\n");
  return 0;
}
