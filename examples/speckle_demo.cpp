// The speckle filter through include/vslam_filter_hip.hpp's DenseStereoHip, on the scene of
// unique_demo.cpp: three cameras half a unit apart look at a textured plane that carries a patch without texture.  The
// geometric filter with the uniqueness test at 5 per cent drops nearly all of the arbitrary depths inside the patch; what it
// leaves are islands of a few pixels whose neighbours are gone.  filterSpeckle(0, 4, 1) segments the filtered map into
// connected regions whose planes differ by at most 1 from pixel to pixel and drops the regions of fewer than 4 pixels.
// Prints the number of segments and of kept pixels before and after, and "ok" on success.
#include <cmath>
#include <cstdio>
#include <vector>

#include "vslam_filter_hip.hpp"

static const int W = 96, H = 64, D = 12, TRUE_PLANE = 5, MIN_SIZE = 4, MAX_DIFF = 1;
static const double K[4] = {64.0, 64.0, 48.0, 32.0};
static const double W_MIN = 0.15, W_MAX = 0.40;
static const double RECT[4] = {-1.0, -0.2, -0.6, 0.6};              // x0 < X < x1, y0 < Y < y1 in the world: no texture

static double texture(double X, double Y) {
  return 127.5 + 23.0 * (std::sin(7.3 * X + 1.1 * Y) + std::sin(2.9 * X - 6.1 * Y + 0.7) + std::sin(11.7 * X + 4.3 * Y + 2.1) +
                         std::sin(-4.7 * X + 9.9 * Y + 0.3) + 0.7 * std::sin(17.1 * X - 2.3 * Y) + 0.7 * std::sin(1.3 * X + 15.7 * Y + 1.9));
}

static unsigned char to_byte(double v) {
  v = std::floor(v + 0.5);
  return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// the plane z = Z seen from a camera at (cx, 0, 0) with no rotation
static std::vector<unsigned char> render(double cx, double Z) {
  std::vector<unsigned char> g((size_t)W * H);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const double X = cx + Z * (x - K[2]) / K[0], Y = Z * (y - K[3]) / K[1];
      const bool flat = X > RECT[0] && X < RECT[1] && Y > RECT[2] && Y < RECT[3];
      g[(size_t)y * W + x] = to_byte(flat ? 128.0 : texture(X, Y));
    }
  return g;
}

struct Count { int kept, wrong; };

// pixels of a filtered map with a depth, and those of them more than one plane step from the truth
static Count count(const DenseStereoHip::Depth& f, double Z) {
  const double step = (W_MAX - W_MIN) / (D - 1);
  Count c = {0, 0};
  for (size_t i = 0; i < f.depth.size(); ++i)
    if (f.depth[i] > 0.f) {
      ++c.kept;
      if (std::fabs(1.0 / (double)f.depth[i] - 1.0 / Z) > step) ++c.wrong;
    }
  return c;
}

// segments of at least min_size pixels (a segment's root is the pixel that carries its own index), and their pixels
static Count large(const DenseStereoHip::Segments& s, unsigned min_size) {
  Count c = {0, 0};                                                 // kept: pixels, wrong: segments
  for (size_t i = 0; i < s.label.size(); ++i)
    if (s.label[i] == (unsigned)i && s.size[i] >= min_size) {
      ++c.wrong;
      c.kept += (int)s.size[i];
    }
  return c;
}

int main() {
  const double Z = 1.0 / (W_MIN + TRUE_PLANE * (W_MAX - W_MIN) / (D - 1));
  const double cams[3] = {0.0, 0.5, -0.5};
  DenseStereoHip ds(W, H, 3);
  for (int s = 0; s < 3; ++s) {
    const double pose[7] = {cams[s], 0, 0, 1, 0, 0, 0};
    ds.setView(s, render(cams[s], Z).data(), K, pose);
  }
  ds.profile(true);
  ds.keepRunnerUp(true);
  for (int s = 0; s < 3; ++s) ds.sweep(s, {(s + 1) % 3, (s + 2) % 3}, W_MIN, W_MAX, D, 1, 20);
  ds.filterUnique(0, {1, 2}, 5);
  const DenseStereoHip::Depth before = ds.depth(0, true), swept = ds.depth(0, false);
  ds.filterSpeckle(0, MIN_SIZE, MAX_DIFF);
  const DenseStereoHip::Segments seg = ds.segments(0);              // as they were before the removal
  const DenseStereoHip::Depth after = ds.depth(0, true);
  ds.filterSpeckle(0, MIN_SIZE, MAX_DIFF);                          // idempotent: what is left are segments of 4 pixels or more
  const DenseStereoHip::Segments seg2 = ds.segments(0);
  const DenseStereoHip::Depth again = ds.depth(0, true), swept2 = ds.depth(0, false);
  // the same filter for maps of the caller's own
  std::vector<float> depth = before.depth;
  std::vector<int> plane = before.plane;
  const DenseStereoHip::Segments seg3 = ds.speckleMaps(depth, plane, MIN_SIZE, MAX_DIFF);

  const Count a = count(before, Z), b = count(after, Z), all = large(seg, 1), big = large(seg, MIN_SIZE), left = large(seg2, 1);
  double ms[4];
  long long n[4];
  ds.getSpeckleProfile(ms, n);
  std::printf("of %d pixels the filter with uniqueness 5 kept %d (%d of them wrong) in %d segments; filterSpeckle(%d, %d) kept %d (%d wrong) in %d segments\n",
              W * H, a.kept, a.wrong, all.wrong, MIN_SIZE, MAX_DIFF, b.kept, b.wrong, big.wrong);
  std::printf("k_speckle_label %.3f ms, k_speckle_merge %.3f ms, k_speckle_count %.3f ms, k_speckle_apply %.3f ms, x %lld each\n",
              ms[0] / (double)n[0], ms[1] / (double)n[1], ms[2] / (double)n[2], ms[3] / (double)n[3], n[0]);
  // the pixel counts of the segments are those of the maps; the removal takes whole segments and nothing else
  if (all.kept != a.kept || big.kept != b.kept || left.kept != b.kept || left.wrong != big.wrong) return 2;
  for (size_t i = 0; i < after.depth.size(); ++i) {
    const bool keep = seg.size[i] >= (unsigned)MIN_SIZE;
    if (after.depth[i] != (keep ? before.depth[i] : 0.f) || after.plane[i] != (keep ? before.plane[i] : -1)) return 3;
  }
  if (again.depth != after.depth || again.plane != after.plane || swept2.depth != swept.depth || swept2.plane != swept.plane) return 4;
  if (depth != after.depth || plane != after.plane || seg3.label != seg.label || seg3.size != seg.size) return 5;
  // the oracles' counts on this scene are 4923 kept (1 wrong) in 15 segments and 4905 kept (1 wrong) in 6
  if (!(b.kept < a.kept && 100 * b.kept >= 95 * a.kept && b.wrong <= a.wrong && big.wrong < all.wrong && n[0] == 3 && n[1] == 3 &&
        n[2] == 3 && n[3] == 3))
    return 1;
  std::printf("ok\n");
  return 0;
}
