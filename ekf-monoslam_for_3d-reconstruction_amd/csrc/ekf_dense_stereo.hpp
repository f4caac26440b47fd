// Dense plane-sweep depth maps for key frames: up to 16 posed pinhole views of one size on the device, a
// sweep of D fronto-parallel planes (uniform in inverse depth) of a reference view against 1..8 source views, a geometric
// consistency filter over the swept maps, and the back-projection to world points.  The reference has no counterpart (its
// README defers the dense step to a second program); the arithmetic is pinned here and restated in numpy by
// tests/dense_oracle.py:
//   - every coordinate operation is fp64, rounded once, in the written left-to-right order; contraction is off in every
//     function below (host and device), as in ekf_rectify.hpp;
//   - the image sample is the 5-bit bilinear blend of §14.1; costs are integers, every sum has one fixed order, no atomics.
// Nothing here touches a filter, counts as a launch kind or runs a collective.
#pragma once
#include <climits>
#include <cmath>
#include <cstddef>
#include <limits>
#include <string>
#include <type_traits>
#include <vector>

// EKF_KERNELS_ONLY: the structs, the kernels and what fills their arguments (dense_pose, dense_relative, sweep_args) alone,
// for the host checks (tools/*_host_check.cpp), which run the kernels lane by lane on the host; tools/host_kernels.hpp supplies
// threadIdx, __syncthreads and the like.
#ifndef EKF_KERNELS_ONLY
#include <hip/hip_runtime.h>

#include "ekf_buffers.hpp"
#endif
#include "ekf_pixel.hpp"

namespace ekf {

constexpr int kDenseMaxViews = 16, kDenseMaxSrc = 8, kDenseMaxPlanes = 1024, kDenseMaxRadius = 4, kDenseMaxDim = 8192;
// The output tile of one workgroup and its halo.  32 x 16 on 256 lanes: a lane owns the two pixels (tx, ty) and (tx, ty + 8),
// a row of the tile is one half-wave (the LDS passes below read 32 consecutive words per half-wave: conflict-free), and
// the halo of radius 4 costs 960 / 512 = 1.9 warps per output pixel where a 16 x 16 tile would cost 2.25.
constexpr int kDenseTW = 32, kDenseTH = 16;
constexpr int kDenseHW = kDenseTW + 2 * kDenseMaxRadius, kDenseHH = kDenseTH + 2 * kDenseMaxRadius;
constexpr int kDenseHaloPerLane = (kDenseHW * kDenseHH + 255) / 256;      // 4

struct DenseSrc {
  const unsigned char* img;           // H rows of W bytes, tight
  const unsigned long long* census;   // W H descriptors of img (the census sweeps only, §20)
  const float* depth;                 // the source's swept depth (the filter only)
  double fx, fy, cx, cy;
  double A[9];                        // R_v^T R_r, row-major
  double b[3];                        // R_v^T (t_r - t_v)
};

struct SweepArgs {
  const unsigned char* ref;
  const unsigned long long* ref_census;   // W H descriptors of ref (the census sweeps only, §20)
  float* depth;
  int* plane;
  unsigned* cost;
  unsigned char* views;
  int W, H, D, radius, trunc, n_src;
  double fx, fy, cx, cy;              // the reference view's K
  double w_min, step;
  DenseSrc s[kDenseMaxSrc];
};

// One launch per depth map, one workgroup per 32 x 16 tile.  A halo pixel belongs to one lane for the whole launch, so the
// reference tile with its halo stays in that lane's registers (grey value and ray), not in LDS.  Per plane: every lane
// warps its (at most 4) halo pixels into every source view and writes the truncated absolute
// differences, summed over the views, to LDS as one word (the count of valid warps in the upper half); a horizontal and a
// vertical pass give the window sum.  The pixel costs are integers, so summing over the views before the window gives the
// number that a window sum per view would, with one pair of LDS passes per plane, not one per view.  Registers carry, per
// owned pixel, C of the previous plane, the best C with its plane, its C- and C+ and its count of valid views: the cost
// volume never leaves the CU.
//
// VOLUME (the first stage of the semi-global sweep, §19; ekf_dense_sgm.hpp): the same per-plane cost, but C_k and V_k of the
// owned pixels go to the volumes `vol` and no winner is kept or written.
struct SweepVolume {
  unsigned* C;                        // H x W x D, the planes of a pixel side by side: element (Y W + X) D + k
  unsigned char* V;                   // D x H x W, plane-major: element k W H + Y W + X
};

// depth, plane, cost and views of pixel `o` from the winner ks, its cost c0, its neighbours' cm / cp and its valid views
__device__ __forceinline__ void sweep_write_winner(const SweepArgs& a, size_t o, int ks, int cm, int c0, int cp, int nv) {
#pragma clang fp contract(off)
  double delta = 0.0;
  if (ks > 0 && ks < a.D - 1) {
    const int den = cm - 2 * c0 + cp;                                       // |.| <= 4 * 81 * 8 * 255 (4 * 2^24 aggregated)
    if (den > 0) delta = (double)(cm - cp) / (2.0 * (double)den);
  }
  const double w = a.w_min + ((double)ks + delta) * a.step;
  const bool none = nv == 0;
  a.depth[o] = none ? 0.f : (float)(1.0 / w);
  a.plane[o] = none ? -1 : ks;
  a.cost[o] = (unsigned)c0;
  a.views[o] = (unsigned char)nv;
}

// ---- census descriptors ----------------------------------------------------------------------------------
// T(X, Y) of an 8-bit image: bit b = 0 .. 61 for the offsets (dx, dy), dy = -3 .. 3 outer, dx = -4 .. 4 inner, (0, 0)
// skipped, is 1 iff (X + dx, Y + dy) lies inside the image and I there < I(X, Y).  Bits 62 and 63 are 0.
constexpr int kCensusRX = 4, kCensusRY = 3;
constexpr int kCensusHW = kDenseTW + 2 * kCensusRX, kCensusHH = kDenseTH + 2 * kCensusRY;      // 40 x 22

struct CensusArgs {
  const unsigned char* img;           // H rows of W bytes, tight
  unsigned long long* out;            // W H descriptors
  int W, H;
};

// One workgroup per 32 x 16 tile.  The tile and its 4 x 3 halo go to LDS once, one byte a lane and turn (every image byte is
// read from global memory once per tile); positions outside the image are filled with 255, where `neighbour < centre` is
// never true, so the 62 comparisons need no flag.  A lane owns the pixels (tx, ty) and (tx, ty + 8), as in the sweep: a row
// of the tile is one half-wave, its 32 byte reads of one offset fall into 8 or 9 consecutive LDS words (lanes that share a
// word are served by one broadcast) and its stores of the descriptors are 256 contiguous bytes.
__global__ void __launch_bounds__(256) k_census(CensusArgs a) {
  __shared__ unsigned char s_t[kCensusHH][kCensusHW];
  const int tid = threadIdx.x;
  const int x0 = (int)blockIdx.x * kDenseTW - kCensusRX, y0 = (int)blockIdx.y * kDenseTH - kCensusRY;
  for (int h = tid; h < kCensusHW * kCensusHH; h += 256) {
    const int hy = h / kCensusHW, hx = h - hy * kCensusHW;
    const int X = x0 + hx, Y = y0 + hy;
    const bool in = X >= 0 && X < a.W && Y >= 0 && Y < a.H;
    s_t[hy][hx] = in ? a.img[(size_t)Y * a.W + X] : (unsigned char)255;
  }
  __syncthreads();
  const int tx = tid & 31, ty = tid >> 5;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int oy = ty + 8 * j;
    const int X = (int)blockIdx.x * kDenseTW + tx, Y = (int)blockIdx.y * kDenseTH + oy;
    if (X >= a.W || Y >= a.H) continue;
    const unsigned c = s_t[oy + kCensusRY][tx + kCensusRX];
    unsigned lo = 0, hi = 0;                                                // bits 0 .. 31 and 32 .. 61
    int b = 0;
#pragma unroll
    for (int dy = 0; dy <= 2 * kCensusRY; ++dy)
#pragma unroll
      for (int dx = 0; dx <= 2 * kCensusRX; ++dx) {
        if (dy == kCensusRY && dx == kCensusRX) continue;
        const unsigned bit = (unsigned)s_t[oy + dy][tx + dx] < c ? 1u : 0u;
        if (b < 32) lo |= bit << b;
        else hi |= bit << (b - 32);
        ++b;
      }
    a.out[(size_t)Y * a.W + X] = ((unsigned long long)hi << 32) | lo;
  }
}

// ---- runner-up cost -----------------------------------------------------------------------------------------
// C2 = min { C_k : |k - k*| > 1 }, found in the one pass over the planes, before k* is known: a plane that beats the runner-up
// (cheaper, or as cheap with a smaller index) is k* or one of its two neighbours, so the runner-up is among the four smallest
// pairs (C, k).  C <= 81 * 8 * 255 < 2^18 and k < 1024: key = C << 10 | k < 2^28 orders them as the pairs (an int; the
// aggregate of §19, S < 2^24, takes a long long: k_sgm_winner_unique).  Four keys per pixel, sorted, the largest value of the
// type where there is no plane yet; runner_insert is best_insert's min / max chain (§21.2), every index a compile-time
// constant; runner_take reads the winner's plane from the smallest key and takes the first key two planes away.
constexpr int kRunnerKeys = 4;
constexpr unsigned kRunnerAbsent = 0xffffffffu;   // no plane with |k - k*| > 1 (D <= 3 only)
static_assert(kDenseMaxPlanes <= 1024 && 81 * kDenseMaxSrc * 255 < (1 << 18), "a (cost, plane) pair is a 28-bit key");
template <typename Key>
constexpr Key runner_none() { return std::numeric_limits<Key>::max(); }     // no plane: more than any key

template <typename Key>
__device__ __forceinline__ void runner_insert(Key (&t)[kRunnerKeys], Key key) {
#pragma unroll
  for (int i = 0; i < kRunnerKeys; ++i) {
    const bool less = key < t[i];
    const Key lo = less ? key : t[i];
    key = less ? t[i] : key;
    t[i] = lo;
  }
}
template <typename Key>
__device__ __forceinline__ unsigned runner_take(const Key (&t)[kRunnerKeys]) {
  const int ks = (int)(t[0] & 1023);                                        // the winner of §15.1: least cost, then least k
  unsigned c2 = kRunnerAbsent;
#pragma unroll
  for (int i = kRunnerKeys - 1; i >= 1; --i) {                               // the smallest such key is assigned last
    const int d = (int)(t[i] & 1023) - ks;
    c2 = (t[i] != runner_none<Key>() && (d > 1 || d < -1)) ? (unsigned)(t[i] >> 10) : c2;
  }
  return c2;
}

// The winner of one pixel over the planes k = 0, 1, .. in turn (§15.1), in registers: the cost of the previous plane, the least
// cost C with its plane K (the first of equals), its neighbours' costs M and P and its count of valid views V; with RUNNER the
// four smallest keys as well.  Written once for the sweeps (Key = int) and the aggregate's winner (long long, whose V is read
// from the stored counts after the loop: write takes the count).
template <bool RUNNER, typename Key>
struct SweepWinner {
  int prev = 0, C = INT_MAX, K = -2, M = 0, P = 0, V = 0;
  Key top[kRunnerKeys];                                                     // RUNNER only
  __device__ __forceinline__ SweepWinner() {
    if constexpr (RUNNER) {
#pragma unroll
      for (int i = 0; i < kRunnerKeys; ++i) top[i] = runner_none<Key>();
    }
  }
  // selects, not branches: the plane after the best one delivers its C+ (K = -2 before plane 0: never pending), a strictly
  // smaller cost takes over (C starts at INT_MAX, so plane 0 always does)
  __device__ __forceinline__ void step(int k, int c, int nv = 0) {
    const bool pending = K == k - 1, better = c < C;
    P = (pending || better) ? c : P;
    M = better ? prev : M;
    V = better ? nv : V;
    K = better ? k : K;
    C = better ? c : C;
    prev = c;
    if constexpr (RUNNER) runner_insert(top, ((Key)c << 10) | k);
  }
  __device__ __forceinline__ void write(const SweepArgs& a, size_t o, int nv, unsigned* runner) const {
    sweep_write_winner(a, o, K, M, C, P, nv);
    if constexpr (RUNNER) runner[o] = runner_take(top);
  }
};

// The cost c_v of one halo pixel (ray (hx, hy), reference value or descriptor `ref`) on the plane of depth z in the source
// view s: §15.1's warp and validity test, then the truncated absolute difference of the 5-bit bilinear sample or (CENSUS, §20)
// the truncated Hamming distance at the nearest pixel.  An invalid warp costs trunc; a valid one adds 1 to nv.
template <bool CENSUS, typename Ref>
__device__ __forceinline__ int sweep_view_cost(const SweepArgs& a, const DenseSrc& s, double hx, double hy, double z, Ref ref,
                                               double qx_max, double qy_max, int& nv) {
#pragma clang fp contract(off)
  const int W = a.W, H = a.H;
  const double a0 = s.A[0] * hx + s.A[1] * hy + s.A[2];
  const double a1 = s.A[3] * hx + s.A[4] * hy + s.A[5];
  const double a2 = s.A[6] * hx + s.A[7] * hy + s.A[8];
  const double Q0 = z * a0 + s.b[0];
  const double Q1 = z * a1 + s.b[1];
  const double Q2 = z * a2 + s.b[2];
  int c = a.trunc;
  if (Q2 > 0.0) {
    const double sx = s.fx * (Q0 / Q2) + s.cx;
    const double sy = s.fy * (Q1 / Q2) + s.cy;
    const double fqx = floor(sx * 32.0 + 0.5), fqy = floor(sy * 32.0 + 0.5);
    if (fqx >= 0.0 && fqx <= qx_max && fqy >= 0.0 && fqy <= qy_max) {       // (a NaN fails)
      const int qx = (int)fqx, qy = (int)fqy;
      if constexpr (CENSUS) {
        const int jx = (qx + 16) >> 5, jy = (qy + 16) >> 5;                   // the nearest pixel: jx <= W - 1, jy <= H - 1
        c = min(__builtin_popcountll(ref ^ s.census[(size_t)jy * W + jx]), a.trunc);
      } else {
        const int ix = qx >> 5, ax = qx & 31, iy = qy >> 5, ay = qy & 31;       // ix in [0, W - 1], iy in [0, H - 1]
        const int ix1 = min(ix + 1, W - 1), iy1 = min(iy + 1, H - 1);           // weight 0 where clamped (ax = 0 there)
        const unsigned char* r0 = s.img + (size_t)iy * W;
        const unsigned char* r1 = s.img + (size_t)iy1 * W;
        const int g = ((32 - ax) * (32 - ay) * (int)r0[ix] + ax * (32 - ay) * (int)r0[ix1] + (32 - ax) * ay * (int)r1[ix] +
                       ax * ay * (int)r1[ix1] + 512) >> 10;
        c = min(abs(ref - g), a.trunc);
      }
      ++nv;
    }
  }
  return c;
}

// ---- best-K source selection ------------------------------------------------------------------------------
// Per pixel and plane the cost is the sum of the n_best smallest per-view window sums C_k^v, not the sum of all of them: a
// selection does not commute with the window sum, so the windowed cost must exist per view and the one pair of LDS passes of
// a plane serves one PAIR of views a word, not all views.  Two views share an LDS word as 16-bit halves: a pixel cost is <= 255,
// a horizontal sum <= 9 * 255 = 2295 and a window sum <= 81 * 255 = 20 655 < 2^16, so no carry crosses the halves and one
// integer add serves both.  All kBestPairs planes of words stay in LDS at once (4 * 7104 = 28 416 B), so a plane of the sweep
// still costs two barriers whatever n_src is (§21.2 has the reasons).  The count of valid warps, whose place in the upper
// half is now taken, rides in the top byte of the first pair's word of s_c (bits 8 .. 15 and 24 .. 31 of a pair of pixel costs
// are free); the horizontal pass masks it off.
constexpr int kBestPairs = kDenseMaxSrc / 2;
constexpr int kBestNone = 0xffff;                 // no view: more than any window sum

// The n_best smallest of up to 8 values, in registers: a list s[0 .. 7], sorted, that starts as kBestNone eight times;
// best_insert lets x sink to its place by min / max, the larger value moving on (the largest of the nine drops out), and
// best_take sums the first n_best entries.  Every index is a compile-time constant, so the list never goes to scratch.
__device__ __forceinline__ void best_insert(int (&s)[kDenseMaxSrc], int x) {
#pragma unroll
  for (int i = 0; i < kDenseMaxSrc; ++i) {
    const int lo = min(s[i], x);
    x = max(s[i], x);
    s[i] = lo;
  }
}
// (predicated on i < n_best by a limit of 0, one SGPR each, not by a comparison, which would hold a pair of SGPRs each)
__device__ __forceinline__ int best_take(const int (&s)[kDenseMaxSrc], int n_best) {
  int sum = s[0];                                                           // n_best >= 1
#pragma unroll
  for (int i = 1; i < kDenseMaxSrc; ++i) sum += min(s[i], i < n_best ? kBestNone : 0);
  return sum;
}

// The one body of the twelve sweep kernels: the tile, the halo in registers, the two LDS passes of a plane, the volume stores
// or the winner, and four template parameters for what differs.
// CENSUS (§20; the fp64 warp is sweep_view_cost's either way): the matching cost is the Hamming distance of census
// descriptors, not the absolute grey difference.  A halo pixel's register value is then its 64-bit descriptor, and per source
// the four byte gathers and the blend become one 8-byte load at the nearest pixel and a popcount.
// BEST (§21): the cost of a plane is that of the n_best cheapest views.  It picks three stages: the words a halo pixel
// writes to LDS (one a pair of views, not one), what the horizontal pass masks and how often it runs (once a pair), and the
// vertical pass, which ends in the selection.
// RUNNER (§22): the four smallest keys of each owned pixel ride along and its runner-up goes to `runner`, W H words.
template <bool VOLUME, bool CENSUS, bool BEST, bool RUNNER>
__device__ __forceinline__ void plane_sweep_body(const SweepArgs& a, const SweepVolume& vol, int n_best, unsigned* runner) {
#pragma clang fp contract(off)
  static_assert(!(VOLUME && RUNNER), "the runner-up of an aggregated sweep is k_sgm_winner_unique's");
  constexpr int kWords = BEST ? kBestPairs : 1;                             // LDS words of a halo pixel
  constexpr int kCostMask = BEST ? 0x00ff00ff : 0xffff, kCountShift = BEST ? 24 : 16;     // of a word of s_c
  __shared__ int s_c[kWords][kDenseHH][kDenseHW + 1];
  __shared__ int s_h[kWords][kDenseHH][kDenseTW + 1];
  const int tid = threadIdx.x;
  const int r = a.radius, hw = kDenseTW + 2 * r, hh = kDenseTH + 2 * r, nh = hw * hh;
  const int x0 = (int)blockIdx.x * kDenseTW - r, y0 = (int)blockIdx.y * kDenseTH - r;
  const int W = a.W, H = a.H;
  const int n_pairs = BEST ? (a.n_src + 1) >> 1 : 1;                        // a kernel argument: uniform
  // what ekf_dense_sweep_best has checked: without it every loop below gets a guard, kept as a lane mask in two SGPRs.
  // (BEST only: the other six kernels keep the code, and the registers tests/test_isa_census.py holds, that they have without.)
  if constexpr (BEST) {
    __builtin_assume(r >= 0 && r <= kDenseMaxRadius);
    __builtin_assume(a.n_src >= 1 && a.n_src <= kDenseMaxSrc);
    __builtin_assume(a.D >= 1);
  }
  const double qx_max = (double)(32 * (W - 1)), qy_max = (double)(32 * (H - 1));

  // the lane's halo pixels: position in the halo, ray and reference grey value or descriptor, fixed for the launch
  int h_off[kDenseHaloPerLane];                                           // h_off < 0: none, or outside the image
  typename std::conditional<CENSUS, unsigned long long, int>::type h_ref[kDenseHaloPerLane];
  double h_x[kDenseHaloPerLane], h_y[kDenseHaloPerLane];
#pragma unroll
  for (int i = 0; i < kDenseHaloPerLane; ++i) {
    const int h = tid + 256 * i;
    const int hy = h / hw, hx = h - hy * hw;
    const int X = x0 + hx, Y = y0 + hy;
    const bool in = h < nh && X >= 0 && X < W && Y >= 0 && Y < H;
    h_off[i] = h < nh ? (in ? hy * (kDenseHW + 1) + hx : -1 - (hy * (kDenseHW + 1) + hx)) : INT_MIN;
    if constexpr (CENSUS)
      h_ref[i] = in ? a.ref_census[(size_t)Y * W + X] : 0ull;
    else
      h_ref[i] = in ? (int)a.ref[(size_t)Y * W + X] : 0;
    h_x[i] = ((double)X - a.cx) / a.fx;
    h_y[i] = ((double)Y - a.cy) / a.fy;
  }
  const int tx = tid & 31, ty = tid >> 5;
  constexpr int pair_words = kDenseHH * (kDenseHW + 1);
  static_assert(kDenseTW * kDenseTH >= 512, "halo positions 0 .. 511 exist at every radius");
  int* const sc = &s_c[0][0][0];

  // the two owned pixels: whether pixel j lies inside the image, and its index `o` in a W x H map
  auto owned = [&](int j, size_t& o) {
    const int X = (int)blockIdx.x * kDenseTW + tx, Y = (int)blockIdx.y * kDenseTH + ty + 8 * j;
    o = (size_t)Y * W + X;
    return X < W && Y < H;
  };
  // VOLUME: where they go in the volumes, in the form each pair of kernels was measured with (§15.6).  BEST: the addresses
  // of plane 0 (NULL: outside the image), per lane, so that the plane loop holds no base pointer in SGPRs, of which these
  // kernels have none to spare.  Otherwise the map index (-1: outside the image) beside the base pointers: the pointers cost
  // k_sweep_volume about 1 % at 320 x 240.
  long own[2] = {-1, -1};
  unsigned* own_C[2] = {nullptr, nullptr};
  unsigned char* own_V[2] = {nullptr, nullptr};
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    size_t o;
    if (VOLUME && owned(j, o)) {
      own[j] = (long)o;
      own_C[j] = vol.C + o * (size_t)a.D;
      own_V[j] = vol.V + o;
    }
  }
  const size_t plane_elems = (size_t)W * H;
  SweepWinner<RUNNER, int> win[2];
  for (int k = 0; k < a.D; ++k) {
    const double z = 1.0 / (a.w_min + (double)k * a.step);
#pragma unroll
    for (int i = 0; i < kDenseHaloPerLane; ++i) {
      if ((!BEST || i >= 2) && h_off[i] == INT_MIN) continue;               // (BEST knows r >= 0: the first 512 always exist)
      if (h_off[i] < 0) {                                                   // a window position outside the image: nothing
        for (int p = 0; p < n_pairs; ++p) sc[p * pair_words - 1 - h_off[i]] = 0;
        continue;
      }
      int nv = 0;
      if constexpr (BEST) {
        // one view a turn (the view's 38 words of kernel arguments sit in SGPRs; unrolled by two, the compiler keeps two
        // views' and spills): an even view opens a word, an odd one or the last one closes it.  The upper half of an odd
        // n_src's last word keeps trunc, the cost of a view whose every warp is invalid: no real view's window sum is
        // larger, so it sorts last and is never among the n_best <= n_src smallest.  The branches are uniform.
        int word = 0, word0 = 0;
#pragma unroll 1
        for (int v = 0; v < a.n_src; ++v) {
          const int c = sweep_view_cost<CENSUS>(a, a.s[v], h_x[i], h_y[i], z, h_ref[i], qx_max, qy_max, nv);
          word = (v & 1) ? (word & 0xffff) | (c << 16) : c | (a.trunc << 16);  // each half <= 255
          if ((v & 1) || v == a.n_src - 1) {
            if (v < 2) word0 = word;                                        // waits for the count of all views
            else sc[(v >> 1) * pair_words + h_off[i]] = word;
          }
        }
        sc[h_off[i]] = word0 | (nv << kCountShift);                         // nv <= 8
      } else {
        int csum = 0;
        for (int v = 0; v < a.n_src; ++v) csum += sweep_view_cost<CENSUS>(a, a.s[v], h_x[i], h_y[i], z, h_ref[i], qx_max, qy_max, nv);
        sc[h_off[i]] = csum | (nv << kCountShift);                          // csum <= 8 * 255
      }
    }
    __syncthreads();
    // horizontal pass over the hh halo rows, 32 columns each, of every word; the valid count of the owned pixels is read
    // here, before the barrier after which other lanes may overwrite s_c for the next plane
    for (int e = tid; e < hh * kDenseTW; e += 256) {
      const int row = e >> 5, col = e & 31;
      for (int p = 0; p < n_pairs; ++p) {
        int sum = 0;
        for (int d = 0; d <= 2 * r; ++d) sum += s_c[p][row][col + d] & kCostMask;
        s_h[p][row][col] = sum;                                             // BEST: each half <= 2295
      }
    }
    const int nv_own[2] = {s_c[0][ty + r][tx + r] >> kCountShift, s_c[0][ty + 8 + r][tx + r] >> kCountShift};
    __syncthreads();
    // vertical pass, BEST: and selection: the two owned pixels (the next write of s_h comes after the next plane's first barrier)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int oy = ty + 8 * j;
      int C = 0;
      if constexpr (BEST) {
        int best[kDenseMaxSrc];
#pragma unroll
        for (int i = 0; i < kDenseMaxSrc; ++i) best[i] = kBestNone;
#pragma unroll 1
        for (int p = 0; p < n_pairs; ++p) {
          unsigned word = 0;
          for (int d = 0; d <= 2 * r; ++d) word += (unsigned)s_h[p][oy + d][tx];   // each half <= 20 655
          best_insert(best, (int)(word & 0xffffu));
          best_insert(best, (int)(word >> 16));                             // (an odd n_src's last: the all-trunc view)
        }
        C = best_take(best, n_best);
      } else {
        for (int d = 0; d <= 2 * r; ++d) C += s_h[0][oy + d][tx];
      }
      if constexpr (VOLUME && BEST) {
        if (own_C[j]) {
          own_C[j][k] = (unsigned)C;
          own_V[j][(size_t)k * plane_elems] = (unsigned char)nv_own[j];
        }
      } else if constexpr (VOLUME) {
        if (own[j] >= 0) {
          vol.C[(size_t)own[j] * (size_t)a.D + (size_t)k] = (unsigned)C;
          vol.V[(size_t)k * plane_elems + (size_t)own[j]] = (unsigned char)nv_own[j];
        }
      } else {
        win[j].step(k, C, nv_own[j]);
      }
    }
  }
  if constexpr (!VOLUME) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      size_t o;
      if (owned(j, o)) win[j].write(a, o, win[j].V, runner);
    }
  }
}

__global__ void __launch_bounds__(256) k_plane_sweep(SweepArgs a) { plane_sweep_body<false, false, false, false>(a, {}, 0, nullptr); }
__global__ void __launch_bounds__(256) k_plane_sweep_census(SweepArgs a) { plane_sweep_body<false, true, false, false>(a, {}, 0, nullptr); }
__global__ void __launch_bounds__(256) k_plane_sweep_best(SweepArgs a, int n_best) {
  plane_sweep_body<false, false, true, false>(a, {}, n_best, nullptr);
}
__global__ void __launch_bounds__(256) k_plane_sweep_best_census(SweepArgs a, int n_best) {
  plane_sweep_body<false, true, true, false>(a, {}, n_best, nullptr);
}
// ... their twins that also write the runner-up (§22)
__global__ void __launch_bounds__(256) k_plane_sweep_unique(SweepArgs a, unsigned* runner) {
  plane_sweep_body<false, false, false, true>(a, {}, 0, runner);
}
__global__ void __launch_bounds__(256) k_plane_sweep_census_unique(SweepArgs a, unsigned* runner) {
  plane_sweep_body<false, true, false, true>(a, {}, 0, runner);
}
__global__ void __launch_bounds__(256) k_plane_sweep_best_unique(SweepArgs a, int n_best, unsigned* runner) {
  plane_sweep_body<false, false, true, true>(a, {}, n_best, runner);
}
__global__ void __launch_bounds__(256) k_plane_sweep_best_census_unique(SweepArgs a, int n_best, unsigned* runner) {
  plane_sweep_body<false, true, true, true>(a, {}, n_best, runner);
}
// ... and the first stage of the semi-global sweep (§19; ekf_dense_sgm.hpp has what follows it)
__global__ void __launch_bounds__(256) k_sweep_volume(SweepArgs a, SweepVolume vol) { plane_sweep_body<true, false, false, false>(a, vol, 0, nullptr); }
__global__ void __launch_bounds__(256) k_sweep_volume_census(SweepArgs a, SweepVolume vol) { plane_sweep_body<true, true, false, false>(a, vol, 0, nullptr); }
__global__ void __launch_bounds__(256) k_sweep_volume_best(SweepArgs a, SweepVolume vol, int n_best) {
  plane_sweep_body<true, false, true, false>(a, vol, n_best, nullptr);
}
__global__ void __launch_bounds__(256) k_sweep_volume_best_census(SweepArgs a, SweepVolume vol, int n_best) {
  plane_sweep_body<true, true, true, false>(a, vol, n_best, nullptr);
}

struct FilterArgs {
  const float* depth;                 // the reference view's depth (swept, or filtered for the points of a filtered map)
  const int* plane;
  float* out_depth;                   // NULL: no filter output
  int* out_plane;
  double* xyz;                        // NULL: no points
  int W, H, n_src, min_agree;         // n_src = 0: the depth passes through
  double rel_tol;
  double fx, fy, cx, cy;
  double R[9], t[3];                  // the reference view's pose (the points only)
  DenseSrc s[kDenseMaxSrc];
};

// The uniqueness test of §22.1 on the reference view's own pixel, in 64-bit integers: passed iff there is no runner-up or
// (C2 - C1) 100 >= u C2.  u = 0 passes everything, a flat curve (C2 = C1) fails every u > 0: also the curve that is 0 on
// every plane, the untextured patch itself, which the inequality alone would pass as 0 >= 0.
__device__ __forceinline__ bool unique_pass(unsigned c1, unsigned c2, int u) {
  const bool margin = ((long long)c2 - (long long)c1) * 100ll >= (long long)u * (long long)c2;
  return c2 == kRunnerAbsent || (margin && (u == 0 || c2 != c1));
}

// One lane per pixel: the geometric filter against the swept depths of the sources, and / or the back-projection.
// UNIQUE (§22): a pixel is kept iff it was kept before and unique_pass(cost, runner, uniqueness) of the reference's maps.
template <bool UNIQUE>
__device__ __forceinline__ void depth_filter_points_body(FilterArgs a, const unsigned* cost, const unsigned* runner, int uniqueness) {
#pragma clang fp contract(off)
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned npix = (unsigned)a.W * (unsigned)a.H;
  if (i >= npix) return;
  const int Y = (int)(i / (unsigned)a.W), X = (int)(i % (unsigned)a.W);
  const float zf = a.depth[i];
  const double z = (double)zf;
  const double x = ((double)X - a.cx) / a.fx;
  const double y = ((double)Y - a.cy) / a.fy;
  bool keep = zf > 0.f;
  if (keep && a.n_src > 0) {
    int agree = 0;
    for (int v = 0; v < a.n_src; ++v) {
      const DenseSrc& s = a.s[v];
      const double a0 = s.A[0] * x + s.A[1] * y + s.A[2];
      const double a1 = s.A[3] * x + s.A[4] * y + s.A[5];
      const double a2 = s.A[6] * x + s.A[7] * y + s.A[8];
      const double Q0 = z * a0 + s.b[0];
      const double Q1 = z * a1 + s.b[1];
      const double Q2 = z * a2 + s.b[2];
      if (!(Q2 > 0.0)) continue;
      const double sx = s.fx * (Q0 / Q2) + s.cx;
      const double sy = s.fy * (Q1 / Q2) + s.cy;
      const double fjx = floor(sx + 0.5), fjy = floor(sy + 0.5);
      if (!(fjx >= 0.0 && fjx <= (double)(a.W - 1) && fjy >= 0.0 && fjy <= (double)(a.H - 1))) continue;
      const double zs = (double)s.depth[(size_t)(int)fjy * a.W + (int)fjx];
      if (zs != 0.0 && fabs(Q2 - zs) <= a.rel_tol * Q2) ++agree;
    }
    keep = agree >= a.min_agree;
  }
  if constexpr (UNIQUE) keep = keep && unique_pass(cost[i], runner[i], uniqueness);
  if (a.out_depth) {
    a.out_depth[i] = keep ? zf : 0.f;
    a.out_plane[i] = keep ? a.plane[i] : -1;
  }
  if (a.xyz) {
    const double nan = __builtin_nan("");
    const double p0 = z * x, p1 = z * y, p2 = z;
    double* o = a.xyz + (size_t)i * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = keep ? a.R[3 * c] * p0 + a.R[3 * c + 1] * p1 + a.R[3 * c + 2] * p2 + a.t[c] : nan;
  }
}

__global__ void __launch_bounds__(256) k_depth_filter_points(FilterArgs a) { depth_filter_points_body<false>(a, nullptr, nullptr, 0); }
__global__ void __launch_bounds__(256) k_depth_filter_unique(FilterArgs a, const unsigned* cost, const unsigned* runner, int uniqueness) {
  depth_filter_points_body<true>(a, cost, runner, uniqueness);
}

// ---- colour views --------------------------------------------------------------------------------------------
struct GreyArgs {
  const unsigned char* bgr;           // npix x 3 bytes, tight, 4-byte aligned: B, G, R
  unsigned char* grey;                // npix bytes, tight, 4-byte aligned
  unsigned npix;
};

// The grey image the sweep reads, from a slot's colour image: one lane takes 4 consecutive pixels (three dword loads, one
// dword store: the image is one flat run of pixels), the lane after the last full group takes the up to 3 pixels that are
// left byte by byte.  No byte beyond 3 npix is read: the last word load ends at byte 12 (npix / 4) <= 3 npix.
__global__ void __launch_bounds__(256) k_bgr_to_grey(GreyArgs a) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  const unsigned nvec = a.npix >> 2;
  if (i < nvec) {
    const unsigned* s = reinterpret_cast<const unsigned*>(a.bgr) + 3 * (size_t)i;
    const unsigned w[3] = {s[0], s[1], s[2]};
    unsigned out = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) out |= bgr2gray(byte_of(w, 3 * j), byte_of(w, 3 * j + 1), byte_of(w, 3 * j + 2)) << (8 * j);
    reinterpret_cast<unsigned*>(a.grey)[i] = out;
  } else if (i == nvec) {
    for (unsigned p = nvec * 4u; p < a.npix; ++p)
      a.grey[p] = (unsigned char)bgr2gray(a.bgr[3 * (size_t)p], a.bgr[3 * (size_t)p + 1], a.bgr[3 * (size_t)p + 2]);
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
// pose7 = (t, q = (w x y z)) -> t, R (camera to world, x_cam = R^T (X - t)) and q / |q|.  false: non-finite, or q = 0.
inline bool dense_pose(const double* p, double t[3], double R[9], double q[4]) {
#pragma clang fp contract(off)
  for (int i = 0; i < 7; ++i)
    if (!std::isfinite(p[i])) return false;
  const double n = std::sqrt(p[3] * p[3] + p[4] * p[4] + p[5] * p[5] + p[6] * p[6]);
  if (!(n > 0.0) || !std::isfinite(n)) return false;
  const double w = p[3] / n, x = p[4] / n, y = p[5] / n, z = p[6] / n;
  t[0] = p[0]; t[1] = p[1]; t[2] = p[2];
  q[0] = w; q[1] = x; q[2] = y; q[3] = z;
  R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - z * w);       R[2] = 2.0 * (x * z + y * w);
  R[3] = 2.0 * (x * y + z * w);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - x * w);
  R[6] = 2.0 * (x * z - y * w);       R[7] = 2.0 * (y * z + x * w);       R[8] = 1.0 - 2.0 * (x * x + y * y);
  return true;
}

// A view as the host holds it: K = (fx fy cx cy) and the t and R of dense_pose.
struct DenseCam {
  const double *K, *t, *R;
};

// A (row-major), b and K of source view s seen from reference view r
inline void dense_relative(const DenseCam& r, const DenseCam& s, DenseSrc& o) {
#pragma clang fp contract(off)
  const double d[3] = {r.t[0] - s.t[0], r.t[1] - s.t[1], r.t[2] - s.t[2]};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) o.A[3 * i + j] = s.R[i] * r.R[j] + s.R[3 + i] * r.R[3 + j] + s.R[6 + i] * r.R[6 + j];
    o.b[i] = s.R[i] * d[0] + s.R[3 + i] * d[1] + s.R[6 + i] * d[2];
  }
  o.fx = s.K[0]; o.fy = s.K[1]; o.cx = s.K[2]; o.cy = s.K[3];
}

// The arguments of a sweep of view cam[0] against cam[1 .. n_src], but for the pointers, which the caller adds.
inline SweepArgs sweep_args(const DenseCam* cam, int n_src, int W, int H, int D, int radius, int trunc, double w_min, double w_max) {
#pragma clang fp contract(off)
  SweepArgs a{};
  a.W = W; a.H = H; a.D = D; a.radius = radius; a.trunc = trunc; a.n_src = n_src;
  a.fx = cam[0].K[0]; a.fy = cam[0].K[1]; a.cx = cam[0].K[2]; a.cy = cam[0].K[3];
  a.w_min = w_min;
  a.step = (w_max - w_min) / (double)(D - 1);
  for (int i = 0; i < n_src; ++i) dense_relative(cam[0], cam[1 + i], a.s[i]);
  return a;
}

#ifndef EKF_KERNELS_ONLY
// timed kinds of §22: k_plane_sweep_unique, k_plane_sweep_census_unique, k_plane_sweep_best_unique,
// k_plane_sweep_best_census_unique, k_sgm_winner_unique, k_depth_filter_unique
constexpr int kUniqueKinds = 6;

struct DenseView {
  DevBuf<unsigned char> img;
  DevBuf<unsigned char> bgr;          // W x H x 3, tight: the colour image `img` was derived from (colour = true only)
  DevBuf<float> depth, fdepth;
  DevBuf<int> plane, fplane;
  DevBuf<unsigned> cost;
  DevBuf<unsigned char> nviews;
  DevBuf<unsigned long long> census;  // W x H descriptors of `img` (§20), allocated by the slot's first census sweep or getter
  DevBuf<unsigned> runner;            // W x H runner-up costs (§22), allocated by the slot's first sweep that keeps them
  double K[4] = {}, t[3] = {}, R[9] = {}, q[4] = {};
  bool set = false;                   // an image, K and a pose
  bool colour = false;                // `bgr` holds the slot's image in colour (§18): every grey setter drops it
  bool swept = false;                 // swept since the image or the pose last changed
  bool filtered = false;              // filtered since it was last swept
  bool sgm = false;                   // the handle's cost volumes are those of this slot's maps (§19: DenseSgm)
  bool census_valid = false;          // `census` is that of `img`: every setter of the image clears it, a new pose does not
  bool has_runner = false;            // `runner` belongs to the slot's swept maps (§22): cleared wherever `swept` is
  bool seg = false;                   // the handle's segment planes are those of this slot's filtered map (§23: DenseSpeckle):
                                      // cleared wherever `filtered` is
  DenseCam cam() const { return {K, t, R}; }
};

// Host side of one handle (`ekf_dense`).  Everything runs on the default stream of the handle's device, as the rectified
// getters of a key-frame selector do (§14.4): a view may come from a selector that outlives its filter.
struct DenseStereo {
  std::string err;
  int device = 0, W = 0, H = 0, max_views = 0;
  std::vector<DenseView> v;
  DevBuf<double> d_xyz;               // the points on their way to the host (allocated by the first ekf_dense_get_points)
  KernelTimer<2> timer;               // k_plane_sweep, k_depth_filter_points
  KernelTimer<3> census_timer;        // k_census, k_plane_sweep_census, k_sweep_volume_census (§20)
  KernelTimer<4> best_timer;          // k_plane_sweep_best, .._best_census, k_sweep_volume_best, .._best_census (§21)
  KernelTimer<kUniqueKinds> unique_timer;   // the twins of §22, in the order of kUniqueKinds' comment
  bool keep_runner = false;           // ekf_dense_keep_runner_up: every sweep launches its twin and records the runner-up

  size_t npix() const { return (size_t)W * H; }
  const unsigned char* colour_of(int slot) const { return v[slot].colour ? (const unsigned char*)v[slot].bgr : nullptr; }

  // v.bgr -> v.img: the one launch of k_bgr_to_grey, enqueued on the default stream.
  hipError_t grey_from_colour(DenseView& vw) {
    const GreyArgs a{vw.bgr, vw.img, (unsigned)npix()};
    const unsigned groups = a.npix / 4u + 1u;
    k_bgr_to_grey<<<(groups + 255u) / 256u, 256, 0, nullptr>>>(a);
    return hipGetLastError();
  }
  ~DenseStereo() {                    // the members (events, buffers) go after this body, on the handle's device
    if (max_views) hipSetDevice(device);
  }

  // A (row-major) and b of source view s seen from reference view r
  void relative(const DenseView& r, const DenseView& s, DenseSrc& o) const {
    dense_relative(r.cam(), s.cam(), o);
    source_pointers(s, o);
  }
  // ... and what a kernel reads of source view s
  static void source_pointers(const DenseView& s, DenseSrc& o) {
    o.img = s.img;
    o.census = s.census;
    o.depth = s.depth;
  }

  // The descriptor buffers of a census sweep (§20), before anything is marked stale: a failed allocation leaves every map.
  hipError_t census_reserve(int ref, const int* src, int n_src) {
    hipError_t e = v[ref].census.reserve(npix());
    for (int i = 0; i < n_src && e == hipSuccess; ++i) e = v[src[i]].census.reserve(npix());
    if (e != hipSuccess) (void)hipGetLastError();
    return e;
  }

  // The slot's descriptors, if they are not those of its image: one launch of k_census (the buffer exists).
  hipError_t census_update(int slot) {
    DenseView& vw = v[slot];
    if (vw.census_valid) return hipSuccess;
    const CensusArgs a{vw.img, vw.census, W, H};
    const dim3 grid((unsigned)((W + kDenseTW - 1) / kDenseTW), (unsigned)((H + kDenseTH - 1) / kDenseTH));
    const hipError_t e = census_timer.run(0, [&] { k_census<<<grid, 256, 0, nullptr>>>(a); });
    vw.census_valid = e == hipSuccess;
    return e;
  }

  // ... of the reference and then of every source, in their order
  hipError_t census_update(int ref, const int* src, int n_src) {
    hipError_t e = census_update(ref);
    for (int i = 0; i < n_src && e == hipSuccess; ++i) e = census_update(src[i]);
    return e;
  }

  // The one launch of k_depth_filter_points.  n_src > 0: the filter of view `ref` (swept -> filtered); xyz: the points of
  // its swept or filtered map, into d_xyz.  uniqueness > 0 (§22; with n_src > 0, on a slot with a runner-up map): the one
  // launch is k_depth_filter_unique's.
  hipError_t filter_points(int ref, const int* src, int n_src, double rel_tol, int min_agree, bool from_filtered, bool xyz,
                           int uniqueness = 0) {
    DenseView& r = v[ref];
    hipError_t e;
    const size_t n = npix();
    FilterArgs a{};
    a.depth = from_filtered ? r.fdepth : r.depth;
    a.plane = from_filtered ? r.fplane : r.plane;
    if (n_src > 0) {
      if ((e = r.fdepth.reserve(n)) != hipSuccess || (e = r.fplane.reserve(n)) != hipSuccess) return e;
      a.out_depth = r.fdepth;
      a.out_plane = r.fplane;
      r.filtered = r.seg = false;
    }
    if (xyz) {
      if ((e = d_xyz.reserve(n * 3)) != hipSuccess) return e;
      a.xyz = d_xyz;
    }
    a.W = W; a.H = H; a.n_src = n_src; a.min_agree = min_agree; a.rel_tol = rel_tol;
    a.fx = r.K[0]; a.fy = r.K[1]; a.cx = r.K[2]; a.cy = r.K[3];
    for (int i = 0; i < 9; ++i) a.R[i] = r.R[i];
    for (int i = 0; i < 3; ++i) a.t[i] = r.t[i];
    for (int i = 0; i < n_src; ++i) relative(r, v[src[i]], a.s[i]);
    const unsigned wg = (unsigned)((n + 255) / 256);
    const unsigned *c1 = r.cost, *c2 = r.runner;
    e = uniqueness > 0 ? unique_timer.run(5, [&] { k_depth_filter_unique<<<wg, 256, 0, nullptr>>>(a, c1, c2, uniqueness); })
                       : timer.run(1, [&] { k_depth_filter_points<<<wg, 256, 0, nullptr>>>(a); });
    if (e != hipSuccess) return e;
    if (n_src > 0) r.filtered = true;
    return hipSuccess;
  }
};
#endif  // EKF_KERNELS_ONLY

}  // namespace ekf
