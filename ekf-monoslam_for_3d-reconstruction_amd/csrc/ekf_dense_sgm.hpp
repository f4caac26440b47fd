// Semi-global cost aggregation for the dense plane sweep: the windowed cost volume of k_plane_sweep written
// to device memory (k_sweep_volume: the same body, ekf_dense_stereo.hpp), summed along 4 or 8 path directions
// (k_sgm_path, one launch per direction) and its winner taken (k_sgm_winner) into the four maps of the slot that
// k_plane_sweep writes.  Integers throughout; tests/sgm_oracle.py restates the contract in numpy.
//
// Both cost volumes keep the planes of a pixel side by side, element (y W + x) D + d: the aggregation, whose lanes are the
// planes of ONE pixel and which makes 8 passes over both volumes, then loads and stores whole cache lines; the volume sweep
// pays with stores D words apart and the host getter with a transposition (§19.2 has the measurement behind the choice).
// The valid-view counts, which only the winner reads, one byte a pixel, stay plane-major.
#pragma once
#include "ekf_dense_stereo.hpp"

namespace ekf {

constexpr int kSgmMaxPenalty = 1 << 20;
constexpr long long kSgmMaxElems = 1LL << 28;    // W H D of one volume: 1 GiB of unsigned (the cap of the fusion volume)
constexpr int kSgmBig = 0x3fffffff;              // "no such plane": + P1 still fits an int
constexpr int kSgmAhead = 4;                     // pixels of a line whose C (and S) are in flight ahead of the chain
constexpr int kSgmKinds = 10;                    // timed kinds: the volume sweep, directions r0 .. r7, the winner

// The (dx, dy) of §19.1, in their order; paths = 4 takes the first four.
constexpr int kSgmDir[8][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}, {1, 1}, {-1, -1}, {1, -1}, {-1, 1}};

__global__ void __launch_bounds__(256) k_sweep_volume(SweepArgs a, SweepVolume vol) { plane_sweep_body<true>(a, vol); }
__global__ void __launch_bounds__(256) k_sweep_volume_census(SweepArgs a, SweepVolume vol) { plane_sweep_body<true, true>(a, vol); }

// What a lane of k_sgm_path takes from other lanes of its wave (every lane of the wave makes each call):
//   wave_read(v, src)  v of lane src (ds_bpermute; once a launch, for the longest line of the wave);
//   lane_below(v)      v of lane - 1, lane_above(v): v of lane + 1 (lane 0 / 63: its own v) -- one DPP move each;
//   group_min<G>(v)    the least v of the lane's aligned group of G = 16 or 64 lanes, in every lane of it: four DPP moves
//                      inside the row of 16 (two quad permutations, the mirror of 8, the mirror of 16: after each, twice
//                      as many lanes agree), then for 64 a ds_swizzle (lane ^ 16) and a ds_bpermute (lane ^ 32).
// These sit on the serial chain of a line, once a pixel: with ds_bpermute for all of them the eight directions took 1.74 ms
// against 1.49 ms at 640 x 480 with 128 planes, and 0.65 against 0.46 ms at 320 x 240 with 64 (§19.5).  The host check has wave_read from its shim (tools/host_kernels.hpp: an exchange array and a barrier a wave)
// and the other two written on top of it.
#ifndef EKF_KERNELS_ONLY
__device__ __forceinline__ int wave_read(int v, int src) { return __shfl(v, src, 64); }
template <int CTRL>
__device__ __forceinline__ int dpp_move(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xf, 0xf, false); }
__device__ __forceinline__ int lane_below(int v) { return dpp_move<0x138>(v); }                 // wave_shr:1
__device__ __forceinline__ int lane_above(int v) { return dpp_move<0x130>(v); }                 // wave_shl:1
template <int G>
__device__ __forceinline__ int group_min(int v) {
  static_assert(G == 16 || G == 64, "a row of 16 lanes or the wave");
  v = min(v, dpp_move<0xB1>(v));                                            // quad_perm [1, 0, 3, 2]
  v = min(v, dpp_move<0x4E>(v));                                            // quad_perm [2, 3, 0, 1]
  v = min(v, dpp_move<0x141>(v));                                           // row_half_mirror
  v = min(v, dpp_move<0x140>(v));                                           // row_mirror
  if (G == 64) {
    v = min(v, __builtin_amdgcn_ds_swizzle(v, 0x401F));                     // lane ^ 16
    v = min(v, __shfl_xor(v, 32, 64));
  }
  return v;
}
#else
inline int lane_below(int v) {
  const int lane = (int)threadIdx.x & 63, got = wave_read(v, (lane + 63) & 63);
  return lane == 0 ? v : got;
}
inline int lane_above(int v) {
  const int lane = (int)threadIdx.x & 63, got = wave_read(v, (lane + 1) & 63);
  return lane == 63 ? v : got;
}
template <int G>
inline int group_min(int v) {
  for (int off = 1; off < G; off <<= 1) v = min(v, wave_read(v, ((int)threadIdx.x & 63) ^ off));
  return v;
}
#endif

struct SgmPathArgs {
  const unsigned* C;                  // the raw volume
  unsigned* S;                        // the aggregate: written by the first direction, added to by the later ones
  int W, H, D, p1, p2, dx, dy;
};

// One direction.  A line is the run of pixels from a border pixel (p - r outside the image) along r; G lanes walk one line,
// lane g of them carrying the NP planes g NP .. g NP + NP - 1 in registers, so a wave takes 64 / G lines and a workgroup
// 256 / G.  Per pixel: m of the previous pixel by group_min over the G lanes, the d - 1 / d + 1 neighbours from the lane's
// own registers and, at its two ends, from the lanes beside it.  C and S of the pixel kSgmAhead steps on are requested before the step's arithmetic: they do
// not depend on L, the chain never waits for memory.  Every (pixel, plane) belongs to one lane of one line of the launch:
// plain loads and stores, FIRST writes S and the later directions add to it.
//   L(first pixel) = C falls out of the recurrence with L(before) = 0 and m = 0: min(0, P1, P1, P2) - 0 = 0.
//   Lanes without a plane (d >= D) hold kSgmBig and load / store nothing of their own (their loads are clamped to element 0);
//   the lanes of a line that has ended idle the same way until the longest line of the wave is done.
template <int G, int NP, bool FIRST>
__global__ void __launch_bounds__(256) k_sgm_path(SgmPathArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, g = lane & (G - 1);
  const int W = a.W, H = a.H, D = a.D;
  const bool diag = a.dx != 0 && a.dy != 0;
  const int nlines = diag ? W + H - 1 : (a.dy == 0 ? H : W);
  const int line = ((int)blockIdx.x * 4 + (tid >> 6)) * (64 / G) + lane / G;
  // the line in mirrored coordinates (u, v), where every direction walks towards larger u and / or v
  int u0 = 0, v0 = 0, len = 0;
  if (line < nlines) {
    if (diag) {
      const int c = line - (H - 1);
      u0 = max(c, 0); v0 = max(-c, 0);
      len = min(W - u0, H - v0);
    } else if (a.dy == 0) {
      v0 = line; len = W;
    } else {
      u0 = line; len = H;
    }
  }
  const int x0 = a.dx < 0 ? W - 1 - u0 : u0, y0 = a.dy < 0 ? H - 1 - v0 : v0;
  const long stride = ((long)a.dy * W + a.dx) * D;                          // elements from a pixel of the line to the next
  int steps = len;                                                          // the longest line of the wave
#pragma unroll
  for (int off = G; off < 64; off <<= 1) steps = max(steps, wave_read(steps, lane ^ off));

  const long base = ((long)y0 * W + x0) * D + g * NP;                       // element of (first pixel, first plane of the lane)
  bool has[NP];
  int L[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    has[j] = g * NP + j < D && len > 0;
    L[j] = g * NP + j < D ? 0 : kSgmBig;
  }
  int m = 0;

  unsigned c[kSgmAhead][NP], s[kSgmAhead][NP];
  auto request = [&](int slot, int t) {
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const long e = (has[j] && t < len) ? base + j + (long)t * stride : 0;
      c[slot][j] = a.C[e];
      s[slot][j] = FIRST ? 0u : a.S[e];
    }
  };
#pragma unroll
  for (int q = 0; q < kSgmAhead; ++q) request(q, q);

  for (int t0 = 0; t0 < steps; t0 += kSgmAhead) {
#pragma unroll
    for (int q = 0; q < kSgmAhead; ++q) {
      const int t = t0 + q;
      unsigned cq[NP], sq[NP];
#pragma unroll
      for (int j = 0; j < NP; ++j) { cq[j] = c[q][j]; sq[j] = s[q][j]; }
      request(q, t + kSgmAhead);
      // the neighbours beyond the lane's own planes
      int below = lane_below(L[NP - 1]), above = lane_above(L[0]);
      below = g == 0 ? kSgmBig : below;
      above = g == G - 1 ? kSgmBig : above;
      const int far = m + a.p2;
      int Ln[NP], lo = kSgmBig;
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        const int dn = j == 0 ? below : L[max(j - 1, 0)], up = j == NP - 1 ? above : L[min(j + 1, NP - 1)];
        const int best = min(min(L[j], far), min(dn, up) + a.p1);
        Ln[j] = L[j] == kSgmBig ? kSgmBig : (int)cq[j] + best - m;
        lo = min(lo, Ln[j]);
      }
      m = group_min<G>(lo);
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        L[j] = Ln[j];
        if (has[j] && t < len) a.S[base + j + (long)t * stride] = sq[j] + (unsigned)Ln[j];
      }
    }
  }
}

struct SgmWinnerArgs {
  const unsigned* S;
  const unsigned char* V;
  SweepArgs out;                      // depth, plane, cost, views, W, H, D, w_min, step: what sweep_write_winner reads
};

// One lane per pixel over the aggregate: the winner update of k_plane_sweep (selects), V of the winning plane from the
// stored counts, and the same write.  The lanes of a wave read D words apart, but a lane's next 31 planes lie in the cache
// line it has just touched.
// RUNNER: the twin that also writes the runner-up of §22, C2 = min { S_k : |k - k*| > 1 } (kRunnerAbsent where D <= 3 leaves
// no such plane), in the same pass by the four smallest keys of the pixel-wise sweeps; S < 2^24 and k < 1024 make a 34-bit
// key, a long long.  (A second pass with a masked min, k* being known by then, read the volume twice, and the compiler made
// of the mask a branch round every load: 0.458 ms beside k_sgm_winner's 0.062 ms at 640 x 480 with 128 planes, §22.5.)
template <bool RUNNER>
__device__ __forceinline__ void sgm_winner_body(const SgmWinnerArgs& a, unsigned* runner) {
  const size_t n = (size_t)a.out.W * a.out.H;
  const size_t o = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (o >= n) return;
  long long top[kRunnerKeys];                                               // RUNNER only
  if constexpr (RUNNER) {
#pragma unroll
    for (int i = 0; i < kRunnerKeys; ++i) top[i] = runner_none<long long>();
  }
  int prev = 0, bestC = INT_MAX, bestK = -2, bestM = 0, bestP = 0;
#pragma unroll 8
  for (int k = 0; k < a.out.D; ++k) {
    const int C = (int)a.S[o * (size_t)a.out.D + (size_t)k];               // < 2^24
    const bool pending = bestK == k - 1, better = C < bestC;
    bestP = (pending || better) ? C : bestP;
    bestM = better ? prev : bestM;
    bestK = better ? k : bestK;
    bestC = better ? C : bestC;
    prev = C;
    if constexpr (RUNNER) runner_insert(top, ((long long)C << 10) | k);
  }
  sweep_write_winner(a.out, o, bestK, bestM, bestC, bestP, (int)a.V[(size_t)bestK * n + o]);
  if constexpr (RUNNER) runner[o] = runner_take(top);
}

__global__ void __launch_bounds__(256) k_sgm_winner(SgmWinnerArgs a) { sgm_winner_body<false>(a, nullptr); }
__global__ void __launch_bounds__(256) k_sgm_winner_unique(SgmWinnerArgs a, unsigned* runner) { sgm_winner_body<true>(a, runner); }

// A cost volume as the host getter delivers it: plane-major, D x H x W.
inline void sgm_volume_to_planes(const unsigned* vol, unsigned* out, size_t npix, int D) {
  for (int d = 0; d < D; ++d)
    for (size_t p = 0; p < npix; ++p) out[(size_t)d * npix + p] = vol[p * (size_t)D + (size_t)d];
}

#ifndef EKF_KERNELS_ONLY
// The planes a lane carries for D planes on G lanes, and the launch of one direction.
template <int G, int NP>
inline void sgm_launch_path(const SgmPathArgs& a, bool first, unsigned grid) {
  if (first)
    k_sgm_path<G, NP, true><<<grid, 256, 0, nullptr>>>(a);
  else
    k_sgm_path<G, NP, false><<<grid, 256, 0, nullptr>>>(a);
}

// Host side of the semi-global sweep of one handle: one raw and one aggregated volume (and the valid-view counts), grow-only,
// and a timer of its own.  DenseView::sgm says which slot, if any, the volumes belong to.
struct DenseSgm {
  DevBuf<unsigned> C, S;
  DevBuf<unsigned char> V;
  int D = 0;                          // planes of the volumes' sweep
  KernelTimer<kSgmKinds> timer;

  hipError_t sweep(DenseStereo& d, int ref, const int* src, int n_src, double w_min, double w_max, int D_, int radius, int trunc,
                   int p1, int p2, int paths, bool census = false, int n_best = 0) {
#pragma clang fp contract(off)
    DenseView& r = d.v[ref];
    hipError_t e;
    const size_t n = d.npix(), elems = n * (size_t)D_;
    for (DenseView& v : d.v) v.sgm = false;                                 // the volumes are about to change hands
    if ((e = r.depth.reserve(n)) != hipSuccess || (e = r.plane.reserve(n)) != hipSuccess ||
        (e = r.cost.reserve(n)) != hipSuccess || (e = r.nviews.reserve(n)) != hipSuccess ||
        (e = C.reserve(elems)) != hipSuccess || (e = S.reserve(elems)) != hipSuccess || (e = V.reserve(elems)) != hipSuccess ||
        (d.keep_runner && (e = r.runner.reserve(n)) != hipSuccess)) {
      (void)hipGetLastError();                                              // the slot's maps are as they were
      return e;
    }
    if (census && ((e = d.census_reserve(ref, src, n_src)) != hipSuccess || (e = d.census_update(ref, src, n_src)) != hipSuccess)) return e;
    SweepArgs a{};
    a.ref = r.img; a.ref_census = r.census; a.depth = r.depth; a.plane = r.plane; a.cost = r.cost; a.views = r.nviews;
    a.W = d.W; a.H = d.H; a.D = D_; a.radius = radius; a.trunc = trunc; a.n_src = n_src;
    a.fx = r.K[0]; a.fy = r.K[1]; a.cx = r.K[2]; a.cy = r.K[3];
    a.w_min = w_min;
    a.step = (w_max - w_min) / (double)(D_ - 1);
    for (int i = 0; i < n_src; ++i) d.relative(r, d.v[src[i]], a.s[i]);
    r.swept = r.filtered = r.has_runner = r.seg = false;
    const SweepVolume vol{C, V};
    const dim3 grid((unsigned)((d.W + kDenseTW - 1) / kDenseTW), (unsigned)((d.H + kDenseTH - 1) / kDenseTH));
    // the census volume (§20) counts under the census profile, its directions and winner below like any other
    // and the volume of the n_best cheapest sources (§21; n_best = 0: of all of them) under the best profile
    if (n_best > 0)
      e = census ? d.best_timer.run(3, [&] { k_sweep_volume_best_census<<<grid, 256, 0, nullptr>>>(a, vol, n_best); })
                 : d.best_timer.run(2, [&] { k_sweep_volume_best<<<grid, 256, 0, nullptr>>>(a, vol, n_best); });
    else
      e = census ? d.census_timer.run(2, [&] { k_sweep_volume_census<<<grid, 256, 0, nullptr>>>(a, vol); })
                 : timer.run(0, [&] { k_sweep_volume<<<grid, 256, 0, nullptr>>>(a, vol); });
    if (e != hipSuccess) return e;
    for (int i = 0; i < paths; ++i) {
      const SgmPathArgs p{C, S, d.W, d.H, D_, p1, p2, kSgmDir[i][0], kSgmDir[i][1]};
      const bool diag = p.dx != 0 && p.dy != 0;
      const int nlines = diag ? d.W + d.H - 1 : (p.dy == 0 ? d.H : d.W);
      const int G = D_ <= 16 ? 16 : 64;
      const unsigned wg = (unsigned)((nlines + 256 / G - 1) / (256 / G));
      const int np = (D_ + 63) / 64;                                        // planes per lane at G = 64: 1 .. 16
      e = timer.run(1 + i, [&] {
        if (G == 16) sgm_launch_path<16, 1>(p, i == 0, wg);
        else if (np <= 1) sgm_launch_path<64, 1>(p, i == 0, wg);
        else if (np <= 2) sgm_launch_path<64, 2>(p, i == 0, wg);
        else if (np <= 4) sgm_launch_path<64, 4>(p, i == 0, wg);
        else if (np <= 8) sgm_launch_path<64, 8>(p, i == 0, wg);
        else sgm_launch_path<64, 16>(p, i == 0, wg);
      });
      if (e != hipSuccess) return e;
    }
    const SgmWinnerArgs w{S, V, a};
    unsigned* const ru = r.runner;
    const unsigned wg_w = (unsigned)((n + 255) / 256);
    e = d.keep_runner ? d.unique_timer.run(4, [&] { k_sgm_winner_unique<<<wg_w, 256, 0, nullptr>>>(w, ru); })   // §22
                      : timer.run(9, [&] { k_sgm_winner<<<wg_w, 256, 0, nullptr>>>(w); });
    if (e != hipSuccess) return e;
    D = D_;
    r.swept = r.sgm = true;
    r.has_runner = d.keep_runner;
    return hipSuccess;
  }
};
#endif  // EKF_KERNELS_ONLY

}  // namespace ekf
