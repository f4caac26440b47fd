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
  SweepWinner<RUNNER, long long> win;
#pragma unroll 8
  for (int k = 0; k < a.out.D; ++k) win.step(k, (int)a.S[o * (size_t)a.out.D + (size_t)k]);      // < 2^24
  win.write(a.out, o, (int)a.V[(size_t)win.K * n + o], runner);
}

__global__ void __launch_bounds__(256) k_sgm_winner(SgmWinnerArgs a) { sgm_winner_body<false>(a, nullptr); }
__global__ void __launch_bounds__(256) k_sgm_winner_unique(SgmWinnerArgs a, unsigned* runner) { sgm_winner_body<true>(a, runner); }

// A cost volume as the host getter delivers it: plane-major, D x H x W.
inline void sgm_volume_to_planes(const unsigned* vol, unsigned* out, size_t npix, int D) {
  for (int d = 0; d < D; ++d)
    for (size_t p = 0; p < npix; ++p) out[(size_t)d * npix + p] = vol[p * (size_t)D + (size_t)d];
}

// ---- the launches of a sweep ---------------------------------------------------------------------------------
// The timed kinds: a pixel-wise sweep is kSweep + 4 (it keeps the runner-up) + 2 (n_best > 0) + 1 (census), a volume sweep
// kVolume + 2 (n_best > 0) + 1 (census), direction i of kSgmDir is kSgmPath + i.
enum SweepKind {
  kSweep, kSweepCensus, kSweepBest, kSweepBestCensus, kSweepUnique, kSweepCensusUnique, kSweepBestUnique, kSweepBestCensusUnique,
  kVolume, kVolumeCensus, kVolumeBest, kVolumeBestCensus,
  kSgmPath, kSgmWinner = kSgmPath + 8, kSgmWinnerUnique
};
struct SweepGrid {
  unsigned x, y;                      // workgroups of 256 lanes
};
struct SweepMode {
  bool census;                        // the census cost (§20), not absolute differences
  int n_best;                         // 0: the sum over all sources; 1 .. n_src: over the cheapest per pixel and plane (§21)
  unsigned* runner;                   // where the runner-up goes (§22); NULL: nowhere
  int paths, p1, p2;                  // paths = 0: the pixel-wise sweep; 4 or 8: the semi-global one (§19)
};

// One direction: G lanes a line and NP planes a lane for D planes, a workgroup for 256 / G lines.
template <bool FIRST, typename Go>
auto sgm_path_launch(Go& go, int kind, const SgmPathArgs& p) {
  const bool diag = p.dx != 0 && p.dy != 0;
  const int nlines = diag ? p.W + p.H - 1 : (p.dy == 0 ? p.H : p.W);
  const int G = p.D <= 16 ? 16 : 64;
  const SweepGrid grid{(unsigned)((nlines + 256 / G - 1) / (256 / G)), 1};
  const int np = (p.D + 63) / 64;                                           // planes per lane at G = 64: 1 .. 16
  if (G == 16) return go(kind, grid, k_sgm_path<16, 1, FIRST>, p);
  if (np <= 1) return go(kind, grid, k_sgm_path<64, 1, FIRST>, p);
  if (np <= 2) return go(kind, grid, k_sgm_path<64, 2, FIRST>, p);
  if (np <= 4) return go(kind, grid, k_sgm_path<64, 4, FIRST>, p);
  if (np <= 8) return go(kind, grid, k_sgm_path<64, 8, FIRST>, p);
  return go(kind, grid, k_sgm_path<64, 16, FIRST>, p);
}

// Every launch of one sweep, in order, each made by go(kind, grid, kernel, args...): which of the twelve sweep kernels, and
// for the semi-global sweep every direction's instantiation of k_sgm_path and the winner or its twin, with their grids.  This
// is the one place that decides them: the library's go times and launches, the host checks' go (tools/host_kernels.hpp) runs
// the kernel on the host.  It returns what go returns, whose value-initialised value (hipSuccess) means that the launch was
// made, and stops at the first that was not.  `vol` and `S` are read with paths > 0 alone.
template <typename Go>
auto sweep_launches(const SweepArgs& a, const SweepVolume& vol, unsigned* S, const SweepMode& m, Go go) {
  const SweepGrid tiles{(unsigned)((a.W + kDenseTW - 1) / kDenseTW), (unsigned)((a.H + kDenseTH - 1) / kDenseTH)};
  const int sub = (m.n_best > 0 ? 2 : 0) + (m.census ? 1 : 0), nb = m.n_best;
  unsigned* const ru = m.runner;
  if (m.paths == 0) {
    switch (kSweep + (ru ? 4 : 0) + sub) {
      case kSweep: return go(kSweep, tiles, k_plane_sweep, a);
      case kSweepCensus: return go(kSweepCensus, tiles, k_plane_sweep_census, a);
      case kSweepBest: return go(kSweepBest, tiles, k_plane_sweep_best, a, nb);
      case kSweepBestCensus: return go(kSweepBestCensus, tiles, k_plane_sweep_best_census, a, nb);
      case kSweepUnique: return go(kSweepUnique, tiles, k_plane_sweep_unique, a, ru);
      case kSweepCensusUnique: return go(kSweepCensusUnique, tiles, k_plane_sweep_census_unique, a, ru);
      case kSweepBestUnique: return go(kSweepBestUnique, tiles, k_plane_sweep_best_unique, a, nb, ru);
      default: return go(kSweepBestCensusUnique, tiles, k_plane_sweep_best_census_unique, a, nb, ru);
    }
  }
  auto e = sub == 0   ? go(kVolume, tiles, k_sweep_volume, a, vol)
           : sub == 1 ? go(kVolumeCensus, tiles, k_sweep_volume_census, a, vol)
           : sub == 2 ? go(kVolumeBest, tiles, k_sweep_volume_best, a, vol, nb)
                      : go(kVolumeBestCensus, tiles, k_sweep_volume_best_census, a, vol, nb);
  const decltype(e) made{};
  for (int i = 0; i < m.paths && e == made; ++i) {
    const SgmPathArgs p{vol.C, S, a.W, a.H, a.D, m.p1, m.p2, kSgmDir[i][0], kSgmDir[i][1]};
    e = i == 0 ? sgm_path_launch<true>(go, kSgmPath, p) : sgm_path_launch<false>(go, kSgmPath + i, p);
  }
  if (!(e == made)) return e;
  const SgmWinnerArgs w{S, vol.V, a};
  const SweepGrid lanes{(unsigned)(((size_t)a.W * a.H + 255) / 256), 1};
  return ru ? go(kSgmWinnerUnique, lanes, k_sgm_winner_unique, w, ru) : go(kSgmWinner, lanes, k_sgm_winner, w);
}

#ifndef EKF_KERNELS_ONLY
// Host side of a sweep of one handle, pixel-wise or semi-global: for the latter one raw and one aggregated volume (and the
// valid-view counts), grow-only, and a timer of its own.  DenseView::sgm says which slot, if any, the volumes belong to.
struct DenseSgm {
  DevBuf<unsigned> C, S;
  DevBuf<unsigned char> V;
  int D = 0;                          // planes of the volumes' sweep
  KernelTimer<kSgmKinds> timer;

  // The launch of one kind under the profile that counts it (the getters' orders of kinds, ekf_capi.hip): a census volume
  // (§20) under the census profile, the volume of the n_best cheapest sources (§21) under the best profile, their directions
  // and winner here like any other, every twin of §22 under the unique profile.
  template <typename F>
  hipError_t timed(DenseStereo& d, int kind, F launch) {
    switch (kind) {
      case kSweep: return d.timer.run(0, launch);
      case kSweepCensus: return d.census_timer.run(1, launch);
      case kSweepBest: case kSweepBestCensus: return d.best_timer.run(kind - kSweepBest, launch);
      case kSweepUnique: case kSweepCensusUnique: case kSweepBestUnique: case kSweepBestCensusUnique:
        return d.unique_timer.run(kind - kSweepUnique, launch);
      case kVolume: return timer.run(0, launch);
      case kVolumeCensus: return d.census_timer.run(2, launch);
      case kVolumeBest: case kVolumeBestCensus: return d.best_timer.run(2 + kind - kVolumeBest, launch);
      case kSgmWinner: return timer.run(9, launch);
      case kSgmWinnerUnique: return d.unique_timer.run(4, launch);
      default: return timer.run(1 + kind - kSgmPath, launch);
    }
  }

  // paths = 0: the pixel-wise sweep of §15 (p1 = p2 = 0; the volumes stay whose they are); 4 or 8: the semi-global one.
  // n_best = 0: the sum over all sources; 1 .. n_src: the n_best cheapest sources per pixel and plane (§21, also for n_src).
  hipError_t sweep(DenseStereo& d, int ref, const int* src, int n_src, double w_min, double w_max, int D_, int radius, int trunc,
                   int p1, int p2, int paths, bool census = false, int n_best = 0) {
    DenseView& r = d.v[ref];
    hipError_t e;
    const size_t n = d.npix(), elems = paths ? n * (size_t)D_ : 0;
    if (paths)
      for (DenseView& v : d.v) v.sgm = false;                               // the volumes are about to change hands
    if ((e = r.depth.reserve(n)) != hipSuccess || (e = r.plane.reserve(n)) != hipSuccess ||
        (e = r.cost.reserve(n)) != hipSuccess || (e = r.nviews.reserve(n)) != hipSuccess ||
        (e = C.reserve(elems)) != hipSuccess || (e = S.reserve(elems)) != hipSuccess || (e = V.reserve(elems)) != hipSuccess ||
        (d.keep_runner && (e = r.runner.reserve(n)) != hipSuccess)) {
      (void)hipGetLastError();                                              // the slot's maps are as they were
      return e;
    }
    if (census && ((e = d.census_reserve(ref, src, n_src)) != hipSuccess || (e = d.census_update(ref, src, n_src)) != hipSuccess)) return e;
    DenseCam cam[1 + kDenseMaxSrc] = {r.cam()};
    for (int i = 0; i < n_src; ++i) cam[1 + i] = d.v[src[i]].cam();
    SweepArgs a = sweep_args(cam, n_src, d.W, d.H, D_, radius, trunc, w_min, w_max);
    a.ref = r.img; a.ref_census = r.census; a.depth = r.depth; a.plane = r.plane; a.cost = r.cost; a.views = r.nviews;
    for (int i = 0; i < n_src; ++i) DenseStereo::source_pointers(d.v[src[i]], a.s[i]);
    r.swept = r.filtered = r.sgm = r.has_runner = r.seg = false;
    const SweepMode m{census, n_best, d.keep_runner ? (unsigned*)r.runner : nullptr, paths, p1, p2};
    e = sweep_launches(a, SweepVolume{C, V}, S, m, [&](int kind, SweepGrid g, auto kernel, const auto&... args) {
      return timed(d, kind, [&] { kernel<<<dim3(g.x, g.y), 256, 0, nullptr>>>(args...); });
    });
    if (e != hipSuccess) return e;
    if (paths) D = D_;
    r.swept = true;
    r.sgm = paths != 0;
    r.has_runner = d.keep_runner;
    return hipSuccess;
  }
};
#endif  // EKF_KERNELS_ONLY

}  // namespace ekf
