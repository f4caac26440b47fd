// Speckle filter of a depth map: the connected segments of its plane map and the removal of the small ones,
// between the geometric filter and the fusion.  Integers only; tests/speckle_oracle.py restates the contract:
//   - a pixel is valid iff plane >= 0; two 4-neighbours are linked iff both are valid and |plane_a - plane_b| <= max_diff
//     (in 64 bits: planes 0 and INT_MAX are "not linked", whatever a host caller passes);
//   - a segment is a connected component of the links, its label the least linear index y W + x of its pixels, its size their
//     number; an invalid pixel has label 0xFFFFFFFF and size 0;
//   - depth = 0, plane = -1 where size < min_size, every other element as it was.
// Labels, sizes and the output are functions of the plane map alone, so the integer atomics below, whose order of arrival
// differs from run to run, cost no bit of the result.
//
// Four launches a call, whatever the image holds, over three width x height planes of unsigned: L (the forest), R (a
// pixel's root: its label) and S (the pixel count at a root):
//   k_speckle_label  one 32 x 16 tile a workgroup: a union-find of the tile in LDS, then L = the global index of a pixel's
//                    root within its tile, S = 0;
//   k_speckle_merge  one lane per pixel on the right or the lower edge of a tile: the union with its neighbour across the
//                    border, in L, between workgroups (the visibility argument stands at the kernel);
//   k_speckle_count  R = the root of L, and S[root] += 1, summed in LDS before it goes to memory;
//   k_speckle_apply  one lane a pixel: its size S[R] (written to L, which nobody reads any more) and the removal.
//
// The forest.  L[x] <= x always; x is a root iff L[x] = x; a word only ever decreases, and only to the index of a pixel of
// the same segment, or of one that the writing lane is in the course of uniting with it.  seg_find walks x, L[x], L[L[x]],
// ..., a strictly decreasing sequence of indices, to a root; seg_union finds both roots and hooks the larger to the smaller
// with fetch_min.  If the value fetch_min returns is not the root it was aimed at, another lane has hooked that word in the
// meantime: the union goes on with the returned value, which is smaller.  So every loop here runs down a chain of
// strictly decreasing indices >= 0 and ends after at most W H steps whatever other lanes or workgroups do at the same
// time; no lane ever waits for another: no flag, no spin, no ordered hand-over.
#pragma once
#include "ekf_dense_stereo.hpp"
#include "ekf_union_find.hpp"

namespace ekf {

constexpr unsigned kSegNone = 0xffffffffu;       // the label of an invalid pixel
constexpr int kSpeckleMaxSize = 1 << 26;         // min_size: 1 .. 2^26 = kDenseMaxDim^2, the largest map
constexpr int kSpeckleMaxDiff = kDenseMaxPlanes - 1;
constexpr int kSpeckleKinds = 4;                 // timed kinds: k_speckle_label, _merge, _count, _apply
constexpr int kSegTile = kDenseTW * kDenseTH;    // 512 pixels, two a lane as in the sweeps
static_assert((long long)kDenseMaxDim * kDenseMaxDim <= (long long)kSpeckleMaxSize, "a linear index and a size fit 27 bits");

// The accessors of the forest (SegGlobal for the words of L that k_speckle_merge shares between workgroups, SegLds for the
// tile's forest in k_speckle_label and the counters of k_speckle_count), seg_find and seg_union: ekf_union_find.hpp, which
// the components of the welded mesh share (ekf_mesh_components.hpp).  The host check
// (tools/speckle_host_check.cpp) defines EKF_SPECKLE_HOST_ATOMICS and the six accessor functions with the __atomic builtins
// before it includes this header.

// Linked iff both valid and at most max_diff apart; the difference in 64 bits.
__device__ __forceinline__ bool seg_linked(int p, int q, int max_diff) {
  const long long d = (long long)p - (long long)q;
  return p >= 0 && q >= 0 && (d < 0 ? -d : d) <= (long long)max_diff;
}

struct SpeckleArgs {
  float* depth;                       // the map, filtered in place by k_speckle_apply
  int* plane;
  unsigned* L;                        // W H words each
  unsigned* R;
  unsigned* S;
  int W, H, min_size, max_diff;
};

// One workgroup per 32 x 16 tile, a lane owns the pixels (tx, ty) and (tx, ty + 8) as in the sweeps.  The tile's planes go
// to LDS once (-1 outside the image); every pixel computes its links to its right and lower neighbour inside the tile once
// and makes the union for each, all lanes at once, in the tile's forest in LDS.  One pass over the links is all a union-find
// needs: behind the barrier every pixel's find gives the least local index of its part of the segment, and row-major order
// inside the tile is the order of the global index, so that is the part's least global index as well.
__global__ void __launch_bounds__(256) k_speckle_label(SpeckleArgs a) {
  __shared__ int s_p[kSegTile];
  __shared__ unsigned s_l[kSegTile];
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
  const int X = (int)blockIdx.x * kDenseTW + tx, Y0 = (int)blockIdx.y * kDenseTH;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int oy = ty + 8 * j, l = oy * kDenseTW + tx, Y = Y0 + oy;
    s_p[l] = (X < a.W && Y < a.H) ? a.plane[(size_t)Y * a.W + X] : -1;
    s_l[l] = (unsigned)l;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int oy = ty + 8 * j, l = oy * kDenseTW + tx;
    const int p = s_p[l];
    if (tx < kDenseTW - 1 && seg_linked(p, s_p[l + 1], a.max_diff)) seg_union<SegLds>(s_l, (unsigned)l, (unsigned)(l + 1));
    if (oy < kDenseTH - 1 && seg_linked(p, s_p[l + kDenseTW], a.max_diff)) seg_union<SegLds>(s_l, (unsigned)l, (unsigned)(l + kDenseTW));
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int oy = ty + 8 * j, l = oy * kDenseTW + tx, Y = Y0 + oy;
    if (X >= a.W || Y >= a.H) continue;
    unsigned label = kSegNone;
    if (s_p[l] >= 0) {
      const unsigned r = seg_find<SegLds>(s_l, (unsigned)l);                 // r <= l: inside the tile and the image
      label = (unsigned)(Y0 + (int)(r >> 5)) * (unsigned)a.W + (unsigned)((int)blockIdx.x * kDenseTW + (int)(r & 31));
    }
    const size_t o = (size_t)Y * a.W + X;
    a.L[o] = label;
    a.S[o] = 0;
  }
}

// The links across the tile borders: nbx = (W - 1) / 32 vertical borders of H pixels each, the pixels of column 32 k + 31
// with their right neighbour, then nby = (H - 1) / 16 horizontal borders of W pixels each, row 16 k + 15 with the row below;
// one lane an item (a map of one tile has none: the one workgroup of its launch returns).
//
// Visibility.  This is the one launch in which workgroups communicate through data while they run.  The XCDs' L2s are not
// coherent with each other and a CU's L1 is never refreshed by another CU's stores, so EVERY access to L in this kernel, the
// loads of seg_find included, is a relaxed atomic of agent scope (SegGlobal); there is no plain load or store of L.  What L
// holds at the start comes from k_speckle_label and is visible by the kernel boundary.  Relaxed suffices: the algorithm uses
// the modification order of each single word (it only ever decreases) and the value fetch_min returns, the one proof that a
// hook took place; it never infers from one word what another word holds.  A load that returns an older, larger value of a
// word only lengthens a walk: the value is still an ancestor.  The planes are read-only for the whole call and take plain
// loads.  Termination: the header's argument; nothing here waits.
__global__ void __launch_bounds__(256) k_speckle_merge(SpeckleArgs a) {
  const unsigned nbx = (unsigned)(a.W - 1) / kDenseTW, nby = (unsigned)(a.H - 1) / kDenseTH;
  const unsigned n_v = nbx * (unsigned)a.H, n_h = nby * (unsigned)a.W;       // <= 2^26 / 32 and 2^26 / 16
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n_v + n_h) return;
  unsigned X, Y, step;
  if (i < n_v) {
    X = (i / (unsigned)a.H) * kDenseTW + (kDenseTW - 1);                     // X + 1 <= nbx * 32 <= W - 1
    Y = i % (unsigned)a.H;
    step = 1u;
  } else {
    const unsigned k = i - n_v;
    Y = (k / (unsigned)a.W) * kDenseTH + (kDenseTH - 1);                     // Y + 1 <= nby * 16 <= H - 1
    X = k % (unsigned)a.W;
    step = (unsigned)a.W;
  }
  const unsigned o = Y * (unsigned)a.W + X;
  if (seg_linked(a.plane[o], a.plane[o + step], a.max_diff)) seg_union<SegGlobal>(a.L, o, o + step);
}

// Behind the kernel boundary L is final and takes plain loads.  One workgroup per tile, two pixels a lane: a valid pixel walks
// to its root (no word of L is written: R is another buffer) and the root gains 1.  Before anything goes to memory
// (cdna_hip_programming.md, Guideline 12):
//   - a root inside the workgroup's own tile, the common case, is counted in an LDS word of the tile, and the tile adds each
//     word that is not 0 to S once;
//   - the other roots: a run of equal roots along a tile row becomes one number at its first pixel, and the first pixels of
//     runs that stand in one column with equal roots become one number at the uppermost.  A tile inside a large segment so
//     adds to the segment's one word once, not 512 times.
// Unsigned sums are exact in any order.
__global__ void __launch_bounds__(256) k_speckle_count(SpeckleArgs a) {
  __shared__ unsigned s_own[kSegTile];          // pixels of the roots inside this tile
  __shared__ unsigned s_key[kSegTile];          // a pixel's root outside this tile; kSegNone: none
  __shared__ unsigned s_run[kSegTile];          // at the first pixel of a run of equal keys: its length; 0 elsewhere
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
  const int X = (int)blockIdx.x * kDenseTW + tx, Y0 = (int)blockIdx.y * kDenseTH;
#pragma unroll
  for (int j = 0; j < 2; ++j) s_own[(ty + 8 * j) * kDenseTW + tx] = 0;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int oy = ty + 8 * j, l = oy * kDenseTW + tx, Y = Y0 + oy;
    unsigned key = kSegNone;
    if (X < a.W && Y < a.H) {
      const size_t o = (size_t)Y * a.W + X;
      unsigned r = kSegNone;
      if (a.plane[o] >= 0) {
        r = (unsigned)o;
        for (unsigned p = a.L[r]; p != r; p = a.L[r]) r = p;                 // strictly decreasing
        const unsigned rx = r % (unsigned)a.W, ry = r / (unsigned)a.W;
        if (rx / kDenseTW == blockIdx.x && ry / kDenseTH == blockIdx.y)
          seg_lds_add(&s_own[(ry - (unsigned)Y0) * kDenseTW + (rx - blockIdx.x * kDenseTW)], 1u);
        else
          key = r;
      }
      a.R[o] = r;
    }
    s_key[l] = key;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int oy = ty + 8 * j, l = oy * kDenseTW + tx;
    const unsigned key = s_key[l];
    unsigned run = 0;
    if (key != kSegNone && (tx == 0 || s_key[l - 1] != key)) {
      run = 1;
      while (tx + (int)run < kDenseTW && s_key[l + (int)run] == key) ++run;
    }
    s_run[l] = run;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int oy = ty + 8 * j, l = oy * kDenseTW + tx, Y = Y0 + oy;
    if (X < a.W && Y < a.H && s_own[l] != 0) seg_global_add(&a.S[(size_t)Y * a.W + X], s_own[l]);
    const unsigned key = s_key[l];
    if (s_run[l] == 0 || (oy > 0 && s_run[l - kDenseTW] != 0 && s_key[l - kDenseTW] == key)) continue;
    unsigned sum = 0;
    for (int n = oy; n < kDenseTH && s_run[n * kDenseTW + tx] != 0 && s_key[n * kDenseTW + tx] == key; ++n) sum += s_run[n * kDenseTW + tx];
    seg_global_add(&a.S[key], sum);                                          // key: a root, an index inside the image
  }
}

// One lane per pixel: its size, S at its root (0 for an invalid pixel), goes to L, and the pixel goes where that is less than
// min_size.  S is only read here and L only written, each word by its own lane.
__global__ void __launch_bounds__(256) k_speckle_apply(SpeckleArgs a) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= (unsigned)a.W * (unsigned)a.H) return;
  const unsigned r = a.R[i];
  const unsigned size = r == kSegNone ? 0u : a.S[r];
  a.L[i] = size;
  if (size < (unsigned)a.min_size) {
    a.depth[i] = 0.f;
    a.plane[i] = -1;
  }
}

#ifndef EKF_KERNELS_ONLY
// Host side of the speckle filter of one handle: the three planes, the staging maps of ekf_dense_speckle_host, all grow-only
// and allocated by the first call that needs them, and a timer of its own.  DenseView::seg says which slot's filtered map,
// if any, R and L (labels and sizes before the removal) belong to.
struct DenseSpeckle {
  DevBuf<unsigned> L, R, S;
  DevBuf<float> h_depth;              // a host caller's maps on the device
  DevBuf<int> h_plane;
  KernelTimer<kSpeckleKinds> timer;

  // The four launches on the default stream over the W x H maps `depth` / `plane`, filtered in place.
  hipError_t run(int W, int H, float* depth, int* plane, int min_size, int max_diff) {
    const size_t n = (size_t)W * H;
    hipError_t e;
    if ((e = L.reserve(n)) != hipSuccess || (e = R.reserve(n)) != hipSuccess || (e = S.reserve(n)) != hipSuccess) {
      (void)hipGetLastError();
      return e;
    }
    const SpeckleArgs a{depth, plane, L, R, S, W, H, min_size, max_diff};
    const dim3 tiles((unsigned)((W + kDenseTW - 1) / kDenseTW), (unsigned)((H + kDenseTH - 1) / kDenseTH));
    const size_t border = (size_t)((W - 1) / kDenseTW) * H + (size_t)((H - 1) / kDenseTH) * W;
    const unsigned wg_m = (unsigned)std::max<size_t>(1, (border + 255) / 256), wg_n = (unsigned)((n + 255) / 256);
    if ((e = timer.run(0, [&] { k_speckle_label<<<tiles, 256, 0, nullptr>>>(a); })) != hipSuccess) return e;
    if ((e = timer.run(1, [&] { k_speckle_merge<<<wg_m, 256, 0, nullptr>>>(a); })) != hipSuccess) return e;
    if ((e = timer.run(2, [&] { k_speckle_count<<<tiles, 256, 0, nullptr>>>(a); })) != hipSuccess) return e;
    return timer.run(3, [&] { k_speckle_apply<<<wg_n, 256, 0, nullptr>>>(a); });
  }
};
#endif  // EKF_KERNELS_ONLY

}  // namespace ekf
