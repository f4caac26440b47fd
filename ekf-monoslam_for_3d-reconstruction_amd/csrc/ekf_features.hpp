// Corner seeding of the filter: VSlamFilter::findNewFeatures (vslamRansac.cpp:783-837) -- the mask of the
// existing patches and OpenCV's goodFeaturesToTrack(frame, features, num, 0.01f, 12, mask) -- on the device.
// The arithmetic is pinned; tests/frame_oracle.py restates it and the GPU tests hold these kernels to it bit for bit.
//
//   1. Mask (vR.cpp:788-818): 255 on Rect(w, w, W - 2w, H - 2w), w = window_size; then, for every feature whose
//      centre satisfies w < cx < W - w and w < cy < H - w (float compares), 0 on the square with origin
//      ((int)(cx - w), (int)(cy - w)) and side 2w + 1 (the reference's width / height correction is 0 inside
//      that margin).
//   2. Response: cornerMinEigenVal(blockSize 3, ksize 3) computed exactly.  Sobel 3 x 3 of the 8-bit frame in
//      integers with BORDER_REFLECT_101 (|Dx|, |Dy| <= 1020); unnormalised 3 x 3 box sums a, b, c of Dx^2, DxDy,
//      Dy^2, also REFLECT_101 (exact in int32, < 2^24); lambda = 0.5 ((a + c) - sqrt((a - c)^2 + 4 b^2)) in fp64:
//      every operand is an integer below 2^53, the square root is correctly rounded (__dsqrt_rn), so lambda is a
//      deterministic function of the frame and lambda >= 0.  In exact arithmetic it is OpenCV's value times
//      (4 * 3 * 255)^2: ranking and the relative threshold are the same; the only difference is OpenCV's fp32
//      rounding (the deterministic equivalent, as the RANSAC "best hypothesis" is).
//   3. Selection (goodFeaturesToTrack): thr = max(lambda over the mask) * quality_level; lambda kept where
//      lambda > thr over the WHOLE image (THRESH_TOZERO); 3 x 3 dilation, border pixels not contributing;
//      candidates: 1 <= x <= W-2, 1 <= y <= H-2, mask set, lambda != 0, lambda == its dilated value; order: lambda
//      descending, ties by raster index descending (OpenCV >= 3.4's greaterThanPtr; older builds left ties
//      unspecified); greedy: a candidate is accepted when no accepted corner lies at squared distance
//      < min_distance^2, until num corners (OpenCV's grid only accelerates this rule).
//
// Launches: k_seed_mask_init + k_seed_mask_paint (the mask), k_seed_response (lambda, masked maximum by an atomic
// max on the fp64 bit pattern: lambda >= 0), k_seed_candidates (threshold, dilation, mask, atomic append), and
// k_seed_select: ONE workgroup that repeatedly takes the largest (lambda, index) candidate not yet suppressed and
// suppresses every candidate within min_distance of it -- the same sequence as sort + greedy, since every corner
// it accepts precedes all remaining candidates in the order.  The candidates sit in LDS when they fit
// (kSeedLdsCands), in the global candidate buffer otherwise (the same code through flat pointers).
#pragma once
#include <hip/hip_runtime.h>
#include "ekf_image.hpp"          // reflect101 (BORDER_REFLECT_101)

namespace ekf {

// Track state (not the detector): the visibility / rho <= 0 flags of ekf_predict / ekf_measure (bit 0 / bit 1 of
// flags) folded into trk: bit 0 <- visible (Patch::setIsInInnovation, vR.cpp:520, 532, 561), bit 1 |= rho <= 0 (the
// sticky Patch::setRemove, vR.cpp:519).  The host reads trk back and clears it when it needs the state.
__global__ void k_track_fold(const unsigned char* __restrict__ flags, unsigned char* __restrict__ trk, int N) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) trk[i] = (unsigned char)((flags[i] & 1) | (trk[i] & 2) | (flags[i] & 2));
}

constexpr int kSeedTile = 16;             // response tile edge (one 256-lane workgroup per 16 x 16 pixels)
constexpr int kSeedSelectThreads = 1024;
constexpr int kSeedLdsCands = 4096;       // candidates k_seed_select keeps in LDS (12 bytes each)

// 255 inside Rect(w, w, W - 2w, H - 2w), 0 elsewhere
__global__ void k_seed_mask_init(unsigned char* __restrict__ mask, int W, int H, int w) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= W * H) return;
  const int x = i % W, y = i / W;
  mask[i] = (x >= w && x < W - w && y >= w && y < H - w) ? 255 : 0;
}

// one workgroup per square: origin (x0, y0) (host-computed from the float centres), side 2w + 1, clipped to the frame
__global__ void k_seed_mask_paint(unsigned char* __restrict__ mask, int W, int H, int w, const int* __restrict__ org) {
  const int x0 = org[2 * blockIdx.x], y0 = org[2 * blockIdx.x + 1], s = 2 * w + 1;
  for (int t = threadIdx.x; t < s * s; t += blockDim.x) {
    const int x = x0 + t % s, y = y0 + t / s;
    if (x >= 0 && x < W && y >= 0 && y < H) mask[(size_t)y * W + x] = 0;
  }
}

// lambda of every pixel; aux[0] <- max over the mask (fp64 bit pattern, atomic max: lambda >= 0)
__global__ void __launch_bounds__(256)
k_seed_response(const unsigned char* __restrict__ frame, int W, int H, const unsigned char* __restrict__ mask,
                double* __restrict__ lam, unsigned long long* __restrict__ aux) {
  constexpr int E = kSeedTile + 2;                  // Dx / Dy with a 1-pixel halo (values at the reflected pixel)
  __shared__ int sdx[E * E], sdy[E * E];
  __shared__ unsigned long long smax;
  const int tx0 = blockIdx.x * kSeedTile, ty0 = blockIdx.y * kSeedTile;
  if (threadIdx.x == 0) smax = 0ull;
  for (int t = threadIdx.x; t < E * E; t += blockDim.x) {
    const int gx = reflect101(tx0 - 1 + t % E, W), gy = reflect101(ty0 - 1 + t / E, H);
    int dx = 0, dy = 0;
    {
      const int xm = reflect101(gx - 1, W), xp = reflect101(gx + 1, W);
      const int ym = reflect101(gy - 1, H), yp = reflect101(gy + 1, H);
      const unsigned char* rm = frame + (size_t)ym * W;
      const unsigned char* r0 = frame + (size_t)gy * W;
      const unsigned char* rp = frame + (size_t)yp * W;
      dx = ((int)rm[xp] + 2 * (int)r0[xp] + (int)rp[xp]) - ((int)rm[xm] + 2 * (int)r0[xm] + (int)rp[xm]);
      dy = ((int)rp[xm] + 2 * (int)rp[gx] + (int)rp[xp]) - ((int)rm[xm] + 2 * (int)rm[gx] + (int)rm[xp]);
    }
    sdx[t] = dx;
    sdy[t] = dy;
  }
  __syncthreads();
  const int lx = threadIdx.x % kSeedTile, ly = threadIdx.x / kSeedTile;
  const int x = tx0 + lx, y = ty0 + ly;
  unsigned long long mine = 0ull;
  if (x < W && y < H) {
    int a = 0, b = 0, c = 0;
    // box sum over the 3 x 3 neighbourhood: the halo entries hold the values at the reflected pixels, so a
    // neighbour outside the frame reads the reflected one (REFLECT_101 of the covariance image)
    for (int j = 0; j < 3; ++j)
      for (int i = 0; i < 3; ++i) {
        const int dx = sdx[(ly + j) * E + lx + i], dy = sdy[(ly + j) * E + lx + i];
        a += dx * dx;
        b += dx * dy;
        c += dy * dy;
      }
    const long long amc = (long long)a - c;
    const long long disc = amc * amc + 4ll * (long long)b * b;          // < 2^51: exact in fp64
    const double l = 0.5 * ((double)(a + c) - __dsqrt_rn((double)disc));
    lam[(size_t)y * W + x] = l;
    if (mask[(size_t)y * W + x]) mine = (unsigned long long)__double_as_longlong(l);
  }
  if (mine) atomicMax(&smax, mine);
  __syncthreads();
  if (threadIdx.x == 0 && smax) atomicMax(aux, smax);
}

// threshold (> max * quality), 3 x 3 dilation, mask: append (lambda bits, raster index) of every local maximum
__global__ void k_seed_candidates(const double* __restrict__ lam, int W, int H, const unsigned char* __restrict__ mask,
                                  double quality, const unsigned long long* __restrict__ aux, int* __restrict__ count,
                                  unsigned long long* __restrict__ ckey, int* __restrict__ cidx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= W * H) return;
  const int x = i % W, y = i / W;
  if (x < 1 || x > W - 2 || y < 1 || y > H - 2 || !mask[i]) return;
  const double thr = __longlong_as_double((long long)aux[0]) * quality;
  const double v = lam[i];
  if (!(v > thr)) return;                          // thresholded to 0: never a candidate
  // the neighbours are all inside the frame here (1 <= x <= W-2): the dilation's border rule never applies
  for (int j = -1; j <= 1; ++j)
    for (int k = -1; k <= 1; ++k) {
      const double u = lam[(size_t)(y + j) * W + x + k];
      if (u > thr && u > v) return;
    }
  const int slot = atomicAdd(count, 1);
  ckey[slot] = (unsigned long long)__double_as_longlong(v);
  cidx[slot] = i;
}

__device__ __forceinline__ bool seed_before(unsigned long long ka, int ia, unsigned long long kb, int ib) {
  return ka > kb || (ka == kb && ia > ib);        // lambda descending, then raster index descending
}

// ONE workgroup: out[0] = corners accepted (<= num), out[1 + k] = raster index of corner k in acceptance order
__global__ void __launch_bounds__(kSeedSelectThreads)
k_seed_select(const int* __restrict__ count, unsigned long long* __restrict__ gkey, int* __restrict__ gidx, int W,
              int num, long long md2, int* __restrict__ out) {
  __shared__ unsigned long long lkey[kSeedLdsCands];
  __shared__ int lidx[kSeedLdsCands];
  __shared__ unsigned long long wkey[kSeedSelectThreads / 64];
  __shared__ int widx[kSeedSelectThreads / 64];
  __shared__ int wslot[kSeedSelectThreads / 64];
  __shared__ int s_best_idx;
  const int K = *count, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  unsigned long long* key = gkey;
  int* idx = gidx;
  if (K <= kSeedLdsCands) {
    for (int t = tid; t < K; t += kSeedSelectThreads) { lkey[t] = gkey[t]; lidx[t] = gidx[t]; }
    key = lkey;
    idx = lidx;
  }
  __syncthreads();
  int taken = 0, last = -1;                        // raster index of the corner accepted last (-1: none yet)
  while (taken < num) {
    const int lxp = last >= 0 ? last % W : 0, lyp = last >= 0 ? last / W : 0;
    unsigned long long bk = 0ull;
    int bi = -1, bs = -1;
    for (int t = tid; t < K; t += kSeedSelectThreads) {
      const int ci = idx[t];
      if (ci < 0) continue;                        // accepted or suppressed
      if (last >= 0) {
        const long long dx = ci % W - lxp, dy = ci / W - lyp;
        if (dx * dx + dy * dy < md2) { idx[t] = -1; continue; }
      }
      const unsigned long long ck = key[t];
      if (bi < 0 || seed_before(ck, ci, bk, bi)) { bk = ck; bi = ci; bs = t; }
    }
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long ok = __shfl_xor(bk, off, 64);
      const int oi = __shfl_xor(bi, off, 64), os = __shfl_xor(bs, off, 64);
      if (oi >= 0 && (bi < 0 || seed_before(ok, oi, bk, bi))) { bk = ok; bi = oi; bs = os; }
    }
    if (lane == 0) { wkey[wv] = bk; widx[wv] = bi; wslot[wv] = bs; }
    __syncthreads();
    if (tid == 0) {
      unsigned long long k0 = wkey[0];
      int i0 = widx[0], s0 = wslot[0];
      for (int w = 1; w < kSeedSelectThreads / 64; ++w)
        if (widx[w] >= 0 && (i0 < 0 || seed_before(wkey[w], widx[w], k0, i0))) { k0 = wkey[w]; i0 = widx[w]; s0 = wslot[w]; }
      s_best_idx = i0;
      if (i0 >= 0) { out[1 + taken] = i0; idx[s0] = -1; }
    }
    __syncthreads();
    last = s_best_idx;
    if (last < 0) break;                           // no candidate left
    ++taken;
    __syncthreads();                               // (s_best_* are rewritten by the next round)
  }
  if (tid == 0) out[0] = taken;
}

}  // namespace ekf
