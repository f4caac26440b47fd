// Ray casting of the TSDF volume of ekf_fusion.hpp into a depth, a normal and a grey image from any pinhole pose (DESIGN.md
// §17).  The reference has no counterpart; the arithmetic is pinned here and restated in numpy by tests/raycast_oracle.py:
//   - k_tsdf_mean turns the sum and count planes into one fp32 plane of means, a quiet NaN where cnt < min_count, so that the
//     march loads 8 floats a sample and divides nothing;
//   - k_tsdf_raycast marches one ray a lane at samples z_n = z_near + n step of the camera-z depth, keeps the previous
//     sample's validity and value, and ends at the first pair of valid samples that goes from v >= 0 to v < 0;
//   - every coordinate operation is fp64, rounded once, in the written left-to-right order; contraction is off in every
//     function below (host and device), as in ekf_fusion.hpp; poses go through dense_pose unchanged.
//   - k_tsdf_raycast_colour runs the same march, rc_march, for a colour volume: it also writes the B, G, R of
//     the hit.
// No atomics, no LDS: a pixel belongs to one lane.  Nothing here touches a filter, counts as a launch kind or runs a collective.
#pragma once
#include <cmath>
#include <cstddef>

// EKF_KERNELS_ONLY: the structs and the kernel bodies alone, for tools/raycast_host_check.cpp, which runs the kernels lane
// by lane on the host; tools/host_kernels.hpp supplies threadIdx, blockIdx and the like.
#include "ekf_fusion.hpp"

namespace ekf {

constexpr int kRaycastMaxDim = 8192, kRaycastMaxSamples = 65536;
constexpr int kRaycastTile = 16;                 // a workgroup owns 16 x 16 pixels, each of its four waves 8 x 8 of them

struct MeanArgs {
  const float* sum;
  const unsigned short* cnt;
  float* mean;
  unsigned nvox;
  int min_count;
};

// One lane per voxel: two contiguous loads, one contiguous store.
__global__ void __launch_bounds__(256) k_tsdf_mean(MeanArgs a) {
#pragma clang fp contract(off)
  const unsigned lin = blockIdx.x * (unsigned)kFusionBlock + threadIdx.x;
  if (lin >= a.nvox) return;
  const unsigned short c = a.cnt[lin];
  a.mean[lin] = (int)c >= a.min_count ? (float)((double)a.sum[lin] / (double)c) : __builtin_nanf("");
}

struct RaycastArgs {
  const float* mean;
  const unsigned short* cnt;
  const unsigned* gsum;
  float* depth;                       // H rows of W floats, tight; 0 = no hit
  float* normal;                      // H rows of W x 3 floats
  unsigned char* grey;                // H rows of W bytes
  int W, H;
  TsdfGrid g;
  double inv;                         // 1.0 / voxel
  double fx, fy, cx, cy;
  double R[9], t[3];                  // the view's pose: X = t + R x_cam
  double z_near, step;
  int N;                              // samples n = 0 .. N - 1
};

// The grid coordinates of X on axis c, as every sample computes them.
__device__ __forceinline__ double rc_coord(const RaycastArgs& a, int c, double X) {
#pragma clang fp contract(off)
  return (X - a.g.origin[c]) * a.inv;
}

// The cell of X: false unless 0 <= floor(g_c) <= n_c - 2 on every axis (a NaN fails); lin0 of its corner 0 and the fractions.
__device__ __forceinline__ bool rc_locate(const RaycastArgs& a, double X0, double X1, double X2, unsigned& lin0, double& f0,
                                          double& f1, double& f2) {
#pragma clang fp contract(off)
  const double g0 = rc_coord(a, 0, X0), g1 = rc_coord(a, 1, X1), g2 = rc_coord(a, 2, X2);
  const double i0 = floor(g0), i1 = floor(g1), i2 = floor(g2);
  if (!(i0 >= 0.0 && i0 <= (double)(a.g.nx - 2) && i1 >= 0.0 && i1 <= (double)(a.g.ny - 2) && i2 >= 0.0 &&
        i2 <= (double)(a.g.nz - 2)))
    return false;
  f0 = g0 - i0;
  f1 = g1 - i1;
  f2 = g2 - i2;
  lin0 = (unsigned)(int)i0 + (unsigned)a.g.nx * ((unsigned)(int)i1 + (unsigned)a.g.ny * (unsigned)(int)i2);
  return true;
}

__device__ __forceinline__ unsigned rc_corner(const RaycastArgs& a, unsigned lin0, int c) {      // corner c = dx + 2 dy + 4 dz
  return lin0 + (unsigned)(c & 1) + (unsigned)((c >> 1) & 1) * (unsigned)a.g.nx + (unsigned)(c >> 2) * ((unsigned)a.g.nx * (unsigned)a.g.ny);
}

// The 8 means of a cell as doubles; false if one of them is NaN.
__device__ __forceinline__ bool rc_means(const RaycastArgs& a, unsigned lin0, double v[8]) {
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const float m = a.mean[rc_corner(a, lin0, c)];
    ok = ok && m == m;
    v[c] = (double)m;
  }
  return ok;
}

__device__ __forceinline__ double rc_lerp(double p, double q, double f) {
#pragma clang fp contract(off)
  return p + f * (q - p);
}

// x first, then y, then z.
__device__ __forceinline__ double rc_trilinear(const double v[8], double f0, double f1, double f2) {
  const double a00 = rc_lerp(v[0], v[1], f0), a10 = rc_lerp(v[2], v[3], f0), a01 = rc_lerp(v[4], v[5], f0), a11 = rc_lerp(v[6], v[7], f0);
  return rc_lerp(rc_lerp(a00, a10, f1), rc_lerp(a01, a11, f1), f2);
}

__device__ __forceinline__ double rc_bilinear(double d0, double d1, double d2, double d3, double fa, double fb) {
  return rc_lerp(rc_lerp(d0, d1, fa), rc_lerp(d2, d3, fa), fb);
}

// The samples a ray cannot skip: n_lo .. n_hi.  Every rounded operation between n and a grid coordinate is monotone, so the
// coordinate on axis c is monotone in n, in the direction of the sign of dw_c: if the sample before n_lo is out of range on
// an axis on the side the ray comes from, so is every earlier one, and likewise after n_hi.  The candidates are the slab
// intersections of the box, two samples wide of them; a candidate that the test does not confirm falls back to the full
// march (so does a NaN).  A direction component of 0 leaves the coordinate at t_c for every n: out of range there, the ray
// has no sample at all.
__device__ __forceinline__ void rc_range(const RaycastArgs& a, const double dw[3], int& n_lo, int& n_hi) {
#pragma clang fp contract(off)
  const double top[3] = {(double)(a.g.nx - 1), (double)(a.g.ny - 1), (double)(a.g.nz - 1)};
  double z_in = -INFINITY, z_out = INFINITY;
  bool empty = false;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (dw[c] == 0.0) {
      const double g0 = rc_coord(a, c, a.t[c]);
      empty = empty || !(g0 >= 0.0 && g0 < top[c]);
    } else {
      const double za = (a.g.origin[c] - a.t[c]) / dw[c], zb = ((a.g.origin[c] + top[c] * a.g.voxel) - a.t[c]) / dw[c];
      z_in = fmax(z_in, fmin(za, zb));
      z_out = fmin(z_out, fmax(za, zb));
    }
  }
  const double last = (double)(a.N - 1);
  double lo = floor((z_in - a.z_near) / a.step) - 2.0, hi = ceil((z_out - a.z_near) / a.step) + 2.0;
  lo = lo >= 1.0 ? fmin(lo, last + 1.0) : 0.0;
  hi = hi <= last - 1.0 ? fmax(hi, -1.0) : last;
  n_lo = (int)lo;
  n_hi = (int)hi;
  const double zb = a.z_near + (double)(n_lo > 0 ? n_lo - 1 : 0) * a.step, ze = a.z_near + (double)(n_hi < a.N - 1 ? n_hi + 1 : a.N - 1) * a.step;
  bool out_lo = false, out_hi = false;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double gb = rc_coord(a, c, a.t[c] + zb * dw[c]), ge = rc_coord(a, c, a.t[c] + ze * dw[c]);
    out_lo = out_lo || (dw[c] > 0.0 && gb < 0.0) || (dw[c] < 0.0 && gb >= top[c]);
    out_hi = out_hi || (dw[c] > 0.0 && ge >= top[c]) || (dw[c] < 0.0 && ge < 0.0);
  }
  if (n_lo > 0 && !out_lo) n_lo = 0;
  if (n_hi < a.N - 1 && !out_hi) n_hi = a.N - 1;
  if (empty) n_lo = a.N;
}

// What the march of a colour volume has beside RaycastArgs.
struct RaycastColour {
  const unsigned* csum;               // three planes of nvox back to back
  unsigned char* bgr;                 // H rows of W x 3 bytes: B, G, R; 0, 0, 0 = no hit
  size_t nvox;
};

// The march of pixel (px, py) over the samples n .. n_hi of rc_range, and its stores: the one body of both ray-cast kernels.
// The loop of a wave ends when each of its lanes has hit or run out of samples; a lane that is done is masked off and loads
// nothing.  A hit gives 1 + C bytes: byte 0 from gsum and, for C = 3, one from each plane of k->csum (k is not read for C = 0);
// each is plane / cnt at the eight corners of the hit's cell, blended as the means are and rounded half up.  Each kernel keeps
// its own prologue (the pixel, the off-image return, dw and rc_range): with the prologue in here too, k_tsdf_raycast compiles
// to other instructions than it did with a body of its own.
template <int C>
__device__ __forceinline__ void rc_march(const RaycastArgs& a, const RaycastColour* k, int px, int py, const double dw[3], int n,
                                         int n_hi) {
#pragma clang fp contract(off)
  float depth = 0.f, nrm0 = 0.f, nrm1 = 0.f, nrm2 = 0.f;
  unsigned char byte[1 + C] = {};
  bool pok = false;                   // the previous sample was valid, and its value
  double pv = 0.0;
  for (; n <= n_hi; ++n) {
    const double z = a.z_near + (double)n * a.step;
    unsigned lin0;
    double f0, f1, f2, v[8];
    bool ok = rc_locate(a, a.t[0] + z * dw[0], a.t[1] + z * dw[1], a.t[2] + z * dw[2], lin0, f0, f1, f2);
    double val = 0.0;
    if (ok) {
      ok = rc_means(a, lin0, v);
      val = rc_trilinear(v, f0, f1, f2);
    }
    if (ok && pok && pv >= 0.0 && val < 0.0) {
      const double u = pv / (pv - val);
      const double zs = (a.z_near + (double)(n - 1) * a.step) + u * a.step;
      if (rc_locate(a, a.t[0] + zs * dw[0], a.t[1] + zs * dw[1], a.t[2] + zs * dw[2], lin0, f0, f1, f2) && rc_means(a, lin0, v)) {
        const double gx = rc_bilinear(v[1] - v[0], v[3] - v[2], v[5] - v[4], v[7] - v[6], f1, f2);
        const double gy = rc_bilinear(v[2] - v[0], v[3] - v[1], v[6] - v[4], v[7] - v[5], f0, f2);
        const double gz = rc_bilinear(v[4] - v[0], v[5] - v[1], v[6] - v[2], v[7] - v[3], f0, f1);
        const double len = sqrt((gx * gx + gy * gy) + gz * gz);
        if (len > 0.0) {
          nrm0 = (float)(gx / len);
          nrm1 = (float)(gy / len);
          nrm2 = (float)(gz / len);
        }
#pragma unroll
        for (int p = 0; p <= C; ++p) {
          const unsigned* plane = p == 0 ? a.gsum : k->csum + (p - 1) * k->nvox;
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            const unsigned l = rc_corner(a, lin0, c);
            v[c] = (double)plane[l] / (double)a.cnt[l];
          }
          byte[p] = (unsigned char)(int)floor(rc_trilinear(v, f0, f1, f2) + 0.5);
        }
        depth = (float)zs;
        break;
      }
    }
    pok = ok;
    pv = val;
  }
  const size_t pix = (size_t)py * (size_t)a.W + (size_t)px;
  a.depth[pix] = depth;
  a.normal[pix * 3 + 0] = nrm0;
  a.normal[pix * 3 + 1] = nrm1;
  a.normal[pix * 3 + 2] = nrm2;
  a.grey[pix] = byte[0];
#pragma unroll
  for (int ch = 0; ch < C; ++ch) k->bgr[pix * 3 + ch] = byte[1 + ch];
}

// One lane per pixel.  A wave owns an 8 x 8 tile of pixels and a workgroup 16 x 16, so that the rays of a wave walk
// neighbouring voxels and its 8 corner loads fall in few cache lines.
__global__ void __launch_bounds__(256) k_tsdf_raycast(RaycastArgs a) {
#pragma clang fp contract(off)
  const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int px = (int)(blockIdx.x * (unsigned)kRaycastTile + (wave & 1) * 8 + (lane & 7));
  const int py = (int)(blockIdx.y * (unsigned)kRaycastTile + (wave >> 1) * 8 + (lane >> 3));
  if (px >= a.W || py >= a.H) return;
  const double dc0 = ((double)px - a.cx) / a.fx, dc1 = ((double)py - a.cy) / a.fy;
  const double dw[3] = {a.R[0] * dc0 + a.R[1] * dc1 + a.R[2], a.R[3] * dc0 + a.R[4] * dc1 + a.R[5],
                        a.R[6] * dc0 + a.R[7] * dc1 + a.R[8]};
  int n, n_hi;
  rc_range(a, dw, n, n_hi);
  rc_march<0>(a, nullptr, px, py, dw, n, n_hi);
}

// The one launch of a colour volume: k_tsdf_raycast with the B, G, R of the hit beside its depth, normal and grey.
// tests/test_gpu_colour.py holds the depth, normal and grey of the two kernels against each other bit for bit.
__global__ void __launch_bounds__(256) k_tsdf_raycast_colour(RaycastArgs a, RaycastColour k) {
#pragma clang fp contract(off)
  const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int px = (int)(blockIdx.x * (unsigned)kRaycastTile + (wave & 1) * 8 + (lane & 7));
  const int py = (int)(blockIdx.y * (unsigned)kRaycastTile + (wave >> 1) * 8 + (lane >> 3));
  if (px >= a.W || py >= a.H) return;
  const double dc0 = ((double)px - a.cx) / a.fx, dc1 = ((double)py - a.cy) / a.fy;
  const double dw[3] = {a.R[0] * dc0 + a.R[1] * dc1 + a.R[2], a.R[3] * dc0 + a.R[4] * dc1 + a.R[5],
                        a.R[6] * dc0 + a.R[7] * dc1 + a.R[8]};
  int n, n_hi;
  rc_range(a, dw, n, n_hi);
  rc_march<3>(a, &k, px, py, dw, n, n_hi);
}

#ifndef EKF_KERNELS_ONLY
// Host side: the buffers of a render, owned by the fusion handle they belong to.  The mean plane is made at the first render
// and kept until the volume changes (TsdfFusion::changes) or min_count differs.  The two launches are kinds 4 (k_tsdf_mean)
// and 5 (k_tsdf_raycast) of the fusion handle's timer.
struct TsdfRaycast {
  DevBuf<float> mean;
  DevBuf<float> depth, normal;
  DevBuf<unsigned char> grey, bgr;    // bgr: colour volumes only
  int mean_count = 0;                 // the min_count of the plane in `mean`; 0 = none
  unsigned long long mean_changes = 0, render_changes = 0;      // TsdfFusion::changes when the plane and the render were made
  int W = 0, H = 0;
  bool valid = false;                 // a render exists (of the volume as it was at render_changes)

  bool current(const TsdfFusion& f) const { return valid && render_changes == f.changes; }

  // (mean plane) -> grow the images -> march.  A failed allocation leaves the previous render (the new images replace the old
  // ones only when all of them exist), the mesh and the volume as they were.
  hipError_t render(TsdfFusion& f, int width, int height, const double K[4], const double R[9], const double t[3],
                    double z_near, double step, int N, int min_count) {
    hipError_t e;
    const size_t npix = (size_t)width * height;
    if ((e = mean.reserve(f.nvox())) != hipSuccess) {
      (void)hipGetLastError();
      return e;
    }
    if (npix > depth.capacity() || npix * 3 > normal.capacity() || npix > grey.capacity() || (f.colour && npix * 3 > bgr.capacity())) {
      DevBuf<float> d, nr;
      DevBuf<unsigned char> gr, co;
      if ((e = d.reserve(npix)) != hipSuccess || (e = nr.reserve(npix * 3)) != hipSuccess || (e = gr.reserve(npix)) != hipSuccess ||
          (f.colour && (e = co.reserve(npix * 3)) != hipSuccess)) {
        (void)hipGetLastError();
        return e;
      }
      depth = std::move(d);
      normal = std::move(nr);
      grey = std::move(gr);
      bgr = std::move(co);
      valid = false;
    }
    if (mean_count != min_count || mean_changes != f.changes) {
      mean_count = 0;
      const MeanArgs m{f.sum, f.cnt, mean, (unsigned)f.nvox(), min_count};
      const unsigned nblk = (unsigned)((f.nvox() + kFusionBlock - 1) / kFusionBlock);
      if ((e = f.timer.run(4, [&] { k_tsdf_mean<<<nblk, kFusionBlock, 0, nullptr>>>(m); })) != hipSuccess) return e;
      mean_count = min_count;
      mean_changes = f.changes;
    }
    RaycastArgs a{};
    a.mean = mean; a.cnt = f.cnt; a.gsum = f.gsum;
    a.depth = depth; a.normal = normal; a.grey = grey;
    a.W = width; a.H = height;
    a.g = f.g; a.inv = 1.0 / f.g.voxel;
    a.fx = K[0]; a.fy = K[1]; a.cx = K[2]; a.cy = K[3];
    for (int i = 0; i < 9; ++i) a.R[i] = R[i];
    for (int i = 0; i < 3; ++i) a.t[i] = t[i];
    a.z_near = z_near; a.step = step; a.N = N;
    valid = false;
    const dim3 grid((unsigned)((width + kRaycastTile - 1) / kRaycastTile), (unsigned)((height + kRaycastTile - 1) / kRaycastTile));
    if (f.colour) {
      const RaycastColour k{f.csum, bgr, f.nvox()};
      e = f.timer.run(8, [&] { k_tsdf_raycast_colour<<<grid, kRaycastTile * kRaycastTile, 0, nullptr>>>(a, k); });
    } else {
      e = f.timer.run(5, [&] { k_tsdf_raycast<<<grid, kRaycastTile * kRaycastTile, 0, nullptr>>>(a); });
    }
    if (e != hipSuccess) return e;
    W = width;
    H = height;
    render_changes = f.changes;
    valid = true;
    return hipSuccess;
  }
};
#endif  // EKF_KERNELS_ONLY

}  // namespace ekf
