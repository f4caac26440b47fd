// Rectification for pinhole consumers: the images the library already holds on the device (matcher frame,
// raw frame, the key-frame emit slots) remapped through the lens model, pixel coordinates undistorted, and the pinhole
// camera that goes with each resolution.  The reference does none of this (its key frames and projections stay in the
// distorted image); the arithmetic is pinned here and restated in numpy by tests/rectify_oracle.py:
//   - every coordinate operation is fp64, rounded once, in the written left-to-right order; contraction is off in every
//     function below, so no product and sum fuse (the fp64 division the compiler expands is still correctly rounded);
//   - the image interpolation is integer: 5-bit fractions, four weights that sum to 1024 (what cv::remap uses for 8-bit
//     INTER_LINEAR), taps outside the image count as 0.
// Nothing here runs per frame: the launches go out only when a caller asks for rectified data.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>

#include "ekf_buffers.hpp"
#include "ekf_math.hpp"

namespace ekf {

// The lens model in fp64 (the config's floats widened) and the factor s between the matcher frame and the addressed
// resolution: 1 for the matcher frame, ekf_config.scale for the raw frame.  Matcher pixel u and pixel X of the addressed
// resolution: u = (X + 0.5) / s - 0.5 (the pixel-centre convention of k_frame_ingest's resize).
struct RectCam {
  double fx, fy, u0, v0, k1, k2, k3, p1, p2, s;
};

inline RectCam rect_cam(const CamParams& c, int s) {
  return RectCam{(double)c.fx, (double)c.fy, (double)c.u0, (double)c.v0, (double)c.k1, (double)c.k2,
                 (double)c.k3, (double)c.p1, (double)c.p2, (double)s};
}

// K of the rectified image at the resolution of `c.s`: (fx s, fy s, (u0 + 0.5) s - 0.5, (v0 + 0.5) s - 0.5); s = 1 leaves
// the config's fx fy u0 v0.  K[4] = fx fy cx cy.
inline void rect_camera(const RectCam& c, double K[4]) {
#pragma clang fp contract(off)
  K[0] = c.fx * c.s;
  K[1] = c.fy * c.s;
  K[2] = (c.u0 + 0.5) * c.s - 0.5;
  K[3] = (c.v0 + 0.5) * c.s - 0.5;
}

struct RectifyArgs {
  const unsigned char* src;           // H rows of W * C bytes, tight: the held (distorted) image
  unsigned char* dst;                 // the same geometry: the rectified image
  int W, H;
  RectCam c;
};

// One launch, grid-stride, no LDS: a lane takes one output pixel, evaluates the forward lens model once (project_distort's
// op order: the rectified pixel's ray lands at (ud, vd) of the distorted matcher frame) and blends its 4 taps for every
// channel.  Consecutive lanes write consecutive pixels; the taps of a wave lie on neighbouring rows of the source.
template <int C>
__global__ void __launch_bounds__(256) k_frame_rectify(RectifyArgs a) {
#pragma clang fp contract(off)
  // (frames of 2^31 bytes or more are refused at ingest: pixel counts fit 32 bits, byte offsets are formed in size_t)
  const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned nthreads = gridDim.x * blockDim.x;
  const unsigned npix = (unsigned)a.W * (unsigned)a.H;
  const size_t pitch = (size_t)a.W * C;
  const RectCam c = a.c;
  for (unsigned i = tid; i < npix; i += nthreads) {
    const int Y = (int)(i / (unsigned)a.W), X = (int)(i % (unsigned)a.W);
    const double u = ((double)X + 0.5) / c.s - 0.5;
    const double v = ((double)Y + 0.5) / c.s - 0.5;
    const double x1 = (u - c.u0) / c.fx;
    const double y1 = (v - c.v0) / c.fy;
    const double r2 = x1 * x1 + y1 * y1;
    const double l = 1.0 + c.k1 * r2 + c.k2 * r2 * r2 + c.k3 * r2 * r2 * r2;
    const double x2 = x1 * l + 2.0 * c.p1 * x1 * y1 + c.p2 * (r2 + 2.0 * x1 * x1);
    const double y2 = y1 * l + 2.0 * c.p2 * x1 * y1 + c.p1 * (r2 + 2.0 * y1 * y1);
    const double ud = c.fx * x2 + c.u0;
    const double vd = c.fy * y2 + c.v0;
    const double sx = (ud + 0.5) * c.s - 0.5;
    const double sy = (vd + 0.5) * c.s - 0.5;
    unsigned out[C];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) out[ch] = 0u;
    if (sx > -1.0 && sx < (double)a.W && sy > -1.0 && sy < (double)a.H) {          // (a NaN fails: the pixel stays 0)
      const int qx = (int)floor(sx * 32.0 + 0.5), qy = (int)floor(sy * 32.0 + 0.5);
      const int ix = qx >> 5, ax = qx & 31, iy = qy >> 5, ay = qy & 31;            // ix in [-1, W], iy in [-1, H]
      // a tap outside the image counts as 0: its weight is dropped and its address clamped into the image
      const int wx0 = (ix >= 0 && ix < a.W) ? 32 - ax : 0, wx1 = (ix + 1 < a.W) ? ax : 0;
      const int wy0 = (iy >= 0 && iy < a.H) ? 32 - ay : 0, wy1 = (iy + 1 < a.H) ? ay : 0;
      const int cx0 = min(max(ix, 0), a.W - 1), cx1 = min(ix + 1, a.W - 1);
      const int cy0 = min(max(iy, 0), a.H - 1), cy1 = min(iy + 1, a.H - 1);
      const unsigned char* r0 = a.src + (size_t)cy0 * pitch;
      const unsigned char* r1 = a.src + (size_t)cy1 * pitch;
      const size_t o0 = (size_t)cx0 * C, o1 = (size_t)cx1 * C;
      const unsigned w00 = (unsigned)(wx0 * wy0), w10 = (unsigned)(wx1 * wy0);
      const unsigned w01 = (unsigned)(wx0 * wy1), w11 = (unsigned)(wx1 * wy1);
#pragma unroll
      for (int ch = 0; ch < C; ++ch)
        out[ch] = (w00 * r0[o0 + ch] + w10 * r0[o1 + ch] + w01 * r1[o0 + ch] + w11 * r1[o1 + ch] + 512u) >> 10;
    }
    unsigned char* d = a.dst + (size_t)i * C;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) d[ch] = (unsigned char)out[ch];
  }
}

// One lane per point: (u, v) in pixels of the resolution of `c.s` -> matcher pixels -> the 50 fixed-point iterations of
// undistort_deproject (same op order, fp64) -> the pinhole pixel of the ray -> back to that resolution.  A non-finite
// input gives NaN, NaN.
__global__ void __launch_bounds__(64) k_undistort_pixels(const double* __restrict__ uv, double* __restrict__ out, int n,
                                                         RectCam c) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double ui = uv[2 * (size_t)i], vi = uv[2 * (size_t)i + 1];
  double ur = __builtin_nan(""), vr = __builtin_nan("");
  if (isfinite(ui) && isfinite(vi)) {
    const double u = (ui + 0.5) / c.s - 0.5;
    const double v = (vi + 0.5) / c.s - 0.5;
    const double x2 = (u - c.u0) / c.fx;
    const double y2 = (v - c.v0) / c.fy;
    double x1 = x2, y1 = y2;
    for (int it = 0; it < 50; ++it) {
      const double r2 = x1 * x1 + y1 * y1;
      const double l = 1.0 + c.k1 * r2 + c.k2 * r2 * r2 + c.k3 * r2 * r2 * r2;
      const double dx = 2.0 * c.p1 * x1 * y1 + c.p2 * (r2 + 2.0 * x1 * x1);
      const double dy = 2.0 * c.p2 * x1 * y1 + c.p1 * (r2 + 2.0 * y1 * y1);
      x1 = (x2 - dx) / l;
      y1 = (y2 - dy) / l;
    }
    const double um = c.fx * x1 + c.u0;
    const double vm = c.fy * y1 + c.v0;
    ur = (um + 0.5) * c.s - 0.5;
    vr = (vm + 0.5) * c.s - 0.5;
  }
  out[2 * (size_t)i] = ur;
  out[2 * (size_t)i + 1] = vr;
}

// Grow-only device scratch of one owner (a filter, a key-frame selector): the rectified image before its one copy to the
// host, and the points on their way in and out.  Allocated by the first call that needs it, never per frame.
struct RectScratch {
  DevBuf<unsigned char> d_img;
  DevBuf<double> d_pts;               // n inputs, then n outputs (2 doubles each)
};

// src (W x H x C, tight, device) -> rectified, in rs.d_img: the one launch, on `stream`.
inline hipError_t rectify_launch(RectScratch& rs, hipStream_t stream, const unsigned char* d_src, int W, int H, int C,
                                 const RectCam& c) {
  const hipError_t e = rs.d_img.reserve((size_t)W * C * H);
  if (e != hipSuccess) return e;
  const RectifyArgs a{d_src, rs.d_img, W, H, c};
  const size_t npix = (size_t)W * H;
  const int grid = (int)std::min<size_t>((npix + 255) / 256, 1024);
  if (C == 1) k_frame_rectify<1><<<grid, 256, 0, stream>>>(a);
  else k_frame_rectify<3><<<grid, 256, 0, stream>>>(a);
  return hipGetLastError();
}

// rs.d_img -> out (host, `stride` bytes per row): the one copy the image makes; `stream` is synchronised before the return.
inline hipError_t rectified_to_host(RectScratch& rs, hipStream_t stream, int W, int H, int C, unsigned char* out, size_t stride) {
  const size_t row = (size_t)W * C;
  const hipError_t e = hipMemcpy2DAsync(out, stride, rs.d_img, row, row, (size_t)H, hipMemcpyDeviceToHost, stream);
  return e != hipSuccess ? e : hipStreamSynchronize(stream);
}

// uv (host, n points) -> undistorted -> out (host).  As above: `stream` is synchronised before the return.
inline hipError_t undistort_to_host(RectScratch& rs, hipStream_t stream, const double* uv, int n, const RectCam& c, double* out) {
  if (n <= 0) return hipSuccess;
  hipError_t e;
  if ((e = rs.d_pts.reserve((size_t)n * 4)) != hipSuccess) return e;
  double* d_in = rs.d_pts;
  double* d_out = rs.d_pts + 2 * (size_t)n;
  const size_t bytes = (size_t)n * 2 * sizeof(double);
  if ((e = hipMemcpyAsync(d_in, uv, bytes, hipMemcpyHostToDevice, stream)) != hipSuccess) return e;
  k_undistort_pixels<<<(n + 63) / 64, 64, 0, stream>>>(d_in, d_out, n, c);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
  return hipStreamSynchronize(stream);
}

}  // namespace ekf
