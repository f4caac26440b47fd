// A rasteriser for the indexed meshes of the fusion handle: the welded, the pruned, the smoothed, the simplified mesh or one
// the caller gave, seen from any pinhole pose as a depth, a triangle, a barycentric, a normal and a shaded image (DESIGN.md
// §30).  The reference has no counterpart; the contract is pinned here and restated in numpy, twice, by tests/raster_oracle.py.
// The input is a source mesh (X fp64, F uint32, the vertex grey and, where it has them, B, G, R), an image of W x H (both in
// 1..8192), K = fx fy cx cy, a pose (through dense_pose, as the ray cast takes it), z_near >= 0, cull 0 or 1, shading 0 (vertex
// colours) or 1 (the atlas of §29) and cover 0 or 1.  Every fp64 operation is rounded once, in the written order, with
// contraction off:
//   1. a vertex: p2, sx, sy are tex_project's (ekf_mesh_texture.hpp, the one function).  It is usable iff p2 > z_near and sx
//      and sy are finite;
//   2. a triangle t with the vertex indices (i0, i1, i2) is dropped if a vertex is unusable: there is no clipping, a triangle
//      that straddles z_near disappears whole.  area2 = (x1 - x0)(y2 - y0) - (y1 - y0)(x2 - x0), k_tex_select's order;
//      area2 == 0 or NaN drops the triangle; front = area2 < 0 (§29's sigma = -1: the weld's triangles face free space and the
//      image's y runs downwards); with cull a triangle that is not front is dropped; s = front ? -1 : +1.  The box: x from
//      max(0, ceil(min sx)) to min(W - 1, floor(max sx)), y likewise; an empty box drops the triangle.  Pixel (px, py) is
//      sampled at ((double) px, (double) py): a pixel's centre is its integer coordinate;
//   3. coverage, watertight by construction.  Edge k runs from corner k to corner k + 1 mod 3 and weighs corner k + 2 mod 3;
//      it is evaluated from the endpoint with the lower vertex index: if i_a < i_b, E = (xb - xa)(py - ya) - (yb - ya)(px - xa)
//      and canon = true, otherwise E = -((xa - xb)(py - yb) - (ya - yb)(px - xb)) and canon = false, so that two triangles
//      that share an edge get exactly negated values whatever their corner order.  e_k = s E.  The pixel is inside edge k iff
//      e_k > 0, or e_k == 0 and canon != front: the triangle that runs the edge in ascending index order after its flip owns
//      the tie.  A pixel is covered iff it is inside all three edges and ssum = (b0 + b1) + b2 > 0, b_k the e of the edge
//      opposite corner k (b0 = e_1, b1 = e_2, b2 = e_0);
//   4. depth: w_k = (b_k / ssum) / p2_k, ws = (w0 + w1) + w2, z = 1.0 / ws, z32 = (float) z; the pixel is skipped unless
//      ws > 0 and z32 is finite.  Perspective-correct barycentrics l_k = w_k / ws.  The pixel's key is
//      ((uint64) bits(z32) << 32) | t; the image of keys starts at all ones and takes the minimum: the nearest depth wins and,
//      among equal depths, the least triangle index.  With cover a uint32 image counts, for every pixel, the triangles that
//      gave it a key (integer adds, exact in any order);
//   5. resolve, for every pixel whose key is not all ones, applies 2 to 4 again for the winning triangle through the same
//      device function, so that the depth is the key's own: depth (float32) = z32, tri (int32) = t, bary = ((float) l1,
//      (float) l2), normal = (X1 - X0) x (X2 - X0), each component a b - c d in fp64, divided by sqrt((n0 n0 + n1 n1) + n2 n2)
//      and converted to float, 0 where that length is 0 or not finite, not flipped for a back face.  Shading 0: per channel
//      floor(((l0 g0 + l1 g1) + l2 g2) + 0.5) clamped to 0..255 (k_tex_fallback's expression): the grey image and, where the
//      source has B, G, R, the colour image.  Shading 1: tx = ((l0 c0x + l1 c1x) + l2 c2x) + (double)(bx B), ty likewise, c_i,
//      bx, by §29.1's for t; both clamped to [0, A - 1]; k_tex_fill's 5-bit blend: q = (int) floor(s 32 + 0.5), i = q >> 5,
//      alpha = q & 31, the second tap min(i + 1, A - 1), (sum w tap + 512) >> 10.  A 3-channel atlas gives the colour image
//      and the grey image is its bgr2gray; a 1-channel atlas gives the grey image and no colour image.  A pixel without a hit
//      has depth 0, tri -1, bary 0, normal 0 and colour 0.
//
// The launches, 256 lanes a workgroup, on the default stream; the result does not depend on how the work is divided:
//                (hipMemsetAsync: keys = 0xff, the cover image and the cursor of the deferred list = 0)
//   k_rast_project   ceil(n_vert / 256)   one lane a vertex: step 1 into scratch (p2, sx, sy and a flag: 25 bytes a vertex)
//   k_rast_small     ceil(n_tri / 256)    one lane a triangle: step 2; a box of at most small_limit pixels is walked by the
//                                         lane itself (steps 3 and 4); a larger one appends t to a list through the cursor
//   k_rast_large     min(n_tri, 1024)     one workgroup a deferred triangle, its lanes over the box 256 pixels at a time; the
//                                         grid strides over the list and reads its length from device memory: no read-back.
//                                         Not launched when small_limit >= W H: no box is larger than the image
//   k_rast_resolve   16 x 16 tiles        one lane a pixel, 8 x 8 pixels a wave as k_tsdf_raycast has them: step 5
// The only atomics are the 64-bit minimum of the keys, the integer add of the cover image and the cursor, all relaxed, agent
// scope and exact in any order; the order of the deferred list costs no bit.  No kernel uses LDS, scratch memory or a per-lane
// array.  Device memory, grow-only: 8 bytes a pixel of keys, 29 of outputs (32 with a colour image), 4 of cover when it is
// asked for, 25 bytes a vertex and 4 a triangle of scratch, and the rows of a mesh the caller gave.
#pragma once
#include "ekf_mesh_texture.hpp"

namespace ekf {

constexpr int kRastKinds = 4;                    // k_rast_project, k_rast_small, k_rast_large, k_rast_resolve
constexpr unsigned kRastSmallLimit = 16, kRastMaxSmallLimit = 65536, kRastLargeGrid = 1024;
constexpr unsigned long long kRastNoKey = ~0ull;

struct RastArgs {
  const double* xyz;                  // the source's rows
  const unsigned* faces;
  const unsigned char* grey;
  const unsigned char* bgr;           // NULL: no colour image from shading 0
  unsigned n_vert, n_tri;
  int W, H;
  double z_near;
  int cull, shading, want_cover;
  unsigned small_limit, large_grid;
  double fx, fy, cx, cy;
  double R[9], t[3];                  // x_cam = R^T (X - t)
  double* proj;                       // n_vert triples: p2, sx, sy
  unsigned char* usable;              // n_vert
  unsigned* list;                     // n_tri: the deferred triangles, in any order
  unsigned* cursor;                   // their number
  unsigned long long* keys;           // H rows of W, tight
  unsigned* cover;                    // likewise; read with want_cover only
  float* depth;                       // the outputs: H rows of W
  float* normal;                      //   x 3
  float* bary;                        //   x 2
  int* tri;
  unsigned char* out_grey;
  unsigned char* out_bgr;             //   x 3; NULL: no colour image
  const unsigned char* atlas;         // shading 1: A rows of A x C bytes, and its layout
  int P, B, Q, A, C;
};

#ifndef EKF_RASTER_HOST_ATOMICS
__device__ __forceinline__ void rast_key_min(unsigned long long* p, unsigned long long v) {
  __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
#endif

// Step 2's triangle: its indices, its projected corners (z is p2), its facing and its clamped box.
struct RastTri {
  unsigned i0, i1, i2;
  double x0, y0, z0, x1, y1, z1, x2, y2, z2;
  bool front;
  int bx0, bx1, by0, by1;
};

// Step 2 for triangle t < n_tri: false if it is dropped.
__device__ __forceinline__ bool rast_triangle(const RastArgs& a, unsigned t, RastTri& T) {
#pragma clang fp contract(off)
  T.i0 = a.faces[(size_t)t * 3];
  T.i1 = a.faces[(size_t)t * 3 + 1];
  T.i2 = a.faces[(size_t)t * 3 + 2];
  if (!(a.usable[T.i0] && a.usable[T.i1] && a.usable[T.i2])) return false;
  const double* p0 = a.proj + (size_t)T.i0 * 3;
  const double* p1 = a.proj + (size_t)T.i1 * 3;
  const double* p2 = a.proj + (size_t)T.i2 * 3;
  T.z0 = p0[0]; T.x0 = p0[1]; T.y0 = p0[2];
  T.z1 = p1[0]; T.x1 = p1[1]; T.y1 = p1[2];
  T.z2 = p2[0]; T.x2 = p2[1]; T.y2 = p2[2];
  const double area2 = (T.x1 - T.x0) * (T.y2 - T.y0) - (T.y1 - T.y0) * (T.x2 - T.x0);
  if (area2 == 0.0 || area2 != area2) return false;
  T.front = area2 < 0.0;
  if (a.cull && !T.front) return false;
  // the corners are finite, so the box is; it is clamped as a double and only then converted
  const double xl = fmax(0.0, ceil(fmin(fmin(T.x0, T.x1), T.x2))), xh = fmin((double)(a.W - 1), floor(fmax(fmax(T.x0, T.x1), T.x2)));
  const double yl = fmax(0.0, ceil(fmin(fmin(T.y0, T.y1), T.y2))), yh = fmin((double)(a.H - 1), floor(fmax(fmax(T.y0, T.y1), T.y2)));
  if (!(xl <= xh && yl <= yh)) return false;
  T.bx0 = (int)xl; T.bx1 = (int)xh; T.by0 = (int)yl; T.by1 = (int)yh;
  return true;
}

// Step 3's edge from corner a to corner b at the pixel: its e, and whether the pixel is inside it.
__device__ __forceinline__ bool rast_edge(unsigned ia, unsigned ib, double xa, double ya, double xb, double yb, double px, double py,
                                          bool front, double& e) {
#pragma clang fp contract(off)
  const bool canon = ia < ib;
  const double E = canon ? (xb - xa) * (py - ya) - (yb - ya) * (px - xa) : -((xa - xb) * (py - yb) - (ya - yb) * (px - xb));
  e = (front ? -1.0 : 1.0) * E;
  return e > 0.0 || (e == 0.0 && canon != front);
}

// Steps 3 and 4 for a pixel of the triangle's box: false unless it is covered and has a depth; z32 and the barycentrics.
__device__ __forceinline__ bool rast_pixel(const RastTri& T, int ipx, int ipy, float& z32, double& l0, double& l1, double& l2) {
#pragma clang fp contract(off)
  const double px = (double)ipx, py = (double)ipy;
  double e0, e1, e2;
  const bool in0 = rast_edge(T.i0, T.i1, T.x0, T.y0, T.x1, T.y1, px, py, T.front, e0);
  const bool in1 = rast_edge(T.i1, T.i2, T.x1, T.y1, T.x2, T.y2, px, py, T.front, e1);
  const bool in2 = rast_edge(T.i2, T.i0, T.x2, T.y2, T.x0, T.y0, px, py, T.front, e2);
  const double ssum = (e1 + e2) + e0;
  if (!(in0 && in1 && in2 && ssum > 0.0)) return false;
  const double w0 = (e1 / ssum) / T.z0, w1 = (e2 / ssum) / T.z1, w2 = (e0 / ssum) / T.z2;
  const double ws = (w0 + w1) + w2;
  const double z = 1.0 / ws;
  z32 = (float)z;
  if (!(ws > 0.0) || !(fabsf(z32) <= 3.402823466e38f)) return false;      // (a NaN and an infinity fail)
  l0 = w0 / ws;
  l1 = w1 / ws;
  l2 = w2 / ws;
  return true;
}

// A pixel of triangle t's box into the image of keys, and into the cover image if there is one.
__device__ __forceinline__ void rast_emit(const RastArgs& a, const RastTri& T, unsigned t, int px, int py) {
  float z32;
  double l0, l1, l2;
  if (!rast_pixel(T, px, py, z32, l0, l1, l2)) return;
  const size_t pix = (size_t)py * (size_t)a.W + (size_t)px;               // inside the image: the box is clamped to it
  rast_key_min(&a.keys[pix], ((unsigned long long)__builtin_bit_cast(unsigned, z32) << 32) | (unsigned long long)t);
  if (a.want_cover) seg_global_add(&a.cover[pix], 1u);
}

// One lane a source vertex: step 1.
__global__ void __launch_bounds__(256) k_rast_project(RastArgs a) {
#pragma clang fp contract(off)
  const unsigned v = blockIdx.x * (unsigned)kFusionBlock + threadIdx.x;
  if (v >= a.n_vert) return;
  const double* X = a.xyz + (size_t)v * 3;
  double sx, sy;
  const double p2 = tex_project(a, X[0], X[1], X[2], sx, sy);
  a.proj[(size_t)v * 3] = p2;
  a.proj[(size_t)v * 3 + 1] = sx;
  a.proj[(size_t)v * 3 + 2] = sy;
  a.usable[v] = (p2 > a.z_near && fabs(sx) <= 1.7976931348623157e308 && fabs(sy) <= 1.7976931348623157e308) ? 1 : 0;
}

// One lane a triangle: step 2, then its box if that is small, otherwise a place in the deferred list.
__global__ void __launch_bounds__(256) k_rast_small(RastArgs a) {
  const unsigned t = blockIdx.x * (unsigned)kFusionBlock + threadIdx.x;
  if (t >= a.n_tri) return;
  RastTri T;
  if (!rast_triangle(a, t, T)) return;
  const unsigned bw = (unsigned)(T.bx1 - T.bx0 + 1), bh = (unsigned)(T.by1 - T.by0 + 1);           // bw bh <= 2^26
  if (bw * bh > a.small_limit) {
    a.list[seg_global_add(a.cursor, 1u)] = t;    // a triangle is appended at most once: the cursor stays <= n_tri
    return;
  }
  for (int py = T.by0; py <= T.by1; ++py)
    for (int px = T.bx0; px <= T.bx1; ++px) rast_emit(a, T, t, px, py);
}

// One workgroup a deferred triangle, striding over the list; its lanes take the box's pixels 256 at a time, along its rows.
__global__ void __launch_bounds__(256) k_rast_large(RastArgs a) {
  const unsigned n = min(seg_global_load(a.cursor), a.n_tri);
  for (unsigned j = blockIdx.x; j < n; j += a.large_grid) {
    const unsigned t = a.list[j];
    RastTri T;
    if (!rast_triangle(a, t, T)) continue;       // (k_rast_small kept it, so it is kept)
    const unsigned bw = (unsigned)(T.bx1 - T.bx0 + 1), cnt = bw * (unsigned)(T.by1 - T.by0 + 1);
    for (unsigned i = threadIdx.x; i < cnt; i += (unsigned)kFusionBlock) {
      const unsigned row = i / bw;
      rast_emit(a, T, t, T.bx0 + (int)(i - row * bw), T.by0 + (int)row);
    }
  }
}

// Step 5's blend of three vertex values with the barycentrics.
__device__ __forceinline__ unsigned char rast_blend(double l0, double l1, double l2, unsigned char g0, unsigned char g1, unsigned char g2) {
#pragma clang fp contract(off)
  double v = floor(((l0 * (double)g0 + l1 * (double)g1) + l2 * (double)g2) + 0.5);
  v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
  return (unsigned char)(int)v;
}

// One lane a pixel, 8 x 8 pixels a wave: step 5.
__global__ void __launch_bounds__(256) k_rast_resolve(RastArgs a) {
#pragma clang fp contract(off)
  const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int px = (int)(blockIdx.x * (unsigned)kRaycastTile + (wave & 1) * 8 + (lane & 7));
  const int py = (int)(blockIdx.y * (unsigned)kRaycastTile + (wave >> 1) * 8 + (lane >> 3));
  if (px >= a.W || py >= a.H) return;
  const size_t pix = (size_t)py * (size_t)a.W + (size_t)px;
  float depth = 0.f, n0 = 0.f, n1 = 0.f, n2 = 0.f, b1 = 0.f, b2 = 0.f;
  int tri = -1;
  unsigned char g = 0, cb = 0, cg = 0, cr = 0;
  const unsigned long long key = a.keys[pix];
  RastTri T;
  float z32;
  double l0, l1, l2;
  const unsigned t = (unsigned)(key & 0xffffffffull);
  if (key != kRastNoKey && t < a.n_tri && rast_triangle(a, t, T) && rast_pixel(T, px, py, z32, l0, l1, l2)) {
    depth = z32;
    tri = (int)t;
    b1 = (float)l1;
    b2 = (float)l2;
    const double* X0 = a.xyz + (size_t)T.i0 * 3;
    const double* X1 = a.xyz + (size_t)T.i1 * 3;
    const double* X2 = a.xyz + (size_t)T.i2 * 3;
    const double u0 = X1[0] - X0[0], u1 = X1[1] - X0[1], u2 = X1[2] - X0[2];
    const double v0 = X2[0] - X0[0], v1 = X2[1] - X0[1], v2 = X2[2] - X0[2];
    const double m0 = u1 * v2 - u2 * v1, m1 = u2 * v0 - u0 * v2, m2 = u0 * v1 - u1 * v0;
    const double len = sqrt((m0 * m0 + m1 * m1) + m2 * m2);
    if (len > 0.0 && len <= 1.7976931348623157e308) {
      n0 = (float)(m0 / len);
      n1 = (float)(m1 / len);
      n2 = (float)(m2 / len);
    }
    if (a.shading == 0) {
      g = rast_blend(l0, l1, l2, a.grey[T.i0], a.grey[T.i1], a.grey[T.i2]);
      if (a.bgr) {
        cb = rast_blend(l0, l1, l2, a.bgr[(size_t)T.i0 * 3], a.bgr[(size_t)T.i1 * 3], a.bgr[(size_t)T.i2 * 3]);
        cg = rast_blend(l0, l1, l2, a.bgr[(size_t)T.i0 * 3 + 1], a.bgr[(size_t)T.i1 * 3 + 1], a.bgr[(size_t)T.i2 * 3 + 1]);
        cr = rast_blend(l0, l1, l2, a.bgr[(size_t)T.i0 * 3 + 2], a.bgr[(size_t)T.i1 * 3 + 2], a.bgr[(size_t)T.i2 * 3 + 2]);
      }
    } else {
      const unsigned q = t >> 1;
      const int bx = (int)(q % (unsigned)a.Q), by = (int)(q / (unsigned)a.Q);
      const bool upper = (t & 1u) != 0;
      const double c0 = upper ? (double)(a.P + 1) : 0.0;                   // c0 = (c0, c0), c1 = (c1x, c0), c2 = (c0, c1x)
      const double c1x = upper ? 2.0 : (double)(a.P - 1);
      double tx = ((l0 * c0 + l1 * c1x) + l2 * c0) + (double)(bx * a.B);
      double ty = ((l0 * c0 + l1 * c0) + l2 * c1x) + (double)(by * a.B);
      const double top = (double)(a.A - 1);
      tx = tx < 0.0 ? 0.0 : (tx > top ? top : tx);                         // (a NaN cannot arise: l and c are finite)
      ty = ty < 0.0 ? 0.0 : (ty > top ? top : ty);
      const int qx = (int)floor(tx * 32.0 + 0.5), qy = (int)floor(ty * 32.0 + 0.5);
      const int ix = qx >> 5, ax = qx & 31, iy = qy >> 5, ay = qy & 31;   // ix, iy in [0, A - 1]
      const int jx = min(ix + 1, a.A - 1), jy = min(iy + 1, a.A - 1);
      const size_t pitch = (size_t)a.A * (size_t)a.C;
      const unsigned char* r0 = a.atlas + (size_t)iy * pitch;
      const unsigned char* r1 = a.atlas + (size_t)jy * pitch;
      const size_t o0 = (size_t)ix * (size_t)a.C, o1 = (size_t)jx * (size_t)a.C;
      const unsigned w00 = (unsigned)((32 - ax) * (32 - ay)), w10 = (unsigned)(ax * (32 - ay));
      const unsigned w01 = (unsigned)((32 - ax) * ay), w11 = (unsigned)(ax * ay);
      if (a.C == 3) {
        cb = (unsigned char)((w00 * r0[o0] + w10 * r0[o1] + w01 * r1[o0] + w11 * r1[o1] + 512u) >> 10);
        cg = (unsigned char)((w00 * r0[o0 + 1] + w10 * r0[o1 + 1] + w01 * r1[o0 + 1] + w11 * r1[o1 + 1] + 512u) >> 10);
        cr = (unsigned char)((w00 * r0[o0 + 2] + w10 * r0[o1 + 2] + w01 * r1[o0 + 2] + w11 * r1[o1 + 2] + 512u) >> 10);
        g = (unsigned char)((cb * 1868u + cg * 9617u + cr * 4899u + 8192u) >> 14);
      } else {
        g = (unsigned char)((w00 * r0[o0] + w10 * r0[o1] + w01 * r1[o0] + w11 * r1[o1] + 512u) >> 10);
      }
    }
  }
  a.depth[pix] = depth;
  a.tri[pix] = tri;
  a.bary[pix * 2] = b1;
  a.bary[pix * 2 + 1] = b2;
  a.normal[pix * 3] = n0;
  a.normal[pix * 3 + 1] = n1;
  a.normal[pix * 3 + 2] = n2;
  a.out_grey[pix] = g;
  if (a.out_bgr) {
    a.out_bgr[pix * 3] = cb;
    a.out_bgr[pix * 3 + 1] = cg;
    a.out_bgr[pix * 3 + 2] = cr;
  }
}

#ifndef EKF_KERNELS_ONLY
// The atlas a render with shading 1 samples: TsdfTexture's, only read.
struct RastAtlas {
  const unsigned char* atlas = nullptr;
  int P = 0, B = 0, Q = 0, A = 0, C = 0;
};

// Host side: the keys, the images and the scratch of the rasteriser, owned by the fusion handle beside its TsdfTexture;
// grow-only.  The sources are only read.  A timer of its own, so that the other getters count what they counted.
struct TsdfRaster {
  DevBuf<unsigned long long> keys;
  DevBuf<float> depth, normal, bary;
  DevBuf<int> tri;
  DevBuf<unsigned char> grey, bgr, usable;
  DevBuf<unsigned> cover, list, cursor;
  DevBuf<double> proj;
  CallerMesh own;                                // source 4: the mesh ekf_raster_set_mesh was given
  int W = 0, H = 0;
  bool valid = false, has_bgr = false, has_cover = false;      // of the last render
  unsigned small_limit = kRastSmallLimit;
  KernelTimer<kRastKinds> timer;

  // grow -> memsets -> project -> small -> (large) -> resolve.  A failed allocation leaves the previous images as they were:
  // new buffers replace the old ones only when all of them exist.
  hipError_t render(const MeshView& s, const RastAtlas* tex, int width, int height, const double K[4], const double R[9], const double t[3],
                    double z_near, int cull, int want_cover) {
    hipError_t e;
    if ((e = timer.create()) != hipSuccess) return e;
    const size_t npix = (size_t)width * (size_t)height, nv = (size_t)s.n_vert, nt = (size_t)s.n_tri;
    const bool colour = tex ? tex->C == 3 : s.bgr != nullptr;
    if (npix > keys.capacity() || npix > depth.capacity() || npix * 3 > normal.capacity() || npix * 2 > bary.capacity() ||
        npix > tri.capacity() || npix > grey.capacity() || (colour && npix * 3 > bgr.capacity()) ||
        (want_cover && npix > cover.capacity()) || nv * 3 > proj.capacity() || nv > usable.capacity() || nt > list.capacity() ||
        1 > cursor.capacity()) {
      DevBuf<unsigned long long> n_keys;
      DevBuf<float> n_depth, n_normal, n_bary;
      DevBuf<int> n_tri;
      DevBuf<unsigned char> n_grey, n_bgr, n_usable;
      DevBuf<unsigned> n_cover, n_list, n_cursor;
      DevBuf<double> n_proj;
      const size_t cpix = (want_cover || cover.capacity() > 0) ? std::max(npix, cover.capacity()) : 0;
      const size_t bpix = (colour || bgr.capacity() > 0) ? std::max(npix * 3, bgr.capacity()) : 0;
      if ((e = n_keys.reserve(std::max(npix, keys.capacity()))) != hipSuccess || (e = n_depth.reserve(std::max(npix, depth.capacity()))) != hipSuccess ||
          (e = n_normal.reserve(std::max(npix * 3, normal.capacity()))) != hipSuccess ||
          (e = n_bary.reserve(std::max(npix * 2, bary.capacity()))) != hipSuccess || (e = n_tri.reserve(std::max(npix, tri.capacity()))) != hipSuccess ||
          (e = n_grey.reserve(std::max(npix, grey.capacity()))) != hipSuccess || (e = n_bgr.reserve(bpix)) != hipSuccess ||
          (e = n_cover.reserve(cpix)) != hipSuccess || (e = n_proj.reserve(std::max(nv * 3, proj.capacity()))) != hipSuccess ||
          (e = n_usable.reserve(std::max(nv, usable.capacity()))) != hipSuccess || (e = n_list.reserve(std::max(nt, list.capacity()))) != hipSuccess ||
          (e = n_cursor.reserve(1)) != hipSuccess) {
        (void)hipGetLastError();
        return e;
      }
      keys = std::move(n_keys); depth = std::move(n_depth); normal = std::move(n_normal); bary = std::move(n_bary); tri = std::move(n_tri);
      grey = std::move(n_grey); bgr = std::move(n_bgr); cover = std::move(n_cover); proj = std::move(n_proj); usable = std::move(n_usable);
      list = std::move(n_list); cursor = std::move(n_cursor);
    }
    valid = false;
    RastArgs a{};
    a.xyz = s.xyz; a.faces = s.faces; a.grey = s.grey; a.bgr = s.bgr;
    a.n_vert = (unsigned)s.n_vert; a.n_tri = (unsigned)s.n_tri;
    a.W = width; a.H = height; a.z_near = z_near; a.cull = cull; a.shading = tex ? 1 : 0; a.want_cover = want_cover;
    a.small_limit = small_limit; a.large_grid = (unsigned)std::min<unsigned long long>(s.n_tri, kRastLargeGrid);
    a.fx = K[0]; a.fy = K[1]; a.cx = K[2]; a.cy = K[3];
    for (int i = 0; i < 9; ++i) a.R[i] = R[i];
    for (int i = 0; i < 3; ++i) a.t[i] = t[i];
    a.proj = proj; a.usable = usable; a.list = list; a.cursor = cursor; a.keys = keys; a.cover = cover;
    a.depth = depth; a.normal = normal; a.bary = bary; a.tri = tri; a.out_grey = grey; a.out_bgr = colour ? (unsigned char*)bgr : nullptr;
    if (tex) { a.atlas = tex->atlas; a.P = tex->P; a.B = tex->B; a.Q = tex->Q; a.A = tex->A; a.C = tex->C; }
    if ((e = hipMemsetAsync(keys, 0xff, npix * sizeof(unsigned long long), nullptr)) != hipSuccess) return e;
    if (want_cover && (e = hipMemsetAsync(cover, 0, npix * sizeof(unsigned), nullptr)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(cursor, 0, sizeof(unsigned), nullptr)) != hipSuccess) return e;
    if ((e = timer.run(0, [&] { k_rast_project<<<fusion_blocks(a.n_vert), kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
    if ((e = timer.run(1, [&] { k_rast_small<<<fusion_blocks(a.n_tri), kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
    if ((unsigned long long)small_limit < (unsigned long long)npix &&       // otherwise no box is larger than the limit
        (e = timer.run(2, [&] { k_rast_large<<<a.large_grid, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess)
      return e;
    const dim3 grid((unsigned)((width + kRaycastTile - 1) / kRaycastTile), (unsigned)((height + kRaycastTile - 1) / kRaycastTile));
    if ((e = timer.run(3, [&] { k_rast_resolve<<<grid, kRaycastTile * kRaycastTile, 0, nullptr>>>(a); })) != hipSuccess) return e;
    W = width; H = height; has_bgr = colour; has_cover = want_cover != 0;
    valid = true;
    return hipSuccess;
  }
};
#endif  // EKF_KERNELS_ONLY

}  // namespace ekf
