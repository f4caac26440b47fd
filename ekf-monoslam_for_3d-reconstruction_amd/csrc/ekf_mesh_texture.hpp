// A per-triangle texture atlas for the welded, the pruned, the smoothed or the simplified mesh, filled on the device from views
// that are fed one at a time.  The reference has no counterpart; the contract is pinned here and restated in
// numpy, twice, by tests/texture_oracle.py.  The input is a source mesh (X fp64, F uint32, the vertex grey and, of a colour
// volume, B, G, R) with n_tri > 0 triangles, a patch size P in 2..32 and `channels`, 1 or 3.  Every fp64 operation is rounded
// once, in the written order, with contraction off:
//   1. the layout.  Triangles are paired into square blocks of side B = P + 2 texels: block q = t >> 1 holds triangle 2 q (the
//      lower one) and 2 q + 1 (the upper one).  n_sq = (n_tri + 1) >> 1, Q the least integer with Q Q >= n_sq, the atlas is
//      A x A texels with A = Q B, row 0 first; block q sits at (bx, by) = (q % Q, q / Q).  The texel with block-local
//      coordinates (a, b) belongs to the lower triangle iff a + b <= P, otherwise to the upper one.  Corner texel centres:
//      lower c0 = (0, 0), c1 = (P - 1, 0), c2 = (0, P - 1); upper c0 = (P + 1, P + 1), c1 = (2, P + 1), c2 = (P + 1, 2): a
//      bilinear look-up inside a triangle's UV triangle touches texels of that triangle only; the diagonals a + b = P and P + 1
//      are gutters, filled by extrapolation.  Barycentrics of a texel: lower l1 = (double) a / (double)(P - 1),
//      l2 = (double) b / (double)(P - 1); upper l1 = (double)(P + 1 - a) / (double)(P - 1), l2 = (double)(P + 1 - b) /
//      (double)(P - 1); l0 = (1.0 - l1) - l2 (slightly negative in a gutter).  UV of corner i of triangle t:
//      ((double)(bx B + c_i.x) + 0.5) / (double) A and likewise for y, from row 0: a function of n_tri and P alone, made on
//      the host (tex_uv), without a launch;
//   2. a vertex in a view (an image of W x H, K = fx fy cx cy, a pose, an optional z-buffer): d = X - t, p = R^T d,
//      sx = fx (p0 / p2) + cx, sy = fy (p1 / p2) + cy: tsdf_sample's operations in its order.  It is visible iff p2 > 0,
//      0 <= sx <= W - 1 and 0 <= sy <= H - 1 (a NaN fails) and, with occlusion on, D = (double) zbuf[floor(sy + 0.5) W +
//      floor(sx + 0.5)] has D > 0 and p2 <= D + tol.  D == 0 (the ray cast found no surface) fails: the conservative choice;
//   3. a triangle in a view is a candidate iff its three vertices are visible.  Its score is sigma ((sx1 - sx0) (sy2 - sy0) -
//      (sy1 - sy0) (sx2 - sx0)), twice its signed area in pixels, with sigma = -1: the weld's triangles have (B - A) x (C - A)
//      towards free space (ekf_fusion.hpp), the image's y runs downwards, so a triangle seen from the free-space side scores
//      positive (tests/test_oracle_texture.py holds that on the sphere).  The view wins triangle t iff score > min_area2 and
//      score > best_score[t]; best_score starts at 0 and best_view at -1; the strict > lets the earlier view keep a tie.  A
//      view's number is the count of views added since begin;
//   4. the fill, for every texel of a triangle that the current view has just won: Xp = (l0 X0 + l1 X1) + l2 X2 per coordinate,
//      projected as in 2; if !(p2 > 0) or sx or sy is NaN the texel is left as it is; sx is clamped to [0, W - 1] and sy to
//      [0, H - 1]; the sample is k_frame_rectify's blend: q = (int) floor(s 32 + 0.5), i = q >> 5, alpha = q & 31, the second
//      tap min(i + 1, dim - 1), the weights (32 - ax)(32 - ay) and so on, the value (sum w tap + 512) >> 10; after the clamp
//      all four taps are inside the image.  A 3-channel atlas takes B, G, R, a grey view replicates its value; a 1-channel
//      atlas takes the view's grey image (of a colour view: its bgr2gray image);
//   5. the finish: the texels of a triangle with best_view = -1 get, per channel, floor(((l0 g0 + l1 g1) + l2 g2) + 0.5) clamped
//      to 0..255, g the source's vertex grey, or its B, G, R on a colour volume with a 3-channel atlas.  Padding (t >= n_tri)
//      stays 0.  n_textured is the number of triangles with a view.
//
// The launches, 256 lanes a workgroup, on the default stream; vblk = ceil(n_vert / 256), tblk = ceil(n_tri / 256),
// ablk = ceil(n_texel / 256), n_texel = A B ceil(n_sq / Q): the block rows that hold a triangle (none for padding alone):
//                (hipMemsetAsync: the view's two counters = 0)
//   k_tex_project    vblk    a view: sx, sy and the visible flag of every source vertex into scratch (17 bytes a vertex)
//   k_tex_select     tblk    a view: best_score, best_view and the flag "won now" of every triangle; the workgroup's triangles
//                            won and won for the first time, reduced in LDS, one integer add each a workgroup that has any
//                one read-back of the two counters
//   k_tex_fill       ablk    a view that won a triangle: one lane a texel, along the atlas's rows; a texel whose triangle is not
//                            flagged is left
//   k_tex_fallback   ablk    finish: one lane a texel
// A triangle and a texel belong to one lane; the only atomics are those two integer adds a workgroup, exact in any order.  No
// kernel has a per-lane array and none uses scratch memory.  Device memory: A A channels bytes of atlas, 13 bytes a triangle
// (best_score, best_view, won), 17 bytes a source vertex, 8 bytes of counters and, for a view from the host, its image.
#pragma once
#include "ekf_mesh_simplify.hpp"

namespace ekf {

constexpr int kTexKinds = 4;                     // k_tex_project, k_tex_select, k_tex_fill, k_tex_fallback
constexpr int kTexMinPatch = 2, kTexMaxPatch = 32, kTexMaxSide = 16384;
constexpr double kTexSigma = -1.0;               // step 3's sigma

struct TexArgs {
  const double* xyz;                  // the source's rows
  const unsigned* faces;
  const unsigned char* grey;
  const unsigned char* bgr;           // NULL unless a colour volume and a 3-channel atlas
  unsigned n_vert, n_tri;
  int P, B, Q, A, C;                  // the layout: patch, block side, blocks a row, atlas side, channels
  unsigned n_texel;                   // A texels a row times the rows of the block rows that hold a triangle: the rest is padding
  unsigned char* atlas;               // A rows of A x C bytes, tight
  double* best_score;                 // n_tri each
  int* best_view;
  unsigned char* won;                 //   1 iff the current view has just won the triangle
  double* sxy;                        // n_vert pairs: sx, sy of the current view
  unsigned char* vis;                 // n_vert: its visible flag
  unsigned* counts;                   // the current view's triangles won, and won for the first time
  // the current view
  const unsigned char* img;           // H rows of W x vch bytes, tight
  int vch;                            // 1: grey, 3: B, G, R
  int W, H, view;
  const float* zbuf;                  // H rows of W floats, tight: the depths of a ray cast; NULL = occlusion off
  double tol, min_area2;
  double fx, fy, cx, cy;
  double R[9], t[3];                  // x_cam = R^T (X - t)
};

// Step 2's projection: p2 (the caller tests it), sx and sy.  `a` is whatever holds the view's K, R and t: the rasteriser of
// ekf_mesh_raster.hpp projects through this function too.
template <typename Args>
__device__ __forceinline__ double tex_project(const Args& a, double X0, double X1, double X2, double& sx, double& sy) {
#pragma clang fp contract(off)
  const double d0 = X0 - a.t[0], d1 = X1 - a.t[1], d2 = X2 - a.t[2];
  const double p0 = a.R[0] * d0 + a.R[3] * d1 + a.R[6] * d2;
  const double p1 = a.R[1] * d0 + a.R[4] * d1 + a.R[7] * d2;
  const double p2 = a.R[2] * d0 + a.R[5] * d1 + a.R[8] * d2;
  sx = a.fx * (p0 / p2) + a.cx;
  sy = a.fy * (p1 / p2) + a.cy;
  return p2;
}

// Step 1 for the texel of linear index i < n_texel (x = i % A along the lanes): false for padding, otherwise its triangle and
// its barycentrics.
__device__ __forceinline__ bool tex_texel(const TexArgs& a, unsigned i, unsigned& t, double& l0, double& l1, double& l2) {
#pragma clang fp contract(off)
  const unsigned A = (unsigned)a.A, B = (unsigned)a.B;
  const unsigned y = i / A, x = i - y * A;
  const unsigned by = y / B, lb = y - by * B, bx = x / B, la = x - bx * B;
  const bool upper = la + lb > (unsigned)a.P;
  t = 2u * (by * (unsigned)a.Q + bx) + (upper ? 1u : 0u);   // < 2 Q Q <= 2^31
  if (t >= a.n_tri) return false;
  const double den = (double)(a.P - 1);
  l1 = (double)(upper ? (unsigned)a.P + 1u - la : la) / den;
  l2 = (double)(upper ? (unsigned)a.P + 1u - lb : lb) / den;
  l0 = (1.0 - l1) - l2;
  return true;
}

// One lane a source vertex: step 2.
__global__ void __launch_bounds__(256) k_tex_project(TexArgs a) {
#pragma clang fp contract(off)
  const unsigned v = blockIdx.x * (unsigned)kFusionBlock + threadIdx.x;
  if (v >= a.n_vert) return;
  const double* X = a.xyz + (size_t)v * 3;
  double sx, sy;
  const double p2 = tex_project(a, X[0], X[1], X[2], sx, sy);
  bool ok = p2 > 0.0 && sx >= 0.0 && sx <= (double)(a.W - 1) && sy >= 0.0 && sy <= (double)(a.H - 1);      // (a NaN fails)
  if (ok && a.zbuf) {                 // floor(s + 0.5) lies in 0 .. dim - 1: s does
    const double D = (double)a.zbuf[(size_t)(int)floor(sy + 0.5) * (size_t)a.W + (size_t)(int)floor(sx + 0.5)];
    ok = D > 0.0 && p2 <= D + a.tol;
  }
  a.sxy[(size_t)v * 2] = sx;
  a.sxy[(size_t)v * 2 + 1] = sy;
  a.vis[v] = ok ? 1 : 0;
}

// One lane a triangle: step 3.  The triangles the view won, and those among them that had no view, are summed over the
// workgroup in LDS (both fit 16 bits: at most 256 each); lane 0 adds what is not zero to the two counters.
__global__ void __launch_bounds__(256) k_tex_select(TexArgs a) {
#pragma clang fp contract(off)
  __shared__ unsigned s_n[kFusionBlock];
  const unsigned tid = threadIdx.x, t = blockIdx.x * (unsigned)kFusionBlock + tid;
  unsigned mine = 0u;
  if (t < a.n_tri) {
    const unsigned v0 = a.faces[(size_t)t * 3], v1 = a.faces[(size_t)t * 3 + 1], v2 = a.faces[(size_t)t * 3 + 2];
    bool win = a.vis[v0] && a.vis[v1] && a.vis[v2];
    if (win) {
      const double x0 = a.sxy[(size_t)v0 * 2], y0 = a.sxy[(size_t)v0 * 2 + 1];
      const double x1 = a.sxy[(size_t)v1 * 2], y1 = a.sxy[(size_t)v1 * 2 + 1];
      const double x2 = a.sxy[(size_t)v2 * 2], y2 = a.sxy[(size_t)v2 * 2 + 1];
      const double score = kTexSigma * ((x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0));
      win = score > a.min_area2 && score > a.best_score[t];
      if (win) {
        mine = a.best_view[t] < 0 ? 0x10001u : 1u;
        a.best_score[t] = score;
        a.best_view[t] = a.view;
      }
    }
    a.won[t] = win ? 1 : 0;
  }
  s_n[tid] = mine;
  __syncthreads();
  for (unsigned h = kFusionBlock / 2; h > 0; h >>= 1) {
    if (tid < h) s_n[tid] += s_n[tid + h];
    __syncthreads();
  }
  if (tid == 0 && s_n[0] != 0u) {
    seg_global_add(&a.counts[0], s_n[0] & 0xffffu);
    if (s_n[0] >> 16) seg_global_add(&a.counts[1], s_n[0] >> 16);
  }
}

// One lane a texel, x along the lanes: step 4 where the texel's triangle is flagged.  The lanes of a row of a block share a
// triangle, so its flag, its three indices and its nine coordinates are the same addresses across them; the taps of
// neighbouring texels are neighbouring pixels; the stores of a wave are consecutive bytes.
__global__ void __launch_bounds__(256) k_tex_fill(TexArgs a) {
#pragma clang fp contract(off)
  const unsigned i = blockIdx.x * (unsigned)kFusionBlock + threadIdx.x;
  if (i >= a.n_texel) return;
  unsigned t;
  double l0, l1, l2;
  if (!tex_texel(a, i, t, l0, l1, l2) || !a.won[t]) return;
  const double* X0 = a.xyz + (size_t)a.faces[(size_t)t * 3] * 3;
  const double* X1 = a.xyz + (size_t)a.faces[(size_t)t * 3 + 1] * 3;
  const double* X2 = a.xyz + (size_t)a.faces[(size_t)t * 3 + 2] * 3;
  const double P0 = (l0 * X0[0] + l1 * X1[0]) + l2 * X2[0];
  const double P1 = (l0 * X0[1] + l1 * X1[1]) + l2 * X2[1];
  const double P2 = (l0 * X0[2] + l1 * X1[2]) + l2 * X2[2];
  double sx, sy;
  const double p2 = tex_project(a, P0, P1, P2, sx, sy);
  if (!(p2 > 0.0) || sx != sx || sy != sy) return;
  const double mx = (double)(a.W - 1), my = (double)(a.H - 1);
  sx = sx < 0.0 ? 0.0 : (sx > mx ? mx : sx);
  sy = sy < 0.0 ? 0.0 : (sy > my ? my : sy);
  const int qx = (int)floor(sx * 32.0 + 0.5), qy = (int)floor(sy * 32.0 + 0.5);
  const int ix = qx >> 5, ax = qx & 31, iy = qy >> 5, ay = qy & 31;            // ix in [0, W - 1], iy in [0, H - 1]
  const int jx = min(ix + 1, a.W - 1), jy = min(iy + 1, a.H - 1);
  const size_t pitch = (size_t)a.W * (size_t)a.vch;
  const unsigned char* r0 = a.img + (size_t)iy * pitch;
  const unsigned char* r1 = a.img + (size_t)jy * pitch;
  const size_t o0 = (size_t)ix * (size_t)a.vch, o1 = (size_t)jx * (size_t)a.vch;
  const unsigned w00 = (unsigned)((32 - ax) * (32 - ay)), w10 = (unsigned)(ax * (32 - ay));
  const unsigned w01 = (unsigned)((32 - ax) * ay), w11 = (unsigned)(ax * ay);
  unsigned char* out = a.atlas + (size_t)i * (size_t)a.C;
  if (a.vch == 3) {                   // (uniform: a kernel argument) a colour view, so a 3-channel atlas
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
      out[ch] = (unsigned char)((w00 * r0[o0 + ch] + w10 * r0[o1 + ch] + w01 * r1[o0 + ch] + w11 * r1[o1 + ch] + 512u) >> 10);
  } else {
    const unsigned char g = (unsigned char)((w00 * r0[o0] + w10 * r0[o1] + w01 * r1[o0] + w11 * r1[o1] + 512u) >> 10);
    out[0] = g;
    if (a.C == 3) {
      out[1] = g;
      out[2] = g;
    }
  }
}

// One lane a texel: step 5 where the texel's triangle has no view.
__global__ void __launch_bounds__(256) k_tex_fallback(TexArgs a) {
#pragma clang fp contract(off)
  const unsigned i = blockIdx.x * (unsigned)kFusionBlock + threadIdx.x;
  if (i >= a.n_texel) return;
  unsigned t;
  double l0, l1, l2;
  if (!tex_texel(a, i, t, l0, l1, l2) || a.best_view[t] >= 0) return;
  const size_t v0 = a.faces[(size_t)t * 3], v1 = a.faces[(size_t)t * 3 + 1], v2 = a.faces[(size_t)t * 3 + 2];
  unsigned char* out = a.atlas + (size_t)i * (size_t)a.C;
  for (int ch = 0; ch < a.C; ++ch) {
    const double g0 = (double)(a.bgr ? a.bgr[v0 * 3 + ch] : a.grey[v0]);
    const double g1 = (double)(a.bgr ? a.bgr[v1 * 3 + ch] : a.grey[v1]);
    const double g2 = (double)(a.bgr ? a.bgr[v2 * 3 + ch] : a.grey[v2]);
    double v = floor(((l0 * g0 + l1 * g1) + l2 * g2) + 0.5);
    v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
    out[ch] = (unsigned char)(int)v;
  }
}

// Step 1's numbers for n_tri triangles and a patch of P: B, Q and A (A may exceed kTexMaxSide: the caller refuses that).
inline void tex_layout(unsigned long long n_tri, int P, int& B, long long& Q, long long& A) {
  const unsigned long long n_sq = (n_tri + 1) >> 1;
  unsigned long long q = (unsigned long long)std::sqrt((double)n_sq);
  while (q * q < n_sq) ++q;
  while (q > 0 && (q - 1) * (q - 1) >= n_sq) --q;
  B = P + 2;
  Q = (long long)q;
  A = (long long)q * B;
}

// The six UV coordinates of triangle t: u and v of its corners 0, 1 and 2, v measured from row 0.
inline void tex_uv(unsigned long long t, int P, int B, long long Q, long long A, double uv[6]) {
#pragma clang fp contract(off)
  const unsigned long long q = t >> 1;
  const long long bx = (long long)(q % (unsigned long long)Q), by = (long long)(q / (unsigned long long)Q);
  const bool upper = (t & 1ull) != 0;
  const int c[3][2] = {{upper ? P + 1 : 0, upper ? P + 1 : 0}, {upper ? 2 : P - 1, upper ? P + 1 : 0}, {upper ? P + 1 : 0, upper ? 2 : P - 1}};
  for (int i = 0; i < 3; ++i) {
    uv[2 * i] = ((double)(bx * B + c[i][0]) + 0.5) / (double)A;
    uv[2 * i + 1] = ((double)(by * B + c[i][1]) + 0.5) / (double)A;
  }
}

#ifndef EKF_KERNELS_ONLY
// Host side: the atlas, the per-triangle state and the scratch of the texture, owned by the fusion handle beside its
// TsdfSimplify; (re)allocated by begin, grow-only.  The source mesh is only read.  A timer of its own, so that the other getters
// count what they counted.
struct TsdfTexture {
  DevBuf<unsigned char> atlas, won, vis, d_img;
  DevBuf<double> best_score, sxy;
  DevBuf<int> best_view;
  DevBuf<unsigned> counts;
  MeshView src;                                  // the mesh begin was given: its arrays, read while the texture is current
  int P = 0, B = 0, C = 0;
  long long Q = 0, A = 0;
  bool colour = false;                           // the fallback reads the source's B, G, R
  bool finished = false;
  int views = 0;
  unsigned long long n_textured = 0;
  KernelTimer<kTexKinds> timer;

  // New buffers beside the old ones, which they replace only when all of them exist: a failed allocation leaves the texture begun
  // before as it was.  Then everything is cleared; the buffers may be that texture's own, so from the first clear on the handle
  // has no texture until all four clears are queued.  (d_img, the staging image of a view from the host, grows by itself: a
  // failed reserve loses only that image and adds no view.)
  hipError_t begin(MeshStamps& st, const MeshView& s, int source, int patch, int channels, bool use_bgr) {
    hipError_t e;
    if ((e = timer.create()) != hipSuccess) return e;
    int b;
    long long q, side;
    tex_layout(s.n_tri, patch, b, q, side);
    const size_t na = (size_t)side * (size_t)side * (size_t)channels, nt = (size_t)s.n_tri, nv = (size_t)s.n_vert;
    if (na > atlas.capacity() || nt > won.capacity() || nt > best_score.capacity() || nt > best_view.capacity() ||
        nv > vis.capacity() || nv * 2 > sxy.capacity() || 2 > counts.capacity()) {
      DevBuf<unsigned char> n_atlas, n_won, n_vis;
      DevBuf<double> n_score, n_sxy;
      DevBuf<int> n_view;
      DevBuf<unsigned> n_counts;
      if ((e = n_atlas.reserve(na)) != hipSuccess || (e = n_won.reserve(nt)) != hipSuccess || (e = n_vis.reserve(nv)) != hipSuccess ||
          (e = n_score.reserve(nt)) != hipSuccess || (e = n_sxy.reserve(nv * 2)) != hipSuccess || (e = n_view.reserve(nt)) != hipSuccess ||
          (e = n_counts.reserve(2)) != hipSuccess) {
        (void)hipGetLastError();
        return e;
      }
      atlas = std::move(n_atlas); won = std::move(n_won); vis = std::move(n_vis); best_score = std::move(n_score);
      sxy = std::move(n_sxy); best_view = std::move(n_view); counts = std::move(n_counts);
    }
    st.tex.valid = false;
    if ((e = hipMemsetAsync(atlas, 0, na, nullptr)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(best_score, 0, nt * sizeof(double), nullptr)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(best_view, 0xff, nt * sizeof(int), nullptr)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(won, 0, nt, nullptr)) != hipSuccess) return e;
    src = s;
    P = patch; B = b; Q = q; A = side; C = channels; colour = use_bgr;
    views = 0; n_textured = 0;
    finished = false;
    st.made(st.tex, s.id, source);
    return hipSuccess;
  }

  // the texels of the block rows that hold a triangle (nothing is launched for rows of padding alone)
  unsigned n_texel() const {
    const unsigned long long n_sq = (src.n_tri + 1) >> 1, rows = (n_sq + (unsigned long long)Q - 1) / (unsigned long long)Q;
    return (unsigned)(rows * (unsigned long long)B * (unsigned long long)A);
  }

  TexArgs args() const {
    TexArgs a{};
    a.xyz = src.xyz; a.faces = src.faces; a.grey = src.grey; a.bgr = colour ? src.bgr : nullptr;
    a.n_vert = (unsigned)src.n_vert; a.n_tri = (unsigned)src.n_tri;
    a.P = P; a.B = B; a.Q = (int)Q; a.A = (int)A; a.C = C; a.n_texel = n_texel();
    a.atlas = atlas; a.best_score = best_score; a.best_view = best_view; a.won = won; a.sxy = sxy; a.vis = vis; a.counts = counts;
    return a;
  }

  // memset -> project -> select -> one read-back of the two counters -> (fill, if the view won a triangle).
  hipError_t add_view(const unsigned char* img, int vch, int W, int H, const double K[4], const double R[9], const double t[3],
                      const float* zbuf, double tol, double min_area2, unsigned long long* n_won) {
    hipError_t e;
    TexArgs a = args();
    a.img = img; a.vch = vch; a.W = W; a.H = H; a.view = views; a.zbuf = zbuf; a.tol = tol; a.min_area2 = min_area2;
    a.fx = K[0]; a.fy = K[1]; a.cx = K[2]; a.cy = K[3];
    for (int i = 0; i < 9; ++i) a.R[i] = R[i];
    for (int i = 0; i < 3; ++i) a.t[i] = t[i];
    if ((e = hipMemsetAsync(counts, 0, 2 * sizeof(unsigned), nullptr)) != hipSuccess) return e;
    if ((e = timer.run(0, [&] { k_tex_project<<<fusion_blocks(a.n_vert), kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
    if ((e = timer.run(1, [&] { k_tex_select<<<fusion_blocks(a.n_tri), kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
    unsigned got[2] = {0, 0};
    if ((e = hipMemcpy(got, counts, sizeof(got), hipMemcpyDeviceToHost)) != hipSuccess) return e;
    ++views;
    n_textured += got[1];
    const unsigned ablk = fusion_blocks(a.n_texel);
    if (got[0] > 0 && (e = timer.run(2, [&] { k_tex_fill<<<ablk, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
    *n_won = got[0];
    return hipSuccess;
  }

  hipError_t finish() {
    const TexArgs a = args();
    const unsigned ablk = fusion_blocks(a.n_texel);
    const hipError_t e = timer.run(3, [&] { k_tex_fallback<<<ablk, kFusionBlock, 0, nullptr>>>(a); });
    if (e == hipSuccess) finished = true;
    return e;
  }
};
#endif  // EKF_KERNELS_ONLY

}  // namespace ekf
