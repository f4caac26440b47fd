// Fusion of key-frame depth maps into a truncated signed distance volume and the extraction of a triangle mesh by marching
// tetrahedra.  A volume of nx x ny x nz voxels keeps three planes, each x-contiguous (lin = i + nx (j + ny k)):
// the running sum of truncated distances (fp32), the number of maps that touched the voxel (uint16) and the sum of the grey
// values they saw (uint32).  The reference has no counterpart; the arithmetic is pinned here and restated in numpy by
// tests/fusion_oracle.py:
//   - every coordinate operation is fp64, rounded once, in the written left-to-right order; contraction is off in every
//     function below (host and device), as in ekf_dense_stereo.hpp; poses go through dense_pose unchanged;
//   - no atomics: a voxel belongs to one lane, and the mesh is written at offsets of a two-level exclusive scan, so the
//     output order is fixed (cells by lin of their corner 0, tetrahedra 0..5, table order).
// A colour volume keeps three more uint32 planes, the sums of the B, G and R values, and has two kernels of
// its own: k_tsdf_integrate_colour and k_tsdf_colour_vertices; tests/colour_oracle.py restates them.
// Nothing here touches a filter, counts as a launch kind or runs a collective.
#pragma once
#include <cmath>
#include <cstddef>
#include <string>
#include <utility>

// EKF_KERNELS_ONLY: the structs and the kernel bodies alone, for tools/fusion_host_check.cpp, which runs the kernels lane
// by lane on the host; tools/host_kernels.hpp supplies threadIdx, __syncthreads and the like.
#ifndef EKF_KERNELS_ONLY
#include <hip/hip_runtime.h>

#include "ekf_buffers.hpp"
#endif
#include "ekf_pixel.hpp"

namespace ekf {

constexpr int kFusionMaxDim = 1024, kFusionMaxMaps = 65535, kFusionMaxMapDim = 8192;
constexpr long long kFusionMaxVoxels = 1ll << 28;
constexpr int kFusionBlock = 256;                // cells per workgroup of the extraction, voxels per workgroup of the integration
// the workgroups of a launch with one lane for each of n items
inline unsigned fusion_blocks(unsigned long long n) { return (unsigned)((n + kFusionBlock - 1) / kFusionBlock); }

struct TsdfGrid {
  int nx, ny, nz;
  double origin[3], voxel;
};

struct IntegrateArgs {
  float* sum;
  unsigned short* cnt;
  unsigned* gsum;
  const float* depth;                 // H rows of W floats, tight; 0 = none
  const unsigned char* img;           // H rows of W bytes, tight
  int W, H;
  TsdfGrid g;
  double trunc;
  double fx, fy, cx, cy;
  double R[9], t[3];                  // the map's pose: x_cam = R^T (X - t)
};

// The voxel of a lane against the map: false where the voxel is skipped (past the volume, behind the camera, outside the
// image, no depth, more than trunc behind the surface), otherwise the pixel it samples and its truncated distance, rounded to
// fp32 once as the sum takes it.  The one body of both integration kernels.
__device__ __forceinline__ bool tsdf_sample(const IntegrateArgs& a, unsigned lin, size_t& pix, float& tau) {
#pragma clang fp contract(off)
  const unsigned nx = (unsigned)a.g.nx, ny = (unsigned)a.g.ny;
  if (lin >= nx * ny * (unsigned)a.g.nz) return false;
  const unsigned row = lin / nx, i = lin - row * nx;
  const unsigned k = row / ny, j = row - k * ny;
  const double d0 = (a.g.origin[0] + (double)i * a.g.voxel) - a.t[0];
  const double d1 = (a.g.origin[1] + (double)j * a.g.voxel) - a.t[1];
  const double d2 = (a.g.origin[2] + (double)k * a.g.voxel) - a.t[2];
  const double p0 = a.R[0] * d0 + a.R[3] * d1 + a.R[6] * d2;
  const double p1 = a.R[1] * d0 + a.R[4] * d1 + a.R[7] * d2;
  const double p2 = a.R[2] * d0 + a.R[5] * d1 + a.R[8] * d2;
  if (!(p2 > 0.0)) return false;
  const double sx = a.fx * (p0 / p2) + a.cx;
  const double sy = a.fy * (p1 / p2) + a.cy;
  const double fjx = floor(sx + 0.5), fjy = floor(sy + 0.5);
  if (!(fjx >= 0.0 && fjx <= (double)(a.W - 1) && fjy >= 0.0 && fjy <= (double)(a.H - 1))) return false;   // (a NaN fails)
  pix = (size_t)(int)fjy * (size_t)a.W + (size_t)(int)fjx;
  const double zs = (double)a.depth[pix];
  if (zs == 0.0) return false;
  const double s = zs - p2;
  if (s < -a.trunc) return false;
  tau = (float)((s >= a.trunc) ? 1.0 : s / a.trunc);
  return true;
}

// One lane per voxel, x along the lanes: the loads and stores of the three planes are contiguous across a wave, and a voxel
// that is skipped (behind the camera, outside the image, no depth, more than trunc behind the surface) touches none of them.
__global__ void __launch_bounds__(256) k_tsdf_integrate(IntegrateArgs a) {
  const unsigned lin = blockIdx.x * (unsigned)kFusionBlock + threadIdx.x;
  size_t pix;
  float tau;
  if (!tsdf_sample(a, lin, pix, tau)) return;
  a.sum[lin] = a.sum[lin] + tau;
  a.cnt[lin] = (unsigned short)(a.cnt[lin] + 1);
  a.gsum[lin] = a.gsum[lin] + (unsigned)a.img[pix];
}

// ---- colour volumes ------------------------------------------------------------------------------------------
struct IntegrateColourArgs {
  IntegrateArgs g;                    // g.img is read only where bgr is NULL
  const unsigned char* bgr;           // H rows of W x 3 bytes, tight: B, G, R; NULL = a map without colour
  unsigned* csum;                     // three planes of nvox back to back: the sums of B, G and R
  size_t nvox;
};

// k_tsdf_integrate for a colour volume: the same voxels, the same sum and cnt; gsum takes bgr2gray of the pixel and csum[c] its
// channel c (exactly three byte reads at 3 pix).  A map without colour (a uniform branch: bgr is a kernel argument) adds its
// grey value to all three colour planes, so that the one count plane serves all four sums.
__global__ void __launch_bounds__(256) k_tsdf_integrate_colour(IntegrateColourArgs c) {
  const unsigned lin = blockIdx.x * (unsigned)kFusionBlock + threadIdx.x;
  size_t pix;
  float tau;
  if (!tsdf_sample(c.g, lin, pix, tau)) return;
  unsigned b, g, r, grey;
  if (c.bgr) {
    const unsigned char* p = c.bgr + 3 * pix;
    b = p[0]; g = p[1]; r = p[2];
    grey = bgr2gray(b, g, r);
  } else {
    b = g = r = grey = (unsigned)c.g.img[pix];
  }
  c.g.sum[lin] = c.g.sum[lin] + tau;
  c.g.cnt[lin] = (unsigned short)(c.g.cnt[lin] + 1);
  c.g.gsum[lin] = c.g.gsum[lin] + grey;
  c.csum[lin] = c.csum[lin] + b;
  c.csum[c.nvox + lin] = c.csum[c.nvox + lin] + g;
  c.csum[2 * c.nvox + lin] = c.csum[2 * c.nvox + lin] + r;
}

// ---- extraction ------------------------------------------------------------------------------------------------------------
// Corners of a cell are numbered c = dx + 2 dy + 4 dz.  The six Kuhn tetrahedra round the diagonal 0-7, all of one
// orientation: tetrahedron t = (0, kTetC1[t], kTetC2[t], 7) = (0,1,3,7) (0,3,2,7) (0,2,6,7) (0,6,4,7) (0,4,5,7) (0,5,1,7).
// Tet-local edges e = 0..5 join the tet-local vertices (0,1) (0,2) (0,3) (1,2) (1,3) (2,3).  tet_tris(mask), bit i of mask =
// tet-local vertex i is inside: up to two triangles of tet-local edges, three bits an edge, the first triangle in the low
// nine bits; the normal ((B - A) x (C - A)) points to the outside.  tests/fusion_oracle.py carries the same table.
__device__ __forceinline__ int tet_corner(int t, int v) {      // cube corner of tet-local vertex v of tetrahedron t
  constexpr int kTetC1 = 1 | 3 << 3 | 2 << 6 | 6 << 9 | 4 << 12 | 5 << 15;   // 1 3 2 6 4 5, three bits each
  constexpr int kTetC2 = 3 | 2 << 3 | 6 << 6 | 4 << 9 | 5 << 12 | 1 << 15;   // 3 2 6 4 5 1
  const int c1 = (kTetC1 >> (3 * t)) & 7, c2 = (kTetC2 >> (3 * t)) & 7;
  return v == 0 ? 0 : (v == 3 ? 7 : (v == 1 ? c1 : c2));
}
#define EKF_TRI(a, b, c) ((a) | ((b) << 3) | ((c) << 6))
__device__ __forceinline__ unsigned tet_tris(int mask) {
  switch (mask) {
    case 1: return EKF_TRI(0, 1, 2);
    case 2: return EKF_TRI(0, 4, 3);
    case 3: return EKF_TRI(1, 2, 4) | (EKF_TRI(1, 4, 3) << 9);
    case 4: return EKF_TRI(1, 3, 5);
    case 5: return EKF_TRI(0, 5, 2) | (EKF_TRI(0, 3, 5) << 9);
    case 6: return EKF_TRI(0, 4, 5) | (EKF_TRI(0, 5, 1) << 9);
    case 7: return EKF_TRI(2, 4, 5);
    case 8: return EKF_TRI(2, 5, 4);
    case 9: return EKF_TRI(0, 1, 5) | (EKF_TRI(0, 5, 4) << 9);
    case 10: return EKF_TRI(0, 5, 3) | (EKF_TRI(0, 2, 5) << 9);
    case 11: return EKF_TRI(1, 5, 3);
    case 12: return EKF_TRI(1, 3, 4) | (EKF_TRI(1, 4, 2) << 9);
    case 13: return EKF_TRI(0, 3, 4);
    case 14: return EKF_TRI(0, 2, 1);
    default: return 0;
  }
}
#undef EKF_TRI
__device__ __forceinline__ int tet_ntri(int mask) {            // 0 inside or 4: none; 2 inside: a quad; otherwise one triangle
  const int b = (mask & 1) + ((mask >> 1) & 1) + ((mask >> 2) & 1) + ((mask >> 3) & 1);
  return (b == 0 || b == 4) ? 0 : (b == 2 ? 2 : 1);
}

struct ExtractArgs {
  const float* sum;
  const unsigned short* cnt;
  const unsigned* gsum;
  TsdfGrid g;
  int min_count;
  unsigned ncell;
  unsigned* blk_tot;                  // triangles per block of 256 cells (k_tsdf_count)
  const unsigned long long* blk_off;  // their exclusive scan (k_tsdf_emit)
  double* xyz;
  unsigned long long* key;
  unsigned char* grey;
};

// The cell of index cl = ci + (nx - 1) (cj + (ny - 1) ck) (the order of lin of its corner 0): -1 unless all eight corners are
// valid (cnt >= min_count), otherwise bit c = corner c is inside.  Inside is v = (double) sum / (double) cnt < 0, and with
// cnt >= 1 the quotient is negative exactly when the sum is (-0 and NaN are not): the test is made on the sum.
__device__ __forceinline__ int tsdf_cell(const ExtractArgs& a, unsigned cl, unsigned& lin0) {
  const unsigned cx = (unsigned)a.g.nx - 1, cy = (unsigned)a.g.ny - 1;
  const unsigned row = cl / cx, ci = cl - row * cx;
  const unsigned ck = row / cy, cj = row - ck * cy;
  lin0 = ci + (unsigned)a.g.nx * (cj + (unsigned)a.g.ny * ck);
  const unsigned sy = (unsigned)a.g.nx, sz = (unsigned)a.g.nx * (unsigned)a.g.ny;
  int in8 = 0;
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const unsigned l = lin0 + (c & 1) + ((c >> 1) & 1) * sy + (c >> 2) * sz;
    ok = ok && (int)a.cnt[l] >= a.min_count;
    in8 |= (a.sum[l] < 0.f ? 1 : 0) << c;
  }
  return ok ? in8 : -1;
}

__device__ __forceinline__ int tet_mask(int in8, int t) {
  return (in8 & 1) | (((in8 >> tet_corner(t, 1)) & 1) << 1) | (((in8 >> tet_corner(t, 2)) & 1) << 2) | (((in8 >> 7) & 1) << 3);
}

__device__ __forceinline__ int tsdf_cell_count(int in8) {
  if (in8 < 0) return 0;
  int n = 0;
#pragma unroll
  for (int t = 0; t < 6; ++t) n += tet_ntri(tet_mask(in8, t));
  return n;
}

// Pass 1: triangles per cell, reduced to one total per block of 256 cells (at most 256 x 12).
__global__ void __launch_bounds__(256) k_tsdf_count(ExtractArgs a) {
  __shared__ unsigned s_n[kFusionBlock];
  const unsigned tid = threadIdx.x, cl = blockIdx.x * (unsigned)kFusionBlock + tid;
  unsigned lin0;
  s_n[tid] = cl < a.ncell ? (unsigned)tsdf_cell_count(tsdf_cell(a, cl, lin0)) : 0u;
  __syncthreads();
  for (unsigned h = kFusionBlock / 2; h > 0; h >>= 1) {
    if (tid < h) s_n[tid] += s_n[tid + h];
    __syncthreads();
  }
  if (tid == 0) a.blk_tot[blockIdx.x] = s_n[0];
}

// Pass 2, one workgroup: off[b] = the sum of tot[0 .. b), off[nblk] = the grand total, in 64 bits.  Lane l owns the
// `chunk` consecutive blocks from l chunk on; the 256 chunk sums are scanned in LDS.
__global__ void __launch_bounds__(256) k_tsdf_scan(const unsigned* __restrict__ tot, unsigned long long* __restrict__ off,
                                                   unsigned nblk) {
  __shared__ unsigned long long s_c[kFusionBlock];
  const unsigned tid = threadIdx.x;
  const unsigned chunk = (nblk + kFusionBlock - 1) / kFusionBlock;
  const unsigned b0 = min(tid * chunk, nblk), b1 = min(b0 + chunk, nblk);
  unsigned long long mine = 0;
  for (unsigned b = b0; b < b1; ++b) mine += tot[b];
  s_c[tid] = mine;
  __syncthreads();
  unsigned long long run = 0;
  for (unsigned l = 0; l < tid; ++l) run += s_c[l];
  for (unsigned b = b0; b < b1; ++b) {
    off[b] = run;
    run += tot[b];
  }
  if (tid == kFusionBlock - 1) off[nblk] = run;              // (the last lane's run ends at the grand total, its chunk empty or not)
}

// One vertex on the edge of cube corners (ca, cb) of the cell at lin0: from the corner with the smaller lin to the larger
// (every Kuhn edge runs componentwise upwards, so that is the smaller corner number), whichever tetrahedron asks.
__device__ __forceinline__ void tsdf_vertex(const ExtractArgs& a, unsigned lin0, int c0, int c1, double* __restrict__ xyz,
                                            unsigned long long* __restrict__ key, unsigned char* __restrict__ grey) {
#pragma clang fp contract(off)
  const int ca = min(c0, c1), cb = max(c0, c1);
  const unsigned nx = (unsigned)a.g.nx, ny = (unsigned)a.g.ny;
  const unsigned row = lin0 / nx, i0 = lin0 - row * nx;
  const unsigned k0 = row / ny, j0 = row - k0 * ny;
  const unsigned ia[3] = {i0 + (ca & 1), j0 + ((ca >> 1) & 1), k0 + (ca >> 2)};
  const unsigned ib[3] = {i0 + (cb & 1), j0 + ((cb >> 1) & 1), k0 + (cb >> 2)};
  const unsigned la = ia[0] + nx * (ia[1] + ny * ia[2]), lb = ib[0] + nx * (ib[1] + ny * ib[2]);
  const double na = (double)a.cnt[la], nb = (double)a.cnt[lb];
  const double va = (double)a.sum[la] / na, vb = (double)a.sum[lb] / nb;
  const double ga = (double)a.gsum[la] / na, gb = (double)a.gsum[lb] / nb;
  const double u = va / (va - vb);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double Pa = a.g.origin[c] + (double)ia[c] * a.g.voxel;
    const double Pb = a.g.origin[c] + (double)ib[c] * a.g.voxel;
    xyz[c] = Pa + u * (Pb - Pa);
  }
  const double gv = ga + u * (gb - ga);
  *grey = (unsigned char)(int)floor(gv + 0.5);
  *key = (unsigned long long)la * 8ull + (unsigned long long)(cb - ca);
}

// Pass 3: recount, scan within the block, write at the block's offset.
__global__ void __launch_bounds__(256) k_tsdf_emit(ExtractArgs a) {
  __shared__ unsigned s_p[2][kFusionBlock];
  const unsigned tid = threadIdx.x, cl = blockIdx.x * (unsigned)kFusionBlock + tid;
  unsigned lin0 = 0;
  const int in8 = cl < a.ncell ? tsdf_cell(a, cl, lin0) : -1;
  const unsigned mine = (unsigned)tsdf_cell_count(in8);
  // inclusive Hillis-Steele scan over the 256 counts, ping-pong between the two rows
  int cur = 0;
  s_p[0][tid] = mine;
  __syncthreads();
  for (unsigned d = 1; d < (unsigned)kFusionBlock; d <<= 1) {
    s_p[cur ^ 1][tid] = s_p[cur][tid] + (tid >= d ? s_p[cur][tid - d] : 0u);
    cur ^= 1;
    __syncthreads();
  }
  if (mine == 0) return;
  unsigned long long o = a.blk_off[blockIdx.x] + (unsigned long long)(s_p[cur][tid] - mine);
  for (int t = 0; t < 6; ++t) {
    const int mask = tet_mask(in8, t);
    const int n = tet_ntri(mask);
    unsigned tris = tet_tris(mask);
    for (int j = 0; j < n; ++j, ++o, tris >>= 9) {
#pragma unroll
      for (int v = 0; v < 3; ++v) {
        const int e = (tris >> (3 * v)) & 7;
        // tet-local edge e = (lo, hi): lo = 0 0 0 1 1 2, hi = 1 2 3 2 3 3, two bits each
        constexpr int kEdgeLo = 1 << 6 | 1 << 8 | 2 << 10, kEdgeHi = 1 | 2 << 2 | 3 << 4 | 2 << 6 | 3 << 8 | 3 << 10;
        const int lo = (kEdgeLo >> (2 * e)) & 3, hi = (kEdgeHi >> (2 * e)) & 3;
        tsdf_vertex(a, lin0, tet_corner(t, lo), tet_corner(t, hi), a.xyz + (o * 3 + v) * 3, a.key + o * 3 + v, a.grey + o * 3 + v);
      }
    }
  }
}

struct ColourVertexArgs {
  const float* sum;
  const unsigned short* cnt;
  const unsigned* csum;               // three planes of nvox back to back
  const unsigned long long* key;      // the keys k_tsdf_emit wrote
  unsigned char* bgr;                 // three bytes a vertex
  unsigned long long nv;              // 3 n_tri
  size_t nvox;
  unsigned nx, ny;
};

// The colours of the vertices of a mesh (§18.1), after k_tsdf_emit and from its keys alone, one lane per vertex: key =
// 8 la + d, and since every Kuhn edge runs componentwise upwards the bits of d = cb - ca are the steps to the edge's other
// end.  na, nb, va, vb and u are tsdf_vertex's, operation for operation; a channel is blended and rounded as its grey is.  They
// are restated, not shared: a function for them reorders the instructions of k_tsdf_emit.
__global__ void __launch_bounds__(256) k_tsdf_colour_vertices(ColourVertexArgs a) {
#pragma clang fp contract(off)
  const unsigned long long v = (unsigned long long)blockIdx.x * (unsigned long long)kFusionBlock + threadIdx.x;
  if (v >= a.nv) return;
  const unsigned long long key = a.key[v];
  const unsigned la = (unsigned)(key >> 3), d = (unsigned)(key & 7ull);
  const unsigned lb = la + (d & 1u) + ((d >> 1) & 1u) * a.nx + (d >> 2) * (a.nx * a.ny);
  const double na = (double)a.cnt[la], nb = (double)a.cnt[lb];
  const double va = (double)a.sum[la] / na, vb = (double)a.sum[lb] / nb;
  const double u = va / (va - vb);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double Ca = (double)a.csum[c * a.nvox + la] / na, Cb = (double)a.csum[c * a.nvox + lb] / nb;
    const double cv = Ca + u * (Cb - Ca);
    a.bgr[v * 3 + c] = (unsigned char)(int)floor(cv + 0.5);
  }
}

#ifndef EKF_KERNELS_ONLY
// Host side of one handle (`ekf_fusion`).  Everything runs on the default stream of the handle's device, as ekf_dense_* does
// (§15.4 (2)): a map may come straight from the device buffers of a dense handle.
struct TsdfFusion {
  std::string err;
  int device = 0;
  TsdfGrid g{};
  double trunc = 0.0;
  bool created = false;
  DevBuf<float> sum;
  DevBuf<unsigned short> cnt;
  DevBuf<unsigned> gsum;
  bool colour = false;                // a colour volume (§18): csum exists, the colour kernels run
  DevBuf<unsigned> csum;              // the sums of B, G and R: three planes of nvox back to back
  DevBuf<float> d_depth;              // a host map on its way in
  DevBuf<unsigned char> d_img, d_bgr;
  DevBuf<unsigned> blk_tot;
  DevBuf<unsigned long long> blk_off;
  DevBuf<double> m_xyz;               // the mesh of the last extract (grow-only)
  DevBuf<unsigned long long> m_key;
  DevBuf<unsigned char> m_grey, m_bgr;          // m_bgr: three bytes a vertex, colour volumes only
  unsigned long long n_tri = 0;
  bool mesh_valid = false;            // an extract since the volume last changed
  int mesh_count = 0;                 // the min_count of that extract (ekf_mesh.hpp welds the soup it finds, if it is the one asked for)
  unsigned long long changes = 0;     // counts the changes of the volume (integrate, reset, ekf_fusion_set_volume): ekf_raycast.hpp
  int maps = 0;                       // maps integrated since the last reset (or what ekf_fusion_set_volume said)
  // k_tsdf_integrate, k_tsdf_count, k_tsdf_scan, k_tsdf_emit; 4, 5: ekf_raycast.hpp; 6, 7, 8: k_tsdf_integrate_colour,
  // k_tsdf_colour_vertices, k_tsdf_raycast_colour (§18)
  KernelTimer<9> timer;

  size_t nvox() const { return (size_t)g.nx * g.ny * g.nz; }
  unsigned ncell() const { return (unsigned)((size_t)(g.nx - 1) * (g.ny - 1) * (g.nz - 1)); }
  ~TsdfFusion() {                     // the members (events, buffers) go after this body, on the handle's device
    if (created) hipSetDevice(device);
  }

  hipError_t clear() {
    hipError_t e = hipMemsetAsync(sum, 0, nvox() * sizeof(float), nullptr);
    if (e == hipSuccess) e = hipMemsetAsync(cnt, 0, nvox() * sizeof(unsigned short), nullptr);
    if (e == hipSuccess) e = hipMemsetAsync(gsum, 0, nvox() * sizeof(unsigned), nullptr);
    if (e == hipSuccess && colour) e = hipMemsetAsync(csum, 0, 3 * nvox() * sizeof(unsigned), nullptr);
    mesh_valid = false;
    ++changes;
    if (e == hipSuccess) maps = 0;
    return e;
  }

  // One launch of k_tsdf_integrate over device buffers of W x H (tight rows); of k_tsdf_integrate_colour for a colour volume,
  // where bgr (W x H x 3, tight) may be NULL (a map without colour) and img is read only then.
  hipError_t integrate(const float* depth, const unsigned char* img, int W, int H, const double K[4], const double R[9],
                       const double t[3], const unsigned char* bgr = nullptr) {
    IntegrateArgs a{};
    a.sum = sum; a.cnt = cnt; a.gsum = gsum;
    a.depth = depth; a.img = img; a.W = W; a.H = H;
    a.g = g; a.trunc = trunc;
    a.fx = K[0]; a.fy = K[1]; a.cx = K[2]; a.cy = K[3];
    for (int i = 0; i < 9; ++i) a.R[i] = R[i];
    for (int i = 0; i < 3; ++i) a.t[i] = t[i];
    mesh_valid = false;
    ++changes;
    const unsigned nblk = (unsigned)((nvox() + kFusionBlock - 1) / kFusionBlock);
    hipError_t e;
    if (colour) {
      const IntegrateColourArgs c{a, bgr, csum, nvox()};
      e = timer.run(6, [&] { k_tsdf_integrate_colour<<<nblk, kFusionBlock, 0, nullptr>>>(c); });
    } else {
      e = timer.run(0, [&] { k_tsdf_integrate<<<nblk, kFusionBlock, 0, nullptr>>>(a); });
    }
    if (e != hipSuccess) return e;
    ++maps;
    return hipSuccess;
  }

  // count -> scan -> one 8-byte read-back -> (grow the mesh buffers) -> emit (-> the vertex colours of a colour volume).  A
  // failed allocation leaves the previous mesh (the new buffers replace the old ones only when all of them exist) and the
  // volume as they were.
  hipError_t extract(int min_count) {
    const unsigned nc = ncell(), nblk = (nc + kFusionBlock - 1) / kFusionBlock;
    hipError_t e;
    if ((e = blk_tot.reserve(nblk)) != hipSuccess || (e = blk_off.reserve((size_t)nblk + 1)) != hipSuccess) return e;
    ExtractArgs a{};
    a.sum = sum; a.cnt = cnt; a.gsum = gsum; a.g = g; a.min_count = min_count; a.ncell = nc;
    a.blk_tot = blk_tot; a.blk_off = blk_off;
    if ((e = timer.run(1, [&] { k_tsdf_count<<<nblk, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
    if ((e = timer.run(2, [&] { k_tsdf_scan<<<1, kFusionBlock, 0, nullptr>>>(blk_tot, blk_off, nblk); })) != hipSuccess) return e;
    unsigned long long total = 0;
    if ((e = hipMemcpy(&total, blk_off + nblk, sizeof(total), hipMemcpyDeviceToHost)) != hipSuccess) return e;
    const size_t nv = (size_t)total * 3;
    if (nv > m_key.capacity() || nv > m_grey.capacity() || nv * 3 > m_xyz.capacity() || (colour && nv * 3 > m_bgr.capacity())) {
      DevBuf<double> x;
      DevBuf<unsigned long long> k;
      DevBuf<unsigned char> gr, co;
      if ((e = x.reserve(nv * 3)) != hipSuccess || (e = k.reserve(nv)) != hipSuccess || (e = gr.reserve(nv)) != hipSuccess ||
          (colour && (e = co.reserve(nv * 3)) != hipSuccess)) {
        (void)hipGetLastError();
        return e;
      }
      m_xyz = std::move(x);
      m_key = std::move(k);
      m_grey = std::move(gr);
      m_bgr = std::move(co);
    }
    mesh_valid = false;
    if (total > 0) {
      a.xyz = m_xyz; a.key = m_key; a.grey = m_grey;
      if ((e = timer.run(3, [&] { k_tsdf_emit<<<nblk, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
      if (colour) {
        const ColourVertexArgs c{sum, cnt, csum, m_key, m_bgr, (unsigned long long)nv, nvox(), (unsigned)g.nx, (unsigned)g.ny};
        const unsigned vblk = (unsigned)((nv + kFusionBlock - 1) / kFusionBlock);
        if ((e = timer.run(7, [&] { k_tsdf_colour_vertices<<<vblk, kFusionBlock, 0, nullptr>>>(c); })) != hipSuccess) return e;
      }
    }
    n_tri = total;
    mesh_count = min_count;
    mesh_valid = true;
    return hipSuccess;
  }
};
#endif  // EKF_KERNELS_ONLY

}  // namespace ekf
