// The indexed mesh of a TSDF volume, welded on the device, and its vertex normals.  k_tsdf_emit of
// ekf_fusion.hpp writes a triangle soup whose vertex keys are 8 la + d: la the lin of the smaller end of a Kuhn edge, d in 1..7
// the bits of the steps to its other end.  The welded vertex list is the list of the edges that carry a vertex in (la, d)
// order: an exclusive scan over a 7-bit mask per voxel, with the machinery the extraction has.  No sort, no atomics, no
// communication between workgroups.  The reference has no counterpart; the contract is pinned here and restated in numpy by
// tests/mesh_oracle.py:
//   - edge (la, d) carries a vertex iff inside(la) != inside(lb) (inside: sum < 0, as tsdf_cell has it) and one of the cells
//     that contain it (corner 0 at la - o, o a subset of ~d & 7) lies in the grid with all eight cnt >= min_count;
//   - xyz, grey and bgr are tsdf_vertex's and k_tsdf_colour_vertices's arithmetic, operation for operation, from the key
//     alone (restated, not shared: DESIGN.md §18.4 (5));
//   - faces[3 t + v] is the rank of the soup's key (t, v) among the vertices;
//   - normals are the blend along the edge of the central differences of the mean field at its two ends, one-sided where a
//     neighbour is outside the grid or has cnt < min_count, fp64 throughout, contraction off, normalised as k_tsdf_raycast
//     normalises and rounded once to fp32.
// Nothing here touches a filter, counts as a launch kind or runs a collective.
#pragma once
#include <cmath>
#include <cstddef>

// EKF_KERNELS_ONLY: the structs and the kernel bodies alone, for tools/mesh_host_check.cpp, which runs the kernels lane by
// lane on the host; tools/host_kernels.hpp supplies threadIdx, __syncthreads and the like.
#include "ekf_fusion.hpp"
#include "ekf_mesh_stamp.hpp"

namespace ekf {

constexpr int kMeshKinds = 5;                    // k_mesh_cells, k_mesh_edges, k_tsdf_scan, k_mesh_vertices, k_mesh_faces

struct MeshArgs {
  const float* sum;
  const unsigned short* cnt;
  const unsigned* gsum;
  const unsigned* csum;               // three planes of nvox back to back; NULL = a plain volume
  TsdfGrid g;
  int min_count;
  unsigned nvox, ncell;
  unsigned char* cell_ok;             // one byte a cell, in the extraction's cell order: all eight corners are valid
  unsigned* code;                     // one word a voxel: (edges before it in its block of 256) << 8 | the 7-bit mask of its edges
  unsigned* blk_tot;                  // vertices per block of 256 voxels (k_mesh_edges)
  const unsigned long long* blk_off;  // their exclusive scan (k_tsdf_scan)
  double* xyz;                        // the vertices, by ascending key
  unsigned long long* key;
  unsigned char* grey;
  unsigned char* bgr;                 // three bytes a vertex, colour volumes only
  float* normal;                      // three floats a vertex, k_mesh_vertices<true> only
  const unsigned long long* soup_key; // the keys k_tsdf_emit wrote
  unsigned* faces;
  unsigned long long ncorner;         // 3 n_tri
};

// One lane per cell, in k_tsdf_count's cell order: eight cnt loads, one byte.
__global__ void __launch_bounds__(256) k_mesh_cells(MeshArgs a) {
  const unsigned cl = blockIdx.x * (unsigned)kFusionBlock + threadIdx.x;
  if (cl >= a.ncell) return;
  const unsigned cx = (unsigned)a.g.nx - 1, cy = (unsigned)a.g.ny - 1;
  const unsigned row = cl / cx, ci = cl - row * cx;
  const unsigned ck = row / cy, cj = row - ck * cy;
  const unsigned lin0 = ci + (unsigned)a.g.nx * (cj + (unsigned)a.g.ny * ck);
  const unsigned sy = (unsigned)a.g.nx, sz = (unsigned)a.g.nx * (unsigned)a.g.ny;
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 8; ++c) ok = ok && (int)a.cnt[lin0 + (c & 1) + ((c >> 1) & 1) * sy + (c >> 2) * sz] >= a.min_count;
  a.cell_ok[cl] = ok ? 1 : 0;
}

// One lane per voxel, x along the lanes.  Bit o of `cells`: the cell whose corner o this voxel is lies in the grid and is
// valid; bit c of `in8`: the voxel c steps away is inside (bit c of `have`: it is in the grid).  Edge d carries a vertex iff
// the signs at its ends differ and one of the cells o, o a subset of ~d & 7, is valid.  Then the Hillis-Steele scan of
// k_tsdf_emit over the 256 popcounts.
__global__ void __launch_bounds__(256) k_mesh_edges(MeshArgs a) {
  __shared__ unsigned s_p[2][kFusionBlock];
  const unsigned tid = threadIdx.x, lin = blockIdx.x * (unsigned)kFusionBlock + tid;
  unsigned mask = 0;
  if (lin < a.nvox) {
    const unsigned nx = (unsigned)a.g.nx, ny = (unsigned)a.g.ny, nz = (unsigned)a.g.nz;
    const unsigned row = lin / nx, i = lin - row * nx;
    const unsigned k = row / ny, j = row - k * ny;
    const unsigned cx = nx - 1, cy = ny - 1;
    unsigned cells = 0, in8 = 0, have = 0;
#pragma unroll
    for (int o = 0; o < 8; ++o) {
      const unsigned ox = o & 1, oy = (o >> 1) & 1, oz = o >> 2;
      // the cell at (i - ox, j - oy, k - oz): each coordinate in 0 .. n - 2
      if (i >= ox && i - ox < cx && j >= oy && j - oy < cy && k >= oz && k - oz < nz - 1) {
        const unsigned cl = (i - ox) + cx * ((j - oy) + cy * (k - oz));
        cells |= (unsigned)a.cell_ok[cl] << o;
      }
      if (i + ox < nx && j + oy < ny && k + oz < nz) {
        have |= 1u << o;
        in8 |= (a.sum[lin + ox + oy * nx + oz * (nx * ny)] < 0.f ? 1u : 0u) << o;
      }
    }
#pragma unroll
    for (int d = 1; d < 8; ++d) {
      const int f = ~d & 7;             // the offsets o whose bits are a subset of f: 0, and f's one, two or three submasks
      unsigned any = 0;
#pragma unroll
      for (int o = 0; o < 8; ++o)
        if ((o & ~f) == 0) any |= (cells >> o) & 1u;
      const unsigned cross = ((in8 >> d) ^ in8) & 1u;
      mask |= (((have >> d) & 1u) & cross & any) << d;
    }
  }
  const unsigned mine = (unsigned)__builtin_popcount(mask);
  int cur = 0;
  s_p[0][tid] = mine;
  __syncthreads();
  for (unsigned d = 1; d < (unsigned)kFusionBlock; d <<= 1) {
    s_p[cur ^ 1][tid] = s_p[cur][tid] + (tid >= d ? s_p[cur][tid - d] : 0u);
    cur ^= 1;
    __syncthreads();
  }
  if (lin < a.nvox) a.code[lin] = ((s_p[cur][tid] - mine) << 8) | mask;
  if (tid == kFusionBlock - 1) a.blk_tot[blockIdx.x] = s_p[cur][tid];
}

// Whether l counts for the gradient (cnt >= min_count), and then v(l) = (double) sum / (double) cnt.
__device__ __forceinline__ bool mesh_mean(const MeshArgs& a, unsigned l, double& v) {
#pragma clang fp contract(off)
  const unsigned short c = a.cnt[l];
  if ((int)c < a.min_count) return false;
  v = (double)a.sum[l] / (double)c;
  return true;
}

// Component c of the gradient of the mean field at voxel l = (idx[0], idx[1], idx[2]), in voxel units: the central difference
// where both neighbours on the axis are usable (inside the grid, cnt >= min_count), a one-sided one where one is, else 0.
__device__ __forceinline__ double mesh_gradient(const MeshArgs& a, unsigned l, const unsigned idx[3], int c, double vl) {
#pragma clang fp contract(off)
  const unsigned n = c == 0 ? (unsigned)a.g.nx : (c == 1 ? (unsigned)a.g.ny : (unsigned)a.g.nz);
  const unsigned stride = c == 0 ? 1u : (c == 1 ? (unsigned)a.g.nx : (unsigned)a.g.nx * (unsigned)a.g.ny);
  double vp = 0.0, vm = 0.0;
  const bool up = idx[c] + 1 < n && mesh_mean(a, l + stride, vp);
  const bool dn = idx[c] >= 1 && mesh_mean(a, l - stride, vm);
  if (up && dn) return (vp - vm) * 0.5;
  if (up) return vp - vl;
  if (dn) return vl - vm;
  return 0.0;
}

// One lane per voxel; the lanes whose mask is not 0 write their vertices at blk_off[block] + prefix + rank, d ascending.
// na, nb, va, vb, u, the blends and the rounding are tsdf_vertex's and k_tsdf_colour_vertices's, operation for operation.
template <bool NORMALS>
__global__ void __launch_bounds__(256) k_mesh_vertices(MeshArgs a) {
#pragma clang fp contract(off)
  const unsigned la = blockIdx.x * (unsigned)kFusionBlock + threadIdx.x;
  if (la >= a.nvox) return;
  const unsigned code = a.code[la], mask = code & 0xffu;
  if (mask == 0) return;
  unsigned long long o = a.blk_off[blockIdx.x] + (unsigned long long)(code >> 8);
  const unsigned nx = (unsigned)a.g.nx, ny = (unsigned)a.g.ny;
  const unsigned row = la / nx, i0 = la - row * nx;
  const unsigned k0 = row / ny, j0 = row - k0 * ny;
  const unsigned ia[3] = {i0, j0, k0};
  const double na = (double)a.cnt[la];
  const double va = (double)a.sum[la] / na;
  const double ga = (double)a.gsum[la] / na;
  double grad_a[3] = {0.0, 0.0, 0.0};
  if (NORMALS) {
#pragma unroll
    for (int c = 0; c < 3; ++c) grad_a[c] = mesh_gradient(a, la, ia, c, va);
  }
  for (unsigned d = 1; d < 8; ++d) {
    if (!((mask >> d) & 1u)) continue;
    const unsigned ib[3] = {i0 + (d & 1u), j0 + ((d >> 1) & 1u), k0 + (d >> 2)};
    const unsigned lb = ib[0] + nx * (ib[1] + ny * ib[2]);
    const double nb = (double)a.cnt[lb];
    const double vb = (double)a.sum[lb] / nb;
    const double gb = (double)a.gsum[lb] / nb;
    const double u = va / (va - vb);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double Pa = a.g.origin[c] + (double)ia[c] * a.g.voxel;
      const double Pb = a.g.origin[c] + (double)ib[c] * a.g.voxel;
      a.xyz[o * 3 + c] = Pa + u * (Pb - Pa);
    }
    const double gv = ga + u * (gb - ga);
    a.grey[o] = (unsigned char)(int)floor(gv + 0.5);
    a.key[o] = (unsigned long long)la * 8ull + (unsigned long long)d;
    if (a.csum) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double Ca = (double)a.csum[c * (size_t)a.nvox + la] / na, Cb = (double)a.csum[c * (size_t)a.nvox + lb] / nb;
        const double cv = Ca + u * (Cb - Ca);
        a.bgr[o * 3 + c] = (unsigned char)(int)floor(cv + 0.5);
      }
    }
    if (NORMALS) {
      double n[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double gbc = mesh_gradient(a, lb, ib, c, vb);
        n[c] = grad_a[c] + u * (gbc - grad_a[c]);
      }
      const double len = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
      const bool ok = len > 0.0 && len < INFINITY;            // (a NaN fails)
#pragma unroll
      for (int c = 0; c < 3; ++c) a.normal[o * 3 + c] = ok ? (float)(n[c] / len) : 0.f;
    }
    ++o;
  }
}

// One lane per corner of the soup: the rank of its key among the vertices.  Bit 0 of a mask is never set, so the edges of la
// before d are the bits below d.
__global__ void __launch_bounds__(256) k_mesh_faces(MeshArgs a) {
  const unsigned long long v = (unsigned long long)blockIdx.x * (unsigned long long)kFusionBlock + threadIdx.x;
  if (v >= a.ncorner) return;
  const unsigned long long key = a.soup_key[v];
  const unsigned la = (unsigned)(key >> 3), d = (unsigned)(key & 7ull);
  const unsigned code = a.code[la];
  a.faces[v] = (unsigned)(a.blk_off[la >> 8] + (unsigned long long)((code >> 8) + (unsigned)__builtin_popcount(code & ((1u << d) - 1u))));
}

#ifndef EKF_KERNELS_ONLY
// An indexed mesh on the device as whoever reads it sees it: the six arrays, the counts, and `id`, the stamp that names the mesh
// (ekf_mesh_stamp.hpp; 0 for a mesh the caller gave).  A view owns nothing and holds as long as its mesh does.
struct MeshView {
  const double* xyz = nullptr;
  const unsigned long long* key = nullptr;
  const unsigned char* grey = nullptr;
  const unsigned char* bgr = nullptr;            // of a colour volume only; NULL: the mesh has no B, G, R
  const float* normal = nullptr;                 // to be read with has_normals only
  const unsigned* faces = nullptr;
  unsigned long long n_vert = 0, n_tri = 0;
  bool has_normals = false;
  unsigned long long id = 0;

  static MeshView of(const DevMeshBufs& b, unsigned long long id) {
    MeshView v;
    v.xyz = b.xyz; v.key = b.key; v.grey = b.grey; v.bgr = b.bgr; v.normal = b.normal; v.faces = b.faces;
    v.n_vert = b.n_vert; v.n_tri = b.n_tri; v.has_normals = b.has_normals;
    v.id = id;
    return v;
  }
};

// A mesh the caller gave: source 4 of the rasteriser and of the distance, each with one of its own.  grey and bgr are optional.
struct CallerMesh {
  DevBuf<double> xyz;
  DevBuf<unsigned> faces;
  DevBuf<unsigned char> grey, bgr;
  unsigned long long n_vert = 0, n_tri = 0;
  bool set = false, colour = false;

  // New rows beside the old ones, which they replace only when all of them exist.
  hipError_t upload(const double* x, const unsigned* f, const unsigned char* g, const unsigned char* c, size_t nv, size_t nt) {
    hipError_t e;
    DevBuf<double> nx;
    DevBuf<unsigned> nf;
    DevBuf<unsigned char> ng, nc;
    if ((e = nx.reserve(std::max(nv * 3, xyz.capacity()))) != hipSuccess || (e = nf.reserve(std::max(nt * 3, faces.capacity()))) != hipSuccess ||
        (g && (e = ng.reserve(std::max(nv, grey.capacity()))) != hipSuccess) || (c && (e = nc.reserve(std::max(nv * 3, bgr.capacity()))) != hipSuccess)) {
      (void)hipGetLastError();
      return e;
    }
    if ((e = hipMemcpy(nx, x, nv * 3 * sizeof(double), hipMemcpyHostToDevice)) != hipSuccess) return e;
    if ((e = hipMemcpy(nf, f, nt * 3 * sizeof(unsigned), hipMemcpyHostToDevice)) != hipSuccess) return e;
    if (g && (e = hipMemcpy(ng, g, nv, hipMemcpyHostToDevice)) != hipSuccess) return e;
    if (c && (e = hipMemcpy(nc, c, nv * 3, hipMemcpyHostToDevice)) != hipSuccess) return e;
    xyz = std::move(nx); faces = std::move(nf);
    if (g) grey = std::move(ng);
    if (c) bgr = std::move(nc);
    n_vert = nv; n_tri = nt; colour = c != nullptr; set = true;
    return hipSuccess;
  }

  MeshView view() const {
    MeshView v;
    v.xyz = xyz; v.faces = faces; v.grey = grey; v.bgr = colour ? (const unsigned char*)bgr : nullptr;
    v.n_vert = n_vert; v.n_tri = n_tri;
    return v;
  }
};

// Host side: the scratch and the indexed mesh of the last weld, owned by the fusion handle they belong to; allocated at the
// first weld, grow-only.  The scratch is 4 bytes a voxel and 1 byte a cell (1.25 GB at 2^28 voxels).  The five launches are
// kinds of a timer of their own, so that the fusion handle's counts stay what they are without a weld.
struct TsdfMesh {
  DevBuf<unsigned char> cell_ok;
  DevBuf<unsigned> code, blk_tot;
  DevBuf<unsigned long long> blk_off;
  DevMeshBufs out;                               // the welded mesh; bgr: colour volumes only, normal: welds with normals only
  KernelTimer<kMeshKinds> timer;

  // (extract, unless the handle holds the soup of this min_count) -> cells -> edges -> scan -> one 8-byte read-back -> (grow
  // the mesh buffers) -> vertices -> faces.  A failed allocation leaves the soup and the volume as they were; the previous
  // weld is lost only when its scratch had to grow.
  hipError_t weld(MeshStamps& st, TsdfFusion& f, int min_count, bool normals) {
    hipError_t e;
    if ((e = timer.create()) != hipSuccess) return e;
    if (!f.mesh_valid || f.mesh_count != min_count) {
      if ((e = f.extract(min_count)) != hipSuccess) return e;
    }
    const unsigned nvox = (unsigned)f.nvox(), nc = f.ncell();
    const unsigned vblk = fusion_blocks(nvox), cblk = fusion_blocks(nc);
    st.begin(st.weld);
    if ((e = cell_ok.reserve(nc)) != hipSuccess || (e = code.reserve(nvox)) != hipSuccess || (e = blk_tot.reserve(vblk)) != hipSuccess ||
        (e = blk_off.reserve((size_t)vblk + 1)) != hipSuccess) {
      (void)hipGetLastError();
      return e;
    }
    MeshArgs a{};
    a.sum = f.sum; a.cnt = f.cnt; a.gsum = f.gsum; a.csum = f.colour ? (const unsigned*)f.csum : nullptr;
    a.g = f.g; a.min_count = min_count; a.nvox = nvox; a.ncell = nc;
    a.cell_ok = cell_ok; a.code = code; a.blk_tot = blk_tot; a.blk_off = blk_off;
    if ((e = timer.run(0, [&] { k_mesh_cells<<<cblk, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
    if ((e = timer.run(1, [&] { k_mesh_edges<<<vblk, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
    if ((e = timer.run(2, [&] { k_tsdf_scan<<<1, kFusionBlock, 0, nullptr>>>(blk_tot, blk_off, vblk); })) != hipSuccess) return e;
    unsigned long long total = 0;
    if ((e = hipMemcpy(&total, blk_off + vblk, sizeof(total), hipMemcpyDeviceToHost)) != hipSuccess) return e;
    const size_t nv = (size_t)total, ncorner = (size_t)f.n_tri * 3;
    if ((e = out.grow(nv, ncorner, f.colour, normals)) != hipSuccess) {
      (void)hipGetLastError();
      return e;
    }
    a.xyz = out.xyz; a.key = out.key; a.grey = out.grey; a.bgr = out.bgr; a.normal = out.normal;
    a.soup_key = f.m_key; a.faces = out.faces; a.ncorner = (unsigned long long)ncorner;
    if (nv > 0) {
      if (normals)
        e = timer.run(3, [&] { k_mesh_vertices<true><<<vblk, kFusionBlock, 0, nullptr>>>(a); });
      else
        e = timer.run(3, [&] { k_mesh_vertices<false><<<vblk, kFusionBlock, 0, nullptr>>>(a); });
      if (e != hipSuccess) return e;
    }
    if (ncorner > 0 && (e = timer.run(4, [&] { k_mesh_faces<<<fusion_blocks(ncorner), kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess)
      return e;
    out.n_vert = total;
    out.n_tri = f.n_tri;
    out.has_normals = normals;
    st.weld_changes = f.changes;
    st.weld.valid = true;
    return hipSuccess;
  }
};
#endif  // EKF_KERNELS_ONLY

}  // namespace ekf
