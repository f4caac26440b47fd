// The connected components of the welded mesh and the removal of the small ones, on the device.  The weld of
// ekf_mesh.hpp is an indexed mesh whose vertex order is a function of the volume alone; what is left of a wrong surface in it
// are floating fragments of a few triangles.  The reference has no counterpart; the contract is pinned here and restated in
// numpy by tests/component_oracle.py:
//   1. two vertices of the weld are linked iff some triangle of `faces` has both; a component is a connected component of the
//      links.  Linking is by index, not by coordinate: two vertices with different keys but equal coordinates (u exactly 0, the
//      surface through a voxel) are distinct and may lie in different components.  Every welded vertex lies in at least one
//      triangle (§24.1), so no vertex is without a component;
//   2. label[v] is the least vertex index of v's component, size[v] the number of triangles of that component (a triangle's
//      three vertices share a component), n_comp the number of distinct labels.  All are functions of `faces` alone, so the
//      integer atomics below, whose order of arrival differs from run to run, cost no bit of the result;
//   3. prune(min_triangles >= 1, largest in {0, 1}): a component is kept iff size >= min_triangles and, with `largest`, it is
//      the component of greatest size, the least label among equals.  The pruned mesh is the weld without the vertices and
//      triangles of the other components, order preserved: xyz, key, grey, bgr and normal are the kept rows bit for bit
//      (normal iff the weld had normals), faces the kept triangles in the soup's order, re-indexed by the rank of each vertex
//      among the kept ones.  So min_triangles = 1, largest = 0 is the identity, keys stay ascending, pruning is idempotent, and
//      a min_triangles above every size gives the empty mesh.
//
// The launches, 256 lanes a workgroup, on the default stream; vblk = ceil(n_vert / 256), tblk = ceil(n_tri / 256).  None is
// made when the weld has no triangle.
//   components:  k_comp_init      vblk          L[v] = v, S[v] = 0, and the two single words (the best key, the root count)
//                k_comp_union     tblk          union(f0, f1), union(f0, f2) in L, between workgroups (argument at the kernel)
//                k_comp_count     vblk + tblk   R[v] = root(v) and the number of roots; S[root(f0)] += 1, runs of equal roots
//                                               among a workgroup's 256 triangles as one add
//                k_comp_flags     vblk + tblk   (as below, keeping everything: for the sizes; not when a prune asked)
//                one 4-byte read-back (n_comp)
//   prune:       k_comp_largest   vblk          only with `largest`: the maximum of (size << 32) | (0xFFFFFFFF - label)
//                k_comp_flags     vblk + tblk   L[v] = size, the keep flags of vertices and triangles with their in-block
//                                               exclusive scans, the block totals (vertices, triangles, kept roots)
//                k_tsdf_scan      1, 3 times    ekf_fusion.hpp's, unchanged: vertex blocks, triangle blocks, kept roots
//                one read-back of the three totals
//                k_comp_vertices  vblk          not for an empty result
//                k_comp_faces     tblk          likewise
// Scratch: 16 bytes a vertex (L, R, S and V: the flag word, then the new index), 4 bytes a triangle (T), and per block of 256
// 8 bytes (two totals) a vertex block, 4 a triangle block and 24 (three rows of offsets) the larger of the two; 12 bytes of
// single words.  The pruned mesh has buffers of its own of exactly the weld's row sizes.
#pragma once
#include "ekf_mesh.hpp"
#include "ekf_union_find.hpp"

namespace ekf {

// k_comp_init, k_comp_union, k_comp_count, k_comp_largest, k_comp_flags, k_tsdf_scan, k_comp_vertices, k_comp_faces
constexpr int kCompKinds = 8;
constexpr unsigned kCompNone = 0xffffffffu;      // no root (a lane past the last triangle); the new index of a dropped vertex

// The one 64-bit atomic: the best key of k_comp_largest.  The host check defines it beside the six of ekf_union_find.hpp.
#ifndef EKF_SPECKLE_HOST_ATOMICS
__device__ __forceinline__ void comp_global_max(unsigned long long* p, unsigned long long v) {
  __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
#endif

struct CompArgs {
  const unsigned* faces;              // the weld's: three vertex indices a triangle
  unsigned* L;                        // n_vert words each: the forest, then a vertex's size
  unsigned* R;                        //   a vertex's root: its label
  unsigned* S;                        //   at a root: the triangles of its component
  unsigned* V;                        //   (in-block exclusive prefix << 1) | keep, then the vertex's new index (kCompNone: dropped)
  unsigned* T;                        // n_tri words: (in-block exclusive prefix << 1) | keep
  unsigned* blk_tot;                  // vblk kept vertices, tblk kept triangles, vblk kept roots
  const unsigned long long* off_v;    // their exclusive scans (k_tsdf_scan)
  const unsigned long long* off_t;
  unsigned long long* best;           // one word: the greatest (size << 32) | (0xFFFFFFFF - label) over the roots
  unsigned* n_roots;                  // one word: the number of roots
  unsigned n_vert, vblk;
  unsigned long long n_tri;
  unsigned min_triangles;
  int largest;
  const double* xyz;                  // the weld's rows
  const unsigned long long* key;
  const unsigned char* grey;
  const unsigned char* bgr;           // NULL = a plain volume
  const float* normal;                // NULL = a weld without normals
  double* p_xyz;                      // the pruned mesh's
  unsigned long long* p_key;
  unsigned char* p_grey;
  unsigned char* p_bgr;
  float* p_normal;
  unsigned* p_faces;
};

// One lane a vertex: every vertex a root, no triangle counted; lane 0 of workgroup 0 clears the two single words.
__global__ void __launch_bounds__(256) k_comp_init(CompArgs a) {
  const unsigned v = blockIdx.x * (unsigned)kFusionBlock + threadIdx.x;
  if (v == 0) {
    *a.best = 0ull;
    *a.n_roots = 0u;
  }
  if (v >= a.n_vert) return;
  a.L[v] = v;
  a.S[v] = 0u;
}

// One lane a triangle (a 64-bit lane index, as k_mesh_faces has): its first vertex united with its second and its third.
//
// Visibility.  This is the one launch of the family in which workgroups communicate through data while they run.  The XCDs'
// L2s are not coherent with each other and a CU's L1 is never refreshed by another CU's stores, so EVERY access to L in this
// kernel, the loads of seg_find included, is a relaxed atomic of agent scope (SegGlobal); there is no plain load or store of
// L.  What L holds at the start comes from k_comp_init and is visible by the kernel boundary.  Relaxed suffices: the algorithm
// uses the modification order of each single word (a word only ever decreases) and the value fetch_min returns, the one
// proof that a hook took place; it never infers from one word what another word holds.  A load that returns an older, larger
// value of a word only lengthens a walk: the value is still an ancestor.  `faces` is read-only for the whole call and takes
// plain loads.
// Termination.  Every loop of seg_find and seg_union walks strictly decreasing indices >= 0 (ekf_union_find.hpp), so it ends
// after at most n_vert steps whatever other lanes or workgroups do meanwhile.  No lane waits for another: no flag, no spin,
// no ordered hand-over; a lane whose fetch_min lost against another's goes on with the smaller value it was given.
__global__ void __launch_bounds__(256) k_comp_union(CompArgs a) {
  const unsigned long long t = (unsigned long long)blockIdx.x * (unsigned long long)kFusionBlock + threadIdx.x;
  if (t >= a.n_tri) return;
  const unsigned f0 = a.faces[t * 3], f1 = a.faces[t * 3 + 1], f2 = a.faces[t * 3 + 2];
  seg_union<SegGlobal>(a.L, f0, f1);
  seg_union<SegGlobal>(a.L, f0, f2);
}

// The in-block inclusive scan of one number a lane (Hillis-Steele, the rows of k_mesh_edges); every lane of the workgroup
// calls it, once a kernel.  `total` is the sum over the workgroup.
__device__ __forceinline__ unsigned comp_scan(unsigned (*s_p)[kFusionBlock], unsigned tid, unsigned mine, unsigned& total) {
  int cur = 0;
  s_p[0][tid] = mine;
  __syncthreads();
  for (unsigned d = 1; d < (unsigned)kFusionBlock; d <<= 1) {
    s_p[cur ^ 1][tid] = s_p[cur][tid] + (tid >= d ? s_p[cur][tid - d] : 0u);
    cur ^= 1;
    __syncthreads();
  }
  total = s_p[cur][kFusionBlock - 1];
  return s_p[cur][tid];
}

// Behind the kernel boundary L is final and takes plain loads; no word of it is written (R is another buffer).  Workgroups
// 0 .. vblk - 1, one lane a vertex: R[v] = the root of v, and the workgroup's roots, counted in an LDS word, go to n_roots in
// one add.  The other workgroups, one lane a triangle: the root of its first vertex gains 1.  Before anything goes to memory
// (cdna_hip_programming.md, Guideline 12) a run of equal roots among the workgroup's 256 triangles becomes one add: the lanes
// that start a run are numbered by a scan, each leaves its lane number at its rank, and the run's length is the distance to
// the next one.  A workgroup inside one large component so adds to that component's word once, not 256 times.  Unsigned sums
// are exact in any order.
__global__ void __launch_bounds__(256) k_comp_count(CompArgs a) {
  __shared__ unsigned s_key[kFusionBlock];      // a triangle's root; kCompNone past the last triangle
  __shared__ unsigned s_p[2][kFusionBlock];
  __shared__ unsigned s_pos[kFusionBlock];      // the lane at which run r begins; [0]: the root counter of a vertex workgroup
  const unsigned tid = threadIdx.x;
  if (blockIdx.x < a.vblk) {                    // (the same for every lane of the workgroup)
    const unsigned v = blockIdx.x * (unsigned)kFusionBlock + tid;
    if (tid == 0) s_pos[0] = 0u;
    __syncthreads();
    if (v < a.n_vert) {
      unsigned r = v;
      for (unsigned p = a.L[r]; p != r; p = a.L[r]) r = p;                   // strictly decreasing
      a.R[v] = r;
      if (r == v) seg_lds_add(&s_pos[0], 1u);
    }
    __syncthreads();
    if (tid == 0 && s_pos[0] != 0u) seg_global_add(a.n_roots, s_pos[0]);
    return;
  }
  const unsigned long long base = (unsigned long long)(blockIdx.x - a.vblk) * (unsigned long long)kFusionBlock, t = base + tid;
  unsigned key = kCompNone;
  if (t < a.n_tri) {
    unsigned r = a.faces[t * 3];
    for (unsigned p = a.L[r]; p != r; p = a.L[r]) r = p;
    key = r;
  }
  s_key[tid] = key;
  __syncthreads();
  const bool start = key != kCompNone && (tid == 0 || s_key[tid - 1] != key);
  unsigned nruns;
  const unsigned rank = comp_scan(s_p, tid, start ? 1u : 0u, nruns);         // at a start: the number of its run + 1
  if (start) s_pos[rank - 1] = tid;
  __syncthreads();
  if (tid < nruns) {
    const unsigned long long left = a.n_tri - base;                          // the lanes past the last triangle start no run
    const unsigned valid = left < (unsigned long long)kFusionBlock ? (unsigned)left : (unsigned)kFusionBlock;
    const unsigned p = s_pos[tid], end = tid + 1 < nruns ? s_pos[tid + 1] : valid;
    seg_global_add(&a.S[s_key[p]], end - p);                                 // s_key[p]: a root, an index below n_vert
  }
}

// Only with `largest`, one lane a vertex: the greatest (size << 32) | (0xFFFFFFFF - label) over the roots, so the greatest
// size and among equals the least label; reduced in LDS to one fetch_max a workgroup.  A root has at least one triangle, so
// its key is not 0, the value k_comp_init left; a second call over the same components finds the word at its final value.
__global__ void __launch_bounds__(256) k_comp_largest(CompArgs a) {
  __shared__ unsigned long long s_m[kFusionBlock];
  const unsigned tid = threadIdx.x, v = blockIdx.x * (unsigned)kFusionBlock + tid;
  unsigned long long m = 0ull;
  if (v < a.n_vert && a.R[v] == v) m = ((unsigned long long)a.S[v] << 32) | (unsigned long long)(0xffffffffu - v);
  s_m[tid] = m;
  __syncthreads();
  for (unsigned d = kFusionBlock / 2; d > 0; d >>= 1) {
    if (tid < d) s_m[tid] = max(s_m[tid], s_m[tid + d]);
    __syncthreads();
  }
  if (tid == 0 && s_m[0] != 0ull) comp_global_max(a.best, s_m[0]);
}

// Whether the component with root r and `size` triangles is kept.
__device__ __forceinline__ bool comp_keep(const CompArgs& a, unsigned r, unsigned size) {
  return size >= a.min_triangles && (!a.largest || r == 0xffffffffu - (unsigned)(*a.best & 0xffffffffull));
}

// Workgroups 0 .. vblk - 1, one lane a vertex: its size S[R[v]] goes to L, which nobody reads any more (as k_speckle_apply
// does), its keep flag with the in-block exclusive scan of the flags to V, the block's total and its number of kept roots to
// blk_tot.  The other workgroups, one lane a triangle: the same with the flag of its first vertex, to T.  S, R and `best` are
// only read here; L, V and T are only written, each word by its own lane.
__global__ void __launch_bounds__(256) k_comp_flags(CompArgs a) {
  __shared__ unsigned s_p[2][kFusionBlock];
  __shared__ unsigned s_roots;
  const unsigned tid = threadIdx.x;
  unsigned total;
  if (blockIdx.x < a.vblk) {                    // (the same for every lane of the workgroup)
    const unsigned v = blockIdx.x * (unsigned)kFusionBlock + tid;
    if (tid == 0) s_roots = 0u;
    bool keep = false;
    unsigned r = kCompNone;
    if (v < a.n_vert) {
      r = a.R[v];
      const unsigned size = a.S[r];
      a.L[v] = size;
      keep = comp_keep(a, r, size);
    }
    const unsigned incl = comp_scan(s_p, tid, keep ? 1u : 0u, total);        // (its first barrier stands behind s_roots = 0)
    if (keep && r == v) seg_lds_add(&s_roots, 1u);
    if (v < a.n_vert) a.V[v] = ((incl - (keep ? 1u : 0u)) << 1) | (keep ? 1u : 0u);
    __syncthreads();
    if (tid == 0) {
      a.blk_tot[blockIdx.x] = total;
      a.blk_tot[(unsigned long long)a.vblk + (a.n_tri + kFusionBlock - 1) / kFusionBlock + blockIdx.x] = s_roots;
    }
    return;
  }
  const unsigned long long t = (unsigned long long)(blockIdx.x - a.vblk) * (unsigned long long)kFusionBlock + tid;
  bool keep = false;
  if (t < a.n_tri) {
    const unsigned r = a.R[a.faces[t * 3]];
    keep = comp_keep(a, r, a.S[r]);
  }
  const unsigned incl = comp_scan(s_p, tid, keep ? 1u : 0u, total);
  if (t < a.n_tri) a.T[t] = ((incl - (keep ? 1u : 0u)) << 1) | (keep ? 1u : 0u);
  if (tid == 0) a.blk_tot[blockIdx.x] = total;
}

// One lane a vertex: a kept vertex copies its rows to off_v[block] + prefix and leaves that index in V; a dropped one leaves
// kCompNone.  V is read and written by its own lane alone.
__global__ void __launch_bounds__(256) k_comp_vertices(CompArgs a) {
  const unsigned v = blockIdx.x * (unsigned)kFusionBlock + threadIdx.x;
  if (v >= a.n_vert) return;
  const unsigned code = a.V[v];
  if (!(code & 1u)) {
    a.V[v] = kCompNone;
    return;
  }
  const unsigned long long o = a.off_v[blockIdx.x] + (unsigned long long)(code >> 1);        // o <= v
#pragma unroll
  for (int c = 0; c < 3; ++c) a.p_xyz[o * 3 + c] = a.xyz[(unsigned long long)v * 3 + c];
  a.p_key[o] = a.key[v];
  a.p_grey[o] = a.grey[v];
  if (a.bgr) {
#pragma unroll
    for (int c = 0; c < 3; ++c) a.p_bgr[o * 3 + c] = a.bgr[(unsigned long long)v * 3 + c];
  }
  if (a.normal) {
#pragma unroll
    for (int c = 0; c < 3; ++c) a.p_normal[o * 3 + c] = a.normal[(unsigned long long)v * 3 + c];
  }
  a.V[v] = (unsigned)o;
}

// One lane a triangle: a kept triangle writes the new indices of its three vertices, which its component keeps with it, at
// off_t[block] + prefix.
__global__ void __launch_bounds__(256) k_comp_faces(CompArgs a) {
  const unsigned long long t = (unsigned long long)blockIdx.x * (unsigned long long)kFusionBlock + threadIdx.x;
  if (t >= a.n_tri) return;
  const unsigned code = a.T[t];
  if (!(code & 1u)) return;
  const unsigned long long o = a.off_t[blockIdx.x] + (unsigned long long)(code >> 1);
#pragma unroll
  for (int c = 0; c < 3; ++c) a.p_faces[o * 3 + c] = a.V[a.faces[t * 3 + c]];
}

#ifndef EKF_KERNELS_ONLY
// Host side: the scratch, the labels and sizes of the last weld's components and the pruned copy of that weld, owned by the
// fusion handle beside its TsdfMesh; allocated by the first call that needs them, grow-only.  The handle's MeshStamps say
// which weld they belong to.  A timer of its own, so that the four other getters count what they counted.
struct TsdfComponents {
  DevBuf<unsigned> L, R, S, V, T, blk_tot, n_roots;
  DevBuf<unsigned long long> off, best;
  DevMeshBufs out;                                             // the pruned mesh
  unsigned long long n_comp = 0;                               // of the components
  unsigned long long n_kept = 0;                               // of the pruned mesh
  KernelTimer<kCompKinds> timer;

  // three rows of offsets, each ending at the last word of its row of `pitch` words, so that the totals stand one pitch apart
  static size_t pitch(unsigned vblk, unsigned tblk) { return (size_t)std::max(vblk, tblk) + 1; }

  CompArgs args(const MeshView& m, bool colour) const {
    CompArgs a{};
    a.faces = m.faces;
    a.L = L; a.R = R; a.S = S; a.V = V; a.T = T; a.blk_tot = blk_tot;
    a.best = best; a.n_roots = n_roots;
    a.n_vert = (unsigned)m.n_vert; a.vblk = fusion_blocks(m.n_vert); a.n_tri = m.n_tri;
    const unsigned tblk = fusion_blocks(m.n_tri);
    const size_t P = pitch(a.vblk, tblk);
    a.off_v = off + (P - 1 - a.vblk);
    a.off_t = off + P + (P - 1 - tblk);
    a.min_triangles = 1; a.largest = 0;
    a.xyz = m.xyz; a.key = m.key; a.grey = m.grey;
    a.bgr = colour ? m.bgr : nullptr;
    a.normal = m.has_normals ? m.normal : nullptr;
    return a;
  }

  // init -> union -> count -> (flags, for the sizes in L, unless a prune follows, whose own flags leave them there) -> one
  // 4-byte read-back.  No launch for a weld without triangles.
  hipError_t components(MeshStamps& st, const MeshView& m, bool colour, bool with_sizes = true) {
    hipError_t e;
    if ((e = timer.create()) != hipSuccess) return e;
    st.comp.valid = st.pruned.valid = false;
    if (m.n_tri > 0) {
      const size_t nv = (size_t)m.n_vert, nt = (size_t)m.n_tri;
      const unsigned vblk = fusion_blocks(m.n_vert), tblk = fusion_blocks(m.n_tri);
      if ((e = L.reserve(nv)) != hipSuccess || (e = R.reserve(nv)) != hipSuccess || (e = S.reserve(nv)) != hipSuccess ||
          (e = V.reserve(nv)) != hipSuccess || (e = T.reserve(nt)) != hipSuccess ||
          (e = blk_tot.reserve((size_t)vblk * 2 + tblk)) != hipSuccess || (e = off.reserve(3 * pitch(vblk, tblk))) != hipSuccess ||
          (e = best.reserve(1)) != hipSuccess || (e = n_roots.reserve(1)) != hipSuccess) {
        (void)hipGetLastError();
        return e;
      }
      const CompArgs a = args(m, colour);
      if ((e = timer.run(0, [&] { k_comp_init<<<vblk, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
      if ((e = timer.run(1, [&] { k_comp_union<<<tblk, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
      if ((e = timer.run(2, [&] { k_comp_count<<<vblk + tblk, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
      if (with_sizes && (e = timer.run(4, [&] { k_comp_flags<<<vblk + tblk, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
      unsigned roots = 0;
      if ((e = hipMemcpy(&roots, n_roots, sizeof(roots), hipMemcpyDeviceToHost)) != hipSuccess) return e;
      n_comp = roots;
    } else {
      n_comp = 0;
    }
    st.made(st.comp, m.id, 0);
    return hipSuccess;
  }

  // (components, unless the handle holds them for this weld) -> (largest) -> flags -> three scans -> one read-back of the three
  // totals -> (grow the pruned mesh's buffers) -> vertices -> faces.  The weld is only read.
  hipError_t prune(MeshStamps& st, const MeshView& m, bool colour, unsigned min_triangles, bool largest) {
    hipError_t e;
    if (!st.comp.made_from(m.id) && (e = components(st, m, colour, false)) != hipSuccess) return e;
    st.begin(st.pruned);
    unsigned long long totals[3] = {0, 0, 0};
    if (m.n_tri > 0) {
      const unsigned vblk = fusion_blocks(m.n_vert), tblk = fusion_blocks(m.n_tri);
      const size_t P = pitch(vblk, tblk);
      CompArgs a = args(m, colour);
      a.min_triangles = min_triangles;
      a.largest = largest ? 1 : 0;
      if (largest && (e = timer.run(3, [&] { k_comp_largest<<<vblk, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
      if ((e = timer.run(4, [&] { k_comp_flags<<<vblk + tblk, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) {
        st.comp.valid = false;          // L may not hold the sizes
        return e;
      }
      unsigned long long* off_r = off + 2 * P + (P - 1 - vblk);
      const unsigned* tot = blk_tot;
      if ((e = timer.run(5, [&] { k_tsdf_scan<<<1, kFusionBlock, 0, nullptr>>>(tot, (unsigned long long*)a.off_v, vblk); })) != hipSuccess) return e;
      if ((e = timer.run(5, [&] { k_tsdf_scan<<<1, kFusionBlock, 0, nullptr>>>(tot + vblk, (unsigned long long*)a.off_t, tblk); })) != hipSuccess) return e;
      if ((e = timer.run(5, [&] { k_tsdf_scan<<<1, kFusionBlock, 0, nullptr>>>(tot + vblk + tblk, off_r, vblk); })) != hipSuccess) return e;
      if ((e = hipMemcpy2D(totals, sizeof(totals[0]), off + (P - 1), P * sizeof(totals[0]), sizeof(totals[0]), 3, hipMemcpyDeviceToHost)) != hipSuccess)
        return e;
      const size_t nv = (size_t)totals[0], ncorner = (size_t)totals[1] * 3;
      if ((e = out.grow(nv, ncorner, colour, m.has_normals)) != hipSuccess) {
        (void)hipGetLastError();
        return e;
      }
      a.p_xyz = out.xyz; a.p_key = out.key; a.p_grey = out.grey; a.p_bgr = out.bgr; a.p_normal = out.normal; a.p_faces = out.faces;
      if (nv > 0 && (e = timer.run(6, [&] { k_comp_vertices<<<vblk, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
      if (ncorner > 0 && (e = timer.run(7, [&] { k_comp_faces<<<tblk, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
    }
    out.n_vert = totals[0];
    out.n_tri = totals[1];
    n_kept = totals[2];
    out.has_normals = m.has_normals;
    st.made(st.pruned, m.id, 0);
    return hipSuccess;
  }
};
#endif  // EKF_KERNELS_ONLY

}  // namespace ekf

