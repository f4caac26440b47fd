// Vertex-clustering simplification (Rossignac and Borrel) of the welded, the pruned or the smoothed mesh, on the device
// (DESIGN.md §28).  The surface is marching tetrahedra: up to seven vertices belong to one voxel, far more triangles than the
// geometry needs.  The reference has no counterpart; the contract is pinned here and restated in numpy by
// tests/simplify_oracle.py.  The input is a source mesh (X, F, grey, optional bgr, optional normals) with n_vert vertices and
// n_tri triangles, the volume's origin, dims and voxel, and a cell size `cell` (fp64, finite, cell >= voxel).  Every fp64
// operation is rounded once, with contraction off:
//   1. the grid.  G_a = (int) floor(((double)(dims_a - 1) * voxel) / cell) + 1 for a = x, y, z, so G_a <= dims_a: the grid never
//      has more cells than the volume has voxels.  For a vertex, q_a = floor((X[v][a] - origin[a]) / cell): a division, not a
//      multiplication by a reciprocal; a result that is not finite counts as 0; the result is clamped to [0, G_a - 1] (a smoothed
//      vertex may leave the box, so the clamp is part of the contract).  cell(v) = (q_z G_y + q_y) G_x + q_x, x fastest, as in
//      the volume;
//   2. the triangles.  Triangle t has the cells (cell(F[t][0]), cell(F[t][1]), cell(F[t][2])).  It is degenerate iff two of them
//      are equal.  A non-degenerate triangle is a duplicate iff a non-degenerate triangle with a smaller index has the same
//      unordered triple of cells.  The kept triangles are the rest, in the source's order and with the source's winding;
//   3. the vertices.  A cell is used iff a kept triangle has it.  The output has one vertex per used cell, numbered by ascending
//      cell id; that cell id is the output's key, so keys ascend strictly.  A cell that holds vertices but no kept triangle
//      gives no vertex.  With M(c) the ascending list of the source vertices of cell c and n = |M(c)|:
//        position: per coordinate, s = X[m0], then s = s + X[mi] in the order of M(c), then s / (double) n;
//        grey, and each of B, G, R of a colour volume: (2 S + n) / (2 n) in unsigned 64-bit integer arithmetic, S the sum: the
//          mean, with halves rounded up;
//        normal (iff the source has normals): the members' float normals summed as doubles in the order of M(c), starting from
//          the first one's; len = sqrt((a0 a0 + a1 a1) + a2 a2); each a_c / len rounded once to float; 0 0 0 where len is 0 or
//          not finite: §24's normalisation.  A source without normals gives a result without normals;
//   4. the faces: the kept triangles, each index replaced by the output number of its cell;
//   5. the vertex map: for every source vertex, the output number of its cell, or 0xffffffff if the cell is unused;
//   6. the counts: n_vert_out, n_tri_out, n_degenerate, n_duplicate, with n_tri_out + n_degenerate + n_duplicate = n_tri.
//
// Why arrival order costs no bit.  The only atomics are integer adds (the member count of a cell, the number of non-degenerate
// triangles filed under their least cell, the number of corners of kept triangles in a cell: exact in any order) and the
// cursors of k_simp_fill, which hand every vertex a slot of its own in its cell's segment of `mem` and every non-degenerate
// triangle one in its least cell's segment of `tl`.  Which entry gets which slot differs from run to run; k_simp_lists, the next
// launch, has the one lane that owns a cell put both segments in ascending order before anything reads them: the members by
// vertex index, the triangles by (middle cell, greatest cell, triangle index), so that the triangles of one unordered triple
// stand side by side with the least index first, and a triangle is a duplicate iff its predecessor has its triple.  Every fp64
// sum then runs over a list whose order is a function of X, F and the grid.  No workgroup reads, inside a launch, what another
// one writes, and none waits for another: the atomics' return values are the only communication, and relaxed order suffices.
//
// The launches, 256 lanes a workgroup, on the default stream; vblk = ceil(n_vert / 256), tblk = ceil(n_tri / 256),
// cblk = ceil(G_x G_y G_z / 256).  None is made for a source without triangles.
//                (hipMemsetAsync: the three counters of every cell = 0)
//   k_simp_cells     vblk          cell(v) to vcell, cnt_v[cell(v)] += 1
//   k_simp_count     tblk          degenerate, or the triple's middle and greatest cell to `pair` and cnt_t[least cell] += 1
//   k_simp_offsets   cblk          the in-block exclusive scans of cnt_v and cnt_t, the block totals; both become cursors (0)
//   k_tsdf_scan      1, twice      ekf_fusion.hpp's, unchanged: the block offsets of the members and of the triangle lists
//   k_simp_fill      vblk + tblk   mem[first_v(c) + cursor++] = v; tl[first_t(c) + cursor++] = t (the cursors end at the counts)
//   k_simp_lists     cblk          one lane a cell: both lists in order in place, the duplicates flagged, ref[c] += 1 for the
//                                  three cells of every kept triangle
//   k_simp_flags     cblk + tblk   used = ref > 0 and kept, with their in-block exclusive scans and the block totals, and the
//                                  degenerate triangles of a block
//   k_tsdf_scan      1, 3 times    used cells, kept triangles, degenerate triangles
//                one read-back of the three totals
//   k_simp_map       vblk          the vertex map
//   k_simp_vertices  cblk          not for an empty result: one lane a used cell, the means over M(c)
//   k_simp_faces     tblk          likewise
// Lists are ordered in place in global memory by the one lane that owns them: an insertion sort up to 16 entries, a heap sort
// beyond (the prototype sees member lists of 98 entries at cell = 3.5 voxel; any length is correct, and a cell so large that
// one cell holds every vertex is sorted in n log n steps, by one lane).  No kernel has a per-lane array and none uses scratch.
// Scratch: 20 bytes a cell (cnt_v, cnt_t, pre_v, pre_t, ref), 12 bytes a source vertex (vcell, mem, the map), 20 bytes a
// source triangle (tl, T, pair), 20 + 16 bytes a cell block and 8 + 16 a triangle block; the result has buffers of its own.
#pragma once
#include "ekf_mesh_smooth.hpp"

namespace ekf {

// k_simp_cells, k_simp_count, k_simp_offsets, k_tsdf_scan, k_simp_fill, k_simp_lists, k_simp_flags, k_simp_vertices,
// k_simp_faces, k_simp_map
constexpr int kSimpKinds = 10;
constexpr unsigned kSimpNone = 0xffffffffu;      // the map's word of a vertex whose cell is unused
constexpr unsigned kSimpDegenerate = 0u, kSimpDuplicate = 1u, kSimpKept = 2u;      // T[t] until k_simp_flags
constexpr unsigned kSimpInsertion = 16u;         // the longest list the insertion sort orders

struct SimpArgs {
  const double* xyz;                  // the source's rows
  const unsigned char* grey;
  const unsigned char* bgr;           // NULL = a plain volume
  const float* normal;                // NULL = a source without normals
  const unsigned* faces;
  unsigned n_vert, vblk;
  unsigned long long n_tri;
  double origin[3], cell;
  unsigned G[3], ncell, cblk;
  unsigned* vcell;                    // n_vert words: cell(v)
  unsigned* mem;                      // n_vert words: M(c) at first_v(c)
  unsigned* cnt_v;                    // ncell words each: |M(c)|; k_simp_fill's cursor in between
  unsigned* cnt_t;                    //   the non-degenerate triangles whose least cell is c; likewise
  unsigned* pre_v;                    //   the exclusive prefix of cnt_v inside c's block of 256
  unsigned* pre_t;                    //   and of cnt_t
  unsigned* ref;                      //   the corners of kept triangles in c, then (in-block exclusive prefix << 1) | used
  unsigned* tl;                       // n_tri words: the triangles of c at first_t(c)
  unsigned* T;                        // n_tri words: kSimpDegenerate .. kSimpKept, then (in-block exclusive prefix << 1) | kept
  unsigned long long* pair;           // n_tri words: (middle cell << 32) | greatest cell of a non-degenerate triangle
  unsigned* tot_v;                    // cblk words each: the block totals of cnt_v,
  unsigned* tot_t;                    //   of cnt_t
  unsigned* tot_c;                    //   and of the used cells
  unsigned* tot_k;                    // tblk words each: of the kept
  unsigned* tot_d;                    //   and of the degenerate triangles
  const unsigned long long* off_v;    // their exclusive scans (k_tsdf_scan): first_v(c) = off_v[c / 256] + pre_v[c]
  const unsigned long long* off_t;
  const unsigned long long* off_c;    // the output number of a used cell: off_c[c / 256] + (ref[c] >> 1)
  const unsigned long long* off_k;
  double* o_xyz;                      // the result's
  unsigned long long* o_key;
  unsigned char* o_grey;
  unsigned char* o_bgr;
  float* o_normal;
  unsigned* o_faces;
  unsigned* map;                      // n_vert words
};

__device__ __forceinline__ unsigned long long simp_first_v(const SimpArgs& a, unsigned c) {
  return a.off_v[c >> 8] + (unsigned long long)a.pre_v[c];
}
__device__ __forceinline__ unsigned long long simp_first_t(const SimpArgs& a, unsigned c) {
  return a.off_t[c >> 8] + (unsigned long long)a.pre_t[c];
}
__device__ __forceinline__ unsigned simp_rank(const SimpArgs& a, unsigned c) {
  return (unsigned)(a.off_c[c >> 8] + (unsigned long long)(a.ref[c] >> 1));
}

// The orders of the two lists: the members by index; the triangles by their pair and then by index.
struct SimpByIndex {
  __device__ __forceinline__ bool operator()(unsigned x, unsigned y) const { return x < y; }
};
struct SimpByPair {
  const unsigned long long* pair;
  __device__ __forceinline__ bool operator()(unsigned x, unsigned y) const {
    const unsigned long long px = pair[x], py = pair[y];
    return px < py || (px == py && x < y);
  }
};

// a[root] sinks to its place in the heap a[0 .. n) (the greatest entry at the top).  64-bit indices: 2 root + 1 may pass 2^32.
template <typename Less>
__device__ __forceinline__ void simp_sift(unsigned* a, unsigned long long root, unsigned long long n, Less less) {
  const unsigned x = a[root];
  for (;;) {
    unsigned long long child = 2 * root + 1;
    if (child >= n) break;
    if (child + 1 < n && less(a[child], a[child + 1])) ++child;
    if (!less(x, a[child])) break;
    a[root] = a[child];
    root = child;
  }
  a[root] = x;
}

// a[0 .. n) in ascending order of `less`, in place, by the one lane that owns it: every index it touches lies below n.
template <typename Less>
__device__ __forceinline__ void simp_sort(unsigned* a, unsigned n, Less less) {
  if (n <= kSimpInsertion) {
    for (unsigned i = 1; i < n; ++i) {
      const unsigned x = a[i];
      unsigned j = i;
      for (; j > 0 && less(x, a[j - 1]); --j) a[j] = a[j - 1];
      a[j] = x;
    }
    return;
  }
  for (unsigned long long s = n / 2; s-- > 0;) simp_sift(a, s, n, less);
  for (unsigned long long end = (unsigned long long)n - 1; end > 0; --end) {
    const unsigned top = a[0];
    a[0] = a[end];
    a[end] = top;
    simp_sift(a, 0, end, less);
  }
}

// One lane a source vertex: its cell, and that cell's member count gains 1.  Unsigned sums are exact in any order.  The vertices
// of a weld stand in voxel order, so the adds of a wave go to a few neighbouring words, at most seven to one at cell = voxel
// (cdna_hip_programming.md, Guideline 12); a coarse grid makes a word hotter, which is unmeasured.
__global__ void __launch_bounds__(256) k_simp_cells(SimpArgs a) {
#pragma clang fp contract(off)
  const unsigned v = blockIdx.x * (unsigned)kFusionBlock + threadIdx.x;
  if (v >= a.n_vert) return;
  unsigned q[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double d = floor((a.xyz[(unsigned long long)v * 3 + c] - a.origin[c]) / a.cell);
    if (!(d > -INFINITY && d < INFINITY)) d = 0.0;                           // (a NaN fails both)
    const double top = (double)(a.G[c] - 1u);
    d = d < 0.0 ? 0.0 : (d > top ? top : d);
    q[c] = (unsigned)d;
  }
  const unsigned id = (q[2] * a.G[1] + q[1]) * a.G[0] + q[0];                 // < ncell: every q_a <= G_a - 1
  a.vcell[v] = id;
  seg_global_add(&a.cnt_v[id], 1u);
}

// One lane a source triangle: degenerate, or filed under its least cell with the two other cells of its triple in `pair`.
__global__ void __launch_bounds__(256) k_simp_count(SimpArgs a) {
  const unsigned long long t = (unsigned long long)blockIdx.x * (unsigned long long)kFusionBlock + threadIdx.x;
  if (t >= a.n_tri) return;
  const unsigned c0 = a.vcell[a.faces[t * 3]], c1 = a.vcell[a.faces[t * 3 + 1]], c2 = a.vcell[a.faces[t * 3 + 2]];
  if (c0 == c1 || c0 == c2 || c1 == c2) {
    a.T[t] = kSimpDegenerate;
    return;
  }
  const unsigned lo = min(c0, min(c1, c2)), hi = max(c0, max(c1, c2)), mid = c0 + c1 + c2 - lo - hi;       // (3 ncell < 2^32)
  a.pair[t] = ((unsigned long long)mid << 32) | (unsigned long long)hi;
  a.T[t] = kSimpKept;                                                          // until k_simp_lists finds it a duplicate
  seg_global_add(&a.cnt_t[lo], 1u);
}

// One lane a cell: the in-block exclusive scans of cnt_v and cnt_t to pre_v and pre_t, the block's totals, and both counters
// cleared: they are k_simp_fill's cursors, which end at the counts again.
__global__ void __launch_bounds__(256) k_simp_offsets(SimpArgs a) {
  __shared__ unsigned s_p[2][kFusionBlock];
  const unsigned tid = threadIdx.x, c = blockIdx.x * (unsigned)kFusionBlock + tid;
  const bool in = c < a.ncell;
  const unsigned nv = in ? a.cnt_v[c] : 0u, nt = in ? a.cnt_t[c] : 0u;
  unsigned total_v, total_t;
  const unsigned incl_v = comp_scan(s_p, tid, nv, total_v);
  __syncthreads();                                                             // every lane has read the first scan's rows
  const unsigned incl_t = comp_scan(s_p, tid, nt, total_t);
  if (in) {
    a.pre_v[c] = incl_v - nv;
    a.pre_t[c] = incl_t - nt;
    a.cnt_v[c] = 0u;
    a.cnt_t[c] = 0u;
  }
  if (tid == 0) {
    a.tot_v[blockIdx.x] = total_v;
    a.tot_t[blockIdx.x] = total_t;
  }
}

// Workgroups 0 .. vblk - 1, one lane a source vertex: it takes the next free slot of its cell's segment of mem.  The others,
// one lane a triangle: a non-degenerate one takes the next free slot of its least cell's segment of tl.  The slot depends on
// the order of arrival; k_simp_lists removes that dependence before anything reads a segment.  A cursor stays below the count
// that k_simp_cells or k_simp_count made of exactly these entries, so a slot lies inside its segment.
__global__ void __launch_bounds__(256) k_simp_fill(SimpArgs a) {
  if (blockIdx.x < a.vblk) {                    // (the same for every lane of the workgroup)
    const unsigned v = blockIdx.x * (unsigned)kFusionBlock + threadIdx.x;
    if (v >= a.n_vert) return;
    const unsigned c = a.vcell[v];
    const unsigned slot = seg_global_add(&a.cnt_v[c], 1u);
    a.mem[simp_first_v(a, c) + slot] = v;
    return;
  }
  const unsigned long long t = (unsigned long long)(blockIdx.x - a.vblk) * (unsigned long long)kFusionBlock + threadIdx.x;
  if (t >= a.n_tri || a.T[t] == kSimpDegenerate) return;
  const unsigned c = min(a.vcell[a.faces[t * 3]], min(a.vcell[a.faces[t * 3 + 1]], a.vcell[a.faces[t * 3 + 2]]));
  const unsigned slot = seg_global_add(&a.cnt_t[c], 1u);
  a.tl[simp_first_t(a, c) + slot] = (unsigned)t;
}

// One lane a cell, which alone reads and writes its two segments (what k_simp_fill stored is visible by the kernel boundary).
// M(c) in ascending order; the cell's triangles by (pair, index), so that a triangle is a duplicate iff its predecessor has its
// pair (the least cell is the list's own); the three cells of a kept triangle gain 1 in ref, the one word here that other
// lanes add to as well.  A cell without vertices has neither list.
__global__ void __launch_bounds__(256) k_simp_lists(SimpArgs a) {
  const unsigned c = blockIdx.x * (unsigned)kFusionBlock + threadIdx.x;
  if (c >= a.ncell) return;
  const unsigned nv = a.cnt_v[c];
  if (nv == 0u) return;
  simp_sort(a.mem + simp_first_v(a, c), nv, SimpByIndex());
  const unsigned nt = a.cnt_t[c];
  if (nt == 0u) return;
  unsigned* L = a.tl + simp_first_t(a, c);
  simp_sort(L, nt, SimpByPair{a.pair});
  unsigned long long before = 0ull;                                            // (no pair is 0: the middle cell is not cell 0)
  for (unsigned i = 0; i < nt; ++i) {
    const unsigned t = L[i];
    const unsigned long long p = a.pair[t];
    if (p == before) {
      a.T[t] = kSimpDuplicate;
      continue;
    }
    before = p;
    seg_global_add(&a.ref[c], 1u);
    seg_global_add(&a.ref[(unsigned)(p >> 32)], 1u);
    seg_global_add(&a.ref[(unsigned)(p & 0xffffffffull)], 1u);
  }
}

// Workgroups 0 .. cblk - 1, one lane a cell: used = ref > 0, with the in-block exclusive scan of the flags into ref's own word
// and the block's total.  The others, one lane a triangle: the same with kept, into T, and the block's degenerate triangles.
__global__ void __launch_bounds__(256) k_simp_flags(SimpArgs a) {
  __shared__ unsigned s_p[2][kFusionBlock];
  __shared__ unsigned s_deg;
  const unsigned tid = threadIdx.x;
  unsigned total;
  if (blockIdx.x < a.cblk) {                    // (the same for every lane of the workgroup)
    const unsigned c = blockIdx.x * (unsigned)kFusionBlock + tid;
    const unsigned used = (c < a.ncell && a.ref[c] != 0u) ? 1u : 0u;
    const unsigned incl = comp_scan(s_p, tid, used, total);
    if (c < a.ncell) a.ref[c] = ((incl - used) << 1) | used;
    if (tid == 0) a.tot_c[blockIdx.x] = total;
    return;
  }
  const unsigned b = blockIdx.x - a.cblk;
  const unsigned long long t = (unsigned long long)b * (unsigned long long)kFusionBlock + tid;
  if (tid == 0) s_deg = 0u;
  const unsigned state = t < a.n_tri ? a.T[t] : kSimpDuplicate;
  const unsigned keep = state == kSimpKept ? 1u : 0u;
  const unsigned incl = comp_scan(s_p, tid, keep, total);                      // (its first barrier stands behind s_deg = 0)
  if (t < a.n_tri && state == kSimpDegenerate) seg_lds_add(&s_deg, 1u);
  if (t < a.n_tri) a.T[t] = ((incl - keep) << 1) | keep;
  __syncthreads();
  if (tid == 0) {
    a.tot_k[b] = total;
    a.tot_d[b] = s_deg;
  }
}

// One lane a source vertex: the output number of its cell, or kSimpNone.
__global__ void __launch_bounds__(256) k_simp_map(SimpArgs a) {
  const unsigned v = blockIdx.x * (unsigned)kFusionBlock + threadIdx.x;
  if (v >= a.n_vert) return;
  const unsigned c = a.vcell[v];
  a.map[v] = (a.ref[c] & 1u) ? simp_rank(a, c) : kSimpNone;
}

// One lane a cell: a used one writes its vertex at its output number: the means over M(c), in M(c)'s order, and its own id as
// the key.  A used cell has a member (a kept triangle's corner), so n >= 1.  Running sums, no array.
__global__ void __launch_bounds__(256) k_simp_vertices(SimpArgs a) {
#pragma clang fp contract(off)
  const unsigned c = blockIdx.x * (unsigned)kFusionBlock + threadIdx.x;
  if (c >= a.ncell) return;
  const unsigned code = a.ref[c];
  if (!(code & 1u)) return;
  const unsigned long long o = a.off_c[blockIdx.x] + (unsigned long long)(code >> 1);
  const unsigned n = a.cnt_v[c];
  const unsigned* M = a.mem + simp_first_v(a, c);
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, a0 = 0.0, a1 = 0.0, a2 = 0.0;
  unsigned long long g = 0ull, b0 = 0ull, b1 = 0ull, b2 = 0ull;
  for (unsigned i = 0; i < n; ++i) {
    const unsigned long long m = M[i];
    const double* x = a.xyz + m * 3;
    if (i == 0) {
      s0 = x[0]; s1 = x[1]; s2 = x[2];
    } else {
      s0 = s0 + x[0]; s1 = s1 + x[1]; s2 = s2 + x[2];
    }
    g += a.grey[m];
    if (a.bgr) {
      b0 += a.bgr[m * 3]; b1 += a.bgr[m * 3 + 1]; b2 += a.bgr[m * 3 + 2];
    }
    if (a.normal) {
      const float* nr = a.normal + m * 3;
      if (i == 0) {
        a0 = (double)nr[0]; a1 = (double)nr[1]; a2 = (double)nr[2];
      } else {
        a0 = a0 + (double)nr[0]; a1 = a1 + (double)nr[1]; a2 = a2 + (double)nr[2];
      }
    }
  }
  const double dn = (double)n;
  const unsigned long long n64 = n;
  a.o_xyz[o * 3] = s0 / dn;
  a.o_xyz[o * 3 + 1] = s1 / dn;
  a.o_xyz[o * 3 + 2] = s2 / dn;
  a.o_key[o] = (unsigned long long)c;
  a.o_grey[o] = (unsigned char)((2ull * g + n64) / (2ull * n64));
  if (a.bgr) {
    a.o_bgr[o * 3] = (unsigned char)((2ull * b0 + n64) / (2ull * n64));
    a.o_bgr[o * 3 + 1] = (unsigned char)((2ull * b1 + n64) / (2ull * n64));
    a.o_bgr[o * 3 + 2] = (unsigned char)((2ull * b2 + n64) / (2ull * n64));
  }
  if (a.normal) {
    const double len = sqrt((a0 * a0 + a1 * a1) + a2 * a2);
    const bool ok = len > 0.0 && len < INFINITY;                               // (a NaN fails)
    a.o_normal[o * 3] = ok ? (float)(a0 / len) : 0.f;
    a.o_normal[o * 3 + 1] = ok ? (float)(a1 / len) : 0.f;
    a.o_normal[o * 3 + 2] = ok ? (float)(a2 / len) : 0.f;
  }
}

// One lane a source triangle: a kept one writes the output numbers of its three cells, all used, at off_k[block] + prefix.
__global__ void __launch_bounds__(256) k_simp_faces(SimpArgs a) {
  const unsigned long long t = (unsigned long long)blockIdx.x * (unsigned long long)kFusionBlock + threadIdx.x;
  if (t >= a.n_tri) return;
  const unsigned code = a.T[t];
  if (!(code & 1u)) return;
  const unsigned long long o = a.off_k[blockIdx.x] + (unsigned long long)(code >> 1);
#pragma unroll
  for (int k = 0; k < 3; ++k) a.o_faces[o * 3 + k] = simp_rank(a, a.vcell[a.faces[t * 3 + k]]);
}

// The grid of the contract for a volume and a cell size (host and device agree: one multiplication, one division, a floor).
inline void simp_grid(const int dims[3], double voxel, double cell, unsigned G[3]) {
  for (int c = 0; c < 3; ++c) {
    const double extent = (double)(dims[c] - 1) * voxel;
    G[c] = (unsigned)((int)std::floor(extent / cell) + 1);
  }
}

#ifndef EKF_KERNELS_ONLY
// Host side: the scratch, the simplified mesh and the vertex map of the last run, owned by the fusion handle beside its
// TsdfSmooth; allocated by the first run, grow-only.  A run reads the view of the last weld, of the last pruned mesh or of the
// last smoothed one and only reads it.  A timer of its own, so that the other getters count what they counted.
struct TsdfSimplify {
  DevBuf<unsigned> vcell, mem, cells, tl, T, blk_tot, map;
  DevBuf<unsigned long long> pair, off;
  DevMeshBufs out;                               // the simplified mesh
  unsigned long long n_src_vert = 0, n_degenerate = 0, n_duplicate = 0;
  KernelTimer<kSimpKinds> timer;

  // memset -> cells -> count -> offsets -> two scans -> fill -> lists -> flags -> three scans -> one read-back of the three
  // totals -> (grow the result's buffers) -> map -> vertices -> faces.  A failed allocation leaves every source as it was (they
  // are only read) and the handle without a result.
  hipError_t run(MeshStamps& st, const MeshView& s, int source, const TsdfGrid& g, double cell, bool colour) {
    hipError_t e;
    if ((e = timer.create()) != hipSuccess) return e;
    st.begin(st.simp);
    unsigned long long totals[3] = {0, 0, 0};
    if (s.n_tri > 0) {
      if (s.n_tri > 0xffffffffull) return hipErrorInvalidValue;              // a triangle's number is a word of `tl`
      SimpArgs a{};
      const int dims[3] = {g.nx, g.ny, g.nz};
      simp_grid(dims, g.voxel, cell, a.G);
      const size_t nc = (size_t)a.G[0] * a.G[1] * a.G[2], nv = (size_t)s.n_vert, nt = (size_t)s.n_tri;
      const unsigned vblk = fusion_blocks(s.n_vert), tblk = fusion_blocks(s.n_tri), cblk = fusion_blocks(nc);
      const size_t P = (size_t)std::max(cblk, tblk) + 1;                       // three rows of offsets, as TsdfComponents has them
      if ((e = vcell.reserve(nv)) != hipSuccess || (e = mem.reserve(nv)) != hipSuccess || (e = map.reserve(nv)) != hipSuccess ||
          (e = cells.reserve(nc * 5)) != hipSuccess || (e = tl.reserve(nt)) != hipSuccess || (e = T.reserve(nt)) != hipSuccess ||
          (e = pair.reserve(nt)) != hipSuccess || (e = blk_tot.reserve((size_t)cblk * 3 + (size_t)tblk * 2)) != hipSuccess ||
          (e = off.reserve(2 * ((size_t)cblk + 1) + 3 * P)) != hipSuccess) {
        (void)hipGetLastError();
        return e;
      }
      a.xyz = s.xyz; a.grey = s.grey; a.bgr = colour ? s.bgr : nullptr; a.normal = s.has_normals ? s.normal : nullptr;
      a.faces = s.faces;
      a.n_vert = (unsigned)s.n_vert; a.vblk = vblk; a.n_tri = s.n_tri;
      for (int c = 0; c < 3; ++c) a.origin[c] = g.origin[c];
      a.cell = cell; a.ncell = (unsigned)nc; a.cblk = cblk;
      a.vcell = vcell; a.mem = mem; a.map = map; a.tl = tl; a.T = T; a.pair = pair;
      a.cnt_v = cells; a.cnt_t = cells + nc; a.ref = cells + 2 * nc; a.pre_v = cells + 3 * nc; a.pre_t = cells + 4 * nc;
      a.tot_v = blk_tot; a.tot_t = blk_tot + cblk; a.tot_c = blk_tot + 2 * (size_t)cblk; a.tot_k = blk_tot + 3 * (size_t)cblk;
      a.tot_d = a.tot_k + tblk;
      unsigned long long* o_v = off;
      unsigned long long* o_t = off + ((size_t)cblk + 1);
      unsigned long long* rows = off + 2 * ((size_t)cblk + 1);                 // each row ends at the last word of its pitch
      unsigned long long* o_c = rows + (P - 1 - cblk);
      unsigned long long* o_k = rows + P + (P - 1 - tblk);
      unsigned long long* o_d = rows + 2 * P + (P - 1 - tblk);
      a.off_v = o_v; a.off_t = o_t; a.off_c = o_c; a.off_k = o_k;
      if ((e = hipMemsetAsync(cells, 0, nc * 3 * sizeof(unsigned), nullptr)) != hipSuccess) return e;
      if ((e = timer.run(0, [&] { k_simp_cells<<<vblk, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
      if ((e = timer.run(1, [&] { k_simp_count<<<tblk, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
      if ((e = timer.run(2, [&] { k_simp_offsets<<<cblk, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
      if ((e = timer.run(3, [&] { k_tsdf_scan<<<1, kFusionBlock, 0, nullptr>>>(a.tot_v, o_v, cblk); })) != hipSuccess) return e;
      if ((e = timer.run(3, [&] { k_tsdf_scan<<<1, kFusionBlock, 0, nullptr>>>(a.tot_t, o_t, cblk); })) != hipSuccess) return e;
      if ((e = timer.run(4, [&] { k_simp_fill<<<vblk + tblk, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
      if ((e = timer.run(5, [&] { k_simp_lists<<<cblk, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
      if ((e = timer.run(6, [&] { k_simp_flags<<<cblk + tblk, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
      if ((e = timer.run(3, [&] { k_tsdf_scan<<<1, kFusionBlock, 0, nullptr>>>(a.tot_c, o_c, cblk); })) != hipSuccess) return e;
      if ((e = timer.run(3, [&] { k_tsdf_scan<<<1, kFusionBlock, 0, nullptr>>>(a.tot_k, o_k, tblk); })) != hipSuccess) return e;
      if ((e = timer.run(3, [&] { k_tsdf_scan<<<1, kFusionBlock, 0, nullptr>>>(a.tot_d, o_d, tblk); })) != hipSuccess) return e;
      if ((e = hipMemcpy2D(totals, sizeof(totals[0]), rows + (P - 1), P * sizeof(totals[0]), sizeof(totals[0]), 3,
                           hipMemcpyDeviceToHost)) != hipSuccess)
        return e;
      const size_t ov = (size_t)totals[0], ocorner = (size_t)totals[1] * 3;
      if ((e = out.grow(ov, ocorner, colour, s.has_normals)) != hipSuccess) {
        (void)hipGetLastError();
        return e;
      }
      a.o_xyz = out.xyz; a.o_key = out.key; a.o_grey = out.grey; a.o_bgr = out.bgr; a.o_normal = out.normal; a.o_faces = out.faces;
      if ((e = timer.run(9, [&] { k_simp_map<<<vblk, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
      if (ov > 0 && (e = timer.run(7, [&] { k_simp_vertices<<<cblk, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
      if (ocorner > 0 && (e = timer.run(8, [&] { k_simp_faces<<<tblk, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
    }
    out.n_vert = totals[0];
    out.n_tri = totals[1];
    out.has_normals = s.has_normals;
    n_degenerate = totals[2];
    n_duplicate = s.n_tri - totals[1] - totals[2];
    n_src_vert = s.n_tri > 0 ? s.n_vert : 0;
    st.made(st.simp, s.id, source);
    return hipSuccess;
  }
};
#endif  // EKF_KERNELS_ONLY

}  // namespace ekf
