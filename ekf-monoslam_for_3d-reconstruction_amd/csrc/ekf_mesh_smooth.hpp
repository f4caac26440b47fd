// Taubin smoothing of the welded mesh or of its pruned copy, and normals from the smoothed triangles, on the device
// (DESIGN.md §26).  The weld of ekf_mesh.hpp and the pruned mesh of ekf_mesh_components.hpp are the raw marching-tetrahedra
// surface: the noise of the mean field and the lattice's staircase stand in the vertices.  The reference has no counterpart;
// the contract is pinned here and restated in numpy by tests/smooth_oracle.py.  The input is a mesh (X, F), X n_vert x 3 fp64,
// F n_tri x 3 uint32 with three distinct indices a triangle (every weld: a triangle's vertices lie on three different edges):
//   1. the adjacency is a function of F alone.  T(v): the ascending list of the triangles that contain v, inc(v) = |T(v)|.
//      N(v): the ascending list of the distinct w != v that share a triangle with v, deg(v) = |N(v)|.  m(v, w): the number of
//      triangles that hold both.  boundary(v) = 1 iff some w has m(v, w) = 1.  Every vertex lies in a triangle, so deg >= 2;
//   2. one step with factor f, every operation rounded once (contraction off): s = X[w0][c], then s = s + X[wi][c] in the order
//      of N(v); mean = s / (double) deg(v); X'[v][c] = X[v][c] + f * (mean - X[v][c]).  With pin_boundary, a vertex with
//      boundary(v) = 1 keeps its bits;
//   3. a run is `iterations` times a step with lambda and then, unless mu == 0, a step with mu (Taubin's scheme wants
//      mu < -lambda; mu == 0 is plain Laplacian smoothing).  faces, key, grey and bgr are the source's rows;
//   4. the normals, on request, from the final positions: over t in T(v) ascending, with A, B, C = X[F[t][0..2]], e1 = B - A,
//      e2 = C - A, the cross products (e1[1] e2[2] - e1[2] e2[1], e1[2] e2[0] - e1[0] e2[2], e1[0] e2[1] - e1[1] e2[0]) are
//      summed from left to right, starting from the first triangle's; len = sqrt((a0 a0 + a1 a1) + a2 a2), each a_c / len
//      rounded once to float, 0 0 0 where len is 0 or not finite: §24's normalisation and orientation.
//
// Why arrival order costs no bit.  The only atomics are integer adds: k_smooth_count's on inc (exact in any order) and
// k_smooth_fill's on a vertex's cursor, which hands every corner of v a slot of its own in v's segment of `tri`.  Which triangle
// gets which slot differs from run to run; k_smooth_lists, the next launch, puts each segment in ascending order before
// anything else reads it, and derives N(v) from it in ascending order too.  Every fp64 sum then runs over a list whose order
// is a function of F.  No workgroup reads, inside a launch, what another one writes: the atomics' return values are the only
// communication, and relaxed order suffices for them (a counter's modification order is all that is used).
//
// The launches, 256 lanes a workgroup, on the default stream; vblk = ceil(n_vert / 256), tblk = ceil(n_tri / 256).  None is
// made for a mesh without triangles.
//   adjacency (once a source mesh):
//                (hipMemsetAsync: inc = 0)
//                k_smooth_count    tblk   inc[F[t][c]] += 1
//                k_smooth_offsets  vblk   the in-block exclusive scan of inc, the block totals, the cursors cleared
//                k_tsdf_scan       1      ekf_fusion.hpp's, unchanged: the block offsets
//                k_smooth_fill     tblk   tri[first(v) + cursor(v)++] = t for the three corners of t
//                k_smooth_lists    vblk   T(v) in ascending order in place; N(v), deg(v) and boundary(v) from it
//   a run:       k_smooth_step     vblk   `iterations` times, or twice that with mu != 0; nothing between them
//                k_smooth_normals  vblk   on request
// Lists are ordered in place in global memory by the one lane that owns them (an insertion sort: they hold 9 entries at the
// most on the test volumes, and any length is correct), so no kernel has a per-lane array and none uses scratch.
// Scratch: 13 bytes a vertex (inc, pre, deg, boundary), 36 bytes a triangle (tri: 3 words, nbr: 6 words: a segment of
// 2 inc(v) words holds v's neighbours with their multiplicities, then the distinct ones), 4 + 8 bytes a vertex block; the
// result is two buffers of 24 bytes a vertex (one when a run is a single step) and 12 bytes a vertex of normals.
#pragma once
#include "ekf_mesh_components.hpp"

namespace ekf {

// k_smooth_count, k_smooth_offsets, k_tsdf_scan, k_smooth_fill, k_smooth_lists, k_smooth_step, k_smooth_normals
constexpr int kSmoothKinds = 7;
constexpr int kSmoothMaxIterations = 1024;

struct SmoothArgs {
  const unsigned* faces;              // the source's: three vertex indices a triangle
  unsigned* inc;                      // n_vert words each: |T(v)|
  unsigned* pre;                      //   the exclusive prefix of inc inside v's block of 256
  unsigned* deg;                      //   k_smooth_fill's cursor, then |N(v)|
  unsigned char* boundary;            // n_vert bytes
  unsigned* blk_tot;                  // vblk words: the sum of inc over a block
  const unsigned long long* off;      // their exclusive scan (k_tsdf_scan): first(v) = off[v / 256] + pre[v]
  unsigned* tri;                      // 3 n_tri words: T(v) at first(v)
  unsigned* nbr;                      // 6 n_tri words: N(v) at 2 first(v)
  const double* src;                  // the positions a step or the normals read
  double* dst;                        // the positions a step writes
  float* normal;
  unsigned n_vert;
  unsigned long long n_tri;
  double f;                           // lambda or mu
  int pin;
};

__device__ __forceinline__ unsigned long long smooth_first(const SmoothArgs& a, unsigned v) {
  return a.off[v >> 8] + (unsigned long long)a.pre[v];
}

// One lane a triangle: each of its three vertices gains 1.  Unsigned sums are exact in any order.  The adds of a wave go to
// up to 192 different words spread over the vertex list (cdna_hip_programming.md, Guideline 12: no word is a hot spot; a
// vertex of a weld has 9 triangles at the most).
__global__ void __launch_bounds__(256) k_smooth_count(SmoothArgs a) {
  const unsigned long long t = (unsigned long long)blockIdx.x * (unsigned long long)kFusionBlock + threadIdx.x;
  if (t >= a.n_tri) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) seg_global_add(&a.inc[a.faces[t * 3 + c]], 1u);
}

// One lane a vertex: the in-block exclusive scan of inc to pre, the block's total to blk_tot, and the cursor of
// k_smooth_fill (which lives in deg until k_smooth_lists writes the degree there) cleared.
__global__ void __launch_bounds__(256) k_smooth_offsets(SmoothArgs a) {
  __shared__ unsigned s_p[2][kFusionBlock];
  const unsigned tid = threadIdx.x, v = blockIdx.x * (unsigned)kFusionBlock + tid;
  const unsigned mine = v < a.n_vert ? a.inc[v] : 0u;
  unsigned total;
  const unsigned incl = comp_scan(s_p, tid, mine, total);
  if (v < a.n_vert) {
    a.pre[v] = incl - mine;
    a.deg[v] = 0u;
  }
  if (tid == 0) a.blk_tot[blockIdx.x] = total;
}

// One lane a triangle: each corner takes the next free slot of its vertex's segment.  The slot a triangle gets depends on
// the order of arrival; k_smooth_lists removes that dependence before anything reads the segment.  A cursor stays below
// inc(v), which counted exactly these corners, so a slot lies inside the segment.
__global__ void __launch_bounds__(256) k_smooth_fill(SmoothArgs a) {
  const unsigned long long t = (unsigned long long)blockIdx.x * (unsigned long long)kFusionBlock + threadIdx.x;
  if (t >= a.n_tri) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const unsigned v = a.faces[t * 3 + c];
    const unsigned slot = seg_global_add(&a.deg[v], 1u);
    a.tri[smooth_first(a, v) + slot] = (unsigned)t;
  }
}

// One lane a vertex, which alone reads and writes its two segments (what k_smooth_fill stored is visible by the kernel
// boundary).  T(v) is put in ascending order by an insertion sort in place; then the two other vertices of every triangle of
// T(v) are inserted in ascending order, equal ones side by side, into the 2 inc(v) words of v's segment of nbr; then the runs
// of equal entries are counted, a run of one marks the boundary, and the distinct entries move to the front.  Correct for any
// length; quadratic in it, and a weld's lists hold 9 entries at the most.  No array of the lane's own, so no scratch.
__global__ void __launch_bounds__(256) k_smooth_lists(SmoothArgs a) {
  const unsigned v = blockIdx.x * (unsigned)kFusionBlock + threadIdx.x;
  if (v >= a.n_vert) return;
  const unsigned long long first = smooth_first(a, v);
  const unsigned n = a.inc[v];
  unsigned* T = a.tri + first;
  for (unsigned i = 1; i < n; ++i) {
    const unsigned x = T[i];
    unsigned j = i;
    for (; j > 0 && T[j - 1] > x; --j) T[j] = T[j - 1];
    T[j] = x;
  }
  unsigned* N = a.nbr + 2 * first;
  unsigned m = 0;                                                            // <= 2 n: two others a corner of v
  for (unsigned i = 0; i < n; ++i) {
    const unsigned long long t = T[i];
    for (int c = 0; c < 3; ++c) {
      const unsigned w = a.faces[t * 3 + c];
      if (w == v) continue;
      unsigned j = m;
      for (; j > 0 && N[j - 1] > w; --j) N[j] = N[j - 1];
      N[j] = w;
      ++m;
    }
  }
  unsigned d = 0, b = 0;
  for (unsigned i = 0; i < m;) {
    const unsigned w = N[i];
    unsigned j = i + 1;
    while (j < m && N[j] == w) ++j;
    if (j - i == 1) b = 1u;                                                  // m(v, w) = 1
    N[d++] = w;                                                              // d <= i: behind the entries still to be read
    i = j;
  }
  a.deg[v] = d;
  a.boundary[v] = (unsigned char)b;
}

// One lane a vertex: the mean of its neighbours in the order of N(v), from src, and its new position to dst, another buffer:
// no lane reads what a lane of this launch writes.  Three running sums, no array.
__global__ void __launch_bounds__(256) k_smooth_step(SmoothArgs a) {
#pragma clang fp contract(off)
  const unsigned v = blockIdx.x * (unsigned)kFusionBlock + threadIdx.x;
  if (v >= a.n_vert) return;
  const double* x = a.src + (unsigned long long)v * 3;
  double* y = a.dst + (unsigned long long)v * 3;
  const double x0 = x[0], x1 = x[1], x2 = x[2];
  const unsigned d = a.deg[v];
  if (d == 0u || (a.pin && a.boundary[v])) {                                 // (d = 0: a vertex in no triangle; no weld has one)
    y[0] = x0; y[1] = x1; y[2] = x2;
    return;
  }
  const unsigned* N = a.nbr + 2 * smooth_first(a, v);
  const double* p = a.src + (unsigned long long)N[0] * 3;
  double s0 = p[0], s1 = p[1], s2 = p[2];
  for (unsigned i = 1; i < d; ++i) {
    p = a.src + (unsigned long long)N[i] * 3;
    s0 = s0 + p[0];
    s1 = s1 + p[1];
    s2 = s2 + p[2];
  }
  const double dd = (double)d;
  const double m0 = s0 / dd, m1 = s1 / dd, m2 = s2 / dd;
  y[0] = x0 + a.f * (m0 - x0);
  y[1] = x1 + a.f * (m1 - x1);
  y[2] = x2 + a.f * (m2 - x2);
}

// One lane a vertex: the cross products of its triangles in the order of T(v), summed from the first one's, normalised as
// k_mesh_vertices normalises.
__global__ void __launch_bounds__(256) k_smooth_normals(SmoothArgs a) {
#pragma clang fp contract(off)
  const unsigned v = blockIdx.x * (unsigned)kFusionBlock + threadIdx.x;
  if (v >= a.n_vert) return;
  const unsigned n = a.inc[v];
  const unsigned* T = a.tri + smooth_first(a, v);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  for (unsigned i = 0; i < n; ++i) {
    const unsigned long long t = T[i];
    const double* A = a.src + (unsigned long long)a.faces[t * 3] * 3;
    const double* B = a.src + (unsigned long long)a.faces[t * 3 + 1] * 3;
    const double* C = a.src + (unsigned long long)a.faces[t * 3 + 2] * 3;
    const double A0 = A[0], A1 = A[1], A2 = A[2];
    const double e10 = B[0] - A0, e11 = B[1] - A1, e12 = B[2] - A2;
    const double e20 = C[0] - A0, e21 = C[1] - A1, e22 = C[2] - A2;
    const double n0 = e11 * e22 - e12 * e21;
    const double n1 = e12 * e20 - e10 * e22;
    const double n2 = e10 * e21 - e11 * e20;
    if (i == 0) {
      a0 = n0; a1 = n1; a2 = n2;
    } else {
      a0 = a0 + n0; a1 = a1 + n1; a2 = a2 + n2;
    }
  }
  const double len = sqrt((a0 * a0 + a1 * a1) + a2 * a2);
  const bool ok = len > 0.0 && len < INFINITY;                               // (a NaN fails)
  float* o = a.normal + (unsigned long long)v * 3;
  o[0] = ok ? (float)(a0 / len) : 0.f;
  o[1] = ok ? (float)(a1 / len) : 0.f;
  o[2] = ok ? (float)(a2 / len) : 0.f;
}

#ifndef EKF_KERNELS_ONLY
// Host side: the adjacency of one source mesh and the last run's positions and normals, owned by the fusion handle beside
// its TsdfMesh and TsdfComponents; allocated by the first run, grow-only.  A run reads the view of the last weld or of the last
// pruned mesh and only reads it.  A timer of its own, so that the other getters count what they counted.
struct TsdfSmooth {
  DevBuf<unsigned> inc, pre, deg, blk_tot, tri, nbr;
  DevBuf<unsigned char> boundary;
  DevBuf<unsigned long long> off;
  DevBuf<double> pos[2];
  DevBuf<float> normal;
  bool has_normals = false;
  int last = 0;                       // the buffer that holds the result
  KernelTimer<kSmoothKinds> timer;

  // the last run's mesh, named `id`: the rows of its source with the positions and the normals of the run
  MeshView result(const DevMeshBufs& src, unsigned long long id) const {
    MeshView r = MeshView::of(src, id);
    r.xyz = pos[last];
    r.normal = normal;
    r.has_normals = has_normals;
    return r;
  }

  SmoothArgs args(const MeshView& s) const {
    SmoothArgs a{};
    a.faces = s.faces;
    a.inc = inc; a.pre = pre; a.deg = deg; a.boundary = boundary; a.blk_tot = blk_tot; a.off = off; a.tri = tri; a.nbr = nbr;
    a.n_vert = (unsigned)s.n_vert; a.n_tri = s.n_tri;
    return a;
  }

  // memset -> count -> offsets -> scan -> fill -> lists.  No read-back: the lists' total is 3 n_tri.
  hipError_t adjacency(MeshStamps& st, const MeshView& s, int source) {
    hipError_t e;
    st.adj.valid = false;
    const size_t nv = (size_t)s.n_vert, nt = (size_t)s.n_tri;
    const unsigned vblk = fusion_blocks(s.n_vert), tblk = fusion_blocks(s.n_tri);
    if (s.n_tri > 0xffffffffull) return hipErrorInvalidValue;                // a triangle's number is a word of `tri`
    if ((e = inc.reserve(nv)) != hipSuccess || (e = pre.reserve(nv)) != hipSuccess || (e = deg.reserve(nv)) != hipSuccess ||
        (e = boundary.reserve(nv)) != hipSuccess || (e = blk_tot.reserve(vblk)) != hipSuccess ||
        (e = off.reserve((size_t)vblk + 1)) != hipSuccess || (e = tri.reserve(nt * 3)) != hipSuccess ||
        (e = nbr.reserve(nt * 6)) != hipSuccess) {
      (void)hipGetLastError();
      return e;
    }
    const SmoothArgs a = args(s);
    if ((e = hipMemsetAsync(inc, 0, nv * sizeof(unsigned), nullptr)) != hipSuccess) return e;
    if ((e = timer.run(0, [&] { k_smooth_count<<<tblk, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
    if ((e = timer.run(1, [&] { k_smooth_offsets<<<vblk, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
    const unsigned* tot = blk_tot;
    unsigned long long* o = off;
    if ((e = timer.run(2, [&] { k_tsdf_scan<<<1, kFusionBlock, 0, nullptr>>>(tot, o, vblk); })) != hipSuccess) return e;
    if ((e = timer.run(3, [&] { k_smooth_fill<<<tblk, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
    if ((e = timer.run(4, [&] { k_smooth_lists<<<vblk, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
    st.made(st.adj, s.id, source);
    return hipSuccess;
  }

  // (the adjacency, unless the handle holds it for this mesh) -> the steps, from the source into pos[0], then between pos[0]
  // and pos[1] -> (normals).  Every buffer is there before the first step; nothing is read back.
  hipError_t run(MeshStamps& st, const MeshView& s, int source, int iterations, double lambda, double mu, bool pin, bool normals) {
    hipError_t e;
    if ((e = timer.create()) != hipSuccess) return e;
    st.begin(st.smooth);
    if (s.n_tri > 0) {
      const size_t nv = (size_t)s.n_vert;
      const unsigned vblk = fusion_blocks(s.n_vert);
      const int steps = mu != 0.0 ? 2 * iterations : iterations;
      if ((e = pos[0].reserve(nv * 3)) != hipSuccess || (steps > 1 && (e = pos[1].reserve(nv * 3)) != hipSuccess) ||
          (normals && (e = normal.reserve(nv * 3)) != hipSuccess)) {
        (void)hipGetLastError();
        return e;
      }
      if (!st.adj.made_from(s.id) && (e = adjacency(st, s, source)) != hipSuccess) return e;
      SmoothArgs a = args(s);
      a.pin = pin ? 1 : 0;
      for (int k = 0; k < steps; ++k) {
        a.src = k == 0 ? s.xyz : (const double*)pos[(k - 1) & 1];
        a.dst = pos[k & 1];
        a.f = (mu != 0.0 && (k & 1)) ? mu : lambda;
        if ((e = timer.run(5, [&] { k_smooth_step<<<vblk, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
      }
      last = (steps - 1) & 1;
      if (normals) {
        a.src = pos[last];
        a.normal = normal;
        if ((e = timer.run(6, [&] { k_smooth_normals<<<vblk, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
      }
    }
    has_normals = normals;
    st.made(st.smooth, s.id, source);
    return hipSuccess;
  }
};
#endif  // EKF_KERNELS_ONLY

}  // namespace ekf
