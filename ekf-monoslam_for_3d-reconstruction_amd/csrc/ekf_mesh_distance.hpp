// A mesh-to-mesh distance for the indexed meshes of the fusion handle: for every query point the nearest point on a target
// mesh.  The reference has no counterpart; the contract is pinned here and restated in numpy, twice, by
// tests/distance_oracle.py.  All arithmetic is fp64, every operation rounded once, in the written order, contraction off.
//   1. The target is a mesh (X, F): the welded, the pruned, the smoothed or the simplified mesh (sources 0..3, §29's rules) or
//      a mesh of the feature's own (source 4, ekf_distance_set_mesh).  A triangle t = (i0, i1, i2) with the corners A, B, C is
//      valid iff its indices are distinct, its nine coordinates are finite and, with u = B - A, v = C - A,
//      n = (u1 v2 - u2 v1, u2 v0 - u0 v2, u0 v1 - u1 v0), nn = (n0 n0 + n1 n1) + n2 n2 is finite and > 0.  Invalid triangles
//      take no part; a target without a valid triangle is an error.
//   2. Point to triangle (dist_closest, the one function): Ericson, Real-Time Collision Detection, §5.1.5, the six region
//      tests in the book's order; dot(a, b) = (a0 b0 + a1 b1) + a2 b2 and ab = B - A, ac = C - A, ap = p - A:
//        d1 = dot(ab, ap), d2 = dot(ac, ap);                        d1 <= 0 and d2 <= 0:             c = A
//        bp = p - B, d3 = dot(ab, bp), d4 = dot(ac, bp);            d3 >= 0 and d4 <= d3:            c = B
//        vc = d1 d4 - d3 d2;   vc <= 0 and d1 >= 0 and d3 <= 0:     v = d1 / (d1 - d3),              c = A + v ab
//        cp = p - C, d5 = dot(ab, cp), d6 = dot(ac, cp);            d6 >= 0 and d5 <= d6:            c = C
//        vb = d5 d2 - d1 d6;   vb <= 0 and d2 >= 0 and d6 <= 0:     w = d2 / (d2 - d6),              c = A + w ac
//        va = d3 d6 - d5 d4, e = d4 - d3, f = d5 - d6;  va <= 0 and e >= 0 and f >= 0:  w = e / (e + f),  c = B + w (C - B)
//        otherwise s = (va + vb) + vc, v = vb / s, w = vc / s,                           c = (A + v ab) + w ac
//      (each component of c: one product and one sum, two of each in the last line).  Then every component of c is clamped
//      to the triangle's own box, lo_k = min(A_k, B_k, C_k), hi_k = max(A_k, B_k, C_k), c_k = c_k < lo_k ? lo_k : (c_k > hi_k ?
//      hi_k : c_k), by comparisons (a NaN stays and never wins): a no-op but for an ulp on an edge and for slivers whose v and
//      w rounding has carried away, and what makes the grid's bound below provable.
//      q = p - c, d2 = (q0 q0 + q1 q1) + q2 q2.
//   3. The result for a finite p: over all valid triangles the least (d2, t): t replaces the best iff d2 < best, or
//      d2 == best and t < best_t, from (+inf, 0xffffffff); a d2 that is NaN never wins.  dist = sqrt(d2), tri = t,
//      closest = the winner's c, side = the sign of (q0 n0 + q1 n1) + q2 n2 (+1, -1, or 0 for zero or NaN) with the winner's n:
//      +1 is the free-space side of a weld.  A p with a coordinate that is not finite (or no winner at all) gets dist = NaN,
//      tri = 0xffffffff, closest = NaN, side = 0.
//   4. The queries are the vertices of a source 0..4, or n points from the host.
//   5. Statistics for a threshold thr >= 0: a point is bad iff its dist is NaN; n_bad counts them, n the others; max and its
//      least index; within = #{dist <= thr}; sum of dist and sum2 of dist dist, a bad point giving 0, in a fixed order: per
//      block of 256 consecutive points the tree for s = 128 .. 1: v[l] += v[l + s]; the block partials go to one workgroup
//      whose lane l adds the partials l, l + 256, .. in ascending order from 0.0, then the same tree.  mean = sum / n,
//      rms = sqrt(sum2 / n).
//
// The grid only prunes; the result is the same at every setting.  The box [lo, hi] of the valid triangles' vertices is a
// minimum and a maximum (exact) by a tree in LDS and a second launch: no floating-point atomic.  Axis a has G_a cells of
// h_a = (hi_a - lo_a) / G_a, and cell_a(x) = clamp(floor((x - lo_a) / h_a), 0, G_a - 1) (a NaN goes to 0), a non-decreasing
// function of x, the same for triangles and points.  A valid triangle is filed in every cell of the cell range of its own
// box: counted with integer adds, offsets by a block scan and §16's k_tsdf_scan, filled through cursors; one total is read
// back.  The lists are not ordered: a lexicographic minimum does not depend on the order.
//
// The search of a point p (k_dist_query, one lane a point): p' = p clamped to the box, c = cell(p'), and the Chebyshev shells
// r = 0, 1, .. of cells round c, clipped to the grid.  After shell r the block K_r = prod_a [c_a - r, c_a + r] has been seen.
// If K_r covers the grid the search ends.  Otherwise, for every axis a, g+ = (lo_a + (double)(c_a + r + 1) h_a) - p'_a if
// c_a + r < G_a - 1 and g- = p'_a - (lo_a + (double)(c_a - r) h_a) if c_a - r > 0 (the faces of K_r that do not lie on the
// grid's boundary), m = the least of them, slack = 2^-40 max(|lo_a|, |hi_a|, |p_a|), lb = m - slack, and the search ends iff
// lb >= slack and best_d2 < lb lb: strictly, so that an unseen triangle at an equal d2 with a lower index still wins.
//
// Proof that no triangle T whose computed (d2, t) is less than the best remains unseen.  u = 2^-53, M = max(|lo_a|, |hi_a|).
//   (a) T was filed in the cells prod_a [cell_a(min_a T), cell_a(max_a T)].  Unseen, that product misses K_r, so for one axis a
//       either cell_a(min_a T) >= k + 1 with k = c_a + r, or cell_a(max_a T) <= k - 1 with k = c_a - r; in the first case
//       k + 1 <= G_a - 1 and in the second k >= 1: the face is one of those m was taken over.
//   (b) Step 2's clamp puts the computed c inside T's box, exactly, so c_a >= min_a T in the first case.  cell_a is
//       non-decreasing, so cell_a(c_a) >= k + 1 (a value clamped to G_a - 1 was no smaller before): fl(fl(c_a - lo_a) / h_a)
//       >= k + 1, hence (c_a - lo_a)(1 + u)^2 >= (k + 1) h_a and c_a >= lo_a + (k + 1) h_a - 3 u (k + 1) h_a.  (k + 1) h_a <=
//       (hi_a - lo_a)(1 + 2u) <= 2.01 M, and the face coordinate as computed, fl(lo_a + fl((k + 1) h_a)), is within
//       u 2.01 M + u 3.01 M of the exact one: c_a >= face - 12 u M.  The second case mirrors it.
//   (c) T's box lies in [lo, hi], so clamping to [lo, hi] fixes c, and clamping is non-expansive: |p - c| >= |p' - c| >=
//       c_a - p'_a >= g - u |g| - 12 u M >= m - 15 u M, g the computed gap of that face (|g| <= 2.01 M) and m <= g.
//   (d) d2 as computed is at least |p - c|^2 (1 - u)^5: three roundings on the way to each square, two sums.  No square
//       that matters is subnormal: lb >= slack >= 2^-440 (the host uses one cell unless 2^-400 <= M <= 2^400, and a lane
//       never ends early for a p beyond 2^400), one |q_k| is >= lb / sqrt(3), and a subnormal square of another is below
//       2^-1022, which is 2^-140 of the sum.  So d2 >= (m - 15 u M)^2 (1 - 6u) whenever m >= 15 u M.
//   (e) lb = fl(m - slack) <= m - slack + u 2.01 M and slack >= 8192 u M, so lb <= m - 8189 u M, and fl(lb lb) <=
//       lb^2 (1 + u) < (m - 15 u M)^2 (1 - 6u): (m - 8189 u M)(1 + u) < (m - 15 u M)(1 - 4u) because m <= 2.01 M.
//   So best_d2 < fl(lb lb) <= d2(T): T could not have replaced the best, not even on a tie.  Slack is 2^-40 M where 24 u M
//   would do: the factor 340 is the margin, and it rests on nothing measured.
//
// The launches, 256 lanes a workgroup, on the default stream (T triangles, C cells, N points):
//   k_dist_box      ceil(T / 256)   one lane a triangle: its validity; the workgroup's box and count of valid triangles by a tree
//   k_dist_grid     1               lane l folds the partials l, l + 256, .., then the tree: lo, hi and n_valid.  Read back (56 B);
//                                   the host chooses G_a and h_a
//                   (hipMemsetAsync: counts and cursors = 0)
//   k_dist_count    ceil(T / 256)   one lane a triangle: the cells of its range gain 1
//   k_dist_offsets  ceil(C / 256)   one lane a cell: the in-block exclusive scan and the block's total
//   k_tsdf_scan     1               ekf_fusion.hpp's, unchanged.  The total is read back; 2^32 entries or more is an error
//   k_dist_fill     ceil(T / 256)   one lane a triangle: a slot in each of its cells through the cell's cursor
//   k_dist_query    ceil(N / 256)   one lane a point: the search, then step 3's outputs from the winner through dist_closest again
//   k_dist_stats    ceil(N / 256)   (ekf_distance_get_stats) step 5's block partials
//   k_dist_reduce   1               and their fold
// The only atomics are relaxed, agent-scope integer adds (counts, cursors).  No kernel uses scratch memory, spills or has a
// per-lane array; no workgroup waits for another.  LDS: k_dist_box 3 KiB, k_dist_grid 3 KiB, k_dist_offsets 2 KiB, k_tsdf_scan
// 2 KiB, k_dist_stats 6 KiB, k_dist_reduce 6 KiB, the others none.  Device memory, grow-only: 52 B a triangle block, 12 B a cell,
// 4 B an entry, 37 B a point of outputs, 36 B a point block, and the rows of source 4 and of the host's points.
#pragma once
#include "ekf_mesh_raster.hpp"

namespace ekf {

// k_dist_box, k_dist_grid, k_dist_count, k_dist_offsets, k_tsdf_scan, k_dist_fill, k_dist_query, k_dist_stats, k_dist_reduce
constexpr int kDistKinds = 9;
constexpr unsigned kDistMaxG = 128, kDistNoTri = 0xffffffffu;
constexpr double kDistHuge = 1.7976931348623157e308;
constexpr double kDistSlack = 9.094947017729282e-13;      // 2^-40
constexpr double kDistMagLo = 3.872591914849318e-121;     // 2^-400
constexpr double kDistMagHi = 2.5822498780869086e120;     // 2^400

struct DistGrid {
  double lo[3], hi[3], h[3];
  int G[3];
  double mag;                         // max(|lo_a|, |hi_a|)
};

struct DistSums {                     // k_dist_reduce's result
  double sum, sum2, max;
  unsigned argmax, within, bad, pad;
};

struct DistArgs {
  const double* xyz;                  // the target's rows
  const unsigned* faces;
  unsigned n_tri, tblk;
  const double* pts;                  // the query points
  unsigned n_pts, pblk;
  DistGrid g;
  unsigned ncell;
  double* part;                       // tblk x 6: a triangle block's lo, hi
  unsigned* part_n;                   // tblk: its valid triangles
  double* head;                       // 7: lo, hi, n_valid
  unsigned* cnt;                      // ncell: the entries of a cell
  unsigned* cur;                      // ncell: k_dist_fill's cursors
  unsigned* pre;                      // ncell: the in-block exclusive scan of cnt
  unsigned* tot;                      // cblk: the block totals
  const unsigned long long* off;      // cblk + 1: their exclusive scan (k_tsdf_scan): first(c) = off[c / 256] + pre[c]
  unsigned* list;                     // the entries
  double* dist;                       // the outputs: n_pts
  unsigned* tri;
  double* closest;                    //   x 3
  signed char* side;
  double thr;                         // the statistics
  double* s_part;                     // pblk x 3: sum, sum2, max
  unsigned* s_ipart;                  // pblk x 3: argmax, within, bad
  DistSums* sums;
};

__device__ __forceinline__ bool dist_finite(double x) { return fabs(x) <= kDistHuge; }

__device__ __forceinline__ double dist_dot(double a0, double a1, double a2, double b0, double b1, double b2) {
#pragma clang fp contract(off)
  return (a0 * b0 + a1 * b1) + a2 * b2;
}

// A triangle's corners.
struct DistTri {
  unsigned i0, i1, i2;
  double a0, a1, a2, b0, b1, b2, c0, c1, c2;
};

__device__ __forceinline__ void dist_load(const double* xyz, const unsigned* faces, unsigned t, DistTri& T) {
  T.i0 = faces[(size_t)t * 3];
  T.i1 = faces[(size_t)t * 3 + 1];
  T.i2 = faces[(size_t)t * 3 + 2];
  const double* A = xyz + (size_t)T.i0 * 3;
  const double* B = xyz + (size_t)T.i1 * 3;
  const double* C = xyz + (size_t)T.i2 * 3;
  T.a0 = A[0]; T.a1 = A[1]; T.a2 = A[2];
  T.b0 = B[0]; T.b1 = B[1]; T.b2 = B[2];
  T.c0 = C[0]; T.c1 = C[1]; T.c2 = C[2];
}

// Step 1's normal n = (B - A) x (C - A).
__device__ __forceinline__ void dist_normal(const DistTri& T, double& n0, double& n1, double& n2) {
#pragma clang fp contract(off)
  const double u0 = T.b0 - T.a0, u1 = T.b1 - T.a1, u2 = T.b2 - T.a2;
  const double v0 = T.c0 - T.a0, v1 = T.c1 - T.a1, v2 = T.c2 - T.a2;
  n0 = u1 * v2 - u2 * v1;
  n1 = u2 * v0 - u0 * v2;
  n2 = u0 * v1 - u1 * v0;
}

// Step 1's validity.
__device__ __forceinline__ bool dist_valid(const DistTri& T) {
#pragma clang fp contract(off)
  if (T.i0 == T.i1 || T.i1 == T.i2 || T.i0 == T.i2) return false;
  if (!(dist_finite(T.a0) && dist_finite(T.a1) && dist_finite(T.a2) && dist_finite(T.b0) && dist_finite(T.b1) && dist_finite(T.b2) &&
        dist_finite(T.c0) && dist_finite(T.c1) && dist_finite(T.c2)))
    return false;
  double n0, n1, n2;
  dist_normal(T, n0, n1, n2);
  const double nn = (n0 * n0 + n1 * n1) + n2 * n2;
  return nn > 0.0 && nn <= kDistHuge;
}

// x clamped to [min(a, b, c), max(a, b, c)], by comparisons alone: the first of equal values stays (a zero keeps its sign) and a
// NaN stays a NaN, which then never wins.
__device__ __forceinline__ double dist_clamp(double x, double a, double b, double c) {
  double lo = a, hi = a;
  if (b < lo) lo = b;
  if (c < lo) lo = c;
  if (b > hi) hi = b;
  if (c > hi) hi = c;
  return x < lo ? lo : (x > hi ? hi : x);
}

// Step 2: the closest point of the triangle to p, and d2.  The one function of every kernel and of the host check.
__device__ __forceinline__ double dist_closest(const DistTri& T, double p0, double p1, double p2, double& q0, double& q1, double& q2) {
#pragma clang fp contract(off)
  const double ab0 = T.b0 - T.a0, ab1 = T.b1 - T.a1, ab2 = T.b2 - T.a2;
  const double ac0 = T.c0 - T.a0, ac1 = T.c1 - T.a1, ac2 = T.c2 - T.a2;
  const double ap0 = p0 - T.a0, ap1 = p1 - T.a1, ap2 = p2 - T.a2;
  const double d1 = dist_dot(ab0, ab1, ab2, ap0, ap1, ap2), d2 = dist_dot(ac0, ac1, ac2, ap0, ap1, ap2);
  const double bp0 = p0 - T.b0, bp1 = p1 - T.b1, bp2 = p2 - T.b2;
  const double d3 = dist_dot(ab0, ab1, ab2, bp0, bp1, bp2), d4 = dist_dot(ac0, ac1, ac2, bp0, bp1, bp2);
  const double cp0 = p0 - T.c0, cp1 = p1 - T.c1, cp2 = p2 - T.c2;
  const double d5 = dist_dot(ab0, ab1, ab2, cp0, cp1, cp2), d6 = dist_dot(ac0, ac1, ac2, cp0, cp1, cp2);
  const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  const double e = d4 - d3, f = d5 - d6;
  if (d1 <= 0.0 && d2 <= 0.0) {
    q0 = T.a0; q1 = T.a1; q2 = T.a2;
  } else if (d3 >= 0.0 && d4 <= d3) {
    q0 = T.b0; q1 = T.b1; q2 = T.b2;
  } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
    const double v = d1 / (d1 - d3);
    q0 = T.a0 + v * ab0; q1 = T.a1 + v * ab1; q2 = T.a2 + v * ab2;
  } else if (d6 >= 0.0 && d5 <= d6) {
    q0 = T.c0; q1 = T.c1; q2 = T.c2;
  } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
    const double w = d2 / (d2 - d6);
    q0 = T.a0 + w * ac0; q1 = T.a1 + w * ac1; q2 = T.a2 + w * ac2;
  } else if (va <= 0.0 && e >= 0.0 && f >= 0.0) {
    const double w = e / (e + f);
    q0 = T.b0 + w * (T.c0 - T.b0); q1 = T.b1 + w * (T.c1 - T.b1); q2 = T.b2 + w * (T.c2 - T.b2);
  } else {
    const double s = (va + vb) + vc;
    const double v = vb / s, w = vc / s;
    q0 = (T.a0 + v * ab0) + w * ac0; q1 = (T.a1 + v * ab1) + w * ac1; q2 = (T.a2 + v * ab2) + w * ac2;
  }
  q0 = dist_clamp(q0, T.a0, T.b0, T.c0);
  q1 = dist_clamp(q1, T.a1, T.b1, T.c1);
  q2 = dist_clamp(q2, T.a2, T.b2, T.c2);
  const double r0 = p0 - q0, r1 = p1 - q1, r2 = p2 - q2;
  return (r0 * r0 + r1 * r1) + r2 * r2;
}

// The cell of a coordinate along axis k: non-decreasing in x; a NaN (0 / 0 on an axis of no extent) goes to cell 0.
__device__ __forceinline__ int dist_cell(const DistGrid& g, int k, double x) {
#pragma clang fp contract(off)
  const double q = floor((x - g.lo[k]) / g.h[k]);
  const int top = g.G[k] - 1;
  return q >= (double)top ? top : (q > 0.0 ? (int)q : 0);
}

// The cell range of a valid triangle's own box.
struct DistRange { int x0, x1, y0, y1, z0, z1; };
__device__ __forceinline__ DistRange dist_range(const DistGrid& g, const DistTri& T) {
  DistRange r;
  r.x0 = dist_cell(g, 0, fmin(fmin(T.a0, T.b0), T.c0)); r.x1 = dist_cell(g, 0, fmax(fmax(T.a0, T.b0), T.c0));
  r.y0 = dist_cell(g, 1, fmin(fmin(T.a1, T.b1), T.c1)); r.y1 = dist_cell(g, 1, fmax(fmax(T.a1, T.b1), T.c1));
  r.z0 = dist_cell(g, 2, fmin(fmin(T.a2, T.b2), T.c2)); r.z1 = dist_cell(g, 2, fmax(fmax(T.a2, T.b2), T.c2));
  return r;
}

// One lane a triangle: the workgroup's box of the valid triangles' corners and their number.  The minimum and the maximum
// are exact, so the order of the tree costs no bit.
__global__ void __launch_bounds__(256) k_dist_box(DistArgs a) {
  __shared__ double s_v[kFusionBlock];
  __shared__ unsigned s_n[kFusionBlock];
  const unsigned tid = threadIdx.x, t = blockIdx.x * (unsigned)kFusionBlock + tid;
  DistTri T{};
  bool ok = false;
  if (t < a.n_tri) {
    dist_load(a.xyz, a.faces, t, T);
    ok = dist_valid(T);
  }
  const double inf = __builtin_huge_val();
  s_n[tid] = ok ? 1u : 0u;
  __syncthreads();
  for (unsigned h = kFusionBlock / 2; h > 0; h >>= 1) {
    if (tid < h) s_n[tid] += s_n[tid + h];
    __syncthreads();
  }
  if (tid == 0) a.part_n[blockIdx.x] = s_n[0];
  for (int k = 0; k < 6; ++k) {
    const int ax = k % 3;
    const double x = ax == 0 ? T.a0 : (ax == 1 ? T.a1 : T.a2), y = ax == 0 ? T.b0 : (ax == 1 ? T.b1 : T.b2),
                 z = ax == 0 ? T.c0 : (ax == 1 ? T.c1 : T.c2);
    __syncthreads();
    s_v[tid] = k < 3 ? (ok ? fmin(fmin(x, y), z) : inf) : (ok ? fmax(fmax(x, y), z) : -inf);
    __syncthreads();
    for (unsigned h = kFusionBlock / 2; h > 0; h >>= 1) {
      if (tid < h) s_v[tid] = k < 3 ? fmin(s_v[tid], s_v[tid + h]) : fmax(s_v[tid], s_v[tid + h]);
      __syncthreads();
    }
    if (tid == 0) a.part[(size_t)blockIdx.x * 6 + k] = s_v[0];
  }
}

// One workgroup: the fold of the block partials.  head = lo, hi and the number of valid triangles (below 2^32: exact).
__global__ void __launch_bounds__(256) k_dist_grid(DistArgs a) {
  __shared__ double s_v[kFusionBlock];
  __shared__ unsigned s_n[kFusionBlock];
  const unsigned tid = threadIdx.x;
  const double inf = __builtin_huge_val();
  unsigned n = 0;
  for (unsigned b = tid; b < a.tblk; b += (unsigned)kFusionBlock) n += a.part_n[b];
  s_n[tid] = n;
  __syncthreads();
  for (unsigned h = kFusionBlock / 2; h > 0; h >>= 1) {
    if (tid < h) s_n[tid] += s_n[tid + h];
    __syncthreads();
  }
  if (tid == 0) a.head[6] = (double)s_n[0];
  for (int k = 0; k < 6; ++k) {
    double v = k < 3 ? inf : -inf;
    for (unsigned b = tid; b < a.tblk; b += (unsigned)kFusionBlock) v = k < 3 ? fmin(v, a.part[(size_t)b * 6 + k]) : fmax(v, a.part[(size_t)b * 6 + k]);
    __syncthreads();
    s_v[tid] = v;
    __syncthreads();
    for (unsigned h = kFusionBlock / 2; h > 0; h >>= 1) {
      if (tid < h) s_v[tid] = k < 3 ? fmin(s_v[tid], s_v[tid + h]) : fmax(s_v[tid], s_v[tid + h]);
      __syncthreads();
    }
    if (tid == 0) a.head[k] = s_v[0];
  }
}

// One lane a triangle: every cell of its range gains 1.  Unsigned sums are exact in any order.  A cell index is below ncell:
// dist_cell clamps to the grid.
__global__ void __launch_bounds__(256) k_dist_count(DistArgs a) {
  const unsigned t = blockIdx.x * (unsigned)kFusionBlock + threadIdx.x;
  if (t >= a.n_tri) return;
  DistTri T;
  dist_load(a.xyz, a.faces, t, T);
  if (!dist_valid(T)) return;
  const DistRange r = dist_range(a.g, T);
  for (int z = r.z0; z <= r.z1; ++z)
    for (int y = r.y0; y <= r.y1; ++y)
      for (int x = r.x0; x <= r.x1; ++x) seg_global_add(&a.cnt[(unsigned)((z * a.g.G[1] + y) * a.g.G[0] + x)], 1u);
}

// One lane a cell: the in-block exclusive scan of cnt to pre and the block's total.
__global__ void __launch_bounds__(256) k_dist_offsets(DistArgs a) {
  __shared__ unsigned s_p[2][kFusionBlock];
  const unsigned tid = threadIdx.x, c = blockIdx.x * (unsigned)kFusionBlock + tid;
  const unsigned mine = c < a.ncell ? a.cnt[c] : 0u;
  unsigned total;
  const unsigned incl = comp_scan(s_p, tid, mine, total);
  if (c < a.ncell) a.pre[c] = incl - mine;
  if (tid == 0) a.tot[blockIdx.x] = total;
}

// One lane a triangle: the next free slot of each of its cells.  The slot depends on the order of arrival and nothing that
// reads the list depends on the slot.  A cursor stays below cnt, which counted exactly these entries with the same dist_range,
// so the slot lies inside the cell's segment and below the total the host sized the list by.
__global__ void __launch_bounds__(256) k_dist_fill(DistArgs a) {
  const unsigned t = blockIdx.x * (unsigned)kFusionBlock + threadIdx.x;
  if (t >= a.n_tri) return;
  DistTri T;
  dist_load(a.xyz, a.faces, t, T);
  if (!dist_valid(T)) return;
  const DistRange r = dist_range(a.g, T);
  for (int z = r.z0; z <= r.z1; ++z)
    for (int y = r.y0; y <= r.y1; ++y)
      for (int x = r.x0; x <= r.x1; ++x) {
        const unsigned c = (unsigned)((z * a.g.G[1] + y) * a.g.G[0] + x);
        a.list[a.off[c >> 8] + (unsigned long long)(a.pre[c] + seg_global_add(&a.cur[c], 1u))] = t;
      }
}

// The triangles of one cell against the best so far.
__device__ __forceinline__ void dist_visit(const DistArgs& a, int x, int y, int z, double p0, double p1, double p2, double& best, unsigned& bt) {
  const unsigned c = (unsigned)((z * a.g.G[1] + y) * a.g.G[0] + x);
  const unsigned n = a.cnt[c];
  const unsigned* l = a.list + (a.off[c >> 8] + (unsigned long long)a.pre[c]);
  for (unsigned j = 0; j < n; ++j) {
    const unsigned t = l[j];
    DistTri T;
    dist_load(a.xyz, a.faces, t, T);
    double q0, q1, q2;
    const double d2 = dist_closest(T, p0, p1, p2, q0, q1, q2);
    if (d2 < best || (d2 == best && t < bt)) {
      best = d2;
      bt = t;
    }
  }
}

// One lane a point: the search over the shells, then the outputs from the winner.
__global__ void __launch_bounds__(256) k_dist_query(DistArgs a) {
#pragma clang fp contract(off)
  const unsigned i = blockIdx.x * (unsigned)kFusionBlock + threadIdx.x;
  if (i >= a.n_pts) return;
  const double p0 = a.pts[(size_t)i * 3], p1 = a.pts[(size_t)i * 3 + 1], p2 = a.pts[(size_t)i * 3 + 2];
  const double nan = __builtin_nan("");
  double best = __builtin_huge_val();
  unsigned bt = kDistNoTri;
  if (dist_finite(p0) && dist_finite(p1) && dist_finite(p2)) {
    const DistGrid& g = a.g;
    const double c0 = fmin(fmax(p0, g.lo[0]), g.hi[0]), c1 = fmin(fmax(p1, g.lo[1]), g.hi[1]), c2 = fmin(fmax(p2, g.lo[2]), g.hi[2]);
    const int cx = dist_cell(g, 0, c0), cy = dist_cell(g, 1, c1), cz = dist_cell(g, 2, c2);
    const double mag = fmax(fmax(g.mag, fabs(p0)), fmax(fabs(p1), fabs(p2)));
    const double slack = kDistSlack * mag;
    const bool may_stop = mag <= kDistMagHi;
    for (int r = 0;; ++r) {
      const int x0 = max(cx - r, 0), x1 = min(cx + r, g.G[0] - 1), y0 = max(cy - r, 0), y1 = min(cy + r, g.G[1] - 1);
      const int z0 = max(cz - r, 0), z1 = min(cz + r, g.G[2] - 1);
      for (int z = z0; z <= z1; ++z)
        for (int y = y0; y <= y1; ++y) {
          if (z - cz == r || cz - z == r || y - cy == r || cy - y == r) {
            for (int x = x0; x <= x1; ++x) dist_visit(a, x, y, z, p0, p1, p2, best, bt);
          } else {                                                           // (r > 0 here: at r = 0 the test above holds)
            if (cx - r >= 0) dist_visit(a, cx - r, y, z, p0, p1, p2, best, bt);
            if (cx + r <= g.G[0] - 1) dist_visit(a, cx + r, y, z, p0, p1, p2, best, bt);
          }
        }
      if (cx - r <= 0 && cx + r >= g.G[0] - 1 && cy - r <= 0 && cy + r >= g.G[1] - 1 && cz - r <= 0 && cz + r >= g.G[2] - 1) break;
      double m = __builtin_huge_val();
      if (cx + r < g.G[0] - 1) m = fmin(m, (g.lo[0] + (double)(cx + r + 1) * g.h[0]) - c0);
      if (cx - r > 0) m = fmin(m, c0 - (g.lo[0] + (double)(cx - r) * g.h[0]));
      if (cy + r < g.G[1] - 1) m = fmin(m, (g.lo[1] + (double)(cy + r + 1) * g.h[1]) - c1);
      if (cy - r > 0) m = fmin(m, c1 - (g.lo[1] + (double)(cy - r) * g.h[1]));
      if (cz + r < g.G[2] - 1) m = fmin(m, (g.lo[2] + (double)(cz + r + 1) * g.h[2]) - c2);
      if (cz - r > 0) m = fmin(m, c2 - (g.lo[2] + (double)(cz - r) * g.h[2]));
      const double lb = m - slack;
      if (may_stop && lb >= slack && best < lb * lb) break;
    }
  }
  double dist = nan, q0 = nan, q1 = nan, q2 = nan;
  signed char side = 0;
  if (bt != kDistNoTri) {
    DistTri T;
    dist_load(a.xyz, a.faces, bt, T);
    dist = sqrt(dist_closest(T, p0, p1, p2, q0, q1, q2));
    double n0, n1, n2;
    dist_normal(T, n0, n1, n2);
    const double s = dist_dot(p0 - q0, p1 - q1, p2 - q2, n0, n1, n2);
    side = s > 0.0 ? 1 : (s < 0.0 ? -1 : 0);
  }
  a.dist[i] = dist;
  a.tri[i] = bt;
  a.closest[(size_t)i * 3] = q0;
  a.closest[(size_t)i * 3 + 1] = q1;
  a.closest[(size_t)i * 3 + 2] = q2;
  a.side[i] = side;
}

// The larger of two (value, index) pairs, the lower index among equal values.
__device__ __forceinline__ void dist_max(double& v, unsigned& i, double w, unsigned j) {
  if (w > v || (w == v && j < i)) {
    v = w;
    i = j;
  }
}

// The trees of step 5 over the workgroup's 256 values: sums by v[l] += v[l + s], the maximum with its least index, the counts.
// Lane 0 holds the results afterwards.
__device__ __forceinline__ void dist_trees(double (*s_d)[kFusionBlock], unsigned (*s_u)[kFusionBlock], unsigned tid, double& sum, double& sum2,
                                           double& mx, unsigned& arg, unsigned& within, unsigned& bad) {
#pragma clang fp contract(off)
  s_d[0][tid] = sum; s_d[1][tid] = sum2; s_u[0][tid] = within; s_u[1][tid] = bad;
  __syncthreads();
  for (unsigned s = kFusionBlock / 2; s > 0; s >>= 1) {
    if (tid < s) {
      s_d[0][tid] = s_d[0][tid] + s_d[0][tid + s];
      s_d[1][tid] = s_d[1][tid] + s_d[1][tid + s];
      s_u[0][tid] += s_u[0][tid + s];
      s_u[1][tid] += s_u[1][tid + s];
    }
    __syncthreads();
  }
  sum = s_d[0][0]; sum2 = s_d[1][0]; within = s_u[0][0]; bad = s_u[1][0];
  __syncthreads();
  s_d[0][tid] = mx; s_u[0][tid] = arg;
  __syncthreads();
  for (unsigned s = kFusionBlock / 2; s > 0; s >>= 1) {
    if (tid < s) {
      double v = s_d[0][tid];
      unsigned j = s_u[0][tid];
      dist_max(v, j, s_d[0][tid + s], s_u[0][tid + s]);
      s_d[0][tid] = v; s_u[0][tid] = j;
    }
    __syncthreads();
  }
  mx = s_d[0][0]; arg = s_u[0][0];
}

// One lane a point: step 5's block partials.  A bad point and a lane past the last point give 0 to the sums and (-1, no index)
// to the maximum.
__global__ void __launch_bounds__(256) k_dist_stats(DistArgs a) {
#pragma clang fp contract(off)
  __shared__ double s_d[2][kFusionBlock];
  __shared__ unsigned s_u[2][kFusionBlock];
  const unsigned tid = threadIdx.x, i = blockIdx.x * (unsigned)kFusionBlock + tid;
  double sum = 0.0, sum2 = 0.0, mx = -1.0;
  unsigned arg = kDistNoTri, within = 0, bad = 0;
  if (i < a.n_pts) {
    const double d = a.dist[i];
    if (d != d) {
      bad = 1;
    } else {
      sum = d; sum2 = d * d; mx = d; arg = i;
      within = d <= a.thr ? 1u : 0u;
    }
  }
  dist_trees(s_d, s_u, tid, sum, sum2, mx, arg, within, bad);
  if (tid == 0) {
    a.s_part[(size_t)blockIdx.x * 3] = sum; a.s_part[(size_t)blockIdx.x * 3 + 1] = sum2; a.s_part[(size_t)blockIdx.x * 3 + 2] = mx;
    a.s_ipart[(size_t)blockIdx.x * 3] = arg; a.s_ipart[(size_t)blockIdx.x * 3 + 1] = within; a.s_ipart[(size_t)blockIdx.x * 3 + 2] = bad;
  }
}

// One workgroup: lane l adds the partials l, l + 256, .. in ascending order from 0.0, then the same trees.
__global__ void __launch_bounds__(256) k_dist_reduce(DistArgs a) {
#pragma clang fp contract(off)
  __shared__ double s_d[2][kFusionBlock];
  __shared__ unsigned s_u[2][kFusionBlock];
  const unsigned tid = threadIdx.x;
  double sum = 0.0, sum2 = 0.0, mx = -1.0;
  unsigned arg = kDistNoTri, within = 0, bad = 0;
  for (unsigned b = tid; b < a.pblk; b += (unsigned)kFusionBlock) {
    sum = sum + a.s_part[(size_t)b * 3];
    sum2 = sum2 + a.s_part[(size_t)b * 3 + 1];
    dist_max(mx, arg, a.s_part[(size_t)b * 3 + 2], a.s_ipart[(size_t)b * 3]);
    within += a.s_ipart[(size_t)b * 3 + 1];
    bad += a.s_ipart[(size_t)b * 3 + 2];
  }
  dist_trees(s_d, s_u, tid, sum, sum2, mx, arg, within, bad);
  if (tid == 0) {
    DistSums r;
    r.sum = sum; r.sum2 = sum2; r.max = mx; r.argmax = arg; r.within = within; r.bad = bad; r.pad = 0;
    *a.sums = r;
  }
}

// The grid of a box for g cells along its longest axis, the others in proportion, at least 1.  One cell unless the box's
// magnitude is inside the range the proof above covers.
inline DistGrid dist_make_grid(const double* head, unsigned g) {
#pragma clang fp contract(off)
  DistGrid d{};
  double longest = 0.0;
  for (int k = 0; k < 3; ++k) {
    d.lo[k] = head[k];
    d.hi[k] = head[3 + k];
    d.mag = std::max(d.mag, std::max(std::fabs(d.lo[k]), std::fabs(d.hi[k])));
    longest = std::max(longest, d.hi[k] - d.lo[k]);
  }
  if (!(d.mag >= kDistMagLo && d.mag <= kDistMagHi) || !(longest > 0.0)) g = 1;
  for (int k = 0; k < 3; ++k) {
    const double ext = d.hi[k] - d.lo[k];
    const double want = std::ceil((double)g * (ext / longest));
    d.G[k] = want >= (double)g ? (int)g : (want > 1.0 ? (int)want : 1);
    d.h[k] = ext / (double)d.G[k];
  }
  return d;
}

// The automatic g.  The first guess was sqrt(n_valid / 8); on the MI355X the finest grid was the fastest or tied at every
// target measured, and a target of 18 632 triangles ran 24 % slower at the 49 cells of that guess than at 128.
inline unsigned dist_auto_g(double n_valid) {
  const double g = std::ceil(std::sqrt(n_valid / 2.0));
  return g >= (double)kDistMaxG ? kDistMaxG : (g > 1.0 ? (unsigned)g : 1u);
}

#ifndef EKF_KERNELS_ONLY
// Host side: the grid, the outputs and the statistics of the distance, owned by the fusion handle beside its TsdfRaster;
// grow-only.  The sources are only read.  A timer of its own, so that the other getters count what they counted.
struct TsdfDistance {
  CallerMesh own;                                // source 4: the mesh ekf_distance_set_mesh was given
  DevBuf<double> q_xyz;                          // the host's points of the last ekf_distance_run_points
  DevBuf<double> part, head;                     // the scratch of the grid
  DevBuf<unsigned> part_n, cnt, cur, pre, tot, list;
  DevBuf<unsigned long long> off;
  DevBuf<double> dist, closest, s_part;          // the result
  DevBuf<unsigned> tri, s_ipart;
  DevBuf<signed char> side;
  DevBuf<DistSums> sums;
  unsigned long long n_points = 0, entries = 0;
  bool valid = false;
  unsigned grid_g = 0;                           // ekf_distance_set_grid: 0 = automatic
  DistGrid grid{};                               // of the last run
  unsigned ncell = 0;
  KernelTimer<kDistKinds> timer;

  enum Status { kOk = 0, kNoValid = 1, kTooMany = 2 };

  // The host's points into q_xyz: scratch, not part of the result.
  hipError_t set_points(const double* xyz, size_t n) {
    hipError_t e;
    if ((e = q_xyz.reserve(n * 3)) != hipSuccess) {
      (void)hipGetLastError();
      return e;
    }
    return hipMemcpy(q_xyz, xyz, n * 3 * sizeof(double), hipMemcpyHostToDevice);
  }

  template <typename T>
  static hipError_t scratch(DevBuf<T>& b, size_t n) {
    const hipError_t e = b.reserve(n);
    if (e != hipSuccess) (void)hipGetLastError();
    return e;
  }

  // box -> grid -> (read back) -> count -> offsets -> scan -> (read back) -> fill -> query.  The previous result stays
  // readable until the new outputs exist and the fill begins: the scratch is no part of it.
  hipError_t run(const MeshView& t, const double* pts, unsigned long long np, Status* status) {
    hipError_t e;
    *status = kOk;
    if ((e = timer.create()) != hipSuccess) return e;
    DistArgs a{};
    a.xyz = t.xyz; a.faces = t.faces; a.n_tri = (unsigned)t.n_tri; a.tblk = fusion_blocks(t.n_tri);
    a.pts = pts; a.n_pts = (unsigned)np; a.pblk = fusion_blocks(np);
    if ((e = scratch(part, (size_t)a.tblk * 6)) != hipSuccess || (e = scratch(part_n, a.tblk)) != hipSuccess || (e = scratch(head, 7)) != hipSuccess)
      return e;
    a.part = part; a.part_n = part_n; a.head = head;
    if ((e = timer.run(0, [&] { k_dist_box<<<a.tblk, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
    if ((e = timer.run(1, [&] { k_dist_grid<<<1, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
    double h_head[7];
    if ((e = hipMemcpy(h_head, head, sizeof h_head, hipMemcpyDeviceToHost)) != hipSuccess) return e;
    if (!(h_head[6] >= 1.0)) {
      *status = kNoValid;
      return hipSuccess;
    }
    a.g = dist_make_grid(h_head, grid_g ? grid_g : dist_auto_g(h_head[6]));
    a.ncell = (unsigned)a.g.G[0] * (unsigned)a.g.G[1] * (unsigned)a.g.G[2];
    const unsigned cblk = fusion_blocks(a.ncell);
    if ((e = scratch(cnt, a.ncell)) != hipSuccess || (e = scratch(cur, a.ncell)) != hipSuccess || (e = scratch(pre, a.ncell)) != hipSuccess ||
        (e = scratch(tot, cblk)) != hipSuccess || (e = scratch(off, (size_t)cblk + 1)) != hipSuccess)
      return e;
    a.cnt = cnt; a.cur = cur; a.pre = pre; a.tot = tot; a.off = off;
    if ((e = hipMemsetAsync(cnt, 0, (size_t)a.ncell * sizeof(unsigned), nullptr)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(cur, 0, (size_t)a.ncell * sizeof(unsigned), nullptr)) != hipSuccess) return e;
    if ((e = timer.run(2, [&] { k_dist_count<<<a.tblk, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
    if ((e = timer.run(3, [&] { k_dist_offsets<<<cblk, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
    if ((e = timer.run(4, [&] { k_tsdf_scan<<<1, kFusionBlock, 0, nullptr>>>(tot, off, cblk); })) != hipSuccess) return e;
    unsigned long long total = 0;
    if ((e = hipMemcpy(&total, off + cblk, sizeof total, hipMemcpyDeviceToHost)) != hipSuccess) return e;
    if (total >= (1ull << 32)) {
      *status = kTooMany;
      return hipSuccess;
    }
    if ((e = scratch(list, (size_t)total)) != hipSuccess) return e;
    a.list = list;
    if (np > dist.capacity() || np > tri.capacity() || np * 3 > closest.capacity() || np > side.capacity() ||
        (size_t)a.pblk * 3 > s_part.capacity() || (size_t)a.pblk * 3 > s_ipart.capacity() || 1 > sums.capacity()) {
      DevBuf<double> n_dist, n_closest, n_spart;
      DevBuf<unsigned> n_tri, n_sipart;
      DevBuf<signed char> n_side;
      DevBuf<DistSums> n_sums;
      if ((e = n_dist.reserve(std::max<size_t>(np, dist.capacity()))) != hipSuccess || (e = n_tri.reserve(std::max<size_t>(np, tri.capacity()))) != hipSuccess ||
          (e = n_closest.reserve(std::max<size_t>(np * 3, closest.capacity()))) != hipSuccess ||
          (e = n_side.reserve(std::max<size_t>(np, side.capacity()))) != hipSuccess ||
          (e = n_spart.reserve(std::max<size_t>((size_t)a.pblk * 3, s_part.capacity()))) != hipSuccess ||
          (e = n_sipart.reserve(std::max<size_t>((size_t)a.pblk * 3, s_ipart.capacity()))) != hipSuccess || (e = n_sums.reserve(1)) != hipSuccess) {
        (void)hipGetLastError();
        return e;
      }
      dist = std::move(n_dist); tri = std::move(n_tri); closest = std::move(n_closest); side = std::move(n_side);
      s_part = std::move(n_spart); s_ipart = std::move(n_sipart); sums = std::move(n_sums);
    }
    valid = false;
    a.dist = dist; a.tri = tri; a.closest = closest; a.side = side;
    if ((e = timer.run(5, [&] { k_dist_fill<<<a.tblk, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
    if ((e = timer.run(6, [&] { k_dist_query<<<a.pblk, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
    n_points = np; entries = total; grid = a.g; ncell = a.ncell;
    valid = true;
    return hipSuccess;
  }

  // Step 5 of the last run for a threshold.
  hipError_t stats(double thr, DistSums* out) {
    hipError_t e;
    if ((e = timer.create()) != hipSuccess) return e;
    DistArgs a{};
    a.n_pts = (unsigned)n_points; a.pblk = fusion_blocks(n_points);
    a.dist = dist; a.thr = thr; a.s_part = s_part; a.s_ipart = s_ipart; a.sums = sums;
    if ((e = timer.run(7, [&] { k_dist_stats<<<a.pblk, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
    if ((e = timer.run(8, [&] { k_dist_reduce<<<1, kFusionBlock, 0, nullptr>>>(a); })) != hipSuccess) return e;
    return hipMemcpy(out, sums, sizeof(DistSums), hipMemcpyDeviceToHost);
  }
};
#endif  // EKF_KERNELS_ONLY

}  // namespace ekf
