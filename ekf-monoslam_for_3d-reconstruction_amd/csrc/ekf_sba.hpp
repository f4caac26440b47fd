// Sparse bundle adjustment of the key-frame map: the reference's sba_add step.
// fp64 throughout, as in the reference.  Paths are under sparse_bundle_adjustment/.
//
// One LM iteration (SysSBA::doSBA, sba.cpp:1312-1585) is, on one stream:
//   k_sba_point      per point: error, Jacobians and products of every projection (proj.cpp:60-187), Hpp * lam, its
//                    3 x 3 inverse, tp, and T_a = Hpc_a^T Hppi per projection (setupSparseSys, sba.cpp:1163-1290)
//   k_sba_rhs        B per free camera, over its projections in point order
//   k_sba_pairs      the 6 x 6 blocks of A per (a, b) free-camera pair from a host-built (proj_a, proj_b) list
//   k_sba_diag       the lam scaling of A's diagonal (csparse.cpp:279), identity blocks (deviation 1) and padding
//   Cholesky         k_chol_diag_packed_f64 / k_panel_direct_f64 / k_gemm_mfma_f64 (ekf_dense.hpp) via sba_chol_f64
//   k_sba_trsv       x = A^-1 B (one workgroup), k_sba_resid r = B - A x, k_sba_trsv again, k_sba_refine x += dx
//                    (doChol's one step of iterative refinement, csparse.cpp:307-363) and |x|^2
//   k_sba_update_*   camera and point update (skipped on the device when |x|^2 < 1e-16 or the factor failed)
//   k_sba_node_prep  w2n, w2i, dRd* per node;  k_sba_cost / k_sba_cost_final: the cost, two fixed-order passes
// Every sum has one fixed order (no atomics), so a run is bit-reproducible.
// On a PCG handle k_sba_pairs_blk / k_sba_diag_blk assemble 6 x 6 blocks instead of the dense A, and
// k_sba_blk_inv + the k_sba_cg_* kernels (further down) take the place of the Cholesky and the triangular solves.
//
// Robust cost and pruning: every projection carries a `valid` byte beside its keypoint, and the
// error of a valid projection passes through sba_huber (SysSBA::huber, proj.cpp:162-176) wherever it is used.  An
// invalid projection is skipped by k_sba_point, k_sba_update_points and the cost; the host-built lists of k_sba_rhs /
// k_sba_pairs / k_sba_diag hold valid projections only.  Outside the LM loop:
//   k_sba_flag_bad   countBad / removeBad (sba.cpp:416-462): counts, and optionally clears, the valid projections with
//                    e^2 >= dist^2
//   k_sba_stats      calcAvgError and numBadPoints (sba.cpp:365-411)
// both reduced by k_sba_cost_final, in the cost's fixed order.
#pragma once
#include <hip/hip_runtime.h>

namespace ekf {

struct SbaCamera { double fx, fy, cx, cy; };

// Device result block, read back once per LM iteration.  k_sba_cost_final fills (cost, cost_in, n_in) from whichever
// first pass ran: k_sba_cost as named; k_sba_flag_bad (flagged count, 0, 0); k_sba_stats (sum |e|, valid count,
// count of exactly-zero errors).  The counts are whole numbers below 2^53, exact in a double.
struct SbaResult {
  double x2;          // |x|^2 of the refined step
  double cost;        // sum of squared errors (all valid projections)
  double cost_in;     // sum over the projections with e^2 < dist^2
  double n_in;        // their count
  int status;         // 1: a non-positive pivot
  int pad[3];
};

constexpr int kSbaNM = 52;            // per node: w2n (12), w2i (12), dRdx, dRdy, dRdz (27), pad
constexpr int kSbaMaxN = 6144;        // 6 F + padding: k_sba_trsv keeps its vector in LDS (48 KiB)

// Eigen's Quaternion::toRotationMatrix, q = (w, x, y, z)
__device__ __forceinline__ void sba_quat_rot(const double* q, double R[9]) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1 - (tyy + tzz); R[1] = txy - twz;       R[2] = txz + twy;
  R[3] = txy + twz;       R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy;       R[7] = tyz + twx;       R[8] = 1 - (txx + tyy);
}

// transformW2F + setProjection + setDr(true) (node.cpp:96-108): one thread per node
__global__ void __launch_bounds__(256) k_sba_node_prep(const double* __restrict__ nodes, int nn, SbaCamera K,
                                                       double* __restrict__ nm) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nn) return;
  const double* t = nodes + 7 * i;
  double R[9];
  sba_quat_rot(t + 3, R);
  double* o = nm + (size_t)kSbaNM * i;
  double w2n[12];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) w2n[4 * r + c] = R[3 * c + r];                    // R^T
    w2n[4 * r + 3] = -(w2n[4 * r] * t[0] + w2n[4 * r + 1] * t[1] + w2n[4 * r + 2] * t[2]);
  }
  for (int k = 0; k < 12; ++k) o[k] = w2n[k];
  for (int c = 0; c < 4; ++c) {                                                   // K w2n
    o[12 + c] = K.fx * w2n[c] + K.cx * w2n[8 + c];
    o[16 + c] = K.fy * w2n[4 + c] + K.cy * w2n[8 + c];
    o[20 + c] = w2n[8 + c];
  }
  // dRi* R^T with the constant dRi* of node.cpp:18-30 (rows written out; w2n row r = R^T row r)
  const double* a0 = w2n; const double* a1 = w2n + 4; const double* a2 = w2n + 8;
  for (int c = 0; c < 3; ++c) {
    o[24 + c] = 0.0;          o[27 + c] = 2.0 * a2[c];  o[30 + c] = -2.0 * a1[c];     // dRdx
    o[33 + c] = -2.0 * a2[c]; o[36 + c] = 0.0;          o[39 + c] = 2.0 * a0[c];      // dRdy
    o[42 + c] = 2.0 * a1[c];  o[45 + c] = -2.0 * a0[c]; o[48 + c] = 0.0;              // dRdz
  }
}

// calcErrMono_ (proj.cpp:143-187): e = p1.xy / p1.z - kp, or 0 when p1.z <= 0
__device__ __forceinline__ void sba_error(const double* w2i, const double* X, const double* kp, double e[2]) {
  const double p0 = w2i[0] * X[0] + w2i[1] * X[1] + w2i[2] * X[2] + w2i[3];
  const double p1 = w2i[4] * X[0] + w2i[5] * X[1] + w2i[6] * X[2] + w2i[7];
  const double p2 = w2i[8] * X[0] + w2i[9] * X[1] + w2i[10] * X[2] + w2i[11];
  if (p2 <= 0.0) { e[0] = 0.0; e[1] = 0.0; return; }
  e[0] = p0 / p2 - kp[0];
  e[1] = p1 / p2 - kp[1];
}

// The pseudo-Huber weight of calcErrMono_ (proj.cpp:162-176), in its operation order: for huber > 0 and
// e2 = |e|^2 > huber^2, e *= sqrt((2 huber sqrt(e2) - huber^2) / e2).  huber = 0 leaves e alone.  The one place the
// weight lives: the linear system, the cost and the pruning all call it on what sba_error returned.
__device__ __forceinline__ void sba_huber(double huber, double e[2]) {
  if (huber > 0.0) {
    const double b2 = huber * huber;
    const double e2 = e[0] * e[0] + e[1] * e[1];
    if (e2 > b2) {
      const double c = 2.0 * huber * sqrt(e2) - b2;
      const double w = sqrt(c / e2);
      e[0] *= w;
      e[1] *= w;
    }
  }
}

// Per projection record: Hcc (36), Hpc (18, 3 x 6), T (18, Tpc 6 x 3), JcTE (6)
constexpr int kSbaPR = 78;

// setupSparseSys per point (sba.cpp:1190-1251): one thread per point, its projections in node order
__global__ void __launch_bounds__(256) k_sba_point(const double* __restrict__ nm, const double* __restrict__ nodes,
                                                   const double* __restrict__ pts, const int* __restrict__ poff,
                                                   const int* __restrict__ pnode, const double* __restrict__ uv,
                                                   const unsigned char* __restrict__ valid, double huber, int npts,
                                                   SbaCamera K, double lam, double* __restrict__ prj,
                                                   double* __restrict__ tps) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npts) return;
  const int k0 = poff[p], k1 = poff[p + 1];
  if (k1 == k0) return;
  const double X[3] = {pts[3 * p], pts[3 * p + 1], pts[3 * p + 2]};
  double Hpp[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, bp[3] = {0, 0, 0};
  int nv = 0;
  for (int k = k0; k < k1; ++k) {
    if (!valid[k]) continue;
    ++nv;
    const int n = pnode[k];
    const double* m = nm + (size_t)kSbaNM * n;
    const double* w2n = m;
    double e[2];
    sba_error(m + 12, X, uv + 2 * k, e);
    sba_huber(huber, e);                                                  // the Jacobians stay unweighted
    const double px = w2n[0] * X[0] + w2n[1] * X[1] + w2n[2] * X[2] + w2n[3];
    const double py = w2n[4] * X[0] + w2n[5] * X[1] + w2n[6] * X[2] + w2n[7];
    const double pz = w2n[8] * X[0] + w2n[9] * X[1] + w2n[10] * X[2] + w2n[11];
    const double ipz2 = 1.0 / (pz * pz);
    const double ipz2fx = ipz2 * K.fx, ipz2fy = ipz2 * K.fy;
    const double* t = nodes + 7 * n;
    const double pwt[3] = {X[0] - t[0], X[1] - t[1], X[2] - t[2]};
    double jc[2][6], jp[2][3];
    for (int a = 0; a < 3; ++a) {
      const double* D = m + 24 + 9 * a;
      const double d0 = D[0] * pwt[0] + D[1] * pwt[1] + D[2] * pwt[2];
      const double d1 = D[3] * pwt[0] + D[4] * pwt[1] + D[5] * pwt[2];
      const double d2 = D[6] * pwt[0] + D[7] * pwt[1] + D[8] * pwt[2];
      jc[0][3 + a] = (pz * d0 - px * d2) * ipz2fx;
      jc[1][3 + a] = (pz * d1 - py * d2) * ipz2fy;
    }
    for (int a = 0; a < 3; ++a) {
      const double d0 = w2n[a], d1 = w2n[4 + a], d2 = w2n[8 + a];
      jc[0][a] = (pz * -d0 - px * -d2) * ipz2fx;
      jc[1][a] = (pz * -d1 - py * -d2) * ipz2fy;
      jp[0][a] = (pz * d0 - px * d2) * ipz2fx;
      jp[1][a] = (pz * d1 - py * d2) * ipz2fy;
    }
    double* o = prj + (size_t)kSbaPR * k;
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < 6; ++c) o[6 * r + c] = jc[0][r] * jc[0][c] + jc[1][r] * jc[1][c];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 6; ++c) o[36 + 6 * r + c] = jp[0][r] * jc[0][c] + jp[1][r] * jc[1][c];
    for (int r = 0; r < 6; ++r) o[72 + r] = jc[0][r] * e[0] + jc[1][r] * e[1];
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) Hpp[3 * r + c] += jp[0][r] * jp[0][c] + jp[1][r] * jp[1][c];
      bp[r] -= jp[0][r] * e[0] + jp[1][r] * e[1];
    }
  }
  if (nv == 0) return;                                                    // every projection pruned: as a point without any
  Hpp[0] *= lam; Hpp[4] *= lam; Hpp[8] *= lam;
  // Eigen's 3 x 3 cofactor inverse
  double c[9];
  c[0] = Hpp[4] * Hpp[8] - Hpp[5] * Hpp[7]; c[1] = Hpp[2] * Hpp[7] - Hpp[1] * Hpp[8]; c[2] = Hpp[1] * Hpp[5] - Hpp[2] * Hpp[4];
  c[3] = Hpp[5] * Hpp[6] - Hpp[3] * Hpp[8]; c[4] = Hpp[0] * Hpp[8] - Hpp[2] * Hpp[6]; c[5] = Hpp[2] * Hpp[3] - Hpp[0] * Hpp[5];
  c[6] = Hpp[3] * Hpp[7] - Hpp[4] * Hpp[6]; c[7] = Hpp[1] * Hpp[6] - Hpp[0] * Hpp[7]; c[8] = Hpp[0] * Hpp[4] - Hpp[1] * Hpp[3];
  const double det = Hpp[0] * c[0] + Hpp[1] * c[3] + Hpp[2] * c[6];
  double Hi[9];
  for (int q = 0; q < 9; ++q) Hi[q] = c[q] / det;
  double tp[3];
  for (int r = 0; r < 3; ++r) tp[r] = Hi[3 * r] * bp[0] + Hi[3 * r + 1] * bp[1] + Hi[3 * r + 2] * bp[2];
  tps[3 * p] = tp[0]; tps[3 * p + 1] = tp[1]; tps[3 * p + 2] = tp[2];
  for (int k = k0; k < k1; ++k) {
    if (pnode[k] == 0 || !valid[k]) continue;                             // node 0 is fixed
    double* o = prj + (size_t)kSbaPR * k;
    const double* Hpc = o + 36;
    for (int r = 0; r < 6; ++r)
      for (int q = 0; q < 3; ++q)
        o[54 + 3 * r + q] = Hpc[r] * Hi[q] + Hpc[6 + r] * Hi[3 + q] + Hpc[12 + r] * Hi[6 + q];
  }
}

// B_a = -sum (JcTE + Hpc^T tp) over the camera's projections in point order: one thread per (camera, row)
__global__ void __launch_bounds__(256) k_sba_rhs(const int* __restrict__ coff, const int* __restrict__ cprj,
                                                 const int* __restrict__ ppoint, const double* __restrict__ prj,
                                                 const double* __restrict__ tps, int nfree, double* __restrict__ B) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= 6 * nfree) return;
  const int a = g / 6, r = g % 6;
  double b = 0.0;
  for (int i = coff[a]; i < coff[a + 1]; ++i) {
    const int k = cprj[i];
    const double* o = prj + (size_t)kSbaPR * k;
    const double* tp = tps + 3 * ppoint[k];
    b -= o[72 + r];
    b -= o[36 + r] * tp[0] + o[42 + r] * tp[1] + o[48 + r] * tp[2];
  }
  B[g] = b;
}

// A_ab = sum over the pair's (proj_a, proj_b) list in point order of [Hcc if a == b] - T_a Hpc_b.  One workgroup of 64
// per pair, 36 lanes; a diagonal pair computes its upper triangle (as the reference stores it) and mirrors it.
// sba_pair_sum is the sum of lane t = 6 r + c of pair pr, for both destinations below; false: the lane has no entry.
__device__ __forceinline__ bool sba_pair_sum(const int* __restrict__ pair_ab, const int* __restrict__ pair_off,
                                             const int* __restrict__ items, const double* __restrict__ prj, int pr, int t,
                                             int& a, int& b, int& r, int& c, double& acc) {
  if (t >= 36) return false;
  a = pair_ab[2 * pr];
  b = pair_ab[2 * pr + 1];
  r = t / 6;
  c = t % 6;
  const bool diag = (a == b);
  if (diag && r > c) return false;
  acc = 0.0;
  for (int i = pair_off[pr]; i < pair_off[pr + 1]; ++i) {
    const double* oa = prj + (size_t)kSbaPR * items[2 * i];
    const double* ob = prj + (size_t)kSbaPR * items[2 * i + 1];
    if (diag) acc += oa[6 * r + c];
    const double m = oa[54 + 3 * r] * ob[36 + c] + oa[54 + 3 * r + 1] * ob[42 + c] + oa[54 + 3 * r + 2] * ob[48 + c];
    acc += -m;
  }
  return true;
}

// destination 1: the dense A of the Cholesky solver, both triangles
__global__ void __launch_bounds__(64) k_sba_pairs(const int* __restrict__ pair_ab, const int* __restrict__ pair_off,
                                                  const int* __restrict__ items, const double* __restrict__ prj,
                                                  double* __restrict__ A, int lda) {
  int a, b, r, c;
  double acc;
  if (!sba_pair_sum(pair_ab, pair_off, items, prj, blockIdx.x, threadIdx.x, a, b, r, c, acc)) return;
  A[(size_t)(6 * a + r) * lda + 6 * b + c] = acc;
  A[(size_t)(6 * b + c) * lda + 6 * a + r] = acc;
}

// destination 2: the block array of the PCG solver, 36 doubles per slot, row-major.  slot[pr] is the
// node index for a diagonal pair (mirrored, so all 36 entries are written) and nfree + the running number of the
// off-diagonal pair (a < b) otherwise: the block M of block row a, block column b (CSparse::addOffdiagBlock).
__global__ void __launch_bounds__(64) k_sba_pairs_blk(const int* __restrict__ pair_ab, const int* __restrict__ pair_off,
                                                      const int* __restrict__ items, const double* __restrict__ prj,
                                                      const int* __restrict__ slot, double* __restrict__ blk) {
  int a, b, r, c;
  double acc;
  if (!sba_pair_sum(pair_ab, pair_off, items, prj, blockIdx.x, threadIdx.x, a, b, r, c, acc)) return;
  double* o = blk + (size_t)36 * slot[blockIdx.x];
  o[6 * r + c] = acc;
  if (a == b) o[6 * c + r] = acc;
}

// k_sba_diag for the block array: one thread per diagonal element i = 6 a + r of the free nodes
__global__ void __launch_bounds__(256) k_sba_diag_blk(double* __restrict__ blk, int n6, const int* __restrict__ empty,
                                                      double lam) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n6) return;
  const int a = i / 6, r = i % 6;
  double* row = blk + (size_t)36 * a + 6 * r;
  if (empty[a]) {
    for (int c = 0; c < 6; ++c) row[c] = (c == r) ? 1.0 : 0.0;
  } else {
    row[r] = row[r] * lam;
  }
}

// diagonal: *= lam (csparse.cpp:279); identity for a projection-less free node (deviation 1) and for the padding
__global__ void __launch_bounds__(256) k_sba_diag(double* __restrict__ A, int lda, int n6, int npad,
                                                  const int* __restrict__ empty, double lam) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npad) return;
  double* d = A + (size_t)i * lda + i;
  if (i >= n6 || empty[i / 6]) *d = 1.0;
  else *d = *d * lam;
}

// L L^T x = b for the lower factor L (row-major, ld), one workgroup: column-oriented forward substitution, then
// the transposed solve on the same LDS vector.  Every element is updated in a fixed order.  The finished element j
// is written back at step j + 1 (after the barrier), so no thread reads a value another one is changing.
__global__ void __launch_bounds__(1024) k_sba_trsv(const double* __restrict__ L, int ld, int n,
                                                   const double* __restrict__ b, double* __restrict__ x) {
  __shared__ double y[kSbaMaxN];
  const int tid = threadIdx.x, NT = blockDim.x;
  for (int i = tid; i < n; i += NT) y[i] = b[i];
  double prev = 0.0;
  for (int j = 0; j < n; ++j) {
    __syncthreads();
    if (tid == 0 && j > 0) y[j - 1] = prev;
    const double yj = y[j] / L[(size_t)j * ld + j];
    prev = yj;
    for (int i = j + 1 + tid; i < n; i += NT) y[i] -= L[(size_t)i * ld + j] * yj;
  }
  __syncthreads();
  if (tid == 0 && n > 0) y[n - 1] = prev;
  for (int j = n - 1; j >= 0; --j) {
    __syncthreads();
    if (tid == 0 && j < n - 1) y[j + 1] = prev;
    const double xj = y[j] / L[(size_t)j * ld + j];
    prev = xj;
    const double* Lj = L + (size_t)j * ld;
    for (int i = tid; i < j; i += NT) y[i] -= Lj[i] * xj;
  }
  __syncthreads();
  if (tid == 0 && n > 0) y[0] = prev;
  __syncthreads();
  for (int i = tid; i < n; i += NT) x[i] = y[i];
}

// r = B - A x with the unfactored A: one wave per row, lane-strided partial sums and a fixed-shape tree
__global__ void __launch_bounds__(256) k_sba_resid(const double* __restrict__ A, int lda, int n,
                                                   const double* __restrict__ x, const double* __restrict__ B,
                                                   double* __restrict__ r) {
  __shared__ double s[256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wave;
  double acc = 0.0;
  if (row < n) {
    const double* Ar = A + (size_t)row * lda;
    for (int k = lane; k < n; k += 64) acc += Ar[k] * x[k];
  }
  s[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 32; w > 0; w >>= 1) {
    if (lane < w) s[threadIdx.x] += s[threadIdx.x + w];
    __syncthreads();
  }
  if (lane == 0 && row < n) r[row] = B[row] - s[threadIdx.x];
}

// x += dx and |x|^2 (one workgroup, fixed-order tree)
__global__ void __launch_bounds__(256) k_sba_refine(double* __restrict__ x, const double* __restrict__ dx, int n,
                                                    SbaResult* __restrict__ res) {
  __shared__ double s[256];
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int i = tid; i < n; i += 256) {
    const double v = x[i] + dx[i];
    x[i] = v;
    acc += v * v;
  }
  s[tid] = acc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) s[tid] += s[tid + w];
    __syncthreads();
  }
  if (tid == 0) res->x2 = s[0];
}

__device__ __forceinline__ bool sba_skip_update(const SbaResult* res) {
  return res->status != 0 || res->x2 < 1e-16;            // converged (sba.cpp:1425-1432) or a failed factor
}

// camera update (sba.cpp:1435-1466): trans += x[0:3]; qrot = normalize(qrot * (x[3:6], sqrt(1 - |x[3:6]|^2)))
__global__ void __launch_bounds__(256) k_sba_update_nodes(double* __restrict__ nodes, double* __restrict__ old, int nn,
                                                          const double* __restrict__ x, const SbaResult* __restrict__ res) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nn || sba_skip_update(res)) return;
  double* nd = nodes + 7 * i;
  for (int k = 0; k < 7; ++k) old[7 * i + k] = nd[k];
  if (i == 0) return;                                     // node 0 is fixed
  const double* d = x + 6 * (i - 1);
  nd[0] += d[0]; nd[1] += d[1]; nd[2] += d[2];
  const double vx = d[3], vy = d[4], vz = d[5];
  const double vw = sqrt(1.0 - (vx * vx + vy * vy + vz * vz));
  const double w = nd[3], qx = nd[4], qy = nd[5], qz = nd[6];
  double q[4] = {w * vw - qx * vx - qy * vy - qz * vz,
                 w * vx + qx * vw + qy * vz - qz * vy,
                 w * vy + qy * vw + qz * vx - qx * vz,
                 w * vz + qz * vw + qx * vy - qy * vx};
  const double nrm = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int k = 0; k < 4; ++k) nd[3 + k] = q[k] / nrm;
}

// point update (sba.cpp:1468-1490): X += tp - sum_free T_a^T x_a, node order
__global__ void __launch_bounds__(256) k_sba_update_points(double* __restrict__ pts, double* __restrict__ old, int npts,
                                                           const double* __restrict__ tps, const int* __restrict__ poff,
                                                           const int* __restrict__ pnode,
                                                           const unsigned char* __restrict__ valid,
                                                           const double* __restrict__ prj, const double* __restrict__ x,
                                                           const SbaResult* __restrict__ res) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npts || sba_skip_update(res)) return;
  double* X = pts + 3 * p;
  old[3 * p] = X[0]; old[3 * p + 1] = X[1]; old[3 * p + 2] = X[2];
  const int k0 = poff[p], k1 = poff[p + 1];
  int nv = 0;
  for (int k = k0; k < k1; ++k) nv += valid[k] ? 1 : 0;
  if (nv == 0) return;                                    // no (valid) projection: k_sba_point wrote no tp
  double tp[3] = {tps[3 * p], tps[3 * p + 1], tps[3 * p + 2]};
  for (int k = k0; k < k1; ++k) {
    const int n = pnode[k];
    if (n == 0 || !valid[k]) continue;
    const double* T = prj + (size_t)kSbaPR * k + 54;     // Tpc, 6 x 3
    const double* d = x + 6 * (n - 1);
    for (int q = 0; q < 3; ++q) {
      const double v = T[q] * d[0] + T[3 + q] * d[1] + T[6 + q] * d[2] + T[9 + q] * d[3] + T[12 + q] * d[4] +
                       T[15 + q] * d[5];
      tp[q] -= v;
    }
  }
  X[0] += tp[0]; X[1] += tp[1]; X[2] += tp[2];
}

// cost, pass 1: one projection per thread, a fixed tree per workgroup -> (sum, sum with e^2 < d2, count) partials
__global__ void __launch_bounds__(256) k_sba_cost(const double* __restrict__ nm, const double* __restrict__ pts,
                                                  const int* __restrict__ pnode, const int* __restrict__ ppoint,
                                                  const double* __restrict__ uv, const unsigned char* __restrict__ valid,
                                                  double huber, int nprj, double d2, double* __restrict__ part) {
  __shared__ double s[3][256];
  const int tid = threadIdx.x, k = blockIdx.x * 256 + tid;
  double e2 = 0.0, ein = 0.0, cin = 0.0;
  if (k < nprj && valid[k]) {
    double e[2];
    sba_error(nm + (size_t)kSbaNM * pnode[k] + 12, pts + 3 * ppoint[k], uv + 2 * k, e);
    sba_huber(huber, e);
    e2 = e[0] * e[0] + e[1] * e[1];
    if (e2 < d2) { ein = e2; cin = 1.0; }
  }
  s[0][tid] = e2; s[1][tid] = ein; s[2][tid] = cin;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) { s[0][tid] += s[0][tid + w]; s[1][tid] += s[1][tid + w]; s[2][tid] += s[2][tid + w]; }
    __syncthreads();
  }
  if (tid == 0) { part[3 * blockIdx.x] = s[0][0]; part[3 * blockIdx.x + 1] = s[1][0]; part[3 * blockIdx.x + 2] = s[2][0]; }
}

// cost, pass 2: one workgroup sums the partials (strided, then the same fixed tree)
__global__ void __launch_bounds__(256) k_sba_cost_final(const double* __restrict__ part, int nblk,
                                                        SbaResult* __restrict__ res) {
  __shared__ double s[3][256];
  const int tid = threadIdx.x;
  double a = 0.0, b = 0.0, c = 0.0;
  for (int i = tid; i < nblk; i += 256) { a += part[3 * i]; b += part[3 * i + 1]; c += part[3 * i + 2]; }
  s[0][tid] = a; s[1][tid] = b; s[2][tid] = c;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) { s[0][tid] += s[0][tid + w]; s[1][tid] += s[1][tid + w]; s[2][tid] += s[2][tid + w]; }
    __syncthreads();
  }
  if (tid == 0) { res->cost = s[0][0]; res->cost_in = s[1][0]; res->n_in = s[2][0]; }
}

// The workgroup tree of k_sba_cost for the two kernels below: three values per thread -> part[3 * block ..]
__device__ __forceinline__ void sba_block_sum3(double a, double b, double c, double* __restrict__ part) {
  __shared__ double s[3][256];
  const int tid = threadIdx.x;
  s[0][tid] = a; s[1][tid] = b; s[2][tid] = c;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) { s[0][tid] += s[0][tid + w]; s[1][tid] += s[1][tid + w]; s[2][tid] += s[2][tid + w]; }
    __syncthreads();
  }
  if (tid == 0) { part[3 * blockIdx.x] = s[0][0]; part[3 * blockIdx.x + 1] = s[1][0]; part[3 * blockIdx.x + 2] = s[2][0]; }
}

// countBad / removeBad (sba.cpp:416-462), pass 1: one projection per thread.  A valid projection whose weighted
// e^2 >= d2 counts; with mark != 0 its flag is cleared as well (each thread writes its own byte only).
__global__ void __launch_bounds__(256) k_sba_flag_bad(const double* __restrict__ nm, const double* __restrict__ pts,
                                                      const int* __restrict__ pnode, const int* __restrict__ ppoint,
                                                      const double* __restrict__ uv, unsigned char* __restrict__ valid,
                                                      double huber, int nprj, double d2, int mark,
                                                      double* __restrict__ part) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  double bad = 0.0;
  if (k < nprj && valid[k]) {
    double e[2];
    sba_error(nm + (size_t)kSbaNM * pnode[k] + 12, pts + 3 * ppoint[k], uv + 2 * k, e);
    sba_huber(huber, e);
    if (e[0] * e[0] + e[1] * e[1] >= d2) {
      bad = 1.0;
      if (mark) valid[k] = 0;
    }
  }
  sba_block_sum3(bad, 0.0, 0.0, part);
}

// calcAvgError and numBadPoints (sba.cpp:365-411), pass 1: (sum of the weighted |e|, valid projections, valid
// projections whose unweighted error is exactly (0, 0): in practice p1.z <= 0)
__global__ void __launch_bounds__(256) k_sba_stats(const double* __restrict__ nm, const double* __restrict__ pts,
                                                   const int* __restrict__ pnode, const int* __restrict__ ppoint,
                                                   const double* __restrict__ uv, const unsigned char* __restrict__ valid,
                                                   double huber, int nprj, double* __restrict__ part) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  double en = 0.0, nv = 0.0, nz = 0.0;
  if (k < nprj && valid[k]) {
    double e[2];
    sba_error(nm + (size_t)kSbaNM * pnode[k] + 12, pts + 3 * ppoint[k], uv + 2 * k, e);
    nv = 1.0;
    if (e[0] == 0.0 && e[1] == 0.0) nz = 1.0;
    sba_huber(huber, e);
    en = sqrt(e[0] * e[0] + e[1] * e[1]);
  }
  sba_block_sum3(en, nv, nz, part);
}

// ---------------------------------------------------------------------------------------
// Block-Jacobi preconditioned conjugate gradient: jacobiBPCG<6>::doBPCG2 (bpcg/bpcg.h:238-316) on
// the block array of k_sba_pairs_blk.  Per CG iteration three launches, all on the solver's stream:
//   k_sba_cg_mv      q = A d per block row (neighbours ascending) and the partial sums of d . q
//   k_sba_cg_step    a = dn / (d . q);  x += a d;  r -= a q;  s = J r;  the partial sums of r . s
//   k_sba_cg_dir     dn = r . s;  d = s + (dn / dold) d;  the iteration counter
// The scalars live in SbaCg on the device.  k_sba_cg_mv evaluates the loop's exit test `dn < d0` at the head of every
// round and records it; from then on the launches of that solve return at once.  Every dot product is a per-workgroup
// tree plus a strided sum and the same tree over the partials, which each workgroup of the next kernel repeats for
// itself (same order, same bits), so no kernel waits for another one's last workgroup.
// ---------------------------------------------------------------------------------------
struct SbaCg {
  double dn;          // r . s of the last finished iteration (the value that ends the loop)
  double dold;        // dn of the iteration before (k_sba_cg_step moves it here)
  double d0;          // the stopping bound: tol * dn_0, or the carried-over residual if that is larger
  double a;           // the last step length
  int iters;          // finished CG iterations
  int done;           // 1 once dn < d0 was seen (or the block inverse failed)
  int pad[2];
};

constexpr int kSbaCgRows = 42;        // block rows per 256-thread workgroup: 252 lanes, one per vector element

// Sum of one value per thread over the 256-thread workgroup, k_sba_cost's tree; every thread gets the result.
__device__ __forceinline__ double sba_block_sum(double v, double* __restrict__ s) {
  const int tid = threadIdx.x;
  __syncthreads();                                        // s may still be read from the call before
  s[tid] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) s[tid] += s[tid + w];
    __syncthreads();
  }
  return s[0];
}

// k_sba_cost_final's shape: a strided sum of the n partials, then the tree
__device__ __forceinline__ double sba_part_sum(const double* __restrict__ part, int n, double* __restrict__ s) {
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) a += part[i];
  return sba_block_sum(a, s);
}

// J_i = D_i^-1 through the Cholesky factor D = L L^T: Linv by forward substitution, J = Linv^T Linv.  One thread per
// free node, everything in registers (all loops have constant bounds).  A pivot that is not > 0 sets res->status.
__global__ void __launch_bounds__(256) k_sba_blk_inv(const double* __restrict__ blk, int nfree, double* __restrict__ J,
                                                     SbaResult* __restrict__ res) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nfree) return;
  const double* D = blk + (size_t)36 * i;
  double L[6][6], W[6][6];
  bool bad = false;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double p = D[7 * j];
#pragma unroll
    for (int k = 0; k < j; ++k) p -= L[j][k] * L[j][k];
    if (!(p > 0.0)) bad = true;
    const double l = sqrt(p);
    L[j][j] = l;
#pragma unroll
    for (int r = j + 1; r < 6; ++r) {
      double v = D[6 * r + j];
#pragma unroll
      for (int k = 0; k < j; ++k) v -= L[r][k] * L[j][k];
      L[r][j] = v / l;
    }
  }
  // W = L^-1 (lower): column c of the identity through forward substitution
#pragma unroll
  for (int c = 0; c < 6; ++c) {
#pragma unroll
    for (int r = c; r < 6; ++r) {
      double v = (r == c) ? 1.0 : 0.0;
#pragma unroll
      for (int k = c; k < r; ++k) v -= L[r][k] * W[k][c];
      W[r][c] = v / L[r][r];
    }
  }
  double* o = J + (size_t)36 * i;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
#pragma unroll
    for (int c = r; c < 6; ++c) {
      double v = 0.0;
#pragma unroll
      for (int k = c; k < 6; ++k) v += W[k][r] * W[k][c];
      o[6 * r + c] = v;
      o[6 * c + r] = v;
    }
  }
  if (bad) res->status = 1;
}

// q = A d (jacobiBPCG::mMV2, bpcg.h:142-161) and the partials of d . q.  Lane (row i, r): D_i d_i first, then the
// neighbours of block row i ascending, each as one 6-term product added to the sum: (neighbour, slot, transposed)
// triples in adj, built by the host.  The reference's entry order (block column, then block row, ascending) visits
// the neighbours of one row in the same ascending order.
__global__ void __launch_bounds__(256) k_sba_cg_mv(const double* __restrict__ blk, const int* __restrict__ adj_off,
                                                   const int* __restrict__ adj, const double* __restrict__ d, int nfree,
                                                   double* __restrict__ q, double* __restrict__ part,
                                                   SbaCg* __restrict__ cg, const SbaResult* __restrict__ res) {
  __shared__ double s[256];
  const int tid = threadIdx.x;
  const bool done = cg->dn < cg->d0 || res->status != 0;          // `if (dn < d0) break;` (bpcg.h:298)
  if (blockIdx.x == 0 && tid == 0) cg->done = done ? 1 : 0;       // read by the two kernels after this one
  if (done) return;
  const int row = blockIdx.x * kSbaCgRows + tid / 6, r = tid % 6;
  double v = 0.0;
  if (tid < 6 * kSbaCgRows && row < nfree) {
    const double* D = blk + (size_t)36 * row + 6 * r;
    const double* di = d + 6 * row;
    double acc = D[0] * di[0] + D[1] * di[1] + D[2] * di[2] + D[3] * di[3] + D[4] * di[4] + D[5] * di[5];
    for (int k = adj_off[row]; k < adj_off[row + 1]; ++k) {
      const double* M = blk + (size_t)36 * adj[3 * k + 1];
      const double* dv = d + 6 * adj[3 * k];
      double t;
      if (adj[3 * k + 2])                                         // block row `neighbour`, column `row`: M^T d
        t = M[r] * dv[0] + M[6 + r] * dv[1] + M[12 + r] * dv[2] + M[18 + r] * dv[3] + M[24 + r] * dv[4] + M[30 + r] * dv[5];
      else
        t = M[6 * r] * dv[0] + M[6 * r + 1] * dv[1] + M[6 * r + 2] * dv[2] + M[6 * r + 3] * dv[3] + M[6 * r + 4] * dv[4] +
            M[6 * r + 5] * dv[5];
      acc += t;
    }
    q[6 * row + r] = acc;
    v = di[r] * acc;
  }
  const double sum = sba_block_sum(v, s);
  if (tid == 0) part[blockIdx.x] = sum;
}

// kInit: x = 0, r = b, s = J r and the partials of r . s (the head of doBPCG2, bpcg.h:284-287).
// Otherwise the middle of one iteration (bpcg.h:300-304): a from the partials of d . q, x += a d, r -= a q, s = J r.
// The new r of a block goes through LDS so that the six lanes of the block read each other's value, not memory.
template <bool kInit>
__global__ void __launch_bounds__(256) k_sba_cg_step(const double* __restrict__ J, const double* __restrict__ part_dq,
                                                     int nblk, const double* __restrict__ b, const double* __restrict__ d,
                                                     const double* __restrict__ q, double* __restrict__ x,
                                                     double* __restrict__ r, double* __restrict__ sv, int nfree,
                                                     double* __restrict__ part_rs, SbaCg* __restrict__ cg) {
  __shared__ double s[256];
  __shared__ double rn[256];
  const int tid = threadIdx.x;
  double a = 0.0;
  if (!kInit) {
    if (cg->done) return;
    const double dq = sba_part_sum(part_dq, nblk, s);
    a = cg->dn / dq;
    if (blockIdx.x == 0 && tid == 0) { cg->dold = cg->dn; cg->a = a; }     // dn is not written in this kernel
  }
  const int g = blockIdx.x * 6 * kSbaCgRows + tid;
  const bool active = tid < 6 * kSbaCgRows && g < 6 * nfree;
  double rv = 0.0;
  if (active) {
    if (kInit) {
      x[g] = 0.0;
      rv = b[g];
    } else {
      x[g] += a * d[g];
      rv = r[g] - a * q[g];
    }
    r[g] = rv;
  }
  rn[tid] = rv;
  __syncthreads();
  double v = 0.0;
  if (active) {
    const int c = tid % 6;
    const double* Jr = J + (size_t)36 * (g / 6) + 6 * c;
    const double* rb = rn + (tid - c);
    const double t = Jr[0] * rb[0] + Jr[1] * rb[1] + Jr[2] * rb[2] + Jr[3] * rb[3] + Jr[4] * rb[4] + Jr[5] * rb[5];
    sv[g] = t;
    v = rv * t;
  }
  const double sum = sba_block_sum(v, s);
  if (tid == 0) part_rs[blockIdx.x] = sum;
}

// kInit: dn = r . d, d0 = tol dn, raised to the residual the solve before left when abstol is set (bpcg.h:287-292),
// d = s.  Otherwise the tail of one iteration (bpcg.h:305-308): dn = r . s, d = s + (dn / dold) d, one more iteration.
template <bool kInit>
__global__ void __launch_bounds__(256) k_sba_cg_dir(const double* __restrict__ part_rs, int nblk,
                                                    const double* __restrict__ sv, double* __restrict__ d, int n6,
                                                    SbaCg* __restrict__ cg, double tol, int abstol, double residual) {
  __shared__ double s[256];
  const int tid = threadIdx.x;
  if (!kInit && cg->done) return;
  const double dn = sba_part_sum(part_rs, nblk, s);
  const double beta = kInit ? 0.0 : dn / cg->dold;               // dold is not written in this kernel
  const int g = blockIdx.x * 256 + tid;
  if (g < n6) d[g] = kInit ? sv[g] : sv[g] + beta * d[g];
  if (blockIdx.x == 0 && tid == 0) {
    cg->dn = dn;
    if (kInit) {
      double d0 = tol * dn;
      if (abstol && residual > d0) d0 = residual;
      cg->d0 = d0;
      cg->dold = dn;
      cg->a = 0.0;
      cg->iters = 0;
      cg->done = 0;
    } else {
      cg->iters += 1;
    }
  }
}

// |x|^2 of the CG result, k_sba_refine's sum (one workgroup, fixed-order tree)
__global__ void __launch_bounds__(256) k_sba_cg_end(const double* __restrict__ x, int n, SbaResult* __restrict__ res) {
  __shared__ double s[256];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) acc += x[i] * x[i];
  const double sum = sba_block_sum(acc, s);
  if (threadIdx.x == 0) res->x2 = sum;
}

// Blocked right-looking Cholesky of the lower triangle of the n x n (n % 64 == 0) row-major A in place, with the
// filter's fp64 chain kernels: per 64-column step the packed diagonal factor (and its inverse in Dinv), the panel
// P <- P Linv^T, and the lower tiles of the trailing update.  A non-positive pivot sets status[0].
inline void sba_chol_f64(double* A, int ld, int n, double* Dinv, int* status, hipStream_t st) {
  for (int j = 0; j < n; j += 64) {
    k_chol_diag_packed_f64<<<1, 512, 0, st>>>(A + (size_t)j * ld + j, ld, Dinv, status, 4);
    const int r0 = j + 64, rows = n - r0;
    if (rows <= 0) break;
    double* P = A + (size_t)r0 * ld + j;
    k_panel_direct_f64<<<(rows + 63) / 64, 256, 0, st>>>(P, ld, Dinv, rows);
    GemmArgs g{};                                          // A[r0.., r0..] -= P P^T, lower tiles
    g.A = P; g.lda = ld; g.B = P; g.ldb = ld; g.C = A + (size_t)r0 * ld + r0; g.ldc = ld;
    g.K = 64; g.alpha = -1.0; g.beta = 1.0;
    g.tri = TRI_LOWER; g.row_off = r0; g.col_off = r0;
    k_gemm_mfma_f64<ROLE_TRAILING, false><<<dim3(rows / 64, rows / 64), 256, 0, st>>>(g);
  }
}

}  // namespace ekf
