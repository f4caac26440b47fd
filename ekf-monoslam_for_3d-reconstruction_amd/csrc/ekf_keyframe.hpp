// Key-frame selection: the per-frame rule of mono-slam monoslam_ransac.cpp:585-687 with quat2vec / poses_diff
// (:40-60), as one small launch on the filter's stream behind the update, plus a grid that keeps the candidate's / the emitted
// frame's image on the device.  All arithmetic is fp32 whatever the filter's dtype (the reference's stat14 is a VectorXf): an
// fp64 filter's values are rounded to fp32 first.  Every fp32 product and sum is written with the __f*_rn intrinsics so that
// the compiler contracts nothing into an FMA: apart from acos / sin the numbers are the numpy oracle's (tests/keyframe_oracle.py).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "ekf_rectify.hpp"

namespace ekf {

// enum ekf_keyframe_action of include/ekf_monoslam.h
constexpr int kKfNone = 0, kKfCandidate = 1, kKfEmitCurrent = 2, kKfEmitCandidate = 3, kKfEmitFirst = 4;

constexpr float kKfMinCovInit = 10000000.f;         // min_cov_for_pose (monoslam_ransac.cpp:686)
constexpr float kKfMinCovValid = 1000000.f;         // :630
constexpr float kKfCovSlack = 0.000085f;            // :637
constexpr float kKfMetre = 3.33f;                   // :54
constexpr float kKfDegree = 57.29577951308232f;     // :55

// The selector's state.  Two copies live on the device: a probe reads one and writes the other in full (the host flips
// the roles per frame), so within the kernel a word is either read or written, as with SbaCg (§11.7).
struct KfState {
  float last_pose[7];       // last_image_pose
  float last_vrot[3];       // last_vrot
  float min_cov;            // min_cov_for_pose
  int cand_id;              // Pose_id
  float cand_pose[7];       // min_stat
  float cand_cov[49];       // min_camscov.block<7,7>(0,0), row-major
};

// What one probe reports: read by the host through the bounce buffer, and its action word by k_keyframe_snapshot.
struct KfRecord {
  int action;
  int id;                   // CANDIDATE: this frame; an emit: the emitted id; otherwise the candidate id (0: none yet)
  float dist;               // D = poses_diff(last_pose, s, last_vrot)
  float cov;                // c = Covariance_Parameter() in fp32
  float pose[7];            // of whatever was emitted or just stored (otherwise the current state)
  float sig[49];            // likewise Sigma[0:7, 0:7], row-major
};

// quat2vec (monoslam_ransac.cpp:40-50): n = 2 acos(q0); n > 0.0001 -> q[1:4] * (n / sin(n / 2)), otherwise 0 (a NaN n too)
__device__ __forceinline__ void kf_quat2vec(float q0, float q1, float q2, float q3, float& v0, float& v1, float& v2) {
  const float n = __fmul_rn(acosf(q0), 2.f);
  v0 = v1 = v2 = 0.f;
  if (n > 0.0001f) {
    const float n1 = __fdiv_rn(n, sinf(__fdiv_rn(n, 2.f)));
    v0 = __fmul_rn(q1, n1);
    v1 = __fmul_rn(q2, n1);
    v2 = __fmul_rn(q3, n1);
  }
}

// One workgroup of 64 lanes.  Every lane evaluates c, D and the rule (wave-uniform: loads through uniform addresses); lane
// t < 49 carries element t of the 7 x 7 blocks, lane t < 7 element t of the poses, lane 0 the scalars.  No LDS, no barrier.
template <typename T>
__global__ void __launch_bounds__(64) k_keyframe_probe(const T* __restrict__ mu, const T* __restrict__ S, int ld, int frame_id,
                                                       float move_thresh, const KfState* __restrict__ in,
                                                       KfState* __restrict__ out, KfRecord* __restrict__ rec) {
  const int t = threadIdx.x;
  const float s0 = float(mu[0]), s1 = float(mu[1]), s2 = float(mu[2]);
  const float q0 = float(mu[3]), q1 = float(mu[4]), q2 = float(mu[5]), q3 = float(mu[6]);
  // Covariance_Parameter (vslamRansac.cpp:854-855): (S00 + S11 + S22) then + (S44 + S55 + S66 + S33), left to right
  const float d0 = float(S[0]), d1 = float(S[(size_t)ld + 1]), d2 = float(S[(size_t)2 * ld + 2]), d3 = float(S[(size_t)3 * ld + 3]);
  const float d4 = float(S[(size_t)4 * ld + 4]), d5 = float(S[(size_t)5 * ld + 5]), d6 = float(S[(size_t)6 * ld + 6]);
  const float c = __fadd_rn(__fadd_rn(__fadd_rn(d0, d1), d2), __fadd_rn(__fadd_rn(__fadd_rn(d4, d5), d6), d3));
  // poses_diff (:52-60)
  const float dx = __fsub_rn(in->last_pose[0], s0), dy = __fsub_rn(in->last_pose[1], s1), dz = __fsub_rn(in->last_pose[2], s2);
  const float nrm = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));
  const float a = __fmul_rn(nrm, kKfMetre);
  float v0, v1, v2;
  kf_quat2vec(q0, q1, q2, q3, v0, v1, v2);
  const float b0 = __fmul_rn(__fsub_rn(in->last_vrot[0], v0), kKfDegree);
  const float b1 = __fmul_rn(__fsub_rn(in->last_vrot[1], v1), kKfDegree);
  const float b2 = __fmul_rn(__fsub_rn(in->last_vrot[2], v2), kKfDegree);
  const float D = __fadd_rn(__fadd_rn(__fadd_rn(a, fabsf(b0)), fabsf(b1)), fabsf(b2));

  const float min_cov = in->min_cov;
  const int cand_id = in->cand_id;
  int action = kKfNone;
  float new_min = min_cov;
  if (D > __fmul_rn(move_thresh, 0.5f) && D < move_thresh) {
    if (c < min_cov) { action = kKfCandidate; new_min = c; }
  } else if (D >= move_thresh) {
    if (min_cov < kKfMinCovValid) action = (__fsub_rn(c, min_cov) < kKfCovSlack) ? kKfEmitCurrent : kKfEmitCandidate;
    else if (frame_id < 5) action = kKfEmitFirst;
    new_min = kKfMinCovInit;
  }                                                   // (a NaN D fails every comparison: nothing happens)
  const bool store = action == kKfCandidate;
  const bool emit = action >= kKfEmitCurrent;
  const bool from_cand = action == kKfEmitCandidate;

  if (t < 49) {
    const float cur = float(S[(size_t)(t / 7) * ld + (t % 7)]);
    const float old = in->cand_cov[t];
    out->cand_cov[t] = store ? cur : old;
    rec->sig[t] = from_cand ? old : cur;
  }
  if (t < 7) {
    const float cur = float(mu[t]);
    const float old = in->cand_pose[t];
    out->cand_pose[t] = store ? cur : old;
    rec->pose[t] = from_cand ? old : cur;
    out->last_pose[t] = emit ? cur : in->last_pose[t];
  }
  if (t < 3) {
    const float v = t == 0 ? v0 : (t == 1 ? v1 : v2);
    out->last_vrot[t] = emit ? v : in->last_vrot[t];
  }
  if (t == 0) {
    out->min_cov = new_min;
    out->cand_id = store ? frame_id : cand_id;
    rec->action = action;
    rec->id = (store || action == kKfEmitCurrent || action == kKfEmitFirst) ? frame_id : cand_id;
    rec->dist = D;
    rec->cov = c;
  }
}

// The image side of the action word: CANDIDATE frame -> candidate slot; EMIT_CURRENT / EMIT_FIRST frame -> emit slot;
// EMIT_CANDIDATE candidate slot -> emit slot; otherwise the launch returns at once (the idle launches of §11.7).  16 bytes
// per lane and step where the size allows, grid-stride; the three buffers are hipMalloc'ed (256-byte aligned) and distinct.
__global__ void __launch_bounds__(256) k_keyframe_snapshot(const KfRecord* __restrict__ rec, const unsigned char* __restrict__ frame,
                                                           unsigned char* __restrict__ cand, unsigned char* __restrict__ emit,
                                                           size_t bytes) {
  const int action = rec->action;
  if (action == kKfNone) return;
  const unsigned char* src = action == kKfEmitCandidate ? cand : frame;
  unsigned char* dst = action == kKfCandidate ? cand : emit;
  const size_t n16 = bytes / 16;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint4* s16 = reinterpret_cast<const uint4*>(src);
  uint4* d16 = reinterpret_cast<uint4*>(dst);
  for (size_t i = g; i < n16; i += stride) d16[i] = s16[i];
  for (size_t i = n16 * 16 + g; i < bytes; i += stride) dst[i] = src[i];
}

// Host side of one selector (`ekf_keyframe`).  The rule's state is on the device; the host keeps what is host state already
// (DESIGN.md §10): the Point4sba rows of the candidate and of the last emit, and the last emitted record as it was read back.
struct KfSelector {
  std::string err;
  const void* owner = nullptr;          // the filter it was created for (compared, never dereferenced)
  int device = 0;
  float move_thresh = 18.f;             // MoveThresh (monoslam_ransac.cpp:195)
  int keep_current = 0;                 // EKF_KF_OPT_KEEP_CURRENT_PROJECTIONS
  DevBuf<KfState> d_state;              // two copies; `parity` is the live one
  DevBuf<KfRecord> d_rec;
  int parity = 0;
  DevBuf<unsigned char> d_cand, d_emit;
  int img_w = 0, img_h = 0;
  bool cand_has_image = false, emit_has_image = false, have_emit = false;
  // ekf_keyframe_create_raw: the same two slots for the camera's own frame (raw_w x raw_h x raw_c bytes)
  DevBuf<unsigned char> d_cand_raw, d_emit_raw;
  int raw_w = 0, raw_h = 0, raw_c = 0;
  bool cand_has_raw = false, emit_has_raw = false;
  std::vector<int> cand_rows, emit_rows;                // 3 ints per row
  // rectified getters: the float track centre behind every row (2 per row, none for the "0 0 0" placeholder),
  // the filter's lens model and scale as they were at create, and the scratch of the on-demand launches
  std::vector<float> cand_uv, emit_uv;
  CamParams cam{};
  int scale = 1;
  mutable RectScratch rect;
  KfRecord emitted{};

  static KfState initial() {
    KfState s{};
    s.min_cov = kKfMinCovInit;
    return s;
  }
  // (the buffers are members and go after this body, on the selector's device; d_state is the first one create allocates)
  ~KfSelector() { if (d_state) hipSetDevice(device); }
};

}  // namespace ekf
