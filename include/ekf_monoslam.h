/* ekf_monoslam.h -- C ABI of the MI355X-native EKF-MonoSLAM predict/update core.
 *
 * Drop-in boundary for the math methods of the reference's `class VSlamFilter`
 * (mono-slam/src/vslamRansac.hpp:94-141 of engyasin/EKF-MonoSLAM_for_3D-reconstruction).
 * The reference has no FFI today (it is a plain C++ class subclassed by RosVSLAM,
 * RosVSLAMRansac.hpp:19-38); every entry point below names the reference method or
 * source range it replaces.  "vR.cpp" = mono-slam/src/vslamRansac.cpp.
 *
 * Conventions
 *  - every function returns an `int` status (EKF_OK = 0) unless it documents a count;
 *    `ekf_last_error` gives the message of the last failure on that handle.
 *  - the filter owns all device memory; every pointer crossing the ABI is a caller-owned
 *    HOST buffer unless the parameter is named `d_*` (device pointer, resident in HBM).
 *  - scalars are `float` for an EKF_F32 filter and `double` for an EKF_F64 filter;
 *    such buffers are declared `void*`.
 *  - matrices crossing the ABI are COLUMN-MAJOR (Eigen's default, so a
 *    `VSlamFilter`-shaped C++ wrapper can `Eigen::Map` them directly).
 *  - state layout (vR.hpp:12-25, vR.cpp:163-164, 483-486):
 *      mu = [ r(0:3) | q=(w,x,y,z)(3:7) | v(7:10) | omega(10:13) | map_scale(13) | features... ]
 *    inverse-depth feature = [x y z theta phi rho] (6), XYZ feature = [X Y Z] (3),
 *    contiguous in insertion order.  camera_dim = 14 reproduces the reference
 *    (#define STATE_DIM 14, vR.cpp:22); 13 drops the map-scale element.
 *  - a handle is not thread-safe (the reference filter is single-threaded, node.cpp:865).
 *  - there is no CPU fallback: without a HIP device `ekf_create` fails.
 */
#ifndef EKF_MONOSLAM_H_
#define EKF_MONOSLAM_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3 (round 3): + ekf_export_points_table, ekf_get_feature_ids, ekf_set_feature_meta, ekf_num_archived,
 * EKF_OPT_FUSED_LAUNCHES; the sharded filter accepts the whole update flow; - ekf_debug_flow_trace */
/* 4 (round 4): + EKF_OPT_W_RECOMPUTE (default on), ekf_get_chunk_plan; the map getters are collective on a sharded filter */
/* 5 (round 5): no new entry points; EKF_OPT_SPLIT_BF16 is ON by default (large maps: covariance downdate on the bf16 matrix
 * pipe at fp32 accuracy) and applies to the sharded step too; the sharded step runs the sequential form (EKF_OPT_W_RECOMPUTE);
 * the gathered diagonal blocks of the map getters stay valid between two filter steps */
/* 6 (round 6): + ekf_launch_kinds / ekf_launch_kind_name / ekf_launch_count (which launch structure an update took) */
#define EKF_ABI_VERSION 6

typedef struct ekf_filter ekf_filter;

enum ekf_dtype { EKF_F32 = 0, EKF_F64 = 1 };

enum ekf_status {
  EKF_OK = 0,
  EKF_ERR_ARG = 1,         /* bad argument                                   */
  EKF_ERR_CAPACITY = 2,    /* capacity_features exceeded                     */
  EKF_ERR_DEVICE = 3,      /* HIP runtime failure                            */
  EKF_ERR_STATE = 4,       /* call order (e.g. update before predict)        */
  EKF_ERR_NUMERIC = 5,     /* innovation covariance not positive definite    */
  EKF_ERR_UNSUPPORTED = 6
};

/* ConfigVSLAM (ConfigVSLAM.h:23-48) + camConfig (camModel.hpp:9-11) + frame size.
 * fx, fy, u0, v0 are the values AFTER the reference's division by `scale`
 * (ConfigVSLAM.cpp:87-103); image_width/height are frame.size() after the resize
 * of captureNewFrame (vR.cpp:236). */
typedef struct ekf_config {
  float sigma_vx, sigma_vy, sigma_vz;
  float sigma_wx, sigma_wy, sigma_wz;
  float rho_0, sigma_rho_0;
  int window_size, sigma_pixel, kernel_size, sigma_size, scale;
  float T_camera;
  int nInitFeatures, min_features, max_features, forsePlane;
  float fx, fy, u0, v0, k1, k2, k3, p1, p2;
  int image_width, image_height;
} ekf_config;

enum ekf_option {
  /* 0: in-place strip kernel (touches 26 n elements); 1: streaming out-of-place
   * Sigma' = F Sigma F^T + Q (reads n^2, writes n^2 -- the formulation the reference's
   * `.eval()` at vR.cpp:477 has, and the one the HBM roofline of P-propagate is quoted on). */
  EKF_OPT_PROPAGATE_STREAMING = 0,
  /* 1 (default): hand-written MFMA kernels for the dense contractions (fp32: v_mfma_f32_32x32x2_f32,
   * fp64: v_mfma_f64_16x16x4_f64); 0: plain VALU tiles. */
  EKF_OPT_USE_MFMA = 1,
  /* profiling level: 0 off, 1 HIP events around the dominant kernels (downdate, streaming propagate),
   * 2 around every kernel, 3 as 1 but only in every 8th update since the last ekf_profile_reset (each pair of
   * events costs ~6 microseconds of queue time: 5 % of a step at N = 200). */
  EKF_OPT_PROFILE = 2,
  /* Chunked factorisation: 0 = one chunk, one stream (plain blocked Cholesky + one solve + one downdate; for A/B runs:
   * the solve then goes through the explicit inverse of the WHOLE factor, and Sigma after an update is an order of
   * magnitude further from the fp64 result than on the default path at 2M >= 2000 -- 1.2e-4 against 1.2e-5 of
   * max|Sigma|, tools/acc_check_sizes.py);
   * 1 = the default three column chunks, the solve / downdate / W re-evaluation (or update) of every chunk but the last on a
   * second, CU-masked stream beside the serial chain; k >= 2 = k equal chunks;
   * -1 (default): as 1 when the chain has at least 8 block steps (m >= 1024), else as 0. */
  EKF_OPT_PIPELINE = 3,
  /* 1 (default since round 5): the covariance downdate Sigma -= V_g V_g^T of large maps (at least 23 tile rows of 128: N >= ~480
   * inverse-depth features on a 256-CU device) runs on the bf16 matrix pipe AT FP32 ACCURACY: each fp32 operand is split
   * exactly into three bf16 values, a = a1 + a2 + a3, and six of the nine bf16 products -- all but a2 b3, a3 b2, a3 b3, which
   * together are <= 2^-24 |a||b| in the worst case and 2^-28 |a||b| on average, the size of the fp32 product's own rounding
   * (2^-24 worst, 2^-25.5 mean) -- are accumulated in fp32 by v_mfma_f32_32x32x16_bf16 (csrc/ekf_syrk6.hpp).  Every other contraction, every
   * accumulation, the state and the covariance stay fp32.  Measured against the fp64 oracle the result is as close as the
   * fp32 instruction's (tests/test_gpu_parity.py::test_split_bf16_downdate_is_fp32_accurate runs BOTH arithmetics -- the
   * launch counters prove which kernel each filter ran -- and ::test_n1000_exact_fp32_downdate_matches_fp64_oracle /
   * ::test_n1000_default_pipeline_matches_fp64_oracle hold each at N = 1000 against the fp32-oracle yardstick); it is not bit-equal
   * to it.  Sigma stays exactly symmetric, and a rank of a sharded filter computes bit-identical rows (every element pair is
   * one sum, whoever computes it).  0: every contraction on v_mfma_f32_32x32x2_f32 (the arithmetic of rounds 1-4).  fp32
   * filters only; smaller maps and fp64 filters are not affected. */
  EKF_OPT_SPLIT_BF16 = 4,
  /* 0 (default: the reference's model -- the map is static, features carry no process noise).  v > 0: every
   * predict adds v x 1e-12 to the variance of every feature state (Sigma[i][i], i >= camera_dim): the "stabilising
   * noise" of EKF-SLAM practice, for callers who want it.  The fp32 filter does not need it to stay positive: with
   * every feature measured in every frame Sigma stays positive to rounding over every run followed so far (N = 200:
   * 12000 frames, 1000: 3000, 4000: 1200; profiles/r2_drift_after_fix.txt).  Any dtype. */
  EKF_OPT_FEATURE_NOISE = 5,
  /* 1 (default): launch-bound sequences go out as fused launches where that changes no result beyond rounding --
   * camera step + strip congruence + per-feature h / H of ekf_predict as one launch (bit-identical to the three), and,
   * when the innovation fits one 128-column block (2 M + 3 <= 128: the reference's operating point of <= 35 features),
   * gain solve + state update as one launch without the panel step (same sums in another order: fp32 rounding).
   * 0: one launch per kernel (what the per-kernel profile of EKF_OPT_PROFILE = 2 times). */
  EKF_OPT_FUSED_LAUNCHES = 6,
  /* Chunked factorisation, fp32 MFMA path (round 4).  1 (default): after the downdate of column chunk g the columns of
   * W = Sigma H^T of the NEXT chunk are re-evaluated from the downdated Sigma -- the sequential form of the update:
   * W'_h = (Sigma - sum_{g<h} V_g V_g^T) H_h^T, algebraically what the right-looking GEMM update
   * W_h -= V_g L_hg^T produces, for 26 n w_h flop and one read of those columns of Sigma instead of 2 n w_g w_h flop
   * (15 of the 99 GFLOP of a step at N = M = 1000; 15 % at N = 4000); only the innovation row is still updated
   * right-looking (inside the downdate launch).  0: the right-looking W update of rounds 1-3.  The sharded step runs the
   * same sequential form since round 5 (a rank re-evaluates ITS rows of W from its downdated rows of Sigma).  Same result
   * up to fp32 rounding. */
  EKF_OPT_W_RECOMPUTE = 7
};

/* Fills `cfg` with the reference defaults (ConfigVSLAM.cpp:27-47, camModel.hpp:22-31). */
void ekf_config_default(ekf_config* cfg);

int ekf_abi_version(void);

/* VSlamFilter::VSlamFilter (vR.cpp:142-223): mu0, Sigma0, Vmax, Vmax_n.  `device` is the HIP
 * device ordinal.  capacity_features bounds numOfFeatures() for the life of the handle. */
int ekf_create(const ekf_config* cfg, int camera_dim, int capacity_features, int dtype,
               int device, ekf_filter** out);
void ekf_destroy(ekf_filter* f);
/* Message of the last failure (f may be NULL: last failure of ekf_create). */
const char* ekf_last_error(const ekf_filter* f);

/* captureNewFrame's dT (vR.cpp:226-233) and getDt (vR.cpp:247). */
int ekf_set_dt(ekf_filter* f, double dT);
double ekf_get_dt(const ekf_filter* f);

/* Launch on a caller-provided hipStream_t (e.g. torch.cuda.current_stream().cuda_stream). */
int ekf_set_stream(ekf_filter* f, void* hip_stream);
int ekf_set_option(ekf_filter* f, int option, int value);
int ekf_synchronize(ekf_filter* f);

/* VSlamFilter::addFeature (vR.cpp:309-371).  Returns 1 = added, 0 = pixel outside the image
 * margin (vR.cpp:314), negative = -ekf_status. */
int ekf_add_feature(ekf_filter* f, double u, double v);
/* VSlamFilter::removeFeature (vR.cpp:373-421): splices the feature out of mu / Sigma and
 * shifts position_in_state of later features. */
int ekf_remove_feature(ekf_filter* f, int index);
/* Batched removal, one compaction pass; same result as removing the listed indices in
 * descending order (the order of the loop at vR.cpp:1296-1299). */
int ekf_remove_features(ekf_filter* f, const int* indices, int count);

/* VSlamFilter::predict (vR.cpp:451-603) without the image blur: covariance propagation
 * Sigma <- F Sigma F^T + Q, Predict_State, and for every feature h, the compact
 * measurement Jacobian (2x7 camera block + 2x6 / 2x3 feature block), the visibility test
 * (vR.cpp:529) and the rho <= 0 removal flag (vR.cpp:517-521), and the 2x2 diagonal block
 * of St = H Sigma H^T + sigma_px^2 I that `Patch::findMatch` is gated with (vR.cpp:875).
 * t_ctl / r_ctl: 3 scalars each (may be NULL = 0); vcontrol selects Vmax vs Vmax_n. */
int ekf_predict(ekf_filter* f, const void* t_ctl, const void* r_ctl, int vcontrol);
/* The motion Jacobian Ft (the 13x13 block System_model_jacobian fills, vR.cpp:454, 1492-1507) and the process
 * noise Q = Ft[:,7:13] (V / dT^2) Ft[:,7:13]^T (vR.cpp:463-475) of the last ekf_predict, 13 x 13 column-major each;
 * either pointer may be NULL. */
int ekf_get_motion_jacobian(ekf_filter* f, void* Ft, void* Q);
/* Re-evaluates h / H / flags / 2x2 blocks at the current state (the recomputation at
 * vR.cpp:1080-1117 before the high-innovation update). */
int ekf_measure(ekf_filter* f);

/* Per-feature outputs of the last predict/measure.  Any pointer may be NULL.
 * h: 2 per feature; visible / remove_flag: 1 byte per feature; S2x2: 4 per feature,
 * column-major 2x2; Hc: 14 per feature (2x7 column-major); Hf: 12 per feature (2x6
 * column-major, last 3 columns zero for an XYZ feature). */
int ekf_get_predictions(ekf_filter* f, void* h, unsigned char* visible,
                        unsigned char* remove_flag, void* S2x2, void* Hc, void* Hf);

/* The EKF update block (vR.cpp:1245-1284; the same block at 1053-1061 and 663-676):
 * St = H Sigma H^T + R, Kt = Sigma H^T St^-1, mu += Kt (z - h), Sigma <- (I - Kt H) Sigma,
 * normalizeQuaternion (vR.cpp:1625-1642).  `indices` (strictly ascending feature indices, M of them: the order of
 * position_in_z, vR.cpp:589)
 * is the measured set, z holds 2 pixels per listed feature.  plane_constraint != 0 appends
 * the forsePlane pseudo-measurement (vR.cpp:1250-1263, 1272).  M = 0 and no plane: no-op.
 * A factorisation of St that meets a non-positive pivot is reported as EKF_ERR_NUMERIC by the next
 * synchronising call (ekf_synchronize, any getter).  (Through most of round 2 an fp32 map whose features were ALL
 * measured in EVERY frame ended there after a few hundred frames; the cause -- partial sums rounded at the magnitude
 * of Sigma -- was fixed, see EKF_OPT_FEATURE_NOISE above and DESIGN.md section 8: the fp32 covariance now stays
 * positive over every run followed so far.) */
int ekf_update(ekf_filter* f, const void* z, const int* indices, int M, int plane_constraint);
/* Same with z (2 M scalars) and indices (M ints) already resident in DEVICE memory.  Contract:
 *  - both buffers are read IN PLACE and ASYNCHRONOUSLY by the kernels of the queued step: they must stay allocated
 *    and unmodified until the step has run (ekf_synchronize, any getter, or an event the caller records on the
 *    filter's stream after this call);
 *  - the host cannot validate them.  The first kernel of the step checks every index (inside [0, N), strictly
 *    ascending); a bad list raises a device flag that the next synchronising call reports as EKF_ERR_ARG.  Until
 *    then every kernel clamps the indices it uses into [0, N), so nothing is read out of bounds, but the state
 *    after such a step is meaningless. */
int ekf_update_device(ekf_filter* f, const void* d_z, const int* d_indices, int M,
                      int plane_constraint);

/* computeEllipsoidParameters (vR.cpp:1368-1382) for every feature, from the 2x2 St blocks of the last
 * predict/measure: out holds 3 ints per feature (semi-axis of the smaller eigenvalue, of the larger one,
 * angle in degrees of the minor-axis eigenvector with non-negative x component). */
int ekf_get_search_ellipses(ekf_filter* f, int sigma_size, int* out);

/* 1-point RANSAC hypothesis evaluation (vR.cpp:986-1034), every measured feature as a hypothesis, in
 * one pass on the device: counts[k] = number of listed features within `threshold` pixels of their
 * measurement after the single-feature update with feature indices[k] (the reference uses
 * threshold = 2 * sigma_pixel, :968).  best = the hypothesis with most inliers (lowest k on ties;
 * the reference keeps the flags of the LAST hypothesis it happened to draw, :1022 -- its stopping rule
 * makes that one of the best; returning the best is the deterministic equivalent), inliers_of_best:
 * 1 byte per listed feature.  Any output pointer may be NULL.  Needs ekf_predict / ekf_measure. */
int ekf_ransac_1point(ekf_filter* f, const void* z, const int* indices, int M, double threshold,
                      int* counts, unsigned char* inliers_of_best, int* best);

/* High-innovation rescue (vR.cpp:1066-1117), after the low-innovation update: for the listed features
 * (matched but not low-innovation inliers) h / H are re-evaluated with the feature entries of the CURRENT
 * (updated) state and the camera pose `cam_before` = mu[0:7] of the state BEFORE that update (the
 * reference's choice, :1069-1072), S_hi = H Sigma H^T without measurement noise (:1113), and
 * is_hi[k] = ((h - z)^T S_hi^-1 (h - z) <= chi2_threshold) (the reference uses 1, :1066).  The listed
 * features keep the new h / H, so a following ekf_update over the rescued ones uses them (:1119-1130). */
int ekf_rescue_high_innovation(ekf_filter* f, const void* cam_before, const void* z, const int* indices,
                               int M, double chi2_threshold, unsigned char* is_hi);

/* The RANSAC branch of VSlamFilter::update in ONE call (vR.cpp:964-1130 + 1245-1284), for the matched features
 * `indices` (strictly ascending, M of them) with pixels z:
 *   1. every 1-point hypothesis is evaluated on the device (as ekf_ransac_1point, threshold `ransac_threshold`;
 *      the reference uses 2 * sigma_pixel, :968);
 *   2. seed == 0: the low-innovation set is that of the BEST hypothesis (most inliers, lowest index on ties) -- the
 *      deterministic form.  seed != 0: the reference's own loop is replayed on those counts -- hypotheses drawn
 *      without replacement with glibc's srand(seed) / rand() sequence (the reference seeds with time(NULL), :970),
 *      nhyp adapted as (int)(log(1 - 0.99) / log(1 - best_count / M)) (:1030), and the low-innovation set is that of
 *      the LAST hypothesis drawn (the reference overwrites the flags on every draw, :1022);
 *   3. EKF update with the low-innovation inliers, no plane rows (:1036-1064);
 *   4. the remaining matched features are re-linearised at (camera pose before step 3, features after it) and
 *      gated by (h - z)^T S_hi^-1 (h - z) <= chi2_threshold with S_hi = H Sigma H^T (:1066-1117; the reference uses 1);
 *   5. second EKF update with the rescued features and, if plane_constraint, the forsePlane rows (:1245-1284).
 * Outputs (any may be NULL): is_low_innovation / is_high_innovation, one byte per listed feature;
 * hypotheses_drawn = draws of the replayed loop (M in the deterministic form).  Needs ekf_predict. */
int ekf_update_two_stage(ekf_filter* f, const void* z, const int* indices, int M, int plane_constraint,
                         unsigned int seed, double ransac_threshold, double chi2_threshold,
                         unsigned char* is_low_innovation, unsigned char* is_high_innovation, int* hypotheses_drawn);

/* ---- image side: what sits between predict() and the EKF update in the reference ----
 * captureNewFrame's image (vR.cpp:234-245) AFTER the node's resize / grayscale (ekf_set_frame_raw below takes the
 * frame BEFORE them): 8-bit, single channel,
 * image_width x image_height of the config; `stride` = bytes per row.  The frame is copied to the device.
 * While a frame is set, ekf_add_feature also captures the feature's window_size^2 template at
 * ((int)(u - w/2), (int)(v - w/2)) (Patch::Patch in addFeature, vR.cpp:318) and removals keep the
 * templates aligned with their features (vR.cpp:1296-1299). */
int ekf_set_frame(ekf_filter* f, const unsigned char* gray, int width, int height, int stride);
/* The camera's own frame: 8-bit, `channels` = 1 (grey) or 3 (interleaved B, G, R), width x height,
 * `stride` bytes per row.  The frame is copied once into a device buffer the filter owns and the matcher frame of
 * ekf_set_frame is derived from it ON THE DEVICE by one launch: cv::resize(INTER_LINEAR) by 1 / ekf_config.scale, channel
 * by channel, then cvtColor(BGR2GRAY), both restated as the integer arithmetic section 13 pins (vR.cpp:235-245).
 * width / scale x height / scale (integer division) must be image_width x image_height of the config.  Every consumer
 * (templates, NCC search, corner seeding, key-frame images) sees the derived frame as if ekf_set_frame had delivered it;
 * a raw key-frame selector (ekf_keyframe_create_raw) additionally keeps the raw frame.  A later ekf_set_frame drops the
 * raw frame.  On a sharded filter every rank is given the same frame and derives it itself (no collective).
 * EKF_ERR_ARG, before the device is touched: pixels NULL, channels not 1 / 3, stride < width * channels, scale < 1,
 * derived size != config size.
 *  - ekf_set_frame_raw: `pixels` is host memory; the call synchronises (the buffer may be reused at once);
 *  - ekf_set_frame_raw_device: `d_pixels` is device memory (a decoder's output, a tensor); the copy and the launch are
 *    queued on the filter's stream and the host is NOT synchronised: the buffer must stay valid and unchanged until
 *    ekf_synchronize (or any call that reads results back) returns;
 *  - ekf_get_frame: the matcher frame as the consumers see it, image_height rows of image_width bytes, `stride` bytes
 *    apart (inspection / tests).  EKF_ERR_STATE without a frame. */
int ekf_set_frame_raw(ekf_filter* f, const unsigned char* pixels, int width, int height, int channels, int stride);
int ekf_set_frame_raw_device(ekf_filter* f, const void* d_pixels, int width, int height, int channels, int stride);
int ekf_get_frame(ekf_filter* f, unsigned char* gray, int stride);
/* Patch::patch of feature `index`: window_size^2 bytes, row-major (test injection / inspection).
 * matching != 0 reads Patch::matching_patch (the blurred copy or the last matched window). */
int ekf_set_patch(ekf_filter* f, int index, const unsigned char* pixels);
int ekf_get_patch(ekf_filter* f, int index, int matching, unsigned char* out);
/* hi_out_blurred of every feature (vR.cpp:546, 575): the prediction at the pose r + v T_camera dT,
 * q (x) quat(w T_camera dT), 2 scalars per feature.  ekf_predict computes it, together with
 * Patch::blur (Patch.cpp:50-57, libblur.cpp:17-79: line kernel, filter2D with BORDER_REFLECT_101) of every
 * visible feature's template, whenever templates are present. */
int ekf_get_blur_predictions(ekf_filter* f, void* hb);
/* Patch::findMatch (Patch.cpp:215-293) for every visible feature, on the device: NCC
 * (computeCorrelation, Patch.cpp:295-329) of the matching template against every window whose centre lies
 * in the clamped sigma_size box and inside the Mahalanobis ellipse of the feature's 2x2 St block; first
 * maximum in scan order; found[i] = (score >= threshold) (the reference's patch_matching_threshold is 0.8,
 * Patch.cpp:14).  z: 2 scalars per feature (the matched centre, or -1 -1), score: the best NCC (-1 if no
 * candidate).  A found feature's matching template becomes the matched window (Patch.cpp:286).
 * Any of z / found / score may be NULL. */
int ekf_find_matches(ekf_filter* f, double threshold, void* z, unsigned char* found, float* score);

/* Full St for a measured set (vR.cpp:598): out is m x m column-major, m = 2M (+3). */
int ekf_innovation_covariance(ekf_filter* f, const int* indices, int M, int plane_constraint,
                              void* S_out);
/* Kt of the last update (n x m column-major, n = state dim before normalisation). */
int ekf_get_gain(ekf_filter* f, void* K_out);
int ekf_last_measurement_rows(const ekf_filter* f);

/* VSlamFilter::convert2XYZ_ifLinear (vR.cpp:741-772): returns 1 converted, 0 not, <0 error. */
int ekf_convert_xyz_if_linear(ekf_filter* f, int index);
/* VSlamFilter::convert2XYZ_ifLinearAll (vR.cpp:776-780): returns the number converted. */
int ekf_convert_xyz_if_linear_all(ekf_filter* f);

/* numOfFeatures (vR.cpp:127-129) and mu.size(). */
int ekf_num_features(const ekf_filter* f);
int ekf_state_dim(const ekf_filter* f);
/* Patch::position_in_state / Patch::coding (0 = inverse depth, 1 = XYZ) per feature. */
int ekf_get_feature_layout(const ekf_filter* f, int* position_in_state, int* coding);

/* getState (vR.cpp:135-140) generalised to any segment; set_* inject test inputs. */
int ekf_get_state(ekf_filter* f, void* out, int offset, int count);
int ekf_set_state(ekf_filter* f, const void* in, int offset, int count);
/* getSigma (vR.cpp:131-133) generalised to any block (RosVSLAM reads Sigma.block directly,
 * RosVSLAMRansac.cpp:171-183). Column-major rows x cols. */
int ekf_get_sigma_block(ekf_filter* f, void* out, int r0, int c0, int rows, int cols);
int ekf_set_sigma_block(ekf_filter* f, const void* in, int r0, int c0, int rows, int cols);
/* Diagnostics only (no reference counterpart; tools/determinism_probe_sharded.py): a block of the workspace of the LAST
 * update, row-major rows x cols in the filter's dtype.  which = 0: W = Sigma H^T as the triangular solves read it,
 * 1: V = W L^-T (the factor of the covariance downdate).  Rows: state rows, then the padding; columns: 2 x list slot.
 * which = 3 (round 6; EKF_SMALL_STAMPS=1): the phase stamps of the one-launch update of a small map (k_update_small_onelaunch):
 * 16 64-bit words of the 100 MHz clock as rows = 16, cols = 2 32-bit halves, r0 = c0 = 0 (tools/small_stamps.py).
 * which = 4: the corner response lambda of the last ekf_find_new_features (csrc/ekf_features.hpp), a block of the
 * image_height x image_width frame, row-major, fp64 whatever the filter's dtype (r0 = row, c0 = column). */
int ekf_peek_workspace(ekf_filter* f, int which, void* out, int r0, int c0, int rows, int cols);
/* Covariance_Parameter (vR.cpp:841-866): trace of Sigma[0:7,0:7]. */
int ekf_covariance_parameter(ekf_filter* f, double* out);
/* Invariants of the device-resident covariance, evaluated on the device (no n^2 copy): max |Sigma| outside the live
 * n x n inside the padded buffer (the tile kernels rely on exact zeros there), max |Sigma[i][j] - Sigma[j][i]| and
 * max |Sigma[i][j]| over the live block (the reference never symmetrises, vR.cpp:1279; this implementation keeps
 * Sigma exactly symmetric).  A NaN is never dropped: one anywhere outside the live block makes max_abs_outside_live
 * NaN, one in the live block makes max_abs_live NaN, and one in an off-diagonal live entry (or an entry pair whose
 * difference is NaN, such as inf - inf) makes max_asymmetry NaN as well, so that `pad == 0 && asym <= c * big` is
 * false on a covariance that holds a NaN.  Finite input is reported as its maxima, rounded to float.
 * Any pointer may be NULL.  Test / debug entry: no counterpart in the reference. */
int ekf_check_invariants(ekf_filter* f, double* max_abs_outside_live, double* max_asymmetry, double* max_abs_live);
/* inverseDepth2XyzWorld mode 1 + Jf Sigma_ff Jf^T (vR.cpp:690-738,
 * RosVSLAMRansac.cpp:177-183): world point (3) and 3x3 covariance (column-major). */
int ekf_feature_xyz(ekf_filter* f, int index, void* xyz, void* cov3x3);

/* RosVSLAM::getPointsFeatures (RosVSLAMRansac.cpp:340-418), the table behind `points.txt`: one row of
 * 12 scalars per feature, ROW-MAJOR N x 12: [X Y Z] * map_scale (mu[13]; 1 for camera_dim 13), then the
 * 3x3 covariance block row by row.  The reference fills the rows of XYZ features only; with
 * convert_inverse_depth != 0 the inverse-depth rows carry inverseDepth2XyzWorld(f) and Jf Sigma Jf^T. */
int ekf_export_points(ekf_filter* f, void* out, int convert_inverse_depth);
/* The same table in the reference's own layout (RosVSLAMRansac.cpp:340-418): rows indexed by Patch::real_index --
 * (real_index of the LAST live feature) + 1 rows (:350-352), ROW-MAJOR rows x 12 --, live XYZ features at their rows,
 * live inverse-depth rows zero, then the patches ARCHIVED at removal written over their rows (:406-414): a removed
 * XYZ feature with n_find > 5 leaves XYZ_pos and the 3x3 block of Sigma of the moment of its removal behind
 * (deleted_patches, vR.cpp:394-404; captured on the device by ekf_remove_feature(s)).  The archive is emptied by the
 * call that finds more than 7000 entries in it (:396-404).  *rows receives the row count; out == NULL only queries it;
 * max_rows < rows is EKF_ERR_ARG.  An archived patch whose real_index lies beyond the table is skipped (the reference
 * writes out of bounds there). */
int ekf_export_points_table(ekf_filter* f, void* out, int max_rows, int* rows);
/* Patch::real_index (vR.cpp:148, 318-319: 1, 2, ... in creation order, never reused) and Patch::n_find (Patch.cpp:86,
 * 145: 1 at creation, +1 per ekf_update_two_stage in which the feature is a low- or high-innovation inlier) per live
 * feature; either pointer may be NULL.  ekf_update (the bare update block) does not touch n_find: a caller that
 * composes its own flow keeps it with ekf_set_feature_meta (a negative value leaves that field alone). */
int ekf_get_feature_ids(const ekf_filter* f, int* real_index, int* n_find);
int ekf_set_feature_meta(ekf_filter* f, int index, int real_index, int n_find);
/* deleted_patches.size() */
int ekf_num_archived(const ekf_filter* f);

/* The rest of a Patch's track state per live feature (any pointer may be NULL):
 *   n_tot: Patch::n_tot -- 1 at creation (Patch.cpp:85), +1 for every feature ekf_find_matches searches, i.e. every
 *     feature visible at the last ekf_predict / ekf_measure (Patch.cpp:218; vR.cpp:872-873);
 *   in_innovation: Patch::isInInnovation -- the visibility flag of the last ekf_predict / ekf_measure (vR.cpp:520, 532,
 *     561), cleared by a failed search (Patch.cpp:281);
 *   center: Patch::center, 2 floats per feature -- (u, v) at creation (Patch.cpp:93), after each ekf_find_matches the
 *     matched pixel of a searched feature or (-1, -1) when it was not found (Patch.cpp:253, 279);
 *   remove_flag: Patch::removeFlag, STICKY -- OR of the rho <= 0 flag of every ekf_predict / ekf_measure (vR.cpp:519)
 *     and of the quality rule of ekf_end_update; cleared only when the feature goes away.  (The per-call remove flag
 *     of ekf_get_predictions keeps its own meaning.)
 * Every reordering of the features (add, removal, conversion, sharded or not) carries the state along.
 * ekf_set_feature_track is for callers that run their own matcher, as ekf_set_feature_meta: a negative n_tot /
 * in_innovation / remove_flag leaves that field alone, center == NULL leaves the centre alone. */
int ekf_get_feature_track(ekf_filter* f, int* n_tot, unsigned char* in_innovation, float* center,
                          unsigned char* remove_flag);
int ekf_set_feature_track(ekf_filter* f, int index, int n_tot, int in_innovation, const float* center, int remove_flag);
/* VSlamFilter::findNewFeatures (vR.cpp:783-837) on the device: the mask of the existing patches (their centres) and
 * goodFeaturesToTrack(frame, features, num, quality_level, min_distance, mask) with the exact corner response of
 * csrc/ekf_features.hpp (the arithmetic is pinned there and in DESIGN.md; the reference passes 0.01 and 12).
 * num <= 0 means nInitFeatures (vR.cpp:785).  out_uv (2 floats per corner, room for num corners; may be NULL)
 * receives the corners in order, *n_out (may be NULL) their count.  add != 0 adds them in that order through
 * ekf_add_feature (vR.cpp:830-833; the template is captured from the current frame) until capacity_features is
 * reached: corners that did not fit are reported, not an error -- the first min(*n_out, capacity - N) were added.
 * add == 0 only reports.  No frame: EKF_ERR_STATE; quality_level or min_distance negative or not finite: EKF_ERR_ARG.
 * The detector's launches are timed under the kernel ids "seed_mask", "seed_response", "seed_candidates" and
 * "seed_select" (EKF_OPT_PROFILE).  The lambda image
 * of the last call can be read with ekf_peek_workspace(which = 4). */
int ekf_find_new_features(ekf_filter* f, int num, double quality_level, double min_distance, int add, float* out_uv,
                          int* n_out);
/* The end of VSlamFilter::update() (vR.cpp:1294-1317), in the reference's order:
 *   1. quality = (float)(n_tot - n_find) / (float)n_find per feature, flagged when quality > matching_ratio (host fp32
 *      as Patch.cpp:147-149; the reference's default is 0.2f).  n_find is NOT incremented here: ekf_update_two_stage
 *      already counted the inliers (Patch.cpp:145);
 *   2. every flagged feature (quality or the sticky rho <= 0 flag) is removed in one ekf_remove_features pass;
 *      removed (room for N ints; may be NULL) receives their pre-removal indices in descending order, *n_removed
 *      their count;
 *   3. *n_visible = surviving features with in_innovation;
 *   4. if n_visible < min_features: feature 0 is removed when N > max_features (:1313), then with seed != 0
 *      findNewFeatures(min_features - n_visible) with 0.01 / 12 adds corners (*n_seeded = how many were added); with
 *      seed == 0 *n_seeded is the count the caller should seed and nothing is added;
 *   5. ekf_convert_xyz_if_linear_all (:1317), after the seeding as in the reference.
 * An empty map is a no-op that reports 0.  seed != 0 needs a frame: without one the call returns EKF_ERR_STATE
 * before it changes anything. */
int ekf_end_update(ekf_filter* f, float matching_ratio, int seed, int* removed, int* n_removed, int* n_visible,
                   int* n_seeded);

/* Per-kernel HIP-event timing (EKF_OPT_PROFILE).  Kernel ids are dense in
 * [0, ekf_profile_kernels()). */
int ekf_profile_kernels(void);
const char* ekf_profile_kernel_name(int kernel_id);
int ekf_profile_read(ekf_filter* f, int kernel_id, double* total_ms, long long* launches);
int ekf_profile_reset(ekf_filter* f);
/* Algorithmic flop of the launches timed under `kernel_id` since the last reset (kept for "downdate_syrk" only:
 * n^2 x the real columns of the chunk (symmetric half).  Where the launch also carries a right-looking update of its
 * chunk -- exact-fp32 path, EKF_FUSE_WU -- that product is counted with it: under EKF_OPT_W_RECOMPUTE = 1 (the default)
 * only the innovation ROW is updated, 2 x 1 x (m - c1) x the chunk's columns; under = 0 the whole W, 2 (n + 1) (m - c1)
 * x those columns).  Where the other pieces of the sequential form are booked: the re-evaluation W'_h = Sigma' H_h^T under
 * "sigma_ht"; the innovation-row update under EKF_OPT_SPLIT_BF16 = 1 rides as the first workgroups of the downdate's
 * launch (its time is inside "downdate_syrk", its 2 (m - c1) x columns flop are not counted), a stand-alone one
 * (EKF_FUSE_WU = 0 on the exact-fp32 path, a rank that owns no rows) under "w_update"; the plane image of V_g under "misc". */
int ekf_profile_work(ekf_filter* f, int kernel_id, double* flop);
/* How the last ekf_update factored S (what the algorithmic flop of a step depends on): `block` = rows of a block step
 * (128 fp32 MFMA, 64 otherwise), ends[g] = block step at which column chunk g ends (the last one = m_pad / block),
 * `w_recompute` = 1 if the W columns of the later chunks were re-evaluated from the downdated Sigma (EKF_OPT_W_RECOMPUTE)
 * rather than updated right-looking.  Returns the number of chunks (0 before the first update; at most `max_chunks`
 * entries are written). */
int ekf_get_chunk_plan(ekf_filter* f, int* ends, int max_chunks, int* block, int* w_recompute);

/* Which launch structure the updates of this handle actually took: one host-side counter per kind, incremented at the
 * launch (always on, no device cost), cleared by ekf_profile_reset.  Diagnostics with no reference counterpart: the
 * bit-identity tests of the tuning knobs assert with it that a knob really changed the launches, and bench.py reports the
 * downdate kernel that ran instead of re-deriving the library's selection rule. */
enum ekf_launch_kind {
  EKF_LAUNCH_DOWNDATE_BF16X6 = 0,     /* k_syrk_bf16x6 (EKF_OPT_SPLIT_BF16 = 1, large maps)                              */
  EKF_LAUNCH_DOWNDATE_F32,            /* k_gemm_mfma<DOWNDATE> 128 x 128, plain tile list (also every VALU / fp64 downdate) */
  EKF_LAUNCH_DOWNDATE_F32_FUSED_WU,   /* ... carrying the chunk's right-looking update as its first tiles (EKF_FUSE_WU)  */
  EKF_LAUNCH_DOWNDATE_F32_HALF_TAIL,  /* ... with 64 x 128 half tiles at the end of its list (EKF_SPLIT_TAIL)            */
  EKF_LAUNCH_DOWNDATE_F32_T64,        /* 64 x 64 tiles (small maps)                                                      */
  EKF_LAUNCH_ROW_RIDER,               /* innovation-row update as the first workgroups of k_syrk_bf16x6                  */
  EKF_LAUNCH_ROW_GEMV,                /* ... as a stand-alone k_innov_row_update launch                                  */
  EKF_LAUNCH_ROW_TILE_GEMM,           /* ... through the 64 x 128 tile GEMM (EKF_ROW_GEMV = 0)                           */
  EKF_LAUNCH_W_UPDATE_GEMM,           /* right-looking update of all of W (EKF_OPT_W_RECOMPUTE = 0), stand-alone launch  */
  EKF_LAUNCH_W_RECOMPUTE,             /* W' = Sigma' H^T re-evaluation launches (EKF_OPT_W_RECOMPUTE = 1)                */
  EKF_LAUNCH_CHAIN_STEP,              /* launches of the per-block-step chain (diagonal factor, panel, trailing)          */
  EKF_LAUNCH_CHAIN_PERSISTENT,        /* retired (the look-ahead chain kernel of round 6 is removed): always counts 0    */
  EKF_LAUNCH_SOLVE,                   /* triangular-solve launches on one wave group per tile                            */
  EKF_LAUNCH_SOLVE_TWO_GROUPS,        /* ... on two wave groups per tile (EKF_SOLVE_S2)                                  */
  EKF_LAUNCH_UPDATE_ONEBLOCK,         /* k_solve_state_oneblock (2 M + 3 <= 128)                                         */
  EKF_LAUNCH_UPDATE_ALLINONE,         /* k_update_oneblock_small (... and a small map)                                   */
  EKF_LAUNCH_CHAIN_TRAIL_DIAG,        /* k_trail_diag: the trailing update of a block step and the factor of the next as one launch (round 6) */
  EKF_LAUNCH_SPLIT_IMAGE,             /* k_split_image of V_g as a launch of its own (else: written by the solve's tiles) */
  EKF_LAUNCH_STATE_UPDATE_TAIL,       /* mu += V y done by the workgroups of the last k_syrk_bf16x6 launch that run out of tiles */
  EKF_LAUNCH_UPDATE_ONELAUNCH,        /* k_update_small_onelaunch: W, S, the factor and the whole rest of the update of a small map (n_pad <= 256) as ONE launch (round 6) */
  EKF_LAUNCH_CHAIN_DIST_GATHER,       /* sharded step, distributed chain: all-gathers of a block step's panel (round 6) */
  EKF_LAUNCH_CHAIN_STEP_FUSED,        /* k_chain_step_fused: factor, panel and trailing update of a block step as ONE launch (one-chunk maps, round 6) */
  EKF_LAUNCH_DOWNDATE_MIRROR_BOUNDS,  /* k_syrk_bf16x6 launches that ran with row bounds for their mirror stores (EKF_SYRK_MIRROR_SKIP = 1, round 7): the launches of an update before its last */
  EKF_LAUNCH_SOLVE_POLL_CHAIN,        /* triangular-solve launches that waited for the chain in their prologue instead of behind a stream wait (EKF_SOLVE_POLL_CHAIN = 1, round 7): the overlapped chunks 1 .. G-2 of an update whose plan has at most 16 block steps */
  EKF_LAUNCH_KINDS
};
int ekf_launch_kinds(void);
const char* ekf_launch_kind_name(int kind);
int ekf_launch_count(ekf_filter* f, int kind, long long* launches);

/* ---- multi-GPU: row-panel sharding, one process per GPU ----------------------------------------
 * Every rank holds the same filter (same calls in the same order on every rank: add / remove / convert / predict /
 * update) and OWNS a contiguous range of features: it keeps valid the rows of Sigma of those features (all columns)
 * plus a replica of the camera rows; mu is replicated.  One sharded step:
 *   predict   camera step + strips; h / H / flags of the OWN features
 *       -> all-gather of the per-feature records (32 scalars per feature)             "reassemble H"
 *   update    nu; W = Sigma H^T rows {camera, own}; rows of S of the own MEASURED features
 *       -> all-gather of the row panels of S                                           "reassemble S"
 *             Cholesky chain of S in column chunks -- replicated on every rank up to 39 block steps (N < 2500); from 40 on
 *             DISTRIBUTED (round 6): a rank keeps its own 128-row blocks (cyclic), every diagonal block and the inverse strip of
 *             the trailing matrix up to date, and per block step
 *       -> all-gather of the rank's blocks of the panel                                (64 KB per block; the step's column of L)
 *             (bit-identical to the replicated chain; EKF_SHARD_DIST_CHAIN=0 keeps it replicated, EKF_SHARD_DIST_MIN_BLOCKS
 *             moves the threshold); per chunk g, beside the chain on a second stream:
 *             V_g = W_g Z_gg for rows {camera tile, own panel, innovation row} (one queued launch)
 *       -> all-gather of the own rows of V_g                                           (n x 2M scalars per step in all)
 *             Sigma[own rows, :] -= V_g[own rows] V_g^T (+ the replicated camera tile; the canonical tiles of k_syrk_bf16x6 that
 *             touch an own block: bit-identical rows), then W' of the next chunk re-evaluated on rows {camera, own} from the
 *             downdated Sigma (round 5: the sequential form; the right-looking W update of rounds 1-4 only under
 *             EKF_OPT_W_RECOMPUTE = 0); after the last chunk mu += V y, normalisation.
 * Any measured subset (strictly ascending list, M <= N), inverse-depth and XYZ features, the plane rows and any N
 * (ranks may own different numbers of features, or none) are supported.  add_feature appends to the LAST rank's
 * range, remove / convert compact every rank's copy alike; when a rank owns more than 1.125 x the mean number of
 * rows the next predict re-partitions (ekf_shard_rebalance: all-gather of the row panels of Sigma, after which every
 * row is valid on every rank, then a fresh row-balanced partition).
 *
 * The library does no communication itself: every exchange is ONE call of the host's all-gather on device staging
 * buffers -- `world` equal slots, slot g = the `bytes_per_rank` bytes rank g passed as d_send, delivered to every
 * rank, enqueued on `hip_stream` (the library packs before and unpacks after on that same stream).  With
 * torch.distributed this is `all_gather_into_tensor` (backend "nccl" = RCCL over xGMI; sharded.py); a C++ node
 * passes a function that calls ncclAllGather(d_send, d_recv, bytes_per_rank, ncclChar, comm, stream).  Every rank
 * makes the same sequence of calls with the same sizes.  Return 0 on success. */
typedef int (*ekf_allgather_fn)(void* ctx, const void* d_send, void* d_recv, size_t bytes_per_rank, void* hip_stream);

typedef struct ekf_shard_info {
  int rank, world, N, state_dim;
  int f_begin, f_end;                     /* own feature range                                             */
  int row_begin, row_end;                 /* own state rows                                                 */
  int max_rows_any_rank;                  /* the largest panel (imbalance = this x world / (n - camera_dim)) */
  int rebalances;                         /* re-partitions since ekf_shard_configure                        */
} ekf_shard_info;

/* Switches the filter to sharded operation.  Call it at a point where every rank holds the same, fully valid
 * filter (e.g. right after the identical construction of the map).  From then on ekf_predict, ekf_update (host
 * z / indices), ekf_add_feature, ekf_remove_feature(s) and ekf_convert_xyz_if_linear(_all) run the sharded step;
 * getters of Sigma are valid for the camera rows and the own rows only (ekf_shard_rebalance makes all rows valid).
 * Round 3: the whole update() flow runs sharded as well -- ekf_update_device (the list is copied to the host once),
 * ekf_update_two_stage, ekf_ransac_1point (every rank evaluates the hypotheses on the listed features it owns, the
 * partial inlier counts are all-gathered), ekf_rescue_high_innovation and the 2x2 St blocks behind ekf_get_predictions /
 * ekf_get_search_ellipses (owner-computes, the blocks are all-gathered), ekf_innovation_covariance; under sharding their
 * measured lists must be strictly ascending.  Round 4: the image side (ekf_set_frame, ekf_set_patch, ekf_find_matches,
 * the predicted blur inside ekf_predict) works on a sharded filter too -- frame and templates are replicated (every
 * rank makes the same calls), the 2x2 blocks the search gates with are all-gathered, and every rank searches every
 * feature (at most 124 us at N = 1000, far below one exchange): the templates stay identical on every rank.
 * world = 1 needs no callback.
 *
 * COLLECTIVE CONTRACT.  On a sharded filter (world > 1) the following entry points run one or more all-gathers and are
 * therefore COLLECTIVE: every rank must call them, with the same arguments, in the same order relative to each other --
 * a rank that skips one, or calls them in another order, leaves the others waiting inside the collective:
 *   ekf_predict, ekf_update, ekf_update_device, ekf_shard_update, ekf_update_two_stage, ekf_shard_rebalance,
 *   ekf_remove_feature(s), ekf_convert_xyz_if_linear(_all) (linearity flags; the removal archive gathers the owners'
 *   3 x 3 blocks), ekf_innovation_covariance, ekf_ransac_1point, ekf_rescue_high_innovation,
 *   ekf_get_predictions WITH s2 and ekf_get_search_ellipses (the 2x2 St blocks; gathered once per predict, so the
 *   first of these calls after a predict is the collective one -- make the same calls on every rank),
 *   ekf_find_matches (the same 2x2 blocks),
 *   ekf_end_update (its removals and conversion; the seeding runs replicated: every rank holds the same frame and
 *   centres, so the detector yields the same corners everywhere, and the adds are the ordinary local add),
 *   ekf_find_new_features (replicated detector, as above; with add, the ordinary add on every rank),
 *   ekf_feature_xyz, ekf_export_points, ekf_export_points_table (round 4: a feature's covariance block is valid on
 *   its owner only; the owners' diagonal blocks are all-gathered first, so every rank returns the same table.  Round 5:
 *   the gathered blocks stay valid until the next call that changes mu, Sigma, the layout or the sharding (predict, the
 *   updates, add / remove / convert, the setters, re-balance, ekf_set_option), so a loop of N per-feature getters between
 *   two filter steps costs ONE all-gather, not N -- the first getter after such a call is the collective one, as for the
 *   2x2 blocks above: make the same getter calls on every rank, or none).
 * Local (no exchange): ekf_add_feature, ekf_get_state, ekf_get_sigma_block (valid for camera + own rows),
 * ekf_get_predictions without s2, ekf_covariance_parameter, ekf_shard_get_info, the setters, ekf_last_error. */
int ekf_shard_configure(ekf_filter* f, int rank, int world, ekf_allgather_fn allgather, void* ctx);
int ekf_shard_get_info(ekf_filter* f, ekf_shard_info* out);
/* ekf_update with z (2 M scalars) resident in device memory and the measured list on the host. */
int ekf_shard_update(ekf_filter* f, const void* d_z, const int* indices, int M, int plane_constraint);
/* All-gather of the row panels of Sigma + fresh partition (also done automatically, see above). */
int ekf_shard_rebalance(ekf_filter* f);

/* Raw device pointers for zero-copy plumbing (torch / RCCL): mu, the live Sigma buffer,
 * and its leading dimension (device storage is row-major, ld elements per row). */
void* ekf_device_mu(ekf_filter* f);
void* ekf_device_sigma(ekf_filter* f, int* ld);

/* ---- bundle adjustment of the key-frame map --------------------------------------------------
 * The reference's sparse_bundle_adjustment as sba_add drives it (SysSBA, sba.cpp): monocular projections, node 0
 * fixed, Levenberg-Marquardt on the reduced camera system, fp64.  One handle = one problem on its own stream.
 *  - nodes: (x y z qw qx qy qz), camera centre and attitude, normalised on add as Node::normRot (node.cpp:52-66);
 *  - points: (x y z) world;  projections: (node, point, u v).  A repeat of a (node, point) pair keeps the first
 *    keypoint (addMonoProj, sba.cpp:133-143); `added` (may be NULL) receives the number of new pairs;
 *  - arguments are checked before the device is touched: EKF_ERR_ARG for bad indices or non-finite values,
 *    EKF_ERR_CAPACITY beyond a capacity (the call then adds nothing);  capacity_nodes <= 1024 for the Cholesky
 *    solver (ekf_sba_create), no such limit for the PCG solver (below);
 *  - ekf_sba_run = SysSBA::doSBA(niter, lambda): *iterations = the iteration count, -1 for an empty problem;
 *    lambda > 0 sets the LM damping, otherwise the last run's value continues (initially 1e-4).  A non-positive
 *    pivot other than a projection-less free node (whose step is 0) is EKF_ERR_NUMERIC: the nodes and points stay
 *    at the last accepted iterate, *iterations = the iterations completed before it (the log holds their rows);
 *  - ekf_sba_cost: calcCost (sum of squared errors) and calcRMSCost(dist) (sba.cpp:289-360);
 *  - ekf_sba_get_log: per iteration of the last run, 5 doubles: cost before, cost after the step, lambda after,
 *    accepted (1 / 0), |x|^2;  *n = the number of rows (at most max_rows are written);
 *  - ekf_sba_profile / ekf_sba_get_profile: HIP-event milliseconds per phase (prep, Schur, assemble,
 *    factor + solve, update + cost) summed over the iterations since the last ekf_sba_profile, and per iteration.
 *
 * Robust cost and pruning.  All of it is off by default: huber = 0 and every projection valid.
 *  - ekf_sba_set_huber / ekf_sba_get_huber = SysSBA::huber (sba.h:113), in pixels; 0 switches it off, a negative
 *    or non-finite value is EKF_ERR_ARG.  For huber > 0 a projection with |e|^2 > huber^2 has its error scaled by
 *    sqrt((2 huber |e| - huber^2) / |e|^2) (calcErrMono_, proj.cpp:162-176).  The weighted error enters the cost, the
 *    RMS cost and its dist test (sba.cpp:300, :350), JcTE and bp of the linear system, and everything below; the
 *    Jacobian products are not weighted, as in the reference;
 *  - every stored projection has a validity flag (Proj::isValid), set on add.  An invalid one contributes to
 *    nothing (sba.cpp:299, :1212, :1242, :1255, :1513) but keeps its slot and still blocks a repeat of its
 *    (node, point) pair until ekf_sba_reduce_tracks erases it.  A point whose projections are all invalid is left
 *    alone like a point without any, and a free node whose projections are all invalid takes a zero step;
 *  - ekf_sba_count_bad = countBad(dist) (sba.cpp:416-440): *n = the valid projections whose weighted |e|^2 at the
 *    current nodes and points is >= dist^2 (the state doSBA leaves its stored errors at);  dist > 0;
 *  - ekf_sba_remove_bad = removeBad(dist) (sba.cpp:445-462): marks those invalid, *n = how many;
 *  - ekf_sba_reduce_tracks = reduceTracks (sba.cpp:467-502): erases the invalid projections, then every projection
 *    of a point left with fewer than 2; *cleared = the number of such points, those without any projection
 *    included.  ekf_sba_counts' third figure is the number of stored projections and falls accordingly;
 *  - ekf_sba_num_bad_points = numBadPoints (sba.cpp:389-411): valid projections whose unweighted error is exactly
 *    (0, 0), in practice the ones with p1.z <= 0;
 *  - ekf_sba_avg_error = calcAvgError (sba.cpp:365-386): the mean weighted |e| over the valid projections, NaN
 *    when there are none;
 *  - ekf_sba_get_projections: the stored projections, point-major and node ascending within a point (the order
 *    of the reference's tracks and their maps); *n = their number, at most max_rows rows are written, and each of
 *    node / point / uv (2 per row) / valid may be NULL.
 *
 * Linear solver.  ekf_sba_create gives the dense Cholesky solver.  ekf_sba_create_solver takes
 * doSBA's useCSparse choice: EKF_SBA_SOLVER_CHOLESKY (0, exactly ekf_sba_create, its 1024-node limit included) or
 * EKF_SBA_SOLVER_BPCG (3 = SBA_BLOCK_JACOBIAN_PCG): the reduced system kept as 6 x 6 blocks and solved by a conjugate
 * gradient preconditioned with the inverse diagonal blocks (jacobiBPCG<6>::doBPCG2, bpcg/bpcg.h:238-316).  A PCG handle
 * holds no dense matrix and takes any capacity_nodes up to INT_MAX / 64.  Any other solver value is EKF_ERR_ARG.
 *  - ekf_sba_set_cg / ekf_sba_get_cg: doSBA's initTol and maxCGiters (defaults 1e-8 and 100, sba.h:158-159);
 *    init_tol finite and >= 0, max_iters >= 1, otherwise EKF_ERR_ARG.  A Cholesky handle stores and ignores them;
 *  - a solve that ends at max_iters without reaching its bound is not an error: the step is applied and the cost
 *    test of the LM loop accepts or rejects it, as in the reference.  A diagonal block with a non-positive pivot is
 *    EKF_ERR_NUMERIC, with the state kept as described for ekf_sba_run;
 *  - ekf_sba_get_cg_log: per iteration of the last run, the CG iterations made, the r . s that ended the loop and
 *    the bound d0 it was compared with;  *n = the number of rows (0 on a Cholesky handle), at most max_rows are
 *    written, each of the three arrays may be NULL;
 *  - in ekf_sba_get_profile the "factor + solve" phase of a PCG handle is the block inverse and the CG. */
#define EKF_SBA_SOLVER_CHOLESKY 0
#define EKF_SBA_SOLVER_BPCG 3

typedef struct ekf_sba ekf_sba;
typedef struct ekf_sba_camera {
  double fx, fy, cx, cy;
} ekf_sba_camera;

int ekf_sba_create(const ekf_sba_camera* K, int capacity_nodes, int capacity_points, int capacity_projections,
                   int device, ekf_sba** out);
int ekf_sba_create_solver(const ekf_sba_camera* K, int capacity_nodes, int capacity_points, int capacity_projections,
                          int device, int solver, ekf_sba** out);
int ekf_sba_get_solver(const ekf_sba* s, int* solver);
int ekf_sba_set_cg(ekf_sba* s, double init_tol, int max_iters);
int ekf_sba_get_cg(const ekf_sba* s, double* init_tol, int* max_iters);
int ekf_sba_get_cg_log(const ekf_sba* s, int max_rows, int* cg_iters, double* dn_final, double* d0, int* n);
void ekf_sba_destroy(ekf_sba* s);
/* Message of the last failure (s may be NULL: last failure of ekf_sba_create). */
const char* ekf_sba_last_error(const ekf_sba* s);
int ekf_sba_add_nodes(ekf_sba* s, int n, const double* pose7);
int ekf_sba_add_points(ekf_sba* s, int n, const double* xyz);
int ekf_sba_add_projections(ekf_sba* s, int n, const int* node, const int* point, const double* uv, int* added);
int ekf_sba_counts(const ekf_sba* s, int* nodes, int* points, int* projections);
int ekf_sba_run(ekf_sba* s, int niter, double lambda, int* iterations);
int ekf_sba_cost(ekf_sba* s, double dist, double* sq_cost, double* rms);
int ekf_sba_set_huber(ekf_sba* s, double huber);
int ekf_sba_get_huber(const ekf_sba* s, double* huber);
int ekf_sba_count_bad(ekf_sba* s, double dist, int* n);
int ekf_sba_remove_bad(ekf_sba* s, double dist, int* n);
int ekf_sba_reduce_tracks(ekf_sba* s, int* cleared);
int ekf_sba_num_bad_points(ekf_sba* s, int* n);
int ekf_sba_avg_error(ekf_sba* s, double* avg);
int ekf_sba_get_projections(const ekf_sba* s, int max_rows, int* node, int* point, double* uv, unsigned char* valid,
                            int* n);
int ekf_sba_get_nodes(const ekf_sba* s, double* pose7);
int ekf_sba_get_points(const ekf_sba* s, double* xyz);
int ekf_sba_get_log(const ekf_sba* s, int max_rows, double* rows, int* n);
int ekf_sba_profile(ekf_sba* s, int enable);
int ekf_sba_get_profile(const ekf_sba* s, double* phase_ms, int max_iters, double* iter_ms, int* n);

/* ---- key-frame selection ----------------------------------------------------------------------
 * The per-frame rule of the reference's node (mono-slam monoslam_ransac.cpp:585-687 with quat2vec / poses_diff,
 * :40-60): after every update the caller passes its frame id, and the selector decides whether a frame becomes a key
 * frame, keeping the lowest-covariance pose of the half-to-full move_thresh window as the candidate.  The rule's state
 * (last pose, last rotation vector, the smallest covariance figure, the candidate's pose and 7 x 7 block) and the
 * candidate's / the emitted frame's image live on the device: one observe is one small launch on the filter's stream, one
 * image launch when a frame is set (ekf_set_frame) and ONE synchronisation.  Everything is fp32 whatever the filter's
 * dtype.  The selector belongs to the filter it was created for; it must be observed with that filter and may outlive it
 * only to be read and destroyed.
 *  - create: move_thresh finite and > 0 (the reference's MoveThresh is 18).  A sharded filter is EKF_ERR_STATE (here
 *    and at observe): Sigma[0:7,0:7] lives on one rank, a collective selector does not exist;
 *  - set_option: EKF_KF_OPT_KEEP_CURRENT_PROJECTIONS (0 / 1, default 0).  An emit of the CURRENT frame writes the single
 *    projection row "0 0 0" as the reference does (:640, :672); with 1 it carries the frame's own Point4sba rows;
 *  - observe: frame_id >= 0 is the caller's numbering (the reference counts from 1; ids below 5 may be emitted without
 *    a candidate).  *action = enum ekf_keyframe_action, *dist = poses_diff against the last key frame, *cov = the
 *    covariance figure of ekf_covariance_parameter in fp32 (dist / cov may be NULL).  The status words of earlier
 *    updates are read in the same round trip, as the getters do.  A failed observe leaves the rule's state, the
 *    candidate's and the last emitted record unchanged; when a frame was set, the image launch may have run on a record
 *    nobody read, so the stored images are no longer vouched for: get_image is EKF_ERR_STATE for the last emit and for
 *    an emit of the candidate stored before the failure (its id, pose, block and rows are still delivered);
 *  - get_emitted: the last emitted key frame: its id, pose (7), Sigma[0:7,0:7] (49, column-major as
 *    ekf_get_sigma_block) and its projection rows (real_index, u, v; 3 ints per row).  *n_rows = their number, at most
 *    max_rows rows are written; every output may be NULL.  EKF_ERR_STATE before the first emit;
 *  - get_image: the emitted key frame's image, image_height rows of image_width bytes, `stride` bytes apart: the one
 *    copy an image makes to the host.  EKF_ERR_STATE when nothing was emitted or no frame had been set for it;
 *  - create_raw: a selector that ALSO keeps the camera's own frame: two more device slots of
 *    raw_height x raw_width x channels bytes, allocated here.  When the filter holds a raw frame of exactly that geometry
 *    (ekf_set_frame_raw), observe moves it with a second image launch under the same action word: still one read-back
 *    and one synchronisation.  Otherwise it behaves as a selector of ekf_keyframe_create;
 *  - get_raw_image: the emitted key frame's raw image, raw_height rows of raw_width * channels bytes, `stride` bytes
 *    apart (the node's cv_ptr->image / Selected_Pose, monoslam_ransac.cpp:599-679).  EKF_ERR_STATE when the emitted frame
 *    has none: a plain selector, a frame set with ekf_set_frame, another geometry, or a failed observe in between (the
 *    rule of get_image);
 *  - get_state: last_pose (7), last_vrot (3), min_cov and the candidate id (0: none yet), each may be NULL;
 *  - reset: back to the state after create (options kept).
 * Null handles and out-of-range arguments are EKF_ERR_ARG before the device is touched. */
typedef struct ekf_keyframe ekf_keyframe;
enum ekf_keyframe_action {
  EKF_KF_NONE = 0,            /* nothing stored, nothing emitted                                                  */
  EKF_KF_CANDIDATE = 1,       /* this frame is the new candidate                                                  */
  EKF_KF_EMIT_CURRENT = 2,    /* key frame = this frame (its covariance is within 0.000085 of the candidate's)    */
  EKF_KF_EMIT_CANDIDATE = 3,  /* key frame = the stored candidate                                                 */
  EKF_KF_EMIT_FIRST = 4       /* key frame = this frame, no candidate and frame_id < 5                            */
};
#define EKF_KF_OPT_KEEP_CURRENT_PROJECTIONS 0

int ekf_keyframe_create(const ekf_filter* f, float move_thresh, ekf_keyframe** out);
void ekf_keyframe_destroy(ekf_keyframe* s);
/* Message of the last failure (s may be NULL: last failure of ekf_keyframe_create). */
const char* ekf_keyframe_last_error(const ekf_keyframe* s);
int ekf_keyframe_set_option(ekf_keyframe* s, int option, int value);
int ekf_keyframe_observe(ekf_keyframe* s, ekf_filter* f, int frame_id, int* action, float* dist, float* cov);
int ekf_keyframe_get_emitted(const ekf_keyframe* s, int* id, double* pose7, double* cov49, int max_rows, int* prj_rows,
                             int* n_rows);
int ekf_keyframe_create_raw(const ekf_filter* f, float move_thresh, int raw_width, int raw_height, int channels,
                            ekf_keyframe** out);
int ekf_keyframe_get_image(const ekf_keyframe* s, unsigned char* gray, int stride);
int ekf_keyframe_get_raw_image(const ekf_keyframe* s, unsigned char* pixels, int stride);
int ekf_keyframe_get_state(const ekf_keyframe* s, float* last_pose7, float* last_vrot3, float* min_cov, int* candidate_id);
int ekf_keyframe_reset(ekf_keyframe* s);

/* ---- rectification for pinhole consumers ------------------------------------------------------
 * The filter models lens distortion (k1 k2 k3 p1 p2 of ekf_config); ekf_sba_* and the dense step (ekf_dense_*) are pinhole.  These
 * entry points deliver, on demand, images, pixel coordinates and ONE pinhole K that agree.  The reference has no
 * counterpart (its key frames and Point4sba rows stay distorted).  Nothing here runs per frame, changes the filter or
 * counts as a launch kind; ekf_abi_version() stays 6 (additions only).
 *  - `raw` selects the resolution: 0 = the matcher frame (image_width x image_height, factor s = 1), 1 = the raw frame
 *    of ekf_set_frame_raw / ekf_keyframe_create_raw (width x height x channels, s = ekf_config.scale).  Matcher pixel u
 *    and raw pixel X: u = (X + 0.5) / s - 0.5.  Any other value is EKF_ERR_ARG;
 *  - ekf_rectified_camera: K(raw = 0) = (fx, fy, u0, v0) of the config; K(raw = 1) = (fx s, fy s, (u0 + 0.5) s - 0.5,
 *    (v0 + 0.5) s - 0.5).  raw = 1 before any raw frame was set is EKF_ERR_STATE (the raw geometry is unknown);
 *  - ekf_get_frame_rectified: the frame the filter holds, undistorted by ONE launch on the filter's stream (fp64 map,
 *    5-bit bilinear weights, a source position outside the image gives 0: DESIGN.md §14 pins every operation), rows of
 *    width * channels bytes, `stride` bytes apart.  EKF_ERR_STATE without a frame, or for raw = 1 without a raw frame
 *    (a later ekf_set_frame drops it);
 *  - ekf_undistort_pixels: n pixels (u, v) of resolution `raw` (host, 2 doubles each) -> where the pinhole K of that
 *    resolution sees the same ray: the 50 fixed-point iterations of the filter's own camera model, in fp64 on the
 *    device.  A non-finite input gives NaN, NaN.  n = 0 is a no-op; raw = 1 as for ekf_rectified_camera;
 *  - ekf_keyframe_get_image_rectified: the last emitted key frame's image (raw = 0) or raw image (raw = 1), rectified
 *    on the device from the emit slot.  EKF_ERR_STATE whenever ekf_keyframe_get_image / ekf_keyframe_get_raw_image
 *    refuse;
 *  - ekf_keyframe_get_emitted_rectified: the rows of ekf_keyframe_get_emitted, same selection and order, as the
 *    undistorted FLOAT track centres (not the truncated ints) in resolution `raw`: 2 doubles per row.  *rows = their
 *    number (at most max_rows are written); the "0 0 0" placeholder row is zero rows of coordinates.  EKF_ERR_STATE
 *    before the first emit, and for raw = 1 on a selector that is not a raw one.
 * The selector's two getters use the lens model and scale its filter had at create and run on the default stream (the
 * selector may outlive the filter).  A sharded filter is allowed everywhere: every rank holds the frame, there is no
 * collective.  Argument errors are EKF_ERR_ARG before the device is touched. */
int ekf_rectified_camera(const ekf_filter* f, int raw, ekf_sba_camera* K);
int ekf_get_frame_rectified(ekf_filter* f, int raw, unsigned char* out, int stride);
int ekf_undistort_pixels(ekf_filter* f, int raw, const double* uv, int n, double* out);
int ekf_keyframe_get_image_rectified(const ekf_keyframe* s, int raw, unsigned char* out, int stride);
int ekf_keyframe_get_emitted_rectified(const ekf_keyframe* s, int raw, int max_rows, double* uv, int* rows);

/* ---- dense plane-sweep depth maps for key frames ----------------------------------------------
 * Multi-view plane-sweep stereo on rectified key frames: one handle holds up to max_views (<= 16) views of one size
 * width x height, each an 8-bit grey pinhole image, K = (fx, fy, cx, cy) and a pose in the bundle adjuster's node
 * convention (camera centre t, q = (w, x, y, z), normalised on entry; x_cam = R^T (X - t)).  The reference has no
 * counterpart.  DESIGN.md §15.1 pins every operation (fp64 coordinates, integer costs); tests/dense_oracle.py restates
 * it.  Nothing here touches a filter, counts as a launch kind or runs a collective; ekf_abi_version() stays 6
 * (additions only).  Everything runs on the default stream of the handle's device.
 *  - create: 1 <= width, height <= 8192, 1 <= max_views <= 16;
 *  - set_view: `img` = height rows of width bytes, `pitch` (>= width) bytes apart, on the host; K finite with fx, fy > 0;
 *    pose7 finite with q != 0.  set_view_device: the same from device memory, enqueued without a host synchronisation.
 *    set_view_from_keyframe: the selector's last emitted key frame, rectified by one k_frame_rectify launch straight
 *    into the slot, with the selector's rectified camera of resolution `raw` as K; the selector's image size at that
 *    resolution must be the handle's and a raw selector must be 1-channel (otherwise EKF_ERR_ARG); EKF_ERR_STATE
 *    whenever ekf_keyframe_get_image / ekf_keyframe_get_raw_image would refuse.  set_pose: a new pose for a set slot
 *    (after bundle adjustment), no upload.  Each of them invalidates the slot's swept and filtered maps.  get_view: what
 *    a set slot holds: the image (`pitch` bytes per row), K and the pose with q normalised; each output may be NULL;
 *  - sweep: the depth map of view `ref` against the n_src views src[]: `planes` fronto-parallel planes of the
 *    reference camera, uniform in inverse depth from w_min to w_max; truncated absolute differences (`trunc`) summed
 *    over the sources and a (2 radius + 1)^2 window; the first plane of least cost wins, refined by a parabola through
 *    its neighbours.  One launch.  Limits (EKF_ERR_ARG before the device is touched): planes 2..1024, radius 0..4,
 *    trunc 1..255, n_src 1..8, 0 < w_min < w_max finite, ref not among src, no slot twice in src, every slot in range
 *    and set;
 *  - filter: keeps a pixel of `ref` whose swept depth, projected into each source, lands within rel_tol (relative) of
 *    that source's swept depth in at least min_agree (1..n_src) sources; reads swept maps only and writes the separate
 *    filtered map of `ref`, so the order of calls does not matter.  EKF_ERR_STATE when a named slot has not been swept
 *    since its image or pose last changed;
 *  - get_depth: the swept (filtered = 0) or filtered (1) map of a slot, tight rows: depth float32 (0 = none), plane
 *    int32 (-1 = none), and of the sweep cost uint32 and views uint8; every output may be NULL.  get_points: height x
 *    width x 3 doubles, the world points of that map, NaN where there is no depth.  EKF_ERR_STATE without that map;
 *  - profile / get_profile: HIP-event milliseconds and launch counts of k_plane_sweep ([0]) and
 *    k_depth_filter_points ([1]) since the last ekf_dense_profile (each timed launch is synchronised).  The kernel of
 *    [1] also does the back-projection: every ekf_dense_get_points made while profiling adds its launch and its time
 *    to [1], so fetch points outside the profiled span when [1] is to be read as the filter's time alone. */
typedef struct ekf_dense ekf_dense;
int ekf_dense_create(int width, int height, int max_views, int device, ekf_dense** out);
void ekf_dense_destroy(ekf_dense* h);
/* Message of the last failure (h may be NULL: last failure of ekf_dense_create). */
const char* ekf_dense_last_error(const ekf_dense* h);
int ekf_dense_set_view(ekf_dense* h, int slot, const unsigned char* img, int pitch, const double* K, const double* pose7);
int ekf_dense_set_view_device(ekf_dense* h, int slot, const void* d_img, int pitch, const double* K, const double* pose7);
int ekf_dense_set_view_from_keyframe(ekf_dense* h, int slot, const ekf_keyframe* selector, int raw, const double* pose7);
int ekf_dense_set_pose(ekf_dense* h, int slot, const double* pose7);
int ekf_dense_get_view(const ekf_dense* h, int slot, unsigned char* img, int pitch, double* K, double* pose7);
int ekf_dense_sweep(ekf_dense* h, int ref, const int* src, int n_src, double w_min, double w_max, int planes, int radius,
                    int trunc);
int ekf_dense_filter(ekf_dense* h, int ref, const int* src, int n_src, double rel_tol, int min_agree);
int ekf_dense_get_depth(ekf_dense* h, int slot, int filtered, float* depth, int* plane, unsigned int* cost,
                        unsigned char* views);
int ekf_dense_get_points(ekf_dense* h, int slot, int filtered, double* xyz);
int ekf_dense_profile(ekf_dense* h, int enable);
int ekf_dense_get_profile(const ekf_dense* h, double* kernel_ms, long long* launches);

/* ---- fusion of depth maps into a TSDF volume and a triangle mesh -------------------------------
 * The last stage of the reconstruction: the depth maps of the key frames (ekf_dense_*, or any host arrays) are
 * integrated into one truncated signed distance volume on the device, and an oriented, watertight triangle mesh is
 * extracted from it by marching tetrahedra.  The reference has no counterpart.  DESIGN.md §16.1 pins every operation
 * (fp64 coordinates rounded once in the written order, one fp32 add per voxel and map, no atomics, a fixed output
 * order); tests/fusion_oracle.py restates it.  Nothing here touches a filter, counts as a launch kind or runs a
 * collective; ekf_abi_version() stays 6 (additions only).  Everything runs on the default stream of the handle's device.
 *  - create: nx x ny x nz voxels; the centre of voxel (i, j, k) is origin + (i, j, k) voxel; linear index
 *    i + nx (j + ny k).  Each voxel holds sum (float), cnt (unsigned short) and gsum (unsigned int).  EKF_ERR_ARG before
 *    the device is touched: a dimension outside 2..1024, nx ny nz > 2^28, voxel or trunc not finite or <= 0, origin
 *    not finite;
 *  - integrate: the swept (filtered = 0) or filtered (1) map of a slot of a dense handle, straight from its device
 *    buffers, with the slot's image, K and pose.  A dense handle on another device is EKF_ERR_ARG; a slot without that
 *    map is EKF_ERR_STATE by the rules of ekf_dense_get_depth.  integrate_host: `depth` = height tight rows of width
 *    floats (0 = none), `img` = height rows of width bytes `pitch` (>= width) bytes apart, 1 <= width, height <= 8192,
 *    K = (fx, fy, cx, cy) finite with fx, fy > 0, pose7 as for ekf_dense_set_view.  One k_tsdf_integrate launch each.
 *    A handle integrates at most 65535 maps; the next one is EKF_ERR_CAPACITY and changes nothing;
 *  - reset: clears the three planes and the map counter;
 *  - get_volume / set_volume: the three planes (nx ny nz elements each) and the map counter; every pointer may be
 *    NULL.  They exist for tests, as ekf_set_state does.  set_volume: `maps` = -1 keeps the counter, 0..65535 sets it;
 *    the counter is then raised to the largest count given, so that a voxel's count cannot wrap;
 *  - extract: marching tetrahedra over every cell whose eight corners have cnt >= min_count (1..65535); reports the
 *    number of triangles.  Three launches (k_tsdf_count, k_tsdf_scan, k_tsdf_emit) and one 8-byte read-back; a failed
 *    allocation of the mesh buffers is EKF_ERR_DEVICE and leaves the previous mesh and the volume as they were;
 *  - get_mesh: the first min(n_tri, max_tri) triangles in the fixed order (cells by linear index of their corner 0,
 *    tetrahedra 0..5, table order): xyz = 3 x 3 doubles a triangle, key = 3 vertex keys (equal keys: bit-equal
 *    vertices), grey = 3 bytes; every pointer may be NULL.  EKF_ERR_STATE before an extract or after the volume changed
 *    since the last one (integrate, reset, set_volume);
 *  - profile / get_profile: HIP-event milliseconds and launch counts of k_tsdf_integrate ([0]), k_tsdf_count ([1]),
 *    k_tsdf_scan ([2]) and k_tsdf_emit ([3]) since the last ekf_fusion_profile (each timed launch is synchronised). */
typedef struct ekf_fusion ekf_fusion;
int ekf_fusion_create(int nx, int ny, int nz, const double* origin, double voxel, double trunc, int device, ekf_fusion** out);
void ekf_fusion_destroy(ekf_fusion* h);
/* Message of the last failure (h may be NULL: last failure of ekf_fusion_create). */
const char* ekf_fusion_last_error(const ekf_fusion* h);
int ekf_fusion_integrate(ekf_fusion* h, ekf_dense* dense, int slot, int filtered);
int ekf_fusion_integrate_host(ekf_fusion* h, const float* depth, const unsigned char* img, int pitch, int width, int height,
                              const double* K, const double* pose7);
int ekf_fusion_reset(ekf_fusion* h);
int ekf_fusion_get_volume(ekf_fusion* h, float* sum, unsigned short* cnt, unsigned int* gsum, int* maps);
int ekf_fusion_set_volume(ekf_fusion* h, const float* sum, const unsigned short* cnt, const unsigned int* gsum, int maps);
int ekf_fusion_extract(ekf_fusion* h, int min_count, unsigned long long* n_tri);
int ekf_fusion_get_mesh(ekf_fusion* h, double* xyz, unsigned long long* key, unsigned char* grey, unsigned long long max_tri);
int ekf_fusion_profile(ekf_fusion* h, int enable);
int ekf_fusion_get_profile(const ekf_fusion* h, double* kernel_ms, long long* launches);

/* ---- ray casting of the TSDF volume into depth, normal and grey images ------------------------------
 * The view of the fused surface from any pinhole pose: per pixel the camera-z depth of the first outside-to-inside
 * crossing of the trilinearly interpolated volume, the unit normal there (world frame, towards free space) and the
 * interpolated grey value; depth 0, normal 0, grey 0 where the ray finds none.  The functions take an ekf_fusion handle.
 * DESIGN.md §17.1 pins every operation (fp64 coordinates rounded once in the written order, samples at
 * z_near + n step, no atomics); tests/raycast_oracle.py restates it.  Additions only: ekf_abi_version() stays 6.
 *  - render: a width x height view with K = (fx, fy, cx, cy) and pose7 as for ekf_dense_set_view, samples
 *    n = 0 .. floor((z_far - z_near) / step) of the camera-z depth, over the voxels with cnt >= min_count.  The images
 *    stay in device buffers of the handle (grow-only).  One k_tsdf_raycast launch, and one k_tsdf_mean launch before it
 *    when the volume or min_count changed since the last render.  The mesh of the last extract stays valid.
 *    EKF_ERR_ARG before the device is touched: width or height outside 1..8192, K not finite or fx, fy = 0, a pose that
 *    ekf_dense_set_view would refuse, step not finite or <= 0, not 0 <= z_near < z_far finite, more than 65536 samples,
 *    min_count outside 1..65535.  A failed allocation is EKF_ERR_DEVICE; either leaves the volume, the mesh and the
 *    previous render as they were;
 *  - render_view: the same with the size, K and pose of a slot of a dense handle.  A dense handle on another device is
 *    EKF_ERR_ARG; a slot that was never set is EKF_ERR_STATE;
 *  - get: depth = height tight rows of width floats, normal = 3 floats a pixel, grey = one byte a pixel; every pointer
 *    may be NULL.  EKF_ERR_STATE before a render or after the volume changed since the last one (integrate, reset,
 *    set_volume);
 *  - get_profile: HIP-event milliseconds and launch counts of k_tsdf_mean ([0]) and k_tsdf_raycast ([1]) since the last
 *    ekf_fusion_profile, which switches them on and off with the four entries of ekf_fusion_get_profile. */
int ekf_raycast_render(ekf_fusion* h, int width, int height, const double* K, const double* pose7, double z_near, double z_far,
                       double step, int min_count);
int ekf_raycast_render_view(ekf_fusion* h, ekf_dense* dense, int slot, double z_near, double z_far, double step, int min_count);
int ekf_raycast_get(ekf_fusion* h, float* depth, float* normal, unsigned char* grey, int* width, int* height);
int ekf_raycast_get_profile(const ekf_fusion* h, double* kernel_ms, long long* launches);

/* ---- colour through the dense chain ----------------------------------------------------------------
 * The three stages above carry one grey value a sample; these additions carry the camera's colour beside it.  Channel
 * order is B, G, R everywhere (as ekf_set_frame_raw).  DESIGN.md §18.1 pins every operation (integer colour sums, fp64
 * blends rounded as the grey ones, no atomics); tests/colour_oracle.py restates it.  No grey result, launch or prototype
 * above changes; ekf_abi_version() stays 6 (additions only).  The ekf_colour_* functions take an ekf_fusion handle: they
 * are what a colour volume adds to ekf_fusion_* and ekf_raycast_*, in a family of their own so that those two lists stay
 * as they are.
 *  - ekf_dense_set_view_colour / _device: as ekf_dense_set_view / _device with `bgr` = height rows of width x 3 bytes,
 *    `pitch` (>= 3 width) bytes apart.  The slot keeps the colour image; the grey image the sweep reads is made from it on
 *    the device by one k_bgr_to_grey launch: (b 1868 + g 9617 + r 4899 + 8192) >> 14 a pixel, the conversion of
 *    ekf_set_frame_raw.  ekf_dense_set_view_colour_from_keyframe: the last emitted raw key frame of a 3-channel raw
 *    selector, rectified by one k_frame_rectify launch straight into the slot's colour image, K the selector's raw
 *    rectified camera; any other selector is EKF_ERR_ARG, and EKF_ERR_STATE whenever ekf_keyframe_get_raw_image would
 *    refuse (ekf_dense_set_view_from_keyframe keeps refusing three channels).  Each of them invalidates the slot's maps;
 *    ekf_dense_set_view, _device and _from_keyframe drop the slot's colour;
 *  - ekf_dense_get_view_colour: the colour image of a slot (`pitch` bytes per row); bgr = NULL only asks whether the slot
 *    has one.  EKF_ERR_STATE if it has none;
 *  - ekf_colour_create: ekf_fusion_create for a colour volume, which keeps three more planes of unsigned int: the
 *    sums of B, G and R (65535 maps x 255 < 2^32).  ekf_colour_has: 1 for such a handle, otherwise 0.
 *    ekf_fusion_integrate on a colour volume runs k_tsdf_integrate_colour: the same voxels, sum and cnt; gsum takes the
 *    grey of the pixel, the colour planes its channels.  A slot without colour and ekf_fusion_integrate_host add their
 *    grey value to all three colour planes.  A plain volume behaves as before whatever the slot holds;
 *  - ekf_colour_integrate_host: ekf_fusion_integrate_host with `bgr` = height rows of width x 3 bytes `pitch`
 *    (>= 3 width) bytes apart; gsum takes the conversion above of each pixel;
 *  - ekf_colour_get_volume / ekf_colour_set_volume: the three colour planes back to back (3 nx ny nz elements);
 *  - ekf_fusion_extract on a colour volume launches k_tsdf_colour_vertices after k_tsdf_emit (not for an empty mesh);
 *    ekf_colour_get_mesh: 3 x 3 bytes a triangle, B, G, R of each vertex, in the order of ekf_fusion_get_mesh,
 *    which still delivers the grey; EKF_ERR_STATE by its rules;
 *  - ekf_raycast_render / _render_view on a colour volume make one k_tsdf_raycast_colour launch in place of
 *    k_tsdf_raycast: the same depth, normal and grey, and a colour image; ekf_colour_get_render: 3 bytes a pixel, 0 0 0
 *    without a hit; EKF_ERR_STATE by the rules of ekf_raycast_get;
 *  - every function that only a colour volume answers is EKF_ERR_STATE on a plain volume (after the argument checks) and
 *    leaves all earlier results readable;
 *  - ekf_colour_get_profile: HIP-event milliseconds and launch counts of k_tsdf_integrate_colour ([0]),
 *    k_tsdf_colour_vertices ([1]) and k_tsdf_raycast_colour ([2]) since the last ekf_fusion_profile. */
int ekf_dense_set_view_colour(ekf_dense* h, int slot, const unsigned char* bgr, int pitch, const double* K, const double* pose7);
int ekf_dense_set_view_colour_device(ekf_dense* h, int slot, const void* d_bgr, int pitch, const double* K, const double* pose7);
int ekf_dense_set_view_colour_from_keyframe(ekf_dense* h, int slot, const ekf_keyframe* selector, const double* pose7);
int ekf_dense_get_view_colour(const ekf_dense* h, int slot, unsigned char* bgr, int pitch);
int ekf_colour_create(int nx, int ny, int nz, const double* origin, double voxel, double trunc, int device, ekf_fusion** out);
int ekf_colour_has(const ekf_fusion* h);
int ekf_colour_integrate_host(ekf_fusion* h, const float* depth, const unsigned char* bgr, int pitch, int width, int height,
                              const double* K, const double* pose7);
int ekf_colour_get_volume(ekf_fusion* h, unsigned int* csum);
int ekf_colour_set_volume(ekf_fusion* h, const unsigned int* csum);
int ekf_colour_get_mesh(ekf_fusion* h, unsigned char* bgr, unsigned long long max_tri);
int ekf_colour_get_profile(const ekf_fusion* h, double* kernel_ms, long long* launches);
int ekf_colour_get_render(ekf_fusion* h, unsigned char* bgr);

/* ---- semi-global cost aggregation for the dense sweep ------------------------------------------------
 * An opt-in second sweep beside ekf_dense_sweep for images with textureless regions, where every plane costs the same and
 * the pixel-wise winner is plane 0: the windowed cost volume C of §15.1 is written to device memory, path costs
 *   L_r(p, d) = C_d(p) + min(L_r(p-r, d), L_r(p-r, d-1) + p1, L_r(p-r, d+1) + p1, m + p2) - m,  m = min_i L_r(p-r, i)
 * (L_r = C where p - r lies outside the image) are summed over the directions r = (dx, dy) = (1,0) (-1,0) (0,1) (0,-1)
 * (1,1) (-1,-1) (1,-1) (-1,1) -- paths = 4 takes the first four -- and the winner of the sum S is taken by the rules of
 * ekf_dense_sweep (first plane of least S, the parabola on S, views = valid warps of the pixel at the winning plane).
 * Integers throughout; tests/sgm_oracle.py restates it.  No other result, launch or prototype changes; ekf_abi_version()
 * stays 6 (additions only).
 *  - ekf_dense_sweep_sgm: writes the swept map of `ref` (depth, plane, cost = S of the winner, views) and marks the slot
 *    swept and not filtered, exactly as ekf_dense_sweep does, so ekf_dense_filter, ekf_dense_get_depth / _get_points,
 *    ekf_fusion_integrate and ekf_raycast_render_view consume it unchanged.  Launches: k_sweep_volume, one k_sgm_path per
 *    direction, k_sgm_winner.  EKF_ERR_ARG before the device is touched: everything ekf_dense_sweep refuses, not
 *    1 <= p1 <= p2 <= 2^20, paths other than 4 or 8, width x height x planes > 2^28.  The handle keeps one raw and one
 *    aggregated volume (4 bytes an element each, and 1 byte an element of valid-view counts), grow-only; a failed
 *    allocation is EKF_ERR_DEVICE and leaves the slot's earlier maps readable;
 *  - ekf_dense_get_volume: planes x height x width values, plane-major, of the raw (aggregated = 0) or the aggregated
 *    (1) volume.  EKF_ERR_STATE unless `slot` is the slot of the handle's last successful ekf_dense_sweep_sgm and no
 *    setter or sweep of that slot came after it;
 *  - ekf_dense_get_sgm_profile: HIP-event milliseconds and launch counts of 10 kinds since the last ekf_dense_profile:
 *    k_sweep_volume ([0]), k_sgm_path of direction r0 .. r7 ([1] .. [8]) and k_sgm_winner ([9]).  ekf_dense_get_profile
 *    keeps its two kinds: a semi-global sweep adds nothing to them. */
int ekf_dense_sweep_sgm(ekf_dense* h, int ref, const int* src, int n_src, double w_min, double w_max, int planes, int radius,
                        int trunc, int p1, int p2, int paths);
int ekf_dense_get_volume(ekf_dense* h, int slot, int aggregated, unsigned int* out);
int ekf_dense_get_sgm_profile(const ekf_dense* h, double* kernel_ms, long long* launches);

/* ---- census matching cost for the dense sweeps --------------------------------------------------------
 * An opt-in matching cost for key frames whose exposure or gain differ, where the absolute grey difference of §15.1 fails:
 * the Hamming distance of census descriptors.  The descriptor T(X, Y) of an 8-bit image is a 64-bit word: for the offsets
 * (dx, dy) with dy = -3 .. 3 outer and dx = -4 .. 4 inner, (0, 0) skipped, bit b = 0 .. 61 in that order is 1 iff
 * (X + dx, Y + dy) lies inside the image and I(X + dx, Y + dy) < I(X, Y); bits 62 and 63 are 0.  The warp, its validity
 * test and (qx, qy) are those of ekf_dense_sweep; the source's descriptor is read at the nearest pixel jx = (qx + 16) >> 5,
 * jy = (qy + 16) >> 5, and c = min(popcount(T_r(X, Y) xor T_v(jx, jy)), trunc), an invalid warp costing trunc.  Everything
 * after c -- the sum over the views, the window, the valid-view count, the winner, its refinement, views = 0, the limits,
 * and for the semi-global sweep the path costs -- is that of ekf_dense_sweep / ekf_dense_sweep_sgm.  Integers throughout;
 * tests/census_oracle.py restates it.  The default cost stays the absolute difference: no other result, launch, profile
 * count or prototype changes; ekf_abi_version() stays 6 (additions only).
 *  - ekf_dense_sweep_census: ekf_dense_sweep with the census cost: the same arguments, argument checks, state rules and
 *    maps.  Each slot keeps a descriptor buffer (8 bytes a pixel, allocated on first use) that every setter of the slot's
 *    image invalidates and ekf_dense_set_pose does not; the call first launches k_census for the reference and for every
 *    source whose descriptors are stale, then k_plane_sweep_census.  A failed allocation is EKF_ERR_DEVICE and leaves the
 *    slot's earlier maps readable;
 *  - ekf_dense_sweep_sgm_census: ekf_dense_sweep_sgm with the census cost (k_sweep_volume_census, then the unchanged
 *    k_sgm_path and k_sgm_winner); ekf_dense_get_volume works after it;
 *  - ekf_dense_get_census: the width x height descriptors of a set slot, computed first if they are stale.  EKF_ERR_STATE
 *    for a slot that is not set;
 *  - ekf_dense_get_census_profile: HIP-event milliseconds and launch counts of 3 kinds since the last ekf_dense_profile:
 *    k_census ([0]), k_plane_sweep_census ([1]) and k_sweep_volume_census ([2]).  ekf_dense_get_profile keeps its two kinds
 *    and ekf_dense_get_sgm_profile its ten: a census sweep adds nothing to the former, and a semi-global census sweep counts
 *    its directions and its winner under the latter ([1] .. [9]) and nothing under k_sweep_volume ([0]). */
int ekf_dense_sweep_census(ekf_dense* h, int ref, const int* src, int n_src, double w_min, double w_max, int planes, int radius,
                           int trunc);
int ekf_dense_sweep_sgm_census(ekf_dense* h, int ref, const int* src, int n_src, double w_min, double w_max, int planes,
                               int radius, int trunc, int p1, int p2, int paths);
int ekf_dense_get_census(ekf_dense* h, int slot, unsigned long long* out);
int ekf_dense_get_census_profile(const ekf_dense* h, double* kernel_ms, long long* launches);

/* ---- best-K source selection for the dense sweeps ------------------------------------------------------
 * The sweeps above sum the matching cost over ALL sources, an invalid warp costing trunc: at the image border of a moving
 * camera, behind a depth step, or with a source that looks elsewhere, planes on which the warps are valid then beat planes on
 * which they match.  This opt-in sweep keeps, per pixel and plane, the n_best cheapest sources (Kang & Szeliski).  The warp,
 * its validity test, (qx, qy), the per-pixel cost c_v of source v (absolute difference, or census Hamming distance; an invalid
 * warp costs trunc), the planes and the limits are those of ekf_dense_sweep / ekf_dense_sweep_census.  Then
 *   C_k^v(p) = the sum of c_v over the (2 radius + 1)^2 window around p, positions outside the image contributing nothing
 *              (<= 81 * 255 = 20 655);
 *   C_k(p)   = the sum of the n_best smallest of C_k^0(p) .. C_k^{n_src - 1}(p)  (only the sum is defined: ties need no rule);
 * for n_best = n_src, C_k(p) is the value of the existing sweeps, element for element.  views stays the number of sources
 * whose warp of p itself is valid on the winning plane.  Everything after C is the existing path on the new numbers: the first
 * plane of least cost and the parabola, views = 0 giving plane -1 and depth 0, and with paths of 4 or 8 the path costs of
 * ekf_dense_sweep_sgm and the winner of S.  Integers throughout; tests/best_oracle.py restates it.  No default, result,
 * launch, profile count or prototype of the calls above changes; ekf_abi_version() stays 6 (additions only).
 *  - ekf_dense_sweep_best: census is 0 or 1.  paths = 0 takes the pixel-wise winner, and p1 and p2 must then be 0; paths = 4 or
 *    8 aggregates as ekf_dense_sweep_sgm does, with its checks on p1, p2 and the volume size, and ekf_dense_get_volume works
 *    afterwards.  EKF_ERR_ARG, before the device is touched, for everything the corresponding existing sweep refuses, n_best
 *    outside 1 .. n_src, and census or paths outside their sets.  State rules, allocation failures (EKF_ERR_DEVICE, the
 *    earlier maps still readable) and invalidation are those of the existing sweeps.  The call always launches the kernels
 *    below, also for n_best = n_src;
 *  - ekf_dense_get_best_profile: HIP-event milliseconds and launch counts of 4 kinds since the last ekf_dense_profile:
 *    k_plane_sweep_best ([0]), k_plane_sweep_best_census ([1]), k_sweep_volume_best ([2]), k_sweep_volume_best_census ([3]).
 *    k_census keeps counting under ekf_dense_get_census_profile [0], the directions and the winner under
 *    ekf_dense_get_sgm_profile [1] .. [9]; ekf_dense_get_profile gains nothing. */
int ekf_dense_sweep_best(ekf_dense* h, int ref, const int* src, int n_src, int n_best, double w_min, double w_max,
                         int planes, int radius, int trunc, int census, int paths, int p1, int p2);
int ekf_dense_get_best_profile(const ekf_dense* h, double* kernel_ms, long long* launches);

/* ---- runner-up cost and uniqueness test for the dense sweeps ------------------------------------------
 * The sweeps above keep the plane of least cost and forget how close the other planes came; only the geometric filter
 * rejects a depth, and where the reference image has no texture every view makes the same arbitrary choice and the views
 * agree.  Opt-in, a sweep also records the runner-up: for a pixel with cost curve C_0 .. C_{D-1} and winner k* (the smallest
 * k of least cost),
 *   C2 = min { C_k : |k - k*| > 1 },   0xFFFFFFFF ("absent") where no such plane exists (planes <= 3 only),
 * on the curve the sweep takes its winner from: the summed window cost, the census cost, the best-K cost, or the aggregate S
 * of ekf_dense_sweep_sgm.  C2 is defined for every pixel, whatever views says.  The uniqueness test with u in 0 .. 100 (per
 * cent) passes a pixel iff C2 is absent or (C2 - C1) 100 >= u C2 in 64-bit integers, C1 being the pixel's cost: u = 0 passes
 * everything, a flat curve (C2 = C1) fails every u > 0, the curve that is 0 on every plane included (where the inequality
 * alone reads 0 >= 0).  tests/unique_oracle.py restates it.  No default, result, launch,
 * profile count or prototype of the calls above changes while the switch is off; ekf_abi_version() stays 6 (additions only).
 *  - ekf_dense_keep_runner_up: a switch of the handle, off at creation.  While it is on, every sweep entry point above
 *    (plain, census, best, sgm, sgm_census) launches the twin of its winner kernel, which writes the same four maps byte for
 *    byte and the slot's runner-up map; while it is off, a sweep launches exactly what it did and drops the slot's runner-up
 *    map.  A setter or a sweep of a slot takes its runner-up map together with its swept maps;
 *  - ekf_dense_get_runner_up: the width x height runner-up costs of a slot.  EKF_ERR_STATE if the slot's last sweep did not
 *    record them or the slot was invalidated since;
 *  - ekf_dense_filter_unique: ekf_dense_filter, with all of its argument and state rules, keeping a pixel iff it passed
 *    before AND the reference view's own pixel passes the uniqueness test; the sources' swept depths are read as before.
 *    uniqueness outside 0 .. 100: EKF_ERR_ARG before the device is touched.  uniqueness > 0 on a reference slot without a
 *    runner-up map: EKF_ERR_STATE.  uniqueness = 0 needs no map, launches k_depth_filter_points and equals ekf_dense_filter
 *    byte for byte;
 *  - ekf_dense_get_unique_profile: HIP-event milliseconds and launch counts of 6 kinds since the last ekf_dense_profile:
 *    k_plane_sweep_unique ([0]), k_plane_sweep_census_unique ([1]), k_plane_sweep_best_unique ([2]),
 *    k_plane_sweep_best_census_unique ([3]), k_sgm_winner_unique ([4]), k_depth_filter_unique ([5]).  A twin counts here and
 *    not where the kernel it stands in for does; every other kernel of a sweep keeps counting where it did. */
int ekf_dense_keep_runner_up(ekf_dense* h, int enable);
int ekf_dense_get_runner_up(ekf_dense* h, int slot, unsigned int* out);
int ekf_dense_filter_unique(ekf_dense* h, int ref, const int* src, int n_src, double rel_tol, int min_agree, int uniqueness);
int ekf_dense_get_unique_profile(const ekf_dense* h, double* kernel_ms, long long* launches);

/* ---- speckle filter: connected segments of a depth map -------------------------------------------------
 * What the geometric filter and the uniqueness test leave of a wrong surface are islands of a few pixels whose neighbours
 * were all dropped; the fusion gives them full weight.  The speckle filter segments a map into connected regions of
 * similar plane and drops the small ones.  For a plane map of height x width int with its depth map, min_size >= 1 and
 * max_diff >= 0: a pixel is valid iff plane >= 0; two 4-neighbours are linked iff both are valid and
 * |plane_a - plane_b| <= max_diff (the difference in 64 bits); a segment is a connected component of the links (a ramp
 * 0, 1, 2, ... is one segment at max_diff = 1); a valid pixel's label is the least linear index y width + x of its
 * segment and its size the segment's pixel count; an invalid pixel has label 0xFFFFFFFF and size 0.  The filter sets
 * depth = 0 and plane = -1 where size < min_size and leaves every other element bit for bit.  min_size = 1 changes nothing,
 * the filter is idempotent, and labels, sizes and the output do not depend on any order of execution.
 * tests/speckle_oracle.py restates it.  Four launches a call whatever the map holds: k_speckle_label, k_speckle_merge,
 * k_speckle_count, k_speckle_apply.  Opt-in: nothing above calls it, and no default, result, launch, profile count or
 * prototype of the calls above changes; ekf_abi_version() stays 6 (additions only).
 *  - ekf_dense_filter_speckle: filters the slot's FILTERED map in place; ekf_dense_get_depth(.., filtered = 1),
 *    ekf_dense_get_points, ekf_fusion_integrate(.., filtered = 1) and ekf_raycast_render_view then read it as they read any
 *    filtered map.  The swept map, which the filters of other views read, is never touched.  EKF_ERR_ARG before the device
 *    is touched: slot out of range, min_size outside 1 .. 2^26, max_diff outside 0 .. 1023.  EKF_ERR_STATE: the slot has no
 *    filtered map.  A later ekf_dense_filter / ekf_dense_filter_unique of the slot starts again from the swept map;
 *  - ekf_dense_get_segments: the height x width labels and sizes BEFORE the removal of the handle's last
 *    ekf_dense_filter_speckle; either pointer may be NULL.  EKF_ERR_STATE unless `slot` is the slot of that call and has had
 *    no setter, sweep or filter since and ekf_dense_speckle_host has not run since (the rule of ekf_dense_get_volume);
 *  - ekf_dense_speckle_host: the same launches over tight height x width maps of the handle's size on the host, in and
 *    out, for depth maps that come from elsewhere; label / size (before the removal) may be NULL.  It touches no slot, and
 *    it takes over the planes ekf_dense_get_segments reads.  EKF_ERR_ARG: depth or plane NULL, min_size or max_diff out of
 *    range;
 *  - ekf_dense_get_speckle_profile: HIP-event milliseconds and launch counts of 4 kinds since the last ekf_dense_profile:
 *    k_speckle_label ([0]), k_speckle_merge ([1]), k_speckle_count ([2]), k_speckle_apply ([3]).  The other profile getters
 *    gain nothing. */
int ekf_dense_filter_speckle(ekf_dense* h, int slot, int min_size, int max_diff);
int ekf_dense_get_segments(ekf_dense* h, int slot, unsigned int* label, unsigned int* size);
int ekf_dense_speckle_host(ekf_dense* h, float* depth, int* plane, int min_size, int max_diff, unsigned int* label,
                           unsigned int* size);
int ekf_dense_get_speckle_profile(const ekf_dense* h, double* kernel_ms, long long* launches);

/* ---- the welded mesh of the TSDF volume and its vertex normals -----------------------------------------
 * ekf_fusion_get_mesh delivers a triangle soup, 99 to 108 bytes a triangle, which the caller welds by sorting the vertex
 * keys.  These additions weld on the device: a key is 8 la + d (la the linear index of the smaller end of a cell edge, d in
 * 1..7 the bits of the steps to its other end), so the welded vertices are the edges that carry a vertex in (la, d) order,
 * an exclusive scan over a 7-bit mask per voxel.  Edge (la, d) carries a vertex iff sum[la] < 0 differs from sum[lb] < 0 and
 * one of the cells that contain the edge has all eight cnt >= min_count.  The result equals the host weld of the soup bit
 * for bit: vertices by ascending key with the coordinates, grey and colour of ekf_fusion_get_mesh / ekf_colour_get_mesh,
 * faces[3 t + v] = the rank of key (t, v) of the soup, in the soup's triangle order.  Normals (opt-in): the mean field
 * v = (double) sum / (double) cnt, its gradient at a voxel by central differences ((v+ - v-) * 0.5; one-sided v+ - v or
 * v - v- where only one neighbour is in the grid with cnt >= min_count; 0.0 where none is), blended along the edge by the
 * vertex's u, n = g(la) + u (g(lb) - g(la)), divided by sqrt((n0 n0 + n1 n1) + n2 n2) and rounded once to float; 0 0 0
 * where that length is 0 or not finite.  They point towards free space, as the normals of ekf_raycast_get and the triangles'
 * (B - A) x (C - A) do.  tests/mesh_oracle.py restates all of it.  Opt-in: nothing above calls it, and no result, launch,
 * profile count or prototype above changes; ekf_abi_version() stays 6 (additions only).  The functions take an ekf_fusion
 * handle.
 *  - ekf_mesh_weld: if the handle holds no extract at this min_count since the volume last changed, exactly the launches of
 *    ekf_fusion_extract first; then k_mesh_cells, k_mesh_edges, k_tsdf_scan, one 8-byte read-back, k_mesh_vertices (not for
 *    an empty mesh) and k_mesh_faces (likewise); reports the numbers of vertices and triangles.  ekf_fusion_get_mesh and
 *    ekf_colour_get_mesh stay valid.  The first weld allocates 4 bytes a voxel and 1 byte a cell of scratch (grow-only,
 *    1.25 GB at 2^28 voxels).  EKF_ERR_ARG before the device is touched: min_count outside 1..65535, normals not 0 or 1, a
 *    NULL count.  A failed allocation is EKF_ERR_DEVICE and leaves the soup and the volume as they were;
 *  - ekf_mesh_get: the first min(n_vert, max_vert) vertices (xyz 3 doubles, grey 1 byte, bgr 3 bytes, normal 3 floats, key)
 *    and the first min(n_tri, max_tri) triangles (faces: 3 unsigned int); every pointer may be NULL.  EKF_ERR_ARG: bgr on a
 *    plain volume, or normal after a weld without normals.  EKF_ERR_STATE before a weld or after the volume changed since
 *    the last one (integrate, reset, set_volume);
 *  - ekf_mesh_get_profile: HIP-event milliseconds and launch counts of 5 kinds since the last ekf_fusion_profile:
 *    k_mesh_cells ([0]), k_mesh_edges ([1]), the weld's k_tsdf_scan ([2]), k_mesh_vertices ([3]), k_mesh_faces ([4]).  The
 *    other profile getters gain nothing from a weld but the launches of an extract it had to make. */
int ekf_mesh_weld(ekf_fusion* h, int min_count, int normals, unsigned long long* n_vert, unsigned long long* n_tri);
int ekf_mesh_get(ekf_fusion* h, double* xyz, unsigned int* faces, unsigned char* grey, unsigned char* bgr, float* normal,
                 unsigned long long* key, unsigned long long max_vert, unsigned long long max_tri);
int ekf_mesh_get_profile(const ekf_fusion* h, double* kernel_ms, long long* launches);

/* ---- the connected components of the welded mesh and its pruned copy ----------------------------------
 * The weld still holds floating fragments: what the speckle filter (§23) leaves where maps disagree, where cnt falls below
 * min_count round a voxel, or where noise makes an isolated sign change.  These additions find the connected components of
 * the last ekf_mesh_weld on the device and make a pruned copy of it beside it.  The contract, restated by
 * tests/component_oracle.py:
 *  - two vertices are linked iff some triangle of `faces` has both; a component is a connected component of the links.
 *    Linking is by index, not by coordinate: two vertices with different keys but equal coordinates (u exactly 0) are
 *    distinct.  Every welded vertex lies in at least one triangle;
 *  - label[v] is the least vertex index of v's component, size[v] the number of triangles of that component, n_comp the
 *    number of distinct labels: functions of `faces` alone, whatever the order in which the device's atomics arrive;
 *  - a component is kept iff size >= min_triangles and, with `largest`, it is the component of greatest size, the least
 *    label among equals.  The pruned mesh is the weld without the vertices and triangles of the other components, order
 *    preserved: xyz, key, grey, bgr and normal are the kept rows bit for bit (normal iff the weld had normals), faces the
 *    kept triangles in the soup's order, re-indexed by the rank of each vertex among the kept ones.  So min_triangles = 1,
 *    largest = 0 is the identity, keys stay ascending, pruning is idempotent, and a min_triangles above every size gives
 *    the empty mesh.
 * Opt-in: nothing above calls them, and no result, launch, profile count or prototype above changes; ekf_abi_version()
 * stays 6 (additions only).  ekf_mesh_get, ekf_fusion_get_mesh and ekf_colour_get_mesh stay valid: the weld is only read.
 * All take an ekf_fusion handle and work on its last weld: EKF_ERR_STATE before a weld or after the volume changed since
 * (integrate, reset, set_volume); a new weld invalidates the labels and the pruned mesh.  No kernel is launched for a weld
 * without triangles.  The first call allocates 16 bytes a vertex and 4 bytes a triangle of scratch (grow-only) and the pruned
 * mesh its own buffers; a failed allocation is EKF_ERR_DEVICE and leaves the weld as it was.
 *  - ekf_components_find: k_comp_init, k_comp_union, k_comp_count, k_comp_flags (for the sizes) and one 4-byte read-back;
 *    reports n_comp.  EKF_ERR_ARG: a NULL n_comp;
 *  - ekf_components_get: label and size of the first min(n_vert, max_vert) vertices of the weld; either may be NULL.
 *    EKF_ERR_STATE also where neither ekf_components_find nor ekf_components_prune has run since the last weld;
 *  - ekf_components_prune: the components first (k_comp_init, k_comp_union, k_comp_count) unless the handle holds them for this
 *    weld; then k_comp_largest (only with `largest`), k_comp_flags, k_tsdf_scan three times (kept vertices, kept triangles,
 *    kept components), one read-back of the three totals, k_comp_vertices and k_comp_faces (neither for an empty result);
 *    reports the pruned mesh's vertices and triangles and the number of components kept.  EKF_ERR_ARG before the device is
 *    touched: min_triangles == 0, largest not 0 or 1, a NULL count;
 *  - ekf_components_get_pruned: ekf_mesh_get's rules on the pruned mesh: the first min(n_vert, max_vert) vertices and
 *    min(n_tri, max_tri) triangles, every pointer may be NULL; EKF_ERR_ARG: bgr on a plain volume, or normal after a weld
 *    without normals; EKF_ERR_STATE also where no ekf_components_prune has run since the last weld;
 *  - ekf_components_get_profile: HIP-event milliseconds and launch counts of 8 kinds since the last
 *    ekf_fusion_profile: k_comp_init ([0]), k_comp_union ([1]), k_comp_count ([2]), k_comp_largest ([3]), k_comp_flags
 *    ([4]), the prune's k_tsdf_scan ([5]), k_comp_vertices ([6]), k_comp_faces ([7]).  The other profile getters gain
 *    nothing. */
int ekf_components_find(ekf_fusion* h, unsigned long long* n_comp);
int ekf_components_get(ekf_fusion* h, unsigned int* label, unsigned int* size, unsigned long long max_vert);
int ekf_components_prune(ekf_fusion* h, unsigned int min_triangles, int largest, unsigned long long* n_vert,
                   unsigned long long* n_tri, unsigned long long* n_kept);
int ekf_components_get_pruned(ekf_fusion* h, double* xyz, unsigned int* faces, unsigned char* grey, unsigned char* bgr,
                        float* normal, unsigned long long* key, unsigned long long max_vert, unsigned long long max_tri);
int ekf_components_get_profile(const ekf_fusion* h, double* kernel_ms, long long* launches);

/* ---- Taubin smoothing of the welded or the pruned mesh, and normals from its own triangles -------------
 * The weld is the raw marching-tetrahedra surface: the noise of the mean field and the lattice's staircase stand in its
 * vertices.  These additions smooth the last ekf_mesh_weld (source 0) or the last ekf_components_prune (source 1) on the
 * device with Taubin's lambda | mu scheme, which does not shrink the surface as plain Laplacian smoothing does, and give the
 * result normals from its own triangles (the weld's normals are gradients of the unsmoothed field and are not copied).
 * The contract, restated by tests/smooth_oracle.py, on a mesh (X, F) whose triangles have three distinct indices:
 *  - the adjacency is a function of F alone.  T(v): the ascending list of the triangles that contain v, inc(v) = |T(v)|;
 *    N(v): the ascending list of the distinct w != v that share a triangle with v, deg(v) = |N(v)|; m(v, w): the number of
 *    triangles that hold both; boundary(v) = 1 iff some w has m(v, w) = 1.  Every vertex lies in a triangle, so deg >= 2;
 *  - one step with factor f, every operation rounded once: s = X[w0][c], then s = s + X[wi][c] in the order of N(v);
 *    mean = s / (double) deg(v); X'[v][c] = X[v][c] + f * (mean - X[v][c]).  With pin_boundary, a vertex with
 *    boundary(v) = 1 keeps its bits;
 *  - a run is `iterations` times a step with lambda and then, unless mu == 0, a step with mu.  Taubin's scheme wants
 *    mu < -lambda (0.5 and -0.53 are common); mu == 0 launches single steps: plain Laplacian smoothing;
 *  - faces, key, grey and bgr of the result are the source's rows bit for bit;
 *  - normals, on request, from the final positions: the cross products (B - A) x (C - A) of the triangles of T(v) in
 *    ascending order, summed from left to right from the first one's, len = sqrt((a0 a0 + a1 a1) + a2 a2), each a_c / len
 *    rounded once to float, 0 0 0 where len is 0 or not finite: ekf_mesh_weld's normalisation and orientation (towards
 *    free space), weighted by area.
 * The sums are fp64 over lists the device gathers with integer atomics; every list is put in ascending order before it is
 * read, so the order of arrival costs no bit.
 * Opt-in: nothing above calls them, and no result, launch, profile count or prototype above changes; ekf_abi_version()
 * stays 6 (additions only).  The weld and the pruned mesh are only read and stay valid.  EKF_ERR_STATE before a weld, after
 * the volume changed since (integrate, reset, set_volume), and for source 1 without an ekf_components_prune since the last
 * weld; a new weld invalidates the adjacency and the result, a new prune those made from the pruned mesh.  No kernel is
 * launched for a mesh without triangles.  The adjacency (13 bytes a vertex, 36 bytes a triangle, grow-only) is kept for
 * the source mesh: a second run on the same mesh rebuilds nothing.  A failed allocation is EKF_ERR_DEVICE and leaves the
 * source as it was.
 *  - ekf_smooth_run: the adjacency unless the handle holds it for this mesh (k_smooth_count, k_smooth_offsets, k_tsdf_scan,
 *    k_smooth_fill, k_smooth_lists), then k_smooth_step `iterations` times, or twice that with mu != 0, with nothing between
 *    them, then k_smooth_normals with `normals`; reports the vertices and triangles of the result (the source's).
 *    EKF_ERR_ARG before the device is touched: source not 0 or 1, iterations outside 1..1024, lambda not finite or outside
 *    (0, 1], mu not finite or outside [-1, 0], pin_boundary or normals not 0 or 1, a NULL count;
 *  - ekf_smooth_get: ekf_mesh_get's rules on the result: the first min(n_vert, max_vert) vertices and min(n_tri, max_tri)
 *    triangles, every pointer may be NULL; EKF_ERR_ARG: bgr on a plain volume, or normal after a run without normals;
 *    EKF_ERR_STATE also without an ekf_smooth_run on the current mesh;
 *  - ekf_smooth_get_adjacency: inc, deg (uint32) and boundary (uint8) of the first min(n_vert, max_vert) vertices of the
 *    last run's mesh; any may be NULL.  EKF_ERR_STATE as ekf_smooth_get;
 *  - ekf_smooth_get_profile: HIP-event milliseconds and launch counts of 7 kinds since the last ekf_fusion_profile:
 *    k_smooth_count ([0]), k_smooth_offsets ([1]), k_tsdf_scan ([2]), k_smooth_fill ([3]), k_smooth_lists ([4]),
 *    k_smooth_step ([5]), k_smooth_normals ([6]).  The other profile getters gain nothing. */
int ekf_smooth_run(ekf_fusion* h, int source, int iterations, double lambda, double mu, int pin_boundary, int normals,
                   unsigned long long* n_vert, unsigned long long* n_tri);
int ekf_smooth_get(ekf_fusion* h, double* xyz, unsigned int* faces, unsigned char* grey, unsigned char* bgr, float* normal,
                   unsigned long long* key, unsigned long long max_vert, unsigned long long max_tri);
int ekf_smooth_get_adjacency(ekf_fusion* h, unsigned int* inc, unsigned int* deg, unsigned char* boundary,
                             unsigned long long max_vert);
int ekf_smooth_get_profile(const ekf_fusion* h, double* kernel_ms, long long* launches);

/* ---- Vertex-clustering simplification of the welded, the pruned or the smoothed mesh -------------------
 * The surface is marching tetrahedra: up to seven vertices belong to one voxel, far more triangles than its geometry needs.
 * These additions cluster the vertices of the last ekf_mesh_weld (source 0), the last ekf_components_prune (source 1) or the
 * last ekf_smooth_run's result (source 2) on a grid of cells of side `cell` (Rossignac and Borrel) on the device, into a mesh
 * of its own.  The contract, restated by tests/simplify_oracle.py.  Input: a source mesh (X, F, grey, optional bgr, optional
 * normals) with n_vert vertices and n_tri triangles, the volume's origin, dims and voxel, and `cell` (fp64, finite,
 * cell >= voxel).  Every fp64 operation is rounded once, with contraction off:
 *  1. the grid.  G_a = (int) floor(((double)(dims_a - 1) * voxel) / cell) + 1 for a = x, y, z, so G_a <= dims_a: the grid
 *     never has more cells than the volume has voxels.  For a vertex, q_a = floor((X[v][a] - origin[a]) / cell): a division,
 *     not a multiplication by a reciprocal; a result that is not finite counts as 0; the result is clamped to [0, G_a - 1]
 *     (a smoothed vertex may leave the box, so the clamp is part of the contract).  cell(v) = (q_z G_y + q_y) G_x + q_x, x
 *     fastest, as in the volume;
 *  2. the triangles.  Triangle t has the cells (cell(F[t][0]), cell(F[t][1]), cell(F[t][2])).  It is degenerate iff two of
 *     them are equal.  A non-degenerate triangle is a duplicate iff a non-degenerate triangle with a smaller index has the
 *     same unordered triple of cells.  The kept triangles are the rest, in the source's order and with the source's winding;
 *  3. the vertices.  A cell is used iff a kept triangle has it.  The output has one vertex per used cell, numbered by
 *     ascending cell id; that cell id is the output's key, so keys ascend strictly.  A cell that holds vertices but no kept
 *     triangle gives no vertex.  With M(c) the ascending list of the source vertices of cell c and n = |M(c)|:
 *       position: per coordinate, s = X[m0], then s = s + X[mi] in the order of M(c), then s / (double) n;
 *       grey, and each of B, G, R of a colour volume: (2 S + n) / (2 n) in unsigned 64-bit integer arithmetic, S the sum:
 *         the mean, with halves rounded up;
 *       normal (iff the source has normals): the members' float normals summed as doubles in the order of M(c), starting
 *         from the first one's; len = sqrt((a0 a0 + a1 a1) + a2 a2); each a_c / len rounded once to float; 0 0 0 where len
 *         is 0 or not finite: ekf_mesh_weld's normalisation.  A source without normals gives a result without normals;
 *  4. the faces: the kept triangles, each index replaced by the output number of its cell;
 *  5. the vertex map: for every source vertex, the output number of its cell, or 0xffffffff if the cell is unused;
 *  6. the counts: n_vert_out, n_tri_out, n_degenerate, n_duplicate, with n_tri_out + n_degenerate + n_duplicate = n_tri.
 * Arrival order costs no bit: the only atomics are integer adds and cursors, and every list (the members of a cell, the
 * non-degenerate triangles filed under their least cell for the duplicate test) is put in ascending order by the one lane
 * that owns it before anything reads it, whatever its length; no workgroup waits for another inside a launch.
 * Opt-in and terminal: nothing above calls them, and no result, launch, profile count or prototype above changes;
 * ekf_abi_version() stays 6 (additions only).  The sources are only read and stay valid; ekf_smooth_run keeps refusing
 * source 2.  EKF_ERR_STATE before a weld, after the volume changed since (integrate, reset, set_volume), for source 1
 * without an ekf_components_prune since the last weld and for source 2 without an ekf_smooth_run on the current mesh.  A new
 * weld invalidates the result, a new prune one made from the pruned or a smoothed pruned mesh, a new smooth run one made
 * from source 2.  No kernel is launched for a source without triangles.  Scratch (grow-only): 20 bytes a cell, 12 bytes a
 * source vertex, 20 bytes a source triangle.  A failed allocation is EKF_ERR_DEVICE and leaves every source as it was.
 *  - ekf_simplify_run: k_simp_cells, k_simp_count, k_simp_offsets, k_tsdf_scan twice, k_simp_fill, k_simp_lists,
 *    k_simp_flags, k_tsdf_scan three times, one read-back of the totals, k_simp_map, and for a result that is not empty
 *    k_simp_vertices and k_simp_faces; reports the four counts.  EKF_ERR_ARG before the device is touched: source not 0, 1
 *    or 2, cell not finite or below the voxel, a NULL count;
 *  - ekf_simplify_get: ekf_mesh_get's rules on the result: the first min(n_vert, max_vert) vertices and min(n_tri, max_tri)
 *    triangles, every pointer may be NULL; EKF_ERR_ARG: bgr on a plain volume, or normal after a run on a source without
 *    normals; EKF_ERR_STATE also without an ekf_simplify_run on the current mesh;
 *  - ekf_simplify_get_map: the vertex map of the first min(n_vert of the source, max_vert) source vertices (uint32); map may
 *    be NULL.  EKF_ERR_STATE as ekf_simplify_get;
 *  - ekf_simplify_get_profile: HIP-event milliseconds and launch counts of 10 kinds since the last ekf_fusion_profile:
 *    k_simp_cells ([0]), k_simp_count ([1]), k_simp_offsets ([2]), k_tsdf_scan ([3]), k_simp_fill ([4]), k_simp_lists ([5]),
 *    k_simp_flags ([6]), k_simp_vertices ([7]), k_simp_faces ([8]), k_simp_map ([9]).  The other profile getters gain
 *    nothing. */
int ekf_simplify_run(ekf_fusion* h, int source, double cell, unsigned long long* n_vert, unsigned long long* n_tri,
                     unsigned long long* n_degenerate, unsigned long long* n_duplicate);
int ekf_simplify_get(ekf_fusion* h, double* xyz, unsigned int* faces, unsigned char* grey, unsigned char* bgr, float* normal,
                     unsigned long long* key, unsigned long long max_vert, unsigned long long max_tri);
int ekf_simplify_get_map(ekf_fusion* h, unsigned int* map, unsigned long long max_vert);
int ekf_simplify_get_profile(const ekf_fusion* h, double* kernel_ms, long long* launches);

/* ---- A per-triangle texture atlas of the welded, the pruned, the smoothed or the simplified mesh ----------
 * A simplified mesh carries one grey or B, G, R value per vertex, the mean of up to hundreds of source vertices; the key
 * frames that made it hold far more.  These additions texture the last ekf_mesh_weld (source 0), the last
 * ekf_components_prune (1), the last ekf_smooth_run's result (2) or the last ekf_simplify_run's result (3) on the device from
 * views that are fed one at a time, so that there is no limit on their number and only the current view's image is resident.
 * The contract, restated by tests/texture_oracle.py.  Input: a source mesh (X fp64, F uint32, vertex grey and optional B, G,
 * R) with n_tri > 0 triangles, a patch size P in 2..32 and `channels`, 1 or 3.  Every fp64 operation is rounded once, in the
 * written order, with contraction off:
 *  1. the layout.  Triangles are paired into square blocks of side B = P + 2 texels: block q = t >> 1 holds triangle 2 q
 *     (the lower one) and 2 q + 1 (the upper one).  n_sq = (n_tri + 1) >> 1, Q is the least integer with Q Q >= n_sq, the
 *     atlas is A x A texels with A = Q B, row 0 first, and block q sits at (bx, by) = (q % Q, q / Q).  A texel with
 *     block-local coordinates (a, b) belongs to the lower triangle iff a + b <= P, otherwise to the upper one.  Corner texel
 *     centres: lower c0 = (0, 0), c1 = (P - 1, 0), c2 = (0, P - 1); upper c0 = (P + 1, P + 1), c1 = (2, P + 1),
 *     c2 = (P + 1, 2), so a bilinear look-up inside a triangle's UV triangle touches texels of that triangle only; the
 *     diagonals a + b = P and P + 1 are gutters, filled by extrapolation.  Barycentrics of a texel: lower
 *     l1 = (double) a / (double)(P - 1), l2 = (double) b / (double)(P - 1); upper l1 = (double)(P + 1 - a) / (double)(P - 1),
 *     l2 = (double)(P + 1 - b) / (double)(P - 1); l0 = (1.0 - l1) - l2.  UV of corner i of triangle t:
 *     ((double)(bx B + c_i.x) + 0.5) / (double) A, likewise for y, measured from row 0: made on the host, without a launch;
 *  2. a vertex in a view (an image of W x H, K = fx fy cx cy, a pose, an optional z-buffer): p = R^T (X - t),
 *     sx = fx (p0 / p2) + cx, sy = fy (p1 / p2) + cy in ekf_fusion_integrate's operation order.  It is visible iff p2 > 0,
 *     0 <= sx <= W - 1, 0 <= sy <= H - 1 (a NaN fails) and, with occlusion on, D = (double) zbuf[floor(sy + 0.5) W +
 *     floor(sx + 0.5)] has D > 0 and p2 <= D + tol.  D == 0 (the ray cast found no surface) fails on purpose;
 *  3. a triangle in a view is a candidate iff its three vertices are visible; its score is sigma ((sx1 - sx0)(sy2 - sy0) -
 *     (sy1 - sy0)(sx2 - sx0)), twice its signed area in pixels, with sigma = -1: a triangle of a weld seen from the
 *     free-space side scores positive.  The view wins triangle t iff score > min_area2 and score > best_score[t];
 *     best_score starts at 0 and best_view at -1, and the strict > lets the earlier view keep a tie.  A view's number is the
 *     count of views added since ekf_texture_begin;
 *  4. the fill, for every texel of a triangle the current view has just won: Xp = (l0 X0 + l1 X1) + l2 X2 per coordinate,
 *     projected as in 2; if !(p2 > 0) or a coordinate is NaN the texel is left as it is; sx is clamped to [0, W - 1] and sy to
 *     [0, H - 1]; the sample is ekf_get_frame_rectified's blend: q = (int) floor(s 32 + 0.5), i = q >> 5, alpha = q & 31, the
 *     second tap min(i + 1, dim - 1), weights (32 - ax)(32 - ay) and so on, the value (sum w tap + 512) >> 10.  A 3-channel
 *     atlas takes B, G, R and a grey view replicates its value; a 1-channel atlas takes the view's grey image (of a colour
 *     view: the grey image ekf_dense_set_view_colour derived, the library's B, G, R -> grey conversion);
 *  5. the finish: the texels of a triangle with best_view = -1 get, per channel, floor(((l0 g0 + l1 g1) + l2 g2) + 0.5)
 *     clamped to 0..255, g the source's vertex grey, or its B, G, R on a colour volume with a 3-channel atlas.  Padding
 *     (t >= n_tri) stays 0.  n_textured is the number of triangles with a view.
 * A triangle and a texel belong to one lane; the only atomics are two integer adds a workgroup of k_tex_select (the triangles
 * a view won, and won for the first time), exact in any order.  Opt-in and terminal: nothing above calls them, and no
 * result, launch, profile count or prototype above changes; ekf_abi_version() stays 6 (additions only).  The sources and the
 * last render are only read and stay valid.  EKF_ERR_STATE as ekf_simplify_run's for sources 0, 1 and 2, and for source 3
 * without an ekf_simplify_run on the current mesh; whatever invalidates the source mesh invalidates the texture: a new weld,
 * a prune, smooth or simplify run on which the source depends, a change of the volume.  Device memory (grow-only):
 * A A channels bytes, 13 bytes a triangle, 17 bytes a source vertex.  A failed allocation in ekf_texture_begin is
 * EKF_ERR_DEVICE and leaves everything as it was, the texture begun before included; a clear that fails after it leaves the
 * handle without a texture (the buffers may be the earlier texture's own).  The image of ekf_texture_add_view_host is staged
 * in a buffer that grows by itself: a failed growth is EKF_ERR_DEVICE, loses only that staging buffer and adds no view.
 * Argument errors are reported before the device is touched.
 *  - ekf_texture_begin: allocates and clears; reports A.  EKF_ERR_ARG: source not 0..3, patch not 2..32, channels not 1 or
 *    3, a NULL atlas_side, A > 16384; EKF_ERR_STATE also for a source without triangles;
 *  - ekf_texture_add_view: the image, K and pose of a set slot of a dense handle, read where they lie on the device
 *    (EKF_ERR_ARG: a dense handle on another device): k_tex_project, k_tex_select, one read-back of the two counters and,
 *    if the view won a triangle, k_tex_fill; reports the triangles it won.  occlusion is 0 or 1; 1 takes the depth image of
 *    the handle's current ekf_raycast_render / _render_view as the z-buffer (EKF_ERR_STATE without one since the volume last
 *    changed, or if its size is not the view's; that its pose is the view's is the caller's duty; the render stays
 *    readable).  tol and min_area2 are finite and >= 0.  EKF_ERR_STATE before ekf_texture_begin and after ekf_texture_finish;
 *  - ekf_texture_add_view_host: the same for an image from the host: rows of channels width bytes (1: grey; 3: B, G, R),
 *    1 <= width, height <= 8192, K finite with fx, fy > 0;
 *  - ekf_texture_finish: k_tex_fallback; reports n_textured.  EKF_ERR_STATE when called twice;
 *  - ekf_texture_get: readable any time after ekf_texture_begin; every pointer may be NULL.  atlas: A rows of A channels
 *    bytes, `pitch` bytes apart (EKF_ERR_ARG: pitch < A channels); uv: 6 doubles a triangle (u, v of corners 0, 1, 2); view:
 *    int32; score: double; each for the first min(n_tri, max_tri) triangles;
 *  - ekf_texture_get_profile: HIP-event milliseconds and launch counts of 4 kinds since the last ekf_fusion_profile:
 *    k_tex_project ([0]), k_tex_select ([1]), k_tex_fill ([2]), k_tex_fallback ([3]).  The other profile getters gain
 *    nothing. */
int ekf_texture_begin(ekf_fusion* h, int source, int patch, int channels, int* atlas_side);
int ekf_texture_add_view(ekf_fusion* h, ekf_dense* dense, int slot, int occlusion, double tol, double min_area2,
                         unsigned long long* n_won);
int ekf_texture_add_view_host(ekf_fusion* h, const unsigned char* img, int pitch, int channels, int width, int height,
                              const double* K, const double* pose7, int occlusion, double tol, double min_area2,
                              unsigned long long* n_won);
int ekf_texture_finish(ekf_fusion* h, unsigned long long* n_textured);
int ekf_texture_get(ekf_fusion* h, unsigned char* atlas, int pitch, double* uv, int* view, double* score,
                    unsigned long long max_tri);
int ekf_texture_get_profile(const ekf_fusion* h, double* kernel_ms, long long* launches);

/* ---- A rasteriser for the indexed meshes: depth, triangle, barycentric, normal and shaded images ----------
 * ekf_raycast_* renders the volume; these additions render the mesh itself: the last ekf_mesh_weld (source 0), the last
 * ekf_components_prune (1), the last ekf_smooth_run's result (2), the last ekf_simplify_run's result (3) or a mesh the caller
 * gave with ekf_raster_set_mesh (4), from any pinhole pose, with its vertex colours (shading 0) or the atlas of §29
 * (shading 1).  The contract, restated by tests/raster_oracle.py.  Input: a source mesh (X fp64, F uint32, vertex grey and
 * optional B, G, R), an image of W x H, both in 1..8192, K = fx fy cx cy, a pose (normalised as ekf_raycast_render normalises
 * it), z_near >= 0, cull, shading and cover, each 0 or 1.  Every fp64 operation is rounded once, in the written order, with
 * contraction off:
 *  1. a vertex: p2, sx, sy as in §29's step 2 (the same function).  It is usable iff p2 > z_near and sx and sy are finite;
 *  2. a triangle t with the vertex indices (i0, i1, i2) is dropped if a vertex is unusable: there is no clipping, and a
 *     triangle that straddles z_near disappears whole.  area2 = (x1 - x0)(y2 - y0) - (y1 - y0)(x2 - x0); area2 == 0 or NaN
 *     drops the triangle; front = area2 < 0 (§29's sigma = -1); with cull a triangle that is not front is dropped;
 *     s = front ? -1 : +1.  Its box: x from max(0, ceil(min sx)) to min(W - 1, floor(max sx)), y likewise; an empty box drops
 *     the triangle.  Pixel (px, py) is sampled at ((double) px, (double) py): a pixel's centre is its integer coordinate;
 *  3. coverage, watertight by construction.  Edge k runs from corner k to corner k + 1 mod 3 and weighs corner k + 2 mod 3.
 *     It is evaluated from the endpoint with the lower vertex index: if i_a < i_b, E = (xb - xa)(py - ya) - (yb - ya)(px - xa)
 *     and canon = true; otherwise E = -((xa - xb)(py - yb) - (ya - yb)(px - xb)) and canon = false: two triangles that share
 *     an edge get exactly negated values, whatever their corner order.  e_k = s E.  The pixel is inside edge k iff e_k > 0, or
 *     e_k == 0 and canon != front: the triangle that runs the edge in ascending index order after its flip owns the tie.  A
 *     pixel is covered iff it is inside all three edges and ssum = (b0 + b1) + b2 > 0, b_k the e of the edge opposite
 *     corner k;
 *  4. depth: w_k = (b_k / ssum) / p2_k, ws = (w0 + w1) + w2, z = 1.0 / ws, z32 = (float) z; the pixel is skipped unless
 *     ws > 0 and z32 is finite.  Perspective-correct barycentrics l_k = w_k / ws.  The pixel's key is
 *     ((uint64) bits(z32) << 32) | t; the image of keys starts at all ones and takes the minimum: the nearest depth wins and,
 *     among equal depths, the least triangle index.  With cover a uint32 image counts, for every pixel, the triangles that
 *     gave it a key;
 *  5. resolve, for every pixel whose key is not all ones, applies 2 to 4 again for the winning triangle, so that the depth is
 *     the key's own: depth (float32) = z32, tri (int32) = t, bary = ((float) l1, (float) l2), normal = (X1 - X0) x (X2 - X0),
 *     each component a b - c d in fp64, divided by sqrt((n0 n0 + n1 n1) + n2 n2) and converted to float; it is 0 where that
 *     length is 0 or not finite, and it is not flipped for a back face.  Shading 0: per channel
 *     floor(((l0 g0 + l1 g1) + l2 g2) + 0.5) clamped to 0..255: the grey image and, where the source has B, G, R (sources 0..3
 *     of a colour volume, source 4 given with bgr), the colour image.  Shading 1: tx = ((l0 c0x + l1 c1x) + l2 c2x) +
 *     (double)(bx B), ty likewise, with §29's c_i, bx, by of t; both clamped to [0, A - 1]; §29's 5-bit blend:
 *     q = (int) floor(s 32 + 0.5), i = q >> 5, alpha = q & 31, the second tap min(i + 1, A - 1), (sum w tap + 512) >> 10.  A
 *     3-channel atlas gives the colour image, and the grey image is the library's B, G, R -> grey conversion of it; a
 *     1-channel atlas gives the grey image and no colour image.  A pixel without a hit has depth 0, tri -1, bary 0, normal 0
 *     and colour 0.
 * The only atomics are the 64-bit minimum of the keys, the integer add of the cover image and the cursor of a list of
 * deferred triangles, all exact in any order: the images do not depend on how the work is divided.  Opt-in and terminal:
 * nothing above calls them, and no result, launch, profile count or prototype above changes; ekf_abi_version() stays 6
 * (additions only).  The sources, the atlas and the last ray cast are only read and stay valid.  Sources 0..3 are valid under
 * ekf_texture_begin's rules and give its EKF_ERR_STATE otherwise (also for a source without triangles); source 4 is
 * EKF_ERR_STATE before an ekf_raster_set_mesh.  Shading 1 needs a finished texture (ekf_texture_finish) whose source is the one
 * rendered, otherwise EKF_ERR_STATE; it is EKF_ERR_ARG for source 4.  The images are a snapshot: readable from a successful
 * render until the next render begins, whatever becomes of the source.  Device memory (grow-only): 8 bytes a pixel of keys, 29
 * of images (32 with a colour image), 4 of cover when it is asked for, 25 bytes a vertex and 4 a triangle of scratch, and the
 * rows of source 4.  A failed allocation is EKF_ERR_DEVICE and leaves the previous images and everything else as they were.
 * Argument errors are reported before the device is touched, each with a message through ekf_fusion_last_error.
 *  - ekf_raster_set_mesh: copies a mesh to buffers of the rasteriser's own: xyz 3 doubles a vertex, faces 3 uint32 a
 *    triangle, grey a byte a vertex, bgr 3 bytes a vertex or NULL.  EKF_ERR_ARG: a NULL xyz, faces or grey, n_vert or n_tri
 *    0 or >= 2^32, an xyz that is not finite, an index >= n_vert;
 *  - ekf_raster_render: memsets, k_rast_project, k_rast_small, k_rast_large (unless small_limit >= width height: no box is
 *    larger than the image) and k_rast_resolve on the default stream, without a read-back.  EKF_ERR_ARG: width or height not
 *    in 1..8192, K not finite or fx or fy 0, a pose that is not finite or has q = 0, source not 0..4, z_near not finite or
 *    < 0, cull, shading or cover not 0 or 1;
 *  - ekf_raster_render_view: the same with the K, pose and size of a set slot of a dense handle (EKF_ERR_ARG: a dense handle
 *    on another device, a slot out of range; EKF_ERR_STATE: a slot that is not set);
 *  - ekf_raster_get: every pointer may be NULL.  depth, normal (3 floats a pixel), grey, bgr (3 bytes a pixel), tri (int32),
 *    bary (2 floats a pixel), cover (uint32), tight rows, row 0 first.  EKF_ERR_ARG: bgr when the render has no colour image,
 *    cover when it was rendered with cover = 0; EKF_ERR_STATE without a render;
 *  - ekf_raster_set_small_limit: a triangle whose clamped box has at most `limit` pixels (0..65536, default 16) is walked by
 *    one lane of k_rast_small, a larger one by a workgroup of k_rast_large; 0 defers every triangle.  The images do not
 *    depend on it;
 *  - ekf_raster_get_profile: HIP-event milliseconds and launch counts of 4 kinds since the last ekf_fusion_profile:
 *    k_rast_project ([0]), k_rast_small ([1]), k_rast_large ([2]), k_rast_resolve ([3]).  The other profile getters gain
 *    nothing. */
int ekf_raster_set_mesh(ekf_fusion* h, const double* xyz, const unsigned int* faces, const unsigned char* grey,
                        const unsigned char* bgr, unsigned long long n_vert, unsigned long long n_tri);
int ekf_raster_render(ekf_fusion* h, int source, int width, int height, const double* K, const double* pose7, double z_near,
                      int cull, int shading, int cover);
int ekf_raster_render_view(ekf_fusion* h, int source, ekf_dense* dense, int slot, double z_near, int cull, int shading,
                           int cover);
int ekf_raster_get(ekf_fusion* h, float* depth, float* normal, unsigned char* grey, unsigned char* bgr, int* tri, float* bary,
                   unsigned int* cover, int* width, int* height);
int ekf_raster_set_small_limit(ekf_fusion* h, int limit);
int ekf_raster_get_profile(const ekf_fusion* h, double* kernel_ms, long long* launches);

/* ---- A mesh-to-mesh distance: the nearest triangle of a target mesh for every query point -----------------
 * How far one of the handle's meshes lies from another, in 3-D: for every query point the nearest point on a target mesh,
 * and from it the one-sided Hausdorff distance, the mean, the RMS and the share within a threshold.  The contract, restated by
 * tests/distance_oracle.py.  All arithmetic is fp64, every operation rounded once, in the written order, contraction off:
 *  1. the target is a mesh (X, F): the last ekf_mesh_weld (source 0), the last ekf_components_prune (1), the last
 *     ekf_smooth_run's result (2), the last ekf_simplify_run's result (3), valid under ekf_texture_begin's rules, or a mesh given
 *     with ekf_distance_set_mesh (4), which is independent of the rasteriser's source 4.  A triangle t = (i0, i1, i2) with the
 *     corners A, B, C is valid iff its indices are distinct, its nine coordinates are finite and, with u = B - A, v = C - A,
 *     n = (u1 v2 - u2 v1, u2 v0 - u0 v2, u0 v1 - u1 v0), nn = (n0 n0 + n1 n1) + n2 n2 is finite and > 0.  Invalid triangles take
 *     no part; a target without a valid triangle is EKF_ERR_STATE;
 *  2. point to triangle: Ericson, Real-Time Collision Detection, section 5.1.5, the six region tests in the book's order, with
 *     dot(a, b) = (a0 b0 + a1 b1) + a2 b2, ab = B - A, ac = C - A, ap = p - A, bp = p - B, cp = p - C:
 *       d1 = dot(ab, ap), d2 = dot(ac, ap);  d1 <= 0 and d2 <= 0:                                  c = A
 *       d3 = dot(ab, bp), d4 = dot(ac, bp);  d3 >= 0 and d4 <= d3:                                 c = B
 *       vc = d1 d4 - d3 d2;  vc <= 0 and d1 >= 0 and d3 <= 0:      v = d1 / (d1 - d3),             c = A + v ab
 *       d5 = dot(ab, cp), d6 = dot(ac, cp);  d6 >= 0 and d5 <= d6:                                 c = C
 *       vb = d5 d2 - d1 d6;  vb <= 0 and d2 >= 0 and d6 <= 0:      w = d2 / (d2 - d6),             c = A + w ac
 *       va = d3 d6 - d5 d4, e = d4 - d3, f = d5 - d6;  va <= 0 and e >= 0 and f >= 0:  w = e / (e + f),  c = B + w (C - B)
 *       otherwise s = (va + vb) + vc, v = vb / s, w = vc / s,                                      c = (A + v ab) + w ac
 *     then every component of c is clamped to the triangle's own box by comparisons, lo_k = min(A_k, B_k, C_k),
 *     hi_k = max(A_k, B_k, C_k), c_k = c_k < lo_k ? lo_k : (c_k > hi_k ? hi_k : c_k) (a NaN stays), and with q = p - c,
 *     d2 = (q0 q0 + q1 q1) + q2 q2;
 *  3. the result for a finite p: over all valid triangles the least (d2, t): t replaces the best iff d2 < best, or d2 == best
 *     and t < best_t, from (+inf, 0xffffffff), so a d2 that is NaN never wins and among equal d2 the least index does.
 *     dist = sqrt(d2) (double), tri = t (uint32), closest = the winner's c (3 doubles), side (int8) = the sign of
 *     (q0 n0 + q1 n1) + q2 n2 with the winner's n: +1 is the free-space side of a weld, 0 means zero (or NaN).  A p with a
 *     coordinate that is not finite gets dist = NaN, tri = 0xffffffff, closest = NaN, side = 0;
 *  4. the queries are the vertices of a source 0..4 (target and query may be the same source) or n points from the host;
 *  5. statistics of the last run for a threshold thr >= 0: a point is bad iff its dist is NaN; n_bad counts the bad points and
 *     n the others; max and argmax, its least index; within = #{dist <= thr}; sum of dist and sum2 of dist dist, a bad point
 *     giving 0, summed in a fixed order: per block of 256 consecutive points the tree for s = 128 .. 1: v[l] += v[l + s]; the
 *     block partials go to one workgroup whose lane l adds the partials l, l + 256, .. in ascending order from 0.0, then the
 *     same tree.  mean = sum / n, rms = sqrt(sum2 / n); with n = 0 they and max are NaN and argmax is 0xffffffff.
 * A uniform grid over the box of the valid triangles only prunes the search (csrc/ekf_mesh_distance.hpp has the termination
 * rule and its proof): the result is the same at every setting of ekf_distance_set_grid.  Opt-in and terminal: nothing above
 * calls these, and no result, launch, profile count or prototype above changes; ekf_abi_version() stays 6 (additions only).
 * The sources are only read.  The arrays are a snapshot: readable from a successful run until the next run begins, whatever
 * becomes of the sources.  A failed allocation is EKF_ERR_DEVICE and leaves the previous result and every source intact: new
 * buffers replace old ones only when all exist.  Argument errors are reported before the device is touched, each with a
 * message through ekf_fusion_last_error.
 *  - ekf_distance_set_mesh: copies a mesh to buffers of the feature's own: xyz 3 doubles a vertex, faces 3 uint32 a triangle.
 *    EKF_ERR_ARG: a NULL xyz or faces, n_vert or n_tri 0 or >= 2^32, an xyz that is not finite, an index >= n_vert;
 *  - ekf_distance_run: the vertices of source `query` against source `target`; *n_points (may be NULL) is their number.
 *    EKF_ERR_ARG: target or query not 0..4.  EKF_ERR_STATE: a source that is not valid (ekf_texture_begin's messages; source 4
 *    before an ekf_distance_set_mesh), a target without a valid triangle, a query without a vertex.  EKF_ERR_DEVICE: 2^32
 *    entries or more in the cell lists;
 *  - ekf_distance_run_points: n_points points from the host (3 doubles each), 0 < n_points < 2^32, otherwise EKF_ERR_ARG;
 *  - ekf_distance_get: every pointer may be NULL.  dist (double), tri (uint32), closest (3 doubles a point), side (int8).
 *    EKF_ERR_ARG: a pointer given and max_points less than the points of the run; EKF_ERR_STATE without a run;
 *  - ekf_distance_get_stats: step 5; every output pointer may be NULL.  EKF_ERR_ARG: thr < 0 or NaN; EKF_ERR_STATE without a
 *    run.  It launches k_dist_stats and k_dist_reduce;
 *  - ekf_distance_set_grid: g = 0 (the default) chooses the cells along the longest axis of the box automatically,
 *    clamp(ceil(sqrt(n_valid / 2)), 1, 128), settled from the timing table of DESIGN.md §31.4; g in 1..128 sets them; the
 *    other axes are in proportion, at least 1.  g = 1 is brute force on the device.  EKF_ERR_ARG otherwise.  The result does
 *    not depend on it;
 *  - ekf_distance_get_grid: of the last run, for measurements: the cells along x, y, z, the entries of all cell lists and the
 *    longest list (which costs a copy of the counts); every pointer may be NULL;
 *  - ekf_distance_get_profile: HIP-event milliseconds and launch counts of 9 kinds since the last ekf_fusion_profile:
 *    k_dist_box ([0]), k_dist_grid ([1]), k_dist_count ([2]), k_dist_offsets ([3]), k_tsdf_scan ([4]), k_dist_fill ([5]),
 *    k_dist_query ([6]), k_dist_stats ([7]), k_dist_reduce ([8]).  The other profile getters gain nothing. */
int ekf_distance_set_mesh(ekf_fusion* h, const double* xyz, const unsigned int* faces, unsigned long long n_vert,
                          unsigned long long n_tri);
int ekf_distance_run(ekf_fusion* h, int target, int query, unsigned long long* n_points);
int ekf_distance_run_points(ekf_fusion* h, int target, const double* xyz, unsigned long long n_points);
int ekf_distance_get(ekf_fusion* h, double* dist, unsigned int* tri, double* closest, signed char* side,
                     unsigned long long max_points);
int ekf_distance_get_stats(ekf_fusion* h, double thr, unsigned long long* n, unsigned long long* n_bad, double* max,
                           unsigned long long* argmax, double* mean, double* rms, unsigned long long* within);
int ekf_distance_set_grid(ekf_fusion* h, int g);
int ekf_distance_get_grid(ekf_fusion* h, int* cells, unsigned long long* entries, unsigned int* longest);
int ekf_distance_get_profile(const ekf_fusion* h, double* kernel_ms, long long* launches);

#ifdef __cplusplus
}
#endif
#endif /* EKF_MONOSLAM_H_ */
