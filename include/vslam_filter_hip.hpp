// vslam_filter_hip.hpp -- header-only C++ mirror of the reference's `class VSlamFilter`
// (mono-slam/src/vslamRansac.hpp:94-141) over the C ABI of ekf_monoslam.h.
//
// Same method names, argument meaning and return conventions as the reference, minus the
// drawing methods; captureNewFrame takes the camera's pixels instead of a cv::Mat.  Eigen / OpenCV
// types are replaced by plain float arrays so that the header has no dependencies; a node
// that has Eigen can `Eigen::Map<MatrixXf>` the column-major buffers directly.
// Link: -lekfslam_hip (built by ekf-monoslam_for_3d-reconstruction_amd/csrc/Makefile).
#pragma once
#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "ekf_monoslam.h"

class VSlamFilterHip {
 public:
  static constexpr int STATE_DIM = 14;  // vR.cpp:22

  // VSlamFilter(char* file): the libconfig++ reader (ConfigVSLAM.cpp) stays with the caller, who
  // passes the parsed fields (+ frame size after `scale`) as an ekf_config.
  explicit VSlamFilterHip(const ekf_config& cfg, int capacity_features = 1024, int device = 0) {
    if (ekf_create(&cfg, STATE_DIM, capacity_features, EKF_F32, device, &h_) != EKF_OK)
      throw std::runtime_error(std::string("ekf_create: ") + ekf_last_error(nullptr));
  }
  ~VSlamFilterHip() { ekf_destroy(h_); }
  VSlamFilterHip(const VSlamFilterHip&) = delete;
  VSlamFilterHip& operator=(const VSlamFilterHip&) = delete;

  // captureNewFrame(cv::Mat, double time_stamp): only the dT bookkeeping (vR.cpp:226-233)
  void captureNewFrame(double time_stamp) {
    if (old_ts_ > 0) check(ekf_set_dt(h_, time_stamp - old_ts_));
    old_ts_ = time_stamp;
  }
  // captureNewFrame(cv::Mat newFrame, double time_stamp) (vR.cpp:226-245) with the camera's own frame: dT first, then
  // the image -- 8-bit, `channels` = 1 or 3 (B, G, R), `stride` bytes per row, width / scale x height / scale = the
  // config's frame size.  The resize by `scale` and the grey conversion run on the device.
  void captureNewFrame(const unsigned char* pixels, int width, int height, int channels, int stride, double time_stamp) {
    captureNewFrame(time_stamp);
    check(ekf_set_frame_raw(h_, pixels, width, height, channels, stride));
  }
  // the same from device memory, queued on the filter's stream without a host synchronisation: d_pixels must stay valid
  // and unchanged until ekf_synchronize(handle())
  void captureNewFrameDevice(const void* d_pixels, int width, int height, int channels, int stride, double time_stamp) {
    captureNewFrame(time_stamp);
    check(ekf_set_frame_raw_device(h_, d_pixels, width, height, channels, stride));
  }
  // the matcher frame as the device consumers see it: height rows of width bytes
  std::vector<unsigned char> getFrame(int width, int height) {
    std::vector<unsigned char> g((size_t)width * height);
    check(ekf_get_frame(h_, g.data(), width));
    return g;
  }
  // ---- rectification for pinhole consumers: raw = false the matcher frame, true the raw frame ----
  // K = (fx, fy, cx, cy) of the pinhole camera that the rectified images and pixels of that resolution belong to
  ekf_sba_camera rectifiedCamera(bool raw = false) {
    ekf_sba_camera K = {0, 0, 0, 0};
    check(ekf_rectified_camera(h_, raw ? 1 : 0, &K));
    return K;
  }
  // the held frame with the lens distortion removed on the device: height rows of width * channels bytes
  std::vector<unsigned char> getFrameRectified(int width, int height, int channels = 1, bool raw = false) {
    std::vector<unsigned char> g((size_t)width * height * channels);
    check(ekf_get_frame_rectified(h_, raw ? 1 : 0, g.data(), width * channels));
    return g;
  }
  // pixels (u, v) of the distorted image -> pixels of the rectified one, same resolution; 2 doubles per point
  std::vector<double> undistortPixels(const std::vector<double>& uv, bool raw = false) {
    std::vector<double> out(uv.size());
    check(ekf_undistort_pixels(h_, raw ? 1 : 0, uv.data(), (int)(uv.size() / 2), out.data()));
    return out;
  }
  double getDt() const { return ekf_get_dt(h_); }

  int addFeature(float u, float v) { return count(ekf_add_feature(h_, u, v)); }   // cv::Point2f pf
  void removeFeature(int index) { check(ekf_remove_feature(h_, index)); }
  void predict(const float* Translation_Speed_Control = nullptr, const float* Rotational_Speed_Control = nullptr,
               bool Vcontrol = false) {
    check(ekf_predict(h_, Translation_Speed_Control, Rotational_Speed_Control, Vcontrol ? 1 : 0));
  }
  // What Patch::findMatch / drawPrediction consume after predict(): per-feature h, flags, 2x2 St blocks.
  void predictions(std::vector<float>& h, std::vector<unsigned char>& visible, std::vector<unsigned char>& remove,
                   std::vector<float>& S2x2) {
    const int N = numOfFeatures();
    h.resize(2 * N); visible.resize(N); remove.resize(N); S2x2.resize(4 * N);
    check(ekf_get_predictions(h_, h.data(), visible.data(), remove.data(), S2x2.data(), nullptr, nullptr));
  }
  // update(): the reference takes z from Patch::findMatch inside update(); here the matcher's
  // output is passed in: z (2 per listed feature) and the feature indices that matched.
  void update(const std::vector<float>& z, const std::vector<int>& indices, bool forsePlane = false) {
    check(ekf_update(h_, z.data(), indices.data(), (int)indices.size(), forsePlane ? 1 : 0));
  }
  // Ft (member `Ft`, vR.hpp:36) and the 13x13 process noise of the last predict(), column-major
  void motionJacobian(float Ft[169], float Q[169]) { check(ekf_get_motion_jacobian(h_, Ft, Q)); }
  void measure() { check(ekf_measure(h_)); }   // recompute h/H at the current state (vR.cpp:1080-1117)
  // The image-independent pieces of the reference's two-stage update() (vR.cpp:964-1130):
  // every 1-point hypothesis on the device; returns the index (into `indices`) of the best one.
  int ransac1Point(const std::vector<float>& z, const std::vector<int>& indices, double threshold_px,
                   std::vector<int>& counts, std::vector<unsigned char>& inliers_of_best) {
    const int M = (int)indices.size();
    int best = -1;
    counts.resize(M); inliers_of_best.resize(M);
    check(ekf_ransac_1point(h_, z.data(), indices.data(), M, threshold_px, counts.data(), inliers_of_best.data(), &best));
    return best;
  }
  // high-innovation rescue after the low-innovation update; cam_before = mu[0:7] before that update
  std::vector<unsigned char> rescueHighInnovation(const float cam_before[7], const std::vector<float>& z,
                                                  const std::vector<int>& indices, double chi2_threshold = 1.0) {
    std::vector<unsigned char> hi(indices.size());
    check(ekf_rescue_high_innovation(h_, cam_before, z.data(), indices.data(), (int)indices.size(), chi2_threshold,
                                     hi.data()));
    return hi;
  }
  // update() as the reference runs it (USE_RANSAC, vR.cpp:964-1130 + 1245-1284): RANSAC -> low-innovation update ->
  // rescue -> second update (+ forsePlane rows) in one call.  seed = 0: best hypothesis; else srand(seed) replay.
  void updateTwoStage(const std::vector<float>& z, const std::vector<int>& indices, bool forsePlane, unsigned int seed,
                      float sigma_pixel, std::vector<unsigned char>& isInLi, std::vector<unsigned char>& isInHi) {
    isInLi.assign(indices.size(), 0); isInHi.assign(indices.size(), 0);
    check(ekf_update_two_stage(h_, z.data(), indices.data(), (int)indices.size(), forsePlane ? 1 : 0, seed,
                               2.0 * sigma_pixel, 1.0, isInLi.data(), isInHi.data(), nullptr));
  }
  // ---- image side: captureNewFrame's frame, Patch::findMatch for every visible feature -------------
  // gray: 8-bit single-channel frame after the node's resize (image_width x image_height of the config)
  void setFrame(const unsigned char* gray, int width, int height, int stride) {
    check(ekf_set_frame(h_, gray, width, height, stride));
  }
  // z (2 per feature, -1 -1 when not found), found flags, NCC scores; threshold = patch_matching_threshold
  void findMatches(std::vector<float>& z, std::vector<unsigned char>& found, std::vector<float>& score,
                   double threshold = 0.8) {
    const int N = numOfFeatures();
    z.resize(2 * (size_t)N); found.resize(N); score.resize(N);
    check(ekf_find_matches(h_, threshold, z.data(), found.data(), score.data()));
  }
  std::vector<unsigned char> patch(int index, bool matching = false, int window_size = 0) {
    std::vector<unsigned char> p((size_t)window_size * window_size);
    check(ekf_get_patch(h_, index, matching ? 1 : 0, p.data()));
    return p;
  }
  // drawPrediction's ellipse parameters (computeEllipsoidParameters, vR.cpp:1368-1382): 3 ints per feature
  // (semi-axis of the smaller eigenvalue, of the larger one, angle in degrees) -- what ekf_get_search_ellipses writes
  std::vector<int> searchEllipses(int sigma_size) {
    std::vector<int> e(3 * (size_t)numOfFeatures());
    check(ekf_get_search_ellipses(h_, sigma_size, e.data()));
    return e;
  }
  // the N x 12 table behind points.txt (RosVSLAM::getPointsFeatures, RosVSLAMRansac.cpp:340-418)
  std::vector<float> getPointsFeatures(bool convert_inverse_depth = true) {
    std::vector<float> t(12 * (size_t)numOfFeatures());
    check(ekf_export_points(h_, t.data(), convert_inverse_depth ? 1 : 0));
    return t;
  }

  // the same table in the reference's own layout (rows by Patch::real_index, the patches archived at removal
  // included): `rows` receives the row count; what `f_points << slam.getPointsFeatures()` streams
  std::vector<float> getPointsTable(int* rows = nullptr) {
    int r = 0;
    check(ekf_export_points_table(h_, nullptr, 0, &r));
    std::vector<float> t(12 * (size_t)r);
    if (r) check(ekf_export_points_table(h_, t.data(), r, &r));
    if (rows) *rows = r;
    return t;
  }
  // Patch::real_index / Patch::n_find per live feature
  void featureIds(std::vector<int>& real_index, std::vector<int>& n_find) {
    real_index.assign((size_t)numOfFeatures(), 0);
    n_find.assign((size_t)numOfFeatures(), 0);
    check(ekf_get_feature_ids(h_, real_index.data(), n_find.data()));
  }
  // Patch::n_tot (Patch.cpp:85, 218), Patch::isInInnovation (vR.cpp:520, 532, 561; Patch.cpp:281), Patch::center
  // (2 floats per feature; Patch.cpp:93, 253, 279) and the sticky Patch::removeFlag (vR.cpp:519, Patch.cpp:149)
  void featureTrack(std::vector<int>& n_tot, std::vector<unsigned char>& in_innovation, std::vector<float>& center,
                    std::vector<unsigned char>& remove_flag) {
    const size_t N = (size_t)numOfFeatures();
    n_tot.assign(N, 0); in_innovation.assign(N, 0); center.assign(2 * N, 0.f); remove_flag.assign(N, 0);
    check(ekf_get_feature_track(h_, n_tot.data(), in_innovation.data(), center.data(), remove_flag.data()));
  }
  // for a caller's own matcher: a negative value (center == nullptr) leaves that field alone
  void setFeatureTrack(int index, int n_tot, int in_innovation, const float* center, int remove_flag) {
    check(ekf_set_feature_track(h_, index, n_tot, in_innovation, center, remove_flag));
  }
  // VSlamFilter::findNewFeatures (vR.cpp:783-837): mask + goodFeaturesToTrack(frame, features, num, 0.01f, 12, mask)
  // on the device, the corners added in order; returns the corners, 2 floats each (num <= 0: nInitFeatures, and the
  // corners are added without being returned)
  std::vector<float> findNewFeatures(int num = -1, double quality_level = 0.01, double min_distance = 12.0,
                                     bool add = true) {
    const int cap = std::max(num, 1);
    std::vector<float> uv(2 * (size_t)cap);
    int n = 0;
    check(ekf_find_new_features(h_, num > 0 ? num : -1, quality_level, min_distance, add ? 1 : 0,
                                num > 0 ? uv.data() : nullptr, &n));
    uv.resize(num > 0 ? 2 * (size_t)n : 0);
    return uv;
  }
  // the end of VSlamFilter::update() (vR.cpp:1294-1317): quality rule + removal, visible count, eviction and seeding
  // below min_features, convert2XYZ_ifLinearAll; returns the removed pre-removal indices (descending)
  std::vector<int> endUpdate(float matching_ratio = 0.2f, bool seed = true, int* n_visible = nullptr,
                             int* n_seeded = nullptr) {
    std::vector<int> removed((size_t)std::max(numOfFeatures(), 1));
    int nr = 0;
    check(ekf_end_update(h_, matching_ratio, seed ? 1 : 0, removed.data(), &nr, n_visible, n_seeded));
    removed.resize((size_t)nr);
    return removed;
  }

  // Point4sba (mono-slam vslamRansac.cpp:1319-1336): (real_index, (int) z.x, (int) z.y) of the features in innovation
  // and XYZ-coded, z the track centre; row 0 is (re)written while its first entry is 0, every later row needs
  // u < 640 && v < 480; no feature: the single row 0 0 0.  3 ints per row, as formats.point4sba_rows.
  std::vector<int> keyframeProjections() {
    std::vector<int> ri, nf, nt, pos, cod;
    std::vector<unsigned char> inn, rem;
    std::vector<float> cen;
    featureIds(ri, nf);
    featureTrack(nt, inn, cen, rem);
    pos.assign(ri.size(), 0);
    cod.assign(ri.size(), 0);
    check(ekf_get_feature_layout(h_, pos.data(), cod.data()));
    std::vector<int> rows(3, 0);
    for (size_t i = 0; i < ri.size(); ++i) {
      if (!inn[i] || cod[i] != 1) continue;
      const int r[3] = {ri[i], (int)cen[2 * i], (int)cen[2 * i + 1]};
      if (rows[0] == 0) {
        rows[0] = r[0]; rows[1] = r[1]; rows[2] = r[2];
      } else if (r[1] < 640 && r[2] < 480) {
        rows.insert(rows.end(), r, r + 3);
      }
    }
    return rows;
  }

  std::vector<float> getState() {              // VectorXf(14), vR.cpp:135-140
    std::vector<float> s(STATE_DIM);
    check(ekf_get_state(h_, s.data(), 0, STATE_DIM));
    return s;
  }
  std::vector<float> getSigma() {              // MatrixXf 14x14 column-major, vR.cpp:131-133
    std::vector<float> s(STATE_DIM * STATE_DIM);
    check(ekf_get_sigma_block(h_, s.data(), 0, 0, STATE_DIM, STATE_DIM));
    return s;
  }
  // protected members `mu` / `Sigma` that RosVSLAM reads directly (RosVSLAMRansac.cpp:68-183)
  std::vector<float> mu() {
    std::vector<float> s(ekf_state_dim(h_));
    check(ekf_get_state(h_, s.data(), 0, (int)s.size()));
    return s;
  }
  std::vector<float> SigmaBlock(int r0, int c0, int rows, int cols) {
    std::vector<float> s((size_t)rows * cols);
    check(ekf_get_sigma_block(h_, s.data(), r0, c0, rows, cols));
    return s;
  }
  void convert2XYZ_ifLinear(int index) { count(ekf_convert_xyz_if_linear(h_, index)); }
  void convert2XYZ_ifLinearAll() { count(ekf_convert_xyz_if_linear_all(h_)); }
  // inverseDepth2XyzWorld(f, J, 1) + J Sigma J^T for feature `index` (RosVSLAMRansac.cpp:177-183)
  void featureXYZ(int index, float xyz[3], float cov3x3[9]) { check(ekf_feature_xyz(h_, index, xyz, cov3x3)); }
  int numOfFeatures() const { return ekf_num_features(h_); }
  float Covariance_Parameter() {
    double v = 0;
    check(ekf_covariance_parameter(h_, &v));
    return (float)v;
  }
  ekf_filter* handle() { return h_; }

 private:
  void check(int rc) { if (rc != EKF_OK) throw std::runtime_error(ekf_last_error(h_)); }
  int count(int rc) { if (rc < 0) throw std::runtime_error(ekf_last_error(h_)); return rc; }
  ekf_filter* h_ = nullptr;
  double old_ts_ = -1;   // vR.cpp:145
};

// SysSbaHip -- header-only mirror of the part of the reference's `sba::SysSBA` (sparse_bundle_adjustment/include/
// sparse_bundle_adjustment/sba.h) that sba_add drives, over the ekf_sba_* functions of ekf_monoslam.h: monocular
// projections, node 0 fixed, doSBA with the CHOLMOD solve or the block-Jacobi PCG, calcCost /
// calcRMSCost, the pseudo-Huber cost and the pruning of outlying projections.  Poses are
// (x y z qw qx qy qz), points (x y z), as plain double arrays.  The linear solver belongs to the handle, so it is a
// constructor argument: EKF_SBA_SOLVER_CHOLESKY (the default, at most 1024 nodes) or EKF_SBA_SOLVER_BPCG.
class SysSbaHip {
 public:
  explicit SysSbaHip(double fx, double fy, double cx, double cy, int capacity_nodes = 256,
                     int capacity_points = 65536, int capacity_projections = 262144, int device = 0,
                     int solver = EKF_SBA_SOLVER_CHOLESKY) {
    const ekf_sba_camera K = {fx, fy, cx, cy};
    if (ekf_sba_create_solver(&K, capacity_nodes, capacity_points, capacity_projections, device, solver, &h_) != EKF_OK)
      throw std::runtime_error(std::string("ekf_sba_create_solver: ") + ekf_sba_last_error(nullptr));
  }
  ~SysSbaHip() { ekf_sba_destroy(h_); }
  SysSbaHip(const SysSbaHip&) = delete;
  SysSbaHip& operator=(const SysSbaHip&) = delete;

  // addNode (sba.cpp:83-100): returns the node index
  int addNode(const double pose7[7]) { const int i = counts(0); check(ekf_sba_add_nodes(h_, 1, pose7)); return i; }
  // addPoint: returns the point index
  int addPoint(const double xyz[3]) { const int i = counts(1); check(ekf_sba_add_points(h_, 1, xyz)); return i; }
  // addMonoProj (sba.cpp:133-143): false when the (node, point) pair is already there
  bool addMonoProj(int ci, int pi, const double uv[2]) {
    int added = 0;
    check(ekf_sba_add_projections(h_, 1, &ci, &pi, uv, &added));
    return added == 1;
  }
  // doSBA(niter, sLambda): the iteration count, -1 for an empty problem
  int doSBA(int niter, double sLambda = 1.0e-4) {
    int it = 0;
    check(ekf_sba_run(h_, niter, sLambda, &it));
    return it;
  }
  // doSBA(niter, sLambda, useCSparse, initTol, maxCGiters) (sba.cpp:1312): useCSparse 0 (dense Cholesky) and 1
  // (sparse Cholesky) are this project's Cholesky solver, 3 (SBA_BLOCK_JACOBIAN_PCG) its PCG solver with the two CG
  // settings; 2 (SBA_GRADIENT) is not supported.  The choice must be the one the handle was constructed with.
  int doSBA(int niter, double sLambda, int useCSparse, double initTol = 1.0e-8, int maxCGiters = 100) {
    if (useCSparse == 2) throw std::runtime_error("SysSbaHip::doSBA: useCSparse = 2 (SBA_GRADIENT) is not supported");
    if (useCSparse != 0 && useCSparse != 1 && useCSparse != EKF_SBA_SOLVER_BPCG)
      throw std::runtime_error("SysSbaHip::doSBA: useCSparse must be 0, 1 or 3");
    const int want = useCSparse == EKF_SBA_SOLVER_BPCG ? EKF_SBA_SOLVER_BPCG : EKF_SBA_SOLVER_CHOLESKY;
    if (want != solver())
      throw std::runtime_error("SysSbaHip::doSBA: useCSparse does not match the solver the handle was constructed with");
    if (want == EKF_SBA_SOLVER_BPCG) check(ekf_sba_set_cg(h_, initTol, maxCGiters));
    return doSBA(niter, sLambda);
  }
  int solver() { int v = 0; check(ekf_sba_get_solver(h_, &v)); return v; }
  // per LM iteration of the last doSBA with the PCG solver: the CG iterations made
  std::vector<int> cgIterations() {
    int n = 0;
    check(ekf_sba_get_cg_log(h_, 0, nullptr, nullptr, nullptr, &n));
    std::vector<int> v((size_t)n);
    check(ekf_sba_get_cg_log(h_, n, v.data(), nullptr, nullptr, &n));
    return v;
  }
  double calcCost() { double c = 0, r = 0; check(ekf_sba_cost(h_, 10000.0, &c, &r)); return c; }
  double calcRMSCost(double dist = 10000.0) { double c = 0, r = 0; check(ekf_sba_cost(h_, dist, &c, &r)); return r; }
  // SysSBA::huber (sba.h:113): the pseudo-Huber width in pixels, 0 = off
  void setHuber(double huber) { check(ekf_sba_set_huber(h_, huber)); }
  double huber() { double v = 0; check(ekf_sba_get_huber(h_, &v)); return v; }
  // countBad / removeBad / reduceTracks / numBadPoints / calcAvgError (sba.cpp:365-502)
  int countBad(double dist) { int n = 0; check(ekf_sba_count_bad(h_, dist, &n)); return n; }
  int removeBad(double dist) { int n = 0; check(ekf_sba_remove_bad(h_, dist, &n)); return n; }
  int reduceTracks() { int n = 0; check(ekf_sba_reduce_tracks(h_, &n)); return n; }
  int numBadPoints() { int n = 0; check(ekf_sba_num_bad_points(h_, &n)); return n; }
  double calcAvgError() { double a = 0; check(ekf_sba_avg_error(h_, &a)); return a; }
  std::vector<double> nodes() { std::vector<double> v(7 * (size_t)counts(0)); check(ekf_sba_get_nodes(h_, v.data())); return v; }
  std::vector<double> points() { std::vector<double> v(3 * (size_t)counts(1)); check(ekf_sba_get_points(h_, v.data())); return v; }
  int numNodes() { return counts(0); }
  int numPoints() { return counts(1); }
  int numProjections() { return counts(2); }
  ekf_sba* handle() { return h_; }

 private:
  int counts(int which) {
    int c[3] = {0, 0, 0};
    check(ekf_sba_counts(h_, &c[0], &c[1], &c[2]));
    return c[which];
  }
  void check(int rc) { if (rc != EKF_OK) throw std::runtime_error(ekf_sba_last_error(h_)); }
  ekf_sba* h_ = nullptr;
};

// KeyframeSelectorHip -- header-only mirror of the node's key-frame rule (mono-slam monoslam_ransac.cpp:585-687) over
// the ekf_keyframe_* functions of ekf_monoslam.h: observe(frameId) after every update() is one small
// launch on the filter's stream and one read-back; the candidate's and the emitted frame's image stay on the device.
// The selector must not outlive the use of its filter (observe needs it); values are plain float / int arrays.
class KeyframeSelectorHip {
 public:
  struct Emitted {
    int id = 0;
    float pose[7] = {};                 // r, q
    float cov[49] = {};                 // Sigma[0:7,0:7], column-major
    std::vector<int> projections;       // rows (real_index, u, v); the single row 0 0 0 = none
  };
  struct Result {
    int action = EKF_KF_NONE;           // enum ekf_keyframe_action
    float dist = 0, cov = 0;            // poses_diff against the last key frame, Covariance_Parameter
    bool emitted() const { return action == EKF_KF_EMIT_CURRENT || action == EKF_KF_EMIT_CANDIDATE || action == EKF_KF_EMIT_FIRST; }
  };

  explicit KeyframeSelectorHip(VSlamFilterHip& filter, float MoveThresh = 18.f, bool keep_current_projections = false)
      : f_(filter.handle()) {
    if (ekf_keyframe_create(f_, MoveThresh, &h_) != EKF_OK)
      throw std::runtime_error(std::string("ekf_keyframe_create: ") + ekf_keyframe_last_error(nullptr));
    if (keep_current_projections) check(ekf_keyframe_set_option(h_, EKF_KF_OPT_KEEP_CURRENT_PROJECTIONS, 1));
  }
  // a raw selector: it also keeps the camera's own frame (raw_width x raw_height x channels, as given to
  // VSlamFilterHip::captureNewFrame) of the candidate and of the emitted key frame -- the image the node saves
  KeyframeSelectorHip(VSlamFilterHip& filter, int raw_width, int raw_height, int channels, float MoveThresh = 18.f,
                      bool keep_current_projections = false)
      : f_(filter.handle()) {
    if (ekf_keyframe_create_raw(f_, MoveThresh, raw_width, raw_height, channels, &h_) != EKF_OK)
      throw std::runtime_error(std::string("ekf_keyframe_create_raw: ") + ekf_keyframe_last_error(nullptr));
    if (keep_current_projections) check(ekf_keyframe_set_option(h_, EKF_KF_OPT_KEEP_CURRENT_PROJECTIONS, 1));
  }
  ~KeyframeSelectorHip() { ekf_keyframe_destroy(h_); }
  KeyframeSelectorHip(const KeyframeSelectorHip&) = delete;
  KeyframeSelectorHip& operator=(const KeyframeSelectorHip&) = delete;

  Result observe(int frameId) {
    Result r;
    check(ekf_keyframe_observe(h_, f_, frameId, &r.action, &r.dist, &r.cov));
    return r;
  }
  // the last emitted key frame: what one record of nodes_and_prjcts.txt / cams_cov.txt holds
  Emitted emitted() {
    Emitted e;
    double pose[7], cov[49];
    int n = 0;
    check(ekf_keyframe_get_emitted(h_, &e.id, pose, cov, 0, nullptr, &n));
    e.projections.resize(3 * (size_t)n);
    check(ekf_keyframe_get_emitted(h_, nullptr, nullptr, nullptr, n, e.projections.data(), &n));
    std::copy(pose, pose + 7, e.pose);
    std::copy(cov, cov + 49, e.cov);
    return e;
  }
  // the emitted key frame's image: height rows of width bytes
  std::vector<unsigned char> emittedImage(int width, int height) {
    std::vector<unsigned char> g((size_t)width * height);
    check(ekf_keyframe_get_image(h_, g.data(), width));
    return g;
  }
  // the emitted key frame's raw image (a raw selector): raw_height rows of raw_width * channels bytes
  std::vector<unsigned char> emittedRawImage(int raw_width, int raw_height, int channels) {
    std::vector<unsigned char> p((size_t)raw_width * raw_height * channels);
    check(ekf_keyframe_get_raw_image(h_, p.data(), raw_width * channels));
    return p;
  }
  // the emitted key frame's image with the lens distortion removed: the grey frame, or with `raw`
  // the raw frame of a raw selector; height rows of width * channels bytes
  std::vector<unsigned char> emittedImageRectified(int width, int height, int channels = 1, bool raw = false) {
    std::vector<unsigned char> g((size_t)width * height * channels);
    check(ekf_keyframe_get_image_rectified(h_, raw ? 1 : 0, g.data(), width * channels));
    return g;
  }
  // the undistorted track centres behind the rows of emitted().projections, same order, 2 doubles per row (none for the
  // 0 0 0 placeholder), in matcher or (`raw`) raw pixels
  std::vector<double> emittedRowsRectified(bool raw = false) {
    int n = 0;
    check(ekf_keyframe_get_emitted_rectified(h_, raw ? 1 : 0, 0, nullptr, &n));
    std::vector<double> uv(2 * (size_t)n);
    if (n) check(ekf_keyframe_get_emitted_rectified(h_, raw ? 1 : 0, n, uv.data(), &n));
    return uv;
  }
  void state(float last_pose[7], float last_vrot[3], float* min_cov, int* candidate_id) {
    check(ekf_keyframe_get_state(h_, last_pose, last_vrot, min_cov, candidate_id));
  }
  void reset() { check(ekf_keyframe_reset(h_)); }
  ekf_keyframe* handle() { return h_; }

 private:
  void check(int rc) { if (rc != EKF_OK) throw std::runtime_error(ekf_keyframe_last_error(h_)); }
  ekf_filter* f_ = nullptr;
  ekf_keyframe* h_ = nullptr;
};

// DenseStereoHip -- header-only mirror of the dense plane-sweep step over the ekf_dense_* functions
// of ekf_monoslam.h: up to 16 posed pinhole views of one size on the device, sweep() = one k_plane_sweep launch per depth
// map, filter() = the geometric consistency check against the swept maps of the sources.  Values are plain arrays.
class DenseStereoHip {
 public:
  struct Depth {
    std::vector<float> depth;            // 0 = none
    std::vector<int> plane;              // -1 = none
    std::vector<unsigned int> cost;
    std::vector<unsigned char> views;
  };

  DenseStereoHip(int width, int height, int max_views = 16, int device = 0) : w_(width), h_(height) {
    if (ekf_dense_create(width, height, max_views, device, &d_) != EKF_OK)
      throw std::runtime_error(std::string("ekf_dense_create: ") + ekf_dense_last_error(nullptr));
  }
  ~DenseStereoHip() { ekf_dense_destroy(d_); }
  DenseStereoHip(const DenseStereoHip&) = delete;
  DenseStereoHip& operator=(const DenseStereoHip&) = delete;

  // height rows of width bytes, `pitch` bytes apart (0: tight); K = fx fy cx cy; pose7 = x y z qw qx qy qz
  void setView(int slot, const unsigned char* gray, const double K[4], const double pose7[7], int pitch = 0) {
    check(ekf_dense_set_view(d_, slot, gray, pitch ? pitch : w_, K, pose7));
  }
  void setViewDevice(int slot, const void* d_gray, const double K[4], const double pose7[7], int pitch = 0) {
    check(ekf_dense_set_view_device(d_, slot, d_gray, pitch ? pitch : w_, K, pose7));
  }
  // the selector's last emitted key frame, rectified on the device straight into the slot
  void setViewFromKeyframe(int slot, KeyframeSelectorHip& selector, const double pose7[7], bool raw = false) {
    check(ekf_dense_set_view_from_keyframe(d_, slot, selector.handle(), raw ? 1 : 0, pose7));
  }
  // colour views: height rows of width x 3 bytes in B, G, R order, `pitch` bytes apart (0: tight); the
  // slot keeps the colour image and sweeps its grey conversion
  void setViewColour(int slot, const unsigned char* bgr, const double K[4], const double pose7[7], int pitch = 0) {
    check(ekf_dense_set_view_colour(d_, slot, bgr, pitch ? pitch : 3 * w_, K, pose7));
  }
  void setViewColourDevice(int slot, const void* d_bgr, const double K[4], const double pose7[7], int pitch = 0) {
    check(ekf_dense_set_view_colour_device(d_, slot, d_bgr, pitch ? pitch : 3 * w_, K, pose7));
  }
  // the last emitted raw key frame of a 3-channel raw selector
  void setViewColourFromKeyframe(int slot, KeyframeSelectorHip& selector, const double pose7[7]) {
    check(ekf_dense_set_view_colour_from_keyframe(d_, slot, selector.handle(), pose7));
  }
  bool hasColour(int slot) const { return ekf_dense_get_view_colour(d_, slot, nullptr, 0) == EKF_OK; }
  std::vector<unsigned char> viewColour(int slot) {
    std::vector<unsigned char> c(3 * pixels());
    check(ekf_dense_get_view_colour(d_, slot, c.data(), 3 * w_));
    return c;
  }
  void setPose(int slot, const double pose7[7]) { check(ekf_dense_set_pose(d_, slot, pose7)); }
  std::vector<unsigned char> viewImage(int slot) {
    std::vector<unsigned char> g(pixels());
    check(ekf_dense_get_view(d_, slot, g.data(), w_, nullptr, nullptr));
    return g;
  }
  void sweep(int ref, const std::vector<int>& src, double w_min, double w_max, int planes = 64, int radius = 2, int trunc = 40) {
    check(ekf_dense_sweep(d_, ref, src.data(), (int)src.size(), w_min, w_max, planes, radius, trunc));
  }
  // the sweep with semi-global cost aggregation: the same swept map for filter / depth / points and the
  // fusion.  p1, p2 <= 0: 2 n and 16 n with n = (2 radius + 1)^2 src.size(), the values of the synthetic flat-patch scenes
  // (not measured on real imagery); paths is 4 or 8
  void sweepSgm(int ref, const std::vector<int>& src, double w_min, double w_max, int planes = 64, int radius = 1, int trunc = 40,
                int p1 = 0, int p2 = 0, int paths = 8) {
    const int n = (2 * radius + 1) * (2 * radius + 1) * (int)src.size();
    check(ekf_dense_sweep_sgm(d_, ref, src.data(), (int)src.size(), w_min, w_max, planes, radius, trunc, p1 > 0 ? p1 : 2 * n,
                              p2 > 0 ? p2 : 16 * n, paths));
    sgm_planes_ = planes;
  }
  // planes x height x width values of the last sweepSgm, whose slot `slot` must be: the aggregated or the raw cost volume
  std::vector<unsigned int> volume(int slot, bool aggregated = true) {
    std::vector<unsigned int> v((size_t)sgm_planes_ * pixels());
    check(ekf_dense_get_volume(d_, slot, aggregated ? 1 : 0, v.data()));
    return v;
  }
  // HIP-event milliseconds and launch counts of k_sweep_volume ([0]), k_sgm_path of direction 0 .. 7 ([1] .. [8]), k_sgm_winner ([9])
  void getSgmProfile(double kernel_ms[10], long long launches[10]) { check(ekf_dense_get_sgm_profile(d_, kernel_ms, launches)); }
  // the two sweeps with the census matching cost, for key frames whose exposure or gain differ: the
  // same maps for filter / depth / points and the fusion; here trunc bounds a Hamming distance of 62 bits
  void sweepCensus(int ref, const std::vector<int>& src, double w_min, double w_max, int planes = 64, int radius = 2, int trunc = 40) {
    check(ekf_dense_sweep_census(d_, ref, src.data(), (int)src.size(), w_min, w_max, planes, radius, trunc));
  }
  // p1, p2 <= 0: the 2 n and 16 n of sweepSgm, not measured on real imagery
  void sweepSgmCensus(int ref, const std::vector<int>& src, double w_min, double w_max, int planes = 64, int radius = 1, int trunc = 40,
                      int p1 = 0, int p2 = 0, int paths = 8) {
    const int n = (2 * radius + 1) * (2 * radius + 1) * (int)src.size();
    check(ekf_dense_sweep_sgm_census(d_, ref, src.data(), (int)src.size(), w_min, w_max, planes, radius, trunc, p1 > 0 ? p1 : 2 * n,
                                     p2 > 0 ? p2 : 16 * n, paths));
    sgm_planes_ = planes;
  }
  // height x width census descriptors of a set slot (bits 0 .. 61), computed first if its image changed since
  std::vector<unsigned long long> census(int slot) {
    std::vector<unsigned long long> t(pixels());
    check(ekf_dense_get_census(d_, slot, t.data()));
    return t;
  }
  // HIP-event milliseconds and launch counts of k_census ([0]), k_plane_sweep_census ([1]), k_sweep_volume_census ([2])
  void getCensusProfile(double kernel_ms[3], long long launches[3]) { check(ekf_dense_get_census_profile(d_, kernel_ms, launches)); }
  // the sweeps with best-K source selection: per pixel and plane the n_best cheapest of the sources,
  // for views that do not all see every reference pixel; census: the matching cost of sweepCensus; paths 0: the pixel-wise
  // winner; 4 or 8: the aggregation of sweepSgm, with its 2 n and 16 n for p1, p2 <= 0 where n = (2 radius + 1)^2 n_best
  void sweepBest(int ref, const std::vector<int>& src, int n_best, double w_min, double w_max, int planes = 64, int radius = 2,
                 int trunc = 40, bool census = false, int paths = 0, int p1 = 0, int p2 = 0) {
    const int n = (2 * radius + 1) * (2 * radius + 1) * n_best;
    if (paths != 0) { p1 = p1 > 0 ? p1 : 2 * n; p2 = p2 > 0 ? p2 : 16 * n; }
    check(ekf_dense_sweep_best(d_, ref, src.data(), (int)src.size(), n_best, w_min, w_max, planes, radius, trunc, census ? 1 : 0, paths,
                               p1, p2));
    if (paths != 0) sgm_planes_ = planes;
  }
  // HIP-event milliseconds and launch counts of k_plane_sweep_best ([0]), k_plane_sweep_best_census ([1]), k_sweep_volume_best
  // ([2]), k_sweep_volume_best_census ([3])
  void getBestProfile(double kernel_ms[4], long long launches[4]) { check(ekf_dense_get_best_profile(d_, kernel_ms, launches)); }
  void filter(int ref, const std::vector<int>& src, double rel_tol = 0.01, int min_agree = 1) {
    check(ekf_dense_filter(d_, ref, src.data(), (int)src.size(), rel_tol, min_agree));
  }
  // the runner-up cost and the uniqueness test.  keepRunnerUp: while on, every sweep above also records
  // its slot's runner-up cost, the least cost at least two planes from the winner (0xFFFFFFFF: no such plane); runnerUp reads
  // it.  filterUnique: filter, which also drops the pixels of ref with (C2 - cost) 100 < uniqueness C2; uniqueness is 0 .. 100
  // per cent, 0 being filter itself, and more than 0 needs ref swept while keepRunnerUp was on
  void keepRunnerUp(bool on = true) { check(ekf_dense_keep_runner_up(d_, on ? 1 : 0)); }
  std::vector<unsigned int> runnerUp(int slot) {
    std::vector<unsigned int> r(pixels());
    check(ekf_dense_get_runner_up(d_, slot, r.data()));
    return r;
  }
  void filterUnique(int ref, const std::vector<int>& src, int uniqueness, double rel_tol = 0.01, int min_agree = 1) {
    check(ekf_dense_filter_unique(d_, ref, src.data(), (int)src.size(), rel_tol, min_agree, uniqueness));
  }
  // HIP-event milliseconds and launch counts of k_plane_sweep_unique ([0]), k_plane_sweep_census_unique ([1]),
  // k_plane_sweep_best_unique ([2]), k_plane_sweep_best_census_unique ([3]), k_sgm_winner_unique ([4]), k_depth_filter_unique ([5])
  void getUniqueProfile(double kernel_ms[6], long long launches[6]) { check(ekf_dense_get_unique_profile(d_, kernel_ms, launches)); }
  // the speckle filter.  filterSpeckle: drops, from the slot's filtered map in place, the connected
  // segments of fewer than min_size pixels; two 4-neighbours share a segment if both have a plane and the planes differ by at
  // most max_diff.  segments: the labels (the least index y width + x of a pixel's segment, 0xFFFFFFFF: no plane) and sizes
  // before the removal of the last filterSpeckle, whose slot `slot` must be.  speckleMaps: the same for height x width maps
  // of the caller's, filtered in place; it touches no slot
  struct Segments {
    std::vector<unsigned int> label, size;
  };
  void filterSpeckle(int slot, int min_size, int max_diff = 1) { check(ekf_dense_filter_speckle(d_, slot, min_size, max_diff)); }
  Segments segments(int slot) {
    Segments s;
    s.label.resize(pixels()); s.size.resize(pixels());
    check(ekf_dense_get_segments(d_, slot, s.label.data(), s.size.data()));
    return s;
  }
  Segments speckleMaps(std::vector<float>& depth, std::vector<int>& plane, int min_size, int max_diff = 1) {
    if (depth.size() != pixels() || plane.size() != pixels()) throw std::runtime_error("speckleMaps: depth and plane are height x width");
    Segments s;
    s.label.resize(pixels()); s.size.resize(pixels());
    check(ekf_dense_speckle_host(d_, depth.data(), plane.data(), min_size, max_diff, s.label.data(), s.size.data()));
    return s;
  }
  // HIP-event milliseconds and launch counts of k_speckle_label ([0]), k_speckle_merge ([1]), k_speckle_count ([2]),
  // k_speckle_apply ([3])
  void getSpeckleProfile(double kernel_ms[4], long long launches[4]) { check(ekf_dense_get_speckle_profile(d_, kernel_ms, launches)); }
  Depth depth(int slot, bool filtered = false) {
    Depth r;
    r.depth.resize(pixels()); r.plane.resize(pixels()); r.cost.resize(pixels()); r.views.resize(pixels());
    check(ekf_dense_get_depth(d_, slot, filtered ? 1 : 0, r.depth.data(), r.plane.data(), r.cost.data(), r.views.data()));
    return r;
  }
  // height x width x 3 world points, NaN where there is no depth
  std::vector<double> points(int slot, bool filtered = false) {
    std::vector<double> xyz(3 * pixels());
    check(ekf_dense_get_points(d_, slot, filtered ? 1 : 0, xyz.data()));
    return xyz;
  }
  void profile(bool enable) { check(ekf_dense_profile(d_, enable ? 1 : 0)); }
  // HIP-event milliseconds and launch counts of k_plane_sweep ([0]) and k_depth_filter_points ([1])
  void getProfile(double kernel_ms[2], long long launches[2]) { check(ekf_dense_get_profile(d_, kernel_ms, launches)); }
  int width() const { return w_; }
  int height() const { return h_; }
  ekf_dense* handle() { return d_; }

 private:
  size_t pixels() const { return (size_t)w_ * (size_t)h_; }
  void check(int rc) { if (rc != EKF_OK) throw std::runtime_error(ekf_dense_last_error(d_)); }
  int w_, h_;
  int sgm_planes_ = 0;
  ekf_dense* d_ = nullptr;
};

// TsdfVolumeHip -- header-only mirror of the fusion step over the ekf_fusion_* functions of
// ekf_monoslam.h: depth maps (of a DenseStereoHip slot, or host arrays) integrated into one truncated signed distance volume
// on the device, extract() = marching tetrahedra into a triangle soup in a fixed order.  raycast() / raycastView() mirror
// ekf_raycast_* (section 17): the volume seen from a pose as a depth, a normal and a grey image.  Values are plain arrays.
// A colour volume (the constructor's `colour`, section 18, ekf_colour_*) also fills the `colour` arrays: B, G, R.
// weld() / mesh() mirror ekf_mesh_* (section 24): the indexed mesh welded on the device, with vertex normals on request;
// components() / prune() / pruned() its connected components and the weld without the small ones (section 25);
// smooth() / smoothed() / adjacency() either of them smoothed with Taubin's scheme, with normals of its own (section 26);
// simplify() / simplified() / simplifyMap() any of the three with its vertices clustered on a grid of cells (section 28);
// textureBegin() / textureAddView() / textureAddViewHost() / textureFinish() a per-triangle texture atlas of any of the four,
// filled from views that are fed one at a time (section 29); setRasterMesh() / rasterise() / rasteriseView() / rastered() any of
// the four, or a mesh of the caller's, seen from a pose with its vertex colours or that atlas (section 30); setDistanceMesh() /
// distance() / distancePoints() / distanceStats() how far the vertices of one of them, or points of the caller's, lie from another
// (section 31).
class TsdfVolumeHip {
 public:
  struct Mesh {
    std::vector<double> xyz;                   // 9 per triangle
    std::vector<unsigned long long> key;       // 3 per triangle: equal keys are bit-equal vertices
    std::vector<unsigned char> grey;           // 3 per triangle
    std::vector<unsigned char> colour;         // 9 per triangle, B G R of each vertex: colour volumes only
    size_t triangles() const { return key.size() / 3; }
  };
  struct IndexedMesh {                         // one vertex per distinct key of the soup, by ascending key
    std::vector<double> xyz;                   // 3 per vertex
    std::vector<unsigned int> faces;           // 3 per triangle, into the vertices, in the soup's triangle order
    std::vector<unsigned char> grey;           // 1 per vertex
    std::vector<unsigned char> colour;         // 3 per vertex, B G R: colour volumes only
    std::vector<float> normal;                 // 3 per vertex: unit, towards free space (0 0 0: no gradient); weld(.., true) only
    std::vector<unsigned long long> key;       // 1 per vertex, ascending
    size_t vertices() const { return key.size(); }
    size_t triangles() const { return faces.size() / 3; }
  };
  struct Components {                          // of the last weld(): section 25
    std::vector<unsigned int> label;           // 1 per vertex: the least vertex index of its component
    std::vector<unsigned int> size;            // 1 per vertex: the triangles of its component
    unsigned long long count = 0;              // the number of components
  };
  struct Adjacency {                           // of the mesh the last smooth() ran on: section 26
    std::vector<unsigned int> inc;             // 1 per vertex: the triangles that contain it
    std::vector<unsigned int> deg;             // 1 per vertex: the distinct vertices that share a triangle with it
    std::vector<unsigned char> boundary;       // 1 per vertex: 1 iff it has an edge that lies in exactly one triangle
  };
  struct SimplifyStats {                       // of the last simplify(): section 28
    unsigned long long degenerate = 0;         // the triangles of which two vertices fell into one cell
    unsigned long long duplicate = 0;          // those whose unordered triple of cells a triangle with a smaller index has
  };
  struct Occlusion {                           // the ray cast that gives a view of the texture its z-buffer: section 29
    double z_near, z_far;
    double step = 0.0;                         // 0: half a voxel
    int min_count = 1;
    Occlusion(double near_, double far_, double step_ = 0.0, int min_count_ = 1)
        : z_near(near_), z_far(far_), step(step_), min_count(min_count_) {}
  };
  struct TextureAtlas {                        // of textureFinish(): section 29; triangle t owns one half of block t >> 1
    int side = 0, channels = 0;
    std::vector<unsigned char> atlas;          // side rows of side x channels bytes, row 0 first; 3 channels: B G R
    std::vector<double> uv;                    // 6 per triangle: u, v of its corners 0, 1 and 2, v measured from row 0
    std::vector<int> view;                     // 1 per triangle: the number of the view that textured it, -1: none
    std::vector<double> score;                 // 1 per triangle: twice its area in that view's pixels, 0: none
    unsigned long long n_textured = 0;         // the triangles with a view
    size_t triangles() const { return view.size(); }
  };
  struct Volume {
    std::vector<float> sum;
    std::vector<unsigned short> cnt;
    std::vector<unsigned int> gsum;
    std::vector<unsigned int> csum;            // the sums of B, G and R, three planes back to back: colour volumes only
    int maps = 0;
  };
  struct Render {                              // a pixel without a hit: depth 0, normal 0, grey 0
    int width = 0, height = 0;
    std::vector<float> depth;                  // camera-z depth, height rows of width
    std::vector<float> normal;                 // 3 per pixel: unit, world frame, towards free space
    std::vector<unsigned char> grey;
    std::vector<unsigned char> colour;         // 3 per pixel, B G R: colour volumes only
  };
  struct MeshRender : Render {                 // of rasterise(): section 30; the normal is the triangle's own, not flipped
    std::vector<int> tri;                      // the triangle of the source that the pixel shows, -1: none
    std::vector<float> bary;                   // 2 per pixel: its perspective-correct barycentrics l1, l2
    std::vector<unsigned int> cover;           // the triangles that cover the pixel: rasterise(.., cover = true) only
  };

  struct MeshDistance {                        // of distance() and distancePoints(): section 31
    std::vector<double> dist;                  // NaN for a point that is not finite
    std::vector<unsigned int> tri;             // the nearest triangle of the target, the least index among equally near ones
    std::vector<double> closest;               // 3 per point: the nearest point on it
    std::vector<signed char> side;             // the sign of (p - closest) . n of that triangle: +1 is the free-space side of a weld
    size_t points() const { return dist.size(); }
  };
  struct DistanceStats {                       // of distanceStats(): the last run over its finite points, summed in a fixed order
    unsigned long long n = 0, n_bad = 0, argmax = 0, within = 0;
    double max = 0.0, mean = 0.0, rms = 0.0;   // max: the one-sided Hausdorff distance
  };

  TsdfVolumeHip(int nx, int ny, int nz, const double origin[3], double voxel, double trunc, int device = 0, bool colour = false)
      : n_((size_t)nx * (size_t)ny * (size_t)nz), colour_(colour), voxel_(voxel) {
    if ((colour ? ekf_colour_create : ekf_fusion_create)(nx, ny, nz, origin, voxel, trunc, device, &f_) != EKF_OK)
      throw std::runtime_error(std::string("ekf_fusion_create: ") + ekf_fusion_last_error(nullptr));
  }
  bool hasColour() const { return colour_; }
  ~TsdfVolumeHip() { ekf_fusion_destroy(f_); }
  TsdfVolumeHip(const TsdfVolumeHip&) = delete;
  TsdfVolumeHip& operator=(const TsdfVolumeHip&) = delete;

  // the swept or filtered map of a slot, straight from the dense handle's device buffers
  void integrate(DenseStereoHip& dense, int slot, bool filtered = true) {
    check(ekf_fusion_integrate(f_, dense.handle(), slot, filtered ? 1 : 0));
  }
  // height tight rows of width floats (0 = none); height rows of width bytes, `pitch` bytes apart (0: tight)
  void integrateHost(const float* depth, const unsigned char* gray, int width, int height, const double K[4],
                     const double pose7[7], int pitch = 0) {
    check(ekf_fusion_integrate_host(f_, depth, gray, pitch ? pitch : width, width, height, K, pose7));
  }
  // a colour volume only: height rows of width x 3 bytes in B, G, R order, `pitch` bytes apart (0: tight)
  void integrateHostColour(const float* depth, const unsigned char* bgr, int width, int height, const double K[4],
                           const double pose7[7], int pitch = 0) {
    check(ekf_colour_integrate_host(f_, depth, bgr, pitch ? pitch : 3 * width, width, height, K, pose7));
  }
  void reset() { check(ekf_fusion_reset(f_)); }
  Volume volume() {
    Volume v;
    v.sum.resize(n_); v.cnt.resize(n_); v.gsum.resize(n_);
    check(ekf_fusion_get_volume(f_, v.sum.data(), v.cnt.data(), v.gsum.data(), &v.maps));
    if (colour_) {
      v.csum.resize(3 * n_);
      check(ekf_colour_get_volume(f_, v.csum.data()));
    }
    return v;
  }
  Mesh extract(int min_count = 1) {
    unsigned long long n = 0;
    check(ekf_fusion_extract(f_, min_count, &n));
    Mesh m;
    m.xyz.resize((size_t)n * 9); m.key.resize((size_t)n * 3); m.grey.resize((size_t)n * 3);
    check(ekf_fusion_get_mesh(f_, m.xyz.data(), m.key.data(), m.grey.data(), n));
    if (colour_) {
      m.colour.resize((size_t)n * 9);
      check(ekf_colour_get_mesh(f_, m.colour.data(), n));
    }
    return m;
  }
  // The indexed mesh, welded on the device: what sorting the keys of extract(min_count) gives, bit for bit.  It extracts first
  // unless the handle holds the soup of this min_count; the mesh of extract() stays valid.  The first weld allocates 4 bytes a
  // voxel and 1 byte a cell of scratch on the device.
  IndexedMesh weld(int min_count = 1, bool normals = false) {
    check(ekf_mesh_weld(f_, min_count, normals ? 1 : 0, &weld_vertices_, &weld_triangles_));
    weld_normals_ = normals;
    return mesh();
  }
  // the arrays of the last weld() again
  IndexedMesh mesh() { return fetch(ekf_mesh_get, weld_vertices_, weld_triangles_, weld_normals_); }
  // HIP-event milliseconds and launch counts of k_mesh_cells, k_mesh_edges, the weld's k_tsdf_scan, k_mesh_vertices, k_mesh_faces
  void getMeshProfile(double kernel_ms[5], long long launches[5]) { check(ekf_mesh_get_profile(f_, kernel_ms, launches)); }
  // The connected components of the last weld() (section 25), found on the device: two vertices are linked iff a triangle has
  // both, by index.  label: the least vertex index of a vertex's component; size: the triangles of that component.
  Components components() {
    Components c;
    check(ekf_components_find(f_, &c.count));
    c.label.resize((size_t)weld_vertices_);
    c.size.resize((size_t)weld_vertices_);
    check(ekf_components_get(f_, c.label.data(), c.size.data(), weld_vertices_));
    return c;
  }
  // The last weld() without the components of fewer than min_triangles triangles and, with `largest`, without all but the one
  // of greatest size (the least label among equals); order kept, rows bit for bit, faces re-indexed.  prune(1) is the identity;
  // the weld stays as it was.  kept (optional): the number of components kept.
  IndexedMesh prune(unsigned int min_triangles = 1, bool largest = false, unsigned long long* kept = nullptr) {
    unsigned long long nk = 0;
    check(ekf_components_prune(f_, min_triangles, largest ? 1 : 0, &pruned_vertices_, &pruned_triangles_, &nk));
    if (kept) *kept = nk;
    return pruned();
  }
  // the arrays of the last prune() again
  IndexedMesh pruned() { return fetch(ekf_components_get_pruned, pruned_vertices_, pruned_triangles_, weld_normals_); }
  // HIP-event milliseconds and launch counts of k_comp_init, k_comp_union, k_comp_count, k_comp_largest, k_comp_flags, the
  // prune's k_tsdf_scan, k_comp_vertices, k_comp_faces
  void getComponentProfile(double kernel_ms[8], long long launches[8]) {
    check(ekf_components_get_profile(f_, kernel_ms, launches));
  }
  // The last weld() (pruned = false) or the last prune() smoothed on the device with Taubin's scheme (section 26): `iterations`
  // times a step towards the mean of a vertex's neighbours with factor lambda and then, unless mu is 0, one with mu (Taubin
  // wants mu < -lambda; mu = 0 is plain Laplacian smoothing).  pin_boundary keeps the bits of the vertices on an open edge.
  // normals: unit vertex normals from the smoothed triangles, weighted by area; without it the result has none.  faces, grey,
  // colour and key are the source's; the source stays as it was.
  IndexedMesh smooth(int iterations = 10, double lambda = 0.5, double mu = -0.53, bool pin_boundary = false, bool normals = false,
                     bool pruned = false) {
    check(ekf_smooth_run(f_, pruned ? 1 : 0, iterations, lambda, mu, pin_boundary ? 1 : 0, normals ? 1 : 0, &smooth_vertices_,
                         &smooth_triangles_));
    smooth_normals_ = normals;
    return smoothed();
  }
  // the arrays of the last smooth() again
  IndexedMesh smoothed() { return fetch(ekf_smooth_get, smooth_vertices_, smooth_triangles_, smooth_normals_); }
  // the adjacency of the mesh the last smooth() ran on
  Adjacency adjacency() {
    Adjacency a;
    const size_t nv = (size_t)smooth_vertices_;
    a.inc.resize(nv); a.deg.resize(nv); a.boundary.resize(nv);
    check(ekf_smooth_get_adjacency(f_, a.inc.data(), a.deg.data(), a.boundary.data(), smooth_vertices_));
    return a;
  }
  // HIP-event milliseconds and launch counts of k_smooth_count, k_smooth_offsets, the adjacency's k_tsdf_scan, k_smooth_fill,
  // k_smooth_lists, k_smooth_step, k_smooth_normals
  void getSmoothProfile(double kernel_ms[7], long long launches[7]) { check(ekf_smooth_get_profile(f_, kernel_ms, launches)); }
  // The last weld() (source 0), the last prune() (1) or the last smooth() (2) simplified on the device by vertex clustering
  // (section 28): the vertices that fall into one cell of side `cell` (>= the voxel) of a grid from the volume's origin become
  // one vertex, their mean, with the cell's id as its key; a triangle whose vertices share a cell goes, and so does one whose
  // three cells an earlier triangle has; a cell that no kept triangle has gives no vertex.  Normals iff the source has them.
  // The source stays as it was.  stats (optional): the numbers of degenerate and duplicate triangles.
  IndexedMesh simplify(double cell, int source = 0, SimplifyStats* stats = nullptr) {
    SimplifyStats st;
    check(ekf_simplify_run(f_, source, cell, &simplify_vertices_, &simplify_triangles_, &st.degenerate, &st.duplicate));
    simplify_cell_ = cell;
    simplify_normals_ = source == 2 ? smooth_normals_ : weld_normals_;
    simplify_source_vertices_ = source == 2 ? smooth_vertices_ : (source == 1 ? pruned_vertices_ : weld_vertices_);
    if (stats) *stats = st;
    return simplified();
  }
  // the arrays of the last simplify() again
  IndexedMesh simplified() { return fetch(ekf_simplify_get, simplify_vertices_, simplify_triangles_, simplify_normals_); }
  // for every vertex of the source of the last simplify(), the number of its vertex in the result, or 0xffffffff
  std::vector<unsigned int> simplifyMap() {
    std::vector<unsigned int> map((size_t)simplify_source_vertices_);
    check(ekf_simplify_get_map(f_, map.data(), simplify_source_vertices_));
    return map;
  }
  // HIP-event milliseconds and launch counts of k_simp_cells, k_simp_count, k_simp_offsets, the simplification's k_tsdf_scan,
  // k_simp_fill, k_simp_lists, k_simp_flags, k_simp_vertices, k_simp_faces, k_simp_map
  void getSimplifyProfile(double kernel_ms[10], long long launches[10]) { check(ekf_simplify_get_profile(f_, kernel_ms, launches)); }
  // Starts a texture atlas (section 29) of the last weld() (source 0), prune() (1), smooth() (2) or simplify() (3): every pair of
  // triangles gets a block of patch + 2 texels a side (patch 2..32); channels 1 or 3 (0: 3 for a colour volume, else 1).  Returns
  // the atlas's side.  The source is only read.
  int textureBegin(int source = 0, int patch = 8, int channels = 0) {
    const int c = channels ? channels : (colour_ ? 3 : 1);
    int side = 0;
    check(ekf_texture_begin(f_, source, patch, c, &side));
    texture_side_ = side;
    texture_channels_ = c;
    texture_source_ = source;
    texture_triangles_ = source == 3 ? simplify_triangles_ : (source == 2 ? smooth_triangles_ : (source == 1 ? pruned_triangles_ : weld_triangles_));
    return side;
  }
  // The image, K and pose of a set slot of a dense handle as the next view, straight from its device buffers; returns the
  // triangles it won.  occlusion (optional): the volume is ray-cast at the slot's pose first (raycastView with that range), and a
  // vertex counts as seen only if it lies no more than tol behind that render; tol < 0: the voxel, and for a simplified source
  // its cell.  min_area2: twice the least area in pixels a triangle must have.
  unsigned long long textureAddView(DenseStereoHip& dense, int slot, const Occlusion* occlusion = nullptr, double tol = -1.0,
                                    double min_area2 = 0.0) {
    if (occlusion)
      check(ekf_raycast_render_view(f_, dense.handle(), slot, occlusion->z_near, occlusion->z_far,
                                    occlusion->step > 0.0 ? occlusion->step : voxel_ / 2.0, occlusion->min_count));
    unsigned long long n = 0;
    check(ekf_texture_add_view(f_, dense.handle(), slot, occlusion ? 1 : 0, textureTol(tol), min_area2, &n));
    return n;
  }
  // the same for an image from the host: height rows of channels x width bytes (1: grey, 3: B G R), `pitch` bytes apart (0: tight);
  // occlusion: the volume is ray-cast with that size, K and pose first (raycast with that range)
  unsigned long long textureAddViewHost(const unsigned char* img, int channels, int width, int height, const double K[4],
                                        const double pose7[7], const Occlusion* occlusion = nullptr, double tol = -1.0,
                                        double min_area2 = 0.0, int pitch = 0) {
    if (occlusion)
      check(ekf_raycast_render(f_, width, height, K, pose7, occlusion->z_near, occlusion->z_far,
                               occlusion->step > 0.0 ? occlusion->step : voxel_ / 2.0, occlusion->min_count));
    unsigned long long n = 0;
    check(ekf_texture_add_view_host(f_, img, pitch ? pitch : channels * width, channels, width, height, K, pose7, occlusion ? 1 : 0,
                                    textureTol(tol), min_area2, &n));
    return n;
  }
  // fills the triangles no view won with the blend of their vertices' grey (or B, G, R) and returns the atlas
  TextureAtlas textureFinish() {
    unsigned long long n = 0;
    check(ekf_texture_finish(f_, &n));
    TextureAtlas t = texture();
    t.n_textured = n;
    return t;
  }
  // the atlas as it is now, any time after textureBegin() (n_textured: the triangles with a view)
  TextureAtlas texture() {
    TextureAtlas t;
    t.side = texture_side_;
    t.channels = texture_channels_;
    const size_t nt = (size_t)texture_triangles_;
    t.atlas.resize((size_t)t.side * (size_t)t.side * (size_t)t.channels);
    t.uv.resize(nt * 6); t.view.resize(nt); t.score.resize(nt);
    check(ekf_texture_get(f_, t.atlas.data(), t.side * t.channels, t.uv.data(), t.view.data(), t.score.data(), texture_triangles_));
    for (size_t i = 0; i < nt; ++i) t.n_textured += t.view[i] >= 0 ? 1 : 0;
    return t;
  }
  // HIP-event milliseconds and launch counts of k_tex_project, k_tex_select, k_tex_fill, k_tex_fallback
  void getTextureProfile(double kernel_ms[4], long long launches[4]) { check(ekf_texture_get_profile(f_, kernel_ms, launches)); }
  // Gives the rasteriser a mesh of the caller's (source 4, section 30): xyz 3 per vertex, faces 3 per triangle, grey 1 per vertex,
  // colour 3 per vertex (B G R) or empty.  It is copied to buffers of the rasteriser's own.
  void setRasterMesh(const std::vector<double>& xyz, const std::vector<unsigned int>& faces, const std::vector<unsigned char>& grey,
                     const std::vector<unsigned char>& colour = std::vector<unsigned char>()) {
    check(ekf_raster_set_mesh(f_, xyz.data(), faces.data(), grey.data(), colour.empty() ? nullptr : colour.data(), xyz.size() / 3,
                              faces.size() / 3));
    raster_mesh_colour_ = !colour.empty();
  }
  // The last weld() (source 0), prune() (1), smooth() (2), simplify() (3) or the mesh of setRasterMesh() (4) seen by a width x
  // height pinhole camera K = (fx, fy, cx, cy) at pose7 (section 30): the nearest triangle of every pixel, its depth, barycentrics,
  // normal and colour.  A triangle with a vertex at or in front of z_near is dropped whole; cull drops the triangles seen from
  // behind; shading 0 blends the vertex colours, 1 samples the finished texture of that source; cover also counts the triangles
  // that cover every pixel.  The source is only read.
  MeshRender rasterise(int width, int height, const double K[4], const double pose7[7], int source = 0, double z_near = 0.0,
                       bool cull = true, int shading = 0, bool cover = false) {
    check(ekf_raster_render(f_, source, width, height, K, pose7, z_near, cull ? 1 : 0, shading, cover ? 1 : 0));
    return rastered(source, shading, cover);
  }
  // the same with the size, K and pose of a set slot of a dense handle
  MeshRender rasteriseView(DenseStereoHip& dense, int slot, int source = 0, double z_near = 0.0, bool cull = true, int shading = 0,
                           bool cover = false) {
    check(ekf_raster_render_view(f_, source, dense.handle(), slot, z_near, cull ? 1 : 0, shading, cover ? 1 : 0));
    return rastered(source, shading, cover);
  }
  // the images of the last rasterise(), given what it was asked for
  MeshRender rastered(int source = 0, int shading = 0, bool cover = false) {
    MeshRender r;
    check(ekf_raster_get(f_, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &r.width, &r.height));
    const size_t n = (size_t)r.width * (size_t)r.height;
    const bool colour = shading ? texture_channels_ == 3 : (source == 4 ? raster_mesh_colour_ : colour_);
    r.depth.resize(n); r.normal.resize(n * 3); r.grey.resize(n); r.tri.resize(n); r.bary.resize(n * 2);
    if (colour) r.colour.resize(n * 3);
    if (cover) r.cover.resize(n);
    check(ekf_raster_get(f_, r.depth.data(), r.normal.data(), r.grey.data(), colour ? r.colour.data() : nullptr, r.tri.data(),
                         r.bary.data(), cover ? r.cover.data() : nullptr, nullptr, nullptr));
    return r;
  }
  // a triangle whose box on the image has at most `limit` pixels (0..65536) is walked by one lane, a larger one by a workgroup
  void setRasterSmallLimit(int limit) { check(ekf_raster_set_small_limit(f_, limit)); }
  // HIP-event milliseconds and launch counts of k_rast_project, k_rast_small, k_rast_large, k_rast_resolve
  void getRasterProfile(double kernel_ms[4], long long launches[4]) { check(ekf_raster_get_profile(f_, kernel_ms, launches)); }
  // Gives the distance a mesh of the caller's (source 4, section 31), for instance a ground truth: xyz 3 per vertex, faces 3 per
  // triangle.  It is copied to buffers of the distance's own and is independent of setRasterMesh().
  void setDistanceMesh(const std::vector<double>& xyz, const std::vector<unsigned int>& faces) {
    check(ekf_distance_set_mesh(f_, xyz.data(), faces.data(), xyz.size() / 3, faces.size() / 3));
  }
  // For every vertex of source `query` the nearest point on source `target` (section 31): the last weld() (0), prune() (1),
  // smooth() (2), simplify() (3) or the mesh of setDistanceMesh() (4); they may be the same.  Both are only read.
  MeshDistance distance(int target = 0, int query = 3) {
    unsigned long long n = 0;
    check(ekf_distance_run(f_, target, query, &n));
    return distanced((size_t)n);
  }
  // the same for points of the caller's, 3 doubles each, at least one
  MeshDistance distancePoints(int target, const std::vector<double>& xyz) {
    check(ekf_distance_run_points(f_, target, xyz.data(), xyz.size() / 3));
    return distanced(xyz.size() / 3);
  }
  // the arrays of the last distance() or distancePoints(), which had n points
  MeshDistance distanced(size_t n) {
    MeshDistance r;
    r.dist.resize(n); r.tri.resize(n); r.closest.resize(n * 3); r.side.resize(n);
    check(ekf_distance_get(f_, r.dist.data(), r.tri.data(), r.closest.data(), r.side.data(), n));
    return r;
  }
  // the last run summed up: the maximum and where, the mean, the RMS and the points with dist <= threshold (>= 0)
  DistanceStats distanceStats(double threshold = 0.0) {
    DistanceStats s;
    check(ekf_distance_get_stats(f_, threshold, &s.n, &s.n_bad, &s.max, &s.argmax, &s.mean, &s.rms, &s.within));
    return s;
  }
  // the cells of the search grid along the longest axis of the target's box: 1..128, 0 = automatic; the result does not depend on it
  void setDistanceGrid(int g) { check(ekf_distance_set_grid(f_, g)); }
  // HIP-event milliseconds and launch counts of k_dist_box, k_dist_grid, k_dist_count, k_dist_offsets, k_tsdf_scan, k_dist_fill,
  // k_dist_query, k_dist_stats, k_dist_reduce
  void getDistanceProfile(double kernel_ms[9], long long launches[9]) { check(ekf_distance_get_profile(f_, kernel_ms, launches)); }
  // The volume seen by a width x height pinhole camera K = (fx, fy, cx, cy) at pose7: samples of the camera-z depth at
  // z_near + n step up to z_far over the voxels with at least min_count maps.  The mesh of the last extract stays valid.
  Render raycast(int width, int height, const double K[4], const double pose7[7], double z_near, double z_far, double step,
                 int min_count = 1) {
    check(ekf_raycast_render(f_, width, height, K, pose7, z_near, z_far, step, min_count));
    return render();
  }
  // the same with the size, K and pose of a set slot of a dense handle
  Render raycastView(DenseStereoHip& dense, int slot, double z_near, double z_far, double step, int min_count = 1) {
    check(ekf_raycast_render_view(f_, dense.handle(), slot, z_near, z_far, step, min_count));
    return render();
  }
  // HIP-event milliseconds and launch counts of k_tsdf_mean, k_tsdf_raycast (switched by profile())
  void getRaycastProfile(double kernel_ms[2], long long launches[2]) { check(ekf_raycast_get_profile(f_, kernel_ms, launches)); }
  void profile(bool enable) { check(ekf_fusion_profile(f_, enable ? 1 : 0)); }
  // HIP-event milliseconds and launch counts of k_tsdf_integrate, k_tsdf_count, k_tsdf_scan, k_tsdf_emit
  void getProfile(double kernel_ms[4], long long launches[4]) { check(ekf_fusion_get_profile(f_, kernel_ms, launches)); }
  // ... and of k_tsdf_integrate_colour, k_tsdf_colour_vertices, k_tsdf_raycast_colour
  void getColourProfile(double kernel_ms[3], long long launches[3]) { check(ekf_colour_get_profile(f_, kernel_ms, launches)); }
  ekf_fusion* handle() { return f_; }

 private:
  void check(int rc) { if (rc != EKF_OK) throw std::runtime_error(ekf_fusion_last_error(f_)); }
  Render render() {
    Render r;
    check(ekf_raycast_get(f_, nullptr, nullptr, nullptr, &r.width, &r.height));
    const size_t n = (size_t)r.width * (size_t)r.height;
    r.depth.resize(n); r.normal.resize(n * 3); r.grey.resize(n);
    check(ekf_raycast_get(f_, r.depth.data(), r.normal.data(), r.grey.data(), nullptr, nullptr));
    if (colour_) {
      r.colour.resize(n * 3);
      check(ekf_colour_get_render(f_, r.colour.data()));
    }
    return r;
  }
  // the arrays of a mesh of n_vert vertices and n_tri triangles on the device, by ekf_mesh_get or one of its three siblings
  using MeshGetter = int (*)(ekf_fusion*, double*, unsigned int*, unsigned char*, unsigned char*, float*, unsigned long long*,
                             unsigned long long, unsigned long long);
  IndexedMesh fetch(MeshGetter getter, unsigned long long n_vert, unsigned long long n_tri, bool normals) {
    IndexedMesh m;
    const size_t nv = (size_t)n_vert, nt = (size_t)n_tri;
    m.xyz.resize(nv * 3); m.faces.resize(nt * 3); m.grey.resize(nv); m.key.resize(nv);
    if (colour_) m.colour.resize(nv * 3);
    if (normals) m.normal.resize(nv * 3);
    check(getter(f_, m.xyz.data(), m.faces.data(), m.grey.data(), colour_ ? m.colour.data() : nullptr,
                 normals ? m.normal.data() : nullptr, m.key.data(), n_vert, n_tri));
    return m;
  }
  // the default of tol: the voxel, and for a simplified source the cell of that run
  double textureTol(double tol) const { return tol >= 0.0 ? tol : (texture_source_ == 3 ? simplify_cell_ : voxel_); }
  size_t n_;
  bool colour_;
  double voxel_, simplify_cell_ = 0.0;
  unsigned long long weld_vertices_ = 0, weld_triangles_ = 0;
  unsigned long long pruned_vertices_ = 0, pruned_triangles_ = 0;
  unsigned long long smooth_vertices_ = 0, smooth_triangles_ = 0;
  unsigned long long simplify_vertices_ = 0, simplify_triangles_ = 0, simplify_source_vertices_ = 0;
  unsigned long long texture_triangles_ = 0;
  int texture_side_ = 0, texture_channels_ = 0, texture_source_ = 0;
  bool weld_normals_ = false, smooth_normals_ = false, simplify_normals_ = false;
  bool raster_mesh_colour_ = false;
  ekf_fusion* f_ = nullptr;
};
