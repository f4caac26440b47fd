// Host side of libekfslam_hip.so: the filter object (device buffers, feature table, launch
// sequences) and the C ABI declared in include/ekf_monoslam.h.  gfx950 only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/ekf_monoslam.h"
#include "ekf_buffers.hpp"
#include "ekf_feature_table.hpp"
#include "ekf_dense.hpp"
#include "ekf_image.hpp"
#include "ekf_features.hpp"
#include "ekf_syrk6.hpp"
#include "ekf_chain.hpp"
#include "ekf_small.hpp"
#include "ekf_step.hpp"
#include "ekf_kernels.hpp"
#include "ekf_shard.hpp"
#include "ekf_sba.hpp"
#include "ekf_rectify.hpp"
#include "ekf_keyframe.hpp"
#include "ekf_dense_stereo.hpp"
#include "ekf_dense_sgm.hpp"
#include "ekf_dense_speckle.hpp"
#include "ekf_fusion.hpp"
#include "ekf_raycast.hpp"
#include "ekf_mesh.hpp"
#include "ekf_mesh_components.hpp"
#include "ekf_mesh_smooth.hpp"
#include "ekf_mesh_simplify.hpp"
#include "ekf_mesh_texture.hpp"
#include "ekf_mesh_raster.hpp"
#include "ekf_mesh_distance.hpp"

namespace ekf {

static thread_local std::string g_create_error;

enum KernelId : int {
  KID_PREDICT_CAMERA = 0,
  KID_PROPAGATE_STRIPS,
  KID_PROPAGATE_STREAMING,
  KID_MEASURE,
  KID_INNOVATION,
  KID_SIGMA_HT,
  KID_INNOVATION_COV,
  KID_CHOL_DIAG,
  KID_CHOL_PANEL,
  KID_CHOL_TRAILING,
  KID_STATE_UPDATE,
  KID_DOWNDATE,
  KID_SOLVE,
  KID_NORMALIZE,
  KID_ADD_FEATURE,
  KID_COMPACT,
  KID_MISC,
  KID_WUPDATE,
  KID_GATHER_H,
  KID_GATHER_S,
  KID_GATHER_V,
  KID_GATHER_SIGMA,
  KID_SEED_MASK,
  KID_SEED_RESPONSE,
  KID_SEED_CANDIDATES,
  KID_SEED_SELECT,
  KID_FRAME_UPLOAD,
  KID_FRAME_INGEST,
  KID_FRAME_RECTIFY,
  KID_COUNT
};

static const char* kKernelNames[KID_COUNT] = {
    "predict_camera",  "propagate_strips", "propagate_streaming", "measure",
    "innovation",      "sigma_ht",         "innovation_cov",      "chol_diag",
    "chol_panel",      "chol_trailing",    "state_update",        "downdate_syrk",
    "solve_trmm",      "normalize_quat",  "add_feature",      "compact_transform",   "misc",
    "w_update", "allgather_h", "allgather_s", "allgather_v", "allgather_sigma",
    "seed_mask", "seed_response", "seed_candidates", "seed_select", "frame_upload", "frame_ingest", "frame_rectify"};

// Which launch structure an update actually took (ekf_launch_count): host-side counters, always on, one increment per
// launch.  The order is the ABI's `enum ekf_launch_kind`.
static const char* kLaunchNames[EKF_LAUNCH_KINDS] = {
    "downdate_bf16x6", "downdate_f32", "downdate_f32_fused_wu", "downdate_f32_half_tail", "downdate_f32_t64",
    "row_rider", "row_gemv", "row_tile_gemm", "w_update_gemm", "w_recompute",
    "chain_step_launches", "chain_persistent", "solve", "solve_two_groups", "update_oneblock", "update_allinone",
    "chain_trail_diag", "split_image", "state_update_tail", "update_onelaunch", "chain_dist_gather", "chain_step_fused",
    "downdate_mirror_bounds", "solve_poll_chain"};

static inline int round_up(int v, int a) { return (v + a - 1) / a * a; }

// CU-masked streams are never destroyed: hipStreamDestroy of a stream made by hipExtStreamCreateWithCUMask stalls for good about
// once in a few hundred calls on this runtime (ROCm 7.2; tools/lifecycle_soak.py, DESIGN.md 8: the cause of the two test hangs of
// round 6).  A filter that goes away hands its stream back -- idle: its work was synchronised -- and the next filter of the same
// device and mask takes it over.  What is left in the pool at process exit is destroyed by an atexit handler registered on first
// use -- i.e. behind the runtime's own initialisation, so it runs in front of the runtime's (and a profiler's) tear-down: a masked
// stream still alive at that point crashes rocprofv3's exit (SIGSEGV in __cxa_finalize); one destroy per process and mask, on an
// idle device, instead of one per filter.
struct MaskedStreamPool {
  struct Entry { int device, num_cus, reserved; hipStream_t st; };
  std::mutex mu;
  std::vector<Entry> idle;
  bool hooked = false;
  static void at_exit();
  hipStream_t take(int device, int num_cus, int reserved) {
    std::lock_guard<std::mutex> lk(mu);
    for (size_t i = 0; i < idle.size(); ++i)
      if (idle[i].device == device && idle[i].num_cus == num_cus && idle[i].reserved == reserved) {
        hipStream_t st = idle[i].st;
        idle.erase(idle.begin() + i);
        return st;
      }
    return nullptr;
  }
  void give(int device, int num_cus, int reserved, hipStream_t st) {
    std::lock_guard<std::mutex> lk(mu);
    idle.push_back({device, num_cus, reserved, st});
    if (!hooked) { hooked = true; atexit(&MaskedStreamPool::at_exit); }
  }
};
static MaskedStreamPool g_masked_streams;
void MaskedStreamPool::at_exit() {
  std::lock_guard<std::mutex> lk(g_masked_streams.mu);
  for (const Entry& e : g_masked_streams.idle) {
    if (hipSetDevice(e.device) != hipSuccess) continue;
    (void)hipStreamSynchronize(e.st);
    (void)hipStreamDestroy(e.st);
  }
  g_masked_streams.idle.clear();
}

struct FilterBase {
  std::string err;
  bool diag_synced = false;   // sharded filter: the owners' diagonal blocks were gathered and nothing changed Sigma or the layout since (shard_sync_diag_blocks)
  virtual ~FilterBase() {}
  virtual int set_dt(double) = 0;
  virtual double get_dt() const = 0;
  virtual int set_stream(void*) = 0;
  virtual int set_option(int, int) = 0;
  virtual int synchronize() = 0;
  virtual int add_feature(double, double) = 0;
  virtual int remove_features(const int*, int) = 0;
  virtual int predict(const void*, const void*, int) = 0;
  virtual int measure() = 0;
  virtual int motion_jacobian(void*, void*) = 0;
  virtual int get_predictions(void*, unsigned char*, unsigned char*, void*, void*, void*) = 0;
  virtual int update(const void*, const int*, int, int, bool) = 0;
  virtual int innovation_covariance(const int*, int, int, void*) = 0;
  virtual int get_gain(void*) = 0;
  virtual int last_rows() const = 0;
  virtual int convert(int index, bool all) = 0;
  virtual int num_features() const = 0;
  virtual int state_dim() const = 0;
  virtual int get_layout(int*, int*) const = 0;
  virtual int get_state(void*, int, int) = 0;
  virtual int set_state(const void*, int, int) = 0;
  virtual int get_sigma(void*, int, int, int, int) = 0;
  virtual int peek_work(int, void*, int, int, int, int) = 0;
  virtual int set_sigma(const void*, int, int, int, int) = 0;
  virtual int covariance_parameter(double*) = 0;
  virtual int check_invariants(double*, double*, double*) = 0;
  virtual int feature_xyz(int, void*, void*) = 0;
  virtual int profile_read(int, double*, long long*) = 0;
  virtual int profile_reset() = 0;
  virtual int profile_work(int, double*) = 0;
  virtual int chunk_plan(int*, int, int*, int*) = 0;
  long long launch_cnt[EKF_LAUNCH_KINDS] = {};           // ekf_launch_count: since ekf_create / ekf_profile_reset
  virtual void* dev_mu() = 0;
  virtual void* dev_sigma(int*) = 0;
  virtual int export_points(void*, int) = 0;
  virtual int export_points_table(void*, int, int*) = 0;
  virtual int feature_ids(int*, int*) const = 0;
  virtual int set_feature_meta(int, int, int) = 0;
  virtual int num_archived() const = 0;
  virtual int rescue(const void*, const void*, const int*, int, double, unsigned char*) = 0;
  virtual int search_ellipses(int, int*) = 0;
  virtual int ransac(const void*, const int*, int, double, int*, unsigned char*, int*) = 0;
  virtual int update_two_stage(const void*, const int*, int, int, unsigned int, double, double, unsigned char*,
                               unsigned char*, int*) = 0;
  virtual int set_frame(const unsigned char*, int, int, int) = 0;
  virtual int set_frame_raw(const void*, int, int, int, int, bool) = 0;
  virtual int get_frame(unsigned char*, int) = 0;
  virtual int set_patch(int, const unsigned char*) = 0;
  virtual int get_patch(int, int, unsigned char*) = 0;
  virtual int blur_predictions(void*) = 0;
  virtual int find_matches(double, void*, unsigned char*, float*) = 0;
  virtual int get_track(int*, unsigned char*, float*, unsigned char*) = 0;
  virtual int set_track(int, int, int, const float*, int) = 0;
  virtual int find_new_features(int, double, double, int, float*, int*) = 0;
  virtual int end_update(float, int, int*, int*, int*, int*) = 0;
  virtual int shard_configure(int, int, ekf_allgather_fn, void*) = 0;
  virtual int shard_info(ekf_shard_info*) = 0;
  virtual int shard_update(const void*, const int*, int, int) = 0;
  virtual int shard_rebalance() = 0;
  virtual int kf_create(KfSelector*) = 0;
  virtual int kf_observe(KfSelector*, int, KfRecord*) = 0;
  virtual int rectified_camera(int, ekf_sba_camera*) = 0;
  virtual int get_frame_rectified(int, unsigned char*, int) = 0;
  virtual int undistort_pixels(int, const double*, int, double*) = 0;
};

#define HIPCHK(expr)                                                                         \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess) {                                                                  \
      char _b[512];                                                                          \
      snprintf(_b, sizeof(_b), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
               __LINE__);                                                                    \
      err = _b;                                                                              \
      return EKF_ERR_DEVICE;                                                                 \
    }                                                                                        \
  } while (0)

#define FAIL(code, msg) \
  do {                  \
    err = (msg);        \
    return (code);      \
  } while (0)

template <typename T>
struct Filter : FilterBase {
  ekf_config cfg;
  CamParams cam;
  int camera_dim = 14;
  int capN = 0, cap_n = 0, n_pad = 0, ld = 0;
  int N = 0, n = 0;
  int device = 0;
  double dT = 1.0;                                     // vR.cpp:155
  double vmax[6];
  int sigma_pixel_2 = 4;
  // the host records of the features, one per feature (ekf_feature_table.hpp); N == ft.size() at all times.  Of a Patch's track
  // state, ekf_predict / ekf_measure fold their visibility / rho <= 0 flags into d_trk on the device (bit 0: visible at the
  // last one, bit 1: rho <= 0 since the last read-back); pull_track() folds that into the table before anything reads it
  // or reorders the features (d_trk is all zero whenever trk_dirty is false)
  FeatureTable ft;
  DevBuf<unsigned char> d_trk;
  bool trk_dirty = false;
  // corner seeding (ekf_features.hpp): mask, lambda, [max bits | candidate count], candidates, square origins, selection
  DevBuf<unsigned char> d_seed_mask;
  DevBuf<double> d_seed_lam;
  DevBuf<unsigned long long> d_seed_aux, d_seed_ckey;
  DevBuf<int> d_seed_cidx, d_seed_org, d_seed_out;
  bool have_seed_lam = false;
  // the patches archived at removal (vR.cpp:394-404): real_index on the host, XYZ + 3x3 covariance on the device
  std::vector<int> arch_real;
  DevBuf<T> d_archive;                                  // 12 scalars per archived patch
  DevBuf<int> d_arch_idx;
  bool layout_dirty = true;
  DevBuf<int> d_pos, d_coding;
  DevBuf<T> d_mu[2];
  int cur_mu = 0;
  DevBuf<T> d_S[2];
  int cur = 0;
  int extent[2] = {0, 0};                              // largest n ever written per Sigma buffer
  DevBuf<T> d_scr;
  DevBuf<T> d_h, d_Hc, d_Hf, d_Sd;
  DevBuf<unsigned char> d_flags, d_cflag;
  DevBuf<T> d_Jy, d_Yxyz;
  DevBuf<int> d_map_src, d_map_conv;
  // update workspace
  int m_cap = 0, ldy = 0, w_rows = 0;
  DevBuf<T> d_Y;                                        // [S; Z], 2 ldy rows
  DevBuf<T> d_W;                                        // [W; nu block], n_pad + 128 rows
  DevBuf<T> d_V;                                        // [V; y block]
  DevBuf<T> d_Dinv;
  DevBuf<T> d_z;
  DevBuf<int> d_midx;
  DevBuf<int> d_status;
  DevBuf<T> d_tmp;                                      // small D2H staging (>= 16 T)
  DevBuf<T> d_K;                                        // lazily allocated gain buffer
  int last_m = 0, last_m_pad = 0, last_n = 0;
  bool have_meas = false;
  bool have_sd = false;                                  // 2x2 St blocks of the current h/H evaluated?
  bool have_update = false;
  // options
  int opt_streaming = 0, opt_mfma = 1;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  hipStream_t stream_b = nullptr;                       // solve pieces / downdate pieces, overlapped with the chain
  hipEvent_t ev_chain[8] = {}, ev_solve[8] = {}, ev_b = nullptr, ev_wu = nullptr;
  hipStream_t stream_g = nullptr;                       // sharded step: the all-gathers of V_g, beside the rank's solves
  bool stream_b_masked = false;                         // stream_b carries a CU mask: handed back to the pool, never destroyed
  int stream_b_reserved = 0;                            // the mask it was made with (reserved_cus may be changed later)
  hipEvent_t ev_gath[8] = {}, ev_g = nullptr;
  int solve64_off = 0, solve6464_off = 0, tri64_off = 0, tri64_count = 0;
  int tri6_off = 0;                                      // the lower-triangular list, diagonal tiles first (k_syrk_bf16x6)
  int trih_off = 0, trih_count = 0;                      // the 128 x 128 list with its last opt_split_tail tiles as 64 x 128 halves
  // EKF_SPLIT_TAIL (-1: 1.5 tiles per CU, at most a third of the list): tiles at the end of the LAST downdate's queued list
  // that go out as 64 x 128 halves.  Measured at N = 1000: 384 halves 1.348 -> 1.329 ms (on the CU-masked side stream: no gain).
  int opt_split_tail = -1;
  double opt_feature_noise = 0.0;                       // EKF_OPT_FEATURE_NOISE: variance added to every feature state per predict
  int opt_split_bf16 = 1;                               // EKF_OPT_SPLIT_BF16 (default on, round 5): downdate of large maps on the bf16 matrix pipe, 3 x bf16 per operand, six products (ekf_syrk6.hpp)
  DevBuf<s6_u32x4> d_Vimg;                              // plane image of V: (n_pad + 128) / 128 row blocks x ldy / 16 records of 12 KB
  // (six bf16 planes of 2 bytes per element of V = 6 * ldy / 8 records of 16 bytes per row; allocated at the first bf16x6 downdate)
  hipError_t ensure_vimg() { return d_Vimg.reserve((size_t)(n_pad + 128) * ldy * 6 / sizeof(s6_u32x4)); }
  int last_nchunks = 1, last_cend[8] = {};
  // image side (8f4): current frame, templates (original / matching), blur-pose predictions, match results
  DevBuf<unsigned char> d_frame;
  int frame_w = 0, frame_h = 0;
  bool have_frame = false, have_blur = false;
  // the camera's own frame: W x H x C bytes, tight, + kIngestSlack; d_frame is derived from it on the device
  DevBuf<unsigned char> d_raw;
  int raw_w = 0, raw_h = 0, raw_c = 0;
  bool have_raw = false;
  RectScratch rect;                                     // on-demand rectification: never touched per frame
  DevBuf<int4> d_ingest_tab;                            // column records, then row records (ingest_tables)
  int ingest_tab_w = 0, ingest_tab_h = 0;               // the raw geometry the resident tables were computed for
  DevBuf<unsigned char> d_patch[2], d_mpatch[2];
  int cur_patch = 0;
  DevBuf<T> d_hb, d_zm;
  DevBuf<unsigned char> d_found;
  DevBuf<float> d_score;
  DevBuf<int> d_keep;
  int opt_panel_direct = 1;                             // EKF_PANEL_DIRECT=0: panel through the general tile GEMM
  // the trailing update of step j and the diagonal factor of step j + 1 as ONE launch (k_trail_diag, ekf_chain.hpp);
  // EKF_CHAIN_FUSED_DIAG=0: diag -> panel -> trailing, three launches per block step (rounds 1-5; A/B and bit-identity check)
  int opt_chain_fused_diag = 1;
  // the whole update of a small map (n_pad <= 256, one diagonal block) as ONE launch (k_update_small_onelaunch, ekf_small.hpp);
  // EKF_SMALL_ONELAUNCH=0: W, S, the factor and the rest as four launches (rounds 3-5; A/B and bit-identity check)
  int opt_small_onelaunch = 1;
  // a block step of the chain (factor, panel, trailing update) as ONE launch where the step has fewer workgroups than the chip has
  // CUs and the chain runs alone (one column chunk: N up to ~230; k_chain_step_fused, ekf_step.hpp); EKF_STEP_FUSED=0: three launches
  int opt_step_fused = 1;
  struct StepPlan { std::vector<int> off, cnt; } sfp;   // per block step of the plan sf_lists was built for (sf_lists.first() steps)
  WorkList sf_lists{{0}, {}};                           // key (nblk); as the parent: a plan of no steps needs no list
  DevBuf<unsigned long long> d_small_stamps;            // EKF_SMALL_STAMPS=1: phase stamps of its workgroup 0 (ekf_peek_workspace, which = 3)
  unsigned small_gate_total = 0;                        // arrivals the gate word (d_status[9]) has seen when every launch so far is over
  int opt_su_tail = 1;                                  // EKF_SU_TAIL=0: k_state_update as its own launch on the second stream beside the last downdate (round 5)
  // EKF_SYRK_MIRROR_SKIP=0: every k_syrk_bf16x6 launch stores every mirror (rounds 5-6; A/B and bit-identity check).  1: launches
  // 0 .. G-2 of an update mirror only the tiles whose rows the re-evaluation of the next chunk reads as columns (Syrk6Args::mirror_rows)
  int opt_syrk_mirror_skip = 1;
  // EKF_SOLVE_POLL_CHAIN=0: every overlapped solve sits behind a stream wait for the chain's event (rounds 1-7; A/B and
  // bit-identity check).  1: the solves of chunks 1 .. G-2 are launched without it and wait for the chain in their prologue
  // (GemmArgs::chain_word; Filter::update), in plans of at most 16 block steps; 2: in every plan (solve_polls_chain)
  int opt_solve_poll_chain = 1;
  int opt_fuse_split = 1;                               // EKF_FUSE_SPLIT=0: the plane image of V_g by its own launch behind the solve (rounds 5)
  int opt_chain_defer = 1;                              // EKF_CHAIN_DEFER=0: a chunk's event behind the trailing update of its last step (rounds 1-5)
  int td_min_blocks = 24;                               // EKF_TD_MIN_BLOCKS: steps with fewer blocks in their update keep the three launches
  int td_max_blocks = 1 << 30;                          // EKF_TD_MAX_BLOCKS: ... and so do steps with more (many rounds of blocks: the 64 x 64 tile kernel's occupancy wins)
  WorkList td_blocks;                                   // key (nblk, nchunks, chunk ends)
  std::vector<int> td_off, td_cnt;                      // per block step: its list of (I, K) blocks inside td_blocks.d
  // EKF_SYRK_STAGGER="h,m": de-phasing of the bf16x6 downdate's workgroups (Syrk6Args).  Round 6, N = 1000, knob A/B: every
  // (0, m) with m = 1 .. 6 measures 0.897-0.903 ms per step against 0.917-0.922 without; a late second half (h > 0) gains nothing
  int opt_syrk_stag_half = 0, opt_syrk_stag_mod4 = 2;
  int opt_solve_s2 = 1;                                 // EKF_SOLVE_S2: latency-bound solve launches on two wave groups (halves of K)
  // A solve launch of under ~one round of tiles is bounded by the K steps of its heaviest tile: two wave groups per
  // workgroup then take half of K each (k_gemm_mfma<.., S2>).  The rule only looks at the chunk width and the size of the
  // WHOLE state (never at the rows one rank holds), so the plain and the sharded path sum every element in the same order.
  bool want_solve_s2(int width, int npad_live) const {
    return kIsF32 && opt_mfma && opt_solve_s2 && (opt_solve_s2 > 1 || (width / 128) * (npad_live / 64) <= 2 * num_cus);   // (2: always, for A/B runs)
  }
  int opt_fused = 1;                                    // EKF_OPT_FUSED_LAUNCHES: k_predict_fused, k_solve_state_oneblock, k_update_oneblock_small
  int opt_solve_one_per_cu = 1;                         // EKF_SOLVE_ONE_PER_CU: the last solve on one workgroup per CU when it has 1 .. 2 tiles per CU
  int opt_wrecompute = 1;                               // EKF_OPT_W_RECOMPUTE / EKF_W_RECOMPUTE: next chunk's W re-evaluated from the downdated Sigma
  int opt_row_gemv = 1;                                 // EKF_ROW_GEMV=0: the innovation-row update through the tile GEMM (A/B, bit-identity check)
  int opt_fuse_wu = 1;                                  // EKF_FUSE_WU: 0 never, 1 every overlapped chunk but the one before the last, 2 every overlapped chunk
  int env_chunks[8] = {}, env_nchunks = 0;               // EKF_CHUNKS="5,10,14,16": tuning knob (block steps)
  int opt_pipeline = -1;                                 // -1 auto: on when the chain has >= 8 block steps
  WorkList tilemap{{0, 0}, {}};                         // work lists: [lower-tri super-tiles | solve heavy-first], key (nt, ntc)
  int tri_count = 0, solve_off = 0;
  int w_zeroed_n = -1;                                   // n for which the pad rows of W were last cleared
  DevBuf<int> d_counters;                               // one work-queue head per queued launch of an update
  int num_cus = 256, reserved_cus = 32;
  // profiling
  LaunchProfiler<KID_COUNT> prof{KID_DOWNDATE, KID_PROPAGATE_STREAMING};   // mode: EKF_OPT_PROFILE; work[]: downdate only

  static constexpr bool kIsF32 = sizeof(T) == 4;
  int NB() const { return (kIsF32 && opt_mfma) ? 128 : 64; }

  // What is about ordering is spelled out here: the streams are drained, then events and streams go.  The device and pinned
  // buffers are members (DevBuf / PinnedBuf) and are released after this body, i.e. after the streams are gone -- sound, because
  // every stream that could touch them was synchronised first (the device set here stays current for those frees).
  ~Filter() override {
    const bool dbg = getenv("EKF_DEBUG_DTOR") != nullptr;       // (diagnostics: which call of the tear-down a stall sits in)
    auto mark = [&](const char* what) { if (dbg) { fprintf(stderr, "[ekf dtor %p] %s\n", (void*)this, what); fflush(stderr); } };
    hipSetDevice(device);
    mark("sync main stream");
    if (stream) hipStreamSynchronize(stream);
    mark("sync side streams");
    if (stream_b) hipStreamSynchronize(stream_b);
    if (stream_g) hipStreamSynchronize(stream_g);
    mark("events");
    prof.release();                            // the pending pairs, the pool,
    in_ring.release();                         // ... the slots' events: here, so that the members' destructors find nothing left
    mark("streams");
    if (own_stream && stream) hipStreamDestroy(stream);
    mark("stream b");
    const char* pool_env = getenv("EKF_MASKED_STREAM_POOL");        // =0: destroy it, as rounds 1-5 did (A/B; can stall, see the pool)
    if (stream_b && stream_b_masked && !(pool_env && atoi(pool_env) == 0)) g_masked_streams.give(device, num_cus, stream_b_reserved, stream_b);
    else if (stream_b) hipStreamDestroy(stream_b);
    mark("stream g");
    if (stream_g) hipStreamDestroy(stream_g);
    mark("last events");
    for (auto e : ev_gath) if (e) hipEventDestroy(e);
    if (ev_g) hipEventDestroy(ev_g);
    for (auto e : ev_chain) if (e) hipEventDestroy(e);
    for (auto e : ev_solve) if (e) hipEventDestroy(e);
    if (ev_b) hipEventDestroy(ev_b);
    if (ev_wu) hipEventDestroy(ev_wu);
    mark("done");
  }

  // ---- profiling helpers ---------------------------------------------------------------
  // a launch site's `Scope sc(this, KID_X[, stream])`: the profiler's scope on the filter's stream unless one is named
  struct Scope : LaunchProfiler<KID_COUNT>::Scope {
    Scope(Filter* f, int kid, hipStream_t st = nullptr) : LaunchProfiler<KID_COUNT>::Scope(f->prof, kid, st ? st : f->stream) {}
  };
  void resolve_profile() { prof.resolve(stream, stream_b, stream_g); }

  // ---- construction ---------------------------------------------------------------------
  int init(const ekf_config* c, int cdim, int capacity, int dev) {
    cfg = *c;
    camera_dim = cdim;
    device = dev;
    capN = capacity;
    cap_n = camera_dim + 6 * capN;
    n_pad = round_up(cap_n, 128);
    ld = n_pad;
    m_cap = 2 * capN + 3;
    ldy = round_up(m_cap, 128);
    w_rows = n_pad + 128;
    in_ring.configure(sizeof(T), (size_t)capN);
    cam.fx = c->fx; cam.fy = c->fy; cam.u0 = c->u0; cam.v0 = c->v0;
    cam.k1 = c->k1; cam.k2 = c->k2; cam.k3 = c->k3; cam.p1 = c->p1; cam.p2 = c->p2;
    cam.width = c->image_width; cam.height = c->image_height; cam.half_window = c->window_size / 2;
    sigma_pixel_2 = c->sigma_pixel * c->sigma_pixel;               // ints, vR.cpp:150-151
    const float sv[6] = {c->sigma_vx, c->sigma_vy, c->sigma_vz, c->sigma_wx, c->sigma_wy, c->sigma_wz};
    for (int i = 0; i < 6; ++i) vmax[i] = double(T(sv[i]) * T(sv[i]));  // vR.cpp:194-200
    HIPCHK(hipSetDevice(device));
    {
      int lo = 0, hi = 0;
      HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
      HIPCHK(hipStreamCreateWithPriority(&stream, hipStreamNonBlocking, hi));   // the serial chain goes first
    }
    own_stream = true;
    for (auto& e : ev_chain) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (auto& e : ev_solve) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&ev_b, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&ev_wu, hipEventDisableTiming));
    const size_t sig = (size_t)n_pad * ld;
    HIPCHK(d_S[0].reserve(sig));
    HIPCHK(d_S[1].reserve(sig));
    HIPCHK(hipMemsetAsync(d_S[0], 0, sig * sizeof(T), stream));
    HIPCHK(hipMemsetAsync(d_S[1], 0, sig * sizeof(T), stream));
    HIPCHK(d_mu[0].reserve((size_t)n_pad));
    HIPCHK(d_mu[1].reserve((size_t)n_pad));
    HIPCHK(hipMemsetAsync(d_mu[0], 0, (size_t)n_pad * sizeof(T), stream));
    HIPCHK(hipMemsetAsync(d_mu[1], 0, (size_t)n_pad * sizeof(T), stream));
    HIPCHK(d_scr.reserve(SCR_SIZE));
    const size_t cn = (size_t)std::max(capN, 1);
    HIPCHK(d_pos.reserve(cn));
    HIPCHK(d_coding.reserve(cn));
    HIPCHK(d_h.reserve(cn * 2));
    HIPCHK(d_Hc.reserve(cn * 14));
    HIPCHK(d_Hf.reserve(cn * 12));
    HIPCHK(d_Sd.reserve(cn * 4));
    HIPCHK(d_flags.reserve(cn));
    HIPCHK(d_cflag.reserve(cn));
    HIPCHK(d_trk.reserve(cn));
    HIPCHK(hipMemsetAsync(d_trk, 0, cn, stream));
    HIPCHK(d_Jy.reserve(cn * 18));
    HIPCHK(d_Yxyz.reserve(cn * 3));
    HIPCHK(d_map_src.reserve((size_t)n_pad));
    HIPCHK(d_map_conv.reserve((size_t)n_pad));
    HIPCHK(d_Y.reserve((size_t)2 * ldy * ldy));
    HIPCHK(hipMemsetAsync(d_Y, 0, (size_t)2 * ldy * ldy * sizeof(T), stream));
    HIPCHK(d_W.reserve((size_t)w_rows * ldy));
    HIPCHK(hipMemsetAsync(d_W, 0, (size_t)w_rows * ldy * sizeof(T), stream));
    HIPCHK(d_V.reserve((size_t)w_rows * ldy));
    HIPCHK(hipMemsetAsync(d_V, 0, (size_t)w_rows * ldy * sizeof(T), stream));
    HIPCHK(d_Dinv.reserve((size_t)(ldy / 64) * 128 * 128));
    HIPCHK(d_z.reserve((size_t)ldy));
    HIPCHK(d_midx.reserve(cn));
    HIPCHK(d_status.reserve(16));         // [0] pivot <= 0, [1] bad device index list, [3] a bounded device-side wait gave up; [4..7] scratch of ekf_check_invariants; [8] arrival gate of k_predict_fused, [9] of k_update_small_onelaunch
    HIPCHK(hipMemsetAsync(d_status, 0, 16 * sizeof(int), stream));
    HIPCHK(d_tmp.reserve(64));
    // (behind the queue heads: the row bounds of the mirror rule, written by the first launch of every update)
    HIPCHK(d_counters.reserve(kResetInts + kMirrorRowsInts));
    HIPCHK(hipMemset(d_counters, 0, (kResetInts + kMirrorRowsInts) * sizeof(int)));
    {
      hipDeviceProp_t prop;
      HIPCHK(hipGetDeviceProperties(&prop, device));
      num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    {
      // second stream for the pipelined solve / downdate pieces: kept off `reserved_cus` CUs so that
      // the serial chain on the main stream always finds a free CU (a chain workgroup sharing its SIMDs
      // with MFMA-saturating tile-GEMM waves runs ~4x slower: tools/coresidency.hip)
      reserved_cus = std::min(32, num_cus / 4);
      if (const char* e = getenv("EKF_RESERVED_CUS")) reserved_cus = std::max(1, std::min(num_cus / 2, atoi(e)));   // tuning knob
      std::vector<uint32_t> mask((num_cus + 31) / 32, 0xffffffffu);
      for (int i = 0; i < reserved_cus; ++i) mask[i / 32] &= ~(1u << (i % 32));
      // (a runtime that refuses CU masks still gets a second stream: the overlap works, only less well)
      stream_b = g_masked_streams.take(device, num_cus, reserved_cus);      // (a masked stream is reused, never destroyed: see the pool)
      stream_b_masked = stream_b != nullptr;
      if (!stream_b) {
        if (hipExtStreamCreateWithCUMask(&stream_b, (uint32_t)mask.size(), mask.data()) == hipSuccess) {
          stream_b_masked = true;
        } else {
          (void)hipGetLastError();
          stream_b = nullptr;
          reserved_cus = 0;
          HIPCHK(hipStreamCreateWithFlags(&stream_b, hipStreamNonBlocking));
        }
      }
      stream_b_reserved = reserved_cus;

      if (const char* e = getenv("EKF_FUSE_WU")) opt_fuse_wu = atoi(e);
      if (const char* e = getenv("EKF_ROW_GEMV")) opt_row_gemv = atoi(e) ? 1 : 0;
      if (const char* e = getenv("EKF_SOLVE_ONE_PER_CU")) opt_solve_one_per_cu = atoi(e) ? 1 : 0;
      if (const char* e = getenv("EKF_W_RECOMPUTE")) opt_wrecompute = atoi(e) ? 1 : 0;   // = EKF_OPT_W_RECOMPUTE, for A/B runs
      if (const char* e = getenv("EKF_SOLVE_S2")) opt_solve_s2 = atoi(e);
      if (const char* e = getenv("EKF_FUSED_LAUNCHES")) opt_fused = atoi(e) ? 1 : 0;   // = EKF_OPT_FUSED_LAUNCHES, for A/B runs
      if (const char* e = getenv("EKF_PANEL_DIRECT")) opt_panel_direct = atoi(e);
      if (const char* e = getenv("EKF_SYRK_STAGGER")) {
        opt_syrk_stag_half = atoi(e);
        if (const char* c = strchr(e, ',')) opt_syrk_stag_mod4 = atoi(c + 1);
      }
      if (const char* e = getenv("EKF_CHAIN_FUSED_DIAG")) opt_chain_fused_diag = atoi(e) ? 1 : 0;
      if (const char* e = getenv("EKF_FUSE_SPLIT")) opt_fuse_split = atoi(e) ? 1 : 0;
      if (const char* e = getenv("EKF_SU_TAIL")) opt_su_tail = atoi(e) ? 1 : 0;
      if (const char* e = getenv("EKF_SYRK_MIRROR_SKIP")) opt_syrk_mirror_skip = atoi(e) ? 1 : 0;
      if (const char* e = getenv("EKF_SOLVE_POLL_CHAIN")) opt_solve_poll_chain = std::max(0, std::min(2, atoi(e)));
      if (const char* e = getenv("EKF_SMALL_ONELAUNCH")) opt_small_onelaunch = atoi(e) ? 1 : 0;
      if (const char* e = getenv("EKF_STEP_FUSED")) opt_step_fused = atoi(e) ? 1 : 0;
      if (const char* e = getenv("EKF_SHARD_DIST_CHAIN")) opt_shard_dist_chain = atoi(e) ? 1 : 0;
      if (const char* e = getenv("EKF_SHARD_DIST_MIN_BLOCKS")) shard_dist_min_blocks = std::max(2, atoi(e));
      if (const char* e = getenv("EKF_SMALL_STAMPS")) {
        if (atoi(e)) { HIPCHK(d_small_stamps.reserve(16)); HIPCHK(hipMemset(d_small_stamps, 0, 16 * sizeof(unsigned long long))); }
      }
      if (const char* e = getenv("EKF_CHAIN_DEFER")) opt_chain_defer = atoi(e) ? 1 : 0;
      if (const char* e = getenv("EKF_TD_MIN_BLOCKS")) td_min_blocks = std::max(1, atoi(e));
      if (const char* e = getenv("EKF_TD_MAX_BLOCKS")) td_max_blocks = std::max(1, atoi(e));
      if (const char* e = getenv("EKF_SPLIT_TAIL")) opt_split_tail = atoi(e);
      if (const char* e = getenv("EKF_SPLIT_BF16")) opt_split_bf16 = atoi(e) ? 1 : 0;   // = EKF_OPT_SPLIT_BF16, for A/B runs
      if (const char* e = getenv("EKF_CHUNKS")) {           // tuning knob: chunk ends in block steps
        for (const char* q = e; *q && env_nchunks < 8;) {
          env_chunks[env_nchunks++] = atoi(q);
          while (*q && *q != ',') ++q;
          if (*q == ',') ++q;
        }
      }
    }
    // mu0 / Sigma0 (vR.cpp:163-180, 211-216)
    std::vector<T> mu0(camera_dim, T(0));
    mu0[3] = T(0.0); mu0[4] = T(0.0); mu0[5] = T(-0.707106781); mu0[6] = T(0.707106781);
    if (camera_dim == 14) mu0[13] = T(1);
    n = camera_dim;
    N = 0;
    HIPCHK(hipMemcpyAsync(d_mu[0], mu0.data(), camera_dim * sizeof(T), hipMemcpyHostToDevice, stream));
    std::vector<T> S0((size_t)camera_dim * camera_dim, T(0));
    for (int i = 0; i < camera_dim; ++i) S0[(size_t)i * camera_dim + i] = T(0.0000000004);
    if (camera_dim == 14) S0[13 * 14 + 13] = T(0.09);
    const T sv2 = T(0.0004) * T(0.0004);
    for (int i = 7; i < 13; ++i) S0[(size_t)i * camera_dim + i] = sv2;
    HIPCHK(hipMemcpy2DAsync(d_S[0], (size_t)ld * sizeof(T), S0.data(), camera_dim * sizeof(T),
                            camera_dim * sizeof(T), camera_dim, hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
    extent[0] = n; extent[1] = 0;
    // the diagonal-block kernel needs > 64 KiB of LDS
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_chol_diag<T, 64>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, diag_lds(64)));
    // (f32, NB = 128 uses k_chol_diag_packed: 66 KiB of static LDS)
    if constexpr (kIsF32) {
      HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_trail_diag),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)kChainLds));
    }
    return EKF_OK;
  }
  static int diag_lds(int nb) { return 2 * nb * (nb + 1) * (int)sizeof(T); }

  T* S() { return d_S[cur]; }
  T* mu() { return d_mu[cur_mu]; }

  int sync_layout() {
    if (!layout_dirty) return EKF_OK;
    if (N > 0) {
      HIPCHK(hipMemcpyAsync(d_pos, ft.columns().pos.data(), N * sizeof(int), hipMemcpyHostToDevice, stream));
      HIPCHK(hipMemcpyAsync(d_coding, ft.columns().coding.data(), N * sizeof(int), hipMemcpyHostToDevice, stream));
      HIPCHK(hipStreamSynchronize(stream));   // host vectors may change right after
    }
    layout_dirty = false;
    return EKF_OK;
  }

  InputRing in_ring;                                    // z, the index list and the rescue's camera pose of a host caller -> d_z / d_midx / d_tmp
  PinnedBuf<char> h_pred;                               // host-mapped read-back buffer of ekf_get_predictions
  PinnedBuf<unsigned char> h_ransac;                    // ... of ekf_ransac_1point: counts, camera pose, small inlier masks
  static constexpr size_t kRansacMaskBytes = 65536;
  const unsigned char* ransac_mask_host = nullptr;      // the mask of the last ransac() call, if it came back with the counts
  int ransac_mask_M = 0;
  double ransac_cam[7] = {0, 0, 0, 0, 0, 0, 0};
  bool ransac_cam_valid = false;
  PinnedBuf<unsigned char> h_gate;                      // host-mapped gate flags of ekf_rescue_high_innovation
  int stage_inputs(const void* z, const int* idx, int M, const void* cam7 = nullptr) {
    HIPCHK(in_ring.stage(stream, M, d_z, z, d_midx, idx, d_tmp, cam7));   // (cam7: the state before the first update)
    return EKF_OK;
  }

  // Small device -> host reads of the getters: through ONE pinned bounce buffer, several pieces and the status words per
  // synchronisation (a copy into pageable memory is staged by the runtime and costs ~25 us; every getter used to pay that
  // twice, once for its data and once for the status words).
  ReadBack rb;
  // queue `bytes` from device `src` for host `dst` (copied out by rb_finish)
  int rb_add(void* dst, const void* src, size_t bytes) { HIPCHK(rb.add(dst, src, bytes, stream)); return EKF_OK; }
  // queue a rows x cols block (device pitch in bytes), packed row-major at dst
  int rb_add_2d(void* dst, const void* src, size_t pitch, size_t row_bytes, int rows) {
    HIPCHK(rb.add_2d(dst, src, pitch, row_bytes, rows, stream));
    return EKF_OK;
  }
  // one synchronisation for everything queued (+ the status words when asked for), then the pieces go to their places
  int rb_finish(bool with_status) {
    int st[4] = {0, 0, 0, 0};
    if (with_status) { int rc = rb_add(st, d_status, sizeof(st)); if (rc) return rc; }
    HIPCHK(rb.finish(stream));
    return with_status ? eval_status(st) : EKF_OK;
  }
  int eval_status(const int* st) {
    if (st[0] || st[1] || st[3]) {
      HIPCHK(hipMemsetAsync(d_status, 0, 4 * sizeof(int), stream));
      if (st[3]) {
        // the arrival gate of k_predict_fused was left mid-count: every launch that could still add to it has to be
        // over before it is cleared, and the fused predict launch stays off for this filter from here on
        HIPCHK(hipStreamSynchronize(stream));
        HIPCHK(hipMemsetAsync(d_status + 8, 0, 2 * sizeof(int), stream));      // ... and the gate of k_update_small_onelaunch
        small_gate_total = 0;
        opt_fused = 0;
        FAIL(EKF_ERR_DEVICE, "a bounded device-side wait gave up (fused launch); EKF_OPT_FUSED_LAUNCHES is now off for this filter");
      }
      if (st[1])
        FAIL(EKF_ERR_ARG, "ekf_update_device: a device-resident index is outside [0, N) or the list is not strictly "
                          "ascending (indices were clamped; the state is not meaningful)");
      FAIL(EKF_ERR_NUMERIC, "innovation covariance is not positive definite (Cholesky pivot <= 0)");
    }
    return EKF_OK;
  }

  int check_status() {
    return rb_finish(true);
  }
  // ---- simple accessors -----------------------------------------------------------------
  int set_dt(double v) override { if (!(v > 0)) FAIL(EKF_ERR_ARG, "dT must be positive"); dT = v; return EKF_OK; }
  double get_dt() const override { return dT; }
  int set_stream(void* s) override {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamSynchronize(stream));
    resolve_profile();
    if (own_stream) { hipStreamDestroy(stream); own_stream = false; }
    stream = reinterpret_cast<hipStream_t>(s);
    return EKF_OK;
  }
  int set_option(int o, int v) override {
    switch (o) {
      case EKF_OPT_PROPAGATE_STREAMING: opt_streaming = v ? 1 : 0; return EKF_OK;
      case EKF_OPT_USE_MFMA: opt_mfma = v ? 1 : 0; w_zeroed_n = -1; return EKF_OK;   // tile size changes the pads
      case EKF_OPT_PROFILE: resolve_profile(); prof.mode = v; return EKF_OK;
      case EKF_OPT_PIPELINE: opt_pipeline = (v < 0) ? -1 : v; return EKF_OK;
      case EKF_OPT_SPLIT_BF16: opt_split_bf16 = v ? 1 : 0; return EKF_OK;
      case EKF_OPT_FEATURE_NOISE: opt_feature_noise = (v > 0) ? 1e-12 * v : 0.0; return EKF_OK;
      case EKF_OPT_FUSED_LAUNCHES: opt_fused = v ? 1 : 0; return EKF_OK;
      case EKF_OPT_W_RECOMPUTE: opt_wrecompute = v ? 1 : 0; return EKF_OK;
      default: FAIL(EKF_ERR_ARG, "unknown option");
    }
  }
  int synchronize() override {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamSynchronize(stream));
    return check_status();
  }
  int num_features() const override { return N; }
  int state_dim() const override { return n; }
  int last_rows() const override { return last_m; }
  int get_layout(int* p, int* c) const override {
    for (int i = 0; i < N; ++i) { if (p) p[i] = ft.pos(i); if (c) c[i] = ft.coding(i); }
    return EKF_OK;
  }
  // (the caller may write through these pointers: the gathered diagonal blocks of a sharded filter are stale from here on)
  void* dev_mu() override { diag_synced = false; return mu(); }
  void* dev_sigma(int* l) override { diag_synced = false; if (l) *l = ld; return S(); }

  // ---- a12 add feature --------------------------------------------------------------------
  int add_feature(double u, double v) override {
    HIPCHK(hipSetDevice(device));
    const T uT = T(u), vT = T(v);
    const T hw = T(cam.half_window);
    if (!((uT > hw) && (vT > hw) && (uT < T(cam.width) - hw) && (vT < T(cam.height) - hw))) return 0;
    if (N >= capN) { err = "capacity_features exceeded"; return -EKF_ERR_CAPACITY; }
    { int rct = pull_track(); if (rct) return -rct; }
    {
      Scope sc(this, KID_ADD_FEATURE);
      k_add_prepare<T><<<1, 64, 0, stream>>>(mu(), S(), ld, n, cam, uT, vT, T(cfg.rho_0), T(sigma_pixel_2),
                                            T(cfg.sigma_rho_0), d_scr);
      k_add_border<T><<<(n + 255) / 256, 256, 0, stream>>>(S(), ld, n, d_scr);
    }
    if (hipGetLastError() != hipSuccess) { err = "add_feature launch failed"; return -EKF_ERR_DEVICE; }
    if (have_frame) {
      // Patch::Patch(cv::Mat(frame, cv::Rect(pf.x - w/2, pf.y - w/2, w, w)), ...) (vR.cpp:318): float -> int truncation
      const int w = cfg.window_size;
      const int x0 = (int)(float(u) - float(w / 2)), y0 = (int)(float(v) - float(w / 2));
      k_capture_patch<<<1, 256, 0, stream>>>(d_frame, frame_w, frame_h, x0, y0, w,
                                            d_patch[cur_patch] + (size_t)N * w * w, d_mpatch[cur_patch] + (size_t)N * w * w);
    }
    ft.add(n, float(u), float(v));
    N += 1;
    n += 6;
    shard_after_add();
    extent[cur] = std::max(extent[cur], n);
    layout_dirty = true;
    have_meas = false;
    return 1;
  }

  // ---- image side: frame, templates, predicted blur, NCC search ---------------
  int ensure_image_buffers() {
    if (d_patch[0]) return EKF_OK;
    const int w = cfg.window_size;
    if (w < 1 || w > kMaxWindow) FAIL(EKF_ERR_UNSUPPORTED, "window_size outside [1, 32] for the device matcher");
    const size_t bytes = (size_t)std::max(capN, 1) * w * w;
    for (int b = 0; b < 2; ++b) {
      HIPCHK(d_patch[b].reserve(bytes));
      HIPCHK(d_mpatch[b].reserve(bytes));
      HIPCHK(hipMemsetAsync(d_patch[b], 0, bytes, stream));
      HIPCHK(hipMemsetAsync(d_mpatch[b], 0, bytes, stream));
    }
    const size_t cn = (size_t)std::max(capN, 1);
    HIPCHK(d_hb.reserve(cn * 2));
    HIPCHK(d_zm.reserve(cn * 2));
    HIPCHK(d_found.reserve(cn));
    HIPCHK(d_score.reserve(cn));
    HIPCHK(d_keep.reserve(cn));
    return EKF_OK;
  }
  int set_frame(const unsigned char* gray, int width, int height, int stride) override {
    HIPCHK(hipSetDevice(device));
    if (!gray || width <= 0 || height <= 0 || stride < width) FAIL(EKF_ERR_ARG, "bad frame");
    if (width != cam.width || height != cam.height)
      FAIL(EKF_ERR_ARG, "frame size differs from ekf_config image_width / image_height");
    int rc = ensure_image_buffers();
    if (rc) return rc;
    HIPCHK(d_frame.reserve((size_t)width * height));
    HIPCHK(hipMemcpy2DAsync(d_frame, (size_t)width, gray, (size_t)stride, (size_t)width, height, hipMemcpyHostToDevice,
                            stream));
    HIPCHK(hipStreamSynchronize(stream));            // the caller's buffer may be reused at once
    frame_w = width; frame_h = height;
    have_frame = true;
    have_raw = false;                                // a key frame never pairs this frame with an older raw one
    return EKF_OK;
  }
  // The camera's frame as it comes: one 2-D copy into d_raw, one k_frame_ingest launch into d_frame.
  int set_frame_raw(const void* pixels, int width, int height, int channels, int stride, bool on_device) override {
    if (!pixels || width <= 0 || height <= 0) FAIL(EKF_ERR_ARG, "bad raw frame");
    if (channels != 1 && channels != 3) FAIL(EKF_ERR_ARG, "a raw frame has 1 (grey) or 3 (B, G, R) channels");
    if ((long long)stride < (long long)width * channels) FAIL(EKF_ERR_ARG, "stride is shorter than width * channels");
    if (cfg.scale < 1) FAIL(EKF_ERR_ARG, "ekf_config.scale must be >= 1 for a raw frame");
    const int Wo = width / cfg.scale, Ho = height / cfg.scale;
    if (Wo != cam.width || Ho != cam.height)
      FAIL(EKF_ERR_ARG, "raw frame size / scale differs from ekf_config image_width / image_height");
    const size_t row = (size_t)width * channels, need = row * height;
    if (need >= ((size_t)1 << 31)) FAIL(EKF_ERR_UNSUPPORTED, "raw frames of 2 GiB or more are not supported");
    HIPCHK(hipSetDevice(device));
    int rc = ensure_image_buffers();
    if (rc) return rc;
    const size_t out = (size_t)Wo * Ho;
    HIPCHK(d_frame.reserve(out));
    HIPCHK(d_raw.reserve(need + kIngestSlack));
    const int mode = (Wo == width && Ho == height) ? kIngestCopy
                     : (width == 2 * Wo && height == 2 * Ho) ? kIngestArea2 : kIngestLinear;
    if (mode == kIngestLinear && (ingest_tab_w != width || ingest_tab_h != height)) {
      std::vector<int> tab;
      ingest_tables(width, height, Wo, Ho, tab);
      const size_t recs = (size_t)Wo + Ho;
      ingest_tab_w = ingest_tab_h = 0;
      HIPCHK(d_ingest_tab.reserve(recs));
      HIPCHK(hipMemcpyAsync(d_ingest_tab, tab.data(), recs * sizeof(int4), hipMemcpyHostToDevice, stream));
      HIPCHK(hipStreamSynchronize(stream));          // (tab goes out of scope; once per geometry)
      ingest_tab_w = width; ingest_tab_h = height;
    }
    have_raw = false;
    {
      Scope sc(this, KID_FRAME_UPLOAD);
      HIPCHK(hipMemcpy2DAsync(d_raw, row, pixels, (size_t)stride, row, height,
                              on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
    }
    {
      Scope sc(this, KID_FRAME_INGEST);
      IngestArgs a{d_raw, d_frame, d_ingest_tab, d_ingest_tab ? d_ingest_tab + Wo : nullptr, width, height, Wo, Ho};
      // lanes per pass: copy 16 (C = 1) / 4 (C = 3) pixels each, area 4, linear 1; at most 1024 workgroups, then grid-stride
      const size_t per = mode == kIngestCopy ? (channels == 1 ? 16 : 4) : (mode == kIngestArea2 ? 4 : 1);
      const size_t lanes = mode == kIngestArea2 ? (size_t)((Wo + 3) / 4) * Ho : (out + per - 1) / per;
      const int grid = (int)std::min<size_t>((lanes + 255) / 256, 1024);
      auto go = [&](auto cc, auto mm) { k_frame_ingest<decltype(cc)::value, decltype(mm)::value><<<grid, 256, 0, stream>>>(a); };
      using I1 = std::integral_constant<int, 1>; using I3 = std::integral_constant<int, 3>;
      using M0 = std::integral_constant<int, kIngestCopy>; using M1 = std::integral_constant<int, kIngestArea2>;
      using M2 = std::integral_constant<int, kIngestLinear>;
      if (channels == 1) { if (mode == kIngestCopy) go(I1{}, M0{}); else if (mode == kIngestArea2) go(I1{}, M1{}); else go(I1{}, M2{}); }
      else { if (mode == kIngestCopy) go(I3{}, M0{}); else if (mode == kIngestArea2) go(I3{}, M1{}); else go(I3{}, M2{}); }
      HIPCHK(hipGetLastError());
    }
    if (!on_device) HIPCHK(hipStreamSynchronize(stream));     // the caller's buffer may be reused at once
    frame_w = Wo; frame_h = Ho;
    raw_w = width; raw_h = height; raw_c = channels;
    have_frame = true;
    have_raw = true;
    return EKF_OK;
  }
  int get_frame(unsigned char* gray, int stride) override {
    if (!gray || stride < frame_w) FAIL(EKF_ERR_ARG, "ekf_get_frame: gray must not be NULL and stride >= image_width");
    if (!have_frame) FAIL(EKF_ERR_STATE, "ekf_get_frame: no frame was set");
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipMemcpy2DAsync(gray, (size_t)stride, d_frame, (size_t)frame_w, (size_t)frame_w, frame_h, hipMemcpyDeviceToHost,
                            stream));
    HIPCHK(hipStreamSynchronize(stream));
    return EKF_OK;
  }
  // ---- rectification for pinhole consumers (kernels in ekf_rectify.hpp) ---------------------------------
  // raw = 0: the matcher frame (s = 1); raw = 1: the raw frame (s = ekf_config.scale), whose geometry is known once a raw
  // frame was set.  Nothing of the filter's state is read or written, and no launch kind is counted.
  int rectified_camera(int raw, ekf_sba_camera* K) override {
    if ((raw != 0 && raw != 1) || !K) FAIL(EKF_ERR_ARG, "ekf_rectified_camera: raw is 0 or 1 and K must not be NULL");
    if (raw && raw_w <= 0) FAIL(EKF_ERR_STATE, "ekf_rectified_camera: no raw frame was set (the raw geometry is unknown)");
    double k[4];
    rect_camera(rect_cam(cam, raw ? cfg.scale : 1), k);
    K->fx = k[0]; K->fy = k[1]; K->cx = k[2]; K->cy = k[3];
    return EKF_OK;
  }
  int get_frame_rectified(int raw, unsigned char* out, int stride) override {
    if ((raw != 0 && raw != 1) || !out) FAIL(EKF_ERR_ARG, "ekf_get_frame_rectified: raw is 0 or 1 and out must not be NULL");
    if (!have_frame) FAIL(EKF_ERR_STATE, "ekf_get_frame_rectified: no frame was set");
    if (raw && !have_raw) FAIL(EKF_ERR_STATE, "ekf_get_frame_rectified: no raw frame is held (ekf_set_frame_raw)");
    const int W = raw ? raw_w : frame_w, H = raw ? raw_h : frame_h, Cn = raw ? raw_c : 1;
    if ((long long)stride < (long long)W * Cn) FAIL(EKF_ERR_ARG, "ekf_get_frame_rectified: stride is shorter than a row");
    HIPCHK(hipSetDevice(device));
    {
      Scope sc(this, KID_FRAME_RECTIFY);
      HIPCHK(rectify_launch(rect, stream, raw ? d_raw : d_frame, W, H, Cn, rect_cam(cam, raw ? cfg.scale : 1)));
    }
    HIPCHK(rectified_to_host(rect, stream, W, H, Cn, out, (size_t)stride));
    return EKF_OK;
  }
  int undistort_pixels(int raw, const double* uv, int n, double* out) override {
    if ((raw != 0 && raw != 1) || n < 0 || (n > 0 && (!uv || !out)))
      FAIL(EKF_ERR_ARG, "ekf_undistort_pixels: raw is 0 or 1, n >= 0, uv and out must not be NULL");
    if (raw && raw_w <= 0) FAIL(EKF_ERR_STATE, "ekf_undistort_pixels: no raw frame was set (the raw geometry is unknown)");
    if (n == 0) return EKF_OK;
    HIPCHK(hipSetDevice(device));
    HIPCHK(undistort_to_host(rect, stream, uv, n, rect_cam(cam, raw ? cfg.scale : 1), out));
    return EKF_OK;
  }
  int set_patch(int index, const unsigned char* data) override {
    HIPCHK(hipSetDevice(device));
    if (index < 0 || index >= N || !data) FAIL(EKF_ERR_ARG, "feature index out of range");
    int rc = ensure_image_buffers();
    if (rc) return rc;
    const size_t w2 = (size_t)cfg.window_size * cfg.window_size;
    HIPCHK(hipMemcpyAsync(d_patch[cur_patch] + index * w2, data, w2, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_mpatch[cur_patch] + index * w2, data, w2, hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return EKF_OK;
  }
  int get_patch(int index, int matching, unsigned char* out) override {
    HIPCHK(hipSetDevice(device));
    if (index < 0 || index >= N || !out) FAIL(EKF_ERR_ARG, "feature index out of range");
    if (!d_patch[0]) FAIL(EKF_ERR_STATE, "no templates: call ekf_set_frame / ekf_set_patch first");
    const size_t w2 = (size_t)cfg.window_size * cfg.window_size;
    const unsigned char* src = (matching ? d_mpatch[cur_patch] : d_patch[cur_patch]) + index * w2;
    HIPCHK(hipMemcpyAsync(out, src, w2, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return EKF_OK;
  }
  // predicted blur of every visible feature's template (inside predict(), vR.cpp:496-500, 546-548, 575-576)
  int launch_blur() {
    have_blur = false;
    if (!d_patch[0] || N == 0) return EKF_OK;
    Scope sc(this, KID_MISC);
    k_blur_points<T><<<(N + 63) / 64, 64, 0, stream>>>(mu(), d_pos, d_coding, N, cam, T(cfg.T_camera), T(dT), d_hb);
    k_blur_templates<T><<<N, 256, 0, stream>>>(d_h, d_hb, d_flags, cfg.window_size, cfg.kernel_size, d_patch[cur_patch],
                                               d_mpatch[cur_patch]);
    HIPCHK(hipGetLastError());
    have_blur = true;
    return EKF_OK;
  }
  int blur_predictions(void* out) override {
    HIPCHK(hipSetDevice(device));
    if (!have_blur) FAIL(EKF_ERR_STATE, "no blur predictions: ekf_predict with templates present computes them");
    if (N) HIPCHK(hipMemcpyAsync(out, d_hb, (size_t)N * 2 * sizeof(T), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return EKF_OK;
  }
  int find_matches(double threshold, void* z, unsigned char* found, float* score) override {
    HIPCHK(hipSetDevice(device));
    if (!have_frame) FAIL(EKF_ERR_STATE, "ekf_find_matches needs ekf_set_frame");
    if (!have_meas) FAIL(EKF_ERR_STATE, "ekf_find_matches needs the predictions of ekf_predict / ekf_measure");
    if (N == 0) return EKF_OK;
    // (sharded filter: the frame, the templates and -- after ekf_predict's "reassemble H" -- h are replicated, the 2x2 St
    // blocks are owner-computed and all-gathered by ensure_sd(), a COLLECTIVE; every rank then searches every feature:
    // the matching templates the search rewrites stay identical on every rank, and nothing else is exchanged)
    int rc = ensure_sd();
    if (rc) return rc;
    {
      Scope sc(this, KID_MISC);
      k_ncc_search<T><<<N, 256, 0, stream>>>(d_frame, frame_w, frame_h, d_h, d_Sd, d_flags, cfg.window_size,
                                             float(cfg.sigma_size), float(threshold), d_mpatch[cur_patch], d_zm, d_found,
                                             d_score);
    }
    HIPCHK(hipGetLastError());
    // the results through the pinned bounce buffer, together with the folded flags of the last predict: one
    // synchronisation (z and found always come back: the track state follows them)
    std::vector<T> zm((size_t)N * 2);
    std::vector<unsigned char> fd(N), tb;
    const bool fold = trk_dirty;
    if (fold) { tb.resize(N); rc = rb_add(tb.data(), d_trk, (size_t)N); if (rc) return rc; }
    rc = rb_add(zm.data(), d_zm, (size_t)N * 2 * sizeof(T)); if (rc) return rc;
    rc = rb_add(fd.data(), d_found, (size_t)N); if (rc) return rc;
    if (score) { rc = rb_add(score, d_score, (size_t)N * sizeof(float)); if (rc) return rc; }
    rc = rb_finish(false);
    if (rc) return rc;
    if (fold) {
      HIPCHK(hipMemsetAsync(d_trk, 0, (size_t)N, stream));        // (stream-ordered: before the next fold)
      apply_track(tb);
    }
    if (z) memcpy(z, zm.data(), zm.size() * sizeof(T));
    if (found) memcpy(found, fd.data(), fd.size());
    // Patch::findMatch of every searched (= visible) feature: n_tot + 1 (Patch.cpp:218), the centre becomes the matched
    // pixel or (-1, -1) (:253, 279), a failed search clears isInInnovation (:281)
    for (int i = 0; i < N; ++i)
      if (ft.in_innovation(i)) ft.searched(i, fd[i] != 0, float(zm[2 * i]), float(zm[2 * i + 1]));
    return EKF_OK;
  }

  // ---- track state: n_tot, center, isInInnovation, removeFlag ------------------------------------
  int launch_track_fold() {
    if (N > 0) {
      k_track_fold<<<(N + 255) / 256, 256, 0, stream>>>(d_flags, d_trk, N);
      HIPCHK(hipGetLastError());
      trk_dirty = true;
    }
    return EKF_OK;
  }
  void apply_track(const std::vector<unsigned char>& b) {
    ft.fold_track(b);
    trk_dirty = false;
  }
  int pull_track() {
    if (!trk_dirty) return EKF_OK;
    std::vector<unsigned char> b(N);
    if (N > 0) {
      int rc = rb_add(b.data(), d_trk, (size_t)N);
      if (rc) return rc;
      rc = rb_finish(false);
      if (rc) return rc;
      HIPCHK(hipMemsetAsync(d_trk, 0, (size_t)N, stream));
    }
    apply_track(b);
    return EKF_OK;
  }
  int get_track(int* nt, unsigned char* inn, float* cen, unsigned char* rem) override {
    HIPCHK(hipSetDevice(device));
    int rc = pull_track();
    if (rc) return rc;
    for (int i = 0; i < N; ++i) {
      if (nt) nt[i] = ft.n_tot(i);
      if (inn) inn[i] = ft.in_innovation(i);
      if (cen) { cen[2 * i] = ft.center(i)[0]; cen[2 * i + 1] = ft.center(i)[1]; }
      if (rem) rem[i] = ft.remove_flag(i);
    }
    return EKF_OK;
  }
  int set_track(int index, int nt, int inn, const float* cen, int rem) override {
    HIPCHK(hipSetDevice(device));
    if (index < 0 || index >= N) FAIL(EKF_ERR_ARG, "feature index out of range");
    int rc = pull_track();
    if (rc) return rc;
    ft.set_track(index, nt, inn, cen, rem);
    return EKF_OK;
  }

  // ---- corner seeding: VSlamFilter::findNewFeatures (vR.cpp:783-837), kernels in ekf_features.hpp ---------------
  // corners -> out (raster indices, acceptance order), *n_out corners
  int detect_corners(int num, double quality, double min_distance, std::vector<int>& out) {
    const int W = frame_w, H = frame_h, w = cfg.window_size;
    const size_t px = (size_t)W * H;
    if (!d_seed_mask) {
      HIPCHK(d_seed_mask.reserve(px));
      HIPCHK(d_seed_lam.reserve(px));
      HIPCHK(d_seed_aux.reserve(2));
      HIPCHK(d_seed_ckey.reserve(px));
      HIPCHK(d_seed_cidx.reserve(px));
      HIPCHK(d_seed_org.reserve((size_t)std::max(capN, 1) * 2));
      HIPCHK(d_seed_out.reserve(px + 1));                               // (more corners than pixels cannot be accepted)
    }
    int rc = pull_track();
    if (rc) return rc;
    // the squares of the existing patches (vR.cpp:795-817): float compares, (int) truncation of the origin
    std::vector<int> org;
    for (int i = 0; i < N; ++i) {
      const float cx = ft.center(i)[0], cy = ft.center(i)[1];
      if (cx > (float)w && cy > (float)w && cx < (float)(W - w) && cy < (float)(H - w)) {
        org.push_back((int)(cx - (float)w));
        org.push_back((int)(cy - (float)w));
      }
    }
    const int nsq = (int)org.size() / 2;
    if (nsq) HIPCHK(hipMemcpyAsync(d_seed_org, org.data(), org.size() * sizeof(int), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemsetAsync(d_seed_aux, 0, 2 * sizeof(unsigned long long), stream));
    // integer d^2 < md^2  <=>  d^2 < ceil(md^2); no two pixels are further apart than W^2 + H^2 (the clamp keeps the
    // conversion defined for any finite min_distance)
    const double dmax = (double)W * W + (double)H * H + 1.0;
    const long long md2i = (long long)std::ceil(std::min(min_distance * min_distance, dmax));
    const int g = (int)((px + 255) / 256);
    int* d_cnt = reinterpret_cast<int*>(d_seed_aux + 1);
    {
      Scope sc(this, KID_SEED_MASK);
      k_seed_mask_init<<<g, 256, 0, stream>>>(d_seed_mask, W, H, w);
      if (nsq) k_seed_mask_paint<<<nsq, 256, 0, stream>>>(d_seed_mask, W, H, w, d_seed_org);
    }
    {
      Scope sc(this, KID_SEED_RESPONSE);
      k_seed_response<<<dim3((W + kSeedTile - 1) / kSeedTile, (H + kSeedTile - 1) / kSeedTile), 256, 0, stream>>>(
          d_frame, W, H, d_seed_mask, d_seed_lam, d_seed_aux);
    }
    {
      Scope sc(this, KID_SEED_CANDIDATES);
      k_seed_candidates<<<g, 256, 0, stream>>>(d_seed_lam, W, H, d_seed_mask, quality, d_seed_aux, d_cnt, d_seed_ckey,
                                               d_seed_cidx);
    }
    {
      Scope sc(this, KID_SEED_SELECT);
      k_seed_select<<<1, kSeedSelectThreads, 0, stream>>>(d_cnt, d_seed_ckey, d_seed_cidx, W, num, md2i, d_seed_out);
    }
    HIPCHK(hipGetLastError());
    have_seed_lam = true;
    out.assign((size_t)num + 1, 0);
    rc = rb_add(out.data(), d_seed_out, out.size() * sizeof(int));     // (the count and the corners: one copy)
    if (rc) return rc;
    rc = rb_finish(false);
    if (rc) return rc;
    const int cnt = std::min(std::max(out[0], 0), num);
    out.erase(out.begin());
    out.resize(cnt);
    return EKF_OK;
  }
  int find_new_features(int num, double quality, double min_distance, int add, float* out_uv, int* n_out) override {
    HIPCHK(hipSetDevice(device));
    if (!(quality >= 0.0) || !(min_distance >= 0.0) || !std::isfinite(quality) || !std::isfinite(min_distance))
      FAIL(EKF_ERR_ARG, "quality_level and min_distance must be finite and >= 0");
    if (!have_frame) FAIL(EKF_ERR_STATE, "ekf_find_new_features needs ekf_set_frame");
    if (num <= 0) num = cfg.nInitFeatures;                            // vR.cpp:785
    if (n_out) *n_out = 0;
    if (num <= 0) return EKF_OK;
    num = (int)std::min<long long>(num, (long long)frame_w * frame_h);   // (no more corners than pixels exist)
    if (frame_w < 3 || frame_h < 3) FAIL(EKF_ERR_UNSUPPORTED, "frame smaller than 3 x 3");
    std::vector<int> cs;
    int rc = detect_corners(num, quality, min_distance, cs);
    if (rc) return rc;
    const int cnt = (int)cs.size();
    if (out_uv)
      for (int k = 0; k < cnt; ++k) { out_uv[2 * k] = float(cs[k] % frame_w); out_uv[2 * k + 1] = float(cs[k] / frame_w); }
    if (n_out) *n_out = cnt;
    if (add)
      for (int k = 0; k < cnt && N < capN; ++k) {                    // addFeature (vR.cpp:830-833), up to the capacity
        const int ra = add_feature(double(cs[k] % frame_w), double(cs[k] / frame_w));
        if (ra < 0) return -ra;
      }
    return EKF_OK;
  }

  // ---- the end of VSlamFilter::update() (vR.cpp:1294-1317) ---------------------------------------------------
  int end_update(float matching_ratio, int seed, int* removed, int* n_removed, int* n_visible, int* n_seeded) override {
    HIPCHK(hipSetDevice(device));
    if (n_removed) *n_removed = 0;
    if (n_visible) *n_visible = 0;
    if (n_seeded) *n_seeded = 0;
    if (N == 0) return EKF_OK;
    // seeding needs the frame: refused before anything changes, so a failed call leaves the map as it was
    if (seed && !have_frame) FAIL(EKF_ERR_STATE, "ekf_end_update with seed != 0 needs ekf_set_frame");
    int rc = pull_track();
    if (rc) return rc;
    // update_quality_index (Patch.cpp:143-150; n_find was counted by ekf_update_two_stage) and removal in descending order
    std::vector<int> rm;
    for (int i = N - 1; i >= 0; --i) {
      const float q = (float)(ft.n_tot(i) - ft.n_find(i)) / ((float)ft.n_find(i));
      if (q > matching_ratio) ft.flag_removal(i);
      if (ft.remove_flag(i)) rm.push_back(i);
    }
    if (removed) for (size_t k = 0; k < rm.size(); ++k) removed[k] = rm[k];
    if (n_removed) *n_removed = (int)rm.size();
    if (!rm.empty()) {
      rc = remove_features(rm.data(), (int)rm.size());
      if (rc) return rc;
    }
    int vis = 0;                                                       // :1301-1302
    for (int i = 0; i < N; ++i) vis += ft.in_innovation(i) ? 1 : 0;
    if (n_visible) *n_visible = vis;
    if (vis < cfg.min_features) {                                      // :1311-1315
      if (N > cfg.max_features) {
        const int zero = 0;
        rc = remove_features(&zero, 1);
        if (rc) return rc;
      }
      const int want = cfg.min_features - vis;
      if (seed) {
        const int before = N;
        rc = find_new_features(want, 0.01, 12.0, 1, nullptr, nullptr);
        if (rc) return rc;
        if (n_seeded) *n_seeded = N - before;
      } else if (n_seeded) {
        *n_seeded = want;
      }
    }
    rc = convert(0, true);                                             // :1317
    return rc < 0 ? -rc : EKF_OK;
  }

  // zero everything of buffer `b` outside the live n x n (up to what was ever written there)
  int zero_border(int b, int n_live) {
    const int ext = extent[b];
    if (ext > n_live) {
      // rows [n_live, ext): full width; rows [0, n_live): columns [n_live, ext)
      HIPCHK(hipMemset2DAsync(d_S[b] + (size_t)n_live * ld, (size_t)ld * sizeof(T), 0, (size_t)ext * sizeof(T),
                              ext - n_live, stream));
      HIPCHK(hipMemset2DAsync(d_S[b] + n_live, (size_t)ld * sizeof(T), 0, (size_t)(ext - n_live) * sizeof(T),
                              n_live, stream));
    }
    extent[b] = n_live;
    return EKF_OK;
  }

  // ---- a13 / a14: one out-of-place pass for a set of removals and conversions -------------
  hipError_t ensure_arch_idx(size_t count) { return d_arch_idx.reserve(count, std::max<size_t>(2 * count, 256)); }

  // vR.cpp:394-404: a removed XYZ feature that was found more than 5 times is kept (XYZ_pos, cov_4_delete, real_index)
  int archive_removed(const std::vector<char>& rm) {
    std::vector<int> ap, ar;
    for (int i = 0; i < N; ++i)
      if (rm[i] && ft.coding(i) != 0 && ft.n_find(i) > 5) { ap.push_back(ft.pos(i)); ar.push_back(ft.real_index(i)); }
    if (ap.empty()) return EKF_OK;
    // sharded: the 3 x 3 block of a removed feature is valid on its owner only -- gathered first, so that every rank
    // archives the same 12 scalars (the list above is the same on every rank: host metadata is replicated)
    int rc = shard_sync_diag_blocks();
    diag_synced = false;                                     // the removal that follows compacts Sigma
    if (rc) return rc;
    const size_t have = arch_real.size(), need = have + ap.size();
    if (need * 12 > d_archive.capacity()) {                  // the one growth that keeps its contents: new, copy, swap
      DevBuf<T> nbuf;
      HIPCHK(nbuf.reserve(std::max<size_t>(2 * need, 256) * 12));
      if (have) HIPCHK(hipMemcpyAsync(nbuf, d_archive, have * 12 * sizeof(T), hipMemcpyDeviceToDevice, stream));
      HIPCHK(hipStreamSynchronize(stream));
      d_archive = std::move(nbuf);
    }
    HIPCHK(ensure_arch_idx(ap.size()));
    HIPCHK(hipMemcpyAsync(d_arch_idx, ap.data(), ap.size() * sizeof(int), hipMemcpyHostToDevice, stream));
    k_archive_points<T><<<((int)ap.size() * 12 + 255) / 256, 256, 0, stream>>>(mu(), S(), ld, d_arch_idx, (int)ap.size(),
                                                                             d_archive + have * 12);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(stream));          // `ap` goes out of scope
    arch_real.insert(arch_real.end(), ar.begin(), ar.end());
    return EKF_OK;
  }

  int compact(const std::vector<char>& rm, const std::vector<char>& cv) {
    { int rct = pull_track(); if (rct) return rct; }
    { int rca = archive_removed(rm); if (rca) return rca; }
    FeatureTable::Compaction next = ft.compacted(rm, cv, camera_dim);
    const std::vector<int>&msrc = next.msrc, &mconv = next.mconv;
    const int n_new = (int)msrc.size();
    HIPCHK(hipMemcpyAsync(d_map_src, msrc.data(), n_new * sizeof(int), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_map_conv, mconv.data(), n_new * sizeof(int), hipMemcpyHostToDevice, stream));
    const int dst = 1 - cur, dmu = 1 - cur_mu;
    {
      Scope sc(this, KID_COMPACT);
      dim3 grid((n_new + 1023) / 1024, (n_new + kCompactRows - 1) / kCompactRows);   // four columns per lane, kCompactRows rows per workgroup
      k_compact_transform<T><<<grid, 256, 0, stream>>>(S(), d_S[dst], ld, n_new, d_map_src, d_map_conv, d_Jy);
      k_compact_mu<T><<<(n_new + 255) / 256, 256, 0, stream>>>(mu(), d_mu[dmu], n_new, d_map_src, d_map_conv,
                                                              d_Yxyz);
    }
    HIPCHK(hipGetLastError());
    std::vector<int> keep;
    if (d_patch[0]) {                            // the templates follow their features (patches.erase, vR.cpp:1298)
      for (int i = 0; i < N; ++i)
        if (!rm[i]) keep.push_back(i);
      if (!keep.empty() && (int)keep.size() != N) {
        const int w2 = cfg.window_size * cfg.window_size;
        HIPCHK(hipMemcpyAsync(d_keep, keep.data(), keep.size() * sizeof(int), hipMemcpyHostToDevice, stream));
        k_gather_patches<<<(int)keep.size(), 256, 0, stream>>>(d_patch[cur_patch], d_patch[1 - cur_patch], d_keep, w2);
        k_gather_patches<<<(int)keep.size(), 256, 0, stream>>>(d_mpatch[cur_patch], d_mpatch[1 - cur_patch], d_keep, w2);
        cur_patch = 1 - cur_patch;
      }
    }
    extent[dst] = std::max(extent[dst], n_new);
    int rc = zero_border(dst, n_new);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(stream));        // host map vectors go out of scope
    cur = dst; cur_mu = dmu;
    ft.adopt(std::move(next.cols));
    N = ft.size();
    n = n_new;
    shard_after_compact(rm);
    layout_dirty = true;
    have_meas = false;
    return EKF_OK;
  }

  int remove_features(const int* idx, int count) override {
    HIPCHK(hipSetDevice(device));
    if (count <= 0) return EKF_OK;
    std::vector<char> rm(N, 0), cv(N, 0);
    for (int k = 0; k < count; ++k) {
      if (idx[k] < 0 || idx[k] >= N) FAIL(EKF_ERR_ARG, "feature index out of range");
      rm[idx[k]] = 1;
    }
    return compact(rm, cv);
  }

  int convert(int index, bool all) override {
    HIPCHK(hipSetDevice(device));
    if (sh_on) return shard_convert(index, all);
    if (!all && (index < 0 || index >= N)) { err = "feature index out of range"; return -EKF_ERR_ARG; }
    if (N == 0) return 0;
    int rc = sync_layout();
    if (rc) return -rc;
    k_linearity<T><<<(N + 127) / 128, 128, 0, stream>>>(mu(), S(), ld, d_pos, d_coding, N, d_cflag, d_Jy, d_Yxyz, 0);
    std::vector<unsigned char> fl(N);
    if (rb_add(fl.data(), d_cflag, N) != EKF_OK || rb_finish(false) != EKF_OK) { err = "linearity flags D2H failed"; return -EKF_ERR_DEVICE; }
    std::vector<char> rm(N, 0), cv(N, 0);
    int cnt = 0;
    for (int i = 0; i < N; ++i) {
      if (!all && i != index) continue;
      if (fl[i] && ft.coding(i) == 0) { cv[i] = 1; ++cnt; }
    }
    if (cnt == 0) return 0;
    rc = compact(rm, cv);
    if (rc) return -rc;
    return cnt;
  }

  // ---- a1-a6 predict --------------------------------------------------------------------
  int launch_measure() {
    int rc = sync_layout();
    if (rc) return rc;
    if (N > 0) {
      Scope sc(this, KID_MEASURE);
      k_measure<T><<<(N + 63) / 64, 64, 0, stream>>>(mu(), d_pos, d_coding, 0, N, cam, d_h, d_Hc, d_Hf, d_flags);
    }
    HIPCHK(hipGetLastError());
    rc = launch_track_fold();
    if (rc) return rc;
    have_meas = true;
    have_sd = false;
    return EKF_OK;
  }

  MotionArgs motion_args(const void* tc, const void* rc_, int vcontrol) const {
    MotionArgs a;
    a.dT = dT;
    const T* t = static_cast<const T*>(tc);
    const T* r = static_cast<const T*>(rc_);
    for (int i = 0; i < 3; ++i) { a.t_ctl[i] = t ? double(t[i]) : 0.0; a.r_ctl[i] = r ? double(r[i]) : 0.0; }
    for (int i = 0; i < 6; ++i) a.vdiag[i] = vcontrol ? vmax[i] : double(T(vmax[i]) * T(2));   // vR.cpp:202
    return a;
  }

  // Camera step, Sigma's camera rows and columns propagated (in place by strips; `streaming`: into the other buffer), then the
  // feature-noise inflation
  int propagate(const MotionArgs& a, bool streaming) {
    {
      Scope sc(this, KID_PREDICT_CAMERA);
      k_predict_camera<T><<<1, 64, 0, stream>>>(mu(), d_scr, a);
    }
    have_motion = true;
    if (streaming) {
      const int dst = 1 - cur;
      {
        Scope sc(this, KID_PROPAGATE_STREAMING);
        k_propagate_streaming<T><<<n, 256, 0, stream>>>(S(), d_S[dst], ld, n, d_scr + SCR_FT, d_scr + SCR_Q);
      }
      extent[dst] = std::max(extent[dst], n);
      int rc = zero_border(dst, n);
      if (rc) return rc;
      cur = dst;
    } else {
      Scope sc(this, KID_PROPAGATE_STRIPS);
      k_strip_congruence<T, 13><<<(2 * n + 255) / 256, 256, 0, stream>>>(S(), ld, n, 0, d_scr + SCR_FT, d_scr + SCR_Q);
    }
    if (opt_feature_noise > 0.0 && n > camera_dim)
      k_inflate_diagonal<T><<<(n - camera_dim + 255) / 256, 256, 0, stream>>>(S(), ld, camera_dim, n, T(opt_feature_noise));
    HIPCHK(hipGetLastError());
    return EKF_OK;
  }

  int predict(const void* tc, const void* rc_, int vcontrol) override {
    HIPCHK(hipSetDevice(device));
    if (sh_on) return shard_predict(tc, rc_, vcontrol);
    const MotionArgs a = motion_args(tc, rc_, vcontrol);
    if (opt_fused && !opt_streaming && !(opt_feature_noise > 0.0) && N > 0 && !prof.on(KID_PREDICT_CAMERA) &&
        !prof.on(KID_PROPAGATE_STRIPS) && !prof.on(KID_MEASURE)) {
      // camera step, strip congruence and the per-feature h / H as ONE launch (k_predict_fused): same arithmetic,
      // two launches less per frame
      int rc = sync_layout();
      if (rc) return rc;
      const int nstrip = (2 * n + 255) / 256;
      k_predict_fused<T><<<nstrip + (N + 255) / 256, 256, 0, stream>>>(mu(), d_scr, a, S(), ld, n, nstrip, d_pos, d_coding, N,
                                                                      cam, d_h, d_Hc, d_Hf, d_flags, d_status + 8, d_status);
      HIPCHK(hipGetLastError());
      rc = launch_track_fold();
      if (rc) return rc;
      have_motion = true;
      have_update = false;
      have_meas = true;
      have_sd = false;
      return launch_blur();
    }
    int rcp = propagate(a, opt_streaming);
    if (rcp) return rcp;
    have_update = false;
    int rcm = launch_measure();
    if (rcm) return rcm;
    return launch_blur();
  }

  int measure() override {
    HIPCHK(hipSetDevice(device));
    return launch_measure();
  }

  bool have_motion = false;
  int motion_jacobian(void* Ft, void* Q) override {
    HIPCHK(hipSetDevice(device));
    if (!have_motion) FAIL(EKF_ERR_STATE, "no motion Jacobian: call ekf_predict first");
    T buf[2 * 169];
    { int rc = rb_add(buf, d_scr + SCR_FT, sizeof(buf)); if (rc) return rc; rc = rb_finish(false); if (rc) return rc; }   // SCR_FT, SCR_Q adjacent
    for (int b = 0; b < 2; ++b) {
      T* o = static_cast<T*>(b ? Q : Ft);
      if (!o) continue;
      for (int r = 0; r < 13; ++r)
        for (int c = 0; c < 13; ++c) o[c * 13 + r] = buf[b * 169 + r * 13 + c];
    }
    return EKF_OK;
  }

  // 2x2 St blocks on demand (they need the propagated Sigma and the current H; nothing on the device
  // consumes them except the ellipse / RANSAC kernels)
  int ensure_sd() {
    if (have_sd || N == 0) return EKF_OK;
    if (sh_on) {
      // a 2x2 block needs the rows of Sigma of its feature: every rank evaluates the features it owns, then the blocks
      // are all-gathered (4 scalars per feature)
      const int f0 = own_f0(), f1 = own_f1();
      if (f1 > f0)
        k_measure_sd<T><<<(16 * (f1 - f0) + 255) / 256, 256, 0, stream>>>(S(), ld, d_pos, d_coding, f0, f1, T(sigma_pixel_2),
                                                                        d_Hc, d_Hf, d_Sd);
      HIPCHK(hipGetLastError());
      int rc = gather_sd(feature_tab(), nullptr);
      if (rc) return rc;
      have_sd = true;
      return EKF_OK;
    }
    k_measure_sd<T><<<(16 * N + 255) / 256, 256, 0, stream>>>(S(), ld, d_pos, d_coding, 0, N, T(sigma_pixel_2), d_Hc, d_Hf,
                                                             d_Sd);
    HIPCHK(hipGetLastError());
    have_sd = true;
    return EKF_OK;
  }

  int get_predictions(void* h, unsigned char* vis, unsigned char* rem, void* s2, void* hc, void* hf) override {
    HIPCHK(hipSetDevice(device));
    if (!have_meas) FAIL(EKF_ERR_STATE, "no predictions: call ekf_predict / ekf_measure first");
    if (N == 0) return EKF_OK;
    // h, flags and the 2x2 blocks come back through ONE host-mapped pinned buffer the device writes (k_pack_predictions):
    // one launch + one synchronisation per frame for the drop-in caller, instead of three staged copies
    HIPCHK(h_pred.reserve((size_t)capN * (6 * sizeof(T) + 1) + 64));
    T* ph = reinterpret_cast<T*>(static_cast<char*>(h_pred));
    T* psd = ph + (size_t)2 * capN;
    unsigned char* pfl = reinterpret_cast<unsigned char*>(psd + (size_t)4 * capN);
    std::vector<T> vhc, vhf;
    if (s2 && !have_sd && !sh_on) {              // the 2x2 blocks and the packing in ONE launch
      k_measure_sd<T><<<(16 * N + 255) / 256, 256, 0, stream>>>(S(), ld, d_pos, d_coding, 0, N, T(sigma_pixel_2), d_Hc, d_Hf,
                                                               d_Sd, nullptr, 0, d_h, d_flags, ph, psd, pfl);
      have_sd = true;
    } else {
      if (s2) { int rcs = ensure_sd(); if (rcs) return rcs; }
      k_pack_predictions<T><<<(4 * N + 255) / 256, 256, 0, stream>>>(d_h, s2 ? d_Sd : static_cast<const T*>(nullptr), d_flags, N,
                                                                    ph, psd, pfl);
    }
    HIPCHK(hipGetLastError());
    if (hc) { vhc.resize((size_t)N * 14); HIPCHK(hipMemcpyAsync(vhc.data(), d_Hc, vhc.size() * sizeof(T), hipMemcpyDeviceToHost, stream)); }
    if (hf) { vhf.resize((size_t)N * 12); HIPCHK(hipMemcpyAsync(vhf.data(), d_Hf, vhf.size() * sizeof(T), hipMemcpyDeviceToHost, stream)); }
    HIPCHK(hipStreamSynchronize(stream));
    if (h) memcpy(h, ph, (size_t)N * 2 * sizeof(T));
    for (int i = 0; i < N; ++i) { if (vis) vis[i] = pfl[i] & 1; if (rem) rem[i] = (pfl[i] >> 1) & 1; }
    if (s2) {                                    // row-major 2x2 -> column-major
      T* o = static_cast<T*>(s2);
      const T* sd = psd;
      for (int i = 0; i < N; ++i) { o[4 * i] = sd[4 * i]; o[4 * i + 1] = sd[4 * i + 2]; o[4 * i + 2] = sd[4 * i + 1]; o[4 * i + 3] = sd[4 * i + 3]; }
    }
    if (hc) { T* o = static_cast<T*>(hc); for (int i = 0; i < N; ++i) for (int a = 0; a < 2; ++a) for (int c = 0; c < 7; ++c) o[14 * i + c * 2 + a] = vhc[14 * i + a * 7 + c]; }
    if (hf) { T* o = static_cast<T*>(hf); for (int i = 0; i < N; ++i) for (int a = 0; a < 2; ++a) for (int c = 0; c < 6; ++c) o[12 * i + c * 2 + a] = vhf[12 * i + a * 6 + c]; }
    return EKF_OK;
  }

  // ---- dense tile GEMM dispatch -----------------------------------------------------------
  // One launch of the tile GEMM C[rows x cols] = beta C + alpha A op(B); rows, cols multiples of the tile.  tri .. zcol_end
  // and the image triple are GemmArgs' (ekf_dense.hpp); a call site names what it uses, the rest is zero.
  struct GemmCall {
    const T* A = nullptr; int lda = 0;
    const T* B = nullptr; int ldb = 0;
    T* C = nullptr; int ldc = 0;
    int rows = 0, cols = 0, K = 0;
    T alpha = T(1), beta = T(0);
    int tri = TRI_ALL, row_off = 0, col_off = 0, ktri = KTRI_FULL, ktile_off = 0;
    int zrow = 0, zcol_end = 0;
    const int* tile_list = nullptr; int ntiles = 0;     // queued launch: the list, and its work-queue head
    int* counter = nullptr;                             // (UpdateCtx::take_queue(); none left: the plain grid)
    void* img = nullptr; int img_nkc = 0, img_c0 = 0;
    bool two_groups = false;                            // ROLE_SOLVE: two wave groups per workgroup (want_solve_s2)
    bool one_per_cu = false;                            // ROLE_SOLVE, queued: one workgroup per CU (solve_shape)
    const unsigned* chain_word = nullptr; unsigned chain_epoch = 0;   // ROLE_SOLVE: wait for the chain in the kernel (solve_polls_chain)
    hipStream_t st = nullptr;                           // null: the main stream
  };
  // Everything an update decides before its first launch: filled once by plan_update(), a local of update() / shard_update()
  struct Rows { int r0, count; };
  struct UpdatePlan {
    int M = 0, plane = 0;
    int nb = 0, tile = 0, m = 0, m_pad = 0, npad_live = 0, nsteps = 0;
    int nchunks = 1, cend[8] = {};                      // chunk ends in block steps (plan_chunks)
    ChunkTab tab{};                                     // ... in rows
    int strip_rows = 0;                                 // rows of the widest chunk: those of the identity strip under S
    int ntr = 0, ntc = 0;                               // row / column tiles of the solve
    bool oneblock = false, allinone = false, onelaunch = false;   // one diagonal block: see plan_update()
    int small_rc = 0, small_nchunk = 0, small_nt64 = 0; // onelaunch: small_chunking(), and the 64 x 64 lower tiles of Sigma
    bool recompute = false;                             // EKF_OPT_W_RECOMPUTE is in force (both paths: the sequential form)
    // sharded step: own state rows [r0, r1), the tile-padded panel [p0, p0 + prows), and {camera tile, panel, innovation block}
    int r0 = 0, r1 = 0, p0 = 0, prows = 0;
    Rows ranges[3] = {};
    bool sym_panel = false, shard_split = false;
    int c0(int g) const { return (g ? cend[g - 1] : 0) * nb; }
    int c1(int g) const { return cend[g] * nb; }
  };
  // What an update carries from one launch to the next: lives on the stack of update() / shard_update()
  struct UpdateCtx {
    const T* z;                                         // measured pixels and list of this update (device memory)
    const int* midx;
    int* counters;                                      // one work-queue head per queued launch (cleared by the update's first launch)
    int counter_next = 0;
    bool step_fused = false;                            // the chain may take the fused block step (prepare_chain)
    int diag_ahead = -1;                                // block step whose diagonal factor the last k_trail_diag launch has already done
    struct { int step = -1, c0 = 0, c1 = 0; } pending;  // trailing update a chunk left to the next chain_steps call
    bool row_pending = false;                           // sharded, sequential form: the innovation row still waits for its chunk
    bool queue_room(int ints = 8) const { return counter_next + ints <= kQueueCounters; }
    int* take_queue() {
      if (!queue_room()) return nullptr;
      counter_next += 8;
      return counters + counter_next - 8;
    }
  };

  // TM x TN: MFMA tile shape (64 or 128 each); the VALU path always uses 64 x 64.
  template <int ROLE, bool BT, int TM = 128, int TN = 128>
  void gemm(const GemmCall& c) {
    GemmArgs g{};
    g.A = c.A; g.lda = c.lda; g.B = c.B; g.ldb = c.ldb; g.C = c.C; g.ldc = c.ldc;
    g.K = c.K; g.alpha = double(c.alpha); g.beta = double(c.beta);
    g.tri = c.tri; g.row_off = c.row_off; g.col_off = c.col_off; g.ktri = c.ktri; g.ktile_off = c.ktile_off;
    g.zrow = c.zrow; g.zcol_end = c.zcol_end;
    g.stagger = (ROLE == ROLE_DOWNDATE) ? 1 : 0;
    g.img = c.img; g.img_nkc = c.img_nkc; g.img_c0 = c.img_c0;
    g.chain_word = c.chain_word; g.chain_epoch = c.chain_epoch; g.status = d_status;
    hipStream_t st = c.st ? c.st : stream;
    const bool mf = kIsF32 && opt_mfma;
    dim3 grid(c.cols / (mf ? TN : 64), c.rows / (mf ? TM : 64));
    if (c.tile_list && c.counter) {
      g.tile_map = c.tile_list;
      g.ntiles = c.ntiles;
      g.counter = c.counter;
      // persistent grid: two workgroups per CU the stream may use
      const bool side = (st == stream_b);
      int wgs = 2 * (side ? (num_cus - reserved_cus) : num_cus);
      if (ROLE == ROLE_SOLVE && c.one_per_cu) wgs = num_cus;
      grid = dim3(std::min(c.ntiles, wgs), 1);
    }
    if constexpr (kIsF32) {
      if (opt_mfma) {
        if constexpr (ROLE == ROLE_SOLVE) {
          ++launch_cnt[c.two_groups ? EKF_LAUNCH_SOLVE_TWO_GROUPS : EKF_LAUNCH_SOLVE];
          if (c.two_groups) {
            k_gemm_mfma<ROLE, BT, TM, TN, true><<<grid, 512, 0, st>>>(g);
            return;
          }
        }
        k_gemm_mfma<ROLE, BT, TM, TN><<<grid, 256, 0, st>>>(g);
        return;
      }
    }
    if constexpr (!kIsF32) {
      if (opt_mfma) {                            // fp64 matrix pipe, same 64 x 64 tile contract as the VALU kernel
        k_gemm_mfma_f64<ROLE, BT><<<grid, 256, 0, st>>>(g);
        return;
      }
    }
    k_gemm_valu<T, ROLE, BT><<<grid, 256, 0, st>>>(g);
  }

  // Panel of a chain step: P <- P Linv_jj^T in place (vrows rows, block nb).
  void launch_panel(T* P, const T* Dj, int vrows, hipStream_t st) {
    const int nb = NB();
    if constexpr (kIsF32) {
      if (opt_mfma && nb == 128 && opt_panel_direct) {
        k_panel_direct<<<(vrows + 63) / 64, 256, 0, st>>>(P, ldy, Dj, vrows);
        return;
      }
    }
    if constexpr (!kIsF32) {
      if (opt_mfma && nb == 64 && opt_panel_direct) {
        k_panel_direct_f64<<<(vrows + 63) / 64, 256, 0, st>>>(P, ldy, Dj, vrows);
        return;
      }
    }
    GemmCall c;
    c.A = P; c.lda = ldy; c.B = Dj; c.ldb = nb; c.C = P; c.ldc = ldy;
    c.rows = vrows; c.cols = nb; c.K = nb; c.st = st;
    gemm<ROLE_PANEL, false, 64, 128>(c);
  }

  // Work lists for the queued GEMMs: (1) lower-triangular tiles of an nt x nt grid in 8x8
  // super-tiles; (2) the ntr x ntc tiles of the triangular solve, heaviest (largest bj) first.
  int ensure_tilemap(int nt, int ntr, int ntc) {
    const std::vector<int> key = {nt, ntc};
    if (tilemap.current(key)) return EKF_OK;
    std::vector<int> tm;
    const int SB = 8;
    const int ns = (nt + SB - 1) / SB;
    for (int si = 0; si < ns; ++si)
      for (int sj = 0; sj <= si; ++sj)
        for (int i = si * SB; i < std::min(nt, (si + 1) * SB); ++i)
          for (int j = sj * SB; j < std::min(nt, (sj + 1) * SB); ++j)
            if (j <= i) { tm.push_back(i); tm.push_back(j); }
    tri_count = (int)tm.size() / 2;
    solve_off = (int)tm.size();
    for (int j = ntc - 1; j >= 0; --j)
      for (int i = 0; i < ntr; ++i) { tm.push_back(i); tm.push_back(j); }
    solve64_off = (int)tm.size();                  // the same list for 64-row tiles (narrow chunks: more workgroups)
    for (int j = ntc - 1; j >= 0; --j)
      for (int i = 0; i < 2 * ntr; ++i) { tm.push_back(i); tm.push_back(j); }
    solve6464_off = (int)tm.size();                // ... and for 64 x 64 tiles (small maps)
    for (int j = 2 * ntc - 1; j >= 0; --j)
      for (int i = 0; i < 2 * ntr; ++i) { tm.push_back(i); tm.push_back(j); }
    tri64_off = (int)tm.size();                    // lower-triangular 64 x 64 tiles (small maps: 4x the workgroups)
    {
      const int nt64 = 2 * nt, ns64 = (nt64 + SB - 1) / SB;
      for (int si = 0; si < ns64; ++si)
        for (int sj = 0; sj <= si; ++sj)
          for (int i = si * SB; i < std::min(nt64, (si + 1) * SB); ++i)
            for (int j = sj * SB; j < std::min(nt64, (sj + 1) * SB); ++j)
              if (j <= i) { tm.push_back(i); tm.push_back(j); }
      tri64_count = ((int)tm.size() - tri64_off) / 2;
    }
    tri6_off = (int)tm.size();                     // k_syrk_bf16x6: the diagonal tiles first (their element-wise epilogue is the
    for (int i = 0; i < nt; ++i) { tm.push_back(i); tm.push_back(i); }   // longest: not in the tail of the launch), then the rest
    for (int t = 0; t < tri_count; ++t)
      if (tm[2 * t] != tm[2 * t + 1]) { tm.push_back(tm[2 * t]); tm.push_back(tm[2 * t + 1]); }
    trih_off = (int)tm.size();
    {
      const int ns_ = (opt_split_tail < 0) ? std::min(3 * num_cus / 2, tri_count / 3) : std::min(opt_split_tail, tri_count);
      for (int t = 0; t < tri_count - ns_; ++t) { tm.push_back(tm[2 * t]); tm.push_back(tm[2 * t + 1]); }
      for (int t = tri_count - ns_; t < tri_count; ++t)
        for (int h = 0; h < 2; ++h) { tm.push_back((2 * tm[2 * t] + h) | kHalfTile); tm.push_back(tm[2 * t + 1]); }
      trih_count = ((int)tm.size() - trih_off) / 2;
    }
    HIPCHK(hipStreamSynchronize(stream));
    HIPCHK(hipStreamSynchronize(stream_b));
    HIPCHK(tilemap.upload(key, tm));
    return EKF_OK;
  }

  // Chunk ends (in block steps) of the factorisation.  One chunk = the plain algorithm (the strip is the
  // whole inverse); several chunks when the chain is long enough to be worth hiding.
  int plan_chunks(int nsteps, int* cend) const {
    const bool sharded = sh_on;
    const bool pipe = (opt_pipeline < 0) ? (nsteps >= (sharded ? 4 : 8)) : (opt_pipeline != 0);
    // (the sharded step also needs the gather stream; its split by world size below takes chains of one step)
    if (!pipe || !stream_b || (sharded ? !stream_g : nsteps < 2)) { cend[0] = nsteps; return 1; }
    if (env_nchunks > 0 && env_chunks[env_nchunks - 1] == nsteps) {
      for (int g = 0; g < env_nchunks; ++g) cend[g] = env_chunks[g];
      return env_nchunks;
    }
    int want;                                                // chunks of equal width
    if (sharded && (sh_world > 1 || nsteps < 8)) {
      // chunk count by world size: every chunk costs a pass over the remaining columns of W and re-reads the Sigma
      // panel, and a rank's share of that work is 1 / world -- two ranks afford 4 chunks, four and more 8
      // (one rank with >= 8 steps: the plain path's plan, with an earlier first cut)
      const int cap = sh_world <= 1 ? 3 : (sh_world <= 2 ? 4 : 8);
      want = std::min(cap, std::max(2, (nsteps + 1) / 2));
    } else if (opt_pipeline < 2) {
      // default: three chunks ending at 3/16, 7/16 (8/16 through round 3) and 1 of the chain: the first chunk is
      // exposed, so it is short; every further chunk re-reads Sigma once in its downdate, so there are few; the chain and
      // the second stream end together
      // Long chains (>= 32 steps; round 3, tools/knob_ab.py: 32 steps 6/16 -> 4/14: -1 %, 63 steps 12/32 -> 5/25: -2.6 %): the chain
      // is hidden there whatever the plan, so the first two chunks shrink in proportion -- less exposed start-up, and a
      // wider last chunk, whose downdate has every CU
      // round 4 (EKF_OPT_W_RECOMPUTE: no W update, the chain as fast as the second stream): 3 / 7 / 16 -- the last chunk's
      // downdate has every CU and the largest K (tools/knob_ab.py: 1.169 ms against 1.187 with 3 / 8 / 16, 1.216 with 3 / 6)
      // round 5 (EKF_OPT_SPLIT_BF16, the downdate 1.5 x faster): the second stream has slack beside the chain, so one more
      // chunk pays -- the exposed first chunk and the exposed last chunk both get shorter (tools/knob_ab.py, ms per step):
      //   16 steps (N = 1000): 1.063 with 3 / 7 / 16; four chunks: a plateau of 1.01-1.04 over {2, 3} x {5 .. 8} x {10 .. 13} (a sweep of 32
      //   plans), 3 / 7 / 11 / 16 at its low end (1.013-1.018 against 1.026-1.034 for 2 / 6 / 11 / 16); five chunks 1.05-1.11
      //   32 steps (N = 2000): 5.28 with 4 / 13 / 32, 5.05 with 4 / 12 / 22 / 32, 5.09 with five chunks
      //   63 steps (N = 4000): 35.96 with 5 / 25 / 63, 34.97 with 4 / 16 / 36 / 63, 34.27 with 4 / 14 / 30 / 46 / 63
      const bool split = kIsF32 && opt_split_bf16 && opt_mfma;
      if (split && nsteps >= 12) {
        // (the sharded step, whose second stream also carries the gathers in series: 2 / 6 / 11 / 16 -- world 1 with forced
        // collectives 1.305 ms against 1.354 with 3 / 7 / 11 / 16)
        static const double f4p[4] = {3.0 / 16, 7.0 / 16, 11.0 / 16, 1.0}, f4s[4] = {2.0 / 16, 6.0 / 16, 11.0 / 16, 1.0};
        const double* f4 = sharded ? f4s : f4p;
        static const double f4l[4] = {4.0 / 32, 12.0 / 32, 22.0 / 32, 1.0},
                            f5[5] = {4.0 / 63, 14.0 / 63, 30.0 / 63, 46.0 / 63, 1.0};
        const int ng = nsteps >= 48 ? 5 : 4;
        const double* fr = nsteps >= 48 ? f5 : (nsteps >= 32 ? f4l : f4);
        int k = 0, prev = 0;
        for (int g = 0; g < ng; ++g) {
          int e = (g == ng - 1) ? nsteps : (int)(fr[g] * nsteps + 0.5);
          if (e > prev) { cend[k++] = e; prev = e; }
        }
        return k;
      }
      static const int kEnd16[3] = {3, 7, 16};
      int k = 0, prev = 0;
      for (int g = 0; g < 3; ++g) {
        int e = (g == 2) ? nsteps : (nsteps * kEnd16[g] + 8) / 16;
        if (nsteps >= 32 && g == 0) e = 3 + (nsteps - 16) / 16;
        if (nsteps >= 32 && g == 1) e = (int)(2.0 + 0.36 * nsteps + 0.5);
        if (e > prev) { cend[k++] = e; prev = e; }
      }
      return k;
    } else {
      want = std::min(std::min(opt_pipeline, 8), nsteps);
    }
    int k = 0, prev = 0;
    for (int g = 0; g < want; ++g) {
      int e = (int)(((long long)nsteps * (g + 1) + want - 1) / want);
      if (g + 1 == want) e = nsteps;
      if (e > prev) { cend[k++] = e; prev = e; }
    }
    return k;
  }
  // the chunk ends in rows, and the rows of the widest chunk (those of the identity strip under S)
  static ChunkTab chunk_table(const int* cend, int nchunks, int nb, int* strip_rows) {
    ChunkTab tab{nchunks, {}};
    *strip_rows = 0;
    for (int g = 0; g < nchunks; ++g) {
      tab.end[g] = cend[g] * nb;
      *strip_rows = std::max(*strip_rows, (cend[g] - (g ? cend[g - 1] : 0)) * nb);
    }
    return tab;
  }

  // W, S (and nu = zp - h, `with_nu`) for the measured list `ip` (device memory).
  int build_innovation(const T* zp, const int* ip, int M, int plane, bool with_nu, int* m_out, int* m_pad_out,
                       const ChunkTab* tab = nullptr, int strip_rows = 0, bool w_only = false) {
    const int nb = NB();
    const int m = 2 * M + (plane ? 3 : 0);
    const int m_pad = round_up(m, nb);
    const int npad_live = round_up(n, nb);
    T* nu_row = d_W + (size_t)ldy * npad_live;
    // pad rows of W (n..npad_live) and the nu block must be zero; no kernel writes them except row
    // npad_live (nu), so they are cleared only when the layout changed
    if (w_zeroed_n != n) {
      HIPCHK(hipMemsetAsync(d_W + (size_t)n * ldy, 0, (size_t)(npad_live - n + nb) * ldy * sizeof(T), stream));
      w_zeroed_n = n;
    }
    // small problems are latency-bound: fewer rows / features per workgroup so that the grid fills the chip
    const bool small = (size_t)n * m_pad < ((size_t)1 << 22);
    {
      // W = Sigma H^T; with_nu: one more slab of workgroups forms nu = z - h and clears the work-queue heads
      // (k_innovation folded into this launch)
      Scope sc(this, KID_SIGMA_HT);
      const int extra = with_nu ? 1 : 0;
      const T* zq = with_nu ? zp : nullptr;
      T* nuq = with_nu ? nu_row : nullptr;
      // the slab also writes the row bounds of the chunks' features (the mirror rule of the bf16x6 downdate)
      const ChunkTab st = tab ? *tab : ChunkTab{0, {}};
      int* mrows = (with_nu && tab) ? d_counters + kResetInts : nullptr;
      if (small) {
        constexpr int RB = 4;
        dim3 grid((m_pad / 2 + 255) / 256, (n + RB - 1) / RB + extra);
        k_sigma_ht<T, RB><<<grid, 256, 0, stream>>>(S(), ld, n, d_Hc, d_Hf, d_pos, d_coding, ip, M, plane, d_W, ldy,
                                                  m_pad, 0, n, N, zq, d_h, mu(), nuq, d_counters, d_status, d_scr + SCR_QOLD, 0, 0, st, mrows);
      } else if constexpr (kIsF32) {
        // 128 slots x 8 rows per workgroup, the row segments staged through LDS (runs of neighbouring inverse-depth
        // features; other stretches of the list take k_sigma_ht's path inside the same launch): bit-identical sums
        constexpr int RB = 8;
        dim3 grid((m_pad / 2 + 127) / 128, (n + RB - 1) / RB + extra);
        k_sigma_ht_fast<RB><<<grid, 256, 0, stream>>>(S(), ld, n, d_Hc, d_Hf, d_pos, d_coding, ip, M, plane, d_W, ldy, m_pad, N,
                                                      0, 0, zq, d_h, mu(), nuq, d_counters, d_status, d_scr + SCR_QOLD, 0, st, mrows);
      } else {
        constexpr int RB = 32;
        dim3 grid((m_pad / 2 + 255) / 256, (n + RB - 1) / RB + extra);
        k_sigma_ht<T, RB><<<grid, 256, 0, stream>>>(S(), ld, n, d_Hc, d_Hf, d_pos, d_coding, ip, M, plane, d_W, ldy,
                                                  m_pad, 0, n, N, zq, d_h, mu(), nuq, d_counters, d_status, d_scr + SCR_QOLD, 0, 0, st, mrows);
      }
    }
    if (!w_only) {                      // (the 1-point RANSAC reads W only)
      Scope sc(this, KID_INNOVATION_COV);
      T* zid = tab ? d_Y + (size_t)m_pad * ldy : nullptr;
      const ChunkTab ct = tab ? *tab : ChunkTab{0, {}};
      if (small) {
        constexpr int KB = 1;
        dim3 grid((m_pad + 255) / 256, std::max(1, (M + KB - 1) / KB) + (m_pad - 2 * M + 7) / 8);
        k_innovation_cov<T, KB><<<grid, 256, 0, stream>>>(d_W, ldy, d_Hc, d_Hf, d_pos, d_coding, ip, M, plane,
                                                        T(sigma_pixel_2), T(0.00001), d_Y, m_pad, 0, M, zid, N, ct, strip_rows);
      } else {
        constexpr int KB = 8;
        dim3 grid((m_pad + 255) / 256, std::max(1, (M + KB - 1) / KB) + (m_pad - 2 * M + 7) / 8);
        k_innovation_cov<T, KB><<<grid, 256, 0, stream>>>(d_W, ldy, d_Hc, d_Hf, d_pos, d_coding, ip, M, plane,
                                                        T(sigma_pixel_2), T(0.00001), d_Y, m_pad, 0, M, zid, N, ct, strip_rows);
      }
    }
    HIPCHK(hipGetLastError());
    if (m_out) *m_out = m;
    if (m_pad_out) *m_pad_out = m_pad;
    return EKF_OK;
  }

  // ---- trailing update of step j + diagonal factor of step j + 1 as one launch (k_trail_diag) ---------------------------
  bool trail_diag_ok() const {
    return kIsF32 && opt_mfma && opt_chain_fused_diag && (size_t)2 * ldy * ldy * sizeof(T) < ((size_t)1 << 31);
  }
  // per block step j of the chunk plan: the 128 x 128 blocks of its trailing update except (j + 1, j + 1) -- the S blocks
  // (I >= K > j) and the strip blocks of the step's chunk (row blocks nblk + t, t <= j - s0, columns K in (j, s1))
  int ensure_trail_diag_lists(int nblk, int nchunks, const int* cend) {
    std::vector<int> key = {nblk, nchunks};
    key.insert(key.end(), cend, cend + nchunks);
    if (td_blocks.current(key)) return EKF_OK;
    std::vector<int> all;
    td_off.assign(nblk, 0);
    td_cnt.assign(nblk, 0);
    for (int g = 0; g < nchunks; ++g) {
      const int s0 = g ? cend[g - 1] : 0, s1 = cend[g];
      for (int j = s0; j < s1; ++j) {
        td_off[j] = (int)all.size();
        for (int K = j + 1; K < nblk; ++K) {
          for (int I = K; I < nblk; ++I) {
            if (I == j + 1) continue;                                   // (j + 1, j + 1): workgroup 0's
            all.push_back(I); all.push_back(K);
          }
          if (K < s1)
            for (int t = 0; t <= j - s0; ++t) { all.push_back(nblk + t); all.push_back(K); }
        }
        td_cnt[j] = ((int)all.size() - td_off[j]) / 2;
      }
    }
    HIPCHK(hipStreamSynchronize(stream));
    if (stream_b) HIPCHK(hipStreamSynchronize(stream_b));
    HIPCHK(td_blocks.upload(key, all, 2));
    return EKF_OK;
  }
  // true: launched (and the factor of step + 1 is done); false: this step keeps the separate launches
  bool launch_trail_diag(UpdateCtx& ux, int step, int m, hipStream_t sc_) {
    if constexpr (kIsF32) {
      const int td_nblk = td_blocks.first();               // (0: no lists, or those of another plan -- prepare_chain)
      if (!trail_diag_ok() || NB() != 128 || td_nblk == 0 || step + 1 >= td_nblk || td_cnt[step] < td_min_blocks ||
          td_cnt[step] > td_max_blocks)
        return false;
      TrailDiagArgs a{};
      a.Y = d_Y; a.ldy = ldy; a.y_bytes = (unsigned)((size_t)2 * ldy * ldy * sizeof(T));
      a.Dinv = d_Dinv; a.dinv_bytes = (unsigned)((size_t)(ldy / 64) * 128 * 128 * sizeof(T));
      a.status = d_status; a.m = m; a.j = step;
      a.blocks = td_blocks.d + td_off[step]; a.nblocks = td_cnt[step]; a.do_diag = 1;
      Scope sc(this, KID_CHOL_TRAILING, sc_);
      ++launch_cnt[EKF_LAUNCH_CHAIN_TRAIL_DIAG];
      k_trail_diag<<<a.nblocks + 1, 1024, kChainLds, sc_>>>(a);
      ux.diag_ahead = step + 1;
      return true;
    }
    return false;
  }

  // Block steps [step0, step1) of the serial chain of chunk [c0, c1) on stream sc_: diagonal factor, panel (rows
  // below the block + the chunk's identity-strip rows), trailing update (strip tiles stop at c1).
  // `defer_last`: the trailing update of the chunk's LAST step is left to the next call (it only touches columns >= c1, so
  // the chunk -- its columns of L and its strip -- is complete without it, and the caller records the chunk's event one
  // launch earlier: the second stream starts on the chunk while this update is still running)
  // ---- a whole block step as one launch (ekf_step.hpp): the work lists of a ONE-chunk plan of nblk steps -------------------
  int ensure_step_fused_lists(int nblk) {
    const std::vector<int> key = {nblk};
    if (sf_lists.current(key)) return EKF_OK;
    std::vector<int> all;
    sfp.off.assign(nblk, 0);
    sfp.cnt.assign(nblk, 0);
    const int s0 = 0, s1 = nblk;
    for (int j = 0; j < nblk; ++j) {
      sfp.off[j] = (int)all.size();
      const int first = 2 * (j + 1);                        // first 64-row / 64-column block of the trailing matrix
      for (int r = first; r < 2 * nblk; ++r)                // S rows below the diagonal block: lower tiles, the diagonal one writes the panel rows
        for (int c = first; c <= r; ++c) { all.push_back(r); all.push_back(c); all.push_back(SF_TILE | (c == r ? SF_WRITE_PANEL : 0)); }
      for (int r = 2 * nblk; r < 2 * nblk + 2 * (j + 1 - s0); ++r) {   // the strip rows of the chunk: columns up to its end
        if (first < 2 * s1) {
          for (int c = first; c < 2 * s1; ++c) { all.push_back(r); all.push_back(c); all.push_back(SF_TILE | (c == first ? SF_WRITE_PANEL : 0)); }
        } else {
          all.push_back(r); all.push_back(r); all.push_back(SF_WRITE_PANEL);           // no tile: the panel rows only
        }
      }
      sfp.cnt[j] = ((int)all.size() - sfp.off[j]) / 3;
      all[sfp.off[j] + 2] |= SF_WRITE_DIAG;                 // (a step always has a workgroup: the strip rows)
    }
    HIPCHK(hipStreamSynchronize(stream));
    HIPCHK(sf_lists.upload(key, all));
    return EKF_OK;
  }
  bool launch_step_fused(const UpdateCtx& ux, int step, int m, hipStream_t sc_) {
    if constexpr (kIsF32) {
      if (!ux.step_fused || step >= sf_lists.first() || sfp.cnt[step] > num_cus / 2 || sc_ != stream) return false;   // (every workgroup resident, with room to spare)
      StepFusedArgs a{};
      a.Y = d_Y; a.ldy = ldy; a.Dj = d_Dinv + (size_t)step * 128 * 128; a.status = d_status; a.m = m; a.j = step;
      a.wl = sf_lists.d + sfp.off[step]; a.nwg = sfp.cnt[step];
      a.gate = reinterpret_cast<unsigned*>(d_status + 9);
      small_gate_total += (unsigned)a.nwg;
      a.gate_target = small_gate_total;
      Scope sc(this, KID_CHOL_TRAILING, sc_);
      ++launch_cnt[EKF_LAUNCH_CHAIN_STEP_FUSED];
      k_chain_step_fused<<<a.nwg, 1024, 0, sc_>>>(a);
      return true;
    }
    return false;
  }
  void chain_trailing(UpdateCtx& ux, int step, int c0, int c1, int m, int m_pad, hipStream_t sc_, bool allow_fused) {
    const int nb = NB();
    T* Y = d_Y;
    const int j = step * nb, r0 = j + nb;
    const int vrows = m_pad - c0, tcols = m_pad - r0;
    if (r0 >= m_pad || tcols <= 0) return;
    if (allow_fused && launch_trail_diag(ux, step, m, sc_)) return;       // the update of this step and the factor of the next one as one launch
    Scope sc(this, KID_CHOL_TRAILING, sc_);                            // Y[r0.., r0:] -= P P_S^T; strip rows stop at c1
    const T* P = Y + (size_t)r0 * ldy + j;
    T* C = Y + (size_t)r0 * ldy + r0;
    ++launch_cnt[EKF_LAUNCH_CHAIN_STEP];
    GemmCall g;
    g.A = P; g.lda = ldy; g.B = P; g.ldb = ldy; g.C = C; g.ldc = ldy;
    g.rows = vrows; g.cols = tcols; g.K = nb; g.alpha = T(-1); g.beta = T(1);
    g.tri = TRI_LOWER; g.row_off = r0; g.col_off = r0; g.zrow = m_pad; g.zcol_end = c1; g.st = sc_;
    gemm<ROLE_TRAILING, false, 64, 64>(g);
  }
  void chain_steps(UpdateCtx& ux, int step0, int step1, int c0, int c1, int m, int m_pad, hipStream_t sc_,
                   bool skip_panel = false, bool defer_last = false) {
    const int nb = NB();
    T* Y = d_Y;
    if (ux.pending.step >= 0) {
      chain_trailing(ux, ux.pending.step, ux.pending.c0, ux.pending.c1, m, m_pad, sc_, true);
      ux.pending.step = -1;
    }
    for (int step = step0; step < step1; ++step) {
      if (!skip_panel && !defer_last && ux.diag_ahead != step && launch_step_fused(ux, step, m, sc_)) continue;
      const int j = step * nb;
      T* Ajj = Y + (size_t)j * ldy + j;
      T* Dj = d_Dinv + (size_t)step * nb * nb;
      if (ux.diag_ahead != step) {
        Scope sc(this, KID_CHOL_DIAG, sc_);
        ++launch_cnt[EKF_LAUNCH_CHAIN_STEP];
        if (nb == 128) {
          if constexpr (kIsF32)
            k_chol_diag_packed<><<<1, 1024, 0, sc_>>>(Ajj, ldy, Dj, d_status, std::max(1, std::min(8, (m - j + 15) / 16)));
        } else {
          if constexpr (!kIsF32) {
            if (opt_mfma)
              k_chol_diag_packed_f64<<<1, 512, 0, sc_>>>(Ajj, ldy, Dj, d_status, std::max(1, std::min(4, (m - j + 15) / 16)));
            else
              k_chol_diag<T, 64><<<1, 512, diag_lds(64), sc_>>>(Ajj, ldy, Dj, d_status);
          } else {
            k_chol_diag<T, 64><<<1, 512, diag_lds(64), sc_>>>(Ajj, ldy, Dj, d_status);
          }
        }
      }
      // rows that change at this step: S rows below the diagonal block, then strip rows [0, r0 - c0)
      // (Z rows c0..r0 of this chunk): contiguous, m_pad - c0 of them starting at row r0
      const int r0 = j + nb;
      const int vrows = m_pad - c0;
      if (!skip_panel) {
        Scope sc(this, KID_CHOL_PANEL, sc_);                 // P = Y[r0.., j:j+nb] * Linv_jj^T, in place
        T* P = Y + (size_t)r0 * ldy + j;
        ++launch_cnt[EKF_LAUNCH_CHAIN_STEP];
        launch_panel(P, Dj, vrows, sc_);
      }
      if (defer_last && step == step1 - 1 && r0 < m_pad) {
        ux.pending.step = step; ux.pending.c0 = c0; ux.pending.c1 = c1;
      } else {
        chain_trailing(ux, step, c0, c1, m, m_pad, sc_, !skip_panel);
      }
    }
  }
  // ---- checks and launch steps shared by the plain and the sharded step ------------------
  // A measured list from the caller: every index in [0, N), and strictly ascending if `ascending`
  int check_list(const int* idx, int M, bool ascending) {
    for (int k = 0; k < M; ++k) {
      if (idx[k] < 0 || idx[k] >= N) FAIL(EKF_ERR_ARG, "feature index out of range");
      if (ascending && k > 0 && idx[k - 1] >= idx[k]) FAIL(EKF_ERR_ARG, "measured indices must be strictly ascending");
    }
    return EKF_OK;
  }

  // Only the innovation row (row npad_live of [W; nu^T]) updated right-looking for chunk [c0, c1):
  // nu^T[c1:] -= y_g^T L[c1:, g]^T, by k_innov_row_update (`gemv`) or the 64 x 128 tile GEMM
  void launch_row_update(int c0, int c1, int m_pad, hipStream_t ss, bool gemv) {
    const size_t yrow = (size_t)round_up(n, NB()) * ldy;
    Scope sc(this, KID_WUPDATE, ss);
    ++launch_cnt[gemv ? EKF_LAUNCH_ROW_GEMV : EKF_LAUNCH_ROW_TILE_GEMM];
    if constexpr (kIsF32) {
      if (gemv) {
        k_innov_row_update<<<(m_pad - c1 + 63) / 64, 64, 0, ss>>>(d_V + yrow + c0, d_Y + (size_t)c1 * ldy + c0, ldy,
                                                                  d_W + yrow + c1, m_pad - c1, c1 - c0);
        return;
      }
    }
    GemmCall g;
    g.A = d_V + yrow + c0; g.lda = ldy; g.B = d_Y + (size_t)c1 * ldy + c0; g.ldb = ldy; g.C = d_W + yrow + c1; g.ldc = ldy;
    g.rows = NB(); g.cols = m_pad - c1; g.K = c1 - c0; g.alpha = T(-1); g.beta = T(1); g.st = ss;
    gemm<ROLE_WUPDATE, false, 64, 128>(g);
  }

  // EKF_OPT_SPLIT_BF16: Sigma -= V_g V_g^T for chunk [c0, c1) on the bf16 matrix pipe at fp32 accuracy (ekf_syrk6.hpp), over
  // the `ntiles` canonical tiles of `tiles` (none: the image only).  `split`: V_g is split into the plane image first (three
  // bf16 per fp32, one 12 KB record per 128 rows x 16 columns; else the solve's tiles have written it).  Rows of Sigma valid
  // here: [0, cam_rows) and [r0, r1).  `mirror_rows`: Syrk6Args::mirror_rows (the plain step's launches before the last).  `work`: the flop the launch adds to prof.work.  `rider`: the innovation row update of
  // the chunk in the same launch (launch_row_update's sums); `su_tail`: the state update too (the last downdate of an update).
  int launch_downdate_bf16x6(UpdateCtx& ux, int c0, int c1, int m_pad, hipStream_t ss, bool split, const int* tiles, int ntiles, int cam_rows,
                             int r0, int r1, double work, bool rider, bool su_tail, const int* mirror_rows = nullptr) {
    if constexpr (kIsF32) {
      const int npad_live = round_up(n, NB()), width = c1 - c0;
      HIPCHK(ensure_vimg());
      if (split) {
        Scope sc(this, KID_MISC, ss);
        dim3 grid(npad_live / 128, width / 16);
        k_split_image<<<grid, 256, 0, ss>>>(d_V, ldy, npad_live, c0, width, d_Vimg, ldy / 16);
      }
      if (ntiles == 0) return EKF_OK;
      Scope sc(this, KID_DOWNDATE, ss);
      if (sc.on) prof.work[KID_DOWNDATE] += work;
      int* head = ux.take_queue();                        // (the callers have checked queue_room())
      Syrk6Args a{d_Vimg, ldy / 16, c0 / 16, width / 16, S(), ld, tiles, ntiles, head, cam_rows, r0, r1};
      a.stag_half = opt_syrk_stag_half; a.stag_mod4 = opt_syrk_stag_mod4;
      if (su_tail) {
        a.su_mu = mu(); a.su_V = d_V; a.su_ldy = ldy; a.su_n = n; a.su_y = d_V + (size_t)npad_live * ldy; a.su_mpad = m_pad;
        a.su_qn = d_scr + SCR_QN; a.su_counter = head + 1;
        ++launch_cnt[EKF_LAUNCH_STATE_UPDATE_TAIL];
      }
      if (rider) {
        a.ry = d_V + (size_t)npad_live * ldy + c0; a.rL = d_Y + (size_t)c1 * ldy + c0; a.rldl = ldy;
        a.rnu = d_W + (size_t)npad_live * ldy + c1; a.rcols = m_pad - c1; a.rK = width; a.nrider = (m_pad - c1 + 255) / 256;
        ++launch_cnt[EKF_LAUNCH_ROW_RIDER];
      }
      if (mirror_rows) {
        a.mirror_rows = mirror_rows;
        ++launch_cnt[EKF_LAUNCH_DOWNDATE_MIRROR_BOUNDS];
      }
      ++launch_cnt[EKF_LAUNCH_DOWNDATE_BF16X6];
      const int wgs = 2 * (ss == stream_b ? num_cus - reserved_cus : num_cus);
      k_syrk_bf16x6<0><<<a.nrider + std::min(ntiles, wgs), 256, 0, ss>>>(a);
    }
    return EKF_OK;
  }

  // EKF_OPT_W_RECOMPUTE: W[rows, c1:c2) = Sigma' H^T, the columns of the next chunk from the downdated Sigma, for rows
  // [0, rows0) and [row0, row1)
  void launch_w_recompute(int c1, int c2, int m_pad, const int* list, int M, int plane, hipStream_t ss, int rows0,
                          int row0 = 0, int row1 = 0) {
    if constexpr (kIsF32) {
      Scope sc(this, KID_SIGMA_HT, ss);
      ++launch_cnt[EKF_LAUNCH_W_RECOMPUTE];
      const int s0 = c1 / 2, s1 = c2 / 2;
      const int range[2][2] = {{0, rows0}, {row0, row1}};
      for (const auto& r : range) {
        if (r[1] <= r[0]) continue;
        constexpr int RB = 8;
        dim3 grid((s1 - s0 + 127) / 128, (r[1] - r[0] + RB - 1) / RB);
        k_sigma_ht_fast<RB><<<grid, 256, 0, ss>>>(S(), ld, r[1], d_Hc, d_Hf, d_pos, d_coding, list, M, plane, d_W, ldy, m_pad, N,
                                                   s0, s1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, r[0]);
      }
    }
  }

  // mu += V y with the quaternion normalisation, on stream st
  void launch_state_update(int m_pad, hipStream_t st) {
    Scope sc(this, KID_STATE_UPDATE, st);
    k_state_update<T><<<(n + 7) / 8, 512, 0, st>>>(mu(), d_V, ldy, n, d_V + (size_t)round_up(n, NB()) * ldy, m_pad, d_scr + SCR_QN);
  }

  // End of an update on the main stream: the state update (`state_update`), the normalisation congruence of Sigma
  // (`normalize`), and the record of what the update did
  int finish_update(const UpdatePlan& p, bool state_update, bool normalize) {
    last_nchunks = p.nchunks;
    last_recompute = p.recompute;
    for (int g = 0; g < p.nchunks; ++g) last_cend[g] = p.cend[g];
    if (state_update) launch_state_update(p.m_pad, stream);
    if (normalize) {
      Scope sc(this, KID_NORMALIZE);
      k_strip_congruence<T, 4><<<(2 * n + 255) / 256, 256, 0, stream>>>(S(), ld, n, 3, d_scr + SCR_QN,
                                                                       static_cast<const T*>(nullptr));
    }
    HIPCHK(hipGetLastError());
    last_m = p.m; last_m_pad = p.m_pad; last_n = n;
    have_update = true;
    have_meas = false;                                    // h/H belong to the pre-update state
    ++prof.frame_seq;
    return EKF_OK;
  }

  // ---- the plan of an update --------------------------------------------------------------
  // Everything the update of M measured features (+ the plane rows) decides before its first launch, for the plain and
  // the sharded step alike.
  UpdatePlan plan_update(int M, int plane) const {
    UpdatePlan p;
    p.M = M; p.plane = plane;
    p.nb = NB();
    p.tile = (kIsF32 && opt_mfma) ? 128 : 64;
    p.m = 2 * M + (plane ? 3 : 0);
    p.m_pad = round_up(p.m, p.nb);
    p.npad_live = round_up(n, p.nb);
    p.nsteps = p.m_pad / p.nb;
    p.nchunks = plan_chunks(p.nsteps, p.cend);
    p.tab = chunk_table(p.cend, p.nchunks, p.nb, &p.strip_rows);
    p.ntr = (p.npad_live + p.nb) / p.tile;
    p.ntc = p.m_pad / p.tile;
    // EKF_OPT_W_RECOMPUTE (fp32 MFMA path, several chunks): the W columns of chunk g + 1 come from the downdated Sigma
    // instead of the right-looking GEMM update (see the option's comment in ekf_monoslam.h)
    p.recompute = kIsF32 && opt_mfma && opt_wrecompute && p.nchunks > 1;
    if (sh_on) {
      // own state rows, and the tile-padded panel [p0, p0 + prows) the tile GEMMs run on: it covers the own rows and,
      // at its ends, a few foreign ones (whose results nobody reads and the next gather overwrites); it never reaches
      // past the padded live block (row npad_live of W / V is the nu / y row)
      p.r0 = row_of_feature(own_f0()); p.r1 = row_of_feature(own_f1());
      // (round 3: the panel starts on a tile boundary, so that the tiles that lie INSIDE the own rows on both sides -- the
      // own x own block of Sigma minus its ragged ends -- are computed once, as lower tiles, and mirrored: both rows of a
      // mirrored pair are then owned.  Per rank the downdate is rows x m x (2 n - rows) flop instead of 2 rows n m.)
      if (p.r1 > p.r0) {
        p.p0 = p.r0 / p.nb * p.nb;
        p.prows = round_up(p.r1, p.nb) - p.p0;
      }
      p.ranges[0] = {0, p.p0 > 0 || p.prows == 0 ? p.nb : 0};
      p.ranges[1] = {p.p0, p.prows};
      p.ranges[2] = {p.npad_live, p.nb};
      p.sym_panel = kIsF32 && opt_mfma && p.nb == 128 && p.prows > 0 && opt_shard_sym;
      // (the plain path's rule: the lower tiles of the WHOLE matrix fill the chip)
      p.shard_split = kIsF32 && opt_split_bf16 && opt_mfma && p.nb == 128 &&
                      (p.npad_live / 128) * (p.npad_live / 128 + 1) / 2 >= num_cus;
      return p;
    }
    if constexpr (kIsF32) {
      // One diagonal block (2 M + 3 <= 128, the reference's operating point): the chunk inverse is the transposed
      // Linv of the diagonal factor, so the panel launch, the solve and the state update are ONE launch
      // (k_solve_state_oneblock; small maps: the downdate and the normalisation too, k_update_oneblock_small): the step is
      // launch-bound there.
      p.oneblock = opt_fused && opt_mfma && p.nchunks == 1 && p.m_pad == 128 && p.nb == 128 && !prof.on(KID_SOLVE) &&
                   !prof.on(KID_STATE_UPDATE) && !prof.on(KID_CHOL_PANEL);
      // small map: downdate and normalisation congruence in the same launch, one 64 x 64 tile of Sigma per workgroup
      p.small_nt64 = (p.npad_live / 64) * (p.npad_live / 64 + 1) / 2;
      p.allinone = p.oneblock && p.small_nt64 <= num_cus && !prof.on(KID_DOWNDATE) && !prof.on(KID_NORMALIZE);
      // Small map (n_pad <= 256: the reference's 20-35 features): W, S, the factor, the solve, the state update, the downdate
      // and the normalisation as ONE launch (ekf_small.hpp) -- every workgroup forms W, S and the factor for itself
      p.onelaunch = p.oneblock && opt_small_onelaunch && p.npad_live <= kSmallMaxRows && p.small_nt64 <= num_cus && ld % 4 == 0 &&
                    small_chunking(n, round_up(p.m, 4), &p.small_rc, &p.small_nchunk) && M <= 62 && !prof.on(KID_SIGMA_HT) &&
                    !prof.on(KID_INNOVATION_COV) && !prof.on(KID_CHOL_DIAG) && !prof.on(KID_DOWNDATE) && !prof.on(KID_NORMALIZE);
      p.allinone = p.allinone || p.onelaunch;
    }
    return p;
  }
  // The chain's cached work lists for this plan: the blocks of k_trail_diag, and for a one-chunk plan of the plain step
  // those of the fused block step (`dist`: the distributed chain of the sharded step has lists of its own)
  int prepare_chain(const UpdatePlan& p, UpdateCtx& ux, bool dist) {
    if (td_blocks.first() != p.nsteps) td_blocks.key.clear();   // lists of another plan: launch_trail_diag must not take them
    if (!p.oneblock && !dist && trail_diag_ok() && p.nb == 128 && p.nsteps >= 2) {
      int rc = ensure_trail_diag_lists(p.nsteps, p.nchunks, p.cend);
      if (rc) return rc;
    }
    if constexpr (kIsF32) {                                // (the fused block step is the plain path's)
      if (!sh_on && opt_step_fused && opt_mfma && opt_fused && p.nb == 128 && p.nchunks == 1 && !p.oneblock &&
          !prof.on(KID_CHOL_DIAG) && !prof.on(KID_CHOL_PANEL) && !prof.on(KID_CHOL_TRAILING)) {
        int rc = ensure_step_fused_lists(p.nsteps);
        if (rc) return rc;
        ux.step_fused = true;
      }
    }
    return EKF_OK;
  }

  // ---- what chunk g of the plain step does (each rule once; `ux`: the work-queue heads still free) -------------------
  // the last chunk has nothing left to overlap with: it runs on the main stream, on every CU
  bool chunk_overlaps(const UpdatePlan& p, int g) const { return stream_b != nullptr && g + 1 < p.nchunks; }
  // workgroups of a persistent grid on the chunk's stream: two per CU the stream may use
  int chunk_slots(const UpdatePlan& p, int g) const { return 2 * (chunk_overlaps(p, g) ? num_cus - reserved_cus : num_cus); }
  // the downdate on the bf16 matrix pipe (EKF_OPT_SPLIT_BF16): the 128 x 128 lower tiles of Sigma fill the chip
  bool chunk_splits(const UpdatePlan& p, const UpdateCtx& ux) const {
    return kIsF32 && opt_split_bf16 && opt_mfma && p.tile == 128 && tri_count >= num_cus && ux.queue_room();
  }
  // W update and downdate of an overlapped chunk go out as ONE queued launch when both run on 128 x 128 tiles:
  // they read the same V_g, and sharing a launch saves one ramp and one partially filled last round.  Not for
  // the chunk before the last: the last solve starts on that chunk's W update, not on its downdate.
  bool chunk_fuses(const UpdatePlan& p, int g, const UpdateCtx& ux) const {
    return kIsF32 && opt_fuse_wu && (opt_fuse_wu > 1 || p.recompute || g + 2 < p.nchunks) && opt_mfma && chunk_overlaps(p, g) &&
           p.c1(g) < p.m_pad && !opt_split_bf16 && p.tile == 128 && tri_count >= num_cus && ux.queue_room();
  }
  // the innovation row update rides in the chunk's k_syrk_bf16x6 launch
  bool chunk_row_rider(const UpdatePlan& p, int g, const UpdateCtx& ux) const {
    return chunk_splits(p, ux) && p.recompute && opt_row_gemv && p.c1(g) < p.m_pad && !chunk_fuses(p, g, ux);
  }
  // (round 6: when the last downdate is the bf16x6 kernel, its workgroups take the state update's rows when they run out of
  // tiles -- Syrk6Args::su_*: no launch, no second stream, no events at the end of the step)
  bool chunk_su_tail(const UpdatePlan& p, int g, const UpdateCtx& ux) const {
    return kIsF32 && opt_su_tail && !chunk_overlaps(p, g) && p.nchunks > 1 && chunk_splits(p, ux);
  }
  // The overlapped solve waits for the chain inside the kernel, not behind a stream wait (EKF_SOLVE_POLL_CHAIN): a cross-stream
  // wait costs the second stream 6-12 us even when its event fired long ago (profiles/r6_step_timeline.txt), a poll of a word
  // that is already there a fraction of one.  Only where a spinning solve cannot hold what the chain needs: the second stream
  // is masked off the reserved CUs and the chain always finds those.  Not chunk 0 -- its chain has the whole chip, workgroups
  // that sit on the second stream's CUs for its 150 us would confine it to the reserved ones, and its stream wait is also what
  // orders the second stream behind the reset of the queue heads and of the epoch word.  Not the last chunk -- its solve runs
  // on every CU, where spinning workgroups could keep the producer's from being placed: it keeps its event wait.
  // Only plans of at most 16 block steps (N <= 1000), by measurement (profiles/r7_solve_poll_chain_ab.txt): 16 steps 0.865 ->
  // 0.853 ms per step with the poll, 10 steps 0.482 = 0.482, 32 steps (N = 2000) 4.66 -> 4.82.  The likely cause of that loss:
  // a solve that really has to wait sits on the second stream's CUs meanwhile, and k_trail_diag (one workgroup per CU, 141 KB
  // of LDS) fits on none of them, so a chain that is BEHIND stays confined to the reserved CUs where it would have had the
  // idle chip.  EKF_SOLVE_POLL_CHAIN=2
  // polls at any size (A/B runs).
  bool solve_polls_chain(const UpdatePlan& p, int g) const {
    return kIsF32 && opt_mfma && opt_solve_poll_chain && (p.nsteps <= 16 || opt_solve_poll_chain > 1) && g > 0 &&
           chunk_overlaps(p, g) && stream_b_masked && reserved_cus > 0 && !p.oneblock;
  }
  enum SolveShape { SOLVE_64X64, SOLVE_128_ONE_PER_CU, SOLVE_64X128, SOLVE_128 };
  SolveShape solve_shape(const UpdatePlan& p, int g) const {
    const bool mf = kIsF32 && opt_mfma;
    const int tiles = (p.c1(g) - p.c0(g)) / p.tile * p.ntr, slots = chunk_slots(p, g);
    if (mf && 4 * tiles < slots) return SOLVE_64X64;      // small map: 64 x 64 tiles
    // the last chunk's solve, alone on the chip, between one and two tiles of 128 x 128 per CU (N = 1000: 432 tiles with
    // K = 128 .. 1152): ONE workgroup per CU drawing the tiles heaviest-first -- a workgroup that has its CU to itself
    // runs a K step in 2.0 us against 3.2 us beside a second one, and with at most two per CU the heaviest tile bounds
    // the launch either way; the light tiles then fill the CUs that finish first.  96 -> 86 us, bit-identical
    // (round 4; 128 x 128 tiles on two workgroups per CU: 1.203 ms per step, 64 x 128 tiles: 1.149, this: 1.142)
    if (mf && !chunk_overlaps(p, g) && opt_solve_one_per_cu && tiles < slots && tiles > num_cus) return SOLVE_128_ONE_PER_CU;
    if (mf && tiles < slots) return SOLVE_64X128;          // narrow chunk: 64-row tiles fill the chip
    return SOLVE_128;
  }

  // ---- the launches of the plain step, phase by phase --------------------------------------
  // The whole update of a small map as ONE launch (plan: onelaunch)
  int launch_update_small(const UpdatePlan& p, const UpdateCtx& ux) {
    if constexpr (kIsF32) {
      if (w_zeroed_n != n) {              // (what build_innovation keeps: pad rows of W and the rows behind nu are zero)
        HIPCHK(hipMemsetAsync(d_W + (size_t)n * ldy, 0, (size_t)(p.npad_live - n + p.nb) * ldy * sizeof(T), stream));
        w_zeroed_n = n;
      }
      SmallUpdateArgs a{};
      a.S = S(); a.ld = ld; a.n = n; a.npad = p.npad_live;
      a.Hc = d_Hc; a.Hf = d_Hf; a.pos = d_pos; a.coding = d_coding; a.midx = ux.midx;
      a.M = p.M; a.plane = p.plane; a.nfeat = N;
      a.z = ux.z; a.h = d_h; a.mu = mu();
      a.r_pix = T(sigma_pixel_2); a.r_plane = T(0.00001);
      a.W = d_W; a.ldw = ldy; a.Y = d_Y; a.ldy = ldy; a.Dinv = d_Dinv; a.V = d_V; a.ldv = ldy;
      a.scr_qn = d_scr + SCR_QN; a.status = d_status;
      a.gate = reinterpret_cast<unsigned*>(d_status + 9);
      small_gate_total += (unsigned)(p.small_nt64 + 1);
      a.gate_target = small_gate_total;
      a.ntiles = p.small_nt64; a.wp = round_up(p.m, 4); a.stamps = d_small_stamps;
      a.rc = p.small_rc; a.nchunk = p.small_nchunk;
      ++launch_cnt[EKF_LAUNCH_UPDATE_ONELAUNCH];
      k_update_small_onelaunch<<<p.small_nt64 + 1, 1024, 0, stream>>>(a);
    }
    return EKF_OK;
  }

  // The solve V_g = [W_g; nu_g^T] Z_gg of chunk gi on stream ss (one block: with everything behind it, see plan_update).
  // *vimg_done: the tiles have written the plane image of V_g the bf16x6 downdate reads
  int solve_chunk(const UpdatePlan& p, int gi, UpdateCtx& ux, hipStream_t ss, bool* vimg_done) {
    const int c0 = p.c0(gi), width = p.c1(gi) - c0, ntr = p.ntr, ntc = p.ntc;
    T* Zs = d_Y + (size_t)p.m_pad * ldy;                   // the strip
    if (p.oneblock) {
      if constexpr (kIsF32) {
        ++launch_cnt[p.allinone ? EKF_LAUNCH_UPDATE_ALLINONE : EKF_LAUNCH_UPDATE_ONEBLOCK];
        if (p.allinone)
          k_update_oneblock_small<<<p.small_nt64 + 1, 512, 0, ss>>>(d_W, ldy, d_Dinv, d_V, ldy, p.npad_live, mu(), n, d_scr + SCR_QOLD,
                                                                   d_scr + SCR_QN, Zs, ldy, S(), ld, p.small_nt64);
        else
          k_solve_state_oneblock<<<p.npad_live / 64 + 1, 256, 0, ss>>>(d_W, ldy, d_Dinv, d_V, ldy, p.npad_live, mu(), n,
                                                                      d_scr + SCR_QN, Zs, ldy);
      }
      return EKF_OK;
    }
    Scope sc(this, KID_SOLVE, ss);                        // column tiles of the chunk, heaviest first
    const int wt = width / p.tile;
    GemmCall c;
    c.A = d_W + c0; c.lda = ldy; c.B = Zs + c0; c.ldb = ldy; c.C = d_V + c0; c.ldc = ldy;
    c.rows = p.npad_live + p.nb; c.cols = width; c.K = width; c.ktri = KTRI_UPPER;
    c.two_groups = want_solve_s2(width, p.npad_live);
    c.st = ss;
    if (ss == stream_b && solve_polls_chain(p, gi)) {
      c.chain_word = reinterpret_cast<const unsigned*>(d_counters + kChainEpochWord); c.chain_epoch = (unsigned)gi + 1;
      ++launch_cnt[EKF_LAUNCH_SOLVE_POLL_CHAIN];
    }
    switch (solve_shape(p, gi)) {
      case SOLVE_64X64:
        c.tile_list = tilemap.d + solve6464_off + 2 * (2 * ntc - 2 * wt) * 2 * ntr; c.ntiles = 2 * wt * 2 * ntr;
        c.counter = ux.take_queue();
        gemm<ROLE_SOLVE, true, 64, 64>(c);
        break;
      case SOLVE_128_ONE_PER_CU:
        c.tile_list = tilemap.d + solve_off + 2 * (ntc - wt) * ntr; c.ntiles = wt * ntr;
        c.counter = ux.take_queue();
        c.one_per_cu = true;
        gemm<ROLE_SOLVE, true>(c);
        break;
      case SOLVE_64X128:
        // (round 6: when the bf16x6 downdate follows, the tiles also write the plane image of V_g it reads)
        if (kIsF32 && opt_fuse_split && opt_split_bf16 && p.tile == 128 && tri_count >= num_cus && ux.queue_room(16)) {
          HIPCHK(ensure_vimg());
          c.img = d_Vimg; c.img_nkc = ldy / 16; c.img_c0 = c0;
          *vimg_done = true;
        }
        c.tile_list = tilemap.d + solve64_off + 2 * (ntc - wt) * 2 * ntr; c.ntiles = wt * 2 * ntr;
        c.counter = ux.take_queue();
        gemm<ROLE_SOLVE, true, 64, 128>(c);
        break;
      case SOLVE_128:
        c.tile_list = tilemap.d + solve_off + 2 * (ntc - wt) * ntr; c.ntiles = wt * ntr;
        c.counter = ux.take_queue();
        gemm<ROLE_SOLVE, true>(c);
        break;
    }
    return EKF_OK;
  }

  // The W update [W; nu^T][:, c1:] -= V_g L[c1:, c0:c1]^T of chunk gi on stream ss, where it is a launch of its own: the
  // innovation row alone when W is recomputed (nothing when the row rides in the downdate's launch), nothing when the
  // downdate's launch carries the update (chunk_fuses)
  void wupdate_chunk(const UpdatePlan& p, int gi, const UpdateCtx& ux, hipStream_t ss) {
    const int c0 = p.c0(gi), c1 = p.c1(gi);
    if (c1 >= p.m_pad || chunk_fuses(p, gi, ux) || chunk_row_rider(p, gi, ux)) return;
    if (p.recompute) {
      launch_row_update(c0, c1, p.m_pad, ss, kIsF32 && opt_row_gemv);
      return;
    }
    Scope sc(this, KID_WUPDATE, ss);
    ++launch_cnt[EKF_LAUNCH_W_UPDATE_GEMM];
    GemmCall c;
    c.A = d_V + c0; c.lda = ldy; c.B = d_Y + (size_t)c1 * ldy + c0; c.ldb = ldy; c.C = d_W + c1; c.ldc = ldy;
    c.rows = p.npad_live + p.nb; c.cols = p.m_pad - c1; c.K = c1 - c0; c.alpha = T(-1); c.beta = T(1);
    c.st = ss;
    if (kIsF32 && opt_mfma && ((p.m_pad - c1) / 128) * p.ntr < chunk_slots(p, gi))
      gemm<ROLE_WUPDATE, false, 64, 128>(c);
    else
      gemm<ROLE_WUPDATE, false>(c);
  }

  // The downdate Sigma -= V_g V_g^T of chunk gi on stream ss: the bf16x6 kernel (with the row rider / the state update in
  // its tail), the fp32 tiles together with the W update (chunk_fuses), or the fp32 tiles alone; nothing when the
  // solve's launch has done it (allinone)
  int downdate_chunk(const UpdatePlan& p, int gi, UpdateCtx& ux, hipStream_t ss, bool vimg_done) {
    const int c0 = p.c0(gi), c1 = p.c1(gi), width = c1 - c0, m = p.m, m_pad = p.m_pad, npad_live = p.npad_live;
    if (chunk_splits(p, ux)) {
      // the lower tiles of Sigma, downdated from LDS-DMA-fed records of the plane image (only the plain step counts its
      // image launches)
      const bool row_rider = chunk_row_rider(p, gi, ux), su_tail = chunk_su_tail(p, gi, ux);
      if (!vimg_done) ++launch_cnt[EKF_LAUNCH_SPLIT_IMAGE];
      // Every launch but the last of the update mirrors only what is read before the last launch -- which gets no bounds and
      // restores every mirror -- overwrites it: the feature columns of the next chunk's re-evaluation (table entry gi + 1),
      // nothing when W is updated right-looking (nobody reads Sigma between the launches: the empty entry)
      const int* mirror_rows = nullptr;
      if (opt_syrk_mirror_skip && gi + 1 < p.nchunks)
        mirror_rows = d_counters + kResetInts + 2 * (p.recompute ? gi + 1 : kMirrorEmpty);
      return launch_downdate_bf16x6(ux, c0, c1, m_pad, ss, !vimg_done, tilemap.d + tri6_off, tri_count, 0, 0, INT_MAX,
                                    double(n) * n * (std::min(c1, m) - std::min(c0, m)), row_rider, su_tail, mirror_rows);
    }
    if (chunk_fuses(p, gi, ux)) {
      if constexpr (kIsF32) {
        Scope sc(this, KID_DOWNDATE, ss);               // W[:, c1:] -= V_g L[c1:, g]^T, then Sigma -= V_g V_g^T
        // (recompute: of [W; nu^T] only the row tile that holds nu^T -- the rows of W are re-evaluated from Sigma)
        const int nr2 = p.recompute ? 1 : (npad_live + p.nb) / 128, n2 = nr2 * ((m_pad - c1) / 128);
        if (sc.on) {
          const double w = std::min(c1, m) - std::min(c0, m);
          prof.work[KID_DOWNDATE] += double(n) * n * w + 2.0 * (p.recompute ? 1 : n + 1) * std::max(0, m - c1) * w;
        }
        GemmArgs g{};
        g.A = d_V + c0; g.lda = ldy; g.B = d_V + c0; g.ldb = ldy; g.C = S(); g.ldc = ld;
        g.K = width; g.alpha = -1.0; g.beta = 1.0; g.tri = TRI_LOWER_MIRROR;
        g.tile_map = tilemap.d; g.ntiles = n2 + tri_count; g.counter = ux.take_queue(); g.stagger = 1;
        g.B2 = d_Y + (size_t)c1 * ldy + c0; g.ldb2 = ldy; g.C2 = d_W + c1; g.ldc2 = ldy;
        g.n2 = n2; g.nr2 = nr2; g.row2 = p.recompute ? npad_live / 128 : 0;
        ++launch_cnt[EKF_LAUNCH_DOWNDATE_F32_FUSED_WU];
        const int wgs = 2 * (num_cus - reserved_cus);
        k_gemm_mfma<ROLE_DOWNDATE, false><<<std::min(g.ntiles, wgs), 256, 0, ss>>>(g);
      }
      return EKF_OK;
    }
    if (p.allinone) return EKF_OK;
    Scope sc(this, KID_DOWNDATE, ss);                 // Sigma -= V_g V_g^T (lower tiles + mirror)
    if (sc.on) prof.work[KID_DOWNDATE] += double(n) * n * (std::min(c1, m) - std::min(c0, m));   // symmetric half, 2 flop per MAC
    const bool mf = kIsF32 && opt_mfma;
    const bool t64 = mf && tri_count < num_cus;
    const bool half_tail = !t64 && mf && ss != stream_b && trih_count > tri_count && ux.queue_room();
    ++launch_cnt[t64 ? EKF_LAUNCH_DOWNDATE_F32_T64 : (half_tail ? EKF_LAUNCH_DOWNDATE_F32_HALF_TAIL : EKF_LAUNCH_DOWNDATE_F32)];
    GemmCall c;
    c.A = d_V + c0; c.lda = ldy; c.B = d_V + c0; c.ldb = ldy; c.C = S(); c.ldc = ld;
    c.rows = npad_live; c.cols = npad_live; c.K = width; c.alpha = T(-1); c.beta = T(1); c.tri = TRI_LOWER_MIRROR;
    c.counter = ux.take_queue();
    c.st = ss;
    if (t64) {                                        // small map: 64 x 64 tiles, or most of the chip idles
      c.tile_list = tilemap.d + tri64_off; c.ntiles = tri64_count;
      gemm<ROLE_DOWNDATE, false, 64, 64>(c);
    } else if (mf && ss != stream_b) {                // half tiles at the end of the list: the launch on every CU only (128 x 128 MFMA kernel)
      c.tile_list = tilemap.d + trih_off; c.ntiles = trih_count;
      gemm<ROLE_DOWNDATE, false>(c);
    } else {
      c.tile_list = tilemap.d; c.ntiles = tri_count;
      gemm<ROLE_DOWNDATE, false>(c);
    }
    return EKF_OK;
  }

  // ---- a8-a11 update ---------------------------------------------------------------------
  int update(const void* z, const int* idx, int M, int plane, bool on_device) override {
    HIPCHK(hipSetDevice(device));
    if (sh_on) {
      if (on_device) {
        // the ownership split of the list is made on the host: one small D2H of the indices, z stays where it is
        if (M < 0 || M > N) FAIL(EKF_ERR_ARG, "M out of range");
        std::vector<int> hidx((size_t)std::max(M, 0));
        if (M > 0) {
          HIPCHK(hipMemcpyAsync(hidx.data(), idx, (size_t)M * sizeof(int), hipMemcpyDeviceToHost, stream));
          HIPCHK(hipStreamSynchronize(stream));
        }
        return shard_update(z, hidx.data(), M, plane);
      }
      if (M > 0 && z) HIPCHK(hipMemcpyAsync(d_z, z, (size_t)2 * M * sizeof(T), hipMemcpyHostToDevice, stream));
      return shard_update(d_z, idx, M, plane);
    }
    if (M < 0 || M > N) FAIL(EKF_ERR_ARG, "M out of range");
    if (M == 0 && !plane) return EKF_OK;
    if (!have_meas) FAIL(EKF_ERR_STATE, "ekf_update needs the h/H of ekf_predict or ekf_measure");
    if (M > 0 && (!z || !idx)) FAIL(EKF_ERR_ARG, "z / indices are NULL");
    if (!on_device) { int rcl = check_list(idx, M, true); if (rcl) return rcl; }
    UpdateCtx ux{d_z, d_midx, d_counters};
    if (M > 0) {
      if (on_device) {              // resident inputs are read in place (they must outlive the step)
        ux.z = static_cast<const T*>(z);
        ux.midx = idx;
      } else {
        // host z / indices go through a small ring of pinned staging slots: the two copies are then truly asynchronous
        // (a copy from pageable memory is staged by the runtime and costs the caller ~10 us each)
        int rcs = stage_inputs(z, idx, M);
        if (rcs) return rcs;
        sh_list.clear();
      }
    }
    // Blocked right-looking Cholesky of S in column chunks (a few block steps each).  Chunk g carries its
    // own identity block under S (the strip, rows m_pad..), which the same panel / trailing sweeps turn
    // into Z_gg = L_gg^-T: the inverse of the DIAGONAL chunk only.  As soon as the chain has left chunk g
    // the rest runs on the second stream, off the chain's CUs:
    //   solve       V_g = [W_g; nu_g^T] Z_gg                         (K stops at the diagonal)
    //   W update    [W; nu^T][:, c1:] -= V_g L[c1:, c0:c1]^T         (right-looking, rank = chunk width)
    //   downdate    Sigma -= V_g V_g^T
    // so only the last chunk's solve + downdate are exposed after the chain.
    const UpdatePlan p = plan_update(M, plane);
    int rc = p.onelaunch ? launch_update_small(p, ux)
                         : build_innovation(ux.z, ux.midx, M, plane, true, nullptr, nullptr, &p.tab, p.strip_rows);
    if (rc) return rc;
    rc = ensure_tilemap(p.npad_live / p.tile, p.ntr, p.ntc);
    if (rc) return rc;
    rc = prepare_chain(p, ux, false);
    if (rc) return rc;
    const int nchunks = p.nchunks, m_pad = p.m_pad;
    bool b_inflight = false;
    for (int gi = 0; gi < (p.onelaunch ? 0 : nchunks); ++gi) {
      const int c0 = p.c0(gi), c1 = p.c1(gi);
      // chunk 0 has the chip to itself; later chunks run beside the tile GEMMs of stream_b, on the reserved CUs
      chain_steps(ux, gi ? p.cend[gi - 1] : 0, p.cend[gi], c0, c1, p.m, m_pad, stream, p.oneblock,
                  opt_chain_defer && gi + 1 < nchunks);
      const bool overlap = chunk_overlaps(p, gi);
      hipStream_t ss = overlap ? stream_b : stream;
      if (!overlap && b_inflight) {
        if (p.recompute) {                           // W of this chunk is re-evaluated from Sigma: every earlier downdate first
          HIPCHK(hipEventRecord(ev_b, stream_b));
          HIPCHK(hipStreamWaitEvent(stream, ev_b, 0));
          b_inflight = false;
        } else {                                     // the solve reads W: only the last W update has to be done
          HIPCHK(hipStreamWaitEvent(stream, ev_wu, 0));
        }
      }
      if (overlap) {
        b_inflight = true;
        if (solve_polls_chain(p, gi)) {              // the solve's workgroups wait for this word themselves
          if constexpr (kIsF32)
            k_publish_epoch<<<1, 64, 0, stream>>>(reinterpret_cast<unsigned*>(d_counters + kChainEpochWord), (unsigned)gi + 1);
        } else {
          HIPCHK(hipEventRecord(ev_chain[gi], stream));
          HIPCHK(hipStreamWaitEvent(stream_b, ev_chain[gi], 0));
        }
      }
      bool vimg_done = false;                       // this chunk's solve writes the plane image of V_g
      rc = solve_chunk(p, gi, ux, ss, &vimg_done);
      if (rc) return rc;
      const bool fuse = chunk_fuses(p, gi, ux);
      wupdate_chunk(p, gi, ux, ss);
      if (overlap && c1 < m_pad && !fuse && !p.recompute) HIPCHK(hipEventRecord(ev_wu, stream_b));
      if (!overlap && b_inflight) {                  // earlier downdates must be done before Sigma is touched again
        HIPCHK(hipEventRecord(ev_b, stream_b));
        HIPCHK(hipStreamWaitEvent(stream, ev_b, 0));
        b_inflight = false;
      }
      if (!overlap && nchunks > 1 && !chunk_su_tail(p, gi, ux)) {
        // every column of V and y = L^-1 nu exist now: the state update runs beside the last downdate
        HIPCHK(hipEventRecord(ev_chain[gi], stream));
        HIPCHK(hipStreamWaitEvent(stream_b, ev_chain[gi], 0));
        launch_state_update(m_pad, stream_b);
        b_inflight = true;
      }
      rc = downdate_chunk(p, gi, ux, ss, vimg_done);
      if (rc) return rc;
      if (fuse && !p.recompute) HIPCHK(hipEventRecord(ev_wu, stream_b));
      if (p.recompute && gi + 1 < nchunks) {
        // W[:, c1:c2) = Sigma' H^T for the features of the NEXT chunk, Sigma' = Sigma - sum_{g <= gi} V_g V_g^T (stream
        // order: right behind this chunk's downdate, in front of the wait for the chain): the sequential form of the
        // update.  Only these columns of Sigma' are read (a feature's six columns + the camera's), i.e. one more pass
        // over Sigma in all; the right-looking GEMM update W[:, c1:] -= V_g L[c1:, g]^T of every chunk
        // (2 n w_g (m - c1) flop) is not needed
        launch_w_recompute(c1, p.c1(gi + 1), m_pad, ux.midx, M, plane, ss, n);
      }
    }
    if (b_inflight) {
      HIPCHK(hipEventRecord(ev_b, stream_b));
      HIPCHK(hipStreamWaitEvent(stream, ev_b, 0));
    }
    // (several chunks: the state update ran beside the last downdate or inside it; one block: inside the fused launch)
    return finish_update(p, nchunks == 1 && !p.oneblock, !p.allinone);
  }

  int innovation_covariance(const int* idx, int M, int plane, void* out) override {
    HIPCHK(hipSetDevice(device));
    if (M < 0 || M > N) FAIL(EKF_ERR_ARG, "M out of range");
    if (!have_meas) FAIL(EKF_ERR_STATE, "ekf_innovation_covariance needs ekf_predict / ekf_measure first");
    const int mm = 2 * M + (plane ? 3 : 0);
    if (mm == 0) return EKF_OK;
    int rc = check_list(idx, M, sh_on);
    if (rc) return rc;
    if (M > 0) HIPCHK(hipMemcpyAsync(d_midx, idx, (size_t)M * sizeof(int), hipMemcpyHostToDevice, stream));
    sh_list.clear();
    int m = 0, m_pad = 0;
    if (sh_on) {
      rc = shard_build_ws(idx, M, plane, nullptr, &m, &m_pad);       // W rows {camera, own}, own rows of S, "reassemble S"
    } else {
      rc = build_innovation(nullptr, d_midx, M, plane, false, &m, &m_pad);
    }
    if (rc) return rc;
    std::vector<T> tmp((size_t)m * m);
    HIPCHK(hipMemcpy2DAsync(tmp.data(), (size_t)m * sizeof(T), d_Y, (size_t)ldy * sizeof(T), (size_t)m * sizeof(T), m,
                            hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    T* o = static_cast<T*>(out);
    for (int r = 0; r < m; ++r)
      for (int c = 0; c < m; ++c) o[(size_t)c * m + r] = tmp[(size_t)r * m + c];
    have_update = false;                                  // Y no longer holds the last factorisation
    return EKF_OK;
  }

  int get_gain(void* out) override {
    HIPCHK(hipSetDevice(device));
    if (!have_update) FAIL(EKF_ERR_STATE, "no update to take the gain from");
    const int m = last_m, nn = last_n, m_pad = last_m_pad;
    const int nb = NB();
    const int npad_live = round_up(nn, nb);
    const size_t need = (size_t)npad_live * m_pad * 2;     // K and the scratch of the back-substitution
    HIPCHK(d_K.reserve(need));
    // K = V L^-1 by block back-substitution over the chunks of the factorisation (only the diagonal
    // inverses Z_gg = L_gg^-T exist):  K_g = (V_g - K[:, c1:] L[c1:, c0:c1]) Z_gg^T,  last chunk first.
    // One chunk: K = V Z^T.
    const T* Zs = d_Y + (size_t)m_pad * ldy;
    int wmax = 0;
    for (int g = 0; g < last_nchunks; ++g) wmax = std::max(wmax, (last_cend[g] - (g ? last_cend[g - 1] : 0)) * nb);
    T* Tm = d_K + (size_t)npad_live * m_pad;              // npad_live x wmax scratch behind K
    for (int g = last_nchunks - 1; g >= 0; --g) {
      const int c0 = (g ? last_cend[g - 1] : 0) * nb, c1 = last_cend[g] * nb, w = c1 - c0;
      const T* A = d_V + c0;
      int lda = ldy;
      if (c1 < m_pad) {
        dim3 grid((w + 255) / 256, npad_live);
        k_copy2d<T><<<grid, 256, 0, stream>>>(d_V + c0, ldy, Tm, wmax, npad_live, w);
        GemmCall sub;                                       // Tm = V_g - K[:, c1:] L[c1:, c0:c1]
        sub.A = d_K + c1; sub.lda = m_pad; sub.B = d_Y + (size_t)c1 * ldy + c0; sub.ldb = ldy; sub.C = Tm; sub.ldc = wmax;
        sub.rows = npad_live; sub.cols = w; sub.K = m_pad - c1; sub.alpha = T(-1); sub.beta = T(1);
        gemm<ROLE_GAIN, true>(sub);
        A = Tm;
        lda = wmax;
      }
      GemmCall kg;                                          // K_g = A Z_gg^T
      kg.A = A; kg.lda = lda; kg.B = Zs + c0; kg.ldb = ldy; kg.C = d_K + c0; kg.ldc = m_pad;
      kg.rows = npad_live; kg.cols = w; kg.K = w;
      gemm<ROLE_GAIN, false>(kg);
    }
    std::vector<T> tmp((size_t)nn * m);
    HIPCHK(hipMemcpy2DAsync(tmp.data(), (size_t)m * sizeof(T), d_K, (size_t)m_pad * sizeof(T), (size_t)m * sizeof(T), nn,
                            hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    T* o = static_cast<T*>(out);
    for (int r = 0; r < nn; ++r)
      for (int c = 0; c < m; ++c) o[(size_t)c * nn + r] = tmp[(size_t)r * m + c];
    return EKF_OK;
  }

  // ---- state / covariance access ------------------------------------------------------------
  int get_state(void* out, int off, int count) override {
    HIPCHK(hipSetDevice(device));
    if (off < 0 || count < 0 || off + count > n) FAIL(EKF_ERR_ARG, "state segment out of range");
    if (count) { int rc = rb_add(out, mu() + off, (size_t)count * sizeof(T)); if (rc) return rc; }
    return rb_finish(true);                              // data and status words in one synchronisation
  }
  int set_state(const void* in, int off, int count) override {
    HIPCHK(hipSetDevice(device));
    if (off < 0 || count < 0 || off + count > n) FAIL(EKF_ERR_ARG, "state segment out of range");
    if (count) HIPCHK(hipMemcpyAsync(mu() + off, in, (size_t)count * sizeof(T), hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
    have_meas = false;
    return EKF_OK;
  }
  int get_sigma(void* out, int r0, int c0, int rows, int cols) override {
    HIPCHK(hipSetDevice(device));
    if (r0 < 0 || c0 < 0 || rows < 0 || cols < 0 || r0 + rows > n || c0 + cols > n)
      FAIL(EKF_ERR_ARG, "covariance block out of range");
    if (rows == 0 || cols == 0) return EKF_OK;
    std::vector<T> tmp((size_t)rows * cols);
    int rcs = EKF_OK;
    if (tmp.size() * sizeof(T) <= ((size_t)1 << 22)) {    // small blocks: pinned bounce, status in the same round trip
      int rc = rb_add_2d(tmp.data(), S() + (size_t)r0 * ld + c0, (size_t)ld * sizeof(T), (size_t)cols * sizeof(T), rows);
      if (rc) return rc;
      rcs = rb_finish(true);
    } else {
      HIPCHK(hipMemcpy2DAsync(tmp.data(), (size_t)cols * sizeof(T), S() + (size_t)r0 * ld + c0, (size_t)ld * sizeof(T),
                              (size_t)cols * sizeof(T), rows, hipMemcpyDeviceToHost, stream));
      HIPCHK(hipStreamSynchronize(stream));
      rcs = check_status();
    }
    T* o = static_cast<T*>(out);
    for (int r = 0; r < rows; ++r)
      for (int c = 0; c < cols; ++c) o[(size_t)c * rows + r] = tmp[(size_t)r * cols + c];
    return rcs;
  }
  // diagnostics (tools/determinism_probe_sharded.py): a block of the update's workspace as the last update left it --
  // which = 0: W (the columns of every chunk as the solve read them), 1: V = W L^-T; row-major rows x cols
  int peek_work(int which, void* out, int r0, int c0, int rows, int cols) override {
    HIPCHK(hipSetDevice(device));
    if (which == 3) {
      // the phase stamps of k_update_small_onelaunch (EKF_SMALL_STAMPS=1): 16 64-bit words (rows = 16, cols = 2 32-bit halves)
      if (!d_small_stamps) FAIL(EKF_ERR_STATE, "no stamps (create the filter with EKF_SMALL_STAMPS=1)");
      if (rows != 16 || cols != 2 || r0 != 0 || c0 != 0) FAIL(EKF_ERR_ARG, "stamp block out of range");
      HIPCHK(hipDeviceSynchronize());
      HIPCHK(hipMemcpy(out, d_small_stamps, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
      return EKF_OK;
    }
    if (which == 4) {
      // lambda of the last ekf_find_new_features (ekf_features.hpp): fp64 whatever the filter's dtype, frame rows x columns
      if (!have_seed_lam) FAIL(EKF_ERR_STATE, "no corner response (call ekf_find_new_features first)");
      if (r0 < 0 || c0 < 0 || rows < 0 || cols < 0 || r0 + rows > frame_h || c0 + cols > frame_w)
        FAIL(EKF_ERR_ARG, "response block out of range");
      if (rows == 0 || cols == 0) return EKF_OK;
      HIPCHK(hipStreamSynchronize(stream));
      const double* src = d_seed_lam + (size_t)r0 * frame_w + c0;
      HIPCHK(hipMemcpy2D(out, (size_t)cols * sizeof(double), src, (size_t)frame_w * sizeof(double), (size_t)cols * sizeof(double),
                         rows, hipMemcpyDeviceToHost));
      return EKF_OK;
    }
    if (which < 0 || which > 1) FAIL(EKF_ERR_ARG, "workspace id out of range");
    if (r0 < 0 || c0 < 0 || rows < 0 || cols < 0 || r0 + rows > n_pad + NB() || c0 + cols > ldy)
      FAIL(EKF_ERR_ARG, "workspace block out of range");
    if (rows == 0 || cols == 0) return EKF_OK;
    HIPCHK(hipDeviceSynchronize());
    const T* src = (which == 0 ? d_W : d_V) + (size_t)r0 * ldy + c0;
    HIPCHK(hipMemcpy2D(out, (size_t)cols * sizeof(T), src, (size_t)ldy * sizeof(T), (size_t)cols * sizeof(T), rows, hipMemcpyDeviceToHost));
    return EKF_OK;
  }
  int set_sigma(const void* in, int r0, int c0, int rows, int cols) override {
    HIPCHK(hipSetDevice(device));
    if (r0 < 0 || c0 < 0 || rows < 0 || cols < 0 || r0 + rows > n || c0 + cols > n)
      FAIL(EKF_ERR_ARG, "covariance block out of range");
    if (rows == 0 || cols == 0) return EKF_OK;
    const T* i = static_cast<const T*>(in);
    std::vector<T> tmp((size_t)rows * cols);
    for (int r = 0; r < rows; ++r)
      for (int c = 0; c < cols; ++c) tmp[(size_t)r * cols + c] = i[(size_t)c * rows + r];
    HIPCHK(hipMemcpy2DAsync(S() + (size_t)r0 * ld + c0, (size_t)ld * sizeof(T), tmp.data(), (size_t)cols * sizeof(T),
                            (size_t)cols * sizeof(T), rows, hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
    have_meas = false;
    return EKF_OK;
  }
  int covariance_parameter(double* out) override {
    T d[7 * 7];
    int rc = get_sigma(d, 0, 0, 7, 7);
    if (rc) return rc;
    T acc = T(0);
    acc += d[0] + d[8] + d[16];                          // vR.cpp:854
    acc += d[32] + d[40] + d[48] + d[24];                // vR.cpp:855
    *out = double(acc);
    return EKF_OK;
  }
  int check_invariants(double* pad, double* asym, double* big) override {
    HIPCHK(hipSetDevice(device));
    unsigned int* d_out = reinterpret_cast<unsigned int*>(d_status + 4);      // 4 spare ints behind the status words
    HIPCHK(hipMemsetAsync(d_out, 0, 4 * sizeof(int), stream));
    dim3 grid(std::min(16, (ld + 255) / 256), n_pad);
    k_check_invariants<T><<<grid, 256, 0, stream>>>(S(), ld, n, n_pad, d_out);
    unsigned int h[4];
    { int rc = rb_add(h, d_out, sizeof(h)); if (rc) return rc; }
    int rcs = rb_finish(true);
    float f[3];
    memcpy(f, h, sizeof(f));
    if (pad) *pad = f[0];
    if (asym) *asym = f[1];
    if (big) *big = f[2];
    return rcs;
  }
  int feature_xyz(int index, void* xyz, void* cov) override {
    HIPCHK(hipSetDevice(device));
    if (index < 0 || index >= N) FAIL(EKF_ERR_ARG, "feature index out of range");
    { int rcs = shard_sync_diag_blocks(); if (rcs) return rcs; }      // sharded: the owner's block of the feature (collective)
    k_feature_xyz<T><<<1, 64, 0, stream>>>(mu(), S(), ld, ft.pos(index), ft.coding(index), d_tmp);
    T o[12];
    { int rc = rb_add(o, d_tmp, sizeof(o)); if (rc) return rc; rc = rb_finish(false); if (rc) return rc; }
    T* x = static_cast<T*>(xyz);
    T* c = static_cast<T*>(cov);
    if (x) for (int k = 0; k < 3; ++k) x[k] = o[k];
    if (c) for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) c[b * 3 + a] = o[3 + a * 3 + b];
    return EKF_OK;
  }
  // ---- f2 / f1: search ellipses and 1-point RANSAC hypotheses -------------------------------------
  DevBuf<int> d_ibuf;                    // 3 N ints (ellipses) / M ints (counts)
  DevBuf<unsigned char> d_rmask;         // M x M inlier mask
  hipError_t ensure_ibuf() { return d_ibuf.reserve((size_t)std::max(capN, 1) * 3); }
  hipError_t ensure_rmask(int M) { return d_rmask.reserve((size_t)M * M); }
  hipError_t ensure_gate() { return h_gate.reserve((size_t)std::max(capN, 1) + 64); }

  int rescue(const void* cam_before, const void* z, const int* idx, int M, double thr, unsigned char* out) override {
    HIPCHK(hipSetDevice(device));
    if (M <= 0) return EKF_OK;
    if (M > N || !cam_before || !z || !idx || !out) FAIL(EKF_ERR_ARG, "bad arguments");
    int rc = check_list(idx, M, sh_on);
    if (rc) return rc;
    rc = sync_layout();
    if (rc) return rc;
    rc = stage_inputs(z, idx, M, cam_before);          // pinned staging ring -> d_z / d_midx / d_tmp
    if (rc) return rc;
    sh_list.clear();
    HIPCHK(ensure_ibuf());
    // the gate flags go straight into host-mapped pinned memory (one synchronisation, no staged copy)
    HIPCHK(ensure_gate());
    unsigned char* d_out = h_gate;
    {
      Scope sc(this, KID_MEASURE);
      k_measure<T><<<(M + 63) / 64, 64, 0, stream>>>(mu(), d_pos, d_coding, 0, N, cam, d_h, d_Hc, d_Hf, d_flags, d_midx, M,
                                                    d_tmp);
      if (sh_on) {
        // S_hi = H Sigma H^T of a listed feature needs its rows of Sigma: owner-computes, then the 2x2 blocks are gathered
        const ShardTab lt = list_tab(idx, M);
        const int k0 = lt.start[sh_rank], kc = lt.count[sh_rank];
        if (kc > 0)
          k_measure_sd<T><<<(16 * kc + 255) / 256, 256, 0, stream>>>(S(), ld, d_pos, d_coding, 0, N, T(0), d_Hc, d_Hf, d_Sd,
                                                                    d_midx + k0, kc);
        HIPCHK(hipGetLastError());
        int rg = gather_sd(lt, d_midx);
        if (rg) return rg;
      } else {
        k_measure_sd<T><<<(16 * M + 255) / 256, 256, 0, stream>>>(S(), ld, d_pos, d_coding, 0, N, T(0), d_Hc, d_Hf, d_Sd,
                                                                 d_midx, M);
      }
      k_chi2_gate<T><<<(M + 127) / 128, 128, 0, stream>>>(d_h, d_Sd, d_z, d_midx, M, T(thr), d_out);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(stream));
    memcpy(out, d_out, (size_t)M);
    have_meas = true;          // the listed features carry fresh h / H (the others keep older ones)
    have_sd = false;           // the 2x2 blocks just written have no measurement noise: not the St blocks
    return EKF_OK;
  }

  DevBuf<T> d_pts;
  DevBuf<T> d_tab;                       // table of ekf_export_points_table (grow-only), 12 scalars per row
  int export_points(void* out, int convert) override {
    HIPCHK(hipSetDevice(device));
    if (N == 0) return EKF_OK;
    int rc = sync_layout();
    if (rc) return rc;
    HIPCHK(d_pts.reserve((size_t)std::max(capN, 1) * 12));
    rc = shard_sync_diag_blocks();                                      // sharded: every feature's own block from its owner
    if (rc) return rc;
    const T* scale_ptr = (camera_dim == 14) ? mu() + 13 : nullptr;      // the map scale is read on the device
    k_export_points<T><<<(N + 63) / 64, 64, 0, stream>>>(mu(), S(), ld, d_pos, d_coding, N, T(1), convert, d_pts, nullptr, 0,
                                                        scale_ptr);
    HIPCHK(hipGetLastError());
    { int rcb = rb_add(out, d_pts, (size_t)N * 12 * sizeof(T)); if (rcb) return rcb; }
    return rb_finish(true);                                             // table and status words: one synchronisation
  }

  // RosVSLAM::getPointsFeatures with its real_index row order and the archived patches (RosVSLAMRansac.cpp:340-418)
  int export_points_table(void* out, int max_rows, int* rows_out) override {
    HIPCHK(hipSetDevice(device));
    const int rows = N ? ft.real_index(N - 1) + 1 : 0;            // :350-352
    if (rows_out) *rows_out = rows;
    if (!out || rows == 0) return EKF_OK;
    if (max_rows < rows) FAIL(EKF_ERR_ARG, "ekf_export_points_table: the buffer holds fewer rows than the table");
    int rc = sync_layout();
    if (rc) return rc;
    rc = shard_sync_diag_blocks();                                      // sharded: every feature's own block from its owner
    if (rc) return rc;
    if ((size_t)rows * 12 > d_tab.capacity()) {                         // grow-only table buffer
      HIPCHK(hipStreamSynchronize(stream));
      HIPCHK(d_tab.reserve((size_t)rows * 12, std::max<size_t>(2 * (size_t)rows, 256) * 12));
    }
    HIPCHK(hipMemsetAsync(d_tab, 0, (size_t)rows * 12 * sizeof(T), stream));
    const T* scale_ptr = (camera_dim == 14) ? mu() + 13 : nullptr;      // the map scale is read on the device
    const size_t na = arch_real.size();
    HIPCHK(ensure_arch_idx((size_t)N + na));
    HIPCHK(hipMemcpyAsync(d_arch_idx, ft.columns().real_index.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, stream));
    if (na) HIPCHK(hipMemcpyAsync(d_arch_idx + N, arch_real.data(), na * sizeof(int), hipMemcpyHostToDevice, stream));
    k_export_points<T><<<(N + 63) / 64, 64, 0, stream>>>(mu(), S(), ld, d_pos, d_coding, N, T(1), 0, d_tab, d_arch_idx, rows,
                                                        scale_ptr);
    if (na)
      k_export_archived<T><<<((int)na * 12 + 255) / 256, 256, 0, stream>>>(d_archive, d_arch_idx + N, (int)na, T(1), d_tab, rows,
                                                                          scale_ptr);
    int rcs = EKF_OK;
    if ((size_t)rows * 12 * sizeof(T) <= ((size_t)1 << 22)) {
      rcs = rb_add(out, d_tab, (size_t)rows * 12 * sizeof(T));
      if (!rcs) rcs = rb_finish(true);
    } else {
      HIPCHK(hipMemcpyAsync(out, d_tab, (size_t)rows * 12 * sizeof(T), hipMemcpyDeviceToHost, stream));
      HIPCHK(hipStreamSynchronize(stream));
      rcs = check_status();
    }
    if (na > 7000) arch_real.clear();                           // :396-404: the archive is emptied once it is that long
    return rcs;
  }
  int feature_ids(int* ri, int* nf) const override {
    for (int i = 0; i < N; ++i) { if (ri) ri[i] = ft.real_index(i); if (nf) nf[i] = ft.n_find(i); }
    return EKF_OK;
  }
  int set_feature_meta(int index, int ri, int nf) override {
    if (index < 0 || index >= N) FAIL(EKF_ERR_ARG, "feature index out of range");
    ft.set_meta(index, ri, nf);
    return EKF_OK;
  }
  int num_archived() const override { return (int)arch_real.size(); }

  int search_ellipses(int sigma_size, int* out) override {
    HIPCHK(hipSetDevice(device));
    if (!have_meas) FAIL(EKF_ERR_STATE, "ekf_get_search_ellipses needs ekf_predict / ekf_measure first");
    if (N == 0) return EKF_OK;
    { int rcs = ensure_sd(); if (rcs) return rcs; }
    HIPCHK(ensure_ibuf());
    k_search_ellipses<T><<<(N + 127) / 128, 128, 0, stream>>>(d_Sd, N, sigma_size, d_ibuf);
    HIPCHK(hipGetLastError());
    { int rc = rb_add(out, d_ibuf, (size_t)N * 3 * sizeof(int)); if (rc) return rc; }
    return rb_finish(false);
  }

  int ransac(const void* z, const int* idx, int M, double thr, int* counts, unsigned char* inl, int* best) override {
    HIPCHK(hipSetDevice(device));
    if (M <= 0 || M > N || !z || !idx) FAIL(EKF_ERR_ARG, "bad measured set");
    if (!have_meas) FAIL(EKF_ERR_STATE, "ekf_ransac_1point needs ekf_predict / ekf_measure first");
    { int rcl = check_list(idx, M, sh_on); if (rcl) return rcl; }
    { int rcs = stage_inputs(z, idx, M); if (rcs) return rcs; }   // pinned staging ring -> d_z / d_midx
    sh_list.clear();
    int m = 0, m_pad = 0;
    ransac_mask_host = nullptr;
    { int rcs = ensure_sd(); if (rcs) return rcs; }
    if (sh_on) return shard_ransac(idx, M, thr, counts, inl, best);
    int rc = build_innovation(nullptr, d_midx, M, 0, false, &m, &m_pad, nullptr, 0, true);       // W = Sigma H^T for the listed features
    if (rc) return rc;
    have_update = false;
    HIPCHK(ensure_ibuf());
    HIPCHK(ensure_rmask(M));
    {
      Scope sc(this, KID_MISC);
      dim3 grid((M + 127) / 128, M);
      k_ransac_eval<T><<<grid, 128, 0, stream>>>(mu(), d_W, ldy, d_Sd, d_h, d_z, d_pos, d_coding, d_midx, M, cam,
                                                T(thr), d_rmask);
      k_ransac_count<<<(M + 127) / 128, 128, 0, stream>>>(d_rmask, M, d_ibuf);
    }
    // ONE read-back: counts, the camera pose and -- up to 64 KiB -- the whole inlier mask through a host-mapped pinned
    // buffer the device writes (k_pack_ransac), one synchronisation
    const size_t counts_bytes = ((size_t)capN * sizeof(int) + 15) / 16 * 16;   // the pose behind the counts stays 16-byte aligned
    HIPCHK(h_ransac.reserve(counts_bytes + 8 * sizeof(T) + kRansacMaskBytes + 64));
    unsigned char* hr = h_ransac;
    int* pc = reinterpret_cast<int*>(hr);
    T* pcam = reinterpret_cast<T*>(hr + counts_bytes);
    unsigned char* pmask = reinterpret_cast<unsigned char*>(pcam + 8);
    const int with_mask = ((size_t)M * M <= kRansacMaskBytes) ? 1 : 0;
    k_pack_ransac<T><<<with_mask ? std::max(1, std::min(64, (M * M + 255) / 256)) : (M + 255) / 256, 256, 0, stream>>>(
        d_ibuf, M, mu(), d_rmask, with_mask, pc, pcam, pmask);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(stream));
    for (int k = 0; k < 7; ++k) ransac_cam[k] = double(pcam[k]);
    ransac_cam_valid = true;
    if (with_mask) { ransac_mask_host = pmask; ransac_mask_M = M; }
    int b = 0;
    for (int k = 1; k < M; ++k) if (pc[k] > pc[b]) b = k;
    if (counts) for (int k = 0; k < M; ++k) counts[k] = pc[k];
    if (best) *best = b;
    if (inl) {
      if (with_mask) {
        for (int k = 0; k < M; ++k) inl[k] = pmask[(size_t)k * M + b];
      } else {
        int rcf = fetch_mask_column(b, idx, M, inl);
        if (rcf) return rcf;
      }
    }
    return EKF_OK;
  }

  // ---- f1: the whole RANSAC branch of VSlamFilter::update (vR.cpp:964-1130 + 1245-1284) in one call -------------
  // glibc's rand() (random_r TYPE_3: additive feedback r[i] = r[i-3] + r[i-31], seeded by the Lehmer generator
  // 16807 x mod 2^31 - 1, 310 outputs discarded, result >> 1): the reference draws its hypotheses with
  // srand(time(NULL)) / rand() (vR.cpp:970, 989), so a given seed reproduces its draw sequence on a glibc platform.
  struct GlibcRand {
    std::vector<unsigned int> st;
    explicit GlibcRand(unsigned int seed) {
      if (seed == 0) seed = 1;
      st.assign(34, 0);
      st[0] = seed;
      for (int i = 1; i < 31; ++i) {
        long long v = (16807LL * (int)st[i - 1]) % 2147483647LL;
        if (v < 0) v += 2147483647LL;
        st[i] = (unsigned int)v;
      }
      for (int i = 31; i < 34; ++i) st[i] = st[i - 31];
      for (int i = 34; i < 344; ++i) st.push_back(st[i - 31] + st[i - 3]);
    }
    int next() {
      const size_t i = st.size();
      st.push_back(st[i - 31] + st[i - 3]);
      return (int)(st[i] >> 1);
    }
  };

  int update_two_stage(const void* z_, const int* idx, int M, int plane, unsigned int seed, double thr, double chi2,
                       unsigned char* is_li, unsigned char* is_hi, int* hyp_drawn) override {
    HIPCHK(hipSetDevice(device));
    if (M < 0 || M > N) FAIL(EKF_ERR_ARG, "M out of range");
    if (!have_meas) FAIL(EKF_ERR_STATE, "ekf_update_two_stage needs the h / H of ekf_predict");
    const T* z = static_cast<const T*>(z_);
    std::vector<unsigned char> li(M, 0), hi(M, 0);
    int drawn = 0;
    if (M > 0) {
      std::vector<int> counts(M);
      int best = 0;
      int rc = ransac(z, idx, M, thr, counts.data(), nullptr, &best);        // every hypothesis, one device pass
      if (rc) return rc;
      int sel = best;
      if (seed != 0) {
        // the reference's loop (vR.cpp:986-1034): draw without replacement, adapt the number of hypotheses to the best
        // inlier ratio seen; the low-innovation set is that of the LAST hypothesis drawn (its flags are overwritten
        // on every draw, :1022)
        GlibcRand rng(seed);
        std::vector<int> list(M);
        for (int k = 0; k < M; ++k) list[k] = k;
        int nhyp = 10000, num_zli = 0;
        const float p = 0.99f;
        for (int i = 0; i < nhyp && !list.empty(); ++i) {
          const int posr = rng.next() % (int)list.size();
          sel = list[posr];
          list.erase(list.begin() + posr);
          ++drawn;
          if (counts[sel] > num_zli) {
            num_zli = counts[sel];
            nhyp = (int)(std::log(1 - p) / (std::log(1 - (num_zli / (M + 0.0f)))));   // :1030 (-> 0 when all are inliers)
          }
        }
      } else {
        drawn = M;
      }
      rc = fetch_mask_column(sel, idx, M, li.data());
      if (rc) return rc;
    }
    T cam_before[7];
    if (M > 0 && !sh_on && ransac_cam_valid) {                   // came back with the counts (no update since)
      for (int k = 0; k < 7; ++k) cam_before[k] = T(ransac_cam[k]);
    } else {
      HIPCHK(hipMemcpyAsync(cam_before, mu(), sizeof(cam_before), hipMemcpyDeviceToHost, stream));
      HIPCHK(hipStreamSynchronize(stream));
    }
    ransac_cam_valid = false;
    std::vector<T> zl, zr;
    std::vector<int> il, ir, kr;
    for (int k = 0; k < M; ++k) {
      auto& zz = li[k] ? zl : zr;
      (li[k] ? il : ir).push_back(idx[k]);
      if (!li[k]) kr.push_back(k);
      zz.push_back(z[2 * k]);
      zz.push_back(z[2 * k + 1]);
    }
    if (!il.empty()) {                                           // low-innovation update (vR.cpp:1036-1064): no plane rows
      int rc = update(zl.data(), il.data(), (int)il.size(), 0, false);
      if (rc) return rc;
    }
    std::vector<T> zh;
    std::vector<int> ih;
    if (!ir.empty()) {                                           // high-innovation rescue (vR.cpp:1066-1117)
      std::vector<unsigned char> g(ir.size(), 0);
      int rc = rescue(cam_before, zr.data(), ir.data(), (int)ir.size(), chi2, g.data());
      if (rc) return rc;
      for (size_t t = 0; t < ir.size(); ++t)
        if (g[t]) { hi[kr[t]] = 1; ih.push_back(ir[t]); zh.push_back(zr[2 * t]); zh.push_back(zr[2 * t + 1]); }
    }
    if (!ih.empty() || plane) {                                  // second update incl. the plane rows (vR.cpp:1245-1284)
      if (ih.empty()) {                                          // plane rows only: h / H of no feature are needed
        have_meas = true;
      }
      int rc = update(zh.data(), ih.data(), (int)ih.size(), plane, false);
      if (rc) return rc;
    }
    for (int k = 0; k < M; ++k)                                  // update_quality_index (vR.cpp:1297, Patch.cpp:145)
      if (li[k] || hi[k]) ft.count_found(idx[k]);
    if (is_li) memcpy(is_li, li.data(), M);
    if (is_hi) memcpy(is_hi, hi.data(), M);
    if (hyp_drawn) *hyp_drawn = drawn;
    return EKF_OK;
  }

  // ---- key-frame selection (kernels in ekf_keyframe.hpp) ------------------------------------------------
  int kf_create(KfSelector* k) override {
    if (sh_on) FAIL(EKF_ERR_STATE, "ekf_keyframe_create: a sharded filter has no key-frame selector (Sigma[0:7,0:7] lives on one rank)");
    HIPCHK(hipSetDevice(device));
    k->device = device;
    k->img_w = cam.width;
    k->img_h = cam.height;
    k->cam = cam;                                              // the lens model and scale its rectified getters use (§14)
    k->scale = cfg.scale;
    const size_t px = (size_t)std::max(cam.width, 1) * std::max(cam.height, 1);
    HIPCHK(k->d_state.reserve(2));
    HIPCHK(k->d_rec.reserve(1));
    HIPCHK(k->d_cand.reserve(px));
    HIPCHK(k->d_emit.reserve(px));
    if (k->raw_w > 0) {                                        // ekf_keyframe_create_raw: the two slots of the camera's own frame
      const size_t rb = (size_t)k->raw_w * k->raw_h * k->raw_c;
      HIPCHK(k->d_cand_raw.reserve(rb));
      HIPCHK(k->d_emit_raw.reserve(rb));
    }
    const KfState s0 = KfSelector::initial();
    HIPCHK(hipMemcpy(k->d_state, &s0, sizeof(s0), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(k->d_rec, 0, sizeof(KfRecord)));
    return EKF_OK;
  }
  // Point4sba (mono-slam vslamRansac.cpp:1319-1336) from the host's track state, as formats.point4sba_rows
  // uv: the float track centre behind every row (2 per row; none for the placeholder), for ekf_keyframe_get_emitted_rectified
  void kf_point4sba(std::vector<int>& rows, std::vector<float>& uv) const {
    rows.assign(3, 0);
    uv.clear();
    for (int i = 0; i < N; ++i) {
      if (!(ft.in_innovation(i) && ft.coding(i) == 1)) continue;
      const float* c = ft.center(i);
      const int r[3] = {ft.real_index(i), (int)c[0], (int)c[1]};
      if (rows[0] == 0) { std::copy(r, r + 3, rows.begin()); uv.assign(c, c + 2); }
      else if (r[1] < 640 && r[2] < 480) { rows.insert(rows.end(), r, r + 3); uv.insert(uv.end(), c, c + 2); }
    }
    if (rows[0] == 0) uv.clear();
  }
  // One probe on the filter's stream, the image grid when a frame is set (a second one for the raw frame of a raw selector), ONE read-back (record, status words and -- only
  // when a predict / measure left them unread -- the track flags), then the host obeys the action word.
  int kf_observe(KfSelector* k, int frame_id, KfRecord* r) override {
    if (sh_on) FAIL(EKF_ERR_STATE, "ekf_keyframe_observe: the filter is sharded (Sigma[0:7,0:7] lives on one rank)");
    HIPCHK(hipSetDevice(device));
    const bool img = have_frame && frame_w == k->img_w && frame_h == k->img_h;
    const bool raw = img && have_raw && k->d_cand_raw && raw_w == k->raw_w && raw_h == k->raw_h && raw_c == k->raw_c;
    k_keyframe_probe<T><<<1, 64, 0, stream>>>(mu(), S(), ld, frame_id, k->move_thresh, k->d_state + k->parity,
                                              k->d_state + (k->parity ^ 1), k->d_rec);
    if (img) {
      const size_t bytes = (size_t)frame_w * frame_h;
      const int grid = (int)std::min<size_t>((bytes / 16 + 255) / 256 + 1, 1024);
      k_keyframe_snapshot<<<grid, 256, 0, stream>>>(k->d_rec, d_frame, k->d_cand, k->d_emit, bytes);
    }
    if (raw) {                                                 // the same action word moves the raw frame / the raw candidate
      const size_t bytes = (size_t)raw_w * raw_h * raw_c;
      const int grid = (int)std::min<size_t>((bytes / 16 + 255) / 256 + 1, 1024);
      k_keyframe_snapshot<<<grid, 256, 0, stream>>>(k->d_rec, d_raw, k->d_cand_raw, k->d_emit_raw, bytes);
    }
    // A failure from here on leaves the rule's state where it was (the roles are not flipped), but the image grid may have
    // run on a record nobody read: either slot may hold this frame now.  Both stop vouching for their image, so that a
    // later emit reports EKF_ERR_STATE from ekf_keyframe_get_image rather than pair an old id with a newer frame.
    auto failed = [&](int rc) {
      if (img) k->cand_has_image = k->emit_has_image = false;
      if (raw) k->cand_has_raw = k->emit_has_raw = false;
      return rc;
    };
    { const hipError_t launch = hipGetLastError(); if (launch != hipSuccess) failed(0); HIPCHK(launch); }
    { int rc = rb_add(r, k->d_rec, sizeof(KfRecord)); if (rc) return failed(rc); }
    std::vector<unsigned char> tb;
    const bool fold = trk_dirty && N > 0;
    if (fold) { tb.resize(N); int rc = rb_add(tb.data(), d_trk, (size_t)N); if (rc) return failed(rc); }
    { int rc = rb_finish(true); if (rc) return failed(rc); }
    if (fold) { HIPCHK(hipMemsetAsync(d_trk, 0, (size_t)N, stream)); apply_track(tb); }
    k->parity ^= 1;
    switch (r->action) {
      case kKfCandidate:
        kf_point4sba(k->cand_rows, k->cand_uv);
        k->cand_has_image = img;
        k->cand_has_raw = raw;
        break;
      case kKfEmitCandidate:
        k->emit_rows = k->cand_rows;
        k->emit_uv = k->cand_uv;
        k->emit_has_image = img && k->cand_has_image;
        k->emit_has_raw = raw && k->cand_has_raw;
        break;
      case kKfEmitCurrent:
      case kKfEmitFirst:
        if (k->keep_current) kf_point4sba(k->emit_rows, k->emit_uv);
        else { k->emit_rows.assign(3, 0); k->emit_uv.clear(); }   // the literal "0  0  0" (monoslam_ransac.cpp:640, :672)
        k->emit_has_image = img;
        k->emit_has_raw = raw;
        break;
      default: break;
    }
    if (r->action >= kKfEmitCurrent) { k->emitted = *r; k->have_emit = true; }
    return EKF_OK;
  }

  // ---- multi-GPU row-panel sharding ------------------------------------------------
  // One process per GPU; every rank holds the same feature list and runs every resize operation, rank g OWNS the
  // contiguous features [sh_fb[g], sh_fb[g+1]) and keeps valid: the rows of Sigma / W / V of those features (all
  // columns) and the camera rows; mu is replicated.  Every exchange is an all-gather of equal-sized staging slots
  // through the host's collective (sh_ag: RCCL via torch.distributed, or a C++ node's own ncclAllGather).
  bool sh_on = false;
  int sh_rank = 0, sh_world = 1;
  std::vector<int> sh_fb;                                  // feature boundaries of the ranks, world + 1 entries
  ekf_allgather_fn sh_ag = nullptr;
  void* sh_ctx = nullptr;
  DevBuf<T> d_stage_send, d_stage_recv;                    // one slot of scalars, and sh_world of them
  int sh_rebalances = 0;
  bool sh_force = false;                                   // world 1 with a callback and EKF_SHARD_FORCE_COLLECTIVE=1: every exchange still runs (profiling the collective path on one GPU)
  std::vector<int> sh_list;                                // host copy of the measured list resident in d_midx
  double sh_imbalance_limit = 1.125;                       // re-partition when a rank owns > 1.125 x the mean rows

  int own_f0() const { return sh_fb[sh_rank]; }
  int own_f1() const { return sh_fb[sh_rank + 1]; }
  int row_of_feature(int f) const { return f < N ? ft.pos(f) : n; }

  // boundaries that balance the ROWS (6 per inverse-depth, 3 per XYZ feature) of the current map
  void partition_by_rows() {
    sh_fb.assign(sh_world + 1, N);
    sh_fb[0] = 0;
    const long long rows = n - camera_dim;
    int f = 0;
    for (int g = 1; g < sh_world; ++g) {
      const long long target = rows * g / sh_world;
      while (f < N && (long long)(ft.pos(f) - camera_dim) < target) ++f;
      sh_fb[g] = f;
    }
  }

  // ---- distributed chain of the sharded step -----------------------------------------------------------
  // From `shard_dist_min_blocks` block steps on (and two ranks or more) the factorisation of S is no longer replicated: rank r OWNS the 128-row
  // blocks I of S with I % world == r (cyclic: the triangle's work is balanced) and keeps only those rows of the trailing
  // matrix up to date -- plus every diagonal block and the chunk's inverse strip, which every rank updates for itself (one
  // block per remaining step and the strip: cheap, and it saves a broadcast per step).  Block step j:
  //   every rank   factor of the diagonal block (j, j)                       (redundant: 17 us, no exchange)
  //   rank r       panel P(j; I) = S(I, j) Linv_jj^T for its own I > j and for the strip rows
  //   ALL-GATHER   of the own panel blocks: afterwards every rank holds all of column block j of L
  //   rank r       trailing update of its own row blocks, of all diagonal blocks (K, K), K > j, and of the strip
  // Every tile is the plain path's tile (k_panel_direct's product, k_gemm_mfma<TRAILING, 64, 64>'s sums): L, the strips and
  // therefore the whole update are bit-identical to the replicated chain's, whoever computed a tile.
  int opt_shard_dist_chain = 1;                          // EKF_SHARD_DIST_CHAIN=0: the replicated chain at every size
  // EKF_SHARD_DIST_MIN_BLOCKS: 40 block steps (N = 2500).  Per step the distributed form pays ~25 us of stand-alone factor and
  // ~35 us of gather where the replicated one pays the whole trailing update; measured on one rank (profiles/
  // r6_shard_world1_dist_chain.txt) the two meet at 32 steps for 8 ranks (2.1 ms each) and the distributed one wins above
  int shard_dist_min_blocks = 40;
  struct DistPlan {                                      // of the plan dist_lists was built for (dist_lists.first() block steps)
    std::vector<int> pb_off, pb_own, pb_cnt, tl_off, tl_cnt, slot_blocks;
    std::vector<int> tb_off, tb_cnt;                     // the same update as (I, K) pairs of 128 x 128 blocks, without (j + 1, j + 1): k_trail_diag
  } dist;
  WorkList dist_lists;                                   // key (nblk, nchunks, world, rank, chunk ends)
  DevBuf<int> d_dist_counters;
  DevBuf<T> d_dist_send, d_dist_recv;
  bool dist_chain_ok(int nsteps) const {
    return kIsF32 && opt_mfma && opt_shard_dist_chain && sh_on && exchanges() && NB() == 128 && nsteps >= shard_dist_min_blocks;
  }
  int ensure_dist_plan(int nblk, int nchunks, const int* cend) {
    std::vector<int> key = {nblk, nchunks, sh_world, sh_rank};
    key.insert(key.end(), cend, cend + nchunks);
    if (!dist_lists.current(key)) {
      std::vector<int> all;
      dist.pb_off.assign(nblk, 0); dist.pb_own.assign(nblk, 0); dist.pb_cnt.assign(nblk, 0);
      dist.tl_off.assign(nblk, 0); dist.tl_cnt.assign(nblk, 0); dist.slot_blocks.assign(nblk, 0);
      dist.tb_off.assign(nblk, 0); dist.tb_cnt.assign(nblk, 0);
      int maxslot = 0;
      for (int j = 0; j < nblk; ++j) {
        int s0 = 0, s1 = nblk;
        for (int g = 0; g < nchunks; ++g)
          if (j < cend[g]) { s0 = g ? cend[g - 1] : 0; s1 = cend[g]; break; }
        dist.pb_off[j] = (int)all.size();
        for (int I = j + 1; I < nblk; ++I)
          if (I % sh_world == sh_rank) all.push_back(I);
        dist.pb_own[j] = (int)all.size() - dist.pb_off[j];
        for (int t = 0; t <= j - s0; ++t) all.push_back(nblk + t);
        dist.pb_cnt[j] = (int)all.size() - dist.pb_off[j];
        for (int g = 0; g < sh_world; ++g) {
          const int first = j + 1 + ((g - (j + 1)) % sh_world + sh_world) % sh_world;
          const int cnt = first < nblk ? (nblk - 1 - first) / sh_world + 1 : 0;
          dist.slot_blocks[j] = std::max(dist.slot_blocks[j], cnt);
        }
        maxslot = std::max(maxslot, dist.slot_blocks[j]);
        dist.tl_off[j] = (int)all.size();
        for (int I = j + 1; I < nblk; ++I) {             // 64 x 64 tiles relative to row / column block j + 1
          const int d = I - j - 1;
          if (I % sh_world == sh_rank) {
            for (int bi = 2 * d; bi < 2 * d + 2; ++bi)
              for (int bj = 0; bj <= bi; ++bj) { all.push_back(bi); all.push_back(bj); }
          } else {                                       // somebody else's rows: the diagonal block only
            all.push_back(2 * d); all.push_back(2 * d);
            all.push_back(2 * d + 1); all.push_back(2 * d);
            all.push_back(2 * d + 1); all.push_back(2 * d + 1);
          }
        }
        for (int t = 0; t <= j - s0; ++t) {              // the strip rows of the chunk: columns up to the chunk's end
          const int rb = nblk - j - 1 + t;
          for (int bi = 2 * rb; bi < 2 * rb + 2; ++bi)
            for (int bj = 0; bj < 2 * (s1 - j - 1); ++bj) { all.push_back(bi); all.push_back(bj); }
        }
        dist.tl_cnt[j] = ((int)all.size() - dist.tl_off[j]) / 2;
        dist.tb_off[j] = (int)all.size();
        for (int I = j + 1; I < nblk; ++I) {
          if (I % sh_world == sh_rank) {
            for (int K = j + 1; K <= I; ++K)
              if (!(I == j + 1 && K == j + 1)) { all.push_back(I); all.push_back(K); }
          } else if (I != j + 1) {
            all.push_back(I); all.push_back(I);
          }
        }
        for (int t = 0; t <= j - s0; ++t)
          for (int K = j + 1; K < s1; ++K) { all.push_back(nblk + t); all.push_back(K); }
        dist.tb_cnt[j] = ((int)all.size() - dist.tb_off[j]) / 2;
      }
      HIPCHK(hipStreamSynchronize(stream));
      if (stream_b) HIPCHK(hipStreamSynchronize(stream_b));
      HIPCHK(d_dist_counters.reserve((size_t)nblk * 8));
      const size_t slot = (size_t)std::max(maxslot, 1) * 128 * 128;
      HIPCHK(d_dist_send.reserve(slot));
      HIPCHK(d_dist_recv.reserve(slot * sh_world));
      HIPCHK(dist_lists.upload(key, all));
    }
    HIPCHK(hipMemsetAsync(d_dist_counters, 0, (size_t)nblk * 8 * sizeof(int), stream));
    return EKF_OK;
  }
  // block steps [step0, step1) of the distributed chain on stream st (no deferral: a step ends with its trailing update,
  // which carries the factor of the next step when the rank's blocks fit one round of workgroups)
  int dist_chain_steps(UpdateCtx& ux, int step0, int step1, int m, int m_pad, hipStream_t st) {
    if constexpr (kIsF32) {
      T* Y = d_Y;
      const int nblk = dist_lists.first();
      for (int step = step0; step < step1; ++step) {
        const int j = step * 128, r0 = j + 128;
        T* Dj = d_Dinv + (size_t)step * 128 * 128;
        if (ux.diag_ahead != step) {
          Scope sc(this, KID_CHOL_DIAG, st);
          ++launch_cnt[EKF_LAUNCH_CHAIN_STEP];
          k_chol_diag_packed<><<<1, 1024, 0, st>>>(Y + (size_t)j * ldy + j, ldy, Dj, d_status, std::max(1, std::min(8, (m - j + 15) / 16)));
        }
        const int* pb = dist_lists.d + dist.pb_off[step];
        if (dist.pb_cnt[step] > 0) {
          Scope sc(this, KID_CHOL_PANEL, st);
          ++launch_cnt[EKF_LAUNCH_CHAIN_STEP];
          k_panel_direct_blocks<<<2 * dist.pb_cnt[step], 256, 0, st>>>(Y + j, ldy, Dj, pb);
        }
        if (dist.slot_blocks[step] > 0) {
          Scope sc(this, KID_GATHER_S, st);
          const size_t slot = (size_t)dist.slot_blocks[step] * 128 * 128;
          if (dist.pb_own[step] > 0)
            k_dist_pack_panel<T><<<128 * dist.pb_own[step], 32, 0, st>>>(Y + j, ldy, pb, dist.pb_own[step], d_dist_send);
          ++launch_cnt[EKF_LAUNCH_CHAIN_DIST_GATHER];
          const int rc = sh_ag(sh_ctx, d_dist_send, d_dist_recv, slot * sizeof(T), st);
          if (rc != 0) FAIL(EKF_ERR_DEVICE, "the all-gather callback reported a failure");
          if (sh_world > 1)
            k_dist_unpack_panel<T><<<dim3(128 * dist.slot_blocks[step], 1, sh_world), 32, 0, st>>>(d_dist_recv, slot, Y + j, ldy, step,
                                                                                               nblk, sh_world, sh_rank);
        }
        if (trail_diag_ok() && step + 1 < nblk && dist.tb_cnt[step] >= td_min_blocks && dist.tb_cnt[step] <= std::min(td_max_blocks, num_cus)) {
          // the rank's blocks of the update fit one round of workgroups: the update and the factor of the NEXT step as one
          // launch (k_trail_diag: workgroup 0 updates block (j + 1, j + 1) itself and factors it), as on the plain path
          TrailDiagArgs a{};
          a.Y = d_Y; a.ldy = ldy; a.y_bytes = (unsigned)((size_t)2 * ldy * ldy * sizeof(T));
          a.Dinv = d_Dinv; a.dinv_bytes = (unsigned)((size_t)(ldy / 64) * 128 * 128 * sizeof(T));
          a.status = d_status; a.m = m; a.j = step;
          a.blocks = dist_lists.d + dist.tb_off[step]; a.nblocks = dist.tb_cnt[step]; a.do_diag = 1;
          Scope sc(this, KID_CHOL_TRAILING, st);
          ++launch_cnt[EKF_LAUNCH_CHAIN_TRAIL_DIAG];
          k_trail_diag<<<a.nblocks + 1, 1024, kChainLds, st>>>(a);
          ux.diag_ahead = step + 1;
        } else if (dist.tl_cnt[step] > 0) {
          Scope sc(this, KID_CHOL_TRAILING, st);
          ++launch_cnt[EKF_LAUNCH_CHAIN_STEP];
          const T* P = Y + (size_t)r0 * ldy + j;
          GemmArgs g{};                                    // the rank's tiles of Y[r0.., r0..] -= P P^T, as listed
          g.A = P; g.lda = ldy; g.B = P; g.ldb = ldy; g.C = Y + (size_t)r0 * ldy + r0; g.ldc = ldy;
          g.K = 128; g.alpha = -1.0; g.beta = 1.0; g.tri = TRI_ALL; g.row_off = r0; g.col_off = r0;
          g.tile_map = dist_lists.d + dist.tl_off[step]; g.ntiles = dist.tl_cnt[step]; g.counter = d_dist_counters + 8 * step;
          k_gemm_mfma<ROLE_TRAILING, false, 64, 64><<<std::min(dist.tl_cnt[step], 2 * num_cus), 256, 0, st>>>(g);
        }
      }
      HIPCHK(hipGetLastError());
    }
    (void)m_pad;
    return EKF_OK;
  }

  int ensure_stage(size_t slot_elems) {
    if (slot_elems <= d_stage_send.capacity() && slot_elems * sh_world <= d_stage_recv.capacity()) return EKF_OK;
    HIPCHK(hipStreamSynchronize(stream));
    if (stream_b) HIPCHK(hipStreamSynchronize(stream_b));
    if (stream_g) HIPCHK(hipStreamSynchronize(stream_g));
    slot_elems = (slot_elems + 63) / 64 * 64;
    HIPCHK(d_stage_send.reserve(slot_elems));
    HIPCHK(d_stage_recv.reserve(slot_elems * sh_world));
    return EKF_OK;
  }

  // the collective: slot g of d_stage_recv <- d_stage_send of rank g, ordered on stream `st`
  bool exchanges() const { return sh_world > 1 || sh_force; }
  int all_gather(size_t slot_elems, hipStream_t st) {
    if (!exchanges()) return EKF_OK;
    if (!sh_ag) FAIL(EKF_ERR_STATE, "sharded filter without an all-gather callback (ekf_shard_configure)");
    const int rc = sh_ag(sh_ctx, d_stage_send, d_stage_recv, slot_elems * sizeof(T), st);
    if (rc != 0) FAIL(EKF_ERR_DEVICE, "the all-gather callback reported a failure");
    return EKF_OK;
  }

  // rows [tab.start[g], +tab.count[g]) x columns [col0, col0 + ncols) of `buf` (row stride ldb): own range out,
  // everybody else's in
  int exchange_rows(T* buf, int ldb, const ShardTab& tab, int col0, int ncols, hipStream_t st, int kid) {
    if (!exchanges()) return EKF_OK;
    int maxrows = 0;
    for (int g = 0; g < sh_world; ++g) maxrows = std::max(maxrows, tab.count[g]);
    if (maxrows == 0) return EKF_OK;
    const size_t slot = (size_t)maxrows * ncols;
    int rc = ensure_stage(slot);
    if (rc) return rc;
    Scope sc(this, kid, st);
    const int own = tab.count[sh_rank];
    const int gx = std::max(1, std::min(8, (ncols / (int)(16 / sizeof(T)) + 255) / 256));
    if (own > 0)
      k_pack_rows<T><<<dim3(gx, std::min(own, 65535)), 256, 0, st>>>(buf, ldb, tab.start[sh_rank], own, col0, ncols, d_stage_send);
    rc = all_gather(slot, st);
    if (rc) return rc;
    k_unpack_rows<T><<<dim3(gx, std::min(maxrows, 65535), sh_world), 256, 0, st>>>(d_stage_recv, slot, ncols, buf, ldb, col0, tab);
    HIPCHK(hipGetLastError());
    return EKF_OK;
  }

  ShardTab row_tab() const {                               // state rows owned by every rank
    ShardTab t{sh_world, sh_rank, {}, {}};
    for (int g = 0; g < sh_world; ++g) {
      t.start[g] = row_of_feature(sh_fb[g]);
      t.count[g] = row_of_feature(sh_fb[g + 1]) - t.start[g];
    }
    return t;
  }
  ShardTab feature_tab() const {
    ShardTab t{sh_world, sh_rank, {}, {}};
    for (int g = 0; g < sh_world; ++g) { t.start[g] = sh_fb[g]; t.count[g] = sh_fb[g + 1] - sh_fb[g]; }
    return t;
  }

  // Tile list of a rank's row panel [p0, p0 + prows) x [0, npad_live) for the queued downdate launch (tri = 3): a tile
  // whose rows AND columns lie inside the own rows [r0, r1) is listed once (column tile <= row tile) and mirrored;
  // every other tile -- the ragged first / last row tile of the panel (it holds foreign rows), the columns of other
  // ranks -- is a plain tile.  Row tiles are relative to p0, column tiles absolute.
  int opt_shard_sym = 1;                                   // EKF_SHARD_SYM=0: the plain row panel (A/B)
  int dbg_sync = 0;                                        // EKF_DEBUG_SYNC (bisecting an ordering problem): device synchronisation at 1 the end of
                                                           // the sharded update, 2 the end of every chunk, 4 its start, 8 the end of the sharded predict
  WorkList panel_tiles;
  int panel_ntiles = 0;
  int ensure_panel_tiles(int p0, int prows, int r0, int r1, int npad_live) {
    const std::vector<int> key = {p0, prows, r0, r1, npad_live};
    if (panel_tiles.current(key)) return EKF_OK;
    std::vector<int> tl;
    const int t0 = p0 / 128, nt = prows / 128, nc = npad_live / 128;
    auto interior = [&](int T_) { return 128 * T_ >= r0 && 128 * T_ + 128 <= r1; };
    for (int P = 0; P < nt; ++P) {
      const int Tg = t0 + P;
      for (int J = 0; J < nc; ++J) {
        if (interior(Tg) && interior(J)) {
          if (J > Tg) continue;                            // the mirror of (J, Tg)
          tl.push_back(J < Tg ? (P | kMirrorTile) : P);
          tl.push_back(J);
        } else {
          tl.push_back(P);
          tl.push_back(J);
        }
      }
    }
    HIPCHK(hipStreamSynchronize(stream));
    if (stream_b) HIPCHK(hipStreamSynchronize(stream_b));
    HIPCHK(panel_tiles.upload(key, tl));
    panel_ntiles = (int)tl.size() / 2;
    return EKF_OK;
  }

  // Canonical tiles (bi >= bj) of the bf16x6 downdate that touch a row block with a valid row of this rank (the camera
  // block and the blocks of the own rows [r0, r1)), diagonal tiles first, then the plain path's super-tile order.  What
  // each tile reads and stores is decided in the kernel, row by row (k_syrk_bf16x6: cam, v_lo, v_hi).
  WorkList shard_syrk;
  int shard_syrk_n = 0;
  int ensure_shard_syrk_list(int r0, int r1, int npad_live) {
    const std::vector<int> key = {r0, r1, npad_live, camera_dim};
    if (shard_syrk.current(key)) return EKF_OK;
    const int nt = npad_live / 128, SB = 8, ns = (nt + SB - 1) / SB;
    auto touched = [&](int b) { return b * 128 < camera_dim || (r1 > r0 && b * 128 < r1 && b * 128 + 128 > r0); };
    std::vector<int> tl;
    for (int i = 0; i < nt; ++i) if (touched(i)) { tl.push_back(i); tl.push_back(i); }
    for (int si = 0; si < ns; ++si)
      for (int sj = 0; sj <= si; ++sj)
        for (int i = si * SB; i < std::min(nt, (si + 1) * SB); ++i)
          for (int j = sj * SB; j < std::min(nt, (sj + 1) * SB); ++j)
            if (j < i && (touched(i) || touched(j))) { tl.push_back(i); tl.push_back(j); }
    HIPCHK(hipStreamSynchronize(stream));
    if (stream_b) HIPCHK(hipStreamSynchronize(stream_b));
    HIPCHK(shard_syrk.upload(key, tl, 2));
    shard_syrk_n = (int)tl.size() / 2;
    return EKF_OK;
  }

  // Heaviest-first tile list of the triangular solve on a rank's row panel (64 x 128 tiles; the same order as the plain
  // path's list: column tile ntc - 1 first, every row tile of the panel per column tile).  Round 4: the sharded solve ran
  // as a plain 2-D grid of 128 x 128 tiles, whose static placement pairs the heavy tiles of a column on the same CUs:
  // 0.50 ms of solves per step at N = 1000 / world 1 against 0.16 on the plain path.
  WorkList shard_solve;
  int shard_solve_rows = 0;                                // row tiles per column tile of the list
  int shard_ntc_max() const { return ldy / 128; }
  // The list covers every column tile the workspace can hold (ldy / 128), last column tile first; a chunk of wt column tiles
  // starts at entry (ntc_max - wt) * rows (the entries are relative to the chunk: bj = wt - 1 .. 0), so the list depends on
  // the rows of the rank only -- it is rebuilt (streams drained) when the panel of the rank moves, never because M crossed a
  // multiple of 64.  Round 5: the 64-row tiles of the camera block (when the panel does not start at row 0)
  // and of the innovation block (rows npad_live ..) are in the SAME list, as row tiles relative to the panel's first row
  // (negative for the camera block): one queued launch per chunk instead of three launches, two of them a single
  // latency-bound tile row (0.31 -> 0.2 ms of solves per step at N = 1000 / world 1).
  int ensure_shard_solve_list(int p0, int prows, int npad_live, bool with_cam) {
    const std::vector<int> key = {p0, prows, npad_live, with_cam ? 1 : 0, ldy};
    if (shard_solve.current(key)) return EKF_OK;
    std::vector<int> rows;
    if (with_cam) { rows.push_back(-p0 / 64); rows.push_back(-p0 / 64 + 1); }
    for (int i = 0; i < prows / 64; ++i) rows.push_back(i);
    rows.push_back((npad_live - p0) / 64);
    rows.push_back((npad_live - p0) / 64 + 1);
    const int ntc = shard_ntc_max();
    std::vector<int> tl;
    tl.reserve((size_t)2 * rows.size() * ntc);
    for (int j = ntc - 1; j >= 0; --j)
      for (int bi : rows) { tl.push_back(bi); tl.push_back(j); }
    HIPCHK(hipStreamSynchronize(stream));
    if (stream_b) HIPCHK(hipStreamSynchronize(stream_b));
    HIPCHK(shard_solve.upload(key, tl));
    shard_solve_rows = (int)rows.size();
    return EKF_OK;
  }

  // list positions [start, start + count) of every rank's features in an ascending measured list
  ShardTab list_tab(const int* idx, int M) const {
    ShardTab t{sh_world, sh_rank, {}, {}};
    int k = 0;
    for (int g = 0; g < sh_world; ++g) {
      while (k < M && idx[k] < sh_fb[g]) ++k;
      int e = k;
      while (e < M && idx[e] < sh_fb[g + 1]) ++e;
      t.start[g] = k;
      t.count[g] = e - k;
      k = e;
    }
    return t;
  }
  // all-gather of 2x2 blocks: tab counts FEATURES (list == nullptr: feature indices, else positions of `list`)
  int gather_sd(const ShardTab& tab, const int* list) {
    if (!exchanges()) return EKF_OK;
    int mx = 0;
    for (int g = 0; g < sh_world; ++g) mx = std::max(mx, tab.count[g]);
    if (mx == 0) return EKF_OK;
    const size_t slot = (size_t)4 * mx;
    int rc = ensure_stage(slot);
    if (rc) return rc;
    const int own = tab.count[sh_rank];
    if (own > 0) k_pack_sd<T><<<(4 * own + 255) / 256, 256, 0, stream>>>(d_Sd, list, tab.start[sh_rank], own, d_stage_send);
    rc = all_gather(slot, stream);
    if (rc) return rc;
    k_unpack_sd<T><<<dim3((4 * mx + 255) / 256, sh_world), 256, 0, stream>>>(d_stage_recv, slot, list, d_Sd, tab);
    HIPCHK(hipGetLastError());
    return EKF_OK;
  }
  // Sharded filter: the diagonal block of EVERY feature valid on this rank (a rank's Sigma holds valid rows for the camera
  // and its own features only; the map getters and the removal archive read a feature's own 3 x 3 / 6 x 6 block).  One
  // all-gather of 36 scalars per feature; the foreign blocks are written into the local Sigma (rows nobody else reads,
  // which the next gather of those rows overwrites).  A COLLECTIVE: every rank makes the call.
  int shard_sync_diag_blocks() {
    if (!sh_on || !exchanges() || N == 0) return EKF_OK;
    // repeated map getters between two filter steps cost ONE collective: every entry point that changes mu, Sigma or the
    // layout clears the flag (the C wrappers below), on every rank alike -- the getters stay collective calls all the same
    if (diag_synced) return EKF_OK;
    int rc = sync_layout();
    if (rc) return rc;
    const ShardTab tab = feature_tab();
    int mx = 0;
    for (int g = 0; g < sh_world; ++g) mx = std::max(mx, tab.count[g]);
    const size_t slot = (size_t)36 * mx;
    rc = ensure_stage(slot);
    if (rc) return rc;
    const int own = tab.count[sh_rank];
    if (own > 0)
      k_pack_diag<T><<<(36 * own + 255) / 256, 256, 0, stream>>>(S(), ld, d_pos, d_coding, tab.start[sh_rank], own, d_stage_send);
    rc = all_gather(slot, stream);
    if (rc) return rc;
    k_unpack_diag<T><<<dim3((36 * mx + 255) / 256, sh_world), 256, 0, stream>>>(d_stage_recv, slot, S(), ld, d_pos, d_coding, tab);
    HIPCHK(hipGetLastError());
    diag_synced = true;
    return EKF_OK;
  }
  // raw bytes of every rank (own_bytes <= slot_bytes each) -> host buffer of world x slot_bytes
  int gather_bytes_to_host(const void* d_own, size_t own_bytes, size_t slot_bytes, std::vector<unsigned char>& host) {
    const size_t slot = (slot_bytes + sizeof(T) - 1) / sizeof(T);
    int rc = ensure_stage(slot);
    if (rc) return rc;
    if (own_bytes) HIPCHK(hipMemcpyAsync(d_stage_send, d_own, own_bytes, hipMemcpyDeviceToDevice, stream));
    host.assign((size_t)sh_world * stage_bytes_of(slot), 0);
    if (exchanges()) {
      rc = all_gather(slot, stream);
      if (rc) return rc;
      HIPCHK(hipMemcpyAsync(host.data(), d_stage_recv, (size_t)sh_world * stage_bytes_of(slot), hipMemcpyDeviceToHost, stream));
    } else {
      HIPCHK(hipMemcpyAsync(host.data(), d_stage_send, stage_bytes_of(slot), hipMemcpyDeviceToHost, stream));
    }
    HIPCHK(hipStreamSynchronize(stream));
    return EKF_OK;
  }
  static size_t stage_bytes_of(size_t slot_elems) { return slot_elems * sizeof(T); }

  // W rows {camera, own} for the measured list resident in d_midx, the own rows of S (+ plane / padding rows), and the
  // all-gather of the rows of S ("reassemble S"); d_zz != nullptr: the innovation nu and the queue heads as well
  int shard_build_ws(const int* idx, int M, int plane, const T* d_zz, int* m_out, int* m_pad_out) {
    const int nb = NB();
    const int m = 2 * M + (plane ? 3 : 0), m_pad = round_up(m, nb);
    const int npad_live = round_up(n, nb);
    T* nu_row = d_W + (size_t)ldy * npad_live;
    if (w_zeroed_n != n) {
      HIPCHK(hipMemsetAsync(d_W + (size_t)n * ldy, 0, (size_t)(npad_live - n + nb) * ldy * sizeof(T), stream));
      // the pad rows [n, npad_live) of V are the B operand of every rank's downdate, but only the rank whose tile-padded
      // panel reaches them ever solves them: everywhere else they must be cleared when n shrinks, or rows gathered in
      // earlier frames would be subtracted into the zero padding of Sigma
      if (npad_live > n)
        HIPCHK(hipMemsetAsync(d_V + (size_t)n * ldy, 0, (size_t)(npad_live - n) * ldy * sizeof(T), stream));
      w_zeroed_n = n;
    }
    const int f0 = own_f0(), f1 = own_f1();
    const int r0 = row_of_feature(f0), r1 = row_of_feature(f1);
    ShardTab stab = list_tab(idx, M);
    const int k0 = stab.start[sh_rank], k1 = k0 + stab.count[sh_rank];
    for (int g = 0; g < sh_world; ++g) { stab.start[g] *= 2; stab.count[g] *= 2; }      // rows of S
    if (d_zz) {
      Scope sc(this, KID_INNOVATION);
      k_innovation<T><<<(std::max(m_pad, 64) + 255) / 256, 256, 0, stream>>>(d_zz, d_h, d_midx, M, plane, mu(), nu_row, m_pad,
                                                                          d_counters, N, d_status);
    }
    {
      Scope sc(this, KID_SIGMA_HT);                        // W rows {camera, own}
      constexpr int RB = 32;
      dim3 g1((m_pad / 2 + 255) / 256, (camera_dim + RB - 1) / RB);
      k_sigma_ht<T, RB><<<g1, 256, 0, stream>>>(S(), ld, n, d_Hc, d_Hf, d_pos, d_coding, d_midx, M, plane, d_W, ldy,
                                              m_pad, 0, camera_dim, N);
      if (r1 > r0) {
        bool fastk = false;
        if constexpr (kIsF32) {
          if ((size_t)n * m_pad >= ((size_t)1 << 22)) {        // the LDS-staged kernel of the plain path on the own rows (same sums)
            constexpr int RBf = 8;
            dim3 g2((m_pad / 2 + 127) / 128, (r1 - r0 + RBf - 1) / RBf);
            k_sigma_ht_fast<RBf><<<g2, 256, 0, stream>>>(S(), ld, r1, d_Hc, d_Hf, d_pos, d_coding, d_midx, M, plane, d_W, ldy, m_pad, N,
                                                         0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, r0);
            fastk = true;
          }
        }
        if (!fastk) {
          dim3 g2((m_pad / 2 + 255) / 256, (r1 - r0 + RB - 1) / RB);
          k_sigma_ht<T, RB><<<g2, 256, 0, stream>>>(S(), ld, n, d_Hc, d_Hf, d_pos, d_coding, d_midx, M, plane, d_W, ldy,
                                                  m_pad, r0, r1, N);
        }
      }
    }
    {
      Scope sc(this, KID_INNOVATION_COV);                  // S rows of the own measured features + the plane / padding rows
      constexpr int KB = 8;
      dim3 grid((m_pad + 255) / 256, std::max(1, (k1 - k0 + KB - 1) / KB) + (m_pad - 2 * M + 7) / 8);
      k_innovation_cov<T, KB><<<grid, 256, 0, stream>>>(d_W, ldy, d_Hc, d_Hf, d_pos, d_coding, d_midx, M, plane,
                                                      T(sigma_pixel_2), T(0.00001), d_Y, m_pad, k0, k1,
                                                      static_cast<T*>(nullptr), N);
    }
    HIPCHK(hipGetLastError());
    int rc = exchange_rows(d_Y, ldy, stab, 0, m_pad, stream, KID_GATHER_S);     // "reassemble S"
    if (rc) return rc;
    if (m_out) *m_out = m;
    if (m_pad_out) *m_pad_out = m_pad;
    return EKF_OK;
  }

  // 1-point RANSAC under sharding (vR.cpp:986-1034): hypothesis k needs W[:, 2k:2k+2] on the rows of the feature it
  // re-projects -- a rank evaluates EVERY hypothesis on the listed features it owns (its rows of W), the partial inlier
  // counts are all-gathered and summed; the inlier column of one hypothesis is gathered the same way (fetch_mask_column)
  int shard_ransac(const int* idx, int M, double thr, int* counts, unsigned char* inl, int* best) {
    int m = 0, m_pad = 0;
    {
      // W rows {camera, own} only (no S): the sigma_ht half of shard_build_ws
      const int nb = NB();
      m = 2 * M; m_pad = round_up(m, nb);
      const int npad_live = round_up(n, nb);
      if (w_zeroed_n != n) {
        HIPCHK(hipMemsetAsync(d_W + (size_t)n * ldy, 0, (size_t)(npad_live - n + nb) * ldy * sizeof(T), stream));
        if (npad_live > n)
          HIPCHK(hipMemsetAsync(d_V + (size_t)n * ldy, 0, (size_t)(npad_live - n) * ldy * sizeof(T), stream));
        w_zeroed_n = n;
      }
      const int r0 = row_of_feature(own_f0()), r1 = row_of_feature(own_f1());
      Scope sc(this, KID_SIGMA_HT);
      constexpr int RB = 32;
      dim3 g1((m_pad / 2 + 255) / 256, (camera_dim + RB - 1) / RB);
      k_sigma_ht<T, RB><<<g1, 256, 0, stream>>>(S(), ld, n, d_Hc, d_Hf, d_pos, d_coding, d_midx, M, 0, d_W, ldy, m_pad, 0,
                                              camera_dim, N);
      if (r1 > r0) {
        dim3 g2((m_pad / 2 + 255) / 256, (r1 - r0 + RB - 1) / RB);
        k_sigma_ht<T, RB><<<g2, 256, 0, stream>>>(S(), ld, n, d_Hc, d_Hf, d_pos, d_coding, d_midx, M, 0, d_W, ldy, m_pad,
                                                r0, r1, N);
      }
    }
    have_update = false;
    HIPCHK(ensure_ibuf());
    HIPCHK(ensure_rmask(M));
    const ShardTab lt = list_tab(idx, M);
    const int k0 = lt.start[sh_rank], kc = lt.count[sh_rank];
    {
      Scope sc(this, KID_MISC);
      if (kc > 0) {
        dim3 grid((M + 127) / 128, kc);
        k_ransac_eval<T><<<grid, 128, 0, stream>>>(mu(), d_W, ldy, d_Sd, d_h, d_z, d_pos, d_coding, d_midx, M, cam, T(thr),
                                                  d_rmask, k0);
      }
      k_ransac_count<<<(M + 127) / 128, 128, 0, stream>>>(d_rmask, M, d_ibuf, k0, k0 + kc);
    }
    HIPCHK(hipGetLastError());
    std::vector<unsigned char> host;
    int rc = gather_bytes_to_host(d_ibuf, (size_t)M * sizeof(int), (size_t)M * sizeof(int), host);
    if (rc) return rc;
    const size_t slot_b = host.size() / sh_world;
    std::vector<int> cnt(M, 0);
    const int parts = exchanges() ? sh_world : 1;
    for (int g = 0; g < parts; ++g) {
      const int* p = reinterpret_cast<const int*>(host.data() + (size_t)g * slot_b);
      for (int k = 0; k < M; ++k) cnt[k] += p[k];
    }
    int b = 0;
    for (int k = 1; k < M; ++k) if (cnt[k] > cnt[b]) b = k;
    if (counts) for (int k = 0; k < M; ++k) counts[k] = cnt[k];
    if (best) *best = b;
    if (inl) return fetch_mask_column(b, idx, M, inl);
    return EKF_OK;
  }

  // column `sel` of the inlier mask of the last ekf_ransac_1point (rows = list positions); under sharding every rank
  // contributes the rows of its own listed features
  int fetch_mask_column(int sel, const int* idx, int M, unsigned char* out) {
    if (!sh_on && ransac_mask_host && ransac_mask_M == M) {       // it came back with the counts
      for (int k = 0; k < M; ++k) out[k] = ransac_mask_host[(size_t)k * M + sel];
      return EKF_OK;
    }
    if (!sh_on) {
      // a large mask stayed on the device: its column is packed there (a strided 2-D copy of M one-byte rows takes
      // milliseconds at M = 1000) and comes back through pinned memory
      HIPCHK(ensure_gate());
      k_pack_mask_col<<<(M + 255) / 256, 256, 0, stream>>>(d_rmask, M, sel, 0, M, static_cast<unsigned char*>(h_gate));
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(stream));
      memcpy(out, h_gate, (size_t)M);
      return EKF_OK;
    }
    const ShardTab lt = list_tab(idx, M);
    int mx = 0;
    for (int g = 0; g < sh_world; ++g) mx = std::max(mx, lt.count[g]);
    const int k0 = lt.start[sh_rank], kc = lt.count[sh_rank];
    const size_t slot_bytes = (size_t)std::max(mx, 1);
    int rc = ensure_stage((slot_bytes + sizeof(T) - 1) / sizeof(T));
    if (rc) return rc;
    unsigned char* d_col = reinterpret_cast<unsigned char*>(d_ibuf + M);            // behind the counts
    if (kc > 0) k_pack_mask_col<<<(kc + 255) / 256, 256, 0, stream>>>(d_rmask, M, sel, k0, kc, d_col);
    HIPCHK(hipGetLastError());
    std::vector<unsigned char> host;
    rc = gather_bytes_to_host(d_col, (size_t)kc, slot_bytes, host);
    if (rc) return rc;
    const size_t slot_b = host.size() / sh_world;
    if (exchanges()) {
      for (int g = 0; g < sh_world; ++g) memcpy(out + lt.start[g], host.data() + (size_t)g * slot_b, (size_t)lt.count[g]);
    } else {
      memcpy(out, host.data(), (size_t)M);
    }
    return EKF_OK;
  }

  int shard_configure(int rank, int world, ekf_allgather_fn fn, void* ctx) override {
    if (world < 1 || world > kMaxWorld || rank < 0 || rank >= world) FAIL(EKF_ERR_ARG, "bad rank / world");
    if (world > 1 && !fn) FAIL(EKF_ERR_ARG, "world > 1 needs an all-gather callback");
    HIPCHK(hipSetDevice(device));
    sh_rank = rank; sh_world = world; sh_ag = fn; sh_ctx = ctx;
    sh_on = true;
    if (const char* e = getenv("EKF_SHARD_FORCE_COLLECTIVE")) sh_force = (atoi(e) != 0) && fn != nullptr;
    if (const char* e = getenv("EKF_SHARD_SYM")) opt_shard_sym = atoi(e);
    if (const char* e = getenv("EKF_DEBUG_SYNC")) dbg_sync = atoi(e);
    // From four ranks on the REPLICATED chain, not the rank's share of the GEMMs, is what a step of a long list waits for
    // (DESIGN 6): steps with many rounds of trailing blocks then go back to the 64 x 64 tile kernel, whose occupancy makes the
    // chain's own kernel time 21 % shorter at N = 4000 (13.6 -> 10.7 ms at world 1, profiles/r6_shard_world1_nccl_n4000*.json) at
    // the price of the exposed factor -- on one or two ranks the chain is hidden beside the downdate and the fused launch wins.
    if (world >= 4 && !getenv("EKF_TD_MAX_BLOCKS")) td_max_blocks = 256;
    if (!stream_g) {
      HIPCHK(hipStreamCreateWithFlags(&stream_g, hipStreamNonBlocking));
      for (auto& e : ev_gath) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&ev_g, hipEventDisableTiming));
    }
    // every rank was built by the same calls, so all of Sigma is valid everywhere right now: any partition will do
    partition_by_rows();
    have_meas = false;
    return EKF_OK;
  }

  int shard_info(ekf_shard_info* o) override {
    if (!o) FAIL(EKF_ERR_ARG, "null info");
    memset(o, 0, sizeof(*o));
    o->rank = sh_rank; o->world = sh_world; o->N = N; o->state_dim = n;
    if (sh_on) {
      o->f_begin = own_f0(); o->f_end = own_f1();
      o->row_begin = row_of_feature(own_f0()); o->row_end = row_of_feature(own_f1());
      int mx = 0;
      for (int g = 0; g < sh_world; ++g) mx = std::max(mx, row_of_feature(sh_fb[g + 1]) - row_of_feature(sh_fb[g]));
      o->max_rows_any_rank = mx;
    } else {
      o->f_end = N; o->row_begin = camera_dim; o->row_end = n; o->max_rows_any_rank = n - camera_dim;
    }
    o->rebalances = sh_rebalances;
    return EKF_OK;
  }

  // ownership follows the resize operations every rank executes identically
  void shard_after_add() { if (sh_on) sh_fb[sh_world] = N; }
  void shard_after_compact(const std::vector<char>& rm) {
    if (!sh_on) return;
    std::vector<int> kept_before(rm.size() + 1, 0);
    for (size_t i = 0; i < rm.size(); ++i) kept_before[i + 1] = kept_before[i] + (rm[i] ? 0 : 1);
    for (int g = 0; g <= sh_world; ++g) sh_fb[g] = kept_before[std::min<size_t>(sh_fb[g], rm.size())];
  }

  // Makes every row of Sigma valid on every rank (all-gather of the row panels, in column blocks) and re-partitions
  // the features so that the rows are balanced again.  Also the sync point before reading foreign rows of Sigma.
  int shard_rebalance() override {
    HIPCHK(hipSetDevice(device));
    if (!sh_on) FAIL(EKF_ERR_STATE, "ekf_shard_configure first");
    if (exchanges() && N > 0) {
      const ShardTab tab = row_tab();
      const int cw = 4096;                                 // column block: bounds the staging buffers
      const int vec = 16 / (int)sizeof(T);
      for (int c0 = 0; c0 < n; c0 += cw) {
        const int nc = round_up(std::min(cw, n - c0), vec);
        int rc = exchange_rows(S(), ld, tab, c0, nc, stream, KID_GATHER_SIGMA);
        if (rc) return rc;
      }
    }
    partition_by_rows();
    ++sh_rebalances;
    have_meas = false;
    return EKF_OK;
  }

  bool shard_needs_rebalance() const {
    if (sh_world == 1 || N == 0) return false;
    int mx = 0;
    for (int g = 0; g < sh_world; ++g) mx = std::max(mx, row_of_feature(sh_fb[g + 1]) - row_of_feature(sh_fb[g]));
    const double mean = double(n - camera_dim) / sh_world;
    return mx > sh_imbalance_limit * mean + 6.0;
  }

  int shard_predict(const void* tc, const void* rc_, int vcontrol) {
    if (shard_needs_rebalance()) { int rr = shard_rebalance(); if (rr) return rr; }
    int rc = sync_layout();
    if (rc) return rc;
    // rows 0..12 are replicated; the column strip of foreign rows works on stale data nobody reads
    rc = propagate(motion_args(tc, rc_, vcontrol), false);
    if (rc) return rc;
    const int f0 = own_f0(), f1 = own_f1();
    if (f1 > f0) {
      Scope sc(this, KID_MEASURE);
      k_measure<T><<<(f1 - f0 + 63) / 64, 64, 0, stream>>>(mu(), d_pos, d_coding, f0, f1, cam, d_h, d_Hc, d_Hf, d_flags);
    }
    HIPCHK(hipGetLastError());
    if (exchanges() && N > 0) {                            // "reassemble H": h, compact Jacobians, flags of every feature
      const ShardTab tab = feature_tab();
      int mx = 0;
      for (int g = 0; g < sh_world; ++g) mx = std::max(mx, tab.count[g]);
      const size_t slot = (size_t)mx * kFeatRec;
      rc = ensure_stage(slot);
      if (rc) return rc;
      Scope sc(this, KID_GATHER_H);
      if (f1 > f0)
        k_pack_features<T><<<((f1 - f0) * kFeatRec + 255) / 256, 256, 0, stream>>>(d_h, d_Hc, d_Hf, d_flags, f0, f1 - f0, d_stage_send);
      rc = all_gather(slot, stream);
      if (rc) return rc;
      k_unpack_features<T><<<dim3((mx * kFeatRec + 255) / 256, sh_world), 256, 0, stream>>>(d_stage_recv, slot, d_h, d_Hc, d_Hf, d_flags, tab);
      HIPCHK(hipGetLastError());
    }
    rc = launch_track_fold();                              // the flags of every feature are on every rank now
    if (rc) return rc;
    have_update = false;
    have_meas = true;
    have_sd = false;
    if (dbg_sync & 8) HIPCHK(hipDeviceSynchronize());
    return launch_blur();                                  // predicted blur of every template (replicated, like the templates)
  }

  // ---- the rank's launches of the sharded step, phase by phase ---------------------------
  // The rank's rows of the solve V_g = [W_g; nu_g^T] Z_gg of chunk gi on stream ss
  int shard_solve_chunk(const UpdatePlan& p, int gi, UpdateCtx& ux, hipStream_t ss) {
    const int c0 = p.c0(gi), width = p.c1(gi) - c0;
    const T* Zs = d_Y + (size_t)p.m_pad * ldy;
    GemmCall c;
    c.B = Zs + c0; c.ldb = ldy; c.lda = ldy; c.ldc = ldy;
    c.cols = width; c.K = width; c.ktri = KTRI_UPPER;
    c.two_groups = want_solve_s2(width, p.npad_live);
    c.st = ss;
    if constexpr (kIsF32) {
      if (opt_mfma && p.nb == 128 && p.prows > 0 && ux.queue_room()) {
        // camera block, own panel and innovation block as ONE queued launch of 64 x 128 tiles, heaviest column tiles first
        // (row tiles relative to the panel's first row; any tile shape adds the same terms in the same order)
        Scope sc(this, KID_SOLVE, ss);
        int rc = ensure_shard_solve_list(p.p0, p.prows, p.npad_live, p.ranges[0].count > 0);
        if (rc) return rc;
        const int wt = width / 128;
        const size_t off = (size_t)p.p0 * ldy;
        c.A = d_W + off + c0; c.C = d_V + off + c0; c.rows = p.prows;
        c.tile_list = shard_solve.d + 2 * (shard_ntc_max() - wt) * shard_solve_rows; c.ntiles = wt * shard_solve_rows;
        c.counter = ux.take_queue();
        gemm<ROLE_SOLVE, true, 64, 128>(c);
        return EKF_OK;
      }
    }
    for (const Rows& rr : p.ranges) {
      if (rr.count == 0) continue;
      const size_t off = (size_t)rr.r0 * ldy;
      Scope sc(this, KID_SOLVE, ss);
      c.A = d_W + off + c0; c.C = d_V + off + c0; c.rows = rr.count;
      gemm<ROLE_SOLVE, true>(c);
    }
    return EKF_OK;
  }

  // The rank's rows of the W update of chunk gi (needs the OWN rows of V_g only)
  void shard_wupdate_chunk(const UpdatePlan& p, int gi, hipStream_t ss) {
    const int c0 = p.c0(gi), c1 = p.c1(gi);
    for (const Rows& rr : p.ranges) {
      if (rr.count == 0) continue;
      const size_t off = (size_t)rr.r0 * ldy;
      Scope sc(this, KID_WUPDATE, ss);
      ++launch_cnt[EKF_LAUNCH_W_UPDATE_GEMM];
      GemmCall c;
      c.A = d_V + off + c0; c.lda = ldy; c.B = d_Y + (size_t)c1 * ldy + c0; c.ldb = ldy; c.C = d_W + off + c1; c.ldc = ldy;
      c.rows = rr.count; c.cols = p.m_pad - c1; c.K = c1 - c0; c.alpha = T(-1); c.beta = T(1);
      c.st = ss;
      gemm<ROLE_WUPDATE, false>(c);
    }
  }

  // The rank's rows of the downdate Sigma -= V_g V_g^T for columns [c0, c1) on stream ss (every row of V_g is here: the
  // gather is done), with the innovation row update of the chunk where it is still pending (ux.row_pending)
  int shard_downdate_chunk(const UpdatePlan& p, int c0, int c1, UpdateCtx& ux, hipStream_t ss) {
    const int m = p.m, m_pad = p.m_pad;
    const bool split = kIsF32 && p.shard_split && ux.queue_room();
    if (ux.row_pending && !split) {
      launch_row_update(c0, c1, m_pad, ss, true);
      ux.row_pending = false;
    }
    if (split) {
      // V_g -> plane image, then ONE launch over the canonical tiles that touch the camera block or an own block; each
      // element pair is the same sum as on the plain path
      const bool rider = ux.row_pending && shard_syrk_n > 0;
      int rcd = launch_downdate_bf16x6(ux, c0, c1, m_pad, ss, true, shard_syrk.d, shard_syrk_n, camera_dim, p.r0, p.r1,
                                       2.0 * 128 * 128 * shard_syrk_n * double(std::min(c1, m) - std::min(c0, m)), rider, false);
      if (rcd) return rcd;
      if (ux.row_pending && !rider) launch_row_update(c0, c1, m_pad, ss, true);
      ux.row_pending = false;
      return EKF_OK;
    }
    for (int q = 0; q < 2; ++q) {                        // Sigma[rows, :] -= V_g[rows] V_g^T: camera tile, own panel
      const Rows& rr = p.ranges[q];
      if (rr.count == 0) continue;
      Scope sc(this, KID_DOWNDATE, ss);
      ++launch_cnt[EKF_LAUNCH_DOWNDATE_F32];
      GemmCall c;
      c.A = d_V + (size_t)rr.r0 * ldy + c0; c.lda = ldy; c.B = d_V + c0; c.ldb = ldy; c.C = S() + (size_t)rr.r0 * ld; c.ldc = ld;
      c.rows = rr.count; c.cols = p.npad_live; c.K = c1 - c0; c.alpha = T(-1); c.beta = T(1);
      c.st = ss;
      if (q == 1 && p.sym_panel && ux.queue_room()) {
        // the own panel as ONE queued launch over the listed tiles: interior x interior lower tiles + mirror, the rest plain
        if (sc.on) prof.work[KID_DOWNDATE] += 2.0 * 128 * 128 * panel_ntiles * double(std::min(c1, m) - std::min(c0, m));
        c.tri = TRI_LISTED; c.row_off = rr.r0;
        c.tile_list = panel_tiles.d; c.ntiles = panel_ntiles; c.counter = ux.take_queue();
      } else if (sc.on) {
        prof.work[KID_DOWNDATE] += 2.0 * rr.count * double(n) * (std::min(c1, m) - std::min(c0, m));
      }
      gemm<ROLE_DOWNDATE, false>(c);
    }
    return EKF_OK;
  }

  // The sharded EKF update block for the measured list `idx` (host, strictly ascending), z resident on the device.
  int shard_update(const void* dz, const int* idx, int M, int plane) override {
    HIPCHK(hipSetDevice(device));
    if (!sh_on) FAIL(EKF_ERR_STATE, "ekf_shard_configure first");
    if (M < 0 || M > N) FAIL(EKF_ERR_ARG, "M out of range");
    if (M == 0 && !plane) return EKF_OK;
    if (!have_meas) FAIL(EKF_ERR_STATE, "the sharded update needs the h / H of the sharded predict");
    if (M > 0 && (!dz || !idx)) FAIL(EKF_ERR_ARG, "z / indices are NULL");
    int rc = check_list(idx, M, true);
    if (rc) return rc;
    if (M > 0 && ((int)sh_list.size() != M || memcmp(sh_list.data(), idx, (size_t)M * sizeof(int)) != 0)) {
      sh_list.assign(idx, idx + M);
      HIPCHK(hipMemcpyAsync(d_midx, sh_list.data(), (size_t)M * sizeof(int), hipMemcpyHostToDevice, stream));
    }
    UpdateCtx ux{static_cast<const T*>(dz), d_midx, d_counters};
    const UpdatePlan p = plan_update(M, plane);
    if (dbg_sync & 4) HIPCHK(hipDeviceSynchronize());
    // nu (replicated), W rows {camera, own}, own rows of S, "reassemble S"
    rc = shard_build_ws(idx, M, plane, ux.z, nullptr, nullptr);
    if (rc) return rc;
    if (p.sym_panel) { rc = ensure_panel_tiles(p.p0, p.prows, p.r0, p.r1, p.npad_live); if (rc) return rc; }

    // Replicated chain in column chunks; the rank's share of every chunk beside it:
    //   second stream (CU-masked):  solve V_g rows, W update rows, ... downdate of the PREVIOUS chunk
    //   gather stream:              all-gather of the own rows of V_g (needs the solve; the downdate needs it)
    // so a gather travels while the next chunk is being solved, and only the last chunk's solve -> gather -> downdate
    // is exposed after the chain.  With 1 / world of the GEMM work per rank many narrow chunks are affordable: the
    // exposed tail shrinks with the width of the last one.
    const int nchunks = p.nchunks, m_pad = p.m_pad;
    { Scope sc(this, KID_MISC);
      dim3 grid((m_pad + 255) / 256, p.strip_rows);
      k_set_identity_strip<T><<<grid, 256, 0, stream>>>(d_Y + (size_t)m_pad * ldy, ldy, m_pad, p.tab); }
    const ShardTab rtab = row_tab();
    if (p.shard_split) { rc = ensure_shard_syrk_list(p.r0, p.r1, p.npad_live); if (rc) return rc; }
    // Round 5: the SEQUENTIAL form of the chunked update on a rank too (EKF_OPT_W_RECOMPUTE, plan: recompute): after the
    // downdate of chunk g the rank re-evaluates ITS rows of W for chunk g + 1 from its downdated rows of Sigma (local: a
    // rank holds every column of its rows), instead of the right-looking GEMM update of all later columns (0.40 of 1.56 ms
    // per step at N = 1000 / world 1, 8.7 of 44 ms at N = 4000).  Per chunk the rank's second stream then runs solve ->
    // gather of V_g -> downdate -> W' in series; that order is off the critical path as soon as the replicated chain is
    // what a step waits for, which it is from two ranks on.
    const bool dchain = dist_chain_ok(p.nsteps);           // the factorisation distributed over the ranks (see dist_chain_steps)
    if (dchain) { rc = ensure_dist_plan(p.nsteps, nchunks, p.cend); if (rc) return rc; }
    rc = prepare_chain(p, ux, dchain);
    if (rc) return rc;
    bool side_busy = false;
    int pend_g = -1;                                       // overlapped chunk whose downdate is still to be issued
    for (int gi = 0; gi < nchunks; ++gi) {
      const int c0 = p.c0(gi), c1 = p.c1(gi), width = c1 - c0, step0 = gi ? p.cend[gi - 1] : 0;
      if (dchain) { rc = dist_chain_steps(ux, step0, p.cend[gi], p.m, m_pad, stream); if (rc) return rc; }
      else chain_steps(ux, step0, p.cend[gi], c0, c1, p.m, m_pad, stream, false, opt_chain_defer && gi + 1 < nchunks);
      const bool overlap = (gi + 1 < nchunks);
      hipStream_t ss = overlap ? stream_b : stream;
      if (overlap) {
        HIPCHK(hipEventRecord(ev_chain[gi], stream));
        HIPCHK(hipStreamWaitEvent(stream_b, ev_chain[gi], 0));
        side_busy = true;
      } else if (side_busy) {
        // the last chunk runs on the main stream: it needs every earlier W update (second stream) first
        HIPCHK(hipEventRecord(ev_b, stream_b));
        HIPCHK(hipStreamWaitEvent(stream, ev_b, 0));
      }
      rc = shard_solve_chunk(p, gi, ux, ss);
      if (rc) return rc;
      if (p.recompute) {
        // solve -> gather -> innovation row -> downdate -> W' of the next chunk, in this order on the chunk's stream
        if (overlap) {
          HIPCHK(hipEventRecord(ev_solve[gi], stream_b));
          HIPCHK(hipStreamWaitEvent(stream_g, ev_solve[gi], 0));
          rc = exchange_rows(d_V, ldy, rtab, c0, width, stream_g, KID_GATHER_V);
          if (rc) return rc;
          HIPCHK(hipEventRecord(ev_gath[gi], stream_g));
          HIPCHK(hipStreamWaitEvent(stream_b, ev_gath[gi], 0));
        } else {
          if (side_busy) {
            HIPCHK(hipEventRecord(ev_g, stream_g));
            HIPCHK(hipStreamWaitEvent(stream, ev_g, 0));
          }
          rc = exchange_rows(d_V, ldy, rtab, c0, width, stream, KID_GATHER_V);
          if (rc) return rc;
        }
        // nu^T[c1:] -= y_g^T L[c1:, g]^T (replicated, every rank): rides in the downdate's launch when there is one
        ux.row_pending = c1 < m_pad;
        rc = shard_downdate_chunk(p, c0, c1, ux, ss);
        if (rc) return rc;
        // W'[rows, c1:c2) = Sigma'[rows, :] H^T, rows = camera + own
        if (gi + 1 < nchunks) launch_w_recompute(c1, p.c1(gi + 1), m_pad, d_midx, M, plane, ss, camera_dim, p.r0, p.r1);
        if (dbg_sync & 2) HIPCHK(hipDeviceSynchronize());
        continue;
      }
      if (overlap) {
        // own rows of V_g are final: their gather starts now, on the gather stream ...
        HIPCHK(hipEventRecord(ev_solve[gi], stream_b));
        HIPCHK(hipStreamWaitEvent(stream_g, ev_solve[gi], 0));
        rc = exchange_rows(d_V, ldy, rtab, c0, width, stream_g, KID_GATHER_V);
        if (rc) return rc;
        HIPCHK(hipEventRecord(ev_gath[gi], stream_g));
      }
      if (c1 < m_pad) shard_wupdate_chunk(p, gi, ss);      // ... while the W update goes on
      if (pend_g >= 0) {                                   // the downdate of the previous chunk, behind this chunk's solve
        HIPCHK(hipStreamWaitEvent(stream_b, ev_gath[pend_g], 0));
        rc = shard_downdate_chunk(p, p.c0(pend_g), p.c1(pend_g), ux, stream_b);
        if (rc) return rc;
        pend_g = -1;
      }
      if (overlap) {
        pend_g = gi;
      } else {
        // last chunk, everything on the main stream: gather (the staging buffers are free once the gather stream has
        // drained), then its downdate behind every earlier one
        if (side_busy) {
          HIPCHK(hipEventRecord(ev_g, stream_g));
          HIPCHK(hipStreamWaitEvent(stream, ev_g, 0));
        }
        rc = exchange_rows(d_V, ldy, rtab, c0, width, stream, KID_GATHER_V);
        if (rc) return rc;
        if (side_busy) {
          HIPCHK(hipEventRecord(ev_b, stream_b));
          HIPCHK(hipStreamWaitEvent(stream, ev_b, 0));
        }
        rc = shard_downdate_chunk(p, c0, c1, ux, stream);
        if (rc) return rc;
      }
    }
    HIPCHK(hipGetLastError());
    rc = finish_update(p, true, true);                     // mu is replicated: every rank adds V y over all rows
    if (rc) return rc;
    if (dbg_sync & 1) HIPCHK(hipDeviceSynchronize());
    return EKF_OK;
  }

  // convert2XYZ_ifLinear(All) under sharding: the linearity index needs Sigma(rho, rho) -- known to the owner --
  // so every rank tests its own features and the flags are gathered before the (identical) compaction pass
  int shard_convert(int index, bool all) {
    if (!all && (index < 0 || index >= N)) { err = "feature index out of range"; return -EKF_ERR_ARG; }
    if (N == 0) return 0;
    int rc = sync_layout();
    if (rc) return -rc;
    k_linearity<T><<<(N + 127) / 128, 128, 0, stream>>>(mu(), S(), ld, d_pos, d_coding, N, d_cflag, d_Jy, d_Yxyz, 0);
    if (exchanges()) {
      const ShardTab tab = feature_tab();
      int mx = 0;
      for (int g = 0; g < sh_world; ++g) mx = std::max(mx, tab.count[g]);
      const size_t slot = (size_t)mx;
      rc = ensure_stage(slot);
      if (rc) return -rc;
      const int cnt = own_f1() - own_f0();
      if (cnt > 0) k_pack_flags<T><<<(cnt + 255) / 256, 256, 0, stream>>>(d_cflag, own_f0(), cnt, d_stage_send);
      rc = all_gather(slot, stream);
      if (rc) return -rc;
      k_unpack_flags<T><<<dim3((mx + 255) / 256, sh_world), 256, 0, stream>>>(d_stage_recv, slot, d_cflag, tab);
    }
    std::vector<unsigned char> fl(N);
    if (rb_add(fl.data(), d_cflag, N) != EKF_OK || rb_finish(false) != EKF_OK) { err = "linearity flags D2H failed"; return -EKF_ERR_DEVICE; }
    std::vector<char> rm(N, 0), cv(N, 0);
    int cnt = 0;
    for (int i = 0; i < N; ++i) {
      if (!all && i != index) continue;
      if (fl[i] && ft.coding(i) == 0) { cv[i] = 1; ++cnt; }
    }
    if (cnt == 0) return 0;
    rc = compact(rm, cv);
    if (rc) return -rc;
    return cnt;
  }

  int profile_read(int kid, double* ms, long long* cnt) override {
    if (kid < 0 || kid >= KID_COUNT) FAIL(EKF_ERR_ARG, "kernel id out of range");
    hipSetDevice(device);
    resolve_profile();
    prof.read(kid, ms, cnt);
    return EKF_OK;
  }
  bool last_recompute = false;
  int chunk_plan(int* ends, int max_chunks, int* block, int* wrec) override {
    if (block) *block = NB();
    if (wrec) *wrec = last_recompute ? 1 : 0;
    if (last_cend[0] == 0) return 0;                          // no update yet
    for (int g = 0; g < last_nchunks && g < max_chunks; ++g) if (ends) ends[g] = last_cend[g];
    return last_nchunks;
  }
  int profile_work(int kid, double* flop) override {
    if (kid < 0 || kid >= KID_COUNT) FAIL(EKF_ERR_ARG, "kernel id out of range");
    if (flop) *flop = prof.work[kid];
    return EKF_OK;
  }
  int profile_reset() override {
    hipSetDevice(device);
    resolve_profile();
    prof.reset();
    memset(launch_cnt, 0, sizeof(launch_cnt));
    return EKF_OK;
  }
};


// ---------------------------------------------------------------------------------------
// Bundle adjustment of the key-frame map: host side of ekf_sba_*.  The host keeps the problem
// (nodes, points, the (point, node)-sorted projections) and builds the index lists once per change of structure;
// ekf_sba_run uploads the state, runs the LM loop on its own stream and reads back one SbaResult per iteration.
// A change of validity (remove_bad, reduce_tracks) is a change of structure: the per-camera and pair lists hold
// valid projections only, so k_sba_rhs / k_sba_pairs / k_sba_diag need no flag test.
// ---------------------------------------------------------------------------------------
struct SbaProj {
  double u, v;
  bool valid;                                                // Proj::isValid
};

struct SbaSystem {
  std::string err;
  int device = 0;
  hipStream_t stream = nullptr;
  SbaCamera K{};
  int cap_nodes = 0, cap_points = 0, cap_prj = 0;
  std::vector<double> nodes, points;                         // 7 per node (t, q w x y z), 3 per point
  std::map<std::pair<int, int>, SbaProj> prj;                // (point, node) -> keypoint, validity
  double lambda = 1e-4;                                      // kept for continuation, as SysSBA::lambda
  double huber = 0.0;                                        // SysSBA::huber (sba.h:113), 0: plain squared error
  std::vector<double> log;                                   // 5 per iteration of the last run
  bool dirty = true;
  // solver: EKF_SBA_SOLVER_CHOLESKY or EKF_SBA_SOLVER_BPCG; the CG settings of doSBA (sba.h:158-159)
  int solver = EKF_SBA_SOLVER_CHOLESKY;
  double cg_tol = 1e-8;
  int cg_max = 100;
  double cg_residual = 0.0;                                  // jacobiBPCG::residual: dn / 2 of the last solve
  std::vector<double> cg_log;                                // 3 per iteration of the last run: CG iterations, dn, d0
  // profile (ekf_sba_profile): per phase and per iteration, milliseconds
  bool profile = false;
  double phase_ms[5] = {0, 0, 0, 0, 0};
  std::vector<double> iter_ms;
  hipEvent_t ev[6] = {};
  // device
  enum { B_NODES, B_OLDN, B_NM, B_PTS, B_OLDP, B_POFF, B_PNODE, B_PPOINT, B_UV, B_VALID, B_PRJ, B_TPS, B_COFF, B_CPRJ,
         B_PAIR_AB, B_PAIR_OFF, B_ITEMS, B_EMPTY, B_A, B_L, B_B, B_X, B_R, B_DX, B_DINV, B_PART, B_RES,
         B_PAIR_SLOT, B_BLK, B_J, B_ADJ_OFF, B_ADJ, B_Q, B_S, B_PART_DQ, B_PART_RS, B_COUNT };
  DevBuf<unsigned char> buf[B_COUNT];                        // sized in bytes
  int npairs = 0, nfree = 0, npad = 0, noff = 0;
  static constexpr int kCgChunk = 256;                       // CG rounds enqueued between two reads of the CG state
  bool pcg() const { return solver == EKF_SBA_SOLVER_BPCG; }
  SbaCg* dcg() { return reinterpret_cast<SbaCg*>(dp<SbaResult>(B_RES) + 1); }

  // (the buffers are members and go after this body, behind the stream: it is drained first)
  ~SbaSystem() {
    hipSetDevice(device);
    if (stream) hipStreamSynchronize(stream);
    for (auto& e : ev) if (e) hipEventDestroy(e);
    if (stream) hipStreamDestroy(stream);
  }
  template <typename T> T* dp(int i) { return reinterpret_cast<T*>(static_cast<unsigned char*>(buf[i])); }
  int ensure(int i, size_t bytes) {
    HIPCHK(buf[i].reserve(bytes ? bytes : 8));
    return EKF_OK;
  }
  int init(const ekf_sba_camera* cam, int cn, int cp, int cj, int dev, int slv) {
    device = dev;
    solver = slv;
    K = SbaCamera{cam->fx, cam->fy, cam->cx, cam->cy};
    cap_nodes = cn; cap_points = cp; cap_prj = cj;
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    for (auto& e : ev) HIPCHK(hipEventCreate(&e));
    HIPCHK(buf[B_RES].reserve(sizeof(SbaResult) + sizeof(SbaCg)));           // the CG state sits behind the result
    return EKF_OK;
  }
  int nn() const { return (int)nodes.size() / 7; }
  int np() const { return (int)points.size() / 3; }

  // structure: projection arrays in (point, node) order, per-camera lists, the pair lists; allocations
  int build() {
    const int P = (int)prj.size(), N = nn(), M = np();
    nfree = std::max(N - 1, 0);
    npad = (6 * nfree + 63) / 64 * 64;
    std::vector<int> poff(M + 1, 0), pnode(P), ppoint(P);
    std::vector<double> uv(2 * P);
    std::vector<unsigned char> valid(P);
    std::vector<std::vector<int>> cam(nfree);
    int k = 0;
    for (const auto& e : prj) {
      pnode[k] = e.first.second;
      ppoint[k] = e.first.first;
      uv[2 * k] = e.second.u;
      uv[2 * k + 1] = e.second.v;
      valid[k] = e.second.valid ? 1 : 0;
      ++poff[e.first.first + 1];
      if (e.second.valid && e.first.second > 0) cam[e.first.second - 1].push_back(k);
      ++k;
    }
    for (int p = 0; p < M; ++p) poff[p + 1] += poff[p];
    std::vector<int> coff(nfree + 1, 0), cprj, empty(std::max(nfree, 1), 0);
    for (int a = 0; a < nfree; ++a) {
      coff[a + 1] = coff[a] + (int)cam[a].size();
      cprj.insert(cprj.end(), cam[a].begin(), cam[a].end());
      empty[a] = cam[a].empty() ? 1 : 0;
    }
    std::map<std::pair<int, int>, std::vector<int>> pairs;
    for (int p = 0; p < M; ++p)
      for (int i = poff[p]; i < poff[p + 1]; ++i) {
        if (pnode[i] == 0 || !valid[i]) continue;
        for (int j = i; j < poff[p + 1]; ++j) {
          if (!valid[j]) continue;
          auto& v = pairs[{pnode[i] - 1, pnode[j] - 1}];
          v.push_back(i);
          v.push_back(j);
        }
      }
    npairs = (int)pairs.size();
    std::vector<int> pair_ab, pair_off(1, 0), items;
    for (const auto& e : pairs) {
      pair_ab.push_back(e.first.first);
      pair_ab.push_back(e.first.second);
      items.insert(items.end(), e.second.begin(), e.second.end());
      pair_off.push_back((int)items.size() / 2);
    }
    // PCG: the block slot of every pair and, per block row, the ascending (neighbour, slot, transposed) list
    std::vector<int> pair_slot, adj_off, adj;
    noff = 0;
    if (pcg()) {
      std::vector<std::vector<std::array<int, 3>>> rows(nfree);
      for (const auto& e : pairs) {                  // the map's order: (a, b) ascending, a <= b
        const int a = e.first.first, b = e.first.second;
        if (a == b) {
          pair_slot.push_back(a);
          continue;
        }
        const int slot = nfree + noff++;
        pair_slot.push_back(slot);
        rows[a].push_back({b, slot, 0});
        rows[b].push_back({a, slot, 1});
      }
      adj_off.assign(1, 0);
      for (auto& rw : rows) {
        std::sort(rw.begin(), rw.end());
        for (const auto& t : rw) adj.insert(adj.end(), t.begin(), t.end());
        adj_off.push_back((int)adj.size() / 3);
      }
    }
    const size_t D = sizeof(double), I = sizeof(int);
    int rc;
    if ((rc = ensure(B_NODES, 7 * D * N)) || (rc = ensure(B_OLDN, 7 * D * N)) || (rc = ensure(B_NM, kSbaNM * D * N)) ||
        (rc = ensure(B_PTS, 3 * D * M)) || (rc = ensure(B_OLDP, 3 * D * M)) || (rc = ensure(B_POFF, I * (M + 1))) ||
        (rc = ensure(B_PNODE, I * P)) || (rc = ensure(B_PPOINT, I * P)) || (rc = ensure(B_UV, 2 * D * P)) ||
        (rc = ensure(B_VALID, P)) ||
        (rc = ensure(B_PRJ, kSbaPR * D * P)) || (rc = ensure(B_TPS, 3 * D * M)) || (rc = ensure(B_COFF, I * coff.size())) ||
        (rc = ensure(B_CPRJ, I * cprj.size())) || (rc = ensure(B_PAIR_AB, I * pair_ab.size())) ||
        (rc = ensure(B_PAIR_OFF, I * pair_off.size())) || (rc = ensure(B_ITEMS, I * items.size())) ||
        (rc = ensure(B_EMPTY, I * empty.size())) || (rc = ensure(B_B, D * npad)) || (rc = ensure(B_X, D * npad)) ||
        (rc = ensure(B_R, D * npad)) || (rc = ensure(B_DX, D * npad)) ||
        (rc = ensure(B_PART, 3 * D * ((P + 255) / 256))))
      return rc;
    if (pcg()) {                                     // no dense matrix: the blocks, their inverses, the CG vectors
      const size_t nb = (size_t)nfree + noff, wg = (size_t)cg_blocks();
      if ((rc = ensure(B_PAIR_SLOT, I * pair_slot.size())) || (rc = ensure(B_BLK, 36 * D * nb)) ||
          (rc = ensure(B_J, 36 * D * nfree)) || (rc = ensure(B_ADJ_OFF, I * adj_off.size())) ||
          (rc = ensure(B_ADJ, I * adj.size())) || (rc = ensure(B_Q, D * npad)) || (rc = ensure(B_S, D * npad)) ||
          (rc = ensure(B_PART_DQ, D * wg)) || (rc = ensure(B_PART_RS, D * wg)))
        return rc;
    } else if ((rc = ensure(B_A, D * npad * npad)) || (rc = ensure(B_L, D * npad * npad)) ||
               (rc = ensure(B_DINV, D * 64 * 64))) {
      return rc;
    }
    auto up = [&](int i, const void* src, size_t bytes) -> int {
      if (bytes) HIPCHK(hipMemcpyAsync(buf[i], src, bytes, hipMemcpyHostToDevice, stream));
      return EKF_OK;
    };
    if ((rc = up(B_POFF, poff.data(), I * poff.size())) || (rc = up(B_PNODE, pnode.data(), I * P)) ||
        (rc = up(B_PPOINT, ppoint.data(), I * P)) || (rc = up(B_UV, uv.data(), 2 * D * P)) ||
        (rc = up(B_VALID, valid.data(), P)) ||
        (rc = up(B_COFF, coff.data(), I * coff.size())) || (rc = up(B_CPRJ, cprj.data(), I * cprj.size())) ||
        (rc = up(B_PAIR_AB, pair_ab.data(), I * pair_ab.size())) || (rc = up(B_PAIR_OFF, pair_off.data(), I * pair_off.size())) ||
        (rc = up(B_ITEMS, items.data(), I * items.size())) || (rc = up(B_EMPTY, empty.data(), I * empty.size())) ||
        (rc = up(B_PAIR_SLOT, pair_slot.data(), I * pair_slot.size())) ||
        (rc = up(B_ADJ_OFF, adj_off.data(), I * adj_off.size())) || (rc = up(B_ADJ, adj.data(), I * adj.size())))
      return rc;
    HIPCHK(hipStreamSynchronize(stream));          // the host vectors above go out of scope
    dirty = false;
    return EKF_OK;
  }
  int upload_state() {
    int rc;
    if (dirty && (rc = build())) return rc;
    HIPCHK(hipMemcpyAsync(buf[B_NODES], nodes.data(), sizeof(double) * nodes.size(), hipMemcpyHostToDevice, stream));
    if (!points.empty())
      HIPCHK(hipMemcpyAsync(buf[B_PTS], points.data(), sizeof(double) * points.size(), hipMemcpyHostToDevice, stream));
    return EKF_OK;
  }
  static int blocks(int n, int t = 256) { return (n + t - 1) / t; }
  int cg_blocks() const { return std::max(blocks(nfree, kSbaCgRows), 1); }
  // node matrices + the cost pass (dist2: the RMS cut) into B_RES
  int launch_cost(double dist2) {
    const int P = (int)prj.size();
    k_sba_node_prep<<<blocks(nn()), 256, 0, stream>>>(dp<double>(B_NODES), nn(), K, dp<double>(B_NM));
    k_sba_cost<<<blocks(P), 256, 0, stream>>>(dp<double>(B_NM), dp<double>(B_PTS), dp<int>(B_PNODE), dp<int>(B_PPOINT),
                                               dp<double>(B_UV), dp<unsigned char>(B_VALID), huber, P, dist2,
                                               dp<double>(B_PART));
    k_sba_cost_final<<<1, 256, 0, stream>>>(dp<double>(B_PART), blocks(P), dp<SbaResult>(B_RES));
    HIPCHK(hipGetLastError());
    return EKF_OK;
  }
  int read_result(SbaResult* r, SbaCg* cg = nullptr) {
    struct { SbaResult r; SbaCg cg; } both;        // one copy: the CG state sits behind the result
    HIPCHK(hipMemcpyAsync(&both, buf[B_RES], cg ? sizeof(both) : sizeof(SbaResult), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    *r = both.r;
    if (cg) *cg = both.cg;
    return EKF_OK;
  }
  int download_state() {
    HIPCHK(hipMemcpyAsync(nodes.data(), buf[B_NODES], sizeof(double) * nodes.size(), hipMemcpyDeviceToHost, stream));
    if (!points.empty())
      HIPCHK(hipMemcpyAsync(points.data(), buf[B_PTS], sizeof(double) * points.size(), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return EKF_OK;
  }
  int cost(double dist, double* sq, double* rms) {
    HIPCHK(hipSetDevice(device));
    if (prj.empty()) {
      if (sq) *sq = 0.0;
      if (rms) *rms = std::nan("");
      return EKF_OK;
    }
    int rc;
    SbaResult r{};
    if ((rc = upload_state()) || (rc = launch_cost(dist * dist)) || (rc = read_result(&r))) return rc;
    if (sq) *sq = r.cost;
    if (rms) *rms = std::sqrt(r.cost_in / r.n_in);
    return EKF_OK;
  }
  // countBad / removeBad (sba.cpp:416-462) on the Huber-weighted error at the current nodes and points.  Marking
  // clears the flags on the device; one copy of P bytes brings them back for the host's map and its lists.
  int flag_bad(double dist, bool mark_them, int* n) {
    *n = 0;
    if (prj.empty()) return EKF_OK;
    HIPCHK(hipSetDevice(device));
    const int P = (int)prj.size();
    int rc;
    SbaResult r{};
    if ((rc = upload_state())) return rc;
    k_sba_node_prep<<<blocks(nn()), 256, 0, stream>>>(dp<double>(B_NODES), nn(), K, dp<double>(B_NM));
    k_sba_flag_bad<<<blocks(P), 256, 0, stream>>>(dp<double>(B_NM), dp<double>(B_PTS), dp<int>(B_PNODE), dp<int>(B_PPOINT),
                                                   dp<double>(B_UV), dp<unsigned char>(B_VALID), huber, P, dist * dist,
                                                   mark_them ? 1 : 0, dp<double>(B_PART));
    k_sba_cost_final<<<1, 256, 0, stream>>>(dp<double>(B_PART), blocks(P), dp<SbaResult>(B_RES));
    HIPCHK(hipGetLastError());
    if ((rc = read_result(&r))) return rc;
    *n = (int)r.cost;
    if (mark_them && *n > 0) {
      std::vector<unsigned char> valid(P);
      HIPCHK(hipMemcpyAsync(valid.data(), buf[B_VALID], P, hipMemcpyDeviceToHost, stream));
      HIPCHK(hipStreamSynchronize(stream));
      int k = 0;
      for (auto& e : prj) e.second.valid = valid[k++] != 0;
      dirty = true;
    }
    return EKF_OK;
  }
  // reduceTracks (sba.cpp:467-502): erase the invalid projections; a point left with fewer than 2 loses them all
  int reduce_tracks() {
    const int M = np();
    std::vector<int> good(M, 0);
    for (auto it = prj.begin(); it != prj.end();) {
      if (it->second.valid) {
        ++good[it->first.first];
        ++it;
      } else {
        it = prj.erase(it);
        dirty = true;
      }
    }
    int cleared = 0;
    for (int p = 0; p < M; ++p) cleared += good[p] < 2 ? 1 : 0;
    for (auto it = prj.begin(); it != prj.end();) {
      if (good[it->first.first] < 2) {
        it = prj.erase(it);
        dirty = true;
      } else {
        ++it;
      }
    }
    return cleared;
  }
  // calcAvgError and numBadPoints (sba.cpp:365-411)
  int stats(double* avg, int* nbad) {
    if (avg) *avg = std::nan("");
    if (nbad) *nbad = 0;
    if (prj.empty()) return EKF_OK;
    HIPCHK(hipSetDevice(device));
    const int P = (int)prj.size();
    int rc;
    SbaResult r{};
    if ((rc = upload_state())) return rc;
    k_sba_node_prep<<<blocks(nn()), 256, 0, stream>>>(dp<double>(B_NODES), nn(), K, dp<double>(B_NM));
    k_sba_stats<<<blocks(P), 256, 0, stream>>>(dp<double>(B_NM), dp<double>(B_PTS), dp<int>(B_PNODE), dp<int>(B_PPOINT),
                                                dp<double>(B_UV), dp<unsigned char>(B_VALID), huber, P, dp<double>(B_PART));
    k_sba_cost_final<<<1, 256, 0, stream>>>(dp<double>(B_PART), blocks(P), dp<SbaResult>(B_RES));
    HIPCHK(hipGetLastError());
    if ((rc = read_result(&r))) return rc;
    if (avg) *avg = r.cost / r.cost_in;             // 0 / 0 without a valid projection, as the reference
    if (nbad) *nbad = (int)r.n_in;
    return EKF_OK;
  }
  void mark(int e) { if (profile) hipEventRecord(ev[e], stream); }

  // CSparse::doBPCG (csparse.cpp:383-395) on the block array: J, the head of doBPCG2, up to cg_max rounds of three
  // launches, |x|^2.  Up to kCgChunk rounds the whole solve is enqueued blind; the rounds after `dn < d0` return at
  // once on the device.  A larger cg_max is enqueued in chunks of kCgChunk rounds with one read of the CG state
  // between two chunks, so that a converged solve does not pay for thousands of idle launches.
  int solve_pcg(int sba_iter) {
    const int n6 = 6 * nfree, nb = cg_blocks();
    SbaResult* res = dp<SbaResult>(B_RES);
    SbaCg* cg = dcg();
    double *x = dp<double>(B_X), *rr = dp<double>(B_R), *d = dp<double>(B_DX), *q = dp<double>(B_Q), *sv = dp<double>(B_S);
    k_sba_blk_inv<<<blocks(nfree), 256, 0, stream>>>(dp<double>(B_BLK), nfree, dp<double>(B_J), res);
    k_sba_cg_step<true><<<nb, 256, 0, stream>>>(dp<double>(B_J), nullptr, 0, dp<double>(B_B), d, q, x, rr, sv, nfree,
                                                 dp<double>(B_PART_RS), cg);
    k_sba_cg_dir<true><<<blocks(n6), 256, 0, stream>>>(dp<double>(B_PART_RS), nb, sv, d, n6, cg, cg_tol,
                                                        sba_iter > 0 ? 1 : 0, cg_residual);
    for (int i0 = 0; i0 < cg_max; i0 += kCgChunk) {
      const int i1 = std::min(cg_max, i0 + kCgChunk);
      for (int i = i0; i < i1; ++i) {
        k_sba_cg_mv<<<nb, 256, 0, stream>>>(dp<double>(B_BLK), dp<int>(B_ADJ_OFF), dp<int>(B_ADJ), d, nfree, q,
                                            dp<double>(B_PART_DQ), cg, res);
        k_sba_cg_step<false><<<nb, 256, 0, stream>>>(dp<double>(B_J), dp<double>(B_PART_DQ), nb, nullptr, d, q, x, rr, sv,
                                                      nfree, dp<double>(B_PART_RS), cg);
        k_sba_cg_dir<false><<<blocks(n6), 256, 0, stream>>>(dp<double>(B_PART_RS), nb, sv, d, n6, cg, 0.0, 0, 0.0);
      }
      HIPCHK(hipGetLastError());
      if (i1 < cg_max) {
        SbaResult r{};
        SbaCg c{};
        int rc;
        if ((rc = read_result(&r, &c))) return rc;
        if (c.dn < c.d0 || r.status) break;
      }
    }
    k_sba_cg_end<<<1, 256, 0, stream>>>(x, n6, res);
    return EKF_OK;
  }

  // SysSBA::doSBA (sba.cpp:1312-1585)
  int run(int niter, double s_lambda, int* iterations) {
    log.clear();
    cg_log.clear();
    *iterations = -1;
    if (prj.empty() || points.empty() || nodes.empty()) return EKF_OK;
    HIPCHK(hipSetDevice(device));
    if (s_lambda > 0.0) lambda = s_lambda;
    int rc;
    SbaResult r{};
    if ((rc = upload_state()) || (rc = launch_cost(1e300)) || (rc = read_result(&r))) return rc;
    double cost = r.cost, laminc = 2.0;
    const int N = nn(), M = np(), n6 = 6 * nfree, P = (int)prj.size();
    int iter = 0;
    for (; iter < niter; ++iter) {
      if (nfree == 0) break;                       // B has no rows: |x|^2 = 0 < 1e-16 (sba.cpp:1425-1432)
      const double lam = 1.0 + lambda;
      mark(0);
      HIPCHK(hipMemsetAsync(&dp<SbaResult>(B_RES)->status, 0, sizeof(int), stream));
      k_sba_node_prep<<<blocks(N), 256, 0, stream>>>(dp<double>(B_NODES), N, K, dp<double>(B_NM));
      mark(1);
      k_sba_point<<<blocks(M), 256, 0, stream>>>(dp<double>(B_NM), dp<double>(B_NODES), dp<double>(B_PTS), dp<int>(B_POFF),
                                                  dp<int>(B_PNODE), dp<double>(B_UV), dp<unsigned char>(B_VALID), huber, M,
                                                  K, lam, dp<double>(B_PRJ), dp<double>(B_TPS));
      mark(2);
      if (!pcg()) HIPCHK(hipMemsetAsync(buf[B_A], 0, sizeof(double) * npad * npad, stream));
      k_sba_rhs<<<blocks(n6), 256, 0, stream>>>(dp<int>(B_COFF), dp<int>(B_CPRJ), dp<int>(B_PPOINT), dp<double>(B_PRJ),
                                                dp<double>(B_TPS), nfree, dp<double>(B_B));
      if (pcg()) {
        if (npairs)
          k_sba_pairs_blk<<<npairs, 64, 0, stream>>>(dp<int>(B_PAIR_AB), dp<int>(B_PAIR_OFF), dp<int>(B_ITEMS),
                                                     dp<double>(B_PRJ), dp<int>(B_PAIR_SLOT), dp<double>(B_BLK));
        k_sba_diag_blk<<<blocks(n6), 256, 0, stream>>>(dp<double>(B_BLK), n6, dp<int>(B_EMPTY), lam);
        mark(3);
        if ((rc = solve_pcg(iter))) return rc;
      } else {
        if (npairs)
          k_sba_pairs<<<npairs, 64, 0, stream>>>(dp<int>(B_PAIR_AB), dp<int>(B_PAIR_OFF), dp<int>(B_ITEMS), dp<double>(B_PRJ),
                                                 dp<double>(B_A), npad);
        k_sba_diag<<<blocks(npad), 256, 0, stream>>>(dp<double>(B_A), npad, n6, npad, dp<int>(B_EMPTY), lam);
        HIPCHK(hipMemcpyAsync(buf[B_L], buf[B_A], sizeof(double) * npad * npad, hipMemcpyDeviceToDevice, stream));
        mark(3);
        sba_chol_f64(dp<double>(B_L), npad, npad, dp<double>(B_DINV), &dp<SbaResult>(B_RES)->status, stream);
        k_sba_trsv<<<1, 1024, 0, stream>>>(dp<double>(B_L), npad, n6, dp<double>(B_B), dp<double>(B_X));
        k_sba_resid<<<blocks(n6, 4), 256, 0, stream>>>(dp<double>(B_A), npad, n6, dp<double>(B_X), dp<double>(B_B),
                                                        dp<double>(B_R));
        k_sba_trsv<<<1, 1024, 0, stream>>>(dp<double>(B_L), npad, n6, dp<double>(B_R), dp<double>(B_DX));
        k_sba_refine<<<1, 256, 0, stream>>>(dp<double>(B_X), dp<double>(B_DX), n6, dp<SbaResult>(B_RES));
      }
      mark(4);
      k_sba_update_nodes<<<blocks(N), 256, 0, stream>>>(dp<double>(B_NODES), dp<double>(B_OLDN), N, dp<double>(B_X),
                                                         dp<SbaResult>(B_RES));
      k_sba_update_points<<<blocks(M), 256, 0, stream>>>(dp<double>(B_PTS), dp<double>(B_OLDP), M, dp<double>(B_TPS),
                                                          dp<int>(B_POFF), dp<int>(B_PNODE), dp<unsigned char>(B_VALID),
                                                          dp<double>(B_PRJ), dp<double>(B_X), dp<SbaResult>(B_RES));
      if ((rc = launch_cost(1e300))) return rc;
      mark(5);
      SbaCg cgr{};
      if ((rc = read_result(&r, pcg() ? &cgr : nullptr))) return rc;       // the one read-back of the iteration
      if (pcg()) {
        cg_residual = cgr.dn / 2.0;                // bpcg.h:314; kept in the handle, as CSparse keeps its jacobiBPCG
        const double crow[3] = {double(cgr.iters), cgr.dn, cgr.d0};
        cg_log.insert(cg_log.end(), crow, crow + 3);
      }
      if (profile) {
        float ms[5], tot = 0.f;
        for (int e = 0; e < 5; ++e) {
          HIPCHK(hipEventElapsedTime(&ms[e], ev[e], ev[e + 1]));
          phase_ms[e] += ms[e];
          tot += ms[e];
        }
        iter_ms.push_back(tot);
      }
      if (r.status) {
        *iterations = iter;                        // the iterations completed before the failed factor
        if ((rc = download_state())) return rc;
        if (pcg()) FAIL(EKF_ERR_NUMERIC, "ekf_sba_run: a diagonal block of the reduced camera system has a non-positive pivot");
        FAIL(EKF_ERR_NUMERIC, "ekf_sba_run: the reduced camera system has a non-positive pivot");
      }
      if (r.x2 < 1e-16) break;                     // converged: no update was made (a NaN step goes on and is rejected)
      const double before = cost, newcost = r.cost;
      int acc;
      if (newcost < cost) {
        cost = newcost;
        lambda *= 0.5;
        acc = 1;
      } else {
        lambda *= laminc;
        laminc *= 2.0;
        HIPCHK(hipMemcpyAsync(buf[B_NODES], buf[B_OLDN], sizeof(double) * 7 * N, hipMemcpyDeviceToDevice, stream));
        HIPCHK(hipMemcpyAsync(buf[B_PTS], buf[B_OLDP], sizeof(double) * 3 * M, hipMemcpyDeviceToDevice, stream));
        acc = 0;                                   // the restored state's cost is `cost` (same kernels, same data)
      }
      const double row[5] = {before, newcost, lambda, double(acc), r.x2};
      log.insert(log.end(), row, row + 5);
    }
    (void)P;
    *iterations = iter;
    return download_state();
  }
};

}  // namespace ekf

// =============================================================================================
// C ABI
// =============================================================================================
using ekf::FilterBase;

struct ekf_filter { FilterBase* impl; };

extern "C" {

void ekf_config_default(ekf_config* c) {
  if (!c) return;
  memset(c, 0, sizeof(*c));
  c->sigma_vx = c->sigma_vy = c->sigma_vz = 0.01f;                 // ConfigVSLAM.cpp:27-28
  c->sigma_wx = c->sigma_wy = c->sigma_wz = 0.01f;
  c->window_size = 21; c->sigma_pixel = 2;                          // :30-31
  c->rho_0 = 0.1f; c->sigma_rho_0 = 0.25f;                          // :33-34
  c->scale = 1; c->T_camera = 0.5f; c->sigma_size = 2;              // :36-40
  c->nInitFeatures = 5; c->min_features = 30; c->max_features = 100; c->forsePlane = 0;   // :42-47
  c->kernel_size = 0;
  c->fx = 592.2860f; c->fy = 584.9968f; c->u0 = 362.1059f; c->v0 = 275.9642f;            // camModel.hpp:22-31
  c->k1 = -0.3954f; c->k2 = 0.5521f; c->k3 = 0.f; c->p1 = -0.0075f; c->p2 = 0.0140f;
  c->image_width = 640; c->image_height = 480;
}

int ekf_abi_version(void) { return EKF_ABI_VERSION; }

static bool sba_finite(const double* v, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

// K = (fx, fy, cx, cy): finite with fx, fy > 0
static bool pinhole_ok(const double* K) { return sba_finite(K, 4) && K[0] > 0.0 && K[1] > 0.0; }

// What every create checks before it makes a handle: `device` names a HIP device.
static int create_device(const char* who, int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
    ekf::g_create_error = std::string(who) + ": no HIP device (this library has no CPU fallback)";
    return EKF_ERR_DEVICE;
  }
  return EKF_OK;
}

int ekf_create(const ekf_config* cfg, int camera_dim, int capacity_features, int dtype, int device,
               ekf_filter** out) {
  if (!out) return EKF_ERR_ARG;
  *out = nullptr;
  if (!cfg || (camera_dim != 13 && camera_dim != 14) || capacity_features < 0 ||
      (dtype != EKF_F32 && dtype != EKF_F64)) {
    ekf::g_create_error = "ekf_create: bad argument";
    return EKF_ERR_ARG;
  }
  int rc = create_device("ekf_create", device);
  if (rc != EKF_OK) return rc;
  FilterBase* impl = nullptr;
  if (dtype == EKF_F32) {
    auto* f = new ekf::Filter<float>();
    rc = f->init(cfg, camera_dim, capacity_features, device);
    impl = f;
  } else {
    auto* f = new ekf::Filter<double>();
    rc = f->init(cfg, camera_dim, capacity_features, device);
    impl = f;
  }
  if (rc != EKF_OK) {
    ekf::g_create_error = impl->err;
    delete impl;
    return rc;
  }
  *out = new ekf_filter{impl};
  return EKF_OK;
}

void ekf_destroy(ekf_filter* f) {
  if (!f) return;
  delete f->impl;
  delete f;
}

const char* ekf_last_error(const ekf_filter* f) {
  if (!f) return ekf::g_create_error.c_str();
  return f->impl->err.c_str();
}

#define IMPL_OR_ARG(f) \
  if (!(f)) return EKF_ERR_ARG
// entry points that change mu, Sigma, the layout or the sharding: the gathered diagonal blocks are stale afterwards
#define MUTATES(f) (f)->impl->diag_synced = false

int ekf_set_dt(ekf_filter* f, double dT) { IMPL_OR_ARG(f); return f->impl->set_dt(dT); }
double ekf_get_dt(const ekf_filter* f) { return f ? f->impl->get_dt() : 0.0; }
int ekf_set_stream(ekf_filter* f, void* s) { IMPL_OR_ARG(f); return f->impl->set_stream(s); }
int ekf_set_option(ekf_filter* f, int o, int v) { IMPL_OR_ARG(f); MUTATES(f); return f->impl->set_option(o, v); }
int ekf_synchronize(ekf_filter* f) { IMPL_OR_ARG(f); return f->impl->synchronize(); }

int ekf_add_feature(ekf_filter* f, double u, double v) { if (!f) return -EKF_ERR_ARG; MUTATES(f); return f->impl->add_feature(u, v); }
int ekf_remove_feature(ekf_filter* f, int index) { IMPL_OR_ARG(f); MUTATES(f); return f->impl->remove_features(&index, 1); }
int ekf_remove_features(ekf_filter* f, const int* idx, int count) {
  IMPL_OR_ARG(f); MUTATES(f);
  if (count > 0 && !idx) return EKF_ERR_ARG;
  return f->impl->remove_features(idx, count);
}

int ekf_predict(ekf_filter* f, const void* t, const void* r, int vc) { IMPL_OR_ARG(f); MUTATES(f); return f->impl->predict(t, r, vc); }
int ekf_measure(ekf_filter* f) { IMPL_OR_ARG(f); return f->impl->measure(); }
int ekf_get_motion_jacobian(ekf_filter* f, void* Ft, void* Q) { IMPL_OR_ARG(f); return f->impl->motion_jacobian(Ft, Q); }
int ekf_get_predictions(ekf_filter* f, void* h, unsigned char* vis, unsigned char* rem, void* s2, void* hc, void* hf) {
  IMPL_OR_ARG(f);
  return f->impl->get_predictions(h, vis, rem, s2, hc, hf);
}
int ekf_update(ekf_filter* f, const void* z, const int* idx, int M, int plane) {
  IMPL_OR_ARG(f); MUTATES(f);
  return f->impl->update(z, idx, M, plane, false);
}
int ekf_update_device(ekf_filter* f, const void* dz, const int* didx, int M, int plane) {
  IMPL_OR_ARG(f); MUTATES(f);
  return f->impl->update(dz, didx, M, plane, true);
}
int ekf_innovation_covariance(ekf_filter* f, const int* idx, int M, int plane, void* out) {
  IMPL_OR_ARG(f);
  if (!out) return EKF_ERR_ARG;
  return f->impl->innovation_covariance(idx, M, plane, out);
}
int ekf_get_gain(ekf_filter* f, void* out) { IMPL_OR_ARG(f); if (!out) return EKF_ERR_ARG; return f->impl->get_gain(out); }
int ekf_last_measurement_rows(const ekf_filter* f) { return f ? f->impl->last_rows() : 0; }

int ekf_convert_xyz_if_linear(ekf_filter* f, int index) { if (!f) return -EKF_ERR_ARG; MUTATES(f); return f->impl->convert(index, false); }
int ekf_convert_xyz_if_linear_all(ekf_filter* f) { if (!f) return -EKF_ERR_ARG; MUTATES(f); return f->impl->convert(0, true); }

int ekf_num_features(const ekf_filter* f) { return f ? f->impl->num_features() : 0; }
int ekf_state_dim(const ekf_filter* f) { return f ? f->impl->state_dim() : 0; }
int ekf_get_feature_layout(const ekf_filter* f, int* p, int* c) { IMPL_OR_ARG(f); return f->impl->get_layout(p, c); }

int ekf_get_state(ekf_filter* f, void* out, int off, int cnt) { IMPL_OR_ARG(f); if (cnt > 0 && !out) return EKF_ERR_ARG; return f->impl->get_state(out, off, cnt); }
int ekf_set_state(ekf_filter* f, const void* in, int off, int cnt) { IMPL_OR_ARG(f); MUTATES(f); if (cnt > 0 && !in) return EKF_ERR_ARG; return f->impl->set_state(in, off, cnt); }
int ekf_peek_workspace(ekf_filter* f, int which, void* out, int r0, int c0, int rows, int cols) {
  IMPL_OR_ARG(f);
  return f->impl->peek_work(which, out, r0, c0, rows, cols);
}
int ekf_get_sigma_block(ekf_filter* f, void* out, int r0, int c0, int rows, int cols) {
  IMPL_OR_ARG(f);
  if (!out) return EKF_ERR_ARG;
  return f->impl->get_sigma(out, r0, c0, rows, cols);
}
int ekf_set_sigma_block(ekf_filter* f, const void* in, int r0, int c0, int rows, int cols) {
  IMPL_OR_ARG(f); MUTATES(f);
  if (!in) return EKF_ERR_ARG;
  return f->impl->set_sigma(in, r0, c0, rows, cols);
}
int ekf_covariance_parameter(ekf_filter* f, double* out) { IMPL_OR_ARG(f); if (!out) return EKF_ERR_ARG; return f->impl->covariance_parameter(out); }
int ekf_check_invariants(ekf_filter* f, double* pad, double* asym, double* big) { IMPL_OR_ARG(f); return f->impl->check_invariants(pad, asym, big); }
int ekf_feature_xyz(ekf_filter* f, int index, void* xyz, void* cov) { IMPL_OR_ARG(f); return f->impl->feature_xyz(index, xyz, cov); }

int ekf_profile_kernels(void) { return ekf::KID_COUNT; }
const char* ekf_profile_kernel_name(int kid) { return (kid >= 0 && kid < ekf::KID_COUNT) ? ekf::kKernelNames[kid] : ""; }
int ekf_profile_read(ekf_filter* f, int kid, double* ms, long long* cnt) { IMPL_OR_ARG(f); return f->impl->profile_read(kid, ms, cnt); }
int ekf_profile_reset(ekf_filter* f) { IMPL_OR_ARG(f); return f->impl->profile_reset(); }
int ekf_launch_kinds(void) { return EKF_LAUNCH_KINDS; }
const char* ekf_launch_kind_name(int kind) { return (kind >= 0 && kind < EKF_LAUNCH_KINDS) ? ekf::kLaunchNames[kind] : ""; }
int ekf_launch_count(ekf_filter* f, int kind, long long* launches) {
  IMPL_OR_ARG(f);
  if (kind < 0 || kind >= EKF_LAUNCH_KINDS) { f->impl->err = "launch kind out of range"; return EKF_ERR_ARG; }
  if (launches) *launches = f->impl->launch_cnt[kind];
  return EKF_OK;
}
int ekf_profile_work(ekf_filter* f, int kid, double* flop) { IMPL_OR_ARG(f); return f->impl->profile_work(kid, flop); }
int ekf_get_chunk_plan(ekf_filter* f, int* ends, int max_chunks, int* block, int* w_recompute) {
  if (!f || !f->impl) return 0;
  return f->impl->chunk_plan(ends, max_chunks, block, w_recompute);
}

int ekf_rescue_high_innovation(ekf_filter* f, const void* cam, const void* z, const int* idx, int M, double thr,
                               unsigned char* out) {
  IMPL_OR_ARG(f);
  return f->impl->rescue(cam, z, idx, M, thr, out);
}
int ekf_set_frame(ekf_filter* f, const unsigned char* gray, int width, int height, int stride) {
  IMPL_OR_ARG(f);
  return f->impl->set_frame(gray, width, height, stride);
}
int ekf_set_frame_raw(ekf_filter* f, const unsigned char* pixels, int width, int height, int channels, int stride) {
  IMPL_OR_ARG(f);
  return f->impl->set_frame_raw(pixels, width, height, channels, stride, false);
}
int ekf_set_frame_raw_device(ekf_filter* f, const void* d_pixels, int width, int height, int channels, int stride) {
  IMPL_OR_ARG(f);
  return f->impl->set_frame_raw(d_pixels, width, height, channels, stride, true);
}
int ekf_get_frame(ekf_filter* f, unsigned char* gray, int stride) { IMPL_OR_ARG(f); return f->impl->get_frame(gray, stride); }
int ekf_rectified_camera(const ekf_filter* f, int raw, ekf_sba_camera* K) { IMPL_OR_ARG(f); return f->impl->rectified_camera(raw, K); }
int ekf_get_frame_rectified(ekf_filter* f, int raw, unsigned char* out, int stride) {
  IMPL_OR_ARG(f);
  return f->impl->get_frame_rectified(raw, out, stride);
}
int ekf_undistort_pixels(ekf_filter* f, int raw, const double* uv, int n, double* out) {
  IMPL_OR_ARG(f);
  return f->impl->undistort_pixels(raw, uv, n, out);
}
int ekf_set_patch(ekf_filter* f, int index, const unsigned char* pixels) { IMPL_OR_ARG(f); return f->impl->set_patch(index, pixels); }
int ekf_get_patch(ekf_filter* f, int index, int matching, unsigned char* out) {
  IMPL_OR_ARG(f);
  return f->impl->get_patch(index, matching, out);
}
int ekf_get_blur_predictions(ekf_filter* f, void* hb) { IMPL_OR_ARG(f); return f->impl->blur_predictions(hb); }
int ekf_find_matches(ekf_filter* f, double threshold, void* z, unsigned char* found, float* score) {
  IMPL_OR_ARG(f);
  return f->impl->find_matches(threshold, z, found, score);
}
int ekf_get_feature_track(ekf_filter* f, int* n_tot, unsigned char* in_innovation, float* center, unsigned char* remove_flag) {
  IMPL_OR_ARG(f);
  return f->impl->get_track(n_tot, in_innovation, center, remove_flag);
}
int ekf_set_feature_track(ekf_filter* f, int index, int n_tot, int in_innovation, const float* center, int remove_flag) {
  IMPL_OR_ARG(f);
  return f->impl->set_track(index, n_tot, in_innovation, center, remove_flag);
}
int ekf_find_new_features(ekf_filter* f, int num, double quality_level, double min_distance, int add, float* out_uv,
                          int* n_out) {
  IMPL_OR_ARG(f);
  if (add) MUTATES(f);
  return f->impl->find_new_features(num, quality_level, min_distance, add, out_uv, n_out);
}
int ekf_end_update(ekf_filter* f, float matching_ratio, int seed, int* removed, int* n_removed, int* n_visible,
                   int* n_seeded) {
  IMPL_OR_ARG(f);
  MUTATES(f);
  return f->impl->end_update(matching_ratio, seed, removed, n_removed, n_visible, n_seeded);
}
int ekf_export_points(ekf_filter* f, void* out, int conv) { IMPL_OR_ARG(f); if (!out) return EKF_ERR_ARG; return f->impl->export_points(out, conv); }
int ekf_export_points_table(ekf_filter* f, void* out, int max_rows, int* rows) { IMPL_OR_ARG(f); return f->impl->export_points_table(out, max_rows, rows); }
int ekf_get_feature_ids(const ekf_filter* f, int* real_index, int* n_find) { IMPL_OR_ARG(f); return f->impl->feature_ids(real_index, n_find); }
int ekf_set_feature_meta(ekf_filter* f, int index, int real_index, int n_find) { IMPL_OR_ARG(f); return f->impl->set_feature_meta(index, real_index, n_find); }
int ekf_num_archived(const ekf_filter* f) { return f ? f->impl->num_archived() : 0; }
int ekf_get_search_ellipses(ekf_filter* f, int sigma_size, int* out) { IMPL_OR_ARG(f); if (!out) return EKF_ERR_ARG; return f->impl->search_ellipses(sigma_size, out); }
int ekf_ransac_1point(ekf_filter* f, const void* z, const int* idx, int M, double thr, int* counts,
                      unsigned char* inl, int* best) {
  IMPL_OR_ARG(f);
  return f->impl->ransac(z, idx, M, thr, counts, inl, best);
}
int ekf_update_two_stage(ekf_filter* f, const void* z, const int* idx, int M, int plane, unsigned int seed,
                         double thr, double chi2, unsigned char* is_li, unsigned char* is_hi, int* drawn) {
  IMPL_OR_ARG(f); MUTATES(f);
  if (M > 0 && (!z || !idx)) return EKF_ERR_ARG;
  return f->impl->update_two_stage(z, idx, M, plane, seed, thr, chi2, is_li, is_hi, drawn);
}
int ekf_shard_configure(ekf_filter* f, int rank, int world, ekf_allgather_fn fn, void* ctx) {
  IMPL_OR_ARG(f); MUTATES(f);
  return f->impl->shard_configure(rank, world, fn, ctx);
}
int ekf_shard_get_info(ekf_filter* f, ekf_shard_info* out) { IMPL_OR_ARG(f); return f->impl->shard_info(out); }
int ekf_shard_update(ekf_filter* f, const void* dz, const int* idx, int M, int plane) {
  IMPL_OR_ARG(f); MUTATES(f);
  return f->impl->shard_update(dz, idx, M, plane);
}
int ekf_shard_rebalance(ekf_filter* f) { IMPL_OR_ARG(f); MUTATES(f); return f->impl->shard_rebalance(); }

void* ekf_device_mu(ekf_filter* f) { return f ? f->impl->dev_mu() : nullptr; }
void* ekf_device_sigma(ekf_filter* f, int* ld) { return f ? f->impl->dev_sigma(ld) : nullptr; }

// ---- bundle adjustment --------------------------------------------------
struct ekf_sba {
  ekf::SbaSystem* impl;
};

// The node capacity of a PCG handle: 64 * capacity_nodes (above the 52 doubles of node matrices per node and the 6
// rows per node) must fit in int; the block and vector offsets themselves are size_t.
static const int kSbaMaxNodesPcg = INT_MAX / 64;

static int sba_create(const char* who, const ekf_sba_camera* K, int capacity_nodes, int capacity_points,
                      int capacity_projections, int device, int solver, ekf_sba** out) {
  if (!out) return EKF_ERR_ARG;
  *out = nullptr;
  if (solver != EKF_SBA_SOLVER_CHOLESKY && solver != EKF_SBA_SOLVER_BPCG) {
    ekf::g_create_error = std::string(who) + ": solver must be EKF_SBA_SOLVER_CHOLESKY (0) or EKF_SBA_SOLVER_BPCG (3)";
    return EKF_ERR_ARG;
  }
  const int max_nodes = solver == EKF_SBA_SOLVER_BPCG ? kSbaMaxNodesPcg : ekf::kSbaMaxN / 6;
  if (!K || !pinhole_ok(&K->fx) || capacity_nodes < 1 || capacity_nodes > max_nodes || capacity_points < 1 ||
      capacity_projections < 1) {
    ekf::g_create_error = std::string(who) + ": bad argument (K finite with fx, fy > 0; 1 <= capacity_nodes <= " +
                          std::to_string(max_nodes) + "; capacities >= 1)";
    return EKF_ERR_ARG;
  }
  int rc = create_device(who, device);
  if (rc != EKF_OK) return rc;
  auto* s = new ekf::SbaSystem();
  rc = s->init(K, capacity_nodes, capacity_points, capacity_projections, device, solver);
  if (rc != EKF_OK) {
    ekf::g_create_error = s->err;
    delete s;
    return rc;
  }
  *out = new ekf_sba{s};
  return EKF_OK;
}

int ekf_sba_create(const ekf_sba_camera* K, int capacity_nodes, int capacity_points, int capacity_projections,
                   int device, ekf_sba** out) {
  return sba_create("ekf_sba_create", K, capacity_nodes, capacity_points, capacity_projections, device,
                    EKF_SBA_SOLVER_CHOLESKY, out);
}

int ekf_sba_create_solver(const ekf_sba_camera* K, int capacity_nodes, int capacity_points, int capacity_projections,
                          int device, int solver, ekf_sba** out) {
  return sba_create("ekf_sba_create_solver", K, capacity_nodes, capacity_points, capacity_projections, device, solver,
                    out);
}

int ekf_sba_get_solver(const ekf_sba* s, int* solver) {
  if (!s || !solver) return EKF_ERR_ARG;
  *solver = s->impl->solver;
  return EKF_OK;
}

int ekf_sba_set_cg(ekf_sba* s, double init_tol, int max_iters) {
  if (!s) return EKF_ERR_ARG;
  if (!std::isfinite(init_tol) || init_tol < 0.0 || max_iters < 1) {
    s->impl->err = "ekf_sba_set_cg: init_tol must be finite and >= 0, max_iters >= 1";
    return EKF_ERR_ARG;
  }
  s->impl->cg_tol = init_tol;
  s->impl->cg_max = max_iters;
  return EKF_OK;
}

int ekf_sba_get_cg(const ekf_sba* s, double* init_tol, int* max_iters) {
  if (!s) return EKF_ERR_ARG;
  if (init_tol) *init_tol = s->impl->cg_tol;
  if (max_iters) *max_iters = s->impl->cg_max;
  return EKF_OK;
}

int ekf_sba_get_cg_log(const ekf_sba* s, int max_rows, int* cg_iters, double* dn_final, double* d0, int* n) {
  if (!s || !n || max_rows < 0) return EKF_ERR_ARG;
  const std::vector<double>& l = s->impl->cg_log;
  const int total = (int)l.size() / 3;
  *n = total;
  for (int i = 0; i < std::min(total, max_rows); ++i) {
    if (cg_iters) cg_iters[i] = (int)l[3 * i];
    if (dn_final) dn_final[i] = l[3 * i + 1];
    if (d0) d0[i] = l[3 * i + 2];
  }
  return EKF_OK;
}

void ekf_sba_destroy(ekf_sba* s) {
  if (!s) return;
  delete s->impl;
  delete s;
}

const char* ekf_sba_last_error(const ekf_sba* s) {
  if (!s) return ekf::g_create_error.c_str();
  return s->impl->err.c_str();
}

int ekf_sba_add_nodes(ekf_sba* s, int n, const double* pose7) {
  if (!s) return EKF_ERR_ARG;
  auto* q = s->impl;
  if (n < 0 || (n > 0 && !pose7) || !sba_finite(pose7, 7 * n)) {
    q->err = "ekf_sba_add_nodes: n >= 0 finite poses (x y z qw qx qy qz)";
    return EKF_ERR_ARG;
  }
  if (q->nn() + n > q->cap_nodes) {
    q->err = "ekf_sba_add_nodes: capacity_nodes exceeded";
    return EKF_ERR_CAPACITY;
  }
  for (int i = 0; i < n; ++i) {
    const double* p = pose7 + 7 * i;
    // Node::normRot (node.cpp:52-66)
    double v[3] = {p[4], p[5], p[6]};
    if (p[3] < 0) { v[0] = -v[0]; v[1] = -v[1]; v[2] = -v[2]; }
    const double sn = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    if (sn >= 0.9999) {
      const double f = -1.0 / (std::sqrt(sn) * 1.0001);
      v[0] *= f; v[1] *= f; v[2] *= f;
    }
    const double w = std::sqrt(1.0 - (v[0] * v[0] + v[1] * v[1] + v[2] * v[2]));
    const double rec[7] = {p[0], p[1], p[2], w, v[0], v[1], v[2]};
    q->nodes.insert(q->nodes.end(), rec, rec + 7);
  }
  if (n) q->dirty = true;
  return EKF_OK;
}

int ekf_sba_add_points(ekf_sba* s, int n, const double* xyz) {
  if (!s) return EKF_ERR_ARG;
  auto* q = s->impl;
  if (n < 0 || (n > 0 && !xyz) || !sba_finite(xyz, 3 * n)) {
    q->err = "ekf_sba_add_points: n >= 0 finite points";
    return EKF_ERR_ARG;
  }
  if (q->np() + n > q->cap_points) {
    q->err = "ekf_sba_add_points: capacity_points exceeded";
    return EKF_ERR_CAPACITY;
  }
  q->points.insert(q->points.end(), xyz, xyz + 3 * n);
  if (n) q->dirty = true;
  return EKF_OK;
}

int ekf_sba_add_projections(ekf_sba* s, int n, const int* node, const int* point, const double* uv, int* added) {
  if (!s) return EKF_ERR_ARG;
  auto* q = s->impl;
  if (added) *added = 0;
  if (n < 0 || (n > 0 && (!node || !point || !uv))) {
    q->err = "ekf_sba_add_projections: bad argument";
    return EKF_ERR_ARG;
  }
  for (int i = 0; i < n; ++i)
    if (node[i] < 0 || node[i] >= q->nn() || point[i] < 0 || point[i] >= q->np() || !sba_finite(uv + 2 * i, 2)) {
      q->err = "ekf_sba_add_projections: node / point index out of range or keypoint not finite";
      return EKF_ERR_ARG;
    }
  // count the new pairs first: the call is all or nothing
  std::map<std::pair<int, int>, int> fresh;
  for (int i = 0; i < n; ++i) {
    const std::pair<int, int> key{point[i], node[i]};
    if (!q->prj.count(key)) fresh.emplace(key, i);
  }
  if ((long long)q->prj.size() + (long long)fresh.size() > q->cap_prj) {
    q->err = "ekf_sba_add_projections: capacity_projections exceeded";
    return EKF_ERR_CAPACITY;
  }
  int cnt = 0;
  for (int i = 0; i < n; ++i) {
    // addMonoProj (sba.cpp:133-143): a repeat of (node, point) keeps the first keypoint
    auto r = q->prj.emplace(std::pair<int, int>{point[i], node[i]}, ekf::SbaProj{uv[2 * i], uv[2 * i + 1], true});
    cnt += r.second ? 1 : 0;
  }
  if (cnt) q->dirty = true;
  if (added) *added = cnt;
  return EKF_OK;
}

int ekf_sba_counts(const ekf_sba* s, int* nodes, int* points, int* projections) {
  if (!s) return EKF_ERR_ARG;
  if (nodes) *nodes = s->impl->nn();
  if (points) *points = s->impl->np();
  if (projections) *projections = (int)s->impl->prj.size();
  return EKF_OK;
}

int ekf_sba_run(ekf_sba* s, int niter, double lambda, int* iterations) {
  if (!s) return EKF_ERR_ARG;
  if (!iterations) {
    s->impl->err = "ekf_sba_run: iterations must not be NULL";
    return EKF_ERR_ARG;
  }
  if (niter < 0 || std::isnan(lambda) || std::isinf(lambda)) {
    s->impl->err = "ekf_sba_run: niter >= 0, lambda finite";
    return EKF_ERR_ARG;
  }
  return s->impl->run(niter, lambda, iterations);
}

int ekf_sba_cost(ekf_sba* s, double dist, double* sq_cost, double* rms) {
  if (!s) return EKF_ERR_ARG;
  if (!(dist > 0.0)) {
    s->impl->err = "ekf_sba_cost: dist must be > 0";
    return EKF_ERR_ARG;
  }
  return s->impl->cost(dist, sq_cost, rms);
}

int ekf_sba_set_huber(ekf_sba* s, double huber) {
  if (!s) return EKF_ERR_ARG;
  if (!std::isfinite(huber) || huber < 0.0) {
    s->impl->err = "ekf_sba_set_huber: huber must be finite and >= 0 (0 switches the weighting off)";
    return EKF_ERR_ARG;
  }
  s->impl->huber = huber;
  return EKF_OK;
}

int ekf_sba_get_huber(const ekf_sba* s, double* huber) {
  if (!s || !huber) return EKF_ERR_ARG;
  *huber = s->impl->huber;
  return EKF_OK;
}

int ekf_sba_count_bad(ekf_sba* s, double dist, int* n) {
  if (!s) return EKF_ERR_ARG;
  if (!n || !(dist > 0.0)) {
    s->impl->err = "ekf_sba_count_bad: dist must be > 0 and n not NULL";
    return EKF_ERR_ARG;
  }
  return s->impl->flag_bad(dist, false, n);
}

int ekf_sba_remove_bad(ekf_sba* s, double dist, int* n) {
  if (!s) return EKF_ERR_ARG;
  if (!n || !(dist > 0.0)) {
    s->impl->err = "ekf_sba_remove_bad: dist must be > 0 and n not NULL";
    return EKF_ERR_ARG;
  }
  return s->impl->flag_bad(dist, true, n);
}

int ekf_sba_reduce_tracks(ekf_sba* s, int* cleared) {
  if (!s) return EKF_ERR_ARG;
  if (!cleared) {
    s->impl->err = "ekf_sba_reduce_tracks: cleared must not be NULL";
    return EKF_ERR_ARG;
  }
  *cleared = s->impl->reduce_tracks();
  return EKF_OK;
}

int ekf_sba_num_bad_points(ekf_sba* s, int* n) {
  if (!s) return EKF_ERR_ARG;
  if (!n) {
    s->impl->err = "ekf_sba_num_bad_points: n must not be NULL";
    return EKF_ERR_ARG;
  }
  return s->impl->stats(nullptr, n);
}

int ekf_sba_avg_error(ekf_sba* s, double* avg) {
  if (!s) return EKF_ERR_ARG;
  if (!avg) {
    s->impl->err = "ekf_sba_avg_error: avg must not be NULL";
    return EKF_ERR_ARG;
  }
  return s->impl->stats(avg, nullptr);
}

int ekf_sba_get_projections(const ekf_sba* s, int max_rows, int* node, int* point, double* uv, unsigned char* valid,
                            int* n) {
  if (!s || !n || max_rows < 0) return EKF_ERR_ARG;
  *n = (int)s->impl->prj.size();
  int k = 0;
  for (const auto& e : s->impl->prj) {
    if (k >= max_rows) break;
    if (node) node[k] = e.first.second;
    if (point) point[k] = e.first.first;
    if (uv) { uv[2 * k] = e.second.u; uv[2 * k + 1] = e.second.v; }
    if (valid) valid[k] = e.second.valid ? 1 : 0;
    ++k;
  }
  return EKF_OK;
}

int ekf_sba_get_nodes(const ekf_sba* s, double* pose7) {
  if (!s || (!pose7 && s->impl->nn())) return EKF_ERR_ARG;
  std::copy(s->impl->nodes.begin(), s->impl->nodes.end(), pose7);
  return EKF_OK;
}

int ekf_sba_get_points(const ekf_sba* s, double* xyz) {
  if (!s || (!xyz && s->impl->np())) return EKF_ERR_ARG;
  std::copy(s->impl->points.begin(), s->impl->points.end(), xyz);
  return EKF_OK;
}

int ekf_sba_get_log(const ekf_sba* s, int max_rows, double* rows, int* n) {
  if (!s || !n || max_rows < 0 || (max_rows > 0 && !rows)) return EKF_ERR_ARG;
  const int total = (int)s->impl->log.size() / 5;
  *n = total;
  const int m = std::min(total, max_rows);
  std::copy(s->impl->log.begin(), s->impl->log.begin() + 5 * m, rows);
  return EKF_OK;
}

int ekf_sba_profile(ekf_sba* s, int enable) {
  if (!s) return EKF_ERR_ARG;
  s->impl->profile = enable != 0;
  for (double& v : s->impl->phase_ms) v = 0.0;
  s->impl->iter_ms.clear();
  return EKF_OK;
}

int ekf_sba_get_profile(const ekf_sba* s, double* phase_ms, int max_iters, double* iter_ms, int* n) {
  if (!s || !phase_ms || !n || max_iters < 0 || (max_iters > 0 && !iter_ms)) return EKF_ERR_ARG;
  std::copy(s->impl->phase_ms, s->impl->phase_ms + 5, phase_ms);
  const int total = (int)s->impl->iter_ms.size();
  *n = total;
  std::copy(s->impl->iter_ms.begin(), s->impl->iter_ms.begin() + std::min(total, max_iters), iter_ms);
  return EKF_OK;
}

// ---- key-frame selection -----------------------------------------------------------------------------
struct ekf_keyframe { ekf::KfSelector* impl; };

static int keyframe_create(const ekf_filter* f, float move_thresh, int raw_w, int raw_h, int raw_c, ekf_keyframe** out) {
  if (!out) return EKF_ERR_ARG;
  *out = nullptr;
  if (!f || !(move_thresh > 0.f) || !std::isfinite(move_thresh)) {
    ekf::g_create_error = "ekf_keyframe_create: a filter and a finite move_thresh > 0";
    return EKF_ERR_ARG;
  }
  auto* k = new ekf::KfSelector();
  k->owner = f->impl;
  k->move_thresh = move_thresh;
  k->raw_w = raw_w; k->raw_h = raw_h; k->raw_c = raw_c;
  const int rc = f->impl->kf_create(k);
  if (rc != EKF_OK) {
    ekf::g_create_error = f->impl->err;
    delete k;
    return rc;
  }
  *out = new ekf_keyframe{k};
  return EKF_OK;
}

int ekf_keyframe_create(const ekf_filter* f, float move_thresh, ekf_keyframe** out) {
  return keyframe_create(f, move_thresh, 0, 0, 0, out);
}

int ekf_keyframe_create_raw(const ekf_filter* f, float move_thresh, int raw_width, int raw_height, int channels,
                            ekf_keyframe** out) {
  if (out && (raw_width <= 0 || raw_height <= 0 || (channels != 1 && channels != 3))) {
    *out = nullptr;
    ekf::g_create_error = "ekf_keyframe_create_raw: raw_width, raw_height > 0 and 1 or 3 channels";
    return EKF_ERR_ARG;
  }
  return keyframe_create(f, move_thresh, raw_width, raw_height, channels, out);
}

void ekf_keyframe_destroy(ekf_keyframe* s) {
  if (!s) return;
  delete s->impl;
  delete s;
}

const char* ekf_keyframe_last_error(const ekf_keyframe* s) {
  if (!s) return ekf::g_create_error.c_str();
  return s->impl->err.c_str();
}

int ekf_keyframe_set_option(ekf_keyframe* s, int option, int value) {
  if (!s) return EKF_ERR_ARG;
  if (option != EKF_KF_OPT_KEEP_CURRENT_PROJECTIONS || (value != 0 && value != 1)) {
    s->impl->err = "ekf_keyframe_set_option: unknown option, or a value other than 0 / 1";
    return EKF_ERR_ARG;
  }
  s->impl->keep_current = value;
  return EKF_OK;
}

int ekf_keyframe_observe(ekf_keyframe* s, ekf_filter* f, int frame_id, int* action, float* dist, float* cov) {
  if (!s || !f) return EKF_ERR_ARG;
  auto* k = s->impl;
  if (!action || frame_id < 0) {
    k->err = "ekf_keyframe_observe: action must not be NULL and frame_id >= 0";
    return EKF_ERR_ARG;
  }
  if (k->owner != f->impl) {
    k->err = "ekf_keyframe_observe: the selector was created for another filter";
    return EKF_ERR_ARG;
  }
  ekf::KfRecord r{};
  const int rc = f->impl->kf_observe(k, frame_id, &r);
  if (rc != EKF_OK) {
    k->err = f->impl->err;
    return rc;
  }
  *action = r.action;
  if (dist) *dist = r.dist;
  if (cov) *cov = r.cov;
  return EKF_OK;
}

int ekf_keyframe_get_emitted(const ekf_keyframe* s, int* id, double* pose7, double* cov49, int max_rows, int* prj_rows,
                             int* n_rows) {
  if (!s) return EKF_ERR_ARG;
  auto* k = s->impl;
  if (max_rows < 0 || (max_rows > 0 && !prj_rows)) {
    k->err = "ekf_keyframe_get_emitted: max_rows >= 0, and prj_rows with it";
    return EKF_ERR_ARG;
  }
  if (!k->have_emit) {
    k->err = "ekf_keyframe_get_emitted: no key frame was emitted yet";
    return EKF_ERR_STATE;
  }
  if (id) *id = k->emitted.id;
  if (pose7) for (int i = 0; i < 7; ++i) pose7[i] = k->emitted.pose[i];
  if (cov49) for (int r = 0; r < 7; ++r) for (int c = 0; c < 7; ++c) cov49[c * 7 + r] = k->emitted.sig[r * 7 + c];
  const int total = (int)k->emit_rows.size() / 3;
  if (n_rows) *n_rows = total;
  std::copy(k->emit_rows.begin(), k->emit_rows.begin() + 3 * std::min(total, max_rows), prj_rows);
  return EKF_OK;
}

int ekf_keyframe_get_image(const ekf_keyframe* s, unsigned char* gray, int stride) {
  if (!s) return EKF_ERR_ARG;
  auto* k = s->impl;
  if (!gray || stride < k->img_w) {
    k->err = "ekf_keyframe_get_image: gray must not be NULL and stride >= image_width";
    return EKF_ERR_ARG;
  }
  if (!k->have_emit || !k->emit_has_image) {
    k->err = "ekf_keyframe_get_image: no emitted key frame with an image (ekf_set_frame before ekf_keyframe_observe)";
    return EKF_ERR_STATE;
  }
  std::string& err = k->err;
  HIPCHK(hipSetDevice(k->device));
  HIPCHK(hipMemcpy2D(gray, (size_t)stride, k->d_emit, (size_t)k->img_w, (size_t)k->img_w, (size_t)k->img_h, hipMemcpyDeviceToHost));
  return EKF_OK;
}

int ekf_keyframe_get_raw_image(const ekf_keyframe* s, unsigned char* pixels, int stride) {
  if (!s) return EKF_ERR_ARG;
  auto* k = s->impl;
  if (!pixels || stride < k->raw_w * k->raw_c) {
    k->err = "ekf_keyframe_get_raw_image: pixels must not be NULL and stride >= raw_width * channels";
    return EKF_ERR_ARG;
  }
  if (!k->have_emit || !k->emit_has_raw) {
    k->err = "ekf_keyframe_get_raw_image: no emitted key frame with a raw image (ekf_keyframe_create_raw, and ekf_set_frame_raw "
             "before ekf_keyframe_observe)";
    return EKF_ERR_STATE;
  }
  std::string& err = k->err;
  const size_t row = (size_t)k->raw_w * k->raw_c;
  HIPCHK(hipSetDevice(k->device));
  HIPCHK(hipMemcpy2D(pixels, (size_t)stride, k->d_emit_raw, row, row, (size_t)k->raw_h, hipMemcpyDeviceToHost));
  return EKF_OK;
}

// The rectified getters of a selector run on the default stream, as the copies of get_image / get_raw_image
// do: the selector may outlive its filter, and observe has synchronised the launch that filled the emit slots.
int ekf_keyframe_get_image_rectified(const ekf_keyframe* s, int raw, unsigned char* out, int stride) {
  if (!s) return EKF_ERR_ARG;
  auto* k = s->impl;
  const int W = raw ? k->raw_w : k->img_w, H = raw ? k->raw_h : k->img_h, Cn = raw ? k->raw_c : 1;
  if ((raw != 0 && raw != 1) || !out || (W > 0 && (long long)stride < (long long)W * Cn)) {
    k->err = "ekf_keyframe_get_image_rectified: raw is 0 or 1, out must not be NULL and stride >= a row of that resolution";
    return EKF_ERR_ARG;
  }
  if (!k->have_emit || !(raw ? k->emit_has_raw : k->emit_has_image) || (raw && k->scale < 1)) {
    k->err = raw ? "ekf_keyframe_get_image_rectified: no emitted key frame with a raw image (ekf_keyframe_create_raw, and "
                   "ekf_set_frame_raw before ekf_keyframe_observe)"
                 : "ekf_keyframe_get_image_rectified: no emitted key frame with an image (ekf_set_frame before ekf_keyframe_observe)";
    return EKF_ERR_STATE;
  }
  std::string& err = k->err;
  HIPCHK(hipSetDevice(k->device));
  HIPCHK(ekf::rectify_launch(k->rect, nullptr, raw ? k->d_emit_raw : k->d_emit, W, H, Cn, ekf::rect_cam(k->cam, raw ? k->scale : 1)));
  HIPCHK(ekf::rectified_to_host(k->rect, nullptr, W, H, Cn, out, (size_t)stride));
  return EKF_OK;
}

int ekf_keyframe_get_emitted_rectified(const ekf_keyframe* s, int raw, int max_rows, double* uv, int* rows) {
  if (!s) return EKF_ERR_ARG;
  auto* k = s->impl;
  if ((raw != 0 && raw != 1) || max_rows < 0 || (max_rows > 0 && !uv)) {
    k->err = "ekf_keyframe_get_emitted_rectified: raw is 0 or 1, max_rows >= 0, and uv with it";
    return EKF_ERR_ARG;
  }
  if (!k->have_emit) {
    k->err = "ekf_keyframe_get_emitted_rectified: no key frame was emitted yet";
    return EKF_ERR_STATE;
  }
  if (raw && (k->raw_w <= 0 || k->scale < 1)) {
    k->err = "ekf_keyframe_get_emitted_rectified: not a raw selector (ekf_keyframe_create_raw): the raw geometry is unknown";
    return EKF_ERR_STATE;
  }
  const int total = (int)k->emit_uv.size() / 2;             // the "0 0 0" placeholder carries no coordinates: 0 rows
  if (rows) *rows = total;
  const int n = std::min(total, max_rows);
  if (n == 0) return EKF_OK;
  std::vector<double> in(k->emit_uv.begin(), k->emit_uv.begin() + 2 * (size_t)n);
  if (raw) {                                                 // the track centres are matcher pixels: X = (u + 0.5) s - 0.5
#pragma clang fp contract(off)
    for (double& x : in) x = (x + 0.5) * (double)k->scale - 0.5;
  }
  std::string& err = k->err;
  HIPCHK(hipSetDevice(k->device));
  HIPCHK(ekf::undistort_to_host(k->rect, nullptr, in.data(), n, ekf::rect_cam(k->cam, raw ? k->scale : 1), uv));
  return EKF_OK;
}

int ekf_keyframe_get_state(const ekf_keyframe* s, float* last_pose7, float* last_vrot3, float* min_cov, int* candidate_id) {
  if (!s) return EKF_ERR_ARG;
  auto* k = s->impl;
  std::string& err = k->err;
  ekf::KfState st;
  HIPCHK(hipSetDevice(k->device));
  HIPCHK(hipMemcpy(&st, k->d_state + k->parity, sizeof(st), hipMemcpyDeviceToHost));
  if (last_pose7) std::copy(st.last_pose, st.last_pose + 7, last_pose7);
  if (last_vrot3) std::copy(st.last_vrot, st.last_vrot + 3, last_vrot3);
  if (min_cov) *min_cov = st.min_cov;
  if (candidate_id) *candidate_id = st.cand_id;
  return EKF_OK;
}

int ekf_keyframe_reset(ekf_keyframe* s) {
  if (!s) return EKF_ERR_ARG;
  auto* k = s->impl;
  std::string& err = k->err;
  const ekf::KfState s0 = ekf::KfSelector::initial();
  HIPCHK(hipSetDevice(k->device));
  HIPCHK(hipMemcpy(k->d_state + k->parity, &s0, sizeof(s0), hipMemcpyHostToDevice));
  k->cand_rows.clear();
  k->emit_rows.clear();
  k->cand_uv.clear();
  k->emit_uv.clear();
  k->cand_has_image = k->emit_has_image = k->have_emit = false;
  k->cand_has_raw = k->emit_has_raw = false;
  k->emitted = ekf::KfRecord{};
  return EKF_OK;
}


// ---- dense plane-sweep depth maps ----------------------------------------------------------------------
struct ekf_dense {
  ekf::DenseStereo* impl;
  ekf::DenseSgm sgm;                  // the cost volumes of the semi-global sweep
  ekf::DenseSpeckle speckle;          // the segment planes of the speckle filter
};

int ekf_dense_create(int width, int height, int max_views, int device, ekf_dense** out) {
  if (!out) return EKF_ERR_ARG;
  *out = nullptr;
  if (width < 1 || height < 1 || width > ekf::kDenseMaxDim || height > ekf::kDenseMaxDim || max_views < 1 ||
      max_views > ekf::kDenseMaxViews) {
    ekf::g_create_error = "ekf_dense_create: 1 <= width, height <= 8192 and 1 <= max_views <= 16";
    return EKF_ERR_ARG;
  }
  const int rc = create_device("ekf_dense_create", device);
  if (rc != EKF_OK) return rc;
  auto* d = new ekf::DenseStereo();
  d->device = device;
  d->W = width;
  d->H = height;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = d->timer.create();
  if (e == hipSuccess) e = d->census_timer.create();
  if (e == hipSuccess) e = d->best_timer.create();
  if (e == hipSuccess) e = d->unique_timer.create();
  auto* h = new ekf_dense{d, {}, {}};
  if (e == hipSuccess) e = h->sgm.timer.create();
  if (e == hipSuccess) e = h->speckle.timer.create();
  if (e != hipSuccess) {
    ekf::g_create_error = std::string("ekf_dense_create: ") + hipGetErrorString(e);
    delete h;
    delete d;
    return EKF_ERR_DEVICE;
  }
  d->max_views = max_views;
  d->v.resize((size_t)max_views);
  *out = h;
  return EKF_OK;
}

void ekf_dense_destroy(ekf_dense* h) {
  if (!h) return;
  delete h->impl;
  delete h;
}

const char* ekf_dense_last_error(const ekf_dense* h) {
  if (!h) return ekf::g_create_error.c_str();
  return h->impl->err.c_str();
}

// slot in range, K finite with fx, fy > 0 (when given), pose7 a pose: what every set_view* checks before the device
static int dense_view_args(ekf::DenseStereo* d, const char* who, int slot, const double* K, const double* pose7, double t[3],
                           double R[9], double q[4]) {
  if (slot < 0 || slot >= d->max_views || !pose7 || !ekf::dense_pose(pose7, t, R, q) || (K && !pinhole_ok(K))) {
    d->err = std::string(who) + ": slot in 0..max_views-1, K finite with fx, fy > 0, pose7 finite with q != 0";
    return EKF_ERR_ARG;
  }
  return EKF_OK;
}

static void dense_commit(ekf::DenseView& v, const double* K, const double t[3], const double R[9], const double q[4]) {
  if (K) std::copy(K, K + 4, v.K);
  std::copy(q, q + 4, v.q);
  std::copy(t, t + 3, v.t);
  std::copy(R, R + 9, v.R);
  v.swept = v.filtered = v.sgm = v.has_runner = v.seg = false;
}

// ---- setting a view, grey (C = 1) or colour (C = 3; DESIGN.md §18.1: the slot keeps the B, G, R image, its grey image is
// k_bgr_to_grey of it).  What every setter does to its slot round the fill.  dense_view_begin: the device, the buffers, the
// slot unset, where the fill goes.  dense_view_end: the grey image of a colour one, K and the pose, the slot set.
static hipError_t dense_view_begin(ekf::DenseStereo* d, ekf::DenseView& v, int C, unsigned char** dst) {
  hipError_t e = hipSetDevice(d->device);
  if (e == hipSuccess) e = v.img.reserve(d->npix());
  if (e == hipSuccess && C == 3) e = v.bgr.reserve(3 * d->npix());
  if (e != hipSuccess) return e;
  v.set = v.colour = v.sgm = v.census_valid = false;
  *dst = C == 3 ? (unsigned char*)v.bgr : (unsigned char*)v.img;
  return hipSuccess;
}

static hipError_t dense_view_end(ekf::DenseStereo* d, ekf::DenseView& v, int C, const double* K, const double t[3], const double R[9],
                                 const double q[4]) {
  const hipError_t e = C == 3 ? d->grey_from_colour(v) : hipSuccess;
  if (e != hipSuccess) return e;
  dense_commit(v, K, t, R, q);
  v.set = true;
  v.colour = C == 3;
  return hipSuccess;
}

// An image from the host, or from the device without a host synchronisation: rows of C W bytes, `pitch` apart.
static int dense_set_view(ekf_dense* h, const char* who, int C, int slot, const void* img, int pitch, const double* K,
                          const double* pose7, bool device_src) {
  if (!h) return EKF_ERR_ARG;
  auto* d = h->impl;
  double t[3], R[9], q[4];
  if (!img || !K || pitch < C * d->W) {
    d->err = std::string(who) + (C == 3 ? ": bgr and K must not be NULL and pitch >= 3 width"
                                        : ": img and K must not be NULL and pitch >= width");
    return EKF_ERR_ARG;
  }
  const int rc = dense_view_args(d, who, slot, K, pose7, t, R, q);
  if (rc != EKF_OK) return rc;
  std::string& err = d->err;
  ekf::DenseView& v = d->v[slot];
  const size_t row = (size_t)C * d->W;
  unsigned char* dst;
  HIPCHK(dense_view_begin(d, v, C, &dst));
  if (device_src)
    HIPCHK(hipMemcpy2DAsync(dst, row, img, (size_t)pitch, row, (size_t)d->H, hipMemcpyDeviceToDevice, nullptr));
  else
    HIPCHK(hipMemcpy2D(dst, row, img, (size_t)pitch, row, (size_t)d->H, hipMemcpyHostToDevice));
  HIPCHK(dense_view_end(d, v, C, K, t, R, q));
  return EKF_OK;
}

int ekf_dense_set_view(ekf_dense* h, int slot, const unsigned char* img, int pitch, const double* K, const double* pose7) {
  return dense_set_view(h, "ekf_dense_set_view", 1, slot, img, pitch, K, pose7, false);
}

int ekf_dense_set_view_device(ekf_dense* h, int slot, const void* d_img, int pitch, const double* K, const double* pose7) {
  return dense_set_view(h, "ekf_dense_set_view_device", 1, slot, d_img, pitch, K, pose7, true);
}

int ekf_dense_set_view_colour(ekf_dense* h, int slot, const unsigned char* bgr, int pitch, const double* K, const double* pose7) {
  return dense_set_view(h, "ekf_dense_set_view_colour", 3, slot, bgr, pitch, K, pose7, false);
}

int ekf_dense_set_view_colour_device(ekf_dense* h, int slot, const void* d_bgr, int pitch, const double* K, const double* pose7) {
  return dense_set_view(h, "ekf_dense_set_view_colour_device", 3, slot, d_bgr, pitch, K, pose7, true);
}

// The emitted key frame of a selector, rectified straight into the slot: its image (raw = 0) or its raw image (raw = 1) of one
// channel, or its raw image of three (C = 3, where raw is 1).  K is the rectified camera at that resolution.
static int dense_set_view_from_keyframe(ekf_dense* h, int C, int slot, const ekf_keyframe* selector, int raw, const double* pose7) {
  if (!h) return EKF_ERR_ARG;
  auto* d = h->impl;
  const bool colour = C == 3;
  const char* who = colour ? "ekf_dense_set_view_colour_from_keyframe" : "ekf_dense_set_view_from_keyframe";
  double t[3], R[9], q[4];
  if (!selector || (raw != 0 && raw != 1)) {
    d->err = std::string(who) + (colour ? ": a selector" : ": a selector, and raw is 0 or 1");
    return EKF_ERR_ARG;
  }
  const int rc = dense_view_args(d, who, slot, nullptr, pose7, t, R, q);
  if (rc != EKF_OK) return rc;
  auto* k = selector->impl;
  const int W = raw ? k->raw_w : k->img_w, H = raw ? k->raw_h : k->img_h;
  if (W != d->W || H != d->H || (raw && k->raw_c != C) || k->device != d->device) {
    d->err = std::string(who) + (colour ? ": the selector's raw image must have the handle's size, three channels and the handle's device"
                                        : ": the selector's image at that resolution must have the handle's size, one channel and the "
                                          "handle's device");
    return EKF_ERR_ARG;
  }
  if (!k->have_emit || !(raw ? k->emit_has_raw : k->emit_has_image) || (raw && k->scale < 1)) {
    d->err = std::string(who) + (colour ? ": no emitted key frame with a raw image (the rules of ekf_keyframe_get_raw_image)"
                                        : ": no emitted key frame with such an image (the rules of ekf_keyframe_get_image / "
                                          "ekf_keyframe_get_raw_image)");
    return EKF_ERR_STATE;
  }
  std::string& err = d->err;
  ekf::DenseView& v = d->v[slot];
  unsigned char* dst;
  HIPCHK(dense_view_begin(d, v, C, &dst));
  const ekf::RectCam c = ekf::rect_cam(k->cam, raw ? k->scale : 1);
  const ekf::RectifyArgs a{raw ? k->d_emit_raw : k->d_emit, dst, W, H, c};
  const int grid = (int)std::min<size_t>((d->npix() + 255) / 256, 1024);
  if (colour)
    ekf::k_frame_rectify<3><<<grid, 256, 0, nullptr>>>(a);
  else
    ekf::k_frame_rectify<1><<<grid, 256, 0, nullptr>>>(a);
  HIPCHK(hipGetLastError());
  double K[4];
  ekf::rect_camera(c, K);
  HIPCHK(dense_view_end(d, v, C, K, t, R, q));
  return EKF_OK;
}

int ekf_dense_set_view_from_keyframe(ekf_dense* h, int slot, const ekf_keyframe* selector, int raw, const double* pose7) {
  return dense_set_view_from_keyframe(h, 1, slot, selector, raw, pose7);
}

int ekf_dense_set_view_colour_from_keyframe(ekf_dense* h, int slot, const ekf_keyframe* selector, const double* pose7) {
  return dense_set_view_from_keyframe(h, 3, slot, selector, 1, pose7);
}

// The slot's grey image with K and pose (C = 1) or its colour image (C = 3; K and pose7 NULL).  out == NULL only asks.
static int dense_get_view(const ekf_dense* h, int C, int slot, unsigned char* out, int pitch, double* K, double* pose7) {
  if (!h) return EKF_ERR_ARG;
  auto* d = h->impl;
  const bool colour = C == 3;
  if (slot < 0 || slot >= d->max_views || (out && pitch < C * d->W)) {
    d->err = colour ? "ekf_dense_get_view_colour: slot in 0..max_views-1 and pitch >= 3 width"
                    : "ekf_dense_get_view: slot in 0..max_views-1 and pitch >= width";
    return EKF_ERR_ARG;
  }
  const ekf::DenseView& v = d->v[slot];
  if (!v.set || (colour && !v.colour)) {
    d->err = colour ? "ekf_dense_get_view_colour: the slot holds no colour image" : "ekf_dense_get_view: the slot is not set";
    return EKF_ERR_STATE;
  }
  std::string& err = d->err;
  if (out) {
    const size_t row = (size_t)C * d->W;
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipMemcpy2D(out, (size_t)pitch, colour ? v.bgr : v.img, row, row, (size_t)d->H, hipMemcpyDeviceToHost));
  }
  if (K) std::copy(v.K, v.K + 4, K);
  if (pose7) {
    std::copy(v.t, v.t + 3, pose7);
    std::copy(v.q, v.q + 4, pose7 + 3);
  }
  return EKF_OK;
}

int ekf_dense_get_view(const ekf_dense* h, int slot, unsigned char* img, int pitch, double* K, double* pose7) {
  return dense_get_view(h, 1, slot, img, pitch, K, pose7);
}

int ekf_dense_get_view_colour(const ekf_dense* h, int slot, unsigned char* bgr, int pitch) {
  return dense_get_view(h, 3, slot, bgr, pitch, nullptr, nullptr);
}

int ekf_dense_set_pose(ekf_dense* h, int slot, const double* pose7) {
  if (!h) return EKF_ERR_ARG;
  auto* d = h->impl;
  double t[3], R[9], q[4];
  const int rc = dense_view_args(d, "ekf_dense_set_pose", slot, nullptr, pose7, t, R, q);
  if (rc != EKF_OK) return rc;
  if (!d->v[slot].set) {
    d->err = "ekf_dense_set_pose: the slot is not set";
    return EKF_ERR_ARG;
  }
  dense_commit(d->v[slot], nullptr, t, R, q);
  return EKF_OK;
}

// ref and src[]: in range, set, ref not among src, no slot named twice, 1 <= n_src <= 8
static bool dense_slots_ok(const ekf::DenseStereo* d, int ref, const int* src, int n_src) {
  if (ref < 0 || ref >= d->max_views || !d->v[ref].set || !src || n_src < 1 || n_src > ekf::kDenseMaxSrc) return false;
  for (int i = 0; i < n_src; ++i) {
    if (src[i] < 0 || src[i] >= d->max_views || src[i] == ref || !d->v[src[i]].set) return false;
    for (int j = 0; j < i; ++j)
      if (src[j] == src[i]) return false;
  }
  return true;
}

// the limits of §15.1, which the semi-global sweep shares
static bool dense_sweep_ok(const ekf::DenseStereo* d, int ref, const int* src, int n_src, double w_min, double w_max, int planes,
                           int radius, int trunc) {
  return dense_slots_ok(d, ref, src, n_src) && planes >= 2 && planes <= ekf::kDenseMaxPlanes && radius >= 0 &&
         radius <= ekf::kDenseMaxRadius && trunc >= 1 && trunc <= 255 && std::isfinite(w_min) && std::isfinite(w_max) &&
         w_min > 0.0 && w_min < w_max;
}

// ekf_dense_sweep, and with the census cost ekf_dense_sweep_census: one set of checks and state rules
static int dense_sweep(ekf_dense* h, const char* who, bool census, int ref, const int* src, int n_src, double w_min, double w_max,
                       int planes, int radius, int trunc) {
  if (!h) return EKF_ERR_ARG;
  auto* d = h->impl;
  if (!dense_sweep_ok(d, ref, src, n_src, w_min, w_max, planes, radius, trunc)) {
    d->err = std::string(who) + ": ref and 1..8 other, distinct source slots, all set; planes 2..1024, radius 0..4, trunc 1..255, "
             "0 < w_min < w_max finite";
    return EKF_ERR_ARG;
  }
  std::string& err = d->err;
  HIPCHK(hipSetDevice(d->device));
  HIPCHK(h->sgm.sweep(*d, ref, src, n_src, w_min, w_max, planes, radius, trunc, 0, 0, 0, census));
  return EKF_OK;
}

int ekf_dense_sweep(ekf_dense* h, int ref, const int* src, int n_src, double w_min, double w_max, int planes, int radius,
                    int trunc) {
  return dense_sweep(h, "ekf_dense_sweep", false, ref, src, n_src, w_min, w_max, planes, radius, trunc);
}

// ekf_dense_filter, and with the uniqueness test ekf_dense_filter_unique: one set of checks and state rules
static int dense_filter(ekf_dense* h, const char* who, int ref, const int* src, int n_src, double rel_tol, int min_agree,
                        int uniqueness) {
  if (!h) return EKF_ERR_ARG;
  auto* d = h->impl;
  if (!dense_slots_ok(d, ref, src, n_src) || !std::isfinite(rel_tol) || rel_tol < 0.0 || min_agree < 1 || min_agree > n_src) {
    d->err = std::string(who) + ": ref and 1..8 other, distinct source slots, all set; rel_tol finite and >= 0, min_agree 1..n_src";
    return EKF_ERR_ARG;
  }
  if (uniqueness < 0 || uniqueness > 100) {
    d->err = std::string(who) + ": uniqueness is 0..100 (per cent)";
    return EKF_ERR_ARG;
  }
  bool swept = d->v[ref].swept;
  for (int i = 0; i < n_src; ++i) swept = swept && d->v[src[i]].swept;
  if (!swept) {
    d->err = std::string(who) + ": a named slot has not been swept since its image or pose last changed";
    return EKF_ERR_STATE;
  }
  if (uniqueness > 0 && !d->v[ref].has_runner) {
    d->err = std::string(who) + ": uniqueness > 0 needs the runner-up map of ref (a sweep of it after ekf_dense_keep_runner_up(h, 1))";
    return EKF_ERR_STATE;
  }
  std::string& err = d->err;
  HIPCHK(hipSetDevice(d->device));
  HIPCHK(d->filter_points(ref, src, n_src, rel_tol, min_agree, false, false, uniqueness));
  return EKF_OK;
}

int ekf_dense_filter(ekf_dense* h, int ref, const int* src, int n_src, double rel_tol, int min_agree) {
  return dense_filter(h, "ekf_dense_filter", ref, src, n_src, rel_tol, min_agree, 0);
}

// slot in range with the asked-for map: EKF_OK, or the code with the message set
static int dense_map_ok(ekf::DenseStereo* d, const char* who, int slot, int filtered) {
  if (slot < 0 || slot >= d->max_views || (filtered != 0 && filtered != 1)) {
    d->err = std::string(who) + ": slot in 0..max_views-1 and filtered is 0 or 1";
    return EKF_ERR_ARG;
  }
  const ekf::DenseView& v = d->v[slot];
  if (!v.set || !v.swept || (filtered && !v.filtered)) {
    d->err = std::string(who) + ": the slot has no such map (ekf_dense_sweep, and ekf_dense_filter for filtered = 1, after the "
             "last change of its image or pose)";
    return EKF_ERR_STATE;
  }
  return EKF_OK;
}

int ekf_dense_get_depth(ekf_dense* h, int slot, int filtered, float* depth, int* plane, unsigned int* cost,
                        unsigned char* views) {
  if (!h) return EKF_ERR_ARG;
  auto* d = h->impl;
  const int rc = dense_map_ok(d, "ekf_dense_get_depth", slot, filtered);
  if (rc != EKF_OK) return rc;
  std::string& err = d->err;
  const ekf::DenseView& v = d->v[slot];
  const size_t n = d->npix();
  HIPCHK(hipSetDevice(d->device));
  if (depth) HIPCHK(hipMemcpy(depth, filtered ? v.fdepth : v.depth, n * sizeof(float), hipMemcpyDeviceToHost));
  if (plane) HIPCHK(hipMemcpy(plane, filtered ? v.fplane : v.plane, n * sizeof(int), hipMemcpyDeviceToHost));
  if (cost) HIPCHK(hipMemcpy(cost, v.cost, n * sizeof(unsigned), hipMemcpyDeviceToHost));
  if (views) HIPCHK(hipMemcpy(views, v.nviews, n, hipMemcpyDeviceToHost));
  return EKF_OK;
}

int ekf_dense_get_points(ekf_dense* h, int slot, int filtered, double* xyz) {
  if (!h) return EKF_ERR_ARG;
  auto* d = h->impl;
  if (!xyz) {
    d->err = "ekf_dense_get_points: xyz must not be NULL";
    return EKF_ERR_ARG;
  }
  const int rc = dense_map_ok(d, "ekf_dense_get_points", slot, filtered);
  if (rc != EKF_OK) return rc;
  std::string& err = d->err;
  HIPCHK(hipSetDevice(d->device));
  HIPCHK(d->filter_points(slot, nullptr, 0, 0.0, 0, filtered != 0, true));
  HIPCHK(hipMemcpy(xyz, d->d_xyz, d->npix() * 3 * sizeof(double), hipMemcpyDeviceToHost));
  return EKF_OK;
}

int ekf_dense_profile(ekf_dense* h, int enable) {
  if (!h) return EKF_ERR_ARG;
  h->impl->timer.enable(enable != 0);
  h->impl->census_timer.enable(enable != 0);
  h->impl->best_timer.enable(enable != 0);
  h->impl->unique_timer.enable(enable != 0);
  h->sgm.timer.enable(enable != 0);
  h->speckle.timer.enable(enable != 0);
  return EKF_OK;
}

int ekf_dense_get_profile(const ekf_dense* h, double* kernel_ms, long long* launches) {
  if (!h || !kernel_ms || !launches) return EKF_ERR_ARG;
  h->impl->timer.read(kernel_ms, launches, 0, 2);
  return EKF_OK;
}

// ---- semi-global cost aggregation ---------------------------------------------------------------------------
// ekf_dense_sweep_sgm, and with the census cost (§20) ekf_dense_sweep_sgm_census
static int dense_sweep_sgm(ekf_dense* h, const char* who, bool census, int ref, const int* src, int n_src, double w_min, double w_max,
                           int planes, int radius, int trunc, int p1, int p2, int paths) {
  if (!h) return EKF_ERR_ARG;
  auto* d = h->impl;
  if (!dense_sweep_ok(d, ref, src, n_src, w_min, w_max, planes, radius, trunc) || p1 < 1 || p1 > p2 || p2 > ekf::kSgmMaxPenalty ||
      (paths != 4 && paths != 8) || (long long)d->W * d->H * planes > ekf::kSgmMaxElems) {
    d->err = std::string(who) + ": the arguments of ekf_dense_sweep; 1 <= p1 <= p2 <= 2^20, paths 4 or 8, "
             "width x height x planes <= 2^28";
    return EKF_ERR_ARG;
  }
  std::string& err = d->err;
  HIPCHK(hipSetDevice(d->device));
  HIPCHK(h->sgm.sweep(*d, ref, src, n_src, w_min, w_max, planes, radius, trunc, p1, p2, paths, census));
  return EKF_OK;
}

int ekf_dense_sweep_sgm(ekf_dense* h, int ref, const int* src, int n_src, double w_min, double w_max, int planes, int radius,
                        int trunc, int p1, int p2, int paths) {
  return dense_sweep_sgm(h, "ekf_dense_sweep_sgm", false, ref, src, n_src, w_min, w_max, planes, radius, trunc, p1, p2, paths);
}

int ekf_dense_get_volume(ekf_dense* h, int slot, int aggregated, unsigned int* out) {
  if (!h) return EKF_ERR_ARG;
  auto* d = h->impl;
  if (slot < 0 || slot >= d->max_views || (aggregated != 0 && aggregated != 1) || !out) {
    d->err = "ekf_dense_get_volume: slot in 0..max_views-1, aggregated is 0 or 1, out must not be NULL";
    return EKF_ERR_ARG;
  }
  const ekf::DenseView& v = d->v[slot];
  if (!v.set || !v.swept || !v.sgm) {
    d->err = "ekf_dense_get_volume: the volumes are not those of this slot (the handle's last ekf_dense_sweep_sgm, with no "
             "setter or sweep of the slot since)";
    return EKF_ERR_STATE;
  }
  std::string& err = d->err;
  HIPCHK(hipSetDevice(d->device));
  std::vector<unsigned> vol(d->npix() * (size_t)h->sgm.D);       // the device keeps the planes of a pixel side by side
  HIPCHK(hipMemcpy(vol.data(), aggregated ? h->sgm.S : h->sgm.C, vol.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
  ekf::sgm_volume_to_planes(vol.data(), out, d->npix(), h->sgm.D);
  return EKF_OK;
}

int ekf_dense_get_sgm_profile(const ekf_dense* h, double* kernel_ms, long long* launches) {
  if (!h || !kernel_ms || !launches) return EKF_ERR_ARG;
  h->sgm.timer.read(kernel_ms, launches, 0, ekf::kSgmKinds);
  return EKF_OK;
}

// ---- census matching cost -----------------------------------------------------------------------------------
int ekf_dense_sweep_census(ekf_dense* h, int ref, const int* src, int n_src, double w_min, double w_max, int planes, int radius,
                           int trunc) {
  return dense_sweep(h, "ekf_dense_sweep_census", true, ref, src, n_src, w_min, w_max, planes, radius, trunc);
}

int ekf_dense_sweep_sgm_census(ekf_dense* h, int ref, const int* src, int n_src, double w_min, double w_max, int planes, int radius,
                               int trunc, int p1, int p2, int paths) {
  return dense_sweep_sgm(h, "ekf_dense_sweep_sgm_census", true, ref, src, n_src, w_min, w_max, planes, radius, trunc, p1, p2, paths);
}

int ekf_dense_get_census(ekf_dense* h, int slot, unsigned long long* out) {
  if (!h) return EKF_ERR_ARG;
  auto* d = h->impl;
  if (slot < 0 || slot >= d->max_views || !out) {
    d->err = "ekf_dense_get_census: slot in 0..max_views-1, out must not be NULL";
    return EKF_ERR_ARG;
  }
  if (!d->v[slot].set) {
    d->err = "ekf_dense_get_census: the slot is not set";
    return EKF_ERR_STATE;
  }
  std::string& err = d->err;
  HIPCHK(hipSetDevice(d->device));
  HIPCHK(d->census_reserve(slot, nullptr, 0));
  HIPCHK(d->census_update(slot));
  HIPCHK(hipMemcpy(out, d->v[slot].census, d->npix() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return EKF_OK;
}

int ekf_dense_get_census_profile(const ekf_dense* h, double* kernel_ms, long long* launches) {
  if (!h || !kernel_ms || !launches) return EKF_ERR_ARG;
  h->impl->census_timer.read(kernel_ms, launches, 0, 3);
  return EKF_OK;
}

// ---- best-K source selection ----------------------------------------------------------------------------------
int ekf_dense_sweep_best(ekf_dense* h, int ref, const int* src, int n_src, int n_best, double w_min, double w_max, int planes,
                         int radius, int trunc, int census, int paths, int p1, int p2) {
  if (!h) return EKF_ERR_ARG;
  auto* d = h->impl;
  const bool sgm = paths != 0;
  if (!dense_sweep_ok(d, ref, src, n_src, w_min, w_max, planes, radius, trunc) || n_best < 1 || n_best > n_src ||
      (census != 0 && census != 1) || (paths != 0 && paths != 4 && paths != 8) || (!sgm && (p1 != 0 || p2 != 0)) ||
      (sgm && (p1 < 1 || p1 > p2 || p2 > ekf::kSgmMaxPenalty || (long long)d->W * d->H * planes > ekf::kSgmMaxElems))) {
    d->err = "ekf_dense_sweep_best: the arguments of ekf_dense_sweep; 1 <= n_best <= n_src, census 0 or 1, paths 0, 4 or 8; "
             "paths 0: p1 = p2 = 0; otherwise 1 <= p1 <= p2 <= 2^20 and width x height x planes <= 2^28";
    return EKF_ERR_ARG;
  }
  std::string& err = d->err;
  HIPCHK(hipSetDevice(d->device));
  HIPCHK(h->sgm.sweep(*d, ref, src, n_src, w_min, w_max, planes, radius, trunc, p1, p2, paths, census != 0, n_best));
  return EKF_OK;
}

int ekf_dense_get_best_profile(const ekf_dense* h, double* kernel_ms, long long* launches) {
  if (!h || !kernel_ms || !launches) return EKF_ERR_ARG;
  h->impl->best_timer.read(kernel_ms, launches, 0, 4);
  return EKF_OK;
}

// ---- runner-up cost and uniqueness test -------------------------------------------------------------------------
int ekf_dense_keep_runner_up(ekf_dense* h, int enable) {
  if (!h) return EKF_ERR_ARG;
  h->impl->keep_runner = enable != 0;
  return EKF_OK;
}

int ekf_dense_get_runner_up(ekf_dense* h, int slot, unsigned int* out) {
  if (!h) return EKF_ERR_ARG;
  auto* d = h->impl;
  if (slot < 0 || slot >= d->max_views || !out) {
    d->err = "ekf_dense_get_runner_up: slot in 0..max_views-1, out must not be NULL";
    return EKF_ERR_ARG;
  }
  const ekf::DenseView& v = d->v[slot];
  if (!v.set || !v.swept || !v.has_runner) {
    d->err = "ekf_dense_get_runner_up: the slot has no runner-up map (a sweep after ekf_dense_keep_runner_up(h, 1), with no "
             "setter or sweep of the slot since)";
    return EKF_ERR_STATE;
  }
  std::string& err = d->err;
  HIPCHK(hipSetDevice(d->device));
  HIPCHK(hipMemcpy(out, v.runner, d->npix() * sizeof(unsigned), hipMemcpyDeviceToHost));
  return EKF_OK;
}

int ekf_dense_filter_unique(ekf_dense* h, int ref, const int* src, int n_src, double rel_tol, int min_agree, int uniqueness) {
  return dense_filter(h, "ekf_dense_filter_unique", ref, src, n_src, rel_tol, min_agree, uniqueness);
}

int ekf_dense_get_unique_profile(const ekf_dense* h, double* kernel_ms, long long* launches) {
  if (!h || !kernel_ms || !launches) return EKF_ERR_ARG;
  h->impl->unique_timer.read(kernel_ms, launches, 0, ekf::kUniqueKinds);
  return EKF_OK;
}

// ---- speckle filter: connected segments of a depth map ----------------------------------------------------------
// min_size and max_diff in their ranges: EKF_OK, or EKF_ERR_ARG with the message set
static int speckle_args_ok(ekf::DenseStereo* d, const char* who, int min_size, int max_diff) {
  if (min_size < 1 || min_size > ekf::kSpeckleMaxSize || max_diff < 0 || max_diff > ekf::kSpeckleMaxDiff) {
    d->err = std::string(who) + ": min_size is 1..2^26, max_diff 0..1023";
    return EKF_ERR_ARG;
  }
  return EKF_OK;
}

int ekf_dense_filter_speckle(ekf_dense* h, int slot, int min_size, int max_diff) {
  if (!h) return EKF_ERR_ARG;
  auto* d = h->impl;
  int rc = speckle_args_ok(d, "ekf_dense_filter_speckle", min_size, max_diff);
  if (rc == EKF_OK) rc = dense_map_ok(d, "ekf_dense_filter_speckle", slot, 1);
  if (rc != EKF_OK) return rc;
  std::string& err = d->err;
  ekf::DenseView& v = d->v[slot];
  for (ekf::DenseView& o : d->v) o.seg = false;                             // the planes are about to change hands
  HIPCHK(hipSetDevice(d->device));
  HIPCHK(h->speckle.run(d->W, d->H, v.fdepth, v.fplane, min_size, max_diff));
  v.seg = true;
  return EKF_OK;
}

int ekf_dense_get_segments(ekf_dense* h, int slot, unsigned int* label, unsigned int* size) {
  if (!h) return EKF_ERR_ARG;
  auto* d = h->impl;
  if (slot < 0 || slot >= d->max_views) {
    d->err = "ekf_dense_get_segments: slot in 0..max_views-1";
    return EKF_ERR_ARG;
  }
  const ekf::DenseView& v = d->v[slot];
  if (!v.set || !v.swept || !v.filtered || !v.seg) {
    d->err = "ekf_dense_get_segments: the segments are not those of this slot (the handle's last ekf_dense_filter_speckle, with "
             "no setter, sweep or filter of the slot and no ekf_dense_speckle_host since)";
    return EKF_ERR_STATE;
  }
  std::string& err = d->err;
  HIPCHK(hipSetDevice(d->device));
  if (label) HIPCHK(hipMemcpy(label, h->speckle.R, d->npix() * sizeof(unsigned), hipMemcpyDeviceToHost));
  if (size) HIPCHK(hipMemcpy(size, h->speckle.L, d->npix() * sizeof(unsigned), hipMemcpyDeviceToHost));
  return EKF_OK;
}

int ekf_dense_speckle_host(ekf_dense* h, float* depth, int* plane, int min_size, int max_diff, unsigned int* label,
                           unsigned int* size) {
  if (!h) return EKF_ERR_ARG;
  auto* d = h->impl;
  if (!depth || !plane) {
    d->err = "ekf_dense_speckle_host: depth and plane must not be NULL";
    return EKF_ERR_ARG;
  }
  const int rc = speckle_args_ok(d, "ekf_dense_speckle_host", min_size, max_diff);
  if (rc != EKF_OK) return rc;
  std::string& err = d->err;
  ekf::DenseSpeckle& s = h->speckle;
  const size_t n = d->npix();
  for (ekf::DenseView& o : d->v) o.seg = false;
  HIPCHK(hipSetDevice(d->device));
  HIPCHK(s.h_depth.reserve(n));
  HIPCHK(s.h_plane.reserve(n));
  HIPCHK(hipMemcpy(s.h_depth, depth, n * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(s.h_plane, plane, n * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(s.run(d->W, d->H, s.h_depth, s.h_plane, min_size, max_diff));
  HIPCHK(hipMemcpy(depth, s.h_depth, n * sizeof(float), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(plane, s.h_plane, n * sizeof(int), hipMemcpyDeviceToHost));
  if (label) HIPCHK(hipMemcpy(label, s.R, n * sizeof(unsigned), hipMemcpyDeviceToHost));
  if (size) HIPCHK(hipMemcpy(size, s.L, n * sizeof(unsigned), hipMemcpyDeviceToHost));
  return EKF_OK;
}

int ekf_dense_get_speckle_profile(const ekf_dense* h, double* kernel_ms, long long* launches) {
  if (!h || !kernel_ms || !launches) return EKF_ERR_ARG;
  h->speckle.timer.read(kernel_ms, launches, 0, ekf::kSpeckleKinds);
  return EKF_OK;
}

// ---- TSDF fusion of depth maps and mesh extraction -----------------------------------------------------
struct ekf_fusion {
  ekf::TsdfFusion* impl;
  ekf::TsdfRaycast rc;                // the last render of the volume (ekf_raycast_*)
  ekf::MeshStamps stamps;             // which mesh is which, and what is still made from it
  ekf::TsdfMesh mesh;                 // the last weld of the volume's mesh (ekf_mesh_*)
  ekf::TsdfComponents comp;           // that weld's components and its pruned copy
  ekf::TsdfSmooth smooth;             // the smoothed copy of either of them
  ekf::TsdfSimplify simp;             // the simplified copy of any of the three
  ekf::TsdfTexture tex;               // the texture atlas of any of the four
  ekf::TsdfRaster rast;               // the last rasterisation of any of them, or of a mesh the caller gave
  ekf::TsdfDistance dist;             // the last distance from the vertices of one of them, or from points, to another
};

static int fusion_create(int nx, int ny, int nz, const double* origin, double voxel, double trunc, int device, bool colour,
                         ekf_fusion** out) {
  if (!out) return EKF_ERR_ARG;
  *out = nullptr;
  const bool dims_ok = nx >= 2 && ny >= 2 && nz >= 2 && nx <= ekf::kFusionMaxDim && ny <= ekf::kFusionMaxDim &&
                       nz <= ekf::kFusionMaxDim && (long long)nx * ny * nz <= ekf::kFusionMaxVoxels;
  if (!dims_ok || !origin || !sba_finite(origin, 3) || !std::isfinite(voxel) || !(voxel > 0.0) || !std::isfinite(trunc) ||
      !(trunc > 0.0)) {
    ekf::g_create_error = "ekf_fusion_create: 2 <= nx, ny, nz <= 1024, nx ny nz <= 2^28, origin finite, voxel and trunc finite and > 0";
    return EKF_ERR_ARG;
  }
  const int rc = create_device("ekf_fusion_create", device);
  if (rc != EKF_OK) return rc;
  auto* f = new ekf::TsdfFusion();
  f->device = device;
  f->g.nx = nx; f->g.ny = ny; f->g.nz = nz;
  std::copy(origin, origin + 3, f->g.origin);
  f->g.voxel = voxel;
  f->trunc = trunc;
  hipError_t e = hipSetDevice(device);
  f->created = e == hipSuccess;
  if (e == hipSuccess) e = f->timer.create();
  if (e == hipSuccess) e = f->sum.reserve(f->nvox());
  if (e == hipSuccess) e = f->cnt.reserve(f->nvox());
  if (e == hipSuccess) e = f->gsum.reserve(f->nvox());
  if (e == hipSuccess && colour) e = f->csum.reserve(3 * f->nvox());
  f->colour = colour;
  if (e == hipSuccess) e = f->clear();
  if (e != hipSuccess) {
    ekf::g_create_error = std::string("ekf_fusion_create: ") + hipGetErrorString(e);
    (void)hipGetLastError();
    delete f;
    return EKF_ERR_DEVICE;
  }
  *out = new ekf_fusion{f};
  return EKF_OK;
}

int ekf_fusion_create(int nx, int ny, int nz, const double* origin, double voxel, double trunc, int device, ekf_fusion** out) {
  return fusion_create(nx, ny, nz, origin, voxel, trunc, device, false, out);
}

int ekf_colour_create(int nx, int ny, int nz, const double* origin, double voxel, double trunc, int device, ekf_fusion** out) {
  return fusion_create(nx, ny, nz, origin, voxel, trunc, device, true, out);
}

int ekf_colour_has(const ekf_fusion* h) { return h && h->impl->colour ? 1 : 0; }

void ekf_fusion_destroy(ekf_fusion* h) {
  if (!h) return;
  if (h->impl->created) hipSetDevice(h->impl->device);
  h->rc = ekf::TsdfRaycast();
  delete h->impl;
  delete h;
}

const char* ekf_fusion_last_error(const ekf_fusion* h) {
  if (!h) return ekf::g_create_error.c_str();
  return h->impl->err.c_str();
}

static int fusion_room(ekf::TsdfFusion* f, const char* who) {
  if (f->maps >= ekf::kFusionMaxMaps) {
    f->err = std::string(who) + ": the handle has integrated 65535 maps (the count of a voxel is 16 bits); nothing was changed";
    return EKF_ERR_CAPACITY;
  }
  return EKF_OK;
}

int ekf_fusion_integrate(ekf_fusion* h, ekf_dense* dense, int slot, int filtered) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  if (!dense || dense->impl->device != f->device) {
    f->err = "ekf_fusion_integrate: a dense handle on the volume's device";
    return EKF_ERR_ARG;
  }
  auto* d = dense->impl;
  const int rc = dense_map_ok(d, "ekf_fusion_integrate", slot, filtered);
  if (rc != EKF_OK) {
    f->err = d->err;
    return rc;
  }
  const int room = fusion_room(f, "ekf_fusion_integrate");
  if (room != EKF_OK) return room;
  std::string& err = f->err;
  const ekf::DenseView& v = d->v[slot];
  HIPCHK(hipSetDevice(f->device));
  HIPCHK(f->integrate(filtered ? v.fdepth : v.depth, v.img, d->W, d->H, v.K, v.R, v.t, d->colour_of(slot)));
  return EKF_OK;
}

// A call that only a colour volume answers: EKF_OK, or EKF_ERR_STATE with the message set (nothing else is touched).
static int fusion_colour_only(ekf::TsdfFusion* f, const char* who) {
  if (!f->colour) {
    f->err = std::string(who) + ": the handle is a plain volume (ekf_colour_create makes a colour volume)";
    return EKF_ERR_STATE;
  }
  return EKF_OK;
}

// A map from the host with a grey image (C = 1) or a colour one (C = 3, a colour volume only): rows of C width bytes.
static int fusion_integrate_host(ekf_fusion* h, int C, const float* depth, const unsigned char* img, int pitch, int width, int height,
                                 const double* K, const double* pose7) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  const bool colour = C == 3;
  const char* who = colour ? "ekf_colour_integrate_host" : "ekf_fusion_integrate_host";
  double t[3], R[9], q[4];
  if (!depth || !img || !K || !pose7 || width < 1 || height < 1 || width > ekf::kFusionMaxMapDim ||
      height > ekf::kFusionMaxMapDim || pitch < C * width || !pinhole_ok(K) || !ekf::dense_pose(pose7, t, R, q)) {
    f->err = std::string(who) + (colour ? ": depth, bgr, K and pose7 not NULL; 1 <= width, height <= 8192; pitch >= 3 width; "
                                        : ": depth, img, K and pose7 not NULL; 1 <= width, height <= 8192; pitch >= width; ") +
             "K finite with fx, fy > 0; pose7 finite with q != 0";
    return EKF_ERR_ARG;
  }
  const int kind = colour ? fusion_colour_only(f, who) : EKF_OK;
  if (kind != EKF_OK) return kind;
  const int room = fusion_room(f, who);
  if (room != EKF_OK) return room;
  std::string& err = f->err;
  const size_t n = (size_t)width * height, row = (size_t)C * width;
  ekf::DevBuf<unsigned char>& d_img = colour ? f->d_bgr : f->d_img;
  HIPCHK(hipSetDevice(f->device));
  HIPCHK(f->d_depth.reserve(n));
  HIPCHK(d_img.reserve(C * n));
  HIPCHK(hipMemcpy(f->d_depth, depth, n * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy2D(d_img, row, img, (size_t)pitch, row, (size_t)height, hipMemcpyHostToDevice));
  HIPCHK(f->integrate(f->d_depth, colour ? nullptr : (const unsigned char*)d_img, width, height, K, R, t,
                      colour ? (const unsigned char*)d_img : nullptr));
  return EKF_OK;
}

int ekf_fusion_integrate_host(ekf_fusion* h, const float* depth, const unsigned char* img, int pitch, int width, int height,
                              const double* K, const double* pose7) {
  return fusion_integrate_host(h, 1, depth, img, pitch, width, height, K, pose7);
}

int ekf_colour_integrate_host(ekf_fusion* h, const float* depth, const unsigned char* bgr, int pitch, int width, int height,
                              const double* K, const double* pose7) {
  return fusion_integrate_host(h, 3, depth, bgr, pitch, width, height, K, pose7);
}

int ekf_colour_get_volume(ekf_fusion* h, unsigned int* csum) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  if (!csum) {
    f->err = "ekf_colour_get_volume: csum must not be NULL";
    return EKF_ERR_ARG;
  }
  const int kind = fusion_colour_only(f, "ekf_colour_get_volume");
  if (kind != EKF_OK) return kind;
  std::string& err = f->err;
  HIPCHK(hipSetDevice(f->device));
  HIPCHK(hipMemcpy(csum, f->csum, 3 * f->nvox() * sizeof(unsigned), hipMemcpyDeviceToHost));
  return EKF_OK;
}

int ekf_colour_set_volume(ekf_fusion* h, const unsigned int* csum) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  if (!csum) {
    f->err = "ekf_colour_set_volume: csum must not be NULL";
    return EKF_ERR_ARG;
  }
  const int kind = fusion_colour_only(f, "ekf_colour_set_volume");
  if (kind != EKF_OK) return kind;
  std::string& err = f->err;
  HIPCHK(hipSetDevice(f->device));
  f->mesh_valid = false;
  ++f->changes;
  HIPCHK(hipMemcpy(f->csum, csum, 3 * f->nvox() * sizeof(unsigned), hipMemcpyHostToDevice));
  return EKF_OK;
}

int ekf_fusion_reset(ekf_fusion* h) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  std::string& err = f->err;
  HIPCHK(hipSetDevice(f->device));
  HIPCHK(f->clear());
  return EKF_OK;
}

int ekf_fusion_get_volume(ekf_fusion* h, float* sum, unsigned short* cnt, unsigned int* gsum, int* maps) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  std::string& err = f->err;
  const size_t n = f->nvox();
  HIPCHK(hipSetDevice(f->device));
  if (sum) HIPCHK(hipMemcpy(sum, f->sum, n * sizeof(float), hipMemcpyDeviceToHost));
  if (cnt) HIPCHK(hipMemcpy(cnt, f->cnt, n * sizeof(unsigned short), hipMemcpyDeviceToHost));
  if (gsum) HIPCHK(hipMemcpy(gsum, f->gsum, n * sizeof(unsigned), hipMemcpyDeviceToHost));
  if (maps) *maps = f->maps;
  return EKF_OK;
}

int ekf_fusion_set_volume(ekf_fusion* h, const float* sum, const unsigned short* cnt, const unsigned int* gsum, int maps) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  if (maps < -1 || maps > ekf::kFusionMaxMaps) {
    f->err = "ekf_fusion_set_volume: maps is -1 (keep the counter) or 0..65535";
    return EKF_ERR_ARG;
  }
  std::string& err = f->err;
  const size_t n = f->nvox();
  int most = maps >= 0 ? maps : f->maps;
  if (cnt)                                       // the counter never falls below a voxel's count: cnt + 1 cannot wrap
    for (size_t i = 0; i < n; ++i) most = std::max(most, (int)cnt[i]);
  HIPCHK(hipSetDevice(f->device));
  f->mesh_valid = false;
  ++f->changes;
  if (sum) HIPCHK(hipMemcpy(f->sum, sum, n * sizeof(float), hipMemcpyHostToDevice));
  if (cnt) HIPCHK(hipMemcpy(f->cnt, cnt, n * sizeof(unsigned short), hipMemcpyHostToDevice));
  if (gsum) HIPCHK(hipMemcpy(f->gsum, gsum, n * sizeof(unsigned), hipMemcpyHostToDevice));
  f->maps = most;
  return EKF_OK;
}

int ekf_fusion_extract(ekf_fusion* h, int min_count, unsigned long long* n_tri) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  if (min_count < 1 || min_count > ekf::kFusionMaxMaps || !n_tri) {
    f->err = "ekf_fusion_extract: min_count 1..65535 and n_tri not NULL";
    return EKF_ERR_ARG;
  }
  std::string& err = f->err;
  HIPCHK(hipSetDevice(f->device));
  HIPCHK(f->extract(min_count));
  *n_tri = f->n_tri;
  return EKF_OK;
}

// The mesh of the last extract: positions, keys and grey (ekf_fusion_get_mesh), or the vertex colours of a colour volume
// (ekf_colour_get_mesh: bgr alone, which may be NULL).  A NULL array is not copied.
static int fusion_get_mesh(ekf_fusion* h, const char* who, bool colour, double* xyz, unsigned long long* key, unsigned char* grey,
                           unsigned char* bgr, unsigned long long max_tri) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  const int kind = colour ? fusion_colour_only(f, who) : EKF_OK;
  if (kind != EKF_OK) return kind;
  if (!f->mesh_valid) {
    f->err = std::string(who) + ": no ekf_fusion_extract since the volume last changed";
    return EKF_ERR_STATE;
  }
  std::string& err = f->err;
  const size_t nv = (size_t)std::min(f->n_tri, max_tri) * 3;
  if (nv == 0 || (colour && !bgr)) return EKF_OK;
  HIPCHK(hipSetDevice(f->device));
  if (xyz) HIPCHK(hipMemcpy(xyz, f->m_xyz, nv * 3 * sizeof(double), hipMemcpyDeviceToHost));
  if (key) HIPCHK(hipMemcpy(key, f->m_key, nv * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  if (grey) HIPCHK(hipMemcpy(grey, f->m_grey, nv, hipMemcpyDeviceToHost));
  if (bgr) HIPCHK(hipMemcpy(bgr, f->m_bgr, nv * 3, hipMemcpyDeviceToHost));
  return EKF_OK;
}

int ekf_fusion_get_mesh(ekf_fusion* h, double* xyz, unsigned long long* key, unsigned char* grey, unsigned long long max_tri) {
  return fusion_get_mesh(h, "ekf_fusion_get_mesh", false, xyz, key, grey, nullptr, max_tri);
}

int ekf_colour_get_mesh(ekf_fusion* h, unsigned char* bgr, unsigned long long max_tri) {
  return fusion_get_mesh(h, "ekf_colour_get_mesh", true, nullptr, nullptr, nullptr, bgr, max_tri);
}

int ekf_fusion_profile(ekf_fusion* h, int enable) {
  if (!h) return EKF_ERR_ARG;
  h->impl->timer.enable(enable != 0);   // the four kinds of the fusion, the two of the ray caster and the three of colour
  h->mesh.timer.enable(enable != 0);    // the five of the weld
  h->comp.timer.enable(enable != 0);    // the eight of the components
  h->smooth.timer.enable(enable != 0);  // the seven of the smoothing
  h->simp.timer.enable(enable != 0);    // the ten of the simplification
  h->tex.timer.enable(enable != 0);     // the four of the texture
  h->rast.timer.enable(enable != 0);    // the four of the rasteriser
  h->dist.timer.enable(enable != 0);    // the nine of the distance
  return EKF_OK;
}

// What the getters of a profile of the fusion handle share: `read` is the timer's read of its kinds.
extern "C++" {
template <class Read>
static int fusion_profile(const ekf_fusion* h, const double* kernel_ms, const long long* launches, Read read) {
  if (!h || !kernel_ms || !launches) return EKF_ERR_ARG;
  read();
  return EKF_OK;
}
}

int ekf_fusion_get_profile(const ekf_fusion* h, double* kernel_ms, long long* launches) {
  return fusion_profile(h, kernel_ms, launches, [&] { h->impl->timer.read(kernel_ms, launches, 0, 4); });
}

int ekf_colour_get_profile(const ekf_fusion* h, double* kernel_ms, long long* launches) {
  return fusion_profile(h, kernel_ms, launches, [&] { h->impl->timer.read(kernel_ms, launches, 6, 3); });
}

// ---- ray casting of the volume ---------------------------------------------------------------------------
// Everything but the handle and the pose: EKF_OK with N set, or EKF_ERR_ARG with the message set.
static int raycast_args(ekf::TsdfFusion* f, const char* who, int width, int height, const double* K, double z_near, double z_far,
                        double step, int min_count, int* N) {
  bool ok = width >= 1 && height >= 1 && width <= ekf::kRaycastMaxDim && height <= ekf::kRaycastMaxDim && K && sba_finite(K, 4) &&
            K[0] != 0.0 && K[1] != 0.0 && std::isfinite(step) && step > 0.0 && std::isfinite(z_near) && std::isfinite(z_far) &&
            z_near >= 0.0 && z_near < z_far && min_count >= 1 && min_count <= ekf::kFusionMaxMaps;
  if (ok) {
    const double n = std::floor((z_far - z_near) / step) + 1.0;
    ok = n <= (double)ekf::kRaycastMaxSamples;
    if (ok) *N = (int)n;
  }
  if (!ok) {
    f->err = std::string(who) + ": 1 <= width, height <= 8192; K finite with fx, fy != 0; pose7 finite with q != 0; step finite "
             "and > 0; 0 <= z_near < z_far finite; floor((z_far - z_near) / step) + 1 <= 65536 samples; min_count 1..65535";
    return EKF_ERR_ARG;
  }
  return EKF_OK;
}

int ekf_raycast_render(ekf_fusion* h, int width, int height, const double* K, const double* pose7, double z_near, double z_far,
                       double step, int min_count) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  double t[3], R[9], q[4];
  int N = 0;
  const int rc = raycast_args(f, "ekf_raycast_render", width, height, K, z_near, z_far, step, min_count, &N);
  if (rc != EKF_OK) return rc;
  if (!pose7 || !ekf::dense_pose(pose7, t, R, q)) {
    f->err = "ekf_raycast_render: pose7 finite with q != 0";
    return EKF_ERR_ARG;
  }
  std::string& err = f->err;
  HIPCHK(hipSetDevice(f->device));
  HIPCHK(h->rc.render(*f, width, height, K, R, t, z_near, step, N, min_count));
  return EKF_OK;
}

int ekf_raycast_render_view(ekf_fusion* h, ekf_dense* dense, int slot, double z_near, double z_far, double step, int min_count) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  if (!dense || dense->impl->device != f->device) {
    f->err = "ekf_raycast_render_view: a dense handle on the volume's device";
    return EKF_ERR_ARG;
  }
  auto* d = dense->impl;
  if (slot < 0 || slot >= d->max_views) {
    f->err = "ekf_raycast_render_view: slot in 0..max_views-1";
    return EKF_ERR_ARG;
  }
  const ekf::DenseView& v = d->v[slot];
  if (!v.set) {
    f->err = "ekf_raycast_render_view: the slot is not set";
    return EKF_ERR_STATE;
  }
  int N = 0;
  const int rc = raycast_args(f, "ekf_raycast_render_view", d->W, d->H, v.K, z_near, z_far, step, min_count, &N);
  if (rc != EKF_OK) return rc;
  std::string& err = f->err;
  HIPCHK(hipSetDevice(f->device));
  HIPCHK(h->rc.render(*f, d->W, d->H, v.K, v.R, v.t, z_near, step, N, min_count));
  return EKF_OK;
}

// The last render: depth, normal, grey and size (ekf_raycast_get), or the colour image of a colour volume
// (ekf_colour_get_render: bgr alone, which may be NULL).  A NULL array is not copied.
static int raycast_get(ekf_fusion* h, const char* who, bool colour, float* depth, float* normal, unsigned char* grey,
                       unsigned char* bgr, int* width, int* height) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  const int kind = colour ? fusion_colour_only(f, who) : EKF_OK;
  if (kind != EKF_OK) return kind;
  if (!h->rc.current(*f)) {
    f->err = std::string(who) + ": no ekf_raycast_render since the volume last changed";
    return EKF_ERR_STATE;
  }
  std::string& err = f->err;
  const size_t n = (size_t)h->rc.W * h->rc.H;
  if (colour && !bgr) return EKF_OK;
  HIPCHK(hipSetDevice(f->device));
  if (depth) HIPCHK(hipMemcpy(depth, h->rc.depth, n * sizeof(float), hipMemcpyDeviceToHost));
  if (normal) HIPCHK(hipMemcpy(normal, h->rc.normal, n * 3 * sizeof(float), hipMemcpyDeviceToHost));
  if (grey) HIPCHK(hipMemcpy(grey, h->rc.grey, n, hipMemcpyDeviceToHost));
  if (bgr) HIPCHK(hipMemcpy(bgr, h->rc.bgr, n * 3, hipMemcpyDeviceToHost));
  if (width) *width = h->rc.W;
  if (height) *height = h->rc.H;
  return EKF_OK;
}

int ekf_raycast_get(ekf_fusion* h, float* depth, float* normal, unsigned char* grey, int* width, int* height) {
  return raycast_get(h, "ekf_raycast_get", false, depth, normal, grey, nullptr, width, height);
}

int ekf_colour_get_render(ekf_fusion* h, unsigned char* bgr) {
  return raycast_get(h, "ekf_colour_get_render", true, nullptr, nullptr, nullptr, bgr, nullptr, nullptr);
}

int ekf_raycast_get_profile(const ekf_fusion* h, double* kernel_ms, long long* launches) {
  return fusion_profile(h, kernel_ms, launches, [&] { h->impl->timer.read(kernel_ms, launches, 4, 2); });
}

// ---- the welded mesh of the volume and its vertex normals -------------------------------------------------
int ekf_mesh_weld(ekf_fusion* h, int min_count, int normals, unsigned long long* n_vert, unsigned long long* n_tri) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  if (min_count < 1 || min_count > ekf::kFusionMaxMaps || (normals != 0 && normals != 1) || !n_vert || !n_tri) {
    f->err = "ekf_mesh_weld: min_count 1..65535, normals 0 or 1, n_vert and n_tri not NULL";
    return EKF_ERR_ARG;
  }
  std::string& err = f->err;
  HIPCHK(hipSetDevice(f->device));
  HIPCHK(h->mesh.weld(h->stamps, *f, min_count, normals != 0));
  *n_vert = h->mesh.out.n_vert;
  *n_tri = h->mesh.out.n_tri;
  return EKF_OK;
}

// Which mesh `source` (0 the weld, 1 the pruned, 2 the smoothed, 3 the simplified mesh) means now, for every entry point that
// takes a source: EKF_OK with its view, or EKF_ERR_STATE with the message set.  The message, `who` and ": " before it:
//
//   source | no weld since the volume last changed              | a current weld, but not the source's own mesh
//   -------+----------------------------------------------------+------------------------------------------------------------------
//     0    | no ekf_mesh_weld since the volume last changed     | -
//     1    | no ekf_mesh_weld since the volume last changed     | source 1 needs an ekf_components_prune since the last ekf_mesh_weld
//     2    | no ekf_mesh_weld since the volume last changed     | source 2 needs an ekf_smooth_run on the current mesh
//     3    | source 3 needs an ekf_simplify_run on the current mesh, in both columns: source 3 never speaks of the weld
//
// A source's own mesh is current by the one rule of ekf_mesh_stamp.hpp, so "not the source's own mesh" covers a mesh never
// made, a failed attempt, and a mesh whose own source has been made again since.
static int mesh_source(ekf_fusion* h, const char* who, int source, ekf::MeshView* out) {
  static const char* const kNeeds[4] = {nullptr, ": source 1 needs an ekf_components_prune since the last ekf_mesh_weld",
                                        ": source 2 needs an ekf_smooth_run on the current mesh",
                                        ": source 3 needs an ekf_simplify_run on the current mesh"};
  auto* f = h->impl;
  const ekf::MeshStamps& st = h->stamps;
  const unsigned long long id = st.current(source, f->changes);
  if (id == 0) {
    const bool welded = st.current(0, f->changes) != 0;
    f->err = std::string(who) + (source != 3 && !welded ? ": no ekf_mesh_weld since the volume last changed" : kNeeds[source]);
    return EKF_ERR_STATE;
  }
  switch (source) {
    case 0: *out = ekf::MeshView::of(h->mesh.out, id); break;
    case 1: *out = ekf::MeshView::of(h->comp.out, id); break;
    case 2: *out = h->smooth.result(st.smooth.from == 0 ? h->mesh.out : h->comp.out, id); break;   // the run's source says which
    default: *out = ekf::MeshView::of(h->simp.out, id); break;
  }
  return EKF_OK;
}

// The four getters of an indexed mesh: the rows of `source` to the caller's arrays, at most max_vert vertices and max_tri
// triangles; a NULL array is skipped, and so is every array of a count of 0.  `none` and `no_normals` end the two messages
// that differ from getter to getter.
static int mesh_get(ekf_fusion* h, const char* who, int source, const char* none, const char* no_normals, double* xyz, unsigned* faces,
                    unsigned char* grey, unsigned char* bgr, float* normal, unsigned long long* key, unsigned long long max_vert,
                    unsigned long long max_tri) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  std::string& err = f->err;
  if (bgr && !f->colour) {
    err = std::string(who) + ": bgr must be NULL on a plain volume (ekf_colour_create makes a colour volume)";
    return EKF_ERR_ARG;
  }
  ekf::MeshView m;                                         // of a smoothed mesh faces, key, grey and bgr are the source's own buffers
  if (mesh_source(h, who, source, &m) != EKF_OK) {
    err = std::string(who) + none;
    return EKF_ERR_STATE;
  }
  if (normal && !m.has_normals) {
    err = std::string(who) + ": normal must be NULL after " + no_normals;
    return EKF_ERR_ARG;
  }
  const size_t nv = (size_t)std::min(m.n_vert, max_vert), nc = (size_t)std::min(m.n_tri, max_tri) * 3;
  HIPCHK(hipSetDevice(f->device));
  if (nv > 0) {
    if (xyz) HIPCHK(hipMemcpy(xyz, m.xyz, nv * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (grey) HIPCHK(hipMemcpy(grey, m.grey, nv, hipMemcpyDeviceToHost));
    if (bgr) HIPCHK(hipMemcpy(bgr, m.bgr, nv * 3, hipMemcpyDeviceToHost));
    if (normal) HIPCHK(hipMemcpy(normal, m.normal, nv * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (key) HIPCHK(hipMemcpy(key, m.key, nv * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  }
  if (nc > 0 && faces) HIPCHK(hipMemcpy(faces, m.faces, nc * sizeof(unsigned), hipMemcpyDeviceToHost));
  return EKF_OK;
}

int ekf_mesh_get(ekf_fusion* h, double* xyz, unsigned* faces, unsigned char* grey, unsigned char* bgr, float* normal,
                 unsigned long long* key, unsigned long long max_vert, unsigned long long max_tri) {
  return mesh_get(h, "ekf_mesh_get", 0, ": no ekf_mesh_weld since the volume last changed", "an ekf_mesh_weld without normals", xyz, faces,
                  grey, bgr, normal, key, max_vert, max_tri);
}

int ekf_mesh_get_profile(const ekf_fusion* h, double* kernel_ms, long long* launches) {
  return fusion_profile(h, kernel_ms, launches, [&] { h->mesh.timer.read(kernel_ms, launches, 0, ekf::kMeshKinds); });
}

// ---- the connected components of the welded mesh and its pruned copy ---------------------------------------
int ekf_components_find(ekf_fusion* h, unsigned long long* n_comp) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  if (!n_comp) {
    f->err = "ekf_components_find: n_comp not NULL";
    return EKF_ERR_ARG;
  }
  ekf::MeshView w;
  const int rc = mesh_source(h, "ekf_components_find", 0, &w);
  if (rc != EKF_OK) return rc;
  std::string& err = f->err;
  HIPCHK(hipSetDevice(f->device));
  HIPCHK(h->comp.components(h->stamps, w, f->colour));
  *n_comp = h->comp.n_comp;
  return EKF_OK;
}

int ekf_components_get(ekf_fusion* h, unsigned* label, unsigned* size, unsigned long long max_vert) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  if (!h->stamps.has(h->stamps.comp, f->changes)) {
    f->err = "ekf_components_get: no ekf_components_find or ekf_components_prune since the last ekf_mesh_weld";
    return EKF_ERR_STATE;
  }
  std::string& err = f->err;
  const size_t nv = (size_t)std::min(h->mesh.out.n_vert, max_vert);
  HIPCHK(hipSetDevice(f->device));
  if (nv > 0) {
    if (label) HIPCHK(hipMemcpy(label, h->comp.R, nv * sizeof(unsigned), hipMemcpyDeviceToHost));
    if (size) HIPCHK(hipMemcpy(size, h->comp.L, nv * sizeof(unsigned), hipMemcpyDeviceToHost));
  }
  return EKF_OK;
}

int ekf_components_prune(ekf_fusion* h, unsigned min_triangles, int largest, unsigned long long* n_vert, unsigned long long* n_tri,
                   unsigned long long* n_kept) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  if (min_triangles == 0 || (largest != 0 && largest != 1) || !n_vert || !n_tri || !n_kept) {
    f->err = "ekf_components_prune: min_triangles >= 1, largest 0 or 1, n_vert, n_tri and n_kept not NULL";
    return EKF_ERR_ARG;
  }
  ekf::MeshView w;
  const int rc = mesh_source(h, "ekf_components_prune", 0, &w);
  if (rc != EKF_OK) return rc;
  std::string& err = f->err;
  HIPCHK(hipSetDevice(f->device));
  HIPCHK(h->comp.prune(h->stamps, w, f->colour, min_triangles, largest != 0));
  *n_vert = h->comp.out.n_vert;
  *n_tri = h->comp.out.n_tri;
  *n_kept = h->comp.n_kept;
  return EKF_OK;
}

int ekf_components_get_pruned(ekf_fusion* h, double* xyz, unsigned* faces, unsigned char* grey, unsigned char* bgr, float* normal,
                        unsigned long long* key, unsigned long long max_vert, unsigned long long max_tri) {
  return mesh_get(h, "ekf_components_get_pruned", 1, ": no ekf_components_prune since the last ekf_mesh_weld",
                  "an ekf_mesh_weld without normals", xyz, faces, grey, bgr, normal, key, max_vert, max_tri);
}

int ekf_components_get_profile(const ekf_fusion* h, double* kernel_ms, long long* launches) {
  return fusion_profile(h, kernel_ms, launches, [&] { h->comp.timer.read(kernel_ms, launches, 0, ekf::kCompKinds); });
}

// ---- Taubin smoothing of the welded or the pruned mesh -----------------------------------------------------
// The last run's mesh, if the mesh it smoothed is still the handle's.
static int smooth_result(ekf_fusion* h, const char* who, ekf::MeshView* r) {
  if (mesh_source(h, who, 2, r) == EKF_OK) return EKF_OK;
  h->impl->err = std::string(who) + ": no ekf_smooth_run on the current mesh";
  return EKF_ERR_STATE;
}

int ekf_smooth_run(ekf_fusion* h, int source, int iterations, double lambda, double mu, int pin_boundary, int normals,
                   unsigned long long* n_vert, unsigned long long* n_tri) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  if ((source != 0 && source != 1) || iterations < 1 || iterations > ekf::kSmoothMaxIterations || !std::isfinite(lambda) ||
      !(lambda > 0.0) || lambda > 1.0 || !std::isfinite(mu) || mu < -1.0 || mu > 0.0 || (pin_boundary != 0 && pin_boundary != 1) ||
      (normals != 0 && normals != 1) || !n_vert || !n_tri) {
    f->err = "ekf_smooth_run: source 0 or 1, iterations 1..1024, 0 < lambda <= 1, -1 <= mu <= 0, pin_boundary and normals 0 or 1, "
             "n_vert and n_tri not NULL";
    return EKF_ERR_ARG;
  }
  ekf::MeshView s;
  const int rc = mesh_source(h, "ekf_smooth_run", source, &s);
  if (rc != EKF_OK) return rc;
  std::string& err = f->err;
  HIPCHK(hipSetDevice(f->device));
  HIPCHK(h->smooth.run(h->stamps, s, source, iterations, lambda, mu, pin_boundary != 0, normals != 0));
  *n_vert = s.n_vert;
  *n_tri = s.n_tri;
  return EKF_OK;
}

int ekf_smooth_get(ekf_fusion* h, double* xyz, unsigned* faces, unsigned char* grey, unsigned char* bgr, float* normal,
                   unsigned long long* key, unsigned long long max_vert, unsigned long long max_tri) {
  return mesh_get(h, "ekf_smooth_get", 2, ": no ekf_smooth_run on the current mesh", "an ekf_smooth_run without normals", xyz, faces, grey,
                  bgr, normal, key, max_vert, max_tri);
}

int ekf_smooth_get_adjacency(ekf_fusion* h, unsigned* inc, unsigned* deg, unsigned char* boundary, unsigned long long max_vert) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  ekf::MeshView s;
  const int rc = smooth_result(h, "ekf_smooth_get_adjacency", &s);
  if (rc != EKF_OK) return rc;
  std::string& err = f->err;
  const size_t nv = (size_t)std::min(s.n_vert, max_vert);
  HIPCHK(hipSetDevice(f->device));
  if (nv > 0) {
    if (inc) HIPCHK(hipMemcpy(inc, h->smooth.inc, nv * sizeof(unsigned), hipMemcpyDeviceToHost));
    if (deg) HIPCHK(hipMemcpy(deg, h->smooth.deg, nv * sizeof(unsigned), hipMemcpyDeviceToHost));
    if (boundary) HIPCHK(hipMemcpy(boundary, h->smooth.boundary, nv, hipMemcpyDeviceToHost));
  }
  return EKF_OK;
}

int ekf_smooth_get_profile(const ekf_fusion* h, double* kernel_ms, long long* launches) {
  return fusion_profile(h, kernel_ms, launches, [&] { h->smooth.timer.read(kernel_ms, launches, 0, ekf::kSmoothKinds); });
}

// ---- vertex-clustering simplification of the welded, the pruned or the smoothed mesh -----------------------
// Whether the last run's result is still that of the handle's meshes.
static int simplify_result(ekf_fusion* h, const char* who) {
  if (h->stamps.current(3, h->impl->changes) != 0) return EKF_OK;
  h->impl->err = std::string(who) + ": no ekf_simplify_run on the current mesh";
  return EKF_ERR_STATE;
}

int ekf_simplify_run(ekf_fusion* h, int source, double cell, unsigned long long* n_vert, unsigned long long* n_tri,
                     unsigned long long* n_degenerate, unsigned long long* n_duplicate) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  if (source < 0 || source > 2 || !std::isfinite(cell) || !(cell >= f->g.voxel) || !n_vert || !n_tri || !n_degenerate || !n_duplicate) {
    f->err = "ekf_simplify_run: source 0, 1 or 2, cell finite and >= the voxel, n_vert, n_tri, n_degenerate and n_duplicate not NULL";
    return EKF_ERR_ARG;
  }
  ekf::MeshView s;
  const int rc = mesh_source(h, "ekf_simplify_run", source, &s);
  if (rc != EKF_OK) return rc;
  std::string& err = f->err;
  HIPCHK(hipSetDevice(f->device));
  HIPCHK(h->simp.run(h->stamps, s, source, f->g, cell, f->colour));
  *n_vert = h->simp.out.n_vert;
  *n_tri = h->simp.out.n_tri;
  *n_degenerate = h->simp.n_degenerate;
  *n_duplicate = h->simp.n_duplicate;
  return EKF_OK;
}

int ekf_simplify_get(ekf_fusion* h, double* xyz, unsigned* faces, unsigned char* grey, unsigned char* bgr, float* normal,
                     unsigned long long* key, unsigned long long max_vert, unsigned long long max_tri) {
  return mesh_get(h, "ekf_simplify_get", 3, ": no ekf_simplify_run on the current mesh", "an ekf_simplify_run on a source without normals",
                  xyz, faces, grey, bgr, normal, key, max_vert, max_tri);
}

int ekf_simplify_get_map(ekf_fusion* h, unsigned* map, unsigned long long max_vert) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  const int rc = simplify_result(h, "ekf_simplify_get_map");
  if (rc != EKF_OK) return rc;
  std::string& err = f->err;
  const size_t nv = (size_t)std::min(h->simp.n_src_vert, max_vert);
  HIPCHK(hipSetDevice(f->device));
  if (nv > 0 && map) HIPCHK(hipMemcpy(map, h->simp.map, nv * sizeof(unsigned), hipMemcpyDeviceToHost));
  return EKF_OK;
}

int ekf_simplify_get_profile(const ekf_fusion* h, double* kernel_ms, long long* launches) {
  return fusion_profile(h, kernel_ms, launches, [&] { h->simp.timer.read(kernel_ms, launches, 0, ekf::kSimpKinds); });
}

// ---- a per-triangle texture atlas of the welded, the pruned, the smoothed or the simplified mesh ------------
// Whether the texture begun last is still that of the handle's meshes.
static int texture_current(ekf_fusion* h, const char* who) {
  if (h->stamps.has(h->stamps.tex, h->impl->changes)) return EKF_OK;
  h->impl->err = std::string(who) + ": no ekf_texture_begin on the current mesh";
  return EKF_ERR_STATE;
}

int ekf_texture_begin(ekf_fusion* h, int source, int patch, int channels, int* atlas_side) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  if (source < 0 || source > 3 || patch < ekf::kTexMinPatch || patch > ekf::kTexMaxPatch || (channels != 1 && channels != 3) ||
      !atlas_side) {
    f->err = "ekf_texture_begin: source 0, 1, 2 or 3, patch 2..32, channels 1 or 3, atlas_side not NULL";
    return EKF_ERR_ARG;
  }
  ekf::MeshView s;
  const int rc = mesh_source(h, "ekf_texture_begin", source, &s);
  if (rc != EKF_OK) return rc;
  if (s.n_tri == 0) {
    f->err = "ekf_texture_begin: the source mesh has no triangle";
    return EKF_ERR_STATE;
  }
  int B;
  long long Q, A;
  ekf::tex_layout(s.n_tri, patch, B, Q, A);
  if (A > ekf::kTexMaxSide) {
    f->err = "ekf_texture_begin: the atlas would be " + std::to_string(A) + " texels a side, more than 16384 (a smaller patch, or ekf_simplify_run first)";
    return EKF_ERR_ARG;
  }
  std::string& err = f->err;
  HIPCHK(hipSetDevice(f->device));
  HIPCHK(h->tex.begin(h->stamps, s, source, patch, channels, f->colour && channels == 3));
  *atlas_side = (int)A;
  return EKF_OK;
}

// What both ways of adding a view check after their own arguments: EKF_OK with *zbuf the z-buffer (NULL: occlusion off).
static int texture_view_ok(ekf_fusion* h, const char* who, int width, int height, int occlusion, const float** zbuf) {
  auto* f = h->impl;
  const int rc = texture_current(h, who);
  if (rc != EKF_OK) return rc;
  if (h->tex.finished) {
    f->err = std::string(who) + ": the texture is finished (ekf_texture_begin starts the next)";
    return EKF_ERR_STATE;
  }
  *zbuf = nullptr;
  if (occlusion) {
    if (!h->rc.current(*f) || h->rc.W != width || h->rc.H != height) {
      f->err = std::string(who) + ": occlusion needs an ekf_raycast_render of the view's size since the volume last changed";
      return EKF_ERR_STATE;
    }
    *zbuf = h->rc.depth;
  }
  return EKF_OK;
}

int ekf_texture_add_view(ekf_fusion* h, ekf_dense* dense, int slot, int occlusion, double tol, double min_area2,
                         unsigned long long* n_won) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  if (!dense || dense->impl->device != f->device) {
    f->err = "ekf_texture_add_view: a dense handle on the volume's device";
    return EKF_ERR_ARG;
  }
  auto* d = dense->impl;
  if (slot < 0 || slot >= d->max_views || (occlusion != 0 && occlusion != 1) || !std::isfinite(tol) || tol < 0.0 ||
      !std::isfinite(min_area2) || min_area2 < 0.0 || !n_won) {
    f->err = "ekf_texture_add_view: slot in 0..max_views-1, occlusion 0 or 1, tol and min_area2 finite and >= 0, n_won not NULL";
    return EKF_ERR_ARG;
  }
  const ekf::DenseView& v = d->v[slot];
  if (!v.set) {
    f->err = "ekf_texture_add_view: the slot is not set";
    return EKF_ERR_STATE;
  }
  const float* zbuf = nullptr;
  const int rc = texture_view_ok(h, "ekf_texture_add_view", d->W, d->H, occlusion, &zbuf);
  if (rc != EKF_OK) return rc;
  std::string& err = f->err;
  const unsigned char* bgr = h->tex.C == 3 ? d->colour_of(slot) : nullptr;
  HIPCHK(hipSetDevice(f->device));
  HIPCHK(h->tex.add_view(bgr ? bgr : (const unsigned char*)v.img, bgr ? 3 : 1, d->W, d->H, v.K, v.R, v.t, zbuf, tol, min_area2, n_won));
  return EKF_OK;
}

int ekf_texture_add_view_host(ekf_fusion* h, const unsigned char* img, int pitch, int channels, int width, int height, const double* K,
                              const double* pose7, int occlusion, double tol, double min_area2, unsigned long long* n_won) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  double t[3], R[9], q[4];
  if (!img || (channels != 1 && channels != 3) || width < 1 || height < 1 || width > ekf::kFusionMaxMapDim ||
      height > ekf::kFusionMaxMapDim || pitch < channels * width || !K || !pinhole_ok(K) || !pose7 || !ekf::dense_pose(pose7, t, R, q) ||
      (occlusion != 0 && occlusion != 1) || !std::isfinite(tol) || tol < 0.0 || !std::isfinite(min_area2) || min_area2 < 0.0 || !n_won) {
    f->err = "ekf_texture_add_view_host: img, K, pose7 and n_won not NULL; channels 1 or 3; 1 <= width, height <= 8192; pitch >= "
             "channels width; K finite with fx, fy > 0; pose7 finite with q != 0; occlusion 0 or 1; tol and min_area2 finite and >= 0";
    return EKF_ERR_ARG;
  }
  const float* zbuf = nullptr;
  const int rc = texture_view_ok(h, "ekf_texture_add_view_host", width, height, occlusion, &zbuf);
  if (rc != EKF_OK) return rc;
  std::string& err = f->err;
  ekf::TsdfTexture& m = h->tex;
  const size_t n = (size_t)width * height;
  const int vch = (channels == 3 && m.C == 3) ? 3 : 1;
  HIPCHK(hipSetDevice(f->device));
  HIPCHK(m.d_img.reserve(n * vch));
  if (channels == 3 && vch == 1) {                           // a colour view for a 1-channel atlas: its bgr2gray image
    std::vector<unsigned char> grey(n);
    for (int y = 0; y < height; ++y) {
      const unsigned char* row = img + (size_t)y * (size_t)pitch;
      for (int x = 0; x < width; ++x)
        grey[(size_t)y * width + x] = (unsigned char)((row[3 * x] * 1868u + row[3 * x + 1] * 9617u + row[3 * x + 2] * 4899u + 8192u) >> 14);
    }
    HIPCHK(hipMemcpy(m.d_img, grey.data(), n, hipMemcpyHostToDevice));
  } else {
    const size_t row = (size_t)vch * width;
    HIPCHK(hipMemcpy2D(m.d_img, row, img, (size_t)pitch, row, (size_t)height, hipMemcpyHostToDevice));
  }
  HIPCHK(m.add_view(m.d_img, vch, width, height, K, R, t, zbuf, tol, min_area2, n_won));
  return EKF_OK;
}

int ekf_texture_finish(ekf_fusion* h, unsigned long long* n_textured) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  if (!n_textured) {
    f->err = "ekf_texture_finish: n_textured must not be NULL";
    return EKF_ERR_ARG;
  }
  const int rc = texture_current(h, "ekf_texture_finish");
  if (rc != EKF_OK) return rc;
  if (h->tex.finished) {
    f->err = "ekf_texture_finish: the texture is finished (ekf_texture_begin starts the next)";
    return EKF_ERR_STATE;
  }
  std::string& err = f->err;
  HIPCHK(hipSetDevice(f->device));
  HIPCHK(h->tex.finish());
  *n_textured = h->tex.n_textured;
  return EKF_OK;
}

int ekf_texture_get(ekf_fusion* h, unsigned char* atlas, int pitch, double* uv, int* view, double* score, unsigned long long max_tri) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  const ekf::TsdfTexture& m = h->tex;
  const int rc = texture_current(h, "ekf_texture_get");
  if (rc != EKF_OK) return rc;
  const size_t row = (size_t)m.A * (size_t)m.C;
  if (atlas && (pitch < 0 || (size_t)pitch < row)) {
    f->err = "ekf_texture_get: pitch >= atlas_side channels";
    return EKF_ERR_ARG;
  }
  std::string& err = f->err;
  const size_t nt = (size_t)std::min(m.src.n_tri, max_tri);
  HIPCHK(hipSetDevice(f->device));
  if (atlas && (size_t)pitch == row) {                       // tight rows: one copy
    HIPCHK(hipMemcpy(atlas, m.atlas, row * (size_t)m.A, hipMemcpyDeviceToHost));
  } else if (atlas) {
    HIPCHK(hipMemcpy2D(atlas, (size_t)pitch, m.atlas, row, row, (size_t)m.A, hipMemcpyDeviceToHost));
  }
  if (uv)
    for (size_t t = 0; t < nt; ++t) ekf::tex_uv(t, m.P, m.B, m.Q, m.A, uv + 6 * t);
  if (nt > 0) {
    if (view) HIPCHK(hipMemcpy(view, m.best_view, nt * sizeof(int), hipMemcpyDeviceToHost));
    if (score) HIPCHK(hipMemcpy(score, m.best_score, nt * sizeof(double), hipMemcpyDeviceToHost));
  }
  return EKF_OK;
}

int ekf_texture_get_profile(const ekf_fusion* h, double* kernel_ms, long long* launches) {
  return fusion_profile(h, kernel_ms, launches, [&] { h->tex.timer.read(kernel_ms, launches, 0, ekf::kTexKinds); });
}

// ---- a rasteriser for the indexed meshes: depth, triangle, barycentric, normal and shaded images ------------
// What both ekf_*_set_mesh ask of the caller's rows (each says so in its own words).
static bool caller_mesh_ok(const double* xyz, const unsigned* faces, unsigned long long n_vert, unsigned long long n_tri) {
  bool ok = xyz && faces && n_vert > 0 && n_vert <= 0xffffffffull && n_tri > 0 && n_tri <= 0xffffffffull;
  for (unsigned long long i = 0; ok && i < n_vert * 3; ++i) ok = std::isfinite(xyz[i]);
  for (unsigned long long i = 0; ok && i < n_tri * 3; ++i) ok = faces[i] < n_vert;
  return ok;
}

int ekf_raster_set_mesh(ekf_fusion* h, const double* xyz, const unsigned* faces, const unsigned char* grey, const unsigned char* bgr,
                        unsigned long long n_vert, unsigned long long n_tri) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  if (!grey || !caller_mesh_ok(xyz, faces, n_vert, n_tri)) {
    f->err = "ekf_raster_set_mesh: xyz, faces and grey not NULL; 0 < n_vert, n_tri < 2^32; xyz finite; every index < n_vert";
    return EKF_ERR_ARG;
  }
  std::string& err = f->err;
  HIPCHK(hipSetDevice(f->device));
  HIPCHK(h->rast.own.upload(xyz, faces, grey, bgr, (size_t)n_vert, (size_t)n_tri));
  return EKF_OK;
}

// Everything of a render but the view: EKF_OK with the source's arrays and, for shading 1, the atlas; otherwise the status with
// the message set.  Arguments first, then the state.
static int raster_source(ekf_fusion* h, const char* who, int source, double z_near, int cull, int shading, int cover, ekf::MeshView* s,
                         ekf::RastAtlas* atlas) {
  auto* f = h->impl;
  if (source < 0 || source > 4 || !std::isfinite(z_near) || z_near < 0.0 || (cull != 0 && cull != 1) || (shading != 0 && shading != 1) ||
      (cover != 0 && cover != 1)) {
    f->err = std::string(who) + ": source 0..4; z_near finite and >= 0; cull, shading and cover 0 or 1";
    return EKF_ERR_ARG;
  }
  if (source == 4 && shading == 1) {
    f->err = std::string(who) + ": shading 1 needs a source with a texture: 0, 1, 2 or 3";
    return EKF_ERR_ARG;
  }
  if (source == 4) {
    if (!h->rast.own.set) {
      f->err = std::string(who) + ": source 4 needs an ekf_raster_set_mesh";
      return EKF_ERR_STATE;
    }
    *s = h->rast.own.view();
    return EKF_OK;
  }
  const int rc = mesh_source(h, who, source, s);
  if (rc != EKF_OK) return rc;
  if (s->n_tri == 0) {
    f->err = std::string(who) + ": the source mesh has no triangle";
    return EKF_ERR_STATE;
  }
  if (!f->colour) s->bgr = nullptr;
  if (shading == 1) {
    const ekf::TsdfTexture& t = h->tex;
    if (texture_current(h, who) != EKF_OK || !t.finished || h->stamps.tex.from != source) {
      f->err = std::string(who) + ": shading 1 needs a finished texture (ekf_texture_finish) of the source that is rendered";
      return EKF_ERR_STATE;
    }
    atlas->atlas = t.atlas; atlas->P = t.P; atlas->B = t.B; atlas->Q = (int)t.Q; atlas->A = (int)t.A; atlas->C = t.C;
  }
  return EKF_OK;
}

int ekf_raster_render(ekf_fusion* h, int source, int width, int height, const double* K, const double* pose7, double z_near, int cull,
                      int shading, int cover) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  double t[3], R[9], q[4];
  if (width < 1 || height < 1 || width > ekf::kRaycastMaxDim || height > ekf::kRaycastMaxDim || !K || !sba_finite(K, 4) || K[0] == 0.0 ||
      K[1] == 0.0 || !pose7 || !ekf::dense_pose(pose7, t, R, q)) {
    f->err = "ekf_raster_render: 1 <= width, height <= 8192; K finite with fx, fy != 0; pose7 finite with q != 0";
    return EKF_ERR_ARG;
  }
  ekf::MeshView s;
  ekf::RastAtlas atlas;
  const int rc = raster_source(h, "ekf_raster_render", source, z_near, cull, shading, cover, &s, &atlas);
  if (rc != EKF_OK) return rc;
  std::string& err = f->err;
  HIPCHK(hipSetDevice(f->device));
  HIPCHK(h->rast.render(s, shading ? &atlas : nullptr, width, height, K, R, t, z_near, cull, cover));
  return EKF_OK;
}

int ekf_raster_render_view(ekf_fusion* h, int source, ekf_dense* dense, int slot, double z_near, int cull, int shading, int cover) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  if (!dense || dense->impl->device != f->device) {
    f->err = "ekf_raster_render_view: a dense handle on the volume's device";
    return EKF_ERR_ARG;
  }
  auto* d = dense->impl;
  if (slot < 0 || slot >= d->max_views) {
    f->err = "ekf_raster_render_view: slot in 0..max_views-1";
    return EKF_ERR_ARG;
  }
  ekf::MeshView s;
  ekf::RastAtlas atlas;
  const int rc = raster_source(h, "ekf_raster_render_view", source, z_near, cull, shading, cover, &s, &atlas);
  if (rc != EKF_OK) return rc;
  const ekf::DenseView& v = d->v[slot];
  if (!v.set) {
    f->err = "ekf_raster_render_view: the slot is not set";
    return EKF_ERR_STATE;
  }
  std::string& err = f->err;
  HIPCHK(hipSetDevice(f->device));
  HIPCHK(h->rast.render(s, shading ? &atlas : nullptr, d->W, d->H, v.K, v.R, v.t, z_near, cull, cover));
  return EKF_OK;
}

int ekf_raster_get(ekf_fusion* h, float* depth, float* normal, unsigned char* grey, unsigned char* bgr, int* tri, float* bary,
                   unsigned* cover, int* width, int* height) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  const ekf::TsdfRaster& m = h->rast;
  if (!m.valid) {
    f->err = "ekf_raster_get: no ekf_raster_render";
    return EKF_ERR_STATE;
  }
  if ((bgr && !m.has_bgr) || (cover && !m.has_cover)) {
    f->err = "ekf_raster_get: bgr must be NULL when the render has no colour image, and cover when it was rendered with cover = 0";
    return EKF_ERR_ARG;
  }
  std::string& err = f->err;
  const size_t n = (size_t)m.W * (size_t)m.H;
  HIPCHK(hipSetDevice(f->device));
  if (depth) HIPCHK(hipMemcpy(depth, m.depth, n * sizeof(float), hipMemcpyDeviceToHost));
  if (normal) HIPCHK(hipMemcpy(normal, m.normal, n * 3 * sizeof(float), hipMemcpyDeviceToHost));
  if (grey) HIPCHK(hipMemcpy(grey, m.grey, n, hipMemcpyDeviceToHost));
  if (bgr) HIPCHK(hipMemcpy(bgr, m.bgr, n * 3, hipMemcpyDeviceToHost));
  if (tri) HIPCHK(hipMemcpy(tri, m.tri, n * sizeof(int), hipMemcpyDeviceToHost));
  if (bary) HIPCHK(hipMemcpy(bary, m.bary, n * 2 * sizeof(float), hipMemcpyDeviceToHost));
  if (cover) HIPCHK(hipMemcpy(cover, m.cover, n * sizeof(unsigned), hipMemcpyDeviceToHost));
  if (width) *width = m.W;
  if (height) *height = m.H;
  return EKF_OK;
}

int ekf_raster_set_small_limit(ekf_fusion* h, int limit) {
  if (!h) return EKF_ERR_ARG;
  if (limit < 0 || limit > (int)ekf::kRastMaxSmallLimit) {
    h->impl->err = "ekf_raster_set_small_limit: limit in 0..65536";
    return EKF_ERR_ARG;
  }
  h->rast.small_limit = (unsigned)limit;
  return EKF_OK;
}

int ekf_raster_get_profile(const ekf_fusion* h, double* kernel_ms, long long* launches) {
  return fusion_profile(h, kernel_ms, launches, [&] { h->rast.timer.read(kernel_ms, launches, 0, ekf::kRastKinds); });
}

// ---- a mesh-to-mesh distance: the nearest triangle of a target mesh for every query point ---------------------
int ekf_distance_set_mesh(ekf_fusion* h, const double* xyz, const unsigned* faces, unsigned long long n_vert, unsigned long long n_tri) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  if (!caller_mesh_ok(xyz, faces, n_vert, n_tri)) {
    f->err = "ekf_distance_set_mesh: xyz and faces not NULL; 0 < n_vert, n_tri < 2^32; xyz finite; every index < n_vert";
    return EKF_ERR_ARG;
  }
  std::string& err = f->err;
  HIPCHK(hipSetDevice(f->device));
  HIPCHK(h->dist.own.upload(xyz, faces, nullptr, nullptr, (size_t)n_vert, (size_t)n_tri));
  return EKF_OK;
}

// The rows of a source as the distance reads them: EKF_OK, or EKF_ERR_STATE with the message set.
static int distance_source(ekf_fusion* h, const char* who, int source, ekf::MeshView* s) {
  if (source != 4) return mesh_source(h, who, source, s);
  if (!h->dist.own.set) {
    h->impl->err = std::string(who) + ": source 4 needs an ekf_distance_set_mesh";
    return EKF_ERR_STATE;
  }
  *s = h->dist.own.view();
  return EKF_OK;
}

// The target of a run, then the run: what the two entry points share.  pts: the query's rows on the device.
static int distance_run(ekf_fusion* h, const char* who, const ekf::MeshView& t, const double* pts, unsigned long long n) {
  auto* f = h->impl;
  std::string& err = f->err;
  ekf::TsdfDistance::Status st;
  HIPCHK(h->dist.run(t, pts, n, &st));
  if (st == ekf::TsdfDistance::kNoValid) {
    f->err = std::string(who) + ": the target mesh has no valid triangle";
    return EKF_ERR_STATE;
  }
  if (st == ekf::TsdfDistance::kTooMany) {
    f->err = std::string(who) + ": 2^32 entries or more in the cell lists: use fewer cells (ekf_distance_set_grid)";
    return EKF_ERR_DEVICE;
  }
  return EKF_OK;
}

static int distance_target(ekf_fusion* h, const char* who, int target, ekf::MeshView* t) {
  const int rc = distance_source(h, who, target, t);
  if (rc != EKF_OK) return rc;
  if (t->n_tri == 0) {
    h->impl->err = std::string(who) + ": the target mesh has no valid triangle";
    return EKF_ERR_STATE;
  }
  return EKF_OK;
}

int ekf_distance_run(ekf_fusion* h, int target, int query, unsigned long long* n_points) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  if (target < 0 || target > 4 || query < 0 || query > 4) {
    f->err = "ekf_distance_run: target and query 0..4";
    return EKF_ERR_ARG;
  }
  ekf::MeshView t, q;
  int rc = distance_target(h, "ekf_distance_run", target, &t);
  if (rc != EKF_OK) return rc;
  if ((rc = distance_source(h, "ekf_distance_run", query, &q)) != EKF_OK) return rc;
  if (q.n_vert == 0) {
    f->err = "ekf_distance_run: the query mesh has no vertex";
    return EKF_ERR_STATE;
  }
  std::string& err = f->err;
  HIPCHK(hipSetDevice(f->device));
  rc = distance_run(h, "ekf_distance_run", t, q.xyz, q.n_vert);
  if (rc == EKF_OK && n_points) *n_points = q.n_vert;
  return rc;
}

int ekf_distance_run_points(ekf_fusion* h, int target, const double* xyz, unsigned long long n_points) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  if (target < 0 || target > 4 || !xyz || n_points < 1 || n_points > 0xffffffffull) {
    f->err = "ekf_distance_run_points: target 0..4; xyz not NULL; 0 < n_points < 2^32";
    return EKF_ERR_ARG;
  }
  ekf::MeshView t;
  const int rc = distance_target(h, "ekf_distance_run_points", target, &t);
  if (rc != EKF_OK) return rc;
  std::string& err = f->err;
  HIPCHK(hipSetDevice(f->device));
  HIPCHK(h->dist.set_points(xyz, (size_t)n_points));
  return distance_run(h, "ekf_distance_run_points", t, h->dist.q_xyz, n_points);
}

int ekf_distance_get(ekf_fusion* h, double* dist, unsigned* tri, double* closest, signed char* side, unsigned long long max_points) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  const ekf::TsdfDistance& m = h->dist;
  if (!m.valid) {
    f->err = "ekf_distance_get: no ekf_distance_run";
    return EKF_ERR_STATE;
  }
  if ((dist || tri || closest || side) && max_points < m.n_points) {
    f->err = "ekf_distance_get: max_points is less than the points of the run";
    return EKF_ERR_ARG;
  }
  std::string& err = f->err;
  const size_t n = (size_t)m.n_points;
  HIPCHK(hipSetDevice(f->device));
  if (dist) HIPCHK(hipMemcpy(dist, m.dist, n * sizeof(double), hipMemcpyDeviceToHost));
  if (tri) HIPCHK(hipMemcpy(tri, m.tri, n * sizeof(unsigned), hipMemcpyDeviceToHost));
  if (closest) HIPCHK(hipMemcpy(closest, m.closest, n * 3 * sizeof(double), hipMemcpyDeviceToHost));
  if (side) HIPCHK(hipMemcpy(side, m.side, n, hipMemcpyDeviceToHost));
  return EKF_OK;
}

int ekf_distance_get_stats(ekf_fusion* h, double thr, unsigned long long* n, unsigned long long* n_bad, double* max, unsigned long long* argmax,
                           double* mean, double* rms, unsigned long long* within) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  if (!(thr >= 0.0)) {
    f->err = "ekf_distance_get_stats: thr >= 0";
    return EKF_ERR_ARG;
  }
  if (!h->dist.valid) {
    f->err = "ekf_distance_get_stats: no ekf_distance_run";
    return EKF_ERR_STATE;
  }
  std::string& err = f->err;
  HIPCHK(hipSetDevice(f->device));
  ekf::DistSums s;
  HIPCHK(h->dist.stats(thr, &s));
  const unsigned long long good = h->dist.n_points - s.bad;
  const double nan = __builtin_nan("");
  if (n) *n = good;
  if (n_bad) *n_bad = s.bad;
  if (max) *max = good ? s.max : nan;
  if (argmax) *argmax = good ? s.argmax : 0xffffffffull;
  if (mean) *mean = good ? s.sum / (double)good : nan;
  if (rms) *rms = good ? std::sqrt(s.sum2 / (double)good) : nan;
  if (within) *within = s.within;
  return EKF_OK;
}

int ekf_distance_set_grid(ekf_fusion* h, int g) {
  if (!h) return EKF_ERR_ARG;
  if (g < 0 || g > (int)ekf::kDistMaxG) {
    h->impl->err = "ekf_distance_set_grid: g in 0..128";
    return EKF_ERR_ARG;
  }
  h->dist.grid_g = (unsigned)g;
  return EKF_OK;
}

int ekf_distance_get_grid(ekf_fusion* h, int* cells, unsigned long long* entries, unsigned* longest) {
  if (!h) return EKF_ERR_ARG;
  auto* f = h->impl;
  const ekf::TsdfDistance& m = h->dist;
  if (!m.valid) {
    f->err = "ekf_distance_get_grid: no ekf_distance_run";
    return EKF_ERR_STATE;
  }
  if (cells)
    for (int k = 0; k < 3; ++k) cells[k] = m.grid.G[k];
  if (entries) *entries = m.entries;
  if (longest) {
    std::string& err = f->err;
    std::vector<unsigned> cnt(m.ncell);
    HIPCHK(hipSetDevice(f->device));
    HIPCHK(hipMemcpy(cnt.data(), m.cnt, (size_t)m.ncell * sizeof(unsigned), hipMemcpyDeviceToHost));
    *longest = *std::max_element(cnt.begin(), cnt.end());
  }
  return EKF_OK;
}

int ekf_distance_get_profile(const ekf_fusion* h, double* kernel_ms, long long* launches) {
  return fusion_profile(h, kernel_ms, launches, [&] { h->dist.timer.read(kernel_ms, launches, 0, ekf::kDistKinds); });
}

}  // extern "C"
