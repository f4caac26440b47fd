// Ownership of device and pinned host memory (host-only): the one place that calls hipMalloc / hipFree /
// hipHostMalloc / hipHostFree.  A buffer is a member of what uses it and goes away with it; nothing is released by name.
// Beside the buffers, the small host state machines built on them and on events, each with its invariant in one place:
// KernelTimer (dense chain), WorkList, and the filter's ReadBack (pinned bounce buffer of the getters), InputRing (pinned
// input slots of an update) and LaunchProfiler (event pairs round launches).  Everything returns hipError_t; nothing here
// depends on the filter's scalar type, so tools/filter_host_check.cpp runs it on the CPU against stand-in HIP calls.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <utility>
#include <vector>

namespace ekf {

struct DeviceAlloc {
  static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static void release(void* p) { (void)hipFree(p); }
};
struct PinnedAlloc {
  static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void release(void* p) { (void)hipHostFree(p); }
};

// Move-only owner of `capacity()` elements of T.  It converts to T*, so launches, copies and pointer arithmetic read
// as they do with a raw pointer; it cannot be copied, so it cannot be passed by value by accident.
template <typename T, typename Alloc>
class Buf {
  T* p_ = nullptr;
  size_t cap_ = 0;

 public:
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_; cap_ = o.cap_;
      o.p_ = nullptr; o.cap_ = 0;
    }
    return *this;
  }
  ~Buf() { reset(); }

  // Room for `need` elements.  A buffer that has it is left alone (one comparison, no runtime call); one that has not is
  // freed -- its contents are lost -- and allocated again with max(need, grow_to) elements.  A failed allocation leaves
  // it empty.
  hipError_t reserve(size_t need, size_t grow_to = 0) {
    if (need <= cap_) return hipSuccess;
    reset();
    const size_t count = std::max(need, grow_to);
    void* q = nullptr;
    const hipError_t e = Alloc::alloc(&q, count * sizeof(T));
    if (e != hipSuccess) return e;
    p_ = static_cast<T*>(q);
    cap_ = count;
    return hipSuccess;
  }
  void reset() {
    if (p_) Alloc::release(p_);
    p_ = nullptr;
    cap_ = 0;
  }
  operator T*() const { return p_; }
  size_t capacity() const { return cap_; }
};

template <typename T> using DevBuf = Buf<T, DeviceAlloc>;
template <typename T> using PinnedBuf = Buf<T, PinnedAlloc>;

// Move-only owner of the six arrays of an indexed mesh and of its counts: the weld of ekf_mesh.hpp, its pruned copy and
// whatever is derived from them next.  The holder sets the counts once its kernels have filled the arrays.
template <typename Alloc>
struct IndexedMeshBufs {
  Buf<double, Alloc> xyz;                        // three a vertex, by ascending key
  Buf<unsigned long long, Alloc> key;
  Buf<unsigned char, Alloc> grey, bgr;           // bgr: three a vertex, colour volumes only
  Buf<float, Alloc> normal;                      // three a vertex, meshes with normals only
  Buf<unsigned, Alloc> faces;                    // three a triangle
  unsigned long long n_vert = 0, n_tri = 0;
  bool has_normals = false;

  // Room for nv vertices and ncorner face indices, bgr only with `colour`, normal only with `normals`.  Buffers that have it
  // are left alone.  Otherwise all six are replaced together, by new ones made beside them: a failed allocation returns its
  // error and leaves every buffer, and so the previous mesh, as it was.
  hipError_t grow(size_t nv, size_t ncorner, bool colour, bool normals) {
    if (nv * 3 <= xyz.capacity() && nv <= key.capacity() && nv <= grey.capacity() && (!colour || nv * 3 <= bgr.capacity()) &&
        (!normals || nv * 3 <= normal.capacity()) && ncorner <= faces.capacity())
      return hipSuccess;
    IndexedMeshBufs t;
    hipError_t e;
    if ((e = t.xyz.reserve(nv * 3)) != hipSuccess || (e = t.key.reserve(nv)) != hipSuccess || (e = t.grey.reserve(nv)) != hipSuccess ||
        (colour && (e = t.bgr.reserve(nv * 3)) != hipSuccess) || (normals && (e = t.normal.reserve(nv * 3)) != hipSuccess) ||
        (e = t.faces.reserve(ncorner)) != hipSuccess)
      return e;
    xyz = std::move(t.xyz);
    key = std::move(t.key);
    grey = std::move(t.grey);
    bgr = std::move(t.bgr);
    normal = std::move(t.normal);
    faces = std::move(t.faces);
    return hipSuccess;
  }
};
using DevMeshBufs = IndexedMeshBufs<DeviceAlloc>;

// Per-kernel times of N kinds of launch on the null stream of the owner's device, behind a switch.  Off: run() makes no
// event call at all.  On: it records round the launch, waits for the second event and adds the time to the kind's pair.
// The first failing HIP call's error is returned and nothing is added.  The timer is a member of its owner: like the
// buffers it is destroyed after the owner's destructor body, which selects the device the events were made on.
template <int N>
class KernelTimer {
  hipEvent_t ev_[2] = {nullptr, nullptr};
  bool on_ = false;
  double ms_[N] = {};
  long long cnt_[N] = {};

 public:
  KernelTimer() = default;
  KernelTimer(const KernelTimer&) = delete;
  KernelTimer& operator=(const KernelTimer&) = delete;
  ~KernelTimer() {
    for (hipEvent_t e : ev_)
      if (e) (void)hipEventDestroy(e);
  }

  hipError_t create() {                 // on the current device; an event that exists is kept
    hipError_t e = hipSuccess;
    for (int i = 0; i < 2 && e == hipSuccess; ++i)
      if (!ev_[i]) e = hipEventCreate(&ev_[i]);
    return e;
  }
  void enable(bool on) {                // on or off, the counters start from zero
    on_ = on;
    for (int i = 0; i < N; ++i) { ms_[i] = 0.0; cnt_[i] = 0; }
  }
  void read(double* ms, long long* cnt, int first, int count) const {
    for (int i = 0; i < count; ++i) { ms[i] = ms_[first + i]; cnt[i] = cnt_[first + i]; }
  }
  // begin (if on) -> launch() -> hipGetLastError -> end (if on)
  template <typename F>
  hipError_t run(int which, F launch) {
    hipError_t e;
    if (on_ && (e = hipEventRecord(ev_[0], nullptr)) != hipSuccess) return e;
    launch();
    if ((e = hipGetLastError()) != hipSuccess || !on_) return e;
    e = hipEventRecord(ev_[1], nullptr);
    if (e == hipSuccess) e = hipEventSynchronize(ev_[1]);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev_[0], ev_[1]);
    if (e == hipSuccess) { ms_[which] += ms; cnt_[which] += 1; }
    return e;
  }
};

// A device list of ints that is rebuilt when the key it was built for changes.  The caller drains the streams that may
// still read the old list before it calls upload().  The key is the ONLY record of what the list holds: an owner that has to
// know (first() is the leading key element, by convention the block-step count of a plan) reads it from here, and one that
// wants the list rebuilt clears it.
struct WorkList {
  std::vector<int> key;
  DevBuf<int> d;
  bool current(const std::vector<int>& k) const { return key == k; }
  int first() const { return key.empty() ? 0 : key[0]; }
  hipError_t upload(const std::vector<int>& k, const std::vector<int>& host, size_t min_elems = 1) {
    key.clear();
    hipError_t e = d.reserve(std::max(host.size(), min_elems));
    if (e == hipSuccess && !host.empty()) e = hipMemcpy(d, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) key = k;
    return e;
  }
};

// Small device -> host reads through ONE pinned bounce buffer: several pieces per synchronisation (a copy into pageable
// memory is staged by the runtime and costs ~25 us).  add() / add_2d() queue a copy into the buffer on `st` and remember where
// the piece belongs; finish() synchronises `st` once and hands every piece to its place.  Invariant: the pieces in `pend_` lie
// inside the live buffer below `off_`, 16-byte aligned, and whichever call fails leaves nothing queued and the offset at 0,
// so the next batch starts clean.  A piece that does not fit behind the queued ones makes them be delivered first (the
// buffer may then move); one larger than the buffer grows it to max(64 KiB, twice the piece).
class ReadBack {
  struct Piece { void* dst; size_t off, bytes; };
  PinnedBuf<char> h_;
  size_t off_ = 0;
  std::vector<Piece> pend_;

  void drop() { pend_.clear(); off_ = 0; }
  hipError_t deliver(hipStream_t st) {
    const hipError_t e = hipStreamSynchronize(st);
    if (e == hipSuccess)
      for (const Piece& p : pend_) memcpy(p.dst, static_cast<const char*>(h_) + p.off, p.bytes);
    drop();
    return e;
  }
  hipError_t reserve(size_t bytes, hipStream_t st) {
    if (off_ + bytes + 64 <= h_.capacity()) return hipSuccess;
    if (!pend_.empty()) {                              // pieces already queued: deliver them before the buffer moves
      const hipError_t e = deliver(st);
      if (e != hipSuccess || bytes + 64 <= h_.capacity()) return e;
    }
    off_ = 0;
    return h_.reserve(bytes + 64, std::max<size_t>(1 << 16, 2 * (bytes + 64)));
  }
  // room for the piece, then copy(place in the buffer); the ONE place a failed batch is dropped
  template <typename Copy>
  hipError_t queue(void* dst, size_t bytes, hipStream_t st, Copy copy) {
    hipError_t e = reserve(bytes, st);
    if (e == hipSuccess) e = copy(static_cast<char*>(h_) + off_);
    if (e != hipSuccess) { drop(); return e; }
    pend_.push_back({dst, off_, bytes});
    off_ += (bytes + 15) & ~size_t(15);
    return hipSuccess;
  }

 public:
  // queue `bytes` from device `src` for host `dst`
  hipError_t add(void* dst, const void* src, size_t bytes, hipStream_t st) {
    return queue(dst, bytes, st, [&](char* at) { return hipMemcpyAsync(at, src, bytes, hipMemcpyDeviceToHost, st); });
  }
  // queue `rows` rows of `row_bytes` (device pitch in bytes), packed row-major at dst
  hipError_t add_2d(void* dst, const void* src, size_t pitch, size_t row_bytes, int rows, hipStream_t st) {
    return queue(dst, row_bytes * rows, st, [&](char* at) {
      return hipMemcpy2DAsync(at, row_bytes, src, pitch, row_bytes, rows, hipMemcpyDeviceToHost, st);
    });
  }
  // one synchronisation for everything queued, then the pieces go to their places
  hipError_t finish(hipStream_t st) { return deliver(st); }
  size_t capacity() const { return h_.capacity(); }
  size_t offset() const { return off_; }
  size_t pending() const { return pend_.size(); }
};

// The measurements of a host caller on their way to the device: kSlots pinned slots used in turn, so that the copies of
// one update may still be in flight while the next is staged.  A slot holds z (2 M scalars), the index list (M ints, behind
// room for 2 * capacity scalars) and 7 scalars of camera pose (behind room for capacity indices).  Invariant: a slot is
// written only after the event recorded behind its last copies has passed.
class InputRing {
 public:
  static constexpr int kSlots = 4;

 private:
  PinnedBuf<char> h_[kSlots];
  hipEvent_t ev_[kSlots] = {};
  bool used_[kSlots] = {};
  int slot_ = 0;
  size_t elem_ = 0, cap_ = 0;

 public:
  InputRing() = default;
  InputRing(const InputRing&) = delete;
  InputRing& operator=(const InputRing&) = delete;
  ~InputRing() { release(); }
  void configure(size_t scalar_bytes, size_t capacity) { elem_ = scalar_bytes; cap_ = capacity; }
  // the events go (the owner has drained the stream); the pinned slots go with the ring
  void release() {
    for (hipEvent_t& e : ev_) { if (e) (void)hipEventDestroy(e); e = nullptr; }
    for (bool& u : used_) u = false;
  }
  // z -> d_z, idx -> d_idx and, if given, cam7 -> d_cam, in this order on `st`
  hipError_t stage(hipStream_t st, int M, void* d_z, const void* z, void* d_idx, const int* idx, void* d_cam = nullptr,
                   const void* cam7 = nullptr) {
    const size_t zb = (size_t)2 * M * elem_, ib = (size_t)M * sizeof(int);
    const size_t idx_off = 2 * cap_ * elem_, cam_off = cap_ * (2 * elem_ + sizeof(int));
    const int s = slot_;
    slot_ = (slot_ + 1) % kSlots;
    hipError_t e = hipSuccess;
    if (!h_[s]) {
      if ((e = h_[s].reserve(cam_off + 8 * elem_ + 64)) != hipSuccess) return e;
      if ((e = hipEventCreateWithFlags(&ev_[s], hipEventDisableTiming)) != hipSuccess) return e;
    }
    if (used_[s] && (e = hipEventSynchronize(ev_[s])) != hipSuccess) return e;   // the copies that last used this slot are long done
    char* base = h_[s];
    memcpy(base, z, zb);
    memcpy(base + idx_off, idx, ib);
    if ((e = hipMemcpyAsync(d_z, base, zb, hipMemcpyHostToDevice, st)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(d_idx, base + idx_off, ib, hipMemcpyHostToDevice, st)) != hipSuccess) return e;
    if (cam7) {
      memcpy(base + cam_off, cam7, 7 * elem_);
      if ((e = hipMemcpyAsync(d_cam, base + cam_off, 7 * elem_, hipMemcpyHostToDevice, st)) != hipSuccess) return e;
    }
    if ((e = hipEventRecord(ev_[s], st)) != hipSuccess) return e;
    used_[s] = true;
    return hipSuccess;
  }
};

// Times of N kinds of launch by event pairs on the launch's own stream, resolved later so that nothing waits per launch.
// `mode` (EKF_OPT_PROFILE): 0 off, 1 the two dominant kinds, 2 every kind, 3 the dominant kinds on every kSamplePeriod-th
// frame.  A Scope round a launch records a pair when its kind is on and queues it; resolve() drains the streams, adds the
// times and returns the events to the pool.  Invariant: every event made here is in exactly one of `pending_` and `pool_`
// (or held by a live Scope), so release() destroys each once.
template <int N>
class LaunchProfiler {
  struct Pending { int kid; hipEvent_t a, b; };
  std::vector<Pending> pending_;
  std::vector<hipEvent_t> pool_;
  int dominant_[2];
  double ms_[N] = {};
  long long cnt_[N] = {};

  hipEvent_t get_event() {
    if (!pool_.empty()) { hipEvent_t e = pool_.back(); pool_.pop_back(); return e; }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
  }

 public:
  static constexpr int kSamplePeriod = 8;
  int mode = 0;
  long long frame_seq = 0;                              // updates since the last reset (mode 3 samples on it)
  double work[N] = {};                                  // algorithmic flop of the timed launches, added by the launch site

  LaunchProfiler(int dominant_a, int dominant_b) : dominant_{dominant_a, dominant_b} {}
  LaunchProfiler(const LaunchProfiler&) = delete;
  LaunchProfiler& operator=(const LaunchProfiler&) = delete;
  ~LaunchProfiler() { release(); }

  bool on(int kid) const {
    if (mode == 2) return true;
    const bool dominant = (kid == dominant_[0] || kid == dominant_[1]);
    if (mode == 1) return dominant;
    if (mode == 3) return dominant && (frame_seq % kSamplePeriod == 0);   // every 8th frame: an event pair costs ~6 us of queue time
    return false;
  }
  struct Scope {
    LaunchProfiler& p; int kid; hipEvent_t a = nullptr, b = nullptr; bool on; hipStream_t st;
    Scope(LaunchProfiler& p_, int kid_, hipStream_t st_) : p(p_), kid(kid_), on(p_.on(kid_)), st(st_) {
      if (on) { a = p.get_event(); b = p.get_event(); (void)hipEventRecord(a, st); }
    }
    ~Scope() {
      if (on) { (void)hipEventRecord(b, st); p.pending_.push_back({kid, a, b}); }
    }
  };
  // the three streams the owner launches on (the third may be null), drained before the pairs are read
  void resolve(hipStream_t main, hipStream_t side, hipStream_t gather) {
    if (pending_.empty()) return;
    (void)hipStreamSynchronize(main);
    (void)hipStreamSynchronize(side);
    if (gather) (void)hipStreamSynchronize(gather);
    for (const Pending& q : pending_) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, q.a, q.b) == hipSuccess) { ms_[q.kid] += ms; cnt_[q.kid] += 1; }
      pool_.push_back(q.a); pool_.push_back(q.b);
    }
    pending_.clear();
  }
  void read(int kid, double* ms, long long* cnt) const { if (ms) *ms = ms_[kid]; if (cnt) *cnt = cnt_[kid]; }
  void reset() {                                        // (after resolve(): what is pending would count again)
    frame_seq = 0;
    for (int i = 0; i < N; ++i) { ms_[i] = 0.0; cnt_[i] = 0; work[i] = 0.0; }
  }
  // every event goes: the pending pairs, then the pool (the owner has drained its streams)
  void release() {
    for (const Pending& q : pending_) { (void)hipEventDestroy(q.a); (void)hipEventDestroy(q.b); }
    for (hipEvent_t e : pool_) (void)hipEventDestroy(e);
    pending_.clear();
    pool_.clear();
  }
};

}  // namespace ekf
