// Ownership of device and pinned host memory (host-only): the one place that calls hipMalloc / hipFree /
// hipHostMalloc / hipHostFree.  A buffer is a member of what uses it and goes away with it; nothing is released by name.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
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

}  // namespace ekf
