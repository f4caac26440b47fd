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
