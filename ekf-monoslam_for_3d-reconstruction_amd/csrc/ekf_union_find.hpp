// The lock-free union-find that the speckle filter (ekf_dense_speckle.hpp) and the components of the welded
// mesh (ekf_mesh_components.hpp, §25) share: the accessors of a forest of unsigned words, seg_find and seg_union.
//
// The forest.  L[x] <= x always; x is a root iff L[x] = x; a word only ever decreases, and only to the index of an element of
// the same set, or of one that the writing lane is in the course of uniting with it.  seg_find walks x, L[x], L[L[x]], ...,
// a strictly decreasing sequence of indices, to a root; seg_union finds both roots and hooks the larger to the smaller with
// fetch_min.  If the value fetch_min returns is not the root it was aimed at, another lane has hooked that word in the
// meantime: the union goes on with the returned value, which is smaller.  So every loop here runs down a chain of strictly
// decreasing indices >= 0 and ends after at most as many steps as the forest has words, whatever other lanes or workgroups
// do at the same time; no lane ever waits for another: no flag, no spin, no ordered hand-over.
#pragma once

namespace ekf {

// The accessors of the forest.  Global (words that workgroups share while a launch runs: k_speckle_merge, k_comp_union):
// relaxed atomics of agent scope, which go to the memory all CUs share and never to a CU's own L1.  Lds (the tile's forest in
// k_speckle_label and the counters of k_speckle_count): relaxed atomics of workgroup scope, so that a lane re-reads a word
// another lane may have lowered.  The host checks (tools/speckle_host_check.cpp, tools/component_host_check.cpp) define
// EKF_SPECKLE_HOST_ATOMICS and the same six functions with the __atomic builtins before they include this header.
#ifndef EKF_SPECKLE_HOST_ATOMICS
__device__ __forceinline__ unsigned seg_global_load(const unsigned* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned seg_global_min(unsigned* p, unsigned v) {
  return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned seg_global_add(unsigned* p, unsigned v) {
  return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned seg_lds_load(const unsigned* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ unsigned seg_lds_min(unsigned* p, unsigned v) {
  return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ unsigned seg_lds_add(unsigned* p, unsigned v) {
  return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
#endif

struct SegGlobal {
  static __device__ __forceinline__ unsigned load(const unsigned* p) { return seg_global_load(p); }
  static __device__ __forceinline__ unsigned fetch_min(unsigned* p, unsigned v) { return seg_global_min(p, v); }
};
struct SegLds {
  static __device__ __forceinline__ unsigned load(const unsigned* p) { return seg_lds_load(p); }
  static __device__ __forceinline__ unsigned fetch_min(unsigned* p, unsigned v) { return seg_lds_min(p, v); }
};

// The root of x.  On the way every visited word is lowered to its grandparent (path halving, by fetch_min: the word keeps
// whatever smaller value another lane has given it meanwhile), which keeps the chains of the later calls short.
template <typename A>
__device__ __forceinline__ unsigned seg_find(unsigned* L, unsigned x) {
  unsigned p = A::load(L + x);                                               // p <= x
  while (p != x) {
    const unsigned g = A::load(L + p);                                       // g <= p < x
    if (g != p) A::fetch_min(L + x, g);
    x = p;
    p = g;
  }
  return x;
}

// a and b in one set from now on.  (a, b) -> (old, lo) with old < hi = max(a, b): a + b falls with every turn.
template <typename A>
__device__ __forceinline__ void seg_union(unsigned* L, unsigned a, unsigned b) {
  for (;;) {
    a = seg_find<A>(L, a);
    b = seg_find<A>(L, b);
    if (a == b) return;
    const unsigned hi = max(a, b), lo = min(a, b);
    const unsigned old = A::fetch_min(L + hi, lo);
    if (old == hi) return;                                                   // hi was a root and now hangs below lo
    a = old;                                                                 // hi had been hooked to old < hi by another lane
    b = lo;
  }
}

}  // namespace ekf
