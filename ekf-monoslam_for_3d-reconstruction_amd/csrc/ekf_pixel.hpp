// The one B, G, R -> grey conversion of the library and the byte pick that goes with its word loads, in a
// header of their own: ekf_image.hpp (frame ingest) and the dense chain (§18) share them, and the host checks of the dense
// chain can include them without the HIP runtime (the including file supplies __device__ and __forceinline__).
#pragma once

namespace ekf {

__device__ __forceinline__ unsigned bgr2gray(unsigned b, unsigned g, unsigned r) {
  return (b * 1868u + g * 9617u + r * 4899u + 8192u) >> 14;
}

// byte i of a little-endian word array (i is a compile-time constant after unrolling: one v_bfe_u32)
__device__ __forceinline__ unsigned byte_of(const unsigned* w, int i) { return (w[i >> 2] >> (8 * (i & 3))) & 0xffu; }

}  // namespace ekf
