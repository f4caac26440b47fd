// What the host checks of the reconstruction kernels share (DESIGN.md sections 15.5, 16.5, 17.5, 19.5): stand-ins for the HIP
// names a kernel body uses, a launch that runs the 256 lanes of a workgroup as host threads (a pthread barrier for
// __syncthreads, `static` arrays for LDS, the workgroups one after another), the case-file reader's take, the bit-for-bit
// differs and main.  Include it before the csrc headers, which then give their structs and kernel bodies alone, and define
// `static int run(const char* path)`: 0 = equal, 1 = differs, 2 = unreadable.  Build with the sanitizers on:
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread
//           tools/X_host_check.cpp -o X_host_check
// Usage: X_host_check case.bin [...]; prints "ok" when every case is equal.
#pragma once
#include <pthread.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

struct Idx3 { unsigned x, y, z; };
static thread_local Idx3 threadIdx, blockIdx;
static Idx3 blockDim = {256, 1, 1};
static pthread_barrier_t g_barrier;
#define __global__
#define __device__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(...)
#define __restrict__
#define __syncthreads() pthread_barrier_wait(&g_barrier)
using std::max;
using std::min;
#ifndef __clang__
#define __builtin_assume(x) ((void)0)                       // a hint to the device compiler (csrc/ekf_dense_stereo.hpp)
#endif
#define EKF_KERNELS_ONLY

// A kernel that reads another lane's register (csrc/ekf_dense_sgm.hpp: wave_read, the device's __shfl) gets exactly that
// here: an exchange array and a barrier per wave of 64 lanes.  Every lane of the wave must make the call.
static pthread_barrier_t g_wave_barrier[4];
static int g_wave_xch[4][64];
static inline int wave_read(int v, int src) {
  const unsigned w = threadIdx.x >> 6;
  g_wave_xch[w][threadIdx.x & 63] = v;
  pthread_barrier_wait(&g_wave_barrier[w]);
  const int got = g_wave_xch[w][src & 63];
  pthread_barrier_wait(&g_wave_barrier[w]);
  return got;
}

// body() once per lane of every workgroup of `grid`.  The barrier after a workgroup keeps its LDS from the next one's lanes.
template <typename F>
static void launch(Idx3 grid, F body) {
  std::vector<std::thread> lanes;
  for (unsigned t = 0; t < 256; ++t)
    lanes.emplace_back([=] {
      threadIdx = {t, 0, 0};
      for (unsigned by = 0; by < grid.y; ++by)
        for (unsigned bx = 0; bx < grid.x; ++bx) {
          blockIdx = {bx, by, 0};
          body();
          pthread_barrier_wait(&g_barrier);
        }
    });
  for (auto& l : lanes) l.join();
}

// The launcher that a launch plan of csrc takes (ekf::sweep_launches): the library's times and launches, this one runs the
// kernel the plan chose on the grid it chose.  0: made, as every launch here is.
struct HostGo {
  template <typename Grid, typename Kernel, typename... Args>
  int operator()(int, Grid grid, Kernel kernel, const Args&... args) const {
    launch({grid.x, grid.y, 1}, [&] { kernel(args...); });
    return 0;
  }
};

template <typename T>
static std::vector<T> take(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) { std::fprintf(stderr, "short case file\n"); std::exit(2); }
  return v;
}

template <typename T>
static int differs(const char* what, const std::vector<T>& got, const std::vector<T>& want) {
  size_t n = got.size() != want.size();
  for (size_t i = 0; i < std::min(got.size(), want.size()); ++i) n += std::memcmp(&got[i], &want[i], sizeof(T)) != 0;
  if (n) std::printf("  %s: %zu of %zu differ\n", what, n, want.size());
  return n != 0;
}

static int run(const char* path);

int main(int argc, char** argv) {
  pthread_barrier_init(&g_barrier, nullptr, 256);
  for (auto& w : g_wave_barrier) pthread_barrier_init(&w, nullptr, 64);
  int rc = argc > 1 ? 0 : 64;
  for (int i = 1; i < argc; ++i) rc |= run(argv[i]);
  if (rc == 0) std::printf("ok\n");
  return rc;
}
