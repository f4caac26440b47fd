// k_ncc_search and k_blur_templates of csrc/ekf_image.hpp, float and double, run lane by lane on the host (DESIGN.md section
// 7.1) by host_kernels.hpp, which says how to build and run this.  It reads the case files tools/image_host_check.py writes
// (the raw inputs in buffers of exactly the device's sizes, and the outputs of oracle/image_oracle.py) and compares bit for
// bit.  The LDS arrays of the kernels are `static` here, so AddressSanitizer guards their ends: the staged region's 16-byte
// tail, the `rr[k + 1]` read and the tap list are checked, not argued.
#include "host_kernels.hpp"

// the three device builtins the search uses, in plain C++
static inline unsigned __builtin_amdgcn_alignbyte(unsigned hi, unsigned lo, unsigned sh) {   // v_alignbyte_b32
  return (unsigned)((((unsigned long long)hi << 32) | lo) >> (8 * (sh & 3)));
}
static inline int __builtin_amdgcn_udot4(unsigned a, unsigned b, int c, bool) {               // v_dot4_u32_u8, no clamp
  unsigned s = (unsigned)c;
  for (int k = 0; k < 4; ++k) s += ((a >> (8 * k)) & 0xffu) * ((b >> (8 * k)) & 0xffu);
  return (int)s;
}
static inline int atomicAdd(int* p, int v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }

#include "../ekf-monoslam_for_3d-reconstruction_amd/csrc/ekf_image.hpp"

template <typename T>
static int run_search(const char* path, FILE* f, int N, int w, int fw, int fh, float sigma_size, float threshold) {
  const size_t w2 = (size_t)w * w;
  const auto frame = take<unsigned char>(f, (size_t)fw * fh);
  const auto h = take<T>(f, 2 * (size_t)N);
  const auto Sd = take<T>(f, 4 * (size_t)N);
  const auto flags = take<unsigned char>(f, N);
  auto mpatch = take<unsigned char>(f, N * w2);
  const auto w_found = take<unsigned char>(f, N);
  const auto w_z = take<T>(f, 2 * (size_t)N);
  const auto w_score = take<float>(f, N);
  const auto w_mpatch = take<unsigned char>(f, N * w2);
  std::vector<unsigned char> found(N, 0xA5);
  std::vector<T> z(2 * (size_t)N, T(-7));
  std::vector<float> score(N, -7.f);
  launch({(unsigned)N, 1, 1}, [&] {
    ekf::k_ncc_search<T>(frame.data(), fw, fh, h.data(), Sd.data(), flags.data(), w, sigma_size, threshold, mpatch.data(),
                         z.data(), found.data(), score.data());
  });
  size_t nf = 0;
  for (unsigned char v : found) nf += v == 1;
  const int bad = differs("found", found, w_found) + differs("z", z, w_z) + differs("score", score, w_score) +
                  differs("matching templates", mpatch, w_mpatch);
  std::printf("%s: search, %s, %d features, window %d, frame %d x %d, %zu found: %s\n", path, sizeof(T) == 8 ? "double" : "float",
              N, w, fw, fh, nf, bad ? "DIFFERS" : "equal");
  return bad ? 1 : 0;
}

template <typename T>
static int run_blur(const char* path, FILE* f, int N, int w, int kernel_min_size) {
  const size_t w2 = (size_t)w * w;
  const auto h = take<T>(f, 2 * (size_t)N);
  const auto hb = take<T>(f, 2 * (size_t)N);
  const auto flags = take<unsigned char>(f, N);
  const auto patch = take<unsigned char>(f, N * w2);
  auto mpatch = take<unsigned char>(f, N * w2);
  const auto w_mpatch = take<unsigned char>(f, N * w2);
  launch({(unsigned)N, 1, 1}, [&] {
    ekf::k_blur_templates<T>(h.data(), hb.data(), flags.data(), w, kernel_min_size, patch.data(), mpatch.data());
  });
  const int bad = differs("matching templates", mpatch, w_mpatch);
  std::printf("%s: blur, %s, %d features, window %d, kernel_size %d: %s\n", path, sizeof(T) == 8 ? "double" : "float", N, w,
              kernel_min_size, bad ? "DIFFERS" : "equal");
  return bad ? 1 : 0;
}

static int run(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::perror(path); return 2; }
  const auto hdr = take<int>(f, 8);
  const auto par = take<float>(f, 2);
  const int kind = hdr[0], dbl = hdr[1], N = hdr[2], w = hdr[3];
  int rc;
  if (kind == 0) rc = dbl ? run_search<double>(path, f, N, w, hdr[4], hdr[5], par[0], par[1])
                          : run_search<float>(path, f, N, w, hdr[4], hdr[5], par[0], par[1]);
  else rc = dbl ? run_blur<double>(path, f, N, w, hdr[6]) : run_blur<float>(path, f, N, w, hdr[6]);
  std::fclose(f);
  return rc;
}
