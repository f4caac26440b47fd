// Trailing update of block step j AND the diagonal factor of step j + 1 as ONE launch (k_trail_diag, round 6; the default
// chain): the per-step sequence was diag(j) -> panel(j) -> trailing(j) -> diag(j + 1) ..., three launches of which the
// factor -- one workgroup, 17 us -- had the chip to itself.  Here workgroup 0 first applies step j's update to the diagonal
// block (j + 1, j + 1) ITSELF -- its operands, the rows of P(j; j + 1), are final before the launch: no hand-over inside
// it -- straight into the factor's LDS image, factors it and writes L_(j+1) and Dinv_(j+1), while every other workgroup
// takes one 128 x 128 block of the trailing update (four 64 x 64 tiles of k_gemm_mfma<TRAILING>'s arithmetic).  Each
// element is the same sum of the same products in the same order as in the per-step launches -- the result is
// BIT-IDENTICAL (tests/test_gpu_parity.py::test_launch_structure_knobs_are_bit_identical, EKF_CHAIN_FUSED_DIAG=0).  A step
// costs panel + max(update + factor, trailing) instead of their sum.  Ordinary loads and stores: the hand-overs are launch
// boundaries.
#pragma once
#include "ekf_dense.hpp"

namespace ekf {

constexpr unsigned kChainPimg = 75776;           // LDS: the image of the rows of P(j; j+1) (64 KB) behind the diagonal block's arrays
constexpr unsigned kChainLds = 141568;           // dynamic LDS of k_trail_diag (the image ends at 141312; 256 bytes spare)

namespace chain {
typedef float f4 __attribute__((ext_vector_type(4)));
typedef __amdgpu_buffer_rsrc_t rsrc_t;

// buffer accesses, default cache policy
__device__ __forceinline__ f4 ld16(rsrc_t r, unsigned byte_off) {
  return __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)byte_off, 0, 0));
}
__device__ __forceinline__ float ld4(rsrc_t r, unsigned byte_off) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)byte_off, 0, 0));
}
__device__ __forceinline__ void st4(rsrc_t r, unsigned byte_off, float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, (int)byte_off, 0, 0);
}

// ---- T(j; I, K): block (I, K) -= P(j; I) P(j; K)^T ------------------------------------------------------------
// Four groups of four waves, group (gr, gc) = the 64 x 64 tile at (64 gr, 64 gc) of the block with its own two LDS
// stages -- the tile body of k_gemm_mfma<ROLE_TRAILING, false, 64, 64> (LDS image [k / 4][row][4] with slot = q 64 +
// (row ^ q), one barrier per K step, fragment ping-pong; lane half h of MFMA e of group s multiplies k = 8 s + 4 h + e;
// accumulators from zero, C enters once in the epilogue: C' = fma(-1, acc, C)).  On a diagonal block the tile (0, 1)
// is not computed (the per-step launch skips tiles above the diagonal too).
__device__ __attribute__((noinline)) void trail(rsrc_t ry, unsigned ldy, int j, int I, int K, int only, f32x4* lds_all, int tid,
                                                int lane, int wave) {
  constexpr int NQ = 8, TS = 64, STAGE = NQ * (TS + TS), BK = 32, NG = BK / 8;
  const int grp = wave >> 2, gr = grp >> 1, gc = grp & 1;
  // only >= 0: only the tile of group `only` (k_trail_diag passes -1: the whole block)
  const bool active = !(I == K && gr == 0 && gc == 1) && (only < 0 || only == grp);
  f32x4* lds = lds_all + grp * 2 * STAGE;
  const int t = tid & 255, w4 = wave & 3, wr = w4 >> 1, wc = w4 & 1;
  const int h = lane >> 5, l31 = lane & 31;
  const int arow0 = I * 128 + gr * 64, brow0 = K * 128 + gc * 64, kcol0 = j * 128;
  unsigned aoff[2], boff[2];
  int aslot[2], bslot[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int idx = t + 256 * p;
    const int row = idx >> 3, q = idx & 7;
    aoff[p] = (((unsigned)(arow0 + row)) * ldy + (unsigned)(kcol0 + q * 4)) * 4u;
    boff[p] = (((unsigned)(brow0 + row)) * ldy + (unsigned)(kcol0 + q * 4)) * 4u;
    aslot[p] = q * TS + (row ^ q);
    bslot[p] = q * TS + (row ^ q);
  }
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  f4 ra[2], rb[2];
  auto load_tile = [&](int k0) {
#pragma unroll
    for (int p = 0; p < 2; ++p) { ra[p] = ld16(ry, aoff[p] + 4u * k0); rb[p] = ld16(ry, boff[p] + 4u * k0); }
  };
  auto store_tile = [&](int stage) {
    f32x4* As = lds + stage * STAGE;
    f32x4* Bs = As + NQ * TS;
#pragma unroll
    for (int p = 0; p < 2; ++p) { As[aslot[p]] = ra[p]; Bs[bslot[p]] = rb[p]; }
  };
  f32x4 fa[2], fb[2];
  auto read_frag = [&](int stage, int s, int buf) {
    const f32x4* As = lds + stage * STAGE;
    const f32x4* Bs = As + NQ * TS;
    const int q = 2 * s + h;
    fa[buf] = As[q * TS + ((wr * 32 + l31) ^ q)];
    fb[buf] = Bs[q * TS + ((wc * 32 + l31) ^ q)];
  };
  auto mfma_group = [&](int buf) {
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[buf][e], fb[buf][e], acc, 0, 0, 0);
  };
  // (each workgroup runs ONE block: no earlier use of the LDS to separate these stores from)
  if (active) { load_tile(0); store_tile(0); load_tile(BK); }
  __syncthreads();
  if (active) read_frag(0, 0, 0);
  int stage = 0;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    const bool more = ks < 3, more2 = ks < 2;
#pragma unroll
    for (int s = 0; s < NG; ++s) {
      if (s + 1 < NG) {
        if (active) read_frag(stage, s + 1, (s + 1) & 1);
      } else {
        __syncthreads();                         // stage ^ 1 is complete, everybody has read this stage
        if (active && more) read_frag(stage ^ 1, 0, 0);
      }
      if (active) mfma_group(s & 1);
      if (s == 0 && more && active) {
        store_tile(stage ^ 1);
        if (more2) load_tile(BK * (ks + 2));
      }
    }
    stage ^= 1;
  }
  if (!active) return;
  // epilogue: acc register e of a lane = row (e & 3) + 8 (e >> 2) + 4 h, column l31 of the wave's 32 x 32 block
  const unsigned c = (unsigned)(brow0 + wc * 32 + l31);
  const unsigned rbase = (unsigned)(arow0 + wr * 32 + 4 * h);
  float v[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) v[e] = 1.f * ld4(ry, ((rbase + (e & 3) + 8 * (e >> 2)) * ldy + c) * 4u);
#pragma unroll
  for (int e = 0; e < 16; ++e) v[e] = __builtin_fmaf(-1.f, acc[e], v[e]);
#pragma unroll
  for (int e = 0; e < 16; ++e) st4(ry, ((rbase + (e & 3) + 8 * (e >> 2)) * ldy + c) * 4u, v[e]);
}

// T(.; blk, blk): the lower 32 x 32 blocks, wave w < 10 = block (bi, bj); both operands from the image of the panel rows,
// C in `cv` (requested earlier with load_diag_c); the result goes into the diagonal block's LDS image, zeros above the diagonal
__device__ __forceinline__ void load_diag_c(rsrc_t ry, unsigned ldy, int blk, int wave, int lane, float (&cv)[16]) {
  const int h = lane >> 5, l31 = lane & 31;
  const int bi = wave >= 6 ? 3 : (wave >= 3 ? 2 : (wave >= 1 ? 1 : 0)), bj = wave - bi * (bi + 1) / 2;
  if (wave < 10) {
    const unsigned c = (unsigned)(blk * 128 + 32 * bj + l31), r0 = (unsigned)(blk * 128 + 32 * bi + 4 * h);
#pragma unroll
    for (int e = 0; e < 16; ++e) cv[e] = ld4(ry, ((r0 + (e & 3) + 8 * (e >> 2)) * ldy + c) * 4u);
  }
}
__device__ __forceinline__ void update_diag_image(const f32x4* pimg, float* a, int wave, int lane, const float (&cv)[16]) {
  constexpr int LDA = 132;
  const int h = lane >> 5, l31 = lane & 31;
  if (wave < 10) {
    const int bi = wave >= 6 ? 3 : (wave >= 3 ? 2 : (wave >= 1 ? 1 : 0)), bj = wave - bi * (bi + 1) / 2;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int sg = 0; sg < 4; ++sg) {
        const int q = 2 * sg + h, kq = ks * 8 + q;
        const f32x4 fa = pimg[kq * 128 + ((32 * bi + l31) ^ q)];
        const f32x4 fb = pimg[kq * 128 + ((32 * bj + l31) ^ q)];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[e], fb[e], acc, 0, 0, 0);
      }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = 32 * bi + (e & 3) + 8 * (e >> 2) + 4 * h, col = 32 * bj + l31;
      const float v = __builtin_fmaf(-1.f, acc[e], 1.f * cv[e]);
      a[row * LDA + col] = (col <= row) ? v : 0.f;
    }
  } else {
    // the six blocks above the diagonal: zeros (the factorisation builds Z there)
    const int u = wave - 10;
    const int zi = u < 3 ? 0 : (u < 5 ? 1 : 2), zj = u < 3 ? u + 1 : (u < 5 ? u - 1 : 3);
#pragma unroll
    for (int r = 0; r < 16; ++r) a[(32 * zi + 16 * h + r) * LDA + 32 * zj + l31] = 0.f;
  }
}
}  // namespace chain

struct TrailDiagArgs {
  float* Y; int ldy; unsigned y_bytes;
  float* Dinv; unsigned dinv_bytes;
  int* status;
  int m;                                         // real rows of S
  int j;                                         // the step whose trailing update this is
  const int* blocks; int nblocks;                // (I, K) pairs: the blocks of the update EXCEPT (j + 1, j + 1)
  int do_diag;                                   // 1: workgroup 0 = block (j + 1, j + 1) + the factor of step j + 1
};

__global__ void __launch_bounds__(1024) k_trail_diag(TrailDiagArgs g) {
  using namespace chain;
  extern __shared__ __attribute__((aligned(16))) unsigned char chain_smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(g.Y, 0, (int)g.y_bytes, 0x27000);
  const unsigned ldy = (unsigned)g.ldy;
  __builtin_amdgcn_s_setprio(2);
  if (g.do_diag && blockIdx.x == 0) {
    const int j = g.j, blk = g.j + 1;
    float* a = reinterpret_cast<float*>(chain_smem);
    f32x4* pimg = reinterpret_cast<f32x4*>(chain_smem + kChainPimg);
    // the rows of P(j; j + 1) -> the operand image (slot = kq 128 + (row ^ (kq & 7)), kq = k / 4); C = block (blk, blk)
    f4 v[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int idx = tid + 1024 * p, row = idx >> 5, kq = idx & 31;
      v[p] = ld16(ry, (((unsigned)(blk * 128 + row)) * ldy + (unsigned)(j * 128 + 4 * kq)) * 4u);
    }
    float cv[16];
    load_diag_c(ry, ldy, blk, wave, lane, cv);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int idx = tid + 1024 * p, row = idx >> 5, kq = idx & 31;
      pimg[kq * 128 + (row ^ (kq & 7))] = v[p];
    }
    __syncthreads();
    update_diag_image(pimg, a, wave, lane, cv);
    const DiagLds L{a, reinterpret_cast<float(*)[16 * 20]>(a + 128 * 132),
                    reinterpret_cast<float(*)[16]>(a + 128 * 132 + 2 * 16 * 20), a + 128 * 132 + 2 * 16 * 20 + 2 * 16};
    diag_factor_lds<7>(g.status, max(1, min(8, (g.m - blk * 128 + 15) / 16)), L);      // (starts with a barrier)
    float* Ab = g.Y + (size_t)blk * 128 * g.ldy + (size_t)blk * 128;
    float* Db = g.Dinv + (size_t)blk * 128 * 128;
    const int ld_ = g.ldy;
    diag_store_lds([&](int i, int j0, const f4& x) { *reinterpret_cast<f4*>(Ab + (size_t)i * ld_ + j0) = x; },
                   [&](int i, int jj, float x) { Db[(size_t)i * 128 + jj] = x; }, a);
    return;
  }
  const int t = (int)blockIdx.x - g.do_diag;
  if (t >= g.nblocks) return;
  const int I = g.blocks[2 * t], K = g.blocks[2 * t + 1];
  trail(ry, ldy, g.j, I, K, -1, reinterpret_cast<f32x4*>(chain_smem), tid, lane, wave);
}

}  // namespace ekf
