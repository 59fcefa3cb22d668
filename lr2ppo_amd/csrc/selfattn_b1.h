// What the two single-plane training attention sources share -- selfattn_b1_train.hip (one LDS-resident head, L <= 288) and
// selfattn_b1_blocked.hip (key / query blocks, any L): the fragment, staging, tile-product and store helpers on ONE bf16 plane, the
// launchers' argument pack and the alignment check.  (selfattn_common.h's helpers are two-plane.)
#pragma once
#include "selfattn_common.h"

namespace {

constexpr int B1_NW = 8;      // waves per workgroup: two per SIMD, <= 256 registers each -- 18 S tiles + 18 dP tiles fit unspilled

// 16 rows x 64 columns of ONE plane as MFMA fragments (lane: row l & 15, columns 8 (l >> 4) + 32 ks ..); !ok: zeros
__device__ __forceinline__ void b1_load_frags(const bf16_t* plane, size_t elem_off, bool ok, bf16x8_t (&f)[2]) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    u32x4_t a = {0, 0, 0, 0};
    if (ok) a = *reinterpret_cast<const u32x4_t*>(plane + elem_off + 32 * ks);
    f[ks] = __builtin_bit_cast(bf16x8_t, a);
  }
}
// rows 0 .. 16 NT - 1 of one head's operands A and B into LDS, both in the K image (each is read as row fragments AND transposed);
// rows >= L are zeros.  Every request first, then the LDS writes.
template <int NT, int NTHR>
__device__ __forceinline__ void b1_stage_rows2(const bf16_t* __restrict__ a, int ld_a, const bf16_t* __restrict__ b, int ld_b, size_t row0,
                                               int col0, int L, int tid, char* sA, char* sB) {
  constexpr int LP = 16 * NT, TRIPS = (LP * 8 + NTHR - 1) / NTHR;
  u32x4_t av[TRIPS], bv[TRIPS];
#pragma unroll
  for (int it = 0; it < TRIPS; ++it) {
    const int i = tid + it * NTHR;
    const int r = i >> 3, u = i & 7;
    av[it] = u32x4_t{0, 0, 0, 0};
    bv[it] = av[it];
    if (i < LP * 8 && r < L) {
      av[it] = *reinterpret_cast<const u32x4_t*>(a + (row0 + r) * (size_t)ld_a + col0 + u * 8);
      bv[it] = *reinterpret_cast<const u32x4_t*>(b + (row0 + r) * (size_t)ld_b + col0 + u * 8);
    }
  }
#pragma unroll
  for (int it = 0; it < TRIPS; ++it) {
    const int i = tid + it * NTHR;
    const int r = i >> 3, u = i & 7;
    if (i < LP * 8) {
      *reinterpret_cast<u32x4_t*>(sA + k_off(r, u)) = av[it];
      *reinterpret_cast<u32x4_t*>(sB + k_off(r, u)) = bv[it];
    }
  }
}
// rows 16t .. 16t + 15 of the staged A and B against this lane's x and y fragments: a = A_t x^T, d = B_t y^T
__device__ __forceinline__ void b1_s_dp_tile(const char* sA, const char* sB, int t, int lane, const bf16x8_t (&x)[2], const bf16x8_t (&y)[2],
                                             f32x4_t& a, f32x4_t& d) {
  a = f32x4_t{0.f, 0.f, 0.f, 0.f};
  d = a;
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const int o = k_off(16 * t + (lane & 15), (lane >> 4) + 4 * ks);
    a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8_t*>(sA + o), x[ks], a, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8_t*>(sB + o), y[ks], d, 0, 0, 0);
  }
}
// acc += E^T X over rows 32u .. 32u + 31 of the staged X (transposed reads), E = this lane's 8 values of those rows, rounded to bf16
__device__ __forceinline__ void b1_accum_block(const float (&e)[8], const char* sX, int u, int lane, f32x4_t (&acc)[4]) {
  const int tq = (lane & 15) >> 2, tp = lane & 3;
  const u32x4_t ew = {cvt_pk_bf16(e[0], e[1]), cvt_pk_bf16(e[2], e[3]), cvt_pk_bf16(e[4], e[5]), cvt_pk_bf16(e[6], e[7])};
  const bf16x8_t ef = __builtin_bit_cast(bf16x8_t, ew);
  const int ra = 32 * u + 4 * (lane >> 4) + tq, rb = ra + 16;
#pragma unroll
  for (int n = 0; n < 4; ++n)
    acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ef, tr_pair_k(sX, ra, rb, 2 * n + (tp >> 1), 8 * (tp & 1)), acc[n], 0, 0, 0);
}
// 16 x 64 accumulator tile (o[n][r] = X[row 4g + r][col 16n + (l & 15)]) -> rows of ONE bf16 plane via the wave's LDS slab
__device__ __forceinline__ void b1_store_tile(const f32x4_t (&o)[4], float* slab, int lane, int row_first, int rows_valid, bf16_t* dst,
                                              size_t row_stride, size_t base) {
  const int qn = lane & 15, g = lane >> 4;
#pragma unroll
  for (int n = 0; n < 4; ++n)
#pragma unroll
    for (int r = 0; r < 4; ++r) slab[(4 * g + r) * (HD + 4) + 16 * n + qn] = o[n][r];
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {
    const int r = pass * 4 + (lane >> 4), c = (lane & 15) * 4;
    if (row_first + r < rows_valid) {
      const float4 v = *reinterpret_cast<const float4*>(slab + r * (HD + 4) + c);
      store_bf16x4(dst + base + (size_t)(row_first + r) * row_stride + c, v);
    }
  }
  __builtin_amdgcn_wave_barrier();
}

struct B1Args {
  const bf16_t *q, *k, *v;
  int ld;
  const int64_t* seg;
  int batch, heads, L;
  float scale;
  DropP dr;
  hipStream_t stream;
};

inline bool b1_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace
