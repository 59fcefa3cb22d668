// 256 x 256 "ping-pong" product of SINGLE f16 planes:  C[M,N] = A[M,K] . B[N,K]^T  (one v_mfma_f32_16x16x32_f16 product per tile
// pair, fp32 accumulate) -- the "f16" inference mode (FeatureExtractor(precision="f16")): BASELINE.json configs[2]'s 16-bit dtype in
// the form that keeps 11 significand bits per operand.  NOT the parity path (gemm256.hip's three-product split-bf16 kernel stays the
// default everywhere), and gemm256_b1.hip's twin: the f16 MFMA has the bf16 one's operand bytes and fragment layout, so the ring, the
// LDS-DMA staging and the fragment reads of gemm256_ring.h serve it unchanged.
//
// Replaces, in that mode, the cuBLAS calls reached through nn.Linear in the encoders (tencentpretrain/layers/
// multi_headed_attn.py:55-76, position_ffn.py:12-15) -- the same sites as the bf16 mode; same fused epilogue (gemm_common.h: alpha,
// bias, GELU, residual).
//
// What is this kernel's own against gemm256_b1.hip:
//   * the MFMA section is __builtin_amdgcn_mfma_f32_16x16x32_f16 on the same 16-byte fragments;
//   * the result leaves as fp32 and / or ONE f16 plane (common.h::f16_pack4: clamp to +-65504, round to nearest even;
//     Epilogue::lo_off == 0) or bf16 hi / lo planes (lo_off != 0: the operands of the 3-pass attention kernels, as ever).  The plane
//     format is a compile-time property of these instantiations (gemm_common.h's F16), as EXACT is of lr2_gemm_bf16_train's.
#include "gemm256_ring.h"

namespace lr2gemm {
namespace g256h {

using namespace ring256;
constexpr int BN = 256, BK = 64;
constexpr int LDS_BYTES = RING;

// 16 MFMAs of one accumulator quadrant: k-half 0 of the 8 tiles, then k-half 1 (gemm256_b1.hip's section on the f16 MFMA).  The ring
// hands the fragments over as 16 raw bytes (k_step_bf16's bf16x8_t): only the instruction gives them a format.
struct HalfProductsF16 {
  template <int AH, int BH, int MIH>
  static __device__ __forceinline__ void mfma_section(f32x4_t (&acc)[2 * MIH][4], const bf16x8_t (&a0)[MIH], const bf16x8_t (&a1)[MIH],
                                                      const bf16x8_t (&b0)[2], const bf16x8_t (&b1)[2]) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int i = 0; i < MIH; ++i)
        acc[AH * MIH + i][BH * 2 + j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
            __builtin_bit_cast(f16x8_t, a0[i]), __builtin_bit_cast(f16x8_t, b0[j]), acc[AH * MIH + i][BH * 2 + j], 0, 0, 0);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int i = 0; i < MIH; ++i)
        acc[AH * MIH + i][BH * 2 + j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
            __builtin_bit_cast(f16x8_t, a1[i]), __builtin_bit_cast(f16x8_t, b1[j]), acc[AH * MIH + i][BH * 2 + j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    section_barrier();
  }
};

// MIH = accumulator tiles per half of a wave's rows: 4 -> the 256 x 256 tile; 3 -> the 192 x 256 tile of gemm256.hip.
template <int MIH>
__global__ __launch_bounds__(512, 2) void gemm256_f16_kernel(GemmParams g) {
  constexpr int BMT = 64 * MIH, WMT = 32 * MIH;      // tile rows, wave-tile rows
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;

  int tm, tn;
  tile_coords(g.tiles_m, g.tiles_n, blockIdx.x, tm, tn);
  const int m0 = tm * BMT, n0 = tn * BN;

  Ctx<OnePlane> c;
  c.nt = g.K / BK;
  c.src.a = uniform_rsrc(g.A, g.a_bytes);
  c.src.b = uniform_rsrc(g.B, g.b_bytes);
  lane_setup<MIH>(c, smem, m0, n0, wave, lane, (uint64_t)g.lda * 2u, (uint64_t)g.ldb * 2u, g.M, g.N);

  f32x4_t acc[2 * MIH][4];
#pragma unroll
  for (int i = 0; i < 2 * MIH; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  prologue<NoExtras>(c, wr);
  for (int t = 0; t < c.nt; t += 2) {
    k_step_bf16<HalfProductsF16, 0, MIH>(c, t, acc);
    if (t + 1 < c.nt) k_step_bf16<HalfProductsF16, 1, MIH>(c, t + 1, acc);
  }
  drain(wr);

  float* slab = reinterpret_cast<float*>(smem) + wave * (32 * (64 + 4));
  epilogue_wave<WMT, 64, 2 * MIH, 4, 1, 3, false, true>(g, acc, slab, m0 + wr * WMT, n0 + wc * 64, lane, nullptr);
}

}  // namespace g256h

int gemm256_nt_tile_rows(int M, int N);   // gemm256.hip

// Host entry for lr2_gemm_f16.  Requirements (checked by the caller): single planes, NT, K % 64 == 0, operand extents
// < 4 GiB - 512 B, an inference epilogue (at most the residual as a per-element request).
int launch_gemm256_f16(const GemmParams& p_in, hipStream_t stream) {
  using namespace g256h;
  GemmParams p = p_in;
  const int bm = gemm256_nt_tile_rows(p.M, p.N);
  p.tiles_m = (p.M + bm - 1) / bm;
  p.tiles_n = (p.N + BN - 1) / BN;
  static bool attr_set = false;
  if (!attr_set) {
    if (lr2_allow_dynamic_lds(gemm256_f16_kernel<4>, LDS_BYTES, "gemm256_f16")) return LR2_ERR_LAUNCH;
    if (lr2_allow_dynamic_lds(gemm256_f16_kernel<3>, LDS_BYTES, "gemm256_f16(192 rows)")) return LR2_ERR_LAUNCH;
    attr_set = true;
  }
  if (bm == 192) LR2_LAUNCH(gemm256_f16_kernel<3>, dim3(p.tiles_m * p.tiles_n), dim3(512), LDS_BYTES, stream, p);
  else LR2_LAUNCH(gemm256_f16_kernel<4>, dim3(p.tiles_m * p.tiles_n), dim3(512), LDS_BYTES, stream, p);
  return lr2_launch_status(__func__);
}

}  // namespace lr2gemm
