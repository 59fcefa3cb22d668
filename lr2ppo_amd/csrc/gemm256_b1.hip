// 256 x 256 "ping-pong" product of SINGLE bf16 planes:  C[M,N] = A[M,K] . B[N,K]^T  (one v_mfma_f32_16x16x32_bf16 product per
// tile pair, fp32 accumulate) -- the "bf16" mode of BASELINE.json configs[2] (FeatureExtractor(precision="bf16")).  NOT the parity
// path: an operand keeps 8 mantissa bits (gemm256.hip's three-product split-bf16 kernel stays the default everywhere).
//
// Replaces, in that mode, the cuBLAS calls reached through nn.Linear in the encoders (tencentpretrain/layers/
// multi_headed_attn.py:55-76, position_ffn.py:12-15) -- the same sites as the MX-FP8 mode (gemm256_mx.hip); same contract as
// lr2_gemm's NT form at passes = 1, same fused epilogue (gemm_common.h: alpha, bias, GELU, residual).
//
// Structure: the skeleton of gemm256.hip, unchanged where it can be -- one workgroup of 8 waves per CU, tile 256 x 256 (or
// 192 x 256, MIH = 3), wave (wr, wc) of a 2 x 4 grid owns 128 x 64 = 8 x 4 accumulator tiles, an LDS ring of 2 stages x 4 parts
// (A rows of accumulator half 0 / 1, B columns of half 0 / 1) filled by LDS-DMA with COUNTED s_waitcnt vmcnt and bare s_barrier,
// two wave groups one section apart, the XOR swizzle applied to the DMA's SOURCE address, out-of-range refills past the last step.
// What differs:
//   * a K step is 64 deep.  The slot that holds the lo plane of a part there holds k 32 .. 63 of the SAME plane here: a part is
//     two 8-KiB images [128 rows][4 units of 16 B] (k 0 .. 31, k 32 .. 63), the two DMA pieces of a wave read the same rows 64
//     bytes apart.  Same piece count, same ds_read_b128 pattern, same 64 KiB per step, same counted waits.
//   * an MFMA section is 16 products (two k-halves x 8 tiles) instead of 24: a step is 64 MFMAs per wave for 64 KiB staged.
//   * K must be a whole number of 64-deep steps; ragged M / N through the descriptors' zero fill and explicit out-of-range
//     offsets for rows >= M / columns >= N.
//   * the result leaves as fp32 and / or ONE bf16 plane (round to nearest even; Epilogue::lo_off == 0) or hi / lo planes.
#include "gemm_common.h"

namespace lr2gemm {
namespace g256b {

constexpr int BN = 256, BK = 64;
constexpr int HALF_K = 128 * 32 * 2;   // one k-half of one part: 128 rows x 32 k x 2 B = 8 KiB
constexpr int PART = 2 * HALF_K;       // k 0 .. 31, then k 32 .. 63
constexpr int STAGE = 4 * PART;        // parts A0, B0, B1, A1
constexpr int LDS_BYTES = 2 * STAGE;   // 128 KiB
constexpr int SLOT_A0 = 0, SLOT_B0 = 1, SLOT_B1 = 2, SLOT_A1 = 3;
constexpr uint32_t OOB = 0xFFFFFF00u;  // voffset beyond any descriptor this library builds (operands are < 4 GiB - 512 B)

__device__ __forceinline__ int swz(int r) { return (4 - ((r >> 2) & 3)) & 3; }

template <int IMM>
__device__ __forceinline__ bf16x8_t lds_read16(uint32_t addr) {
  u32x4_t v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(IMM));
  return __builtin_bit_cast(bf16x8_t, v);
}

struct Ctx {
  __amdgpu_buffer_rsrc_t a, b;
  uint32_t voff_a[2], voff_b[2];   // per-lane source byte offsets of this wave's piece of part A(ah) / B(bh) at K step 0, k-half 0
  uint32_t rd_a[2], rd_b[2];       // per-lane LDS read bases for stage 0 / 1
  char* smem;
  int wave, nt;
};

// Two DMA pieces (k 0 .. 31 and k 32 .. 63 of 16 rows) of one part for K step `tile` into stage `stage`.
template <int SLOT, bool IS_A, int HALF>
__device__ __forceinline__ void issue_part(const Ctx& c, int tile, int stage) {
  const uint32_t base = IS_A ? c.voff_a[HALF] : c.voff_b[HALF];
  const bool in = tile < c.nt && base != OOB;
  const uint32_t v0 = in ? base + (uint32_t)tile * (BK * 2) : OOB;
  const uint32_t v1 = in ? v0 + 64u : OOB;
  char* dst = c.smem + stage * STAGE + SLOT * PART + c.wave * 1024;
  __builtin_amdgcn_raw_ptr_buffer_load_lds(IS_A ? c.a : c.b, LDS_PTR(dst), 16, v0, 0, 0, 0);
  __builtin_amdgcn_raw_ptr_buffer_load_lds(IS_A ? c.a : c.b, LDS_PTR(dst + HALF_K), 16, v1, 0, 0, 0);
}

template <int SLOT, int MIH>
__device__ __forceinline__ void read_a_half(uint32_t base, bf16x8_t (&k0)[MIH], bf16x8_t (&k1)[MIH]) {
  k0[0] = lds_read16<SLOT * PART + 0 * 1024>(base);
  k0[1] = lds_read16<SLOT * PART + 1 * 1024>(base);
  k0[2] = lds_read16<SLOT * PART + 2 * 1024>(base);
  if constexpr (MIH == 4) k0[3] = lds_read16<SLOT * PART + 3 * 1024>(base);
  k1[0] = lds_read16<SLOT * PART + HALF_K + 0 * 1024>(base);
  k1[1] = lds_read16<SLOT * PART + HALF_K + 1 * 1024>(base);
  k1[2] = lds_read16<SLOT * PART + HALF_K + 2 * 1024>(base);
  if constexpr (MIH == 4) k1[3] = lds_read16<SLOT * PART + HALF_K + 3 * 1024>(base);
}
template <int SLOT>
__device__ __forceinline__ void read_b_half(uint32_t base, bf16x8_t (&k0)[2], bf16x8_t (&k1)[2]) {
  k0[0] = lds_read16<SLOT * PART + 0 * 1024>(base);
  k0[1] = lds_read16<SLOT * PART + 1 * 1024>(base);
  k1[0] = lds_read16<SLOT * PART + HALF_K + 0 * 1024>(base);
  k1[1] = lds_read16<SLOT * PART + HALF_K + 1 * 1024>(base);
}

// End of a LOAD section (gemm256.hip): counted wait for the DMA parts the NEXT load section reads, retire this section's fragment
// reads, meet the other group.
template <int VM>
__device__ __forceinline__ void end_load_section() {
  constexpr int imm = (VM & 15) | ((VM >> 4) << 14) | (7 << 4) | (0 << 8);
  __builtin_amdgcn_s_waitcnt(imm);
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

// 16 MFMAs of one accumulator quadrant: k-half 0 of the 8 tiles, then k-half 1 -- eight independent accumulators between two
// updates of the same one.
template <int AH, int BH, int MIH>
__device__ __forceinline__ void mfma_section(f32x4_t (&acc)[2 * MIH][4], const bf16x8_t (&a0)[MIH], const bf16x8_t (&a1)[MIH],
                                             const bf16x8_t (&b0)[2], const bf16x8_t (&b1)[2]) {
  __builtin_amdgcn_s_setprio(1);
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int i = 0; i < MIH; ++i)
      acc[AH * MIH + i][BH * 2 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0[i], b0[j], acc[AH * MIH + i][BH * 2 + j], 0, 0, 0);
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int i = 0; i < MIH; ++i)
      acc[AH * MIH + i][BH * 2 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1[i], b1[j], acc[AH * MIH + i][BH * 2 + j], 0, 0, 0);
  __builtin_amdgcn_s_setprio(0);
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

// One K step (tile t, compile-time stage S): gemm256.hip's refill order and counted waits (2 pieces per part):
//   0: B0(t+1) [other stage]  1: A0(t+2)  2: B1(t+2)  3: A1(t+2)
template <int S, int MIH>
__device__ __forceinline__ void k_step(const Ctx& c, int t, f32x4_t (&acc)[2 * MIH][4]) {
  bf16x8_t a0[MIH], a1[MIH], b0[2], b1[2];
  // phase 0: quadrant (A0, B0)
  issue_part<SLOT_B0, false, 0>(c, t + 1, S ^ 1);
  read_a_half<SLOT_A0, MIH>(c.rd_a[S], a0, a1);
  read_b_half<SLOT_B0>(c.rd_b[S], b0, b1);
  end_load_section<12>();
  mfma_section<0, 0, MIH>(acc, a0, a1, b0, b1);
  // phase 1: (A0, B1)
  issue_part<SLOT_A0, true, 0>(c, t + 2, S);
  read_b_half<SLOT_B1>(c.rd_b[S], b0, b1);
  end_load_section<12>();
  mfma_section<0, 1, MIH>(acc, a0, a1, b0, b1);
  // phase 2: (A1, B1)
  issue_part<SLOT_B1, false, 1>(c, t + 2, S);
  read_a_half<SLOT_A1, MIH>(c.rd_a[S], a0, a1);
  end_load_section<12>();
  mfma_section<1, 1, MIH>(acc, a0, a1, b0, b1);
  // phase 3: (A1, B0)
  issue_part<SLOT_A1, true, 1>(c, t + 2, S);
  read_b_half<SLOT_B0>(c.rd_b[S], b0, b1);
  end_load_section<6>();
  mfma_section<1, 0, MIH>(acc, a0, a1, b0, b1);
}

// MIH = accumulator tiles per half of a wave's rows: 4 -> the 256 x 256 tile; 3 -> the 192 x 256 tile of gemm256.hip (same ring: an
// A part then holds 96 rows, the waves whose 16-row pieces fall beyond them issue out-of-range requests).
template <int MIH>
__global__ __launch_bounds__(512, 2) void gemm256_b1_kernel(GemmParams g) {
  constexpr int BMT = 64 * MIH, WMT = 32 * MIH;      // tile rows, wave-tile rows
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;

  int tm, tn;
  tile_coords(g.tiles_m, g.tiles_n, blockIdx.x, tm, tn);
  const int m0 = tm * BMT, n0 = tn * BN;

  Ctx c;
  c.smem = smem;
  c.wave = wave;
  c.nt = g.K / BK;
  c.a = uniform_rsrc(g.A, g.a_bytes);
  c.b = uniform_rsrc(g.B, g.b_bytes);
  {
    // this wave's 1-KiB piece of a k-half = local rows wave*16 .. +16; lane l fills unit (l & 3) of row (l >> 2), which holds
    // K chunk (l & 3) ^ swz(row) of that half's 32 elements
    const int lr = wave * 16 + (lane >> 2);
    const uint32_t ku = (uint32_t)((lane & 3) ^ swz(lr)) * 16u;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      // part A(h): rows wr*WMT + h*(WMT/2) + [0, WMT/2) of both wr (part-local row lr = wr*(WMT/2) + that index)
      const int awr = lr / (WMT / 2), ain = lr - awr * (WMT / 2);
      const int arow = m0 + awr * WMT + h * (WMT / 2) + ain;
      const int bcol = n0 + (lr >> 5) * 64 + h * 32 + (lr & 31);    // part B(h): cols wc*64 + h*32 + [0, 32) of all wc
      const uint64_t oa = (uint64_t)arow * (uint64_t)g.lda * 2u + ku;
      const uint64_t ob = (uint64_t)bcol * (uint64_t)g.ldb * 2u + ku;
      c.voff_a[h] = (lr < WMT && arow < g.M && oa < (uint64_t)OOB) ? (uint32_t)oa : OOB;
      c.voff_b[h] = (bcol < g.N && ob < (uint64_t)OOB) ? (uint32_t)ob : OOB;
    }
    const int r16 = lane & 15;
    const uint32_t lane_off = (uint32_t)(r16 * 64 + (((lane >> 4) ^ swz(r16)) * 16));
    const uint32_t sm = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      c.rd_a[s] = sm + s * STAGE + wr * (MIH * 1024) + lane_off;     // A part: local row wr*(16 MIH) + i*16 + r16
      c.rd_b[s] = sm + s * STAGE + wc * 2048 + lane_off;             // B part: local row wc*32 + j*16 + r16
    }
  }

  f32x4_t acc[2 * MIH][4];
#pragma unroll
  for (int i = 0; i < 2 * MIH; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // prologue: everything of K steps 0 and 1 except B0(1), in the steady-state issue order
  issue_part<SLOT_A0, true, 0>(c, 0, 0);
  issue_part<SLOT_B1, false, 1>(c, 0, 0);
  issue_part<SLOT_A1, true, 1>(c, 0, 0);
  issue_part<SLOT_B0, false, 0>(c, 0, 0);
  issue_part<SLOT_A0, true, 0>(c, 1, 1);
  issue_part<SLOT_B1, false, 1>(c, 1, 1);
  issue_part<SLOT_A1, true, 1>(c, 1, 1);
  end_load_section<6>();                        // A0(0), B1(0), A1(0), B0(0) have landed, everyone's
  if (wr == 1) {                                // waves 4-7 run one section behind waves 0-3 (wr is wave-uniform)
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  }
  for (int t = 0; t < c.nt; t += 2) {
    k_step<0, MIH>(c, t, acc);
    if (t + 1 < c.nt) k_step<1, MIH>(c, t + 1, acc);
  }
  if (wr == 0) {                                // same number of barriers for every wave
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the out-of-range tail refills have landed (zeros): LDS is reusable
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);

  float* slab = reinterpret_cast<float*>(smem) + wave * (32 * (64 + 4));
  epilogue_wave<WMT, 64, 2 * MIH, 4, 1, 3>(g, acc, slab, m0 + wr * WMT, n0 + wc * 64, lane, nullptr);
}

}  // namespace g256b

int gemm256_nt_tile_rows(int M, int N);   // gemm256.hip: 192-row tiles when a round of them fills CUs a round of 256-row tiles leaves idle

// Host entry for lr2_gemm_bf16.  Requirements (checked by the caller): single planes, NT, K % 64 == 0, operand extents
// < 4 GiB - 512 B, an inference epilogue (at most the residual as a per-element request).
int launch_gemm256_b1(const GemmParams& p_in, hipStream_t stream) {
  using namespace g256b;
  GemmParams p = p_in;
  const int bm = gemm256_nt_tile_rows(p.M, p.N);
  p.tiles_m = (p.M + bm - 1) / bm;
  p.tiles_n = (p.N + BN - 1) / BN;
  static bool attr_set = false;
  if (!attr_set) {
    if (lr2_allow_dynamic_lds(gemm256_b1_kernel<4>, LDS_BYTES, "gemm256_b1")) return LR2_ERR_LAUNCH;
    if (lr2_allow_dynamic_lds(gemm256_b1_kernel<3>, LDS_BYTES, "gemm256_b1(192 rows)")) return LR2_ERR_LAUNCH;
    attr_set = true;
  }
  if (bm == 192) LR2_LAUNCH(gemm256_b1_kernel<3>, dim3(p.tiles_m * p.tiles_n), dim3(512), LDS_BYTES, stream, p);
  else LR2_LAUNCH(gemm256_b1_kernel<4>, dim3(p.tiles_m * p.tiles_n), dim3(512), LDS_BYTES, stream, p);
  return lr2_launch_status(__func__);
}

}  // namespace lr2gemm
