// 256 x 256 "ping-pong" weight gradient of SINGLE bf16 planes:  C[M,N] = A^T . B  with A [K][lda] (M contiguous) and B [K][ldb]
// (N contiguous), ONE bf16 plane per operand, one v_mfma_f32_16x16x32_bf16 product per tile pair, fp32 accumulate -- dW = dY^T X of an
// nn.Linear in the "bf16_train" mode (FeatureExtractor(precision="bf16_train")).  NOT the parity path: an operand keeps 8
// mantissa bits (gemm256.hip's three-product gemm256_tn_kernel stays the default everywhere).
//
// Replaces, in that mode, autograd of nn.Linear's weight and bias in tencentpretrain/layers/position_ffn.py:12-15 and
// multi_headed_attn.py:55-76 (cuBLAS with a transposed operand upstream) -- the same sites as gemm256_tn_kernel.
//
// Structure: gemm256.hip::g256t::gemm256_tn_kernel (LDS image [32 k-rows][16 units of 8 consecutive m], ds_read_b64_tr_b16 fragment
// reads, 2-stage ring, counted vmcnt waits, two wave groups one section apart, XCD-chunked tile x split grid in one round of the chip,
// raw fp32 slabs + the fixed-order split-K reducer of gemm.hip) with the operand trick of gemm256_b1.hip:
//   * a K step is 64 token rows deep.  The slot that holds the lo plane in the 3-pass kernel holds k-rows 32 .. 63 of the SAME plane:
//     the two DMA pieces of a wave read the same columns 32 rows apart.
//   * an MFMA section is 16 products (two k-halves x 8 tiles): a step is 64 MFMAs per wave for 64 KiB staged.
//   * ragged K: a_bytes / b_bytes are the exact plane extents, so rows >= K -- a whole second k-half included -- are out-of-range
//     requests and read zeros.  A lane whose columns lie outside the operand stays out of range at every K step (base != OOB, the
//     rule of gemm256_ring.h).
//   * the bias gradient of the same layer comes out of this launch: db[m] = sum_k bf16(dY)[k, m], the column sums of the A fragments
//     AS THE PRODUCT SEES THEM (the one plane, not the fp32 gradient it was rounded from), each K step summed once, by the workgroup
//     with tn == step % tiles_n.
// The small image helpers below repeat g256t's (that kernel's file is left untouched: its instruction stream is a yardstick).
#include "gemm256_ring.h"

namespace lr2gemm {
namespace g256tb {

using ring256::OOB;
constexpr int BM = 256, BN = 256, BK = 64;
constexpr int PLANE = 32 * 256;        // one k-half of one part: 32 k-rows x 128 m x 2 B = 8 KiB
constexpr int STAGE_STRIDE = 2 * PLANE;   // both k-halves of one stage of one part
constexpr int HALF_STRIDE = 2 * STAGE_STRIDE;
constexpr int REGION = 2 * HALF_STRIDE;   // A region, then B region: 64 KiB each
constexpr int LDS_BYTES = 2 * REGION;

__device__ __forceinline__ int swz_tr16(int k) { return ((((k & 3) | (((k >> 3) & 1) << 2))) << 1) & 15; }

template <int IMM>
__device__ __forceinline__ bf16x8_t lds_read_tr(uint32_t addr) {
  u32x2_t lo, hi;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(lo) : "v"(addr), "i"(IMM));
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(hi) : "v"(addr), "i"(IMM + 4 * 256));
  u32x4_t v = {lo[0], lo[1], hi[0], hi[1]};
  return __builtin_bit_cast(bf16x8_t, v);
}

struct Ctx {
  __amdgpu_buffer_rsrc_t a, b;
  uint32_t voff_a[2], voff_b[2];   // per-lane source byte offsets of this wave's piece of part A(h) / B(h) at this split's K step 0
  uint32_t kstep_a, kstep_b;       // bytes per 64-row K step (the second k-half lies half a step further)
  uint32_t rd_a[4], rd_b[2];       // per-lane LDS read bases of the wave's A tiles i = 0..3 / B tiles j = 0..1 (stage 0, half 0, k-half 0)
  char* smem;
  int wave, nt;
};

template <bool IS_A, int HALF>
__device__ __forceinline__ void issue_part(const Ctx& c, int tile, int stage) {
  const uint32_t base = IS_A ? c.voff_a[HALF] : c.voff_b[HALF];
  const uint32_t step = IS_A ? c.kstep_a : c.kstep_b;
  const uint64_t o0 = (uint64_t)base + (uint64_t)(uint32_t)tile * (uint64_t)step;
  const uint64_t o1 = o0 + (uint64_t)(step >> 1);
  const bool in = tile < c.nt && base != OOB;      // an out-of-range lane stays so at every K step
  const uint32_t v0 = (in && o0 < (uint64_t)OOB) ? (uint32_t)o0 : OOB;
  const uint32_t v1 = (in && o1 < (uint64_t)OOB) ? (uint32_t)o1 : OOB;
  char* dst = c.smem + (IS_A ? 0 : REGION) + HALF * HALF_STRIDE + stage * STAGE_STRIDE + c.wave * 1024;
  __builtin_amdgcn_raw_ptr_buffer_load_lds(IS_A ? c.a : c.b, LDS_PTR(dst), 16, v0, 0, 0, 0);
  __builtin_amdgcn_raw_ptr_buffer_load_lds(IS_A ? c.a : c.b, LDS_PTR(dst + PLANE), 16, v1, 0, 0, 0);
}

template <int HALF, int S>
__device__ __forceinline__ void read_a_half(const Ctx& c, bf16x8_t (&k0)[4], bf16x8_t (&k1)[4]) {
  constexpr int O = HALF * HALF_STRIDE + S * STAGE_STRIDE;
  k0[0] = lds_read_tr<O>(c.rd_a[0]);
  k0[1] = lds_read_tr<O>(c.rd_a[1]);
  k0[2] = lds_read_tr<O>(c.rd_a[2]);
  k0[3] = lds_read_tr<O>(c.rd_a[3]);
  k1[0] = lds_read_tr<O + PLANE>(c.rd_a[0]);
  k1[1] = lds_read_tr<O + PLANE>(c.rd_a[1]);
  k1[2] = lds_read_tr<O + PLANE>(c.rd_a[2]);
  k1[3] = lds_read_tr<O + PLANE>(c.rd_a[3]);
}
template <int HALF, int S>
__device__ __forceinline__ void read_b_half(const Ctx& c, bf16x8_t (&k0)[2], bf16x8_t (&k1)[2]) {
  constexpr int O = HALF * HALF_STRIDE + S * STAGE_STRIDE;
  k0[0] = lds_read_tr<O>(c.rd_b[0]);
  k0[1] = lds_read_tr<O>(c.rd_b[1]);
  k1[0] = lds_read_tr<O + PLANE>(c.rd_b[0]);
  k1[1] = lds_read_tr<O + PLANE>(c.rd_b[1]);
}

// 16 MFMAs of one accumulator quadrant: k-half 0 of the 8 tiles, then k-half 1 (gemm256_b1.hip's section).
template <int AH, int BH>
__device__ __forceinline__ void mfma_section(f32x4_t (&acc)[8][4], const bf16x8_t (&a0)[4], const bf16x8_t (&a1)[4],
                                             const bf16x8_t (&b0)[2], const bf16x8_t (&b1)[2]) {
  __builtin_amdgcn_s_setprio(1);
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      acc[AH * 4 + i][BH * 2 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0[i], b0[j], acc[AH * 4 + i][BH * 2 + j], 0, 0, 0);
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      acc[AH * 4 + i][BH * 2 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1[i], b1[j], acc[AH * 4 + i][BH * 2 + j], 0, 0, 0);
  __builtin_amdgcn_s_setprio(0);
  ring256::section_barrier();
}

// Column sums of A from the fragments a wave holds anyway: lane l of a fragment carries A[k = 8 * (l >> 4) + j][m = tile row (l & 15)],
// j = 0..7, as packed bf16 pairs, added in fp32.
__device__ __forceinline__ float frag_sum(const bf16x8_t& f) {
  const u32x4_t w = __builtin_bit_cast(u32x4_t, f);
  float s = 0.f;
#pragma unroll
  for (int d = 0; d < 4; ++d) s += __uint_as_float(w[d] << 16) + __uint_as_float(w[d] & 0xffff0000u);
  return s;
}
// The four waves of one wr hold the same A fragments: wave wc sums tile wc of each half, both k-halves.
template <int AH>
__device__ __forceinline__ void colsum_frags(float (&cs)[2], int wc, const bf16x8_t (&a0)[4], const bf16x8_t (&a1)[4]) {
  if (wc == 0) cs[AH] += frag_sum(a0[0]) + frag_sum(a1[0]);
  else if (wc == 1) cs[AH] += frag_sum(a0[1]) + frag_sum(a1[1]);
  else if (wc == 2) cs[AH] += frag_sum(a0[2]) + frag_sum(a1[2]);
  else cs[AH] += frag_sum(a0[3]) + frag_sum(a1[3]);
}

// One K step: the section / refill / counted-wait schedule of ring256::k_step_bf16.
template <int S>
__device__ __forceinline__ void k_step(const Ctx& c, int t, f32x4_t (&acc)[8][4], float (&cs)[2], int wc, bool do_cs) {
  using ring256::end_load_section;
  bf16x8_t a0[4], a1[4], b0[2], b1[2];
  issue_part<false, 0>(c, t + 1, S ^ 1);          // phase 0: quadrant (A0, B0)
  read_a_half<0, S>(c, a0, a1);
  read_b_half<0, S>(c, b0, b1);
  end_load_section<12>();
  mfma_section<0, 0>(acc, a0, a1, b0, b1);
  issue_part<true, 0>(c, t + 2, S);               // phase 1: (A0, B1)
  read_b_half<1, S>(c, b0, b1);
  if (do_cs) colsum_frags<0>(cs, wc, a0, a1);
  end_load_section<12>();
  mfma_section<0, 1>(acc, a0, a1, b0, b1);
  issue_part<false, 1>(c, t + 2, S);              // phase 2: (A1, B1)
  read_a_half<1, S>(c, a0, a1);
  end_load_section<12>();
  mfma_section<1, 1>(acc, a0, a1, b0, b1);
  issue_part<true, 1>(c, t + 2, S);               // phase 3: (A1, B0)
  read_b_half<0, S>(c, b0, b1);
  if (do_cs) colsum_frags<1>(cs, wc, a0, a1);
  end_load_section<6>();
  mfma_section<1, 0>(acc, a0, a1, b0, b1);
}

__global__ __launch_bounds__(512, 2) void gemm256_tn_b1_kernel(GemmParams g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;

  // work units in split-major order, cut into 8 contiguous chunks (one per XCD): the tiles of one K range run on one XCD's L2
  const int tiles = g.tiles_m * g.tiles_n;
  const int unit = xcd_chunk_index(tiles * g.splits, blockIdx.x);
  const int split = unit / tiles, tile = unit - split * tiles;
  const int tm = tile / g.tiles_n, tn = tile - tm * g.tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;
  const int total_steps = (g.K + BK - 1) / BK;
  const int t0 = split * g.k_tiles_per_split;

  Ctx c;
  c.smem = smem;
  c.wave = wave;
  c.nt = min(g.k_tiles_per_split, total_steps - t0);
  c.a = uniform_rsrc(g.A, g.a_bytes);
  c.b = uniform_rsrc(g.B, g.b_bytes);
  c.kstep_a = (uint32_t)g.lda * 2u * BK;
  c.kstep_b = (uint32_t)g.ldb * 2u * BK;
  {
    // this wave's 1-KiB piece of a k-half = k-rows wave*4 .. +4 of it; lane l fills unit slot (l & 15) of k-row (l >> 4), which
    // holds source unit (l & 15) ^ swz_tr16(k-row) = 8 consecutive m (n) of the part
    const int kl = wave * 4 + (lane >> 4);
    const int pu = ((lane & 15) ^ swz_tr16(kl)) * 8;          // part-local index of the unit's first element
    const uint64_t krow = (uint64_t)t0 * BK + (uint64_t)kl;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int am = m0 + (pu >> 6) * 128 + h * 64 + (pu & 63);   // part A(h): rows wr*128 + h*64 + [0, 64) of both wr
      const int bn = n0 + (pu >> 5) * 64 + h * 32 + (pu & 31);    // part B(h): cols wc*64 + h*32 + [0, 32) of all wc
      const uint64_t oa = (krow * (uint64_t)g.lda + (uint64_t)am) * 2u;
      const uint64_t ob = (krow * (uint64_t)g.ldb + (uint64_t)bn) * 2u;
      // units past the row's end would read the next k-row's first columns: they only feed output rows / columns >= M / N, which
      // the epilogue and the column-sum store mask -- but a unit that STRADDLES lda cannot exist (lda % 8 == 0)
      c.voff_a[h] = (am < g.lda && oa < (uint64_t)OOB) ? (uint32_t)oa : OOB;
      c.voff_b[h] = (bn < g.ldb && ob < (uint64_t)OOB) ? (uint32_t)ob : OOB;
    }
    // fragment bases (TR form): lane (g4, q, p) reads 8 B at k-row 8*g4 + q, unit (rbase >> 3) + (p >> 1)
    const int i16 = lane & 15, q = i16 >> 2, pp = i16 & 3, g4 = lane >> 4;
    const int ka = 8 * g4 + q;
    const int sx = swz_tr16(ka);                               // == swz_tr16(ka + 4)
    const uint32_t sm = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
    const uint32_t rowb = (uint32_t)(ka * 256 + 8 * (pp & 1));
#pragma unroll
    for (int i = 0; i < 4; ++i) c.rd_a[i] = sm + rowb + (uint32_t)((((wr * 8 + 2 * i + (pp >> 1)) ^ sx)) * 16);
#pragma unroll
    for (int j = 0; j < 2; ++j) c.rd_b[j] = sm + REGION + rowb + (uint32_t)((((wc * 4 + 2 * j + (pp >> 1)) ^ sx)) * 16);
  }

  f32x4_t acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // prologue: everything of K steps 0 and 1 except B0(1), in the steady-state issue order
  issue_part<true, 0>(c, 0, 0);
  issue_part<false, 1>(c, 0, 0);
  issue_part<true, 1>(c, 0, 0);
  issue_part<false, 0>(c, 0, 0);
  issue_part<true, 0>(c, 1, 1);
  issue_part<false, 1>(c, 1, 1);
  issue_part<true, 1>(c, 1, 1);
  ring256::end_load_section<6>();
  if (wr == 1) {                                // waves 4-7 run one section behind waves 0-3
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  }
  // Column sums of A (g.epi.colsum_partial): global step tau is summed by the workgroup with tn == tau % tiles_n, wave (wr, wc)
  // taking m-tile wc of each half of its wr rows.  Every workgroup writes its [256] slice of partial row (split * tiles_n + tn).
  float cs[2] = {0.f, 0.f};
  const bool cs_on = g.epi.colsum_partial != nullptr;
  int cs_phase = (t0 + g.tiles_n - tn) % g.tiles_n;      // (global step - tn) mod tiles_n of local step 0
  for (int t = 0; t < c.nt; t += 2) {
    k_step<0>(c, t, acc, cs, wc, cs_on && cs_phase == 0);
    cs_phase = cs_phase + 1 == g.tiles_n ? 0 : cs_phase + 1;
    if (t + 1 < c.nt) k_step<1>(c, t + 1, acc, cs, wc, cs_on && cs_phase == 0);
    cs_phase = cs_phase + 1 == g.tiles_n ? 0 : cs_phase + 1;
  }
  ring256::drain(wr);

  if (cs_on) {
    float* dst = g.epi.colsum_partial + (size_t)(split * g.tiles_n + tn) * (size_t)g.M;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float v = cs[h];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      const int m = m0 + wr * 128 + h * 64 + wc * 16 + (lane & 15);
      if (lane < 16 && m < g.M) dst[m] = v;
    }
  }
  float* slab = reinterpret_cast<float*>(smem) + wave * (32 * (64 + 4));
  float* partial = g.partial ? g.partial + (size_t)split * (size_t)g.M * (size_t)g.N : nullptr;
  epilogue_wave<128, 64, 8, 4, 1>(g, acc, slab, m0 + wr * 128, n0 + wc * 64, lane, partial);
}

}  // namespace g256tb

// Host entry for lr2_gemm_bf16_train's (1,1) form: single planes, TN, a plain epilogue (alpha, fp32 store) or split-K slabs; the
// caller runs the split-K reducer and finishes the column sums.  p.k_tiles_per_split is in units of 64 rows.
int launch_gemm256_tn_b1(const GemmParams& p_in, int splits, hipStream_t stream) {
  using namespace g256tb;
  GemmParams p = p_in;
  p.tiles_m = (p.M + BM - 1) / BM;
  p.tiles_n = (p.N + BN - 1) / BN;
  p.splits = splits;
  static bool attr_set = false;
  if (!attr_set) {
    if (lr2_allow_dynamic_lds(gemm256_tn_b1_kernel, LDS_BYTES, "gemm256_tn_b1")) return LR2_ERR_LAUNCH;
    attr_set = true;
  }
  LR2_LAUNCH(gemm256_tn_b1_kernel, dim3(p.tiles_m * p.tiles_n * splits), dim3(512), LDS_BYTES, stream, p);
  return lr2_launch_status(__func__);
}

}  // namespace lr2gemm
