// The LDS ring of the 256 x 256 "ping-pong" NT products -- gemm256.hip (split-bf16), gemm256_b1.hip (single-pass bf16),
// gemm256_f16.hip (single-pass f16), gemm256_mx.hip (MX-FP8): geometry, lane set-up, DMA issue, fragment reads, the section waits, prologue and drain, once.  A kernel file keeps what
// its operand format differs in: the MFMA section, the epilogue, the launcher (and, for MX-FP8, the scales and its own K step).
//
// Structure (CDNA4, one workgroup of 8 waves per CU, 128 KiB of LDS):
//   * tile 256 x 256 (64 MIH x 256); wave (wr, wc) of a 2 x 4 grid owns a 128 x 64 block = 8 x 4 accumulator tiles (128
//     accumulator VGPRs).  A K step is 128 bytes of every operand row: 64 KiB staged for the whole workgroup.
//   * operands travel HBM/L2 -> LDS by LDS-DMA (buffer_load ... lds, 16 B per lane) into a ring of 2 stages x 4 parts
//     (A rows of accumulator half 0 / 1, B columns of half 0 / 1; a part is two adjacent 8-KiB planes).  A part is
//     refilled for K step t+2 as soon as its last reader of step t has passed, so 6-7 parts (12-14 KiB per wave) are in
//     flight at any time; waits are COUNTED (s_waitcnt vmcnt(12) / (6)), never vmcnt(0), and barriers are bare s_barrier
//     (a __syncthreads() would drain every in-flight DMA).  Past the last K step the refills become out-of-range
//     requests (the buffer descriptor's range check writes zeros) so the counts stay uniform.
//   * a K step is four phases, one accumulator quadrant each (A half x B half): phase = LOAD section (issue 2 DMA pieces,
//     ds_read_b128 the fragments this phase is missing: 12 / 4 / 8 / 4 reads) + MFMA section.  The two wave groups
//     (waves 0-3 and 4-7 = one wave per SIMD each) run ONE SECTION APART: while a group issues its MFMAs its SIMD
//     partner loads, so every SIMD's matrix pipe always has exactly one wave feeding it and the LDS / DMA work of the
//     other hides underneath.  Two s_barrier per phase keep the groups in that lock step.
//   * LDS image of a plane: [128 rows][4 units of 16 B], unit u of row r at u ^ swz(r) (four 64-B rows share a 256-B
//     bank row: conflict-free ds_read_b128); LDS-DMA writes lane-linearly, so the swizzle is applied to the SOURCE address.
//   * hazards: a fragment read happens at least one barrier after every wave's counted wait for that part (RAW); a part is
//     refilled one barrier after both groups' reads of it were retired by lgkmcnt(0) (WAR).
#pragma once
#include "gemm_common.h"

namespace lr2gemm {
namespace ring256 {

constexpr int PLANE = 128 * 64;       // one plane of one part: 128 rows x 64 B = 8 KiB
constexpr int PART = 2 * PLANE;
constexpr int STAGE = 4 * PART;       // parts A0, B0, B1, A1
constexpr int RING = 2 * STAGE;       // 128 KiB
constexpr int SLOT_A0 = 0, SLOT_B0 = 1, SLOT_B1 = 2, SLOT_A1 = 3;
constexpr uint32_t OOB = 0xFFFFFF00u;  // voffset beyond any descriptor this library builds (operands are < 4 GiB - 512 B)

__device__ __forceinline__ int swz(int r) { return (4 - ((r >> 2) & 3)) & 3; }

template <int IMM>
__device__ __forceinline__ u32x4_t lds_read16(uint32_t addr) {
  u32x4_t v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(IMM));
  return v;
}

// Closes a section: the two wave groups meet; nothing moves across.
__device__ __forceinline__ void section_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

// End of a LOAD section: retire the DMA parts the NEXT load section reads (counted), retire this section's fragment
// reads, meet the other group.  s_waitcnt immediates (gfx9 encoding): vmcnt[3:0] in bits 3:0, vmcnt[5:4] in bits 15:14,
// expcnt 7 (no wait) in bits 6:4, lgkmcnt in bits 11:8.
template <int VM>
__device__ __forceinline__ void end_load_section() {
  constexpr int imm = (VM & 15) | ((VM >> 4) << 14) | (7 << 4) | (0 << 8);
  __builtin_amdgcn_s_waitcnt(imm);
  section_barrier();
}

// Where the two DMA pieces of a part come from.  TwoPlanes: the same offset of a second descriptor (the hi and lo plane of
// split-bf16, 64 B of each per K step).  OnePlane: 64 B further along the same descriptor (128 B of a bf16 or fp8 row).
struct TwoPlanes {
  __amdgpu_buffer_rsrc_t a, a2, b, b2;
  static constexpr int STEP = 64, SECOND = 0;
  template <bool IS_A> __device__ __forceinline__ __amdgpu_buffer_rsrc_t second() const { return IS_A ? a2 : b2; }
};
struct OnePlane {
  __amdgpu_buffer_rsrc_t a, b;
  static constexpr int STEP = 128, SECOND = 64;
  template <bool IS_A> __device__ __forceinline__ __amdgpu_buffer_rsrc_t second() const { return IS_A ? a : b; }
};

template <class SRC>
struct Ctx {
  using Src = SRC;
  SRC src;
  uint32_t voff_a[2], voff_b[2];   // per-lane source byte offsets of this wave's piece of part A(h) / B(h) at K step 0
  uint32_t rd_a[2], rd_b[2];       // per-lane LDS read bases for stage 0 / 1
  char* smem;
  int wave, nt;                    // nt: K steps (set by the kernel)
};

// Lane set-up for tile origin (m0, n0): the DMA source offsets and the fragment read bases.  MIH = accumulator tiles per half
// of a wave's rows: 4 -> 256 tile rows; 3 -> 192 (wave tile 96 x 64): an A part then holds 96 rows, the two waves whose 16-row
// pieces fall beyond them issue out-of-range requests (zeros into the unused quarter of the part), so every wave's counted
// waits stay as they are.  Rows >= M and columns >= N are out-of-range requests too.
template <int MIH, class CTX>
__device__ __forceinline__ void lane_setup(CTX& c, char* smem, int m0, int n0, int wave, int lane, uint64_t pitch_a,
                                           uint64_t pitch_b, int M, int N) {
  constexpr int WMT = 32 * MIH;      // wave-tile rows
  const int wr = wave >> 2, wc = wave & 3;
  c.smem = smem;
  c.wave = wave;
  // this wave's 1-KiB piece of a plane = local rows wave*16 .. +16; lane l fills unit (l & 3) of row (l >> 2), which holds
  // the row's 16-byte chunk (l & 3) ^ swz(row) of that plane's 64 bytes
  const int lr = wave * 16 + (lane >> 2);
  const uint32_t ku = (uint32_t)((lane & 3) ^ swz(lr)) * 16u;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    // part A(h): rows wr*WMT + h*(WMT/2) + [0, WMT/2) of both wr (part-local row lr = wr*(WMT/2) + that index)
    const int awr = lr / (WMT / 2), ain = lr - awr * (WMT / 2);
    const int arow = m0 + awr * WMT + h * (WMT / 2) + ain;
    const int bcol = n0 + (lr >> 5) * 64 + h * 32 + (lr & 31);    // part B(h): cols wc*64 + h*32 + [0, 32) of all wc
    const uint64_t oa = (uint64_t)arow * pitch_a + ku;
    const uint64_t ob = (uint64_t)bcol * pitch_b + ku;
    c.voff_a[h] = (lr < WMT && arow < M && oa < (uint64_t)OOB) ? (uint32_t)oa : OOB;
    c.voff_b[h] = (bcol < N && ob < (uint64_t)OOB) ? (uint32_t)ob : OOB;
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

// One LDS-DMA: 16 B per lane from descriptor offset v (out of range: zeros) to dst + 16 * lane.  (Not inside the templates below:
// the host pass cannot name the builtin in a function template it deduces arguments for.)
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t src, char* dst, uint32_t v) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(src, LDS_PTR(dst), 16, v, 0, 0, 0);
}

// Two DMA pieces (one per plane, 16 rows each) of one part for K step `tile` into stage `stage`.
template <int SLOT, bool IS_A, int HALF, class CTX>
__device__ __forceinline__ void issue_part(const CTX& c, int tile, int stage) {
  using SRC = typename CTX::Src;
  const uint32_t base = IS_A ? c.voff_a[HALF] : c.voff_b[HALF];
  const bool in = tile < c.nt && base != OOB;    // an out-of-range lane stays so at every K step (OOB + tile * STEP would wrap)
  const uint32_t v0 = in ? base + (uint32_t)tile * SRC::STEP : OOB;
  const uint32_t v1 = in ? v0 + SRC::SECOND : OOB;
  char* dst = c.smem + stage * STAGE + SLOT * PART + c.wave * 1024;
  dma16(IS_A ? c.src.a : c.src.b, dst, v0);
  dma16(c.src.template second<IS_A>(), dst + PLANE, v1);
}

// The raw fragment reads of an A half (MIH tiles) / a B half (2 tiles): plane 0 of every tile, then plane 1.  V = u32x4_t, or a
// 16-byte vector the bits are cast to.
template <int SLOT, int MIH, class V>
__device__ __forceinline__ void read_a_half(uint32_t base, V (&p0)[MIH], V (&p1)[MIH]) {
  p0[0] = __builtin_bit_cast(V, lds_read16<SLOT * PART + 0 * 1024>(base));
  p0[1] = __builtin_bit_cast(V, lds_read16<SLOT * PART + 1 * 1024>(base));
  p0[2] = __builtin_bit_cast(V, lds_read16<SLOT * PART + 2 * 1024>(base));
  if constexpr (MIH == 4) p0[3] = __builtin_bit_cast(V, lds_read16<SLOT * PART + 3 * 1024>(base));
  p1[0] = __builtin_bit_cast(V, lds_read16<SLOT * PART + PLANE + 0 * 1024>(base));
  p1[1] = __builtin_bit_cast(V, lds_read16<SLOT * PART + PLANE + 1 * 1024>(base));
  p1[2] = __builtin_bit_cast(V, lds_read16<SLOT * PART + PLANE + 2 * 1024>(base));
  if constexpr (MIH == 4) p1[3] = __builtin_bit_cast(V, lds_read16<SLOT * PART + PLANE + 3 * 1024>(base));
}
template <int SLOT, class V>
__device__ __forceinline__ void read_b_half(uint32_t base, V (&p0)[2], V (&p1)[2]) {
  p0[0] = __builtin_bit_cast(V, lds_read16<SLOT * PART + 0 * 1024>(base));
  p0[1] = __builtin_bit_cast(V, lds_read16<SLOT * PART + 1 * 1024>(base));
  p1[0] = __builtin_bit_cast(V, lds_read16<SLOT * PART + PLANE + 0 * 1024>(base));
  p1[1] = __builtin_bit_cast(V, lds_read16<SLOT * PART + PLANE + 1 * 1024>(base));
}

// One K step of the bf16 kernels (tile t, compile-time stage S).  A part may be refilled once its last reader has passed (A0
// after load section 0, B1 after 1, A1 after 2, B0 after 3); the refills go as early as possible, 2 pieces per section:
//   0: B0(t+1) [other stage]  1: A0(t+2)  2: B1(t+2)  3: A1(t+2)
// The counted waits leave exactly the parts issued after the one the NEXT section reads in flight (2 pieces per part).
// PRODUCTS::mfma_section<AH, BH, MIH> is the kernel's list of MFMAs for one quadrant; it ends with section_barrier().
template <class PRODUCTS, int S, int MIH, class CTX>
__device__ __forceinline__ void k_step_bf16(const CTX& c, int t, f32x4_t (&acc)[2 * MIH][4]) {
  bf16x8_t a0[MIH], a1[MIH], b0[2], b1[2];
  // phase 0: quadrant (A0, B0)
  issue_part<SLOT_B0, false, 0>(c, t + 1, S ^ 1);
  read_a_half<SLOT_A0, MIH>(c.rd_a[S], a0, a1);
  read_b_half<SLOT_B0>(c.rd_b[S], b0, b1);
  end_load_section<12>();
  PRODUCTS::template mfma_section<0, 0, MIH>(acc, a0, a1, b0, b1);
  // phase 1: (A0, B1)
  issue_part<SLOT_A0, true, 0>(c, t + 2, S);
  read_b_half<SLOT_B1>(c.rd_b[S], b0, b1);
  end_load_section<12>();
  PRODUCTS::template mfma_section<0, 1, MIH>(acc, a0, a1, b0, b1);
  // phase 2: (A1, B1)
  issue_part<SLOT_B1, false, 1>(c, t + 2, S);
  read_a_half<SLOT_A1, MIH>(c.rd_a[S], a0, a1);
  end_load_section<12>();
  PRODUCTS::template mfma_section<1, 1, MIH>(acc, a0, a1, b0, b1);
  // phase 3: (A1, B0)
  issue_part<SLOT_A1, true, 1>(c, t + 2, S);
  read_b_half<SLOT_B0>(c.rd_b[S], b0, b1);
  end_load_section<6>();
  PRODUCTS::template mfma_section<1, 0, MIH>(acc, a0, a1, b0, b1);
}

// What a kernel adds to the prologue: nothing, for the bf16 kernels.  MX-FP8 issues its scale DMAs here (gemm256_mx.hip), in
// their steady-state place after A1, and counts them in the first wait.
struct NoExtras {
  static constexpr int FIRST_WAIT = 6;     // the parts of K step 1: 3 parts x 2 pieces stay in flight
  template <class CTX> static __device__ __forceinline__ void begin(const CTX&) {}
  template <class CTX> static __device__ __forceinline__ void after_a1(const CTX&, int) {}
};

// Around the K loop.  The loop itself -- for (t = 0; t < nt; t += 2) { k_step<0>(t); if (t + 1 < nt) k_step<1>(t + 1); } -- stays in
// each kernel: inlined from here the compiler rotates it differently (other scalar instructions in the MFMA block), and a shared
// loop would need a functor around every kernel's k_step<S>.
//
// The prologue: everything of K steps 0 and 1 except B0(1), in the steady-state issue order; then waves 4-7 fall one section
// behind waves 0-3 (wr is wave-uniform).
template <class EXTRAS, class CTX>
__device__ __forceinline__ void prologue(const CTX& c, int wr) {
  EXTRAS::begin(c);
  issue_part<SLOT_A0, true, 0>(c, 0, 0);
  issue_part<SLOT_B1, false, 1>(c, 0, 0);
  issue_part<SLOT_A1, true, 1>(c, 0, 0);
  EXTRAS::after_a1(c, 0);
  issue_part<SLOT_B0, false, 0>(c, 0, 0);
  issue_part<SLOT_A0, true, 0>(c, 1, 1);
  issue_part<SLOT_B1, false, 1>(c, 1, 1);
  issue_part<SLOT_A1, true, 1>(c, 1, 1);
  EXTRAS::after_a1(c, 1);
  end_load_section<EXTRAS::FIRST_WAIT>();       // A0(0), B1(0), A1(0), B0(0) have landed, everyone's
  if (wr == 1) {
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  }
}

// After the last K step: the same number of barriers for every wave, and the out-of-range tail refills have landed (zeros), so
// the LDS is reusable.
__device__ __forceinline__ void drain(int wr) {
  if (wr == 0) {
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

}  // namespace ring256
}  // namespace lr2gemm
