// 256 x 256 "ping-pong" product of MX-FP8 operands:  C[M,N] = A_q[M,K] . B_q[N,K]^T  (e4m3fn bytes, one E8M0 scale per 32 elements of a
// row, fp32 accumulate) on gfx950's block-scaled matrix instruction v_mfma_scale_f32_16x16x128_f8f6f4 -- the "fp8 MFMA" mode of
// BASELINE.json configs[4] (ViT-L/14 swap; FeatureExtractor(precision="mxfp8")).  NOT the parity path (3 mantissa bits per element).
//
// Replaces, in that mode, the cuBLAS sgemm calls reached through nn.Linear in the encoders (tencentpretrain/layers/
// multi_headed_attn.py:55-76, position_ffn.py:12-15); same contract as lr2_gemm_mxfp8's 128 x 128 kernel (fp8.hip).
//
// Structure: the ring of gemm256_ring.h (tile 256 x 256) with one-byte operands.  What is this kernel's own:
//   * a K step is 128 elements = 128 bytes per row: plane 0 of a part = K bytes [0, 64) of every row, plane 1 = K bytes [64, 128).
//     The instruction's operand for lane (row l & 15, q = l >> 4) is bytes 16 q .. 16 q + 15 and 64 + 16 q .. (measured layout,
//     fp8.hip): unit q of plane 0 and unit q of plane 1 -- the ring's two conflict-free ds_read_b128 per fragment.  A K step is 32
//     instructions per wave (1024 matrix cycles) for 64 KiB of operands.
//   * the scales travel with the operands: per K step one 4-byte LDS-DMA per lane (waves 0-3: the tile's 256 A rows, waves 4-7: its
//     256 B rows) into a 2-stage [512 rows][4 B] region; a lane's scale (row l & 15, block q) is ONE ds_read_u8.
//   * schedule per K step t (stage t & 1), refills as early as the last reader allows:
//       phase 0 (A0 x B0): issue B0(t+1)            read A0, B0 fragments + their scales     wait vmcnt(14)
//       phase 1 (A0 x B1): issue A0(t+2)            read B1 + scales                         wait vmcnt(14)
//       phase 2 (A1 x B1): issue B1(t+2)            read A1 + scales                         wait vmcnt(13)
//       phase 3 (A1 x B0): issue A1(t+2), S(t+2)    read B0                                  wait vmcnt(7)
//     (2 DMA instructions per part, 1 per scale step; each count = the DMAs issued after the youngest part the NEXT section reads).
//   * epilogue through a wave-private LDS slab, 32 rows at a time: bias, GELU, residual; results as fp32, as bf16 hi / lo planes
//     (what the attention kernels read) and / or re-quantised to MX-FP8 (the next product's A operand).

#include "fp8_common.h"
#include "gemm256_ring.h"

namespace lr2mx256 {

using lr2gemm::lds_addr;
using lr2gemm::tile_coords;
using lr2gemm::uniform_rsrc;
using namespace lr2gemm::ring256;

typedef int v8i_t __attribute__((ext_vector_type(8)));

constexpr int BM = 256, BN = 256, BKB = 128;   // K step in elements = bytes
constexpr int SC_STAGE = 2048;                 // A scales [256 rows][4 B], then B scales [256][4 B]
constexpr int LDS_BYTES = RING + 2 * SC_STAGE;
constexpr int SC16_STAGE = 8192;               // SC16: A scales [256 rows][16 B] (4 K steps each), then B scales [256][16 B]
constexpr int LDS_BYTES16 = RING + 2 * SC16_STAGE;
template <int IMM>
__device__ __forceinline__ int lds_read_u8(uint32_t addr) {
  int v;
  asm volatile("ds_read_u8 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(IMM));
  return v;
}

struct Ctx : lr2gemm::ring256::Ctx<OnePlane> {   // the ring's lane state + the scales'
  __amdgpu_buffer_rsrc_t sc;         // this wave's scale source (A scales for waves 0-3, B scales for waves 4-7)
  uint32_t voff_s;                   // per-lane source byte offset of this lane's scale row at K step 0
  uint32_t rd_sa, rd_sb;             // per-lane LDS read bases (scales), stage 0 (SC16: + the step's offset, see k_step)
  int ks;                            // scale bytes per row (K / 32)
};

// The 4 scale bytes of K step `tile` for this wave's 64 rows (one dword per lane).
__device__ __forceinline__ void issue_scales(const Ctx& c, int tile, int stage) {
  const uint32_t v = (tile < c.nt && c.voff_s != OOB) ? c.voff_s + (uint32_t)tile * 4u : OOB;
  char* dst = c.smem + RING + stage * SC_STAGE + c.wave * 256;
  __builtin_amdgcn_raw_ptr_buffer_load_lds(c.sc, LDS_PTR(dst), 4, v, 0, 0, 0);
}

// an operand = the lane's 16 bytes of plane 0, then of plane 1
__device__ __forceinline__ v8i_t operand(const u32x4_t& l, const u32x4_t& h) {
  return v8i_t{(int)l[0], (int)l[1], (int)l[2], (int)l[3], (int)h[0], (int)h[1], (int)h[2], (int)h[3]};
}
template <int SLOT>
__device__ __forceinline__ void read_a_half(uint32_t base, v8i_t (&a)[4]) {
  u32x4_t l[4], h[4];
  lr2gemm::ring256::read_a_half<SLOT, 4>(base, l, h);
#pragma unroll
  for (int i = 0; i < 4; ++i) a[i] = operand(l[i], h[i]);
}
template <int SLOT>
__device__ __forceinline__ void read_b_half(uint32_t base, v8i_t (&b)[2]) {
  u32x4_t l[2], h[2];
  lr2gemm::ring256::read_b_half<SLOT>(base, l, h);
#pragma unroll
  for (int j = 0; j < 2; ++j) b[j] = operand(l[j], h[j]);
}
// scales of accumulator half AH / BH for stage S: A rows wr*128 + AH*64 + 16 i + r16, B rows wc*64 + BH*32 + 16 j + r16
// SC16 form: the scale bytes of FOUR K steps per row and DMA (16 B per lane): a 4-byte gather per lane and step touched one cache
// line per row and step -- as many L2 -> L1 bytes as the operands themselves, 0.56 of 2.21 us per K step (profiles/experiments/README.md F.3)
__device__ __forceinline__ void issue_scales16(const Ctx& c, int quad, int stage) {
  const uint32_t off = (uint32_t)quad * 16u;
  const uint32_t v = (off < (uint32_t)c.ks && c.voff_s != OOB) ? c.voff_s + off : OOB;
  char* dst = c.smem + RING + stage * SC16_STAGE + c.wave * 1024;
  __builtin_amdgcn_raw_ptr_buffer_load_lds(c.sc, LDS_PTR(dst), 16, v, 0, 0, 0);
}
template <int AH>
__device__ __forceinline__ void read_sa16(uint32_t base, int (&sa)[4]) {
  sa[0] = lds_read_u8<(AH * 64 + 0) * 16>(base);
  sa[1] = lds_read_u8<(AH * 64 + 16) * 16>(base);
  sa[2] = lds_read_u8<(AH * 64 + 32) * 16>(base);
  sa[3] = lds_read_u8<(AH * 64 + 48) * 16>(base);
}
template <int BH>
__device__ __forceinline__ void read_sb16(uint32_t base, int (&sb)[2]) {
  sb[0] = lds_read_u8<(BH * 32 + 0) * 16>(base);
  sb[1] = lds_read_u8<(BH * 32 + 16) * 16>(base);
}
template <int S, int AH>
__device__ __forceinline__ void read_sa(uint32_t base, int (&sa)[4]) {
  sa[0] = lds_read_u8<S * SC_STAGE + (AH * 64 + 0) * 4>(base);
  sa[1] = lds_read_u8<S * SC_STAGE + (AH * 64 + 16) * 4>(base);
  sa[2] = lds_read_u8<S * SC_STAGE + (AH * 64 + 32) * 4>(base);
  sa[3] = lds_read_u8<S * SC_STAGE + (AH * 64 + 48) * 4>(base);
}
template <int S, int BH>
__device__ __forceinline__ void read_sb(uint32_t base, int (&sb)[2]) {
  sb[0] = lds_read_u8<S * SC_STAGE + (BH * 32 + 0) * 4>(base);
  sb[1] = lds_read_u8<S * SC_STAGE + (BH * 32 + 16) * 4>(base);
}

// 8 instructions of one accumulator quadrant (K = 128 each)
template <int AH, int BH>
__device__ __forceinline__ void mfma_section(f32x4_t (&acc)[8][4], const v8i_t (&a)[4], const v8i_t (&b)[2], const int (&sa)[4],
                                             const int (&sb)[2]) {
  __builtin_amdgcn_s_setprio(1);
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      acc[AH * 4 + i][BH * 2 + j] =
          __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[i], b[j], acc[AH * 4 + i][BH * 2 + j], 0, 0, 0, sa[i], 0, sb[j]);
  __builtin_amdgcn_s_setprio(0);
  section_barrier();
}

// The ring's K step (gemm256_ring.h::k_step_bf16: same refill order) with the scales: their reads, sb0 / sb1 live across phases,
// and waits that count the scale DMA of the 4-byte form.
template <int S, bool SC16>
__device__ __forceinline__ void k_step(const Ctx& c, int t, f32x4_t (&acc)[8][4]) {
  v8i_t a[4], b[2];
  int sa[4], sb0[2], sb1[2];
  // SC16: the step's scales sit in stage (t >> 2) & 1 at byte 4 (t & 3) of the lane's row
  const uint32_t soff = SC16 ? (uint32_t)(((t >> 2) & 1) * SC16_STAGE + (t & 3) * 4) : 0u;
  const uint32_t rsa = c.rd_sa + soff, rsb = c.rd_sb + soff;
  // the waits: SC16 issues a scale DMA in one step of four only, so the counts are those of the operand parts alone (an extra DMA in
  // flight makes a counted wait stricter, never laxer); the 4-byte form issues one per step and counts it
  constexpr int W0 = SC16 ? 12 : 14, W2 = SC16 ? 12 : 13, W3 = SC16 ? 6 : 7;
  // phase 0: quadrant (A0, B0)
  issue_part<SLOT_B0, false, 0>(c, t + 1, S ^ 1);
  read_a_half<SLOT_A0>(c.rd_a[S], a);
  read_b_half<SLOT_B0>(c.rd_b[S], b);
  if constexpr (SC16) {
    read_sa16<0>(rsa, sa);
    read_sb16<0>(rsb, sb0);
  } else {
    read_sa<S, 0>(c.rd_sa, sa);
    read_sb<S, 0>(c.rd_sb, sb0);
  }
  end_load_section<W0>();
  mfma_section<0, 0>(acc, a, b, sa, sb0);
  // phase 1: (A0, B1)
  issue_part<SLOT_A0, true, 0>(c, t + 2, S);
  read_b_half<SLOT_B1>(c.rd_b[S], b);
  if constexpr (SC16) read_sb16<1>(rsb, sb1);
  else read_sb<S, 1>(c.rd_sb, sb1);
  end_load_section<W0>();
  mfma_section<0, 1>(acc, a, b, sa, sb1);
  // phase 2: (A1, B1)
  issue_part<SLOT_B1, false, 1>(c, t + 2, S);
  read_a_half<SLOT_A1>(c.rd_a[S], a);
  if constexpr (SC16) read_sa16<1>(rsa, sa);
  else read_sa<S, 1>(c.rd_sa, sa);
  end_load_section<W2>();
  mfma_section<1, 1>(acc, a, b, sa, sb1);
  // phase 3: (A1, B0); every scale read of step t was retired one barrier ago by both groups.  4-byte form: the step's slot takes
  // step t + 2.  SC16: at the first step of a quad the OTHER stage (last read in step t - 1) takes the next quad.
  issue_part<SLOT_A1, true, 1>(c, t + 2, S);
  if constexpr (SC16) {
    if ((t & 3) == 0) issue_scales16(c, (t >> 2) + 1, ((t >> 2) + 1) & 1);
  } else {
    issue_scales(c, t + 2, S);
  }
  read_b_half<SLOT_B0>(c.rd_b[S], b);
  end_load_section<W3>();
  mfma_section<1, 0>(acc, a, b, sa, sb0);
}

// The prologue's scale DMAs, in their steady-state place (... A1, S, B0, A0, B1, A1, S ...).  4-byte form: one per K step, counted
// by the first wait.  SC16: the first quad of scales first (the oldest request: every later counted wait covers it).
template <bool SC16>
struct ScaleExtras {
  static constexpr int FIRST_WAIT = SC16 ? 6 : 7;
  static __device__ __forceinline__ void begin(const Ctx& c) {
    if constexpr (SC16) issue_scales16(c, 0, 0);
  }
  static __device__ __forceinline__ void after_a1(const Ctx& c, int t) {
    if constexpr (!SC16) issue_scales(c, t, t);
  }
};

// ---- epilogue: one 32-row slab of the wave tile (accumulator tile rows 2 HALF, 2 HALF + 1) --------------------------------------
__device__ __forceinline__ float4 mx_finish(const Mx8Params& p, float4 v, float4 b4) {
  v.x += b4.x; v.y += b4.y; v.z += b4.z; v.w += b4.w;
  if (p.act == 1) { v.x = gelu_erf(v.x); v.y = gelu_erf(v.y); v.z = gelu_erf(v.z); v.w = gelu_erf(v.w); }
  return v;
}
// the row's 32-column MX block = 8 consecutive lanes x 4 columns: quantise as lr2_quant_mxfp8 would the stored row
__device__ __forceinline__ void mx_quant_store(const Mx8Params& p, float4 v, int m, int n, int lane, bool ok) {
  int e;
  const int w = mx_quant4_group8(v, e);
  if (ok) {
    *reinterpret_cast<int*>(p.out_q + (size_t)m * p.N + n) = w;
    if ((lane & 7) == 0) p.out_s[(size_t)m * (p.N / 32) + (n >> 5)] = (uint8_t)(e + 127);
  }
}

// Straight-line forms of a slab that lies inside the matrix, chosen ONCE per slab (wave-uniform) -- the encoder's four products:
//   FORM 0: (+ bias) -> ONE bf16 plane (QKV)          FORM 1: -> bf16 hi / lo planes          FORM 2: + residual -> fp32 (output
//   projection, FFN-2)   FORM 3 / 4: (GELU for 4) -> MX-FP8 (FFN-1).
// The general body below decides everything per pass: a dozen wave-uniform branches, exec-masked stores, a residual select that made
// the compiler wait (vmcnt: loads AND stores, in order) for stores two passes back, 64-bit address arithmetic per store -- 16 us per
// K = 1024 tile against 17 us of main loop.  Same operations in the same order per element as the general body: same bytes.
template <int HALF, int FORM>
__device__ __forceinline__ void epilogue_slab_fast(const Mx8Params& p, f32x4_t (&acc)[8][4], float* slab, int mw, int nw, int lane, float4 b4) {
  constexpr int NP = 8, RPP = 4, LDW = 68;
  const int row0 = lane >> 4, col = (lane & 15) * 4, n = nw + col;
  const int mbase = mw + 32 * HALF + row0;
  float4 rr[NP];
  if constexpr (FORM == 2) {
    const float* r0 = p.resid + (size_t)mbase * p.ld_resid + n;
#pragma unroll
    for (int pass = 0; pass < NP; ++pass) rr[pass] = lr2gemm::ld4(r0 + (size_t)(pass * RPP) * p.ld_resid);
  }
  lr2gemm::epilogue_to_slab<64, 8, 4, HALF>(acc, slab, lane);
  float4 v[NP];
  lr2gemm::slab_read_all<64, NP, 0>(lds_addr(slab) + (uint32_t)((row0 * LDW + col) * 4), v);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int pass = 0; pass < NP; ++pass) {
    const int m = mbase + pass * RPP;
    float4 x = v[pass];
    x.x += b4.x; x.y += b4.y; x.z += b4.z; x.w += b4.w;
    if constexpr (FORM == 4) { x.x = gelu_erf(x.x); x.y = gelu_erf(x.y); x.z = gelu_erf(x.z); x.w = gelu_erf(x.w); }
    if constexpr (FORM == 2) {
      x.x += rr[pass].x; x.y += rr[pass].y; x.z += rr[pass].z; x.w += rr[pass].w;
      lr2gemm::st4(p.out + (size_t)m * p.ld_out + n, x);
    } else if constexpr (FORM == 0) {
      store_bf16x4(p.out_hi + (size_t)m * p.ld_planes + n, x);
    } else if constexpr (FORM == 1) {
      store_planes4(p.out_hi + (size_t)m * p.ld_planes + n, p.out_lo_off, x);
    } else {
      mx_quant_store(p, x, m, n, lane, true);
    }
  }
}

template <int HALF>
__device__ __forceinline__ void epilogue_slab(const Mx8Params& p, f32x4_t (&acc)[8][4], float* slab, int mw, int nw, int lane, float4 b4) {
  constexpr int NP = 8, RPP = 4, LDW = 68;
  const int row0 = lane >> 4, col = (lane & 15) * 4, n = nw + col;
  const int mbase = mw + 32 * HALF + row0;
  const bool inside = mw + 32 * HALF + 32 <= p.M;            // wave-uniform
  if (inside && p.act <= 1) {
    const bool f32 = p.out != nullptr, pl = p.out_hi != nullptr, mx = p.out_q != nullptr, rs = p.resid != nullptr;
    if (pl && !f32 && !mx && !rs && p.act == 0) {
      if (p.out_lo_off) epilogue_slab_fast<HALF, 1>(p, acc, slab, mw, nw, lane, b4);
      else epilogue_slab_fast<HALF, 0>(p, acc, slab, mw, nw, lane, b4);
      return;
    }
    if (f32 && rs && !pl && !mx && p.act == 0) { epilogue_slab_fast<HALF, 2>(p, acc, slab, mw, nw, lane, b4); return; }
    if (mx && !f32 && !pl && !rs) {
      if (p.act == 1) epilogue_slab_fast<HALF, 4>(p, acc, slab, mw, nw, lane, b4);
      else epilogue_slab_fast<HALF, 3>(p, acc, slab, mw, nw, lane, b4);
      return;
    }
  }
  float4 rr[NP];
  if (p.resid) {                                             // every residual request of the slab before its first store
    if (inside) {
#pragma unroll
      for (int pass = 0; pass < NP; ++pass) rr[pass] = lr2gemm::ld4(p.resid + (size_t)(mbase + pass * RPP) * p.ld_resid + n);
    } else {
#pragma unroll
      for (int pass = 0; pass < NP; ++pass) {
        const int m = mbase + pass * RPP;
        rr[pass] = lr2gemm::ld4(p.resid + (size_t)(m < p.M ? m : p.M - 1) * p.ld_resid + n);
      }
    }
  }
  lr2gemm::epilogue_to_slab<64, 8, 4, HALF>(acc, slab, lane);
  float4 v[NP];
  lr2gemm::slab_read_all<64, NP, 0>(lds_addr(slab) + (uint32_t)((row0 * LDW + col) * 4), v);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int pass = 0; pass < NP; ++pass) {
    const int m = mbase + pass * RPP;
    const bool ok = inside || m < p.M;
    float4 x = mx_finish(p, v[pass], b4);
    if (p.resid) { x.x += rr[pass].x; x.y += rr[pass].y; x.z += rr[pass].z; x.w += rr[pass].w; }
    if (ok) {
      if (p.out) lr2gemm::st4(p.out + (size_t)m * p.ld_out + n, x);
      if (p.out_hi) { if (p.out_lo_off) store_planes4(p.out_hi + (size_t)m * p.ld_planes + n, p.out_lo_off, x); else store_bf16x4(p.out_hi + (size_t)m * p.ld_planes + n, x); }
    }
    if (p.out_q) mx_quant_store(p, x, m, n, lane, ok);
  }
}

template <bool SC16>
__global__ __launch_bounds__(512, 2) void gemm256_mx_kernel(Mx8Params p, int tiles_m, int tiles_n) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;

  int tm, tn;
  tile_coords(tiles_m, tiles_n, blockIdx.x, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;
  const int ks = p.K / 32;                    // scale bytes per row

  Ctx c;
  c.nt = p.K / BKB;
  c.src.a = uniform_rsrc(p.aq, (uint32_t)((size_t)p.M * p.K));
  c.src.b = uniform_rsrc(p.bq, (uint32_t)((size_t)p.N * p.K));
  lane_setup<4>(c, smem, m0, n0, wave, lane, (uint64_t)p.K, (uint64_t)p.K, p.M, p.N);
  {
    const __amdgpu_buffer_rsrc_t sa = uniform_rsrc(p.as, (uint32_t)((size_t)p.M * ks));
    const __amdgpu_buffer_rsrc_t sb = uniform_rsrc(p.bs, (uint32_t)((size_t)p.N * ks));
    c.sc = wave < 4 ? sa : sb;
    const int srow = (wave < 4 ? m0 : n0) + (wave & 3) * 64 + lane;
    const uint64_t os = (uint64_t)srow * (uint64_t)ks;
    c.voff_s = (srow < (wave < 4 ? p.M : p.N) && os < (uint64_t)OOB) ? (uint32_t)os : OOB;
    const int r16 = lane & 15, q = lane >> 4;
    const uint32_t sm = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
    c.rd_sa = sm + RING + (SC16 ? (uint32_t)((wr * 128 + r16) * 16 + q) : (uint32_t)((wr * 128 + r16) * 4 + q));
    c.rd_sb = sm + RING + (SC16 ? 4096u + (uint32_t)((wc * 64 + r16) * 16 + q) : 1024u + (uint32_t)((wc * 64 + r16) * 4 + q));
    c.ks = ks;
  }

  f32x4_t acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  prologue<ScaleExtras<SC16>>(c, wr);
  for (int t = 0; t < c.nt; t += 2) {
    k_step<0, SC16>(c, t, acc);
    if (t + 1 < c.nt) k_step<1, SC16>(c, t + 1, acc);
  }
  drain(wr);

  const int mw = m0 + wr * 128, nw = n0 + wc * 64;
  if (nw + 64 > p.N || mw >= p.M) return;       // N % 128 == 0 <=> a wave's 64 columns are all inside or all outside
  float* slab = reinterpret_cast<float*>(smem) + wave * (32 * (64 + 4));
  float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (p.bias) b4 = lr2gemm::ld4(p.bias + nw + (lane & 15) * 4);
  asm volatile("" ::"v"(b4.x), "v"(b4.y), "v"(b4.z), "v"(b4.w));      // ONE wait for the bias, here (gemm_common.h::epilogue_wave)
  epilogue_slab<0>(p, acc, slab, mw, nw, lane, b4);
  if (mw + 32 < p.M) epilogue_slab<1>(p, acc, slab, mw, nw, lane, b4);
  if (mw + 64 < p.M) epilogue_slab<2>(p, acc, slab, mw, nw, lane, b4);
  if (mw + 96 < p.M) epilogue_slab<3>(p, acc, slab, mw, nw, lane, b4);
}

}  // namespace lr2mx256

int launch_gemm256_mx(const Mx8Params& p, hipStream_t stream) {
  using namespace lr2mx256;
  const int tiles_m = (p.M + BM - 1) / BM, tiles_n = (p.N + BN - 1) / BN;
  static bool attr_set = false;
  if (!attr_set) {
    if (lr2_allow_dynamic_lds(gemm256_mx_kernel<false>, LDS_BYTES, "gemm256_mx")) return LR2_ERR_LAUNCH;
    if (lr2_allow_dynamic_lds(gemm256_mx_kernel<true>, LDS_BYTES16, "gemm256_mx")) return LR2_ERR_LAUNCH;
    attr_set = true;
  }
  const dim3 grid(tiles_m * tiles_n);
  // whole 16-byte scale chunks per row (K / 32 a multiple of 16): the SC16 form; else the 4-byte form
  // (from K = 2048: at K = 1024 -- 8 steps -- the row gather in the prologue costs more than the seven later gathers it saves)
  const bool sc16 = (p.K % 512) == 0 && p.K >= 2048;
  if (sc16) LR2_LAUNCH(gemm256_mx_kernel<true>, grid, dim3(512), LDS_BYTES16, stream, p, tiles_m, tiles_n);
  else LR2_LAUNCH(gemm256_mx_kernel<false>, grid, dim3(512), LDS_BYTES, stream, p, tiles_m, tiles_n);
  return lr2_launch_status(__func__);
}
