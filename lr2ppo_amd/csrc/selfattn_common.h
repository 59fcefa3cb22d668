// What the self-attention sources share -- selfattn_fwd.hip (one-block, persistent and key-blocked forwards), selfattn_bwd.hip (recomputing
// and streaming persistent backwards), selfattn_mx.hip / selfattn_mx_blocked.hip (the single-plane inference forwards, bf16 and f16)
// and first_token_attn.hip (HD only): the constants and the probability dropout, the LDS images of a head's rows, the movers HBM -> LDS, MFMA fragment loads and tile stores, and
// the host-side pieces of the launchers (CU count, descriptor spans, the "does this shape take the persistent form" predicates), once.
//
// Left alone, on purpose:
//   * the 3-pass phases attn_phase_a / attn_phase_b (selfattn_fwd.hip) and the single-plane mx_phase_a / mx_phase_b (selfattn_mx.hip) are
//     not merged: different arithmetic (three products per tile against one, dropout, lse) and different register budgets (16 waves at
//     <= 128 VGPRs against 12 at <= 168);
//   * the one-block and the 128-row-blocked recomputing backward kernels are not merged into one: their wave counts differ (8 or 4 waves
//     walking sub-tiles against 4 waves with one sub-tile each) and their loops are shaped differently (one pass against two sweeps);
//     they share the staging and tile helpers of selfattn_bwd.hip instead;
//   * the mover / compute / idle loops of the three persistent 3-pass kernels and of the mx persistent kernel are as they were written:
//     DESIGN.md 4.5 has an open finding on the persistent forward, so a shared helper may serve them only if their instruction streams
//     stay what they were.  buf_rsrc, dma_rows and phase_barrier do; load_frags_u does not in self_attn_persist_kernel (the same
//     loads, another schedule of the whole loop), which therefore keeps that helper's body in its own load_q; dma_rows spells the
//     image's swizzle out instead of calling a helper for the same reason;
//   * blocked_subtiles (the key-blocked forward, selfattn_fwd.hip) keeps load_frags' body for its query fragments: no persistent
//     kernel, but through the helper its 5000 - 7000 instructions come out scheduled differently, and nothing here times that kernel
//     against its former self closely enough to accept that;
//   * dispatch thresholds (which L and batch run which kernel) are unchanged.
#pragma once
#include "common.h"
#include "lr2ppo_hip.h"

namespace {

// ---- constants and the dropout on the attention probabilities ----
constexpr int HD = 64;          // head dim
constexpr int ROW_B = HD * 2;   // bytes of one K / V row in one LDS plane
constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;

// Dropout on the attention probabilities (multi_headed_attn.py:72): element (b, h, q, key) of the [B, H, L, L] tensor
// is kept iff dropout_keep(key, flat index, thr); thr == 0 switches it off.
struct DropP {
  uint64_t key;
  uint32_t thr;
  float inv_keep;   // 1 / (1 - p)
};
__device__ __forceinline__ float drop_mul(const DropP& d, uint64_t idx) {
  return dropout_keep(d.key, idx, d.thr) ? d.inv_keep : 0.0f;
}
// The mask of probability (b, h, q, key) is element ((b * heads + h) * L + q) * mask_pitch(L) + key of the mask stream: rows are
// pitched to a multiple of 4 so that a lane's 4 consecutive keys 4j .. 4j + 3 are one aligned group = two hashes (dropout_keep4).
__device__ __forceinline__ uint64_t mask_pitch(int L) { return (uint64_t)((L + 3) & ~3); }
__device__ __forceinline__ f32x4_t drop_mul4v(const DropP& d, uint64_t idx4, f32x4_t x) {
  bool k[4];
  dropout_keep4(d.key, idx4, d.thr, k);
  return f32x4_t{k[0] ? x[0] * d.inv_keep : 0.0f, k[1] ? x[1] * d.inv_keep : 0.0f, k[2] ? x[2] * d.inv_keep : 0.0f,
                 k[3] ? x[3] * d.inv_keep : 0.0f};
}
// x[0..3] *= mask / keep of the aligned group starting at idx4
__device__ __forceinline__ void drop_mul4(const DropP& d, uint64_t idx4, float& x0, float& x1, float& x2, float& x3) {
  bool k[4];
  dropout_keep4(d.key, idx4, d.thr, k);
  x0 = k[0] ? x0 * d.inv_keep : 0.0f;
  x1 = k[1] ? x1 * d.inv_keep : 0.0f;
  x2 = k[2] ? x2 * d.inv_keep : 0.0f;
  x3 = k[3] ? x3 * d.inv_keep : 0.0f;
}
static inline DropP make_drop(float p, uint64_t seed, uint32_t site) {
  DropP d{0, 0, 1.0f};
  if (p > 0.f) {
    d.thr = dropout_threshold(p);
    d.inv_keep = 1.0f / (1.0f - p);
    d.key = (((uint64_t)site) << 40) ^ (seed * 0x9E3779B97F4A7C15ull);
  }
  return d;
}

// ---- LDS images of a plane: [rows][8 units of 16 B], unit u of row r at u ^ x(r) ----
//   IMG_K  x = (r >> 1) & 7: conflict-free ds_read_b128 fragment reads (as in gemm.hip);
//   IMG_V  x = 2 ((r >> 1) & 3), i.e. 32-B chunk c at c ^ ((r >> 1) & 3): the 8 rows one half-wave touches in a transposed read land on
//          8 different 32-B slots of the 256-B bank row;
//   IMG_D  x = 2 ((r >> 1) & 3) + ((r >> 3) & 1), for a plane that is read BOTH as row fragments (ds_read_b128: 16 rows x one 16-B unit)
//          and transposed (ds_read_b64_tr_b16: 8 rows x 32 B per half-wave).  x is a bijection of the 8 row pairs of a 16-row tile
//          (fragment reads: 16 distinct 16-B slots = all 64 banks once) and x >> 1 takes 4 distinct values on the 4 row pairs of each
//          8-row group (transposed reads: 8 distinct 32-B bank groups); IMG_K gives the second only two ways.
enum { IMG_K, IMG_V, IMG_D };
__device__ __forceinline__ int d_swz(int r) { return 2 * ((r >> 1) & 3) + ((r >> 3) & 1); }
__device__ __forceinline__ int k_off(int r, int u) { return r * ROW_B + ((u ^ ((r >> 1) & 7)) << 4); }
__device__ __forceinline__ int v_off(int r, int u) { return r * ROW_B + ((u ^ (((r >> 1) & 3) << 1)) << 4); }
__device__ __forceinline__ int d_off(int r, int u) { return r * ROW_B + ((u ^ d_swz(r)) << 4); }

// LDS fragment addresses as (per-lane base register) + (compile-time offset): the XOR swizzles above depend on the row only through
// bits that the tile index does not touch, so ONE base per (k-step) for K and one per head-column group for V serve every tile; the
// bases are made opaque to the optimiser (else it re-derives one address per read -- 70 live registers where 6 do).
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
  uint32_t a = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const char*)p;
  asm volatile("" : "+v"(a));
  return a;
}
// A copy of a lane-varying value the optimiser cannot see through: what is derived from it inside a loop is RE-derived every
// trip (a few integer instructions) instead of being hoisted and kept live -- or spilled -- across the whole persistent loop.
__device__ __forceinline__ int opaque(int v) {
  asm volatile("" : "+v"(v));
  return v;
}
__device__ __forceinline__ bf16x8_t lds_ld16(uint32_t a) {
  return *(__attribute__((address_space(3))) const bf16x8_t*)(uintptr_t)a;
}
// two ds_read_b64_tr_b16 (4 rows each) = the B fragment of a product whose contraction runs over the rows of the plane
__device__ __forceinline__ bf16x8_t lds_tr_pair(uint32_t a, uint32_t b) {
  const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(uintptr_t)a);
  const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(uintptr_t)b);
  typedef __attribute__((ext_vector_type(8))) short s16x8_t;
  const s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8_t, v);
}
// the same from rows row_a / row_b of a plane in the V image, by pointer ...
__device__ __forceinline__ bf16x8_t tr_pair(const char* plane, int row_a, int row_b, int u, int half8) {
  const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(plane + v_off(row_a, u) + half8));
  const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(plane + v_off(row_b, u) + half8));
  typedef __attribute__((ext_vector_type(8))) short s16x8_t;
  const s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8_t, v);
}
// ... and of a plane kept in the K image: correct, 2-4 way bank conflicts accepted
__device__ __forceinline__ bf16x8_t tr_pair_k(const char* plane, int row_a, int row_b, int u, int half8) {
  const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(plane + k_off(row_a, u) + half8));
  const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(plane + k_off(row_b, u) + half8));
  typedef __attribute__((ext_vector_type(8))) short s16x8_t;
  const s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8_t, v);
}

// ---- the persistent forms: one workgroup per CU walks over (sequence, head) pairs, the resident planes travel by LDS-DMA under the
// compute (self_attn_persist_kernel, self_attn_bwd_{dq,dkv}_persist_kernel, self_attn_plane_persist_kernel) ----
// A one-pair forward spends a quarter of its time waiting for its K / V planes (112 KiB per workgroup, one workgroup per CU: nothing
// else runs meanwhile), every workgroup pays its launch and the drain of its last stores, and its phases (staging, S, softmax, P V,
// stores) barely overlap: two waves per SIMD in the same phase (measured by ablation, profiles/experiments/README.md).  In a persistent
// kernel
//   * a workgroup is PS_WAVES = 16 waves at <= 128 VGPRs (mx: PM_WAVES = 12 at <= 168): compute wave w owns the 16-row sub-tile w of
//     every pair (mx: w and w + 10), the last two waves -- the movers -- only move data, waves with no sub-tile only keep the barriers
//     company: three to four waves per SIMD in different places instead of two in the same one;
//   * the movers issue every LDS-DMA piece (dma_rows below) and write the per-key / per-query scalars (mask, lse, D, dropout bytes);
//     they are the only waves that wait for memory: s_waitcnt vmcnt(0) BEFORE the phase_barrier that publishes what they loaded.  The
//     compute waves' global stores and their own next fragments (requested after the last product of a pair) stay in flight across
//     barriers: phase_barrier waits for lgkmcnt(0) only;
//   * RAW: a compute wave reads a plane only after the barrier that follows the movers' vmcnt(0) for it.  WAR: the movers refill a plane
//     only after the barrier that every compute wave passes once its LDS reads of that plane are retired (the lgkmcnt(0) in
//     phase_barrier); every wave of the workgroup -- movers, compute, idle -- executes the same number of barriers per pair.
// Forward (3-pass and mx), two barriers per pair: phase A = S = Q K^T + softmax touches K and the mask, phase B = O = P V touches V, the
// probabilities stay in registers between them.  During A of pair i the movers load V of pair i (free since the end of pair i - 1);
// barrier "after A" (every K read retired -> K free; V landed); during B they load K of pair i + 1 and write its mask into the OTHER
// half of the two-pair mask buffer (pair number `it` reads half it & 1: the mask of pair i is still being read by nobody in B, but its
// half is rewritten only during B of pair i + 1); barrier "after B" (every V read retired; K, mask landed).
// Streaming backward, two barriers per pair: the resident planes (K, V / Q, dO in IMG_D) are walked in 32-row blocks and refilled IN
// HALVES: after block H1 - 1 (barrier "mid") rows [0, 32 H1) are dead and the movers load them for the NEXT pair, after the last block
// (barrier "end") the rest; a mover waits for its pieces before the NEXT barrier, i.e. half a pair later.
constexpr int PS_WAVES = 16, PS_MOVERS = 2, PS_MAX_SUB = PS_WAVES - PS_MOVERS;
constexpr int PM_WAVES = 12, PM_MOVERS = 2, PM_COMPUTE = PM_WAVES - PM_MOVERS;     // selfattn_mx.hip

// every LDS access of this wave retired, then meet the workgroup (no vmcnt wait: stores and DMA stay in flight)
__device__ __forceinline__ void phase_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// buffer descriptor of `bytes` bytes from p (wave-uniform), raw addressing with the range check on
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* p, uint32_t bytes) {
  const uint64_t a = (uint64_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
  void* q = (void*)(((uint64_t)hi << 32) | (uint64_t)lo);
  return __builtin_amdgcn_make_buffer_rsrc(q, 0, __builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}
constexpr uint32_t DMA_OOB = 0xFFFFFF00u;   // voffset beyond any descriptor built here (operand_span_bytes refuses longer operands)

// Rows 8j .. 8j + 7 (j = j_begin, j_begin + jstep, ... < j_end) of one head's operand into its LDS image (IMG_K / IMG_V / IMG_D): NP = 2
// planes (hi, lo; PLANE = 16 NT rows apart in LDS; issued hi then lo for each j) or NP = 1 (lo is not used: pass hi again).  LDS-DMA
// writes lane-linearly (lane l -> byte 16 l of the 1-KiB piece = row l >> 3, slot l & 7), so the image's swizzle is applied to the SOURCE
// unit; rows >= L are out-of-range requests (the descriptor's range check writes zeros).
template <int NT, int IMG, int NP>
__device__ __forceinline__ void dma_rows(const __amdgpu_buffer_rsrc_t& hi, const __amdgpu_buffer_rsrc_t& lo, char* dst, int lane,
                                         int j_begin, int j_end, int jstep, uint32_t pair_off, uint32_t row_bytes, int L) {
  constexpr int PLANE = 16 * NT * ROW_B;
  const int rl = lane >> 3, sl = lane & 7;
  for (int j = j_begin; j < j_end; j += jstep) {
    const int r = 8 * j + rl;
    const int u = IMG == IMG_V ? (sl ^ (((r >> 1) & 3) << 1)) : IMG == IMG_K ? (sl ^ ((r >> 1) & 7)) : (sl ^ d_swz(r));
    const uint32_t v = r < L ? pair_off + (uint32_t)r * row_bytes + (uint32_t)u * 16u : DMA_OOB;
    char* d = dst + j * 1024;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(hi, LDS_PTR(d), 16, v, 0, 0, 0);
    if constexpr (NP == 2) __builtin_amdgcn_raw_ptr_buffer_load_lds(lo, LDS_PTR(d + PLANE), 16, v, 0, 0, 0);
  }
}

// ---- fragments and stores ----
// 16 rows x 64 columns of one planes matrix as MFMA fragments (lane: row l & 15, columns 8*(l >> 4) + 32*ks ..); !ok: zeros
__device__ __forceinline__ void load_frags(const bf16_t* hi_plane, size_t lo_off, size_t elem_off, bool ok, bf16x8_t (&fh)[2],
                                           bf16x8_t (&fl)[2]) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    u32x4_t a = {0, 0, 0, 0}, c = a;
    if (ok) {
      a = *reinterpret_cast<const u32x4_t*>(hi_plane + elem_off + 32 * ks);
      c = *reinterpret_cast<const u32x4_t*>(hi_plane + elem_off + 32 * ks + lo_off);
    }
    fh[ks] = __builtin_bit_cast(bf16x8_t, a);
    fl[ks] = __builtin_bit_cast(bf16x8_t, c);
  }
}
// the same with a wave-uniform base pointer + a 32-bit lane offset (scalar-base loads: no 64-bit address registers per lane)
__device__ __forceinline__ void load_frags_u(const bf16_t* ubase, size_t lo_off, uint32_t lane_off, bool ok, bf16x8_t (&fh)[2],
                                             bf16x8_t (&fl)[2]) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    u32x4_t a = {0, 0, 0, 0}, c = a;
    if (ok) {
      a = *reinterpret_cast<const u32x4_t*>(ubase + lane_off + 32 * ks);
      c = *reinterpret_cast<const u32x4_t*>(ubase + lo_off + lane_off + 32 * ks);
    }
    fh[ks] = __builtin_bit_cast(bf16x8_t, a);
    fl[ks] = __builtin_bit_cast(bf16x8_t, c);
  }
}

// fp32 x 8 -> A fragment pair (hi, lo) of the split product
__device__ __forceinline__ void split8(const float (&p)[8], bf16x8_t& hi, bf16x8_t& lo) {
  uint32_t h[4], l[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    h[i] = cvt_pk_bf16(p[2 * i], p[2 * i + 1]);
    l[i] = cvt_pk_bf16(p[2 * i] - __uint_as_float(h[i] << 16), p[2 * i + 1] - __uint_as_float(h[i] & 0xffff0000u));
  }
  hi = __builtin_bit_cast(bf16x8_t, (u32x4_t{h[0], h[1], h[2], h[3]}));
  lo = __builtin_bit_cast(bf16x8_t, (u32x4_t{l[0], l[1], l[2], l[3]}));
}
// acc += (ah + al) (bh + bl) without the lo x lo term
__device__ __forceinline__ f32x4_t mfma3(bf16x8_t ah, bf16x8_t al, bf16x8_t bh, bf16x8_t bl, f32x4_t acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, acc, 0, 0, 0);
}

// ---- the two operand formats of the single-plane inference kernels (selfattn_mx.hip, selfattn_mx_blocked.hip) ----
// F16 is a compile-time parameter of those kernels: false = bf16 planes (the "bf16" and MX-FP8 modes), true = IEEE f16 planes (the "f16"
// mode: 11 significand bits, three more).  The f16 MFMA has the bf16 one's operand bytes and fragment layout, so the staging, the
// ds_read_b128 / ds_read_b64_tr_b16 fragment reads and the 16-byte fragment type (bf16x8_t then means "16 raw bytes") are shared.  The
// format selects the three helpers below, whether the MX-FP8 outputs exist (bf16 only), and one sched_barrier of mx_phase_a -- no more.
__device__ __forceinline__ f32x4_t mfma_f16(bf16x8_t a, bf16x8_t b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
}
// two probabilities -> packed f16 pair (low half = a), one v_cvt_pk_f16_f32.  Un-normalised probabilities are in (0, 1]: no clamp needed;
// below 2^-14 they are f16 subnormals, below 2^-25 zero -- an absolute error of at most 2^-25 against a row sum >= 1, which is formed in
// fp32 from the unrounded values in both formats
__device__ __forceinline__ uint32_t prob_pk_f16(float a, float b) {
  f32x2_t v = {a, b};
  f16x2_t r = __builtin_convertvector(v, f16x2_t);
  return __builtin_bit_cast(uint32_t, r);
}
template <bool F16>
__device__ __forceinline__ f32x4_t mfma_plane(bf16x8_t a, bf16x8_t b, f32x4_t c) {
  if constexpr (F16) return mfma_f16(a, b, c);
  else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
template <bool F16>
__device__ __forceinline__ uint32_t prob_pk(float a, float b) {
  if constexpr (F16) return prob_pk_f16(a, b);
  else return cvt_pk_bf16(a, b);
}
// four context values -> ONE plane: round to nearest even (f16: common.h's writer, clamped to +-65504)
template <bool F16>
__device__ __forceinline__ void store_plane4(bf16_t* p, float4 v) {
  if constexpr (F16) store_f16x4(p, v);
  else store_bf16x4(p, v);
}

// 16 x 64 accumulator tile (o[n][r] = X[row 4g + r][col 16n + (l & 15)]) -> planes rows via the wave's LDS slab
__device__ __forceinline__ void store_tile_planes(const f32x4_t (&o)[4], float* slab, int lane, int row_first, int rows_valid,
                                                  bf16_t* dst_hi, size_t lo_off, size_t row_stride, size_t base) {
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
      store_planes4(dst_hi + base + (size_t)(row_first + r) * row_stride + c, lo_off, v);
    }
  }
  __builtin_amdgcn_wave_barrier();
}
// the same through a 16 x 32 slab, 32 columns at a time
__device__ __forceinline__ void store_tile_planes_half(const f32x4_t (&o)[4], float* slab, int lane, int row_first, int rows_valid,
                                                       bf16_t* dst_hi, size_t lo_off, size_t row_stride, size_t base) {
  const int qn = lane & 15, g = lane >> 4;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) slab[(4 * g + r) * (32 + 4) + 16 * n + qn] = o[2 * half + n][r];
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const int r = pass * 8 + (lane >> 3), c = (lane & 7) * 4;
      if (row_first + r < rows_valid) {
        const float4 v = *reinterpret_cast<const float4*>(slab + r * (32 + 4) + c);
        store_planes4(dst_hi + base + 32 * half + ((uint32_t)(row_first + r) * (uint32_t)row_stride + (uint32_t)c), lo_off, v);
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- host side ----
static inline int cu_count() {
  static int n = 0;
  if (n == 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
  }
  return n;
}
// one workgroup per CU, fewer when there are fewer pairs
static inline int persist_grid(int n_pairs) { return n_pairs < cu_count() ? n_pairs : cu_count(); }

template <typename Kern>
int allow_lds_once(Kern kern, size_t lds, bool& done, const char* what) {
  if (!done) {
    if (lr2_allow_dynamic_lds(kern, lds, what)) return LR2_ERR_LAUNCH;
    done = true;
  }
  return 0;
}

// A persistent 3-pass kernel (PS_WAVES waves: not the 12-wave mx kernel, which has one form) is compiled in two forms, DROP = false
// without the hash code and its registers: allow both their LDS once, launch the one this call needs.  what[drop] names the form in
// an error message.
template <typename Kern, typename... Args>
int launch_drop_form(bool drop, Kern plain, Kern with_drop, size_t lds_plain, size_t lds_drop, bool (&done)[2],
                     const char* const (&what)[2], int grid, hipStream_t stream, Args... args) {
  if (allow_lds_once(plain, lds_plain, done[0], what[0]) || allow_lds_once(with_drop, lds_drop, done[1], what[1])) return LR2_ERR_LAUNCH;
  LR2_LAUNCH(drop ? with_drop : plain, dim3(grid), dim3(64 * PS_WAVES), drop ? lds_drop : lds_plain, stream, args...);
  return lr2_launch_status(what[drop]);
}

// Bytes a descriptor spans from an operand's first element: the last row's head columns end (rows - 1) * ld + heads * 64 elements on.
// The persistent forms address an operand by 32-bit byte offsets below DMA_OOB: operand_fits32 says whether this one allows that.
static inline uint64_t operand_span_bytes(int batch, int L, int ld, int heads) {
  return ((uint64_t)batch * L - 1) * (uint64_t)ld * 2u + (uint64_t)heads * HD * 2u;
}
static inline bool operand_fits32(int batch, int L, int ld, int heads) {
  return operand_span_bytes(batch, L, ld, heads) < (uint64_t)DMA_OOB;
}
// Which shapes take the persistent form: at least one pair per CU, every sub-tile owned by a compute wave, 32-bit byte offsets into every
// operand.  One predicate per entry point; its launcher and its *_plan function both call it.
static inline bool fwd_persist_ok(int batch, int heads, int L, int ld) {                       // lr2_self_attn_fwd
  return batch * heads >= cu_count() && (L + 15) / 16 <= PS_MAX_SUB && operand_fits32(batch, L, ld, heads);
}
// the backward also needs the forward's output and log-sum-exp (o_hi != nullptr: lse is then an INPUT)
static inline bool bwd_persist_ok(int batch, int heads, int L, int ld, int ld_do, bool has_o) {  // lr2_self_attn_bwd
  return has_o && L <= 16 * PS_MAX_SUB && batch * heads >= cu_count() && operand_fits32(batch, L, ld, heads) &&
         operand_fits32(batch, L, ld_do, heads);
}
static inline bool bf16_persist_ok(int batch, int heads, int L, int ld) {                      // lr2_self_attn_fwd_bf16
  return batch * heads >= cu_count() && (L + 15) / 16 <= 2 * PM_COMPUTE && operand_fits32(batch, L, ld, heads);
}

// grid.x of the one-pair kernels: how many workgroups share one (sequence, head).  One is best (K/V or Q/dO are staged once) as long as
// the grid still fills the chip; small batches split the sub-tiles over up to 4 workgroups.
static inline int attn_chunks(int batch, int heads, int L) {
  const int n_sub = (L + 15) / 16, max_chunks = (n_sub + 3) / 4;
  int c = (512 + batch * heads - 1) / (batch * heads);
  if (c < 1) c = 1;
  return c > max_chunks ? max_chunks : c;
}

struct AttnArgs {
  const bf16_t *q, *k, *v;      // hi planes (lo plane lo_off elements behind), row stride ld
  size_t lo_off;
  int ld;
  const int64_t* seg;
  int batch, heads, L;
  float scale;
  DropP dr;
  hipStream_t stream;
};

}  // namespace
