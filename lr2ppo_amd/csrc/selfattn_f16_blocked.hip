// Single-plane f16 inference attention for sequences longer than one LDS-resident head (FeatureExtractor(precision="f16",
// f16_attention_long=True); L > 288 through the schedule, any L >= 1 at the entry point): selfattn_f16.hip's contract -- Q, K, V ONE f16
// plane each, single-pass f16 products (v_mfma_f32_16x16x32_f16), fp32 softmax, the context out as fp32 and / or ONE f16 plane -- with the
// keys walked in blocks through LDS.  NOT the parity path: selfattn_fwd.hip's 3-pass kernels stay the default everywhere.
//
//   replaces: MultiHeadedAttention's scores / softmax / context (tencentpretrain/layers/multi_headed_attn.py:60-74) in inference,
//   key mask -10000 * (seg <= 0) added after the 1 / sqrt(64) scale as upstream; no dropout (inference mode), no lse.
//
// The loop is selfattn_mx_blocked.hip's self_attn_bf16_mx_blocked_kernel, statement for statement, on f16 fragments -- as selfattn_f16.hip
// restates selfattn_mx.hip; a file of its own so that every existing kernel keeps its code.  Key blocks of 16 NT keys by
// lr2_self_attn_bf16_blocked_plan's rule (ceil(L / 224) equal rounded blocks of 10, 12 or 14 tiles, so every block holds a real key and the
// running maximum is finite after the first), one plane each of K (k_off image) and V (v_off image) per block; per 16-query sub-tile the
// running maximum m in log2 units, l = the fp32 sum of the unrounded p~ = exp2(s - m) and the un-normalised accumulator, rescaled by
// exp2(m - m') when m grows.  A wave carries up to F16L_SLOTS sub-tiles, more query chunks go into gridDim.x; every wave -- one whose
// sub-tiles lie past the last row too -- walks every block and meets every barrier, only its stores are skipped.  What differs from the
// bf16 kernel is what differs in selfattn_f16.hip:
//   * every product is __builtin_amdgcn_mfma_f32_16x16x32_f16 (the bf16 one's operand bytes and fragment layout: the staging, the
//     ds_read_b128 / ds_read_b64_tr_b16 fragment reads and the 16-byte fragment type -- bf16x8_t here means "16 raw bytes" -- are shared);
//   * p~ (in (0, 1]: no clamp needed) becomes the A operand of P V by the plain round-to-nearest-even conversion; below 2^-14 it is an
//     f16 subnormal, below 2^-25 zero -- an absolute error of at most 2^-25 against l >= 1;
//   * the epilogue is accumulator / l through the wave's private [16][HD + 4] fp32 slab, rows out as float4 and / or through common.h's
//     f16 plane writer (clamp to +-65504, RNE); there are no MX-FP8 outputs.

#include "selfattn_common.h"

namespace {

constexpr int F16L_SLOTS = 4;      // query sub-tiles a wave carries across the key blocks
constexpr int F16L_NW = 8;         // waves per workgroup: two per SIMD, <= 256 registers each

// selfattn_f16.hip's two helpers, restated: that file's kernels keep their code
__device__ __forceinline__ f32x4_t mfma_f16(bf16x8_t a, bf16x8_t b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
}
// two probabilities -> packed f16 pair (low half = a), one v_cvt_pk_f16_f32
__device__ __forceinline__ uint32_t prob_pk_f16(float a, float b) {
  f32x2_t v = {a, b};
  f16x2_t r = __builtin_convertvector(v, f16x2_t);
  return __builtin_bit_cast(uint32_t, r);
}

template <int NT, int NW, int SLOTS>
__global__ __launch_bounds__(64 * NW) void self_attn_f16_blocked_kernel(const f16_t* __restrict__ Q, const f16_t* __restrict__ K,
                                                                        const f16_t* __restrict__ V, int ld,
                                                                        const int64_t* __restrict__ seg, float* __restrict__ Of,
                                                                        f16_t* __restrict__ Oh, int ld_o, int heads, int L, float scale,
                                                                        int n_blocks) {
  constexpr int LP = 16 * NT;
  constexpr int PLANE = LP * ROW_B;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sK = smem;
  char* sV = smem + PLANE;
  float* sMask = reinterpret_cast<float*>(smem + 2 * PLANE);      // [LP], pre-multiplied by log2(e)
  float* sOut = sMask + LP;                                      // [NW waves][16][HD + 4]
  const int h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t row0 = (size_t)b * L;
  const int col0 = h * HD;
  const int qn = lane & 15, g = lane >> 4;
  const int n_sub = (L + 15) >> 4;
  const int sub_first = blockIdx.x * NW + wave, sub_step = gridDim.x * NW;   // host: SLOTS * sub_step >= n_sub
  const float scale2 = scale * LOG2E;

  bf16x8_t q[SLOTS][2];
  f32x4_t o[SLOTS][4];
  float m[SLOTS], l[SLOTS];
#pragma unroll
  for (int j = 0; j < SLOTS; ++j) {
    const int q_row = (sub_first + j * sub_step) * 16 + qn;
    const bool ok = q_row < L;
    const size_t qo = (row0 + (ok ? q_row : 0)) * (size_t)ld + col0 + 8 * g;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      u32x4_t a = {0, 0, 0, 0};
      if (ok) a = *reinterpret_cast<const u32x4_t*>(Q + qo + 32 * ks);
      q[j][ks] = __builtin_bit_cast(bf16x8_t, a);
    }
    m[j] = -INFINITY;
    l[j] = 0.f;
#pragma unroll
    for (int n = 0; n < 4; ++n) o[j][n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }

#pragma unroll 1
  for (int blk = 0; blk < n_blocks; ++blk) {
    const int k0 = blk * LP;
    if (blk) __syncthreads();                       // every wave is done reading the previous block
    {   // every request first, then the LDS writes; rows >= L are zeros
      constexpr int TRIPS = (LP * 8 + 64 * NW - 1) / (64 * NW);
      u32x4_t kk[TRIPS], vv[TRIPS];
#pragma unroll
      for (int it = 0; it < TRIPS; ++it) {
        const int i = tid + it * 64 * NW;
        const int r = i >> 3, u = i & 7;
        kk[it] = u32x4_t{0, 0, 0, 0};
        vv[it] = kk[it];
        if (i < LP * 8 && k0 + r < L) {
          const size_t off = (row0 + k0 + r) * (size_t)ld + col0 + u * 8;
          kk[it] = *reinterpret_cast<const u32x4_t*>(K + off);
          vv[it] = *reinterpret_cast<const u32x4_t*>(V + off);
        }
      }
#pragma unroll
      for (int it = 0; it < TRIPS; ++it) {
        const int i = tid + it * 64 * NW;
        const int r = i >> 3, u = i & 7;
        if (i < LP * 8) {
          *reinterpret_cast<u32x4_t*>(sK + k_off(r, u)) = kk[it];
          *reinterpret_cast<u32x4_t*>(sV + v_off(r, u)) = vv[it];
        }
      }
    }
    for (int j = tid; j < LP; j += 64 * NW)
      sMask[j] = k0 + j < L ? ((seg[row0 + k0 + j] > 0) ? 0.f : -10000.0f * LOG2E) : -INFINITY;
    __syncthreads();

#pragma unroll
    for (int j = 0; j < SLOTS; ++j) {
      const int sub = sub_first + j * sub_step;
      if (sub < n_sub) {            // wave-uniform; no barrier inside
        f32x4_t s[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            const bf16x8_t kf = *reinterpret_cast<const bf16x8_t*>(sK + k_off(16 * t + qn, g + 4 * ks));
            acc = mfma_f16(kf, q[j][ks], acc);
          }
          s[t] = acc;
        }
        float mx = m[j];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const float4 mk = *reinterpret_cast<const float4*>(sMask + 16 * t + 4 * g);
          s[t][0] = __builtin_fmaf(s[t][0], scale2, mk.x);
          s[t][1] = __builtin_fmaf(s[t][1], scale2, mk.y);
          s[t][2] = __builtin_fmaf(s[t][2], scale2, mk.z);
          s[t][3] = __builtin_fmaf(s[t][3], scale2, mk.w);
          mx = fmaxf(fmaxf(mx, fmaxf(s[t][0], s[t][1])), fmaxf(s[t][2], s[t][3]));
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));       // finite: every block holds a real key
        const float alpha = __builtin_amdgcn_exp2f(m[j] - mx);      // first block: exp2(-inf) = 0
        float sum = 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            s[t][r] = __builtin_amdgcn_exp2f(s[t][r] - mx);
            sum += s[t][r];
          }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        m[j] = mx;
        l[j] = l[j] * alpha + sum;                     // the unrounded P~
        // the accumulator holds O[query 4g + r][..] in register r, the statistics belong to query (l & 15)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float a_r = __shfl(alpha, 4 * g + r, 64);
#pragma unroll
          for (int n = 0; n < 4; ++n) o[j][n][r] *= a_r;
        }
        const int i16 = lane & 15, tq = i16 >> 2, tp = i16 & 3;
#pragma unroll
        for (int u = 0; u < NT / 2; ++u) {
          const u32x4_t pw = {prob_pk_f16(s[2 * u][0], s[2 * u][1]), prob_pk_f16(s[2 * u][2], s[2 * u][3]),
                              prob_pk_f16(s[2 * u + 1][0], s[2 * u + 1][1]), prob_pk_f16(s[2 * u + 1][2], s[2 * u + 1][3])};
          const bf16x8_t pf = __builtin_bit_cast(bf16x8_t, pw);
          const int ra = 32 * u + 4 * g + tq, rb = ra + 16;
#pragma unroll
          for (int n = 0; n < 4; ++n) {
            const bf16x8_t vf = tr_pair(sV, ra, rb, 2 * n + (tp >> 1), 8 * (tp & 1));
            o[j][n] = mfma_f16(pf, vf, o[j][n]);
          }
        }
      }
    }
  }

  // ---- o[j][n][r] = O[query 4 g + r][hd 16 n + (l & 15)] / l -> slab -> row-contiguous fp32 / f16 plane ----
  float* slab = sOut + wave * 16 * (HD + 4);        // private to the wave: no barrier from here on
  const size_t ubase = row0 * (size_t)ld_o + col0;
#pragma unroll
  for (int j = 0; j < SLOTS; ++j) {
    const int sub = sub_first + j * sub_step;
    if (sub < n_sub) {
      const float inv = 1.0f / l[j];
      // the lane's row / column numbers are re-derived here from an opaque copy: derived from `lane` itself they are hoisted above the
      // key-block loop and kept live through it (the bf16 kernel's 160- and 192-key instantiations then spill)
      const int ln = opaque(lane), eq = ln & 15, eg = ln >> 4;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float inv_r = __shfl(inv, 4 * eg + r, 64);
#pragma unroll
        for (int n = 0; n < 4; ++n) slab[(4 * eg + r) * (HD + 4) + 16 * n + eq] = o[j][n][r] * inv_r;
      }
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int pass = 0; pass < 4; ++pass) {
        const int r = pass * 4 + eg, c = eq * 4;
        const int qr = sub * 16 + r;
        const bool ok = qr < L;                     // rows >= L of the last sub-tile: computed, not stored
        const float4 v = *reinterpret_cast<const float4*>(slab + r * (HD + 4) + c);
        const size_t lrow = (size_t)(ok ? qr : 0);
        if (Of && ok) *reinterpret_cast<float4*>(Of + ubase + (lrow * (size_t)ld_o + (size_t)c)) = v;
        if (Oh && ok) store_f16x4(Oh + ubase + (lrow * (size_t)ld_o + (size_t)c), v);         // ONE f16 plane: RNE of the fp32 context
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// ---- launcher ----
uint64_t g_f16l_launches = 0;     // accepted calls since load (lr2_self_attn_fwd_f16_blocked_launch_count)

template <int NT>
int f16l_launch(const f16_t* q, const f16_t* k, const f16_t* v, int ld, const int64_t* seg, float* of, f16_t* oh, int ld_o, int batch,
                int heads, int L, float scale, hipStream_t stream) {
  constexpr int LP = 16 * NT, NW = F16L_NW, SLOTS = F16L_SLOTS;
  const size_t lds = (size_t)2 * LP * ROW_B + (size_t)LP * 4 + (size_t)NW * 16 * (HD + 4) * 4;
  static bool done = false;
  if (allow_lds_once(self_attn_f16_blocked_kernel<NT, NW, SLOTS>, lds, done, "self_attn_fwd_f16_blocked")) return LR2_ERR_LAUNCH;
  const int n_sub = (L + 15) / 16;
  const int chunks = (n_sub + NW * SLOTS - 1) / (NW * SLOTS);
  LR2_LAUNCH((self_attn_f16_blocked_kernel<NT, NW, SLOTS>), dim3(chunks, heads, batch), dim3(64 * NW), lds, stream, q, k, v, ld, seg, of, oh,
             ld_o, heads, L, scale, (L + LP - 1) / LP);
  return lr2_launch_status("lr2_self_attn_fwd_f16_blocked");
}

inline bool f16l_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int lr2_self_attn_fwd_f16_blocked(const void* q, const void* k, const void* v, int ld, const int64_t* seg, void* o_f32,
                                             void* o_f16, int ld_o, int batch, int heads, int L, int head_dim, float scale,
                                             void* stream) {
  if (!q || !k || !v || !seg || (!o_f32 && !o_f16) || batch <= 0 || heads <= 0) return LR2_ERR_ARG;
  if (!f16l_aligned16(q) || !f16l_aligned16(k) || !f16l_aligned16(v) || !f16l_aligned16(o_f32) || ((uintptr_t)o_f16 & 7)) return LR2_ERR_ARG;
  if (head_dim != HD || L < 1 || ld < heads * HD || ld_o < heads * HD || (ld % 8) || (ld_o % 4)) return LR2_ERR_SHAPE;
  // the block length is the bf16 kernels': one rule in one place
  int block = 0;
  if (lr2_self_attn_bf16_blocked_plan(L, &block, nullptr, nullptr)) return LR2_ERR_LAUNCH;
  const f16_t *qq = (const f16_t*)q, *kk = (const f16_t*)k, *vv = (const f16_t*)v;
  hipStream_t s = (hipStream_t)stream;
  int rc = LR2_ERR_LAUNCH;      // a plan this dispatch does not know is an error, not another block
#define GO(NT) rc = f16l_launch<NT>(qq, kk, vv, ld, seg, (float*)o_f32, (f16_t*)o_f16, ld_o, batch, heads, L, scale, s)
  if (block == 160) GO(10);
  else if (block == 192) GO(12);
  else if (block == 224) GO(14);
#undef GO
  if (rc == 0) ++g_f16l_launches;
  return rc;
}

extern "C" int lr2_self_attn_fwd_f16_blocked_launch_count(uint64_t* count) {
  if (!count) return LR2_ERR_ARG;
  *count = g_f16l_launches;
  return 0;
}
