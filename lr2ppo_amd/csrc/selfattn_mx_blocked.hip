// Single-plane bf16 inference attention for sequences longer than one LDS-resident head (FeatureExtractor(precision="bf16" | "mxfp8",
// attention_long=True); L > 288 through the schedules, any L >= 1 at the entry point): selfattn_mx.hip's contract -- Q, K, V ONE bf16 plane
// each, single-pass bf16 products, fp32 softmax, the context out as fp32 and / or MX-FP8 and / or ONE bf16 plane -- with the keys walked
// in blocks through LDS.  NOT the parity path: selfattn_fwd.hip's 3-pass kernels stay the default everywhere.
//
//   replaces: MultiHeadedAttention's scores / softmax / context (tencentpretrain/layers/multi_headed_attn.py:60-74) in inference,
//   key mask -10000 * (seg <= 0) added after the 1 / sqrt(64) scale as upstream; no dropout (inference mode), no lse.
//
// The loop is selfattn_b1_blocked.hip's self_attn_b1_train_fwd_blocked_kernel, restated without the dropout hash and the lse (that kernel
// sits at 242 - 254 VGPRs and is left alone): key blocks of 16 NT keys by lr2_self_attn_bf16_blocked_plan's rule (ceil(L / 224) equal
// rounded blocks of 10, 12 or 14 tiles, so every block holds a real key and the running maximum is finite after the first), one plane each
// of K (k_off image) and V (v_off image) per block; per 16-query sub-tile the running maximum m in log2 units, l = the fp32 sum of the
// unrounded p~ = exp2(s - m) and the un-normalised accumulator, rescaled by exp2(m - m') when m grows; p~ rounded to bf16 as the A operand
// of P V.  Same operations in the same order as that kernel at drop_p = 0: the bf16 plane is byte-equal to its output.  A wave carries up
// to MXL_SLOTS sub-tiles, more query chunks go into gridDim.x; every wave -- one whose sub-tiles lie past the last row too -- walks every
// block and meets every barrier, only its stores are skipped.
// The epilogue is the store half of selfattn_mx.hip's mx_phase_b: accumulator / l through the wave's private [16][HD + 4] fp32 slab, rows
// out as float4, through store_bf16x4 (round to nearest even), and as MX-FP8 by lr2_quant_mxfp8's rule per 32-column block.
//
// The same kernel serves the f16 inference mode above 288 tokens (FeatureExtractor(precision="f16", f16_attention_long=True);
// lr2_self_attn_fwd_f16_blocked below) through its compile-time parameter F16, as selfattn_mx.hip's kernels do: f16 planes in, fp32
// and / or ONE f16 plane out, no MX-FP8; one parameter list for both formats, null Oq / Os in f16.

#include "selfattn_b1.h"

namespace {

constexpr int MXL_SLOTS = 4;       // query sub-tiles a wave carries across the key blocks

template <bool F16, int NT, int NW, int SLOTS>
__global__ __launch_bounds__(64 * NW) void self_attn_plane_blocked_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
                                                                          const bf16_t* __restrict__ V, int ld,
                                                                          const int64_t* __restrict__ seg, float* __restrict__ Of,
                                                                          uint8_t* __restrict__ Oq, uint8_t* __restrict__ Os,
                                                                          bf16_t* __restrict__ Ob, int ld_o, int heads, int L,
                                                                          float scale, int n_blocks) {
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
    b1_load_frags(Q, (row0 + (ok ? q_row : 0)) * (size_t)ld + col0 + 8 * g, ok, q[j]);
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
            acc = mfma_plane<F16>(kf, q[j][ks], acc);
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
          const u32x4_t pw = {prob_pk<F16>(s[2 * u][0], s[2 * u][1]), prob_pk<F16>(s[2 * u][2], s[2 * u][3]),
                              prob_pk<F16>(s[2 * u + 1][0], s[2 * u + 1][1]), prob_pk<F16>(s[2 * u + 1][2], s[2 * u + 1][3])};
          const bf16x8_t pf = __builtin_bit_cast(bf16x8_t, pw);
          const int ra = 32 * u + 4 * g + tq, rb = ra + 16;
#pragma unroll
          for (int n = 0; n < 4; ++n) {
            const bf16x8_t vf = tr_pair(sV, ra, rb, 2 * n + (tp >> 1), 8 * (tp & 1));
            o[j][n] = mfma_plane<F16>(pf, vf, o[j][n]);
          }
        }
      }
    }
  }

  // ---- o[j][n][r] = O[query 4 g + r][hd 16 n + (l & 15)] / l -> slab -> row-contiguous fp32 / bf16 plane / MX-FP8 ----
  float* slab = sOut + wave * 16 * (HD + 4);        // private to the wave: no barrier from here on
  const size_t ubase = row0 * (size_t)ld_o + col0, sbase = row0 * (size_t)(ld_o / 32) + (col0 >> 5);
#pragma unroll
  for (int j = 0; j < SLOTS; ++j) {
    const int sub = sub_first + j * sub_step;
    if (sub < n_sub) {
      const float inv = 1.0f / l[j];
      // the lane's row / column numbers are re-derived here from an opaque copy: derived from `lane` itself they are hoisted above the
      // key-block loop and kept live through it, and the 160- and 192-key instantiations then spill
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
        if (Ob && ok) store_plane4<F16>(Ob + ubase + (lrow * (size_t)ld_o + (size_t)c), v);  // ONE bf16 / f16 plane: RNE of the fp32 context
        if (!F16 && Oq) {
          // the row's 32-column MX block = 8 consecutive lanes x 4 columns (the head's 64 columns are two blocks): as lr2_quant_mxfp8
          int e;
          const int w = mx_quant4_group8(v, e);
          if (ok) {
            *reinterpret_cast<int*>(Oq + ubase + (lrow * (size_t)ld_o + (size_t)c)) = w;
            if ((ln & 7) == 0) Os[sbase + (lrow * (size_t)(ld_o / 32) + (size_t)(c >> 5))] = (uint8_t)(e + 127);
          }
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// ---- launcher ----
uint64_t g_mxl_launches = 0;      // accepted calls since load (lr2_self_attn_fwd_bf16_blocked_launch_count)
uint64_t g_f16l_launches = 0;     // ... of the f16 entry point (lr2_self_attn_fwd_f16_blocked_launch_count)

template <bool F16, int NT>
int mxl_launch(const bf16_t* q, const bf16_t* k, const bf16_t* v, int ld, const int64_t* seg, float* of, uint8_t* oq, uint8_t* os,
               bf16_t* ob, int ld_o, int batch, int heads, int L, float scale, hipStream_t stream) {
  constexpr int LP = 16 * NT, NW = B1_NW, SLOTS = MXL_SLOTS;
  const size_t lds = (size_t)2 * LP * ROW_B + (size_t)LP * 4 + (size_t)NW * 16 * (HD + 4) * 4;
  static bool done = false;
  if (allow_lds_once(self_attn_plane_blocked_kernel<F16, NT, NW, SLOTS>, lds, done, F16 ? "self_attn_fwd_f16_blocked" : "self_attn_fwd_bf16_blocked"))
    return LR2_ERR_LAUNCH;
  const int n_sub = (L + 15) / 16;
  const int chunks = (n_sub + NW * SLOTS - 1) / (NW * SLOTS);
  LR2_LAUNCH((self_attn_plane_blocked_kernel<F16, NT, NW, SLOTS>), dim3(chunks, heads, batch), dim3(64 * NW), lds, stream, q, k, v, ld, seg, of,
             oq, os, ob, ld_o, heads, L, scale, (L + LP - 1) / LP);
  return lr2_launch_status(F16 ? "lr2_self_attn_fwd_f16_blocked" : "lr2_self_attn_fwd_bf16_blocked");
}

}  // namespace

extern "C" int lr2_self_attn_fwd_bf16_blocked(const void* q, const void* k, const void* v, int ld, const int64_t* seg, void* o_f32,
                                              void* o_q, void* o_scales, void* o_bf16, int ld_o, int batch, int heads, int L,
                                              int head_dim, float scale, void* stream) {
  if (!q || !k || !v || !seg || (!o_f32 && !o_q && !o_bf16) || batch <= 0 || heads <= 0) return LR2_ERR_ARG;
  if ((o_q != nullptr) != (o_scales != nullptr)) return LR2_ERR_ARG;
  if (!b1_aligned16(q) || !b1_aligned16(k) || !b1_aligned16(v) || !b1_aligned16(o_f32) || ((uintptr_t)o_bf16 & 7) || ((uintptr_t)o_q & 3))
    return LR2_ERR_ARG;
  if (head_dim != HD || L < 1 || ld < heads * HD || ld_o < heads * HD || (ld % 8) || (ld_o % 8) || (o_q && (ld_o % 32))) return LR2_ERR_SHAPE;
  // the block length is the training twin's: one rule in one place
  int block = 0;
  if (lr2_self_attn_bf16_blocked_plan(L, &block, nullptr, nullptr)) return LR2_ERR_LAUNCH;
  const bf16_t *qq = (const bf16_t*)q, *kk = (const bf16_t*)k, *vv = (const bf16_t*)v;
  hipStream_t s = (hipStream_t)stream;
  int rc = LR2_ERR_LAUNCH;      // a plan this dispatch does not know is an error, not another block
#define GO(NT) rc = mxl_launch<false, NT>(qq, kk, vv, ld, seg, (float*)o_f32, (uint8_t*)o_q, (uint8_t*)o_scales, (bf16_t*)o_bf16, ld_o, batch, heads, L, scale, s)
  if (block == 160) GO(10);
  else if (block == 192) GO(12);
  else if (block == 224) GO(14);
#undef GO
  if (rc == 0) ++g_mxl_launches;
  return rc;
}

extern "C" int lr2_self_attn_fwd_bf16_blocked_launch_count(uint64_t* count) {
  if (!count) return LR2_ERR_ARG;
  *count = g_mxl_launches;
  return 0;
}

// the same kernel on f16 planes (the "f16" inference mode with f16_attention_long): no MX-FP8 outputs, its own argument checks
extern "C" int lr2_self_attn_fwd_f16_blocked(const void* q, const void* k, const void* v, int ld, const int64_t* seg, void* o_f32,
                                             void* o_f16, int ld_o, int batch, int heads, int L, int head_dim, float scale,
                                             void* stream) {
  if (!q || !k || !v || !seg || (!o_f32 && !o_f16) || batch <= 0 || heads <= 0) return LR2_ERR_ARG;
  if (!b1_aligned16(q) || !b1_aligned16(k) || !b1_aligned16(v) || !b1_aligned16(o_f32) || ((uintptr_t)o_f16 & 7)) return LR2_ERR_ARG;
  if (head_dim != HD || L < 1 || ld < heads * HD || ld_o < heads * HD || (ld % 8) || (ld_o % 4)) return LR2_ERR_SHAPE;
  // the block length is the bf16 kernels': one rule in one place
  int block = 0;
  if (lr2_self_attn_bf16_blocked_plan(L, &block, nullptr, nullptr)) return LR2_ERR_LAUNCH;
  const f16_t *qq = (const f16_t*)q, *kk = (const f16_t*)k, *vv = (const f16_t*)v;
  hipStream_t s = (hipStream_t)stream;
  int rc = LR2_ERR_LAUNCH;      // a plan this dispatch does not know is an error, not another block
#define GO(NT) rc = mxl_launch<true, NT>(qq, kk, vv, ld, seg, (float*)o_f32, nullptr, nullptr, (f16_t*)o_f16, ld_o, batch, heads, L, scale, s)
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
