// Encoder self-attention for the MX-FP8 mode (BASELINE.json configs[4] "fp8 MFMA"; FeatureExtractor(precision="mxfp8")): Q, K, V as ONE
// bf16 plane each (what lr2_gemm_mxfp8 writes with out_lo_off = 0), single-pass bf16 products on the matrix cores, fp32 softmax, and
// the result handed on as MX-FP8 (e4m3fn bytes + one E8M0 scale per 32 columns of a row): the A operand of the output projection,
// with no fp32 round trip and no separate quantise pass.  NOT the parity path -- selfattn_fwd.hip's split-bf16 (3-pass) kernels stay the
// default everywhere; here an operand keeps 8 mantissa bits, far more than the e4m3 elements around it.
//
//   replaces: MultiHeadedAttention's scores / softmax / context (tencentpretrain/layers/multi_headed_attn.py:60-74) in inference,
//   key mask -10000 * (seg <= 0) added after the 1 / sqrt(64) scale as upstream; no dropout (inference mode).
//
// Structure (selfattn_fwd.hip's one-block forward, with half the bytes and a third of the matrix work): one workgroup of 8 waves per
// (sequence, head); K and V of the head -- L <= 288 keys, one plane each -- resident in LDS (K rows XOR-swizzled for ds_read_b128
// fragments, V for ds_read_b64_tr_b16); each wave walks over 16-query sub-tiles: S^T = K Q^T (2 MFMAs per 16 keys), softmax in the
// log2 domain across the 4 lanes that share a query, P as bf16 straight from the accumulators, O = P V (4 MFMAs per 32 keys),
// 1 / sum on the 16 outputs, rows through the wave's LDS slab -> fp32 and / or MX-FP8.
//
// The same two kernels serve the f16 inference mode (FeatureExtractor(precision="f16"); lr2_self_attn_fwd_f16 below): Q, K, V as ONE f16
// plane each (what lr2_gemm_f16 writes with out_lo_off = 0), the context as fp32 and / or ONE f16 plane.  The format is the kernels'
// compile-time parameter F16; what it selects is listed in selfattn_common.h ("the two operand formats").  Both formats take one
// parameter list -- the f16 instantiations receive null Oq / Os -- so the bf16 instantiations are, instruction for instruction, what
// they were when this file held them alone (DESIGN.md 4.5 says how that is checked).

#include "selfattn_common.h"

namespace {

template <bool F16, int NT, int NW>
__global__ __launch_bounds__(64 * NW) void self_attn_plane_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
                                                                  const bf16_t* __restrict__ V, int ld,
                                                                  const int64_t* __restrict__ seg, float* __restrict__ Of,
                                                                  uint8_t* __restrict__ Oq, uint8_t* __restrict__ Os,
                                                                  bf16_t* __restrict__ Ob, int ld_o, int heads, int L, float scale) {
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

  auto load_q = [&](int sub_, bf16x8_t (&f)[2]) {
    const int q_row_ = sub_ * 16 + qn;
    const bool ok = sub_ < n_sub && q_row_ < L;
    const size_t o = (row0 + (ok ? q_row_ : 0)) * (size_t)ld + col0 + 8 * g;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      u32x4_t a = {0, 0, 0, 0};
      if (ok) a = *reinterpret_cast<const u32x4_t*>(Q + o + 32 * ks);
      f[ks] = __builtin_bit_cast(bf16x8_t, a);
    }
  };
  const int sub_first = blockIdx.x * NW + wave, sub_step = gridDim.x * NW;
  bf16x8_t q[2], q_next[2];
  load_q(sub_first, q_next);

  // ---- stage K, V and the key mask: every request first, then the LDS writes ----
  {
    constexpr int TRIPS = (LP * 8 + 64 * NW - 1) / (64 * NW);
    u32x4_t kk[TRIPS], vv[TRIPS];
#pragma unroll
    for (int it = 0; it < TRIPS; ++it) {
      const int i = tid + it * 64 * NW;
      const int r = i >> 3, u = i & 7;
      kk[it] = u32x4_t{0, 0, 0, 0};
      vv[it] = kk[it];
      if (i < LP * 8 && r < L) {
        const size_t o = (row0 + r) * (size_t)ld + col0 + u * 8;
        kk[it] = *reinterpret_cast<const u32x4_t*>(K + o);
        vv[it] = *reinterpret_cast<const u32x4_t*>(V + o);
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
  for (int j = tid; j < LP; j += 64 * NW) sMask[j] = j < L ? ((seg[row0 + j] > 0) ? 0.f : -10000.0f * LOG2E) : -INFINITY;
  __syncthreads();

  float* slab = sOut + wave * 16 * (HD + 4);
  const float scale2 = scale * LOG2E;
  for (int sub = sub_first; sub < n_sub; sub += sub_step) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) q[ks] = q_next[ks];
    load_q(sub + sub_step, q_next);
    // ---- S^T tiles: s[t][r] = S[query qn][key 16 t + 4 g + r] ----
    f32x4_t s[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const bf16x8_t kf = *reinterpret_cast<const bf16x8_t*>(sK + k_off(16 * t + qn, g + 4 * ks));
        acc = mfma_plane<F16>(kf, q[ks], acc);
      }
      s[t] = acc;
    }
    float mx = -INFINITY;
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
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
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
    const float inv = 1.0f / sum;
    // ---- O = (P~ V) / sum: P~ fragments straight from the accumulators (the contraction index is permuted the same way on both
    // operands: lane (tq, tp) supplies V rows base + tq of a 4-row group, as in selfattn_fwd.hip) ----
    f32x4_t o[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) o[n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
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
        o[n] = mfma_plane<F16>(pf, vf, o[n]);
      }
    }
    // ---- o[n][r] = O[query 4 g + r][hd 16 n + (l & 15)] -> slab -> row-contiguous fp32 / MX-FP8 ----
    float inv_q[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) inv_q[r] = __shfl(inv, 4 * g + r, 64);
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) slab[(4 * g + r) * (HD + 4) + 16 * n + qn] = o[n][r] * inv_q[r];
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
      const int r = pass * 4 + (lane >> 4), c = (lane & 15) * 4;
      const int qr = sub * 16 + r;
      const bool ok = qr < L;
      const float4 v = *reinterpret_cast<const float4*>(slab + r * (HD + 4) + c);
      const size_t row = row0 + (ok ? qr : 0);
      if (Of && ok) *reinterpret_cast<float4*>(Of + row * (size_t)ld_o + col0 + c) = v;
      if (Ob && ok) store_plane4<F16>(Ob + row * (size_t)ld_o + col0 + c, v);   // ONE bf16 / f16 plane: RNE of the fp32 context
      if (!F16 && Oq) {
        // the row's 32-column MX block = 8 consecutive lanes x 4 columns (the head's 64 columns are two blocks): as lr2_quant_mxfp8
        int e;
        const int w = mx_quant4_group8(v, e);
        if (ok) {
          *reinterpret_cast<int*>(Oq + row * (size_t)ld_o + col0 + c) = w;
          if ((lane & 7) == 0) Os[row * (size_t)(ld_o / 32) + ((col0 + c) >> 5)] = (uint8_t)(e + 127);
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- persistent form (round 4): one workgroup per CU walks over the (sequence, head) pairs ----
// selfattn_fwd.hip's persistent forward with one plane per operand (the protocol: selfattn_common.h): a pair is phase A (S = Q K^T +
// softmax of ALL the wave's sub-tiles: K, mask; the probabilities stay in registers as bf16 fragments) and phase B (O = P V: V).
// PM_WAVES = 12 waves (<= 168 VGPRs): compute wave w owns sub-tiles w and w + 10 (L <= 288: 18 sub-tiles at most).  Same arithmetic,
// same bits as the one-pair kernel above.

// phase A of one 16-query sub-tile: S^T = K Q^T, softmax in the log2 domain -> un-normalised probabilities as bf16 fragments + 1 / sum
template <bool F16, int NT>
__device__ __forceinline__ void mx_phase_a(const char* sK, const float* sMask, const bf16x8_t (&q)[2], int lane, float scale2,
                                           bf16x8_t (&pf)[NT / 2], float& inv) {
  const int qn = lane & 15, g = lane >> 4;
  const uint32_t kb[2] = {lds_addr(sK + k_off(qn, g)), lds_addr(sK + k_off(qn, g + 4))};
  f32x4_t s[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      acc = mfma_plane<F16>(lds_ld16(kb[ks] + 2048 * t), q[ks], acc);
    }
    s[t] = acc;
    // f16 only: K fragments are requested at most three tiles (six ds_read_b128) ahead: left free, the scheduler hoists enough of them
    // that the NT = 14 / 18 instantiations spill 2 / 16 VGPRs at the 168 a 12-wave workgroup has (the bf16 kernel lands just inside them)
    if constexpr (F16) {
      if (t % 3 == 2) __builtin_amdgcn_sched_barrier(0);
    }
  }
  float mx = -INFINITY;
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
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
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
  inv = 1.0f / sum;
#pragma unroll
  for (int u = 0; u < NT / 2; ++u) {
    const u32x4_t pw = {prob_pk<F16>(s[2 * u][0], s[2 * u][1]), prob_pk<F16>(s[2 * u][2], s[2 * u][3]),
                        prob_pk<F16>(s[2 * u + 1][0], s[2 * u + 1][1]), prob_pk<F16>(s[2 * u + 1][2], s[2 * u + 1][3])};
    pf[u] = __builtin_bit_cast(bf16x8_t, pw);
  }
}

// phase B: O = (P~ V) / sum, rows through the wave's slab -> fp32 and / or MX-FP8 (the one-pair kernel's code)
template <bool F16, int NT>
__device__ __forceinline__ void mx_phase_b(const char* sV, float* slab, const bf16x8_t (&pf)[NT / 2], float inv, int sub, int lane, int L,
                                           size_t row0, int col0, float* __restrict__ Of, uint8_t* __restrict__ Oq,
                                           uint8_t* __restrict__ Os, bf16_t* __restrict__ Ob, int ld_o) {
  const int qn = lane & 15, g = lane >> 4;
  const int i16 = lane & 15, tq = i16 >> 2, tp = i16 & 3;
  uint32_t vb[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) vb[n] = lds_addr(sV + v_off(4 * g + tq, 2 * n + (tp >> 1)) + 8 * (tp & 1));
  f32x4_t o[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) o[n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < NT / 2; ++u) {
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const uint32_t a = vb[n] + 4096 * u;
      o[n] = mfma_plane<F16>(pf[u], lds_tr_pair(a, a + 2048), o[n]);
    }
  }
  float inv_q[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) inv_q[r] = __shfl(inv, 4 * g + r, 64);
#pragma unroll
  for (int n = 0; n < 4; ++n)
#pragma unroll
    for (int r = 0; r < 4; ++r) slab[(4 * g + r) * (HD + 4) + 16 * n + qn] = o[n][r] * inv_q[r];
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {
    const int r = pass * 4 + (lane >> 4), c = (lane & 15) * 4;
    const int qr = sub * 16 + r;
    const bool ok = qr < L;
    const float4 v = *reinterpret_cast<const float4*>(slab + r * (HD + 4) + c);
    // wave-uniform 64-bit bases + 32-bit lane offsets: the stores take the scalar-base form
    const uint32_t lrow = (uint32_t)(ok ? qr : 0);
    const size_t ubase = row0 * (size_t)ld_o + col0, sbase = row0 * (size_t)(ld_o / 32) + (col0 >> 5);
    if (Of && ok) *reinterpret_cast<float4*>(Of + ubase + (lrow * (uint32_t)ld_o + (uint32_t)c)) = v;
    if (Ob && ok) store_plane4<F16>(Ob + ubase + (lrow * (uint32_t)ld_o + (uint32_t)c), v);
    if (!F16 && Oq) {
      int e;
      const int w = mx_quant4_group8(v, e);
      if (ok) {
        *reinterpret_cast<int*>(Oq + ubase + (lrow * (uint32_t)ld_o + (uint32_t)c)) = w;
        if ((lane & 7) == 0) Os[sbase + (lrow * (uint32_t)(ld_o / 32) + (uint32_t)(c >> 5))] = (uint8_t)(e + 127);
      }
    }
  }
  __builtin_amdgcn_wave_barrier();
}

template <bool F16, int NT>
__global__ __launch_bounds__(64 * PM_WAVES) void self_attn_plane_persist_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
                                                                                const bf16_t* __restrict__ V, int ld,
                                                                                const int64_t* __restrict__ seg, float* __restrict__ Of,
                                                                                uint8_t* __restrict__ Oq, uint8_t* __restrict__ Os,
                                                                                bf16_t* __restrict__ Ob, int ld_o, int heads, int L,
                                                                                float scale, int n_pairs, uint32_t kv_bytes) {
  constexpr int LP = 16 * NT;
  constexpr int PLANE = LP * ROW_B;
  constexpr int MK = (LP + 64 * PM_MOVERS - 1) / (64 * PM_MOVERS);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sK = smem;
  char* sV = smem + PLANE;
  float* sMask = reinterpret_cast<float*>(smem + 2 * PLANE);      // [2][LP]: pair number it reads half it & 1
  float* sOut = sMask + 2 * LP;                                  // [PM_COMPUTE waves][16][HD + 4]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n_sub = (L + 15) >> 4;
  const uint32_t row_bytes = (uint32_t)ld * 2u;
  int p = blockIdx.x;
  if (p >= n_pairs) return;
  int b = __builtin_amdgcn_readfirstlane(p / heads), h = p - b * heads;      // (the quotient comes out of vector instructions)
  size_t row0 = (size_t)b * L;
  int col0 = h * HD;

  if (wave >= PM_COMPUTE) {
    // ---- movers ----
    const __amdgpu_buffer_rsrc_t k_src = buf_rsrc(K, kv_bytes), v_src = buf_rsrc(V, kv_bytes);
    const int j0 = wave - PM_COMPUTE, mtid = tid - 64 * PM_COMPUTE;
    dma_rows<NT, IMG_K, 1>(k_src, k_src, sK, lane, j0, 2 * NT, PM_MOVERS, (uint32_t)((row0 * ld + col0) * 2), row_bytes, L);
    for (int j = mtid; j < LP; j += 64 * PM_MOVERS) sMask[j] = j < L ? ((seg[row0 + j] > 0) ? 0.f : -10000.0f * LOG2E) : -INFINITY;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    phase_barrier();
    for (int it = 0;; ++it) {
      dma_rows<NT, IMG_V, 1>(v_src, v_src, sV, lane, j0, 2 * NT, PM_MOVERS, (uint32_t)((row0 * ld + col0) * 2), row_bytes, L);
      const int pn = p + gridDim.x;
      const bool more = pn < n_pairs;
      const int bn = __builtin_amdgcn_readfirstlane(pn / heads), hn = pn - bn * heads;
      const size_t row0n = (size_t)bn * L;
      float mk[MK];
      if (more) {
#pragma unroll
        for (int i = 0; i < MK; ++i) {
          const int j = mtid + i * 64 * PM_MOVERS;
          mk[i] = j < L ? ((seg[row0n + j] > 0) ? 0.f : -10000.0f * LOG2E) : -INFINITY;
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                // V of this pair has landed
      phase_barrier();
      if (!more) break;
      dma_rows<NT, IMG_K, 1>(k_src, k_src, sK, lane, j0, 2 * NT, PM_MOVERS, (uint32_t)((row0n * ld + hn * HD) * 2), row_bytes, L);
      float* mnext = sMask + ((it + 1) & 1) * LP;
#pragma unroll
      for (int i = 0; i < MK; ++i) {
        const int j = mtid + i * 64 * PM_MOVERS;
        if (j < LP) mnext[j] = mk[i];
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                // K of the next pair has landed
      phase_barrier();
      p = pn; row0 = row0n; col0 = hn * HD;
    }
    return;
  }

  // ---- compute waves: sub-tiles `wave` and `wave + PM_COMPUTE` of every pair ----
  const int sub0 = wave, sub1 = wave + PM_COMPUTE;
  const bool has0 = sub0 < n_sub, has1 = sub1 < n_sub;
  float* slab = sOut + wave * 16 * (HD + 4);
  const float scale2 = scale * LOG2E;
  auto load_q = [&](size_t row0_, int col0_, int sub_, bf16x8_t (&f)[2]) {
    const int lane_ = opaque(lane);
    const int q_row_ = sub_ * 16 + (lane_ & 15);
    const bool ok = sub_ < n_sub && q_row_ < L;
    const bf16_t* ub = Q + row0_ * (size_t)ld + col0_;
    const uint32_t o = (uint32_t)(ok ? q_row_ : 0) * (uint32_t)ld + 8u * (uint32_t)(lane_ >> 4);
    // unconditional loads (rows past the end read row 0 and are zeroed by a select): a branch here drags the uniform address
    // arithmetic into the divergent block, i.e. onto vector registers
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const u32x4_t a = *reinterpret_cast<const u32x4_t*>(ub + o + 32 * ks);
      f[ks] = __builtin_bit_cast(bf16x8_t, (u32x4_t{ok ? a[0] : 0u, ok ? a[1] : 0u, ok ? a[2] : 0u, ok ? a[3] : 0u}));
    }
  };
  bf16x8_t q0[2];
  load_q(row0, col0, sub0, q0);
  phase_barrier();
  for (int it = 0;; ++it) {
    const float* mask = sMask + (it & 1) * LP;
    bf16x8_t p0[NT / 2], p1[NT / 2];
    float inv0 = 0.f, inv1 = 0.f;
    bf16x8_t q1[2];
    load_q(row0, col0, sub1, q1);                  // travels under the first sub-tile's phase A
    if (has0) mx_phase_a<F16, NT>(sK, mask, q0, opaque(lane), scale2, p0, inv0);
    if (has1) mx_phase_a<F16, NT>(sK, mask, q1, opaque(lane), scale2, p1, inv1);
    phase_barrier();
    const int pn = p + gridDim.x;
    const bool more = pn < n_pairs;
    const int bn = __builtin_amdgcn_readfirstlane(pn / heads), hn = pn - bn * heads;
    const size_t row0n = (size_t)bn * L;
    if (has0) mx_phase_b<F16, NT>(sV, slab, p0, inv0, sub0, opaque(lane), L, row0, col0, Of, Oq, Os, Ob, ld_o);
    if (more) load_q(row0n, hn * HD, sub0, q0);    // the next pair's first sub-tile: under the second sub-tile's P V
    if (has1) mx_phase_b<F16, NT>(sV, slab, p1, inv1, sub1, opaque(lane), L, row0, col0, Of, Oq, Os, Ob, ld_o);
    if (!more) break;
    phase_barrier();
    p = pn; row0 = row0n; col0 = hn * HD;
  }
}

template <bool F16, int NT>
int launch_persist(const bf16_t* q, const bf16_t* k, const bf16_t* v, int ld, const int64_t* seg, float* of, uint8_t* oq, uint8_t* os,
                   bf16_t* ob, int ld_o, int batch, int heads, int L, float scale, hipStream_t stream) {
  constexpr int LP = 16 * NT;
  const size_t lds = (size_t)2 * LP * ROW_B + (size_t)2 * LP * 4 + (size_t)PM_COMPUTE * 16 * (HD + 4) * 4;
  static bool done = false;
  if (allow_lds_once(self_attn_plane_persist_kernel<F16, NT>, lds, done, F16 ? "self_attn_fwd_f16(persistent)" : "self_attn_fwd_bf16(persistent)"))
    return LR2_ERR_LAUNCH;
  const int n_pairs = batch * heads;
  LR2_LAUNCH((self_attn_plane_persist_kernel<F16, NT>), dim3(persist_grid(n_pairs)), dim3(64 * PM_WAVES), lds, stream, q, k, v, ld, seg, of,
             oq, os, ob, ld_o, heads, L, scale, n_pairs, (uint32_t)operand_span_bytes(batch, L, ld, heads));
  return lr2_launch_status(F16 ? "lr2_self_attn_fwd_f16(persistent)" : "lr2_self_attn_fwd_bf16(persistent)");
}

template <bool F16, int NT>
int launch(const bf16_t* q, const bf16_t* k, const bf16_t* v, int ld, const int64_t* seg, float* of, uint8_t* oq, uint8_t* os, bf16_t* ob,
           int ld_o, int batch, int heads, int L, float scale, hipStream_t stream) {
  if (bf16_persist_ok(batch, heads, L, ld))
    return launch_persist<F16, NT>(q, k, v, ld, seg, of, oq, os, ob, ld_o, batch, heads, L, scale, stream);
  constexpr int LP = 16 * NT, NW = 8;
  const size_t lds = (size_t)2 * LP * ROW_B + (size_t)LP * 4 + (size_t)NW * 16 * (HD + 4) * 4;
  static bool done = false;
  if (allow_lds_once(self_attn_plane_kernel<F16, NT, NW>, lds, done, F16 ? "self_attn_fwd_f16" : "self_attn_fwd_bf16")) return LR2_ERR_LAUNCH;
  LR2_LAUNCH((self_attn_plane_kernel<F16, NT, NW>), dim3(1, heads, batch), dim3(64 * NW), lds, stream, q, k, v, ld, seg, of, oq, os, ob,
             ld_o, heads, L, scale);
  return lr2_launch_status(F16 ? "lr2_self_attn_fwd_f16" : "lr2_self_attn_fwd_bf16");
}

uint64_t g_launches_f16 = 0;     // accepted calls of lr2_self_attn_fwd_f16 (host-side counter)

}  // namespace

extern "C" int lr2_self_attn_fwd_bf16_plan(int batch, int heads, int L, int ld, int* persistent) {
  if (!persistent || batch <= 0 || heads <= 0 || L <= 0 || L > 288 || ld <= 0) return LR2_ERR_ARG;
  *persistent = bf16_persist_ok(batch, heads, L, ld) ? 1 : 0;
  return 0;
}

extern "C" int lr2_self_attn_fwd_bf16(const void* q, const void* k, const void* v, int ld, const int64_t* seg, void* o_f32, void* o_q,
                                      void* o_scales, void* o_bf16, int ld_o, int batch, int heads, int L, int head_dim, float scale,
                                      void* stream) {
  if (!q || !k || !v || !seg || (!o_f32 && !o_q && !o_bf16) || batch <= 0 || heads <= 0 || L <= 0) return LR2_ERR_ARG;
  if ((o_q != nullptr) != (o_scales != nullptr)) return LR2_ERR_ARG;
  if (head_dim != HD || L > 288 || (ld % 8) || ld_o < heads * HD || (ld_o % 32)) return LR2_ERR_SHAPE;
  const bf16_t *qq = (const bf16_t*)q, *kk = (const bf16_t*)k, *vv = (const bf16_t*)v;
  hipStream_t s = (hipStream_t)stream;
#define GO(NT) return launch<false, NT>(qq, kk, vv, ld, seg, (float*)o_f32, (uint8_t*)o_q, (uint8_t*)o_scales, (bf16_t*)o_bf16, ld_o, batch, heads, L, scale, s)
  if (L <= 64) GO(4);
  if (L <= 128) GO(8);
  if (L <= 224) GO(14);
  GO(18);
#undef GO
}

// the same kernels on f16 planes (the "f16" inference mode): no MX-FP8 outputs, its own argument checks
extern "C" int lr2_self_attn_fwd_f16_launch_count(uint64_t* count) {
  if (!count) return LR2_ERR_ARG;
  *count = g_launches_f16;
  return 0;
}

extern "C" int lr2_self_attn_fwd_f16(const void* q, const void* k, const void* v, int ld, const int64_t* seg, void* o_f32, void* o_f16,
                                     int ld_o, int batch, int heads, int L, int head_dim, float scale, void* stream) {
  if (!q || !k || !v || !seg || (!o_f32 && !o_f16) || batch <= 0 || heads <= 0 || L <= 0) return LR2_ERR_ARG;
  if (head_dim != HD || L > 288 || ld < heads * HD || (ld % 8) || ld_o < heads * HD || (ld_o % 4)) return LR2_ERR_SHAPE;
  const f16_t *qq = (const f16_t*)q, *kk = (const f16_t*)k, *vv = (const f16_t*)v;
  hipStream_t s = (hipStream_t)stream;
  ++g_launches_f16;
#define GO(NT) return launch<true, NT>(qq, kk, vv, ld, seg, (float*)o_f32, nullptr, nullptr, (f16_t*)o_f16, ld_o, batch, heads, L, scale, s)
  if (L <= 64) GO(4);
  if (L <= 128) GO(8);
  if (L <= 224) GO(14);
  GO(18);
#undef GO
}
