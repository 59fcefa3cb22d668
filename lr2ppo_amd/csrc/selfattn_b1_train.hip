// Encoder self-attention of the single-pass bf16 TRAINING mode (FeatureExtractor(precision="bf16_train", bf16_attention=True)):
// forward with dropout and log-sum-exp, and the recomputing backward, every operand and every output ONE bf16 plane, every product
// ONE v_mfma_f32_16x16x32_bf16 per tile pair, fp32 softmax.  NOT the parity path: selfattn_fwd.hip / selfattn_bwd.hip (hi / lo planes,
// three products per tile) stay the default everywhere; the mode opts in layer by layer (head_dim 64, L <= 288).
//
//   replaces: MultiHeadedAttention's scores / softmax / dropout / context (tencentpretrain/layers/multi_headed_attn.py:61-74) and
//   its autograd; key mask -10000 * (seg <= 0) added after the scale as upstream; the dropout mask is lr2_self_attn_fwd's stream.
//
// Structure: the simple one-workgroup-per-(sequence, head) form only -- 8 waves, the head's resident operands (K, V / Q, dO: L <= 288
// rows, one plane each, 72 KiB at most) in LDS, each wave walks over 16-row sub-tiles; small batches split the sub-tiles over up to
// 4 workgroups (attn_chunks).  No persistent form, no LDS-DMA movers.
//   * forward  = self_attn_plane_kernel<false, ..>'s arithmetic (selfattn_mx.hip), instruction for instruction, + the dropout factor on the
//     un-normalised probabilities before they are rounded to the A fragment of P V + lse: at drop_p = 0 the same bytes;
//   * backward = self_attn_bwd_dq_kernel / self_attn_bwd_dkv_kernel's one-block recomputing form (selfattn_bwd.hip) with one plane
//     where those stage two and one MFMA where they call mfma3; dS, Pd = P o M and the three outputs are rounded to bf16 (RNE).
// Rounding sites beside the operands' own: P~ M (forward), dS (both backward kernels), Pd (dK / dV kernel), O, dQ, dK, dV.

#include "selfattn_b1.h"

namespace {

// ---- forward: self_attn_plane_kernel<false, ..> with dropout on the probabilities and the log-sum-exp ----
template <int NT, int NW>
__global__ __launch_bounds__(64 * NW) void self_attn_b1_train_fwd_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
                                                                         const bf16_t* __restrict__ V, int ld,
                                                                         const int64_t* __restrict__ seg, bf16_t* __restrict__ Ob, int ld_o,
                                                                         float* __restrict__ lse, int heads, int L, float scale,
                                                                         DropP dr) {
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
    b1_load_frags(Q, (row0 + (ok ? q_row_ : 0)) * (size_t)ld + col0 + 8 * g, ok, f);
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
    const int q_row = sub * 16 + qn;
    // ---- S^T tiles: s[t][r] = S[query qn][key 16 t + 4 g + r] ----
    f32x4_t s[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const bf16x8_t kf = *reinterpret_cast<const bf16x8_t*>(sK + k_off(16 * t + qn, g + 4 * ks));
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, q[ks], acc, 0, 0, 0);
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
    if (lse && g == 0 && q_row < L) lse[((size_t)b * heads + h) * L + q_row] = mx * LN2 + logf(sum);
    // ---- dropout on the un-normalised probabilities (the row sum above is taken before it): lr2_self_attn_fwd's mask stream ----
    if (dr.thr) {
      const uint64_t drow = (((uint64_t)b * heads + h) * L + (uint64_t)(q_row < L ? q_row : 0)) * mask_pitch(L);
#pragma unroll
      for (int t = 0; t < NT; ++t) s[t] = drop_mul4v(dr, drow + 16 * t + 4 * g, s[t]);
    }
    // ---- O = (P~ V) / sum: P~ fragments straight from the accumulators (the contraction index is permuted the same way on both
    // operands: lane (tq, tp) supplies V rows base + tq of a 4-row group, as in selfattn_fwd.hip) ----
    f32x4_t o[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) o[n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const int i16 = lane & 15, tq = i16 >> 2, tp = i16 & 3;
#pragma unroll
    for (int u = 0; u < NT / 2; ++u) {
      const u32x4_t pw = {cvt_pk_bf16(s[2 * u][0], s[2 * u][1]), cvt_pk_bf16(s[2 * u][2], s[2 * u][3]),
                          cvt_pk_bf16(s[2 * u + 1][0], s[2 * u + 1][1]), cvt_pk_bf16(s[2 * u + 1][2], s[2 * u + 1][3])};
      const bf16x8_t pf = __builtin_bit_cast(bf16x8_t, pw);
      const int ra = 32 * u + 4 * g + tq, rb = ra + 16;
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const bf16x8_t vf = tr_pair(sV, ra, rb, 2 * n + (tp >> 1), 8 * (tp & 1));
        o[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, vf, o[n], 0, 0, 0);
      }
    }
    // ---- o[n][r] = O[query 4 g + r][hd 16 n + (l & 15)] -> slab -> row-contiguous bf16 ----
    float inv_q[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) inv_q[r] = __shfl(inv, 4 * g + r, 64);
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) o[n][r] = o[n][r] * inv_q[r];
    b1_store_tile(o, slab, lane, sub * 16, L, Ob, (size_t)ld_o, row0 * (size_t)ld_o + col0);
  }
}

// ---- backward, part 1: dQ (+ the per-query statistics part 2 needs) ----
// Workgroup = (sequence, head); K and V of the head in LDS, the transposed layout (lane = one query, 4 keys per 16-key tile):
//   S^T = K Q^T, P = softmax;  dPd^T = V dO^T;  dP = dPd o M;  D = sum_k dP P;  dS = P (dP - D) * scale -> bf16;  dQ = dS K
template <int NT, int NW>
__global__ __launch_bounds__(64 * NW) void self_attn_b1_bwd_dq_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
                                                                      const bf16_t* __restrict__ V, int ld, const bf16_t* __restrict__ dO,
                                                                      int ld_do, const int64_t* __restrict__ seg, bf16_t* __restrict__ dQ,
                                                                      int ld_dq, float* __restrict__ lse, float* __restrict__ dsum,
                                                                      int heads, int L, float scale, DropP dr) {
  constexpr int LP = 16 * NT;
  constexpr int PLANE = LP * ROW_B;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sK = smem;
  char* sV = smem + PLANE;            // K image too: V is an A operand here (rows = keys, contraction over hd)
  float* sMask = reinterpret_cast<float*>(smem + 2 * PLANE);
  float* sOut = sMask + LP;
  const int h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t row0 = (size_t)b * L;
  const int col0 = h * HD;
  b1_stage_rows2<NT, 64 * NW>(K, ld, V, ld, row0, col0, L, tid, sK, sV);
  for (int j = tid; j < LP; j += 64 * NW) sMask[j] = j < L ? ((seg[row0 + j] > 0) ? 0.f : -10000.0f) : -INFINITY;
  const int qn = lane & 15, g = lane >> 4;
  __syncthreads();
  const int n_sub = (L + 15) >> 4;
  for (int sub = blockIdx.x * NW + wave; sub < n_sub; sub += gridDim.x * NW) {
    const int q_row = sub * 16 + qn;
    const bool q_ok = q_row < L;
    bf16x8_t qf[2], gf[2];
    b1_load_frags(Q, (row0 + (q_ok ? q_row : 0)) * (size_t)ld + col0 + 8 * g, q_ok, qf);
    b1_load_frags(dO, (row0 + (q_ok ? q_row : 0)) * (size_t)ld_do + col0 + 8 * g, q_ok, gf);

    f32x4_t s[NT], dp[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) b1_s_dp_tile(sK, sV, t, lane, qf, gf, s[t], dp[t]);      // S^T = K Q^T, dPd^T = V dO^T
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const float4 mk = *reinterpret_cast<const float4*>(sMask + 16 * t + 4 * g);
      s[t][0] = s[t][0] * scale + mk.x;
      s[t][1] = s[t][1] * scale + mk.y;
      s[t][2] = s[t][2] * scale + mk.z;
      s[t][3] = s[t][3] * scale + mk.w;
      mx = fmaxf(fmaxf(mx, fmaxf(s[t][0], s[t][1])), fmaxf(s[t][2], s[t][3]));
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[t][r] = exp_fast(s[t][r] - mx);
        sum += s[t][r];
      }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.0f / sum;
    const uint64_t drow = (((uint64_t)b * heads + h) * L + (uint64_t)(q_ok ? q_row : 0)) * mask_pitch(L);
    float dd = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (dr.thr) dp[t] = drop_mul4v(dr, drow + 16 * t + 4 * g, dp[t]);    // dP = dPd o M
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[t][r] *= inv;                                                     // P
        dd += dp[t][r] * s[t][r];
      }
    }
    dd += __shfl_xor(dd, 16, 64);
    dd += __shfl_xor(dd, 32, 64);
    if (g == 0 && q_ok) {
      const size_t si = ((size_t)b * heads + h) * L + q_row;
      lse[si] = mx + logf(sum);
      dsum[si] = dd;
    }
    f32x4_t o[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) o[n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < NT / 2; ++u) {
      float e[8];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        e[r] = s[2 * u][r] * (dp[2 * u][r] - dd) * scale;
        e[4 + r] = s[2 * u + 1][r] * (dp[2 * u + 1][r] - dd) * scale;
      }
      b1_accum_block(e, sK, u, lane, o);                                  // dQ += dS K
    }
    b1_store_tile(o, sOut + wave * 16 * (HD + 4), lane, sub * 16, L, dQ, (size_t)ld_dq, row0 * (size_t)ld_dq + col0);
  }
}

// ---- backward, part 2: dK, dV ----
// Workgroup = (sequence, head); Q and dO of the head in LDS; each wave owns 16 keys (K, V fragments in registers) and walks over the
// queries in the NON-transposed layout (lane = one key, 4 queries per 16-query tile):
//   S = Q K^T, P = exp(S scale + mask - lse[q]);  dPd = dO V^T;  Pd = P o M -> bf16, dS = P (dPd o M - D[q]) * scale -> bf16
//   dV = Pd^T dO,  dK = dS^T Q
template <int NT, int NW>
__global__ __launch_bounds__(64 * NW) void self_attn_b1_bwd_dkv_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
                                                                       const bf16_t* __restrict__ V, int ld, const bf16_t* __restrict__ dO,
                                                                       int ld_do, const int64_t* __restrict__ seg, bf16_t* __restrict__ dK,
                                                                       bf16_t* __restrict__ dV, int ld_dkv, const float* __restrict__ lse,
                                                                       const float* __restrict__ dsum, int heads, int L, float scale,
                                                                       DropP dr) {
  constexpr int LP = 16 * NT;
  constexpr int PLANE = LP * ROW_B;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sQ = smem;                    // K image: fragment reads (rows = queries) + transposed reads
  char* sG = smem + PLANE;            // dO
  float* sLse = reinterpret_cast<float*>(smem + 2 * PLANE);   // [LP]
  float* sD = sLse + LP;                                      // [LP]
  float* sOut = sD + LP;
  const int h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t row0 = (size_t)b * L;
  const int col0 = h * HD;
  b1_stage_rows2<NT, 64 * NW>(Q, ld, dO, ld_do, row0, col0, L, tid, sQ, sG);
  {
    const size_t si0 = ((size_t)b * heads + h) * L;
    for (int j = tid; j < LP; j += 64 * NW) {
      sLse[j] = j < L ? lse[si0 + j] : INFINITY;      // padded queries: P = exp(-inf) = 0
      sD[j] = j < L ? dsum[si0 + j] : 0.f;
    }
  }
  const int kn = lane & 15, g = lane >> 4;
  __syncthreads();
  const int n_sub = (L + 15) >> 4;
  for (int sub = blockIdx.x * NW + wave; sub < n_sub; sub += gridDim.x * NW) {
    const int key = sub * 16 + kn;
    const bool k_ok = key < L;
    bf16x8_t kf[2], vf[2];
    b1_load_frags(K, (row0 + (k_ok ? key : 0)) * (size_t)ld + col0 + 8 * g, k_ok, kf);
    b1_load_frags(V, (row0 + (k_ok ? key : 0)) * (size_t)ld + col0 + 8 * g, k_ok, vf);
    const float kmask = k_ok ? ((seg[row0 + key] > 0) ? 0.f : -10000.0f) : -INFINITY;

    f32x4_t dv[4], dk[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) dv[n] = dk[n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const uint64_t dbase = ((uint64_t)b * heads + h) * (uint64_t)L;
#pragma unroll 1
    for (int u = 0; u < NT / 2; ++u) {
      float pd[8], ds[8];
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int t = 2 * u + half;
        f32x4_t a, d;
        b1_s_dp_tile(sQ, sG, t, lane, kf, vf, a, d);      // S[query 16t + 4g + r][key kn], dPd
        const float4 ls = *reinterpret_cast<const float4*>(sLse + 16 * t + 4 * g);
        const float4 dd = *reinterpret_cast<const float4*>(sD + 16 * t + 4 * g);
        const float lsv[4] = {ls.x, ls.y, ls.z, ls.w}, ddv[4] = {dd.x, dd.y, dd.z, dd.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = exp_fast(a[r] * scale + kmask - lsv[r]);
          float m = 1.0f;
          if (dr.thr) {
            const int q = 16 * t + 4 * g + r;
            m = drop_mul(dr, (dbase + (uint64_t)(q < L ? q : 0)) * mask_pitch(L) + (uint64_t)(k_ok ? key : 0));
          }
          pd[4 * half + r] = p * m;
          ds[4 * half + r] = p * (d[r] * m - ddv[r]) * scale;
        }
      }
      b1_accum_block(pd, sG, u, lane, dv);      // dV += Pd^T dO
      b1_accum_block(ds, sQ, u, lane, dk);      // dK += dS^T Q
    }
    float* slab = sOut + wave * 16 * (HD + 4);
    b1_store_tile(dk, slab, lane, sub * 16, L, dK, (size_t)ld_dkv, row0 * (size_t)ld_dkv + col0);
    b1_store_tile(dv, slab, lane, sub * 16, L, dV, (size_t)ld_dkv, row0 * (size_t)ld_dkv + col0);
  }
}

// ---- launchers ----
uint64_t g_b1_launches[2] = {0, 0};      // forward, backward calls since load (host-side: lr2_self_attn_bf16_train_launch_counts)

// grid.x: attn_chunks, and never more workgroups than there are groups of B1_NW sub-tiles
inline dim3 b1_grid(const B1Args& a) {
  const int n_sub = (a.L + 15) / 16, max_chunks = (n_sub + B1_NW - 1) / B1_NW;
  int chunks = attn_chunks(a.batch, a.heads, a.L);
  if (chunks > max_chunks) chunks = max_chunks;
  return dim3(chunks, a.heads, a.batch);
}

template <int NT>
int b1_launch_fwd(const B1Args& a, bf16_t* o, int ld_o, float* lse) {
  constexpr int LP = 16 * NT, NW = B1_NW;
  const size_t lds = (size_t)2 * LP * ROW_B + (size_t)LP * 4 + (size_t)NW * 16 * (HD + 4) * 4;
  static bool done = false;
  if (allow_lds_once(self_attn_b1_train_fwd_kernel<NT, NW>, lds, done, "self_attn_fwd_bf16_train")) return LR2_ERR_LAUNCH;
  LR2_LAUNCH((self_attn_b1_train_fwd_kernel<NT, NW>), b1_grid(a), dim3(64 * NW), lds, a.stream, a.q, a.k, a.v, a.ld, a.seg, o, ld_o, lse,
             a.heads, a.L, a.scale, a.dr);
  return lr2_launch_status("lr2_self_attn_fwd_bf16_train");
}

template <int NT>
int b1_launch_bwd(const B1Args& a, const bf16_t* go, int ld_do, bf16_t* dq, bf16_t* dk, bf16_t* dv, int ld_d, float* lse, float* dsum) {
  constexpr int LP = 16 * NT, NW = B1_NW;
  const size_t lds1 = (size_t)2 * LP * ROW_B + (size_t)LP * 4 + (size_t)NW * 16 * (HD + 4) * 4;
  const size_t lds2 = (size_t)2 * LP * ROW_B + (size_t)LP * 8 + (size_t)NW * 16 * (HD + 4) * 4;
  static bool done1 = false, done2 = false;
  if (allow_lds_once(self_attn_b1_bwd_dq_kernel<NT, NW>, lds1, done1, "self_attn_bwd_bf16(dq)")) return LR2_ERR_LAUNCH;
  if (allow_lds_once(self_attn_b1_bwd_dkv_kernel<NT, NW>, lds2, done2, "self_attn_bwd_bf16(dkv)")) return LR2_ERR_LAUNCH;
  const dim3 grid = b1_grid(a);
  LR2_LAUNCH((self_attn_b1_bwd_dq_kernel<NT, NW>), grid, dim3(64 * NW), lds1, a.stream, a.q, a.k, a.v, a.ld, go, ld_do, a.seg, dq, ld_d,
             lse, dsum, a.heads, a.L, a.scale, a.dr);
  if (lr2_launch_status("lr2_self_attn_bwd_bf16(dq)")) return LR2_ERR_LAUNCH;
  LR2_LAUNCH((self_attn_b1_bwd_dkv_kernel<NT, NW>), grid, dim3(64 * NW), lds2, a.stream, a.q, a.k, a.v, a.ld, go, ld_do, a.seg, dk, dv,
             ld_d, (const float*)lse, (const float*)dsum, a.heads, a.L, a.scale, a.dr);
  return lr2_launch_status("lr2_self_attn_bwd_bf16(dkv)");
}

}  // namespace

#define LR2_B1_DISPATCH(L, CALL)   \
  if ((L) <= 64) rc = CALL(4);     \
  else if ((L) <= 128) rc = CALL(8);   \
  else if ((L) <= 224) rc = CALL(14);  \
  else rc = CALL(18);

extern "C" int lr2_self_attn_fwd_bf16_train(const void* q, const void* k, const void* v, int ld, const int64_t* seg, void* o_bf16,
                                            int ld_o, void* lse, float drop_p, uint64_t drop_seed, uint32_t drop_site, int batch,
                                            int heads, int L, int head_dim, float scale, void* stream) {
  if (!q || !k || !v || !seg || !o_bf16 || batch <= 0 || heads <= 0) return LR2_ERR_ARG;
  if (!(drop_p >= 0.f && drop_p < 1.f)) return LR2_ERR_ARG;
  if (!b1_aligned16(q) || !b1_aligned16(k) || !b1_aligned16(v) || ((uintptr_t)o_bf16 & 7)) return LR2_ERR_ARG;
  if (head_dim != HD || L < 1 || L > 288 || ld < heads * HD || ld_o < heads * HD || (ld % 8) || (ld_o % 8)) return LR2_ERR_SHAPE;
  const B1Args a{(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, ld, seg, batch, heads, L, scale,
                 make_drop(drop_p, drop_seed, drop_site), (hipStream_t)stream};
  int rc;
#define CALL(NT) b1_launch_fwd<NT>(a, (bf16_t*)o_bf16, ld_o, (float*)lse)
  LR2_B1_DISPATCH(L, CALL)
#undef CALL
  if (rc == 0) ++g_b1_launches[0];
  return rc;
}

extern "C" int lr2_self_attn_bwd_bf16(const void* q, const void* k, const void* v, int ld, const void* d_o, int ld_do, const int64_t* seg,
                                      void* dq, void* dk, void* dv, int ld_d, void* lse_ws, void* dsum_ws, float drop_p,
                                      uint64_t drop_seed, uint32_t drop_site, int batch, int heads, int L, int head_dim, float scale,
                                      void* stream) {
  if (!q || !k || !v || !d_o || !seg || !dq || !dk || !dv || !lse_ws || !dsum_ws || batch <= 0 || heads <= 0) return LR2_ERR_ARG;
  if (!(drop_p >= 0.f && drop_p < 1.f)) return LR2_ERR_ARG;
  if (!b1_aligned16(q) || !b1_aligned16(k) || !b1_aligned16(v) || !b1_aligned16(d_o) || ((uintptr_t)dq & 7) || ((uintptr_t)dk & 7) ||
      ((uintptr_t)dv & 7))
    return LR2_ERR_ARG;
  if (head_dim != HD || L < 1 || L > 288 || ld < heads * HD || ld_do < heads * HD || ld_d < heads * HD || (ld % 8) || (ld_do % 8) ||
      (ld_d % 8))
    return LR2_ERR_SHAPE;
  const B1Args a{(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, ld, seg, batch, heads, L, scale,
                 make_drop(drop_p, drop_seed, drop_site), (hipStream_t)stream};
  int rc;
#define CALL(NT) \
  b1_launch_bwd<NT>(a, (const bf16_t*)d_o, ld_do, (bf16_t*)dq, (bf16_t*)dk, (bf16_t*)dv, ld_d, (float*)lse_ws, (float*)dsum_ws)
  LR2_B1_DISPATCH(L, CALL)
#undef CALL
  if (rc == 0) ++g_b1_launches[1];
  return rc;
}

extern "C" int lr2_self_attn_bf16_train_launch_counts(uint64_t counts[2]) {
  if (!counts) return LR2_ERR_ARG;
  counts[0] = g_b1_launches[0];
  counts[1] = g_b1_launches[1];
  return 0;
}
