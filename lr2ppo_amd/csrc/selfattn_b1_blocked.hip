// Single-plane bf16 training attention for sequences longer than one LDS-resident head
// (FeatureExtractor(precision="bf16_train", bf16_attention=True, bf16_attention_long=True); L > 288 through lr2ppo_amd.ops, any L >= 1 at the
// entry points): the arithmetic contract, the mask, the dropout stream and the rounding sites of selfattn_b1_train.hip, blocked.
//
//   replaces: MultiHeadedAttention's scores / softmax / dropout / context (tencentpretrain/layers/multi_headed_attn.py:61-74) and
//   its autograd; key mask -10000 * (seg <= 0) added after the scale as upstream; the dropout mask is lr2_self_attn_fwd's stream,
//   indexed by (query, key) through mask_pitch(L): blocking does not move it.
//
// The single-plane forms of selfattn_fwd.hip's self_attn_blocked_kernel and selfattn_bwd.hip's self_attn_bwd_{dq,dkv}_blocked_kernel:
// ONE plane staged where those stage two, one MFMA where they call mfma3, and the rounding sites of the one-block kernels (P~ M, dS, Pd, O,
// dQ, dK, dV).  8 waves per workgroup throughout; every wave -- one whose sub-tiles lie past the last row too -- walks every block and
// meets every barrier; only its stores are skipped.
//   * forward: key blocks of 16 NT keys by fwd_blocked_dispatch's rule (nb = ceil(L / 224) equal rounded blocks of 10, 12 or 14 tiles, so
//     every block holds a real key and the running maximum is finite after the first); per 16-query sub-tile the running maximum m (in
//     log2 units, as the one-block forward), the sum l of the unrounded, un-dropped P~ and the un-normalised accumulator; up to
//     B1L_SLOTS sub-tiles per wave, more query chunks in gridDim.x beyond that;
//   * dQ: key blocks of B1L_BWD_NT tiles = 256 keys (one plane each of K and V: the 64 KiB the parity kernel spends on 128), two sweeps:
//     sweep 1 -> m, l, a = sum exp(s - m) dP -> lse, D = a / l (written to the workspaces); sweep 2 -> dS -> bf16, dQ += dS K;
//   * dK / dV: a wave owns 16 keys; Q, dO, lse, D pass through LDS in blocks of 256 queries.

#include "selfattn_b1.h"

namespace {

constexpr int B1L_SLOTS = 4;       // query sub-tiles a forward wave carries across the key blocks
constexpr int B1L_BWD_NT = 16;     // tiles of a backward block: 256 keys (dQ) / 256 queries (dK, dV)

// the forward's key tiles per block: selfattn_fwd.hip's fwd_blocked_dispatch (tests/attn_cases.py::fwd_block restates it)
inline int b1l_fwd_tiles(int L) {
  const int nb = (L + 223) / 224;
  const int tiles = (((L + nb - 1) / nb) + 15) / 16;
  return tiles <= 10 ? 10 : tiles <= 12 ? 12 : 14;
}

// rows k0 .. k0 + 16 NT - 1 of one head's operands A and B into LDS, both in the K image; rows >= L are zeros
template <int NT, int NTHR>
__device__ __forceinline__ void b1l_stage_block2(const bf16_t* __restrict__ a, int ld_a, const bf16_t* __restrict__ b, int ld_b, size_t row0,
                                                 int col0, int k0, int L, int tid, char* sA, char* sB) {
  constexpr int LP = 16 * NT, TRIPS = (LP * 8 + NTHR - 1) / NTHR;
  u32x4_t av[TRIPS], bv[TRIPS];
#pragma unroll
  for (int it = 0; it < TRIPS; ++it) {
    const int i = tid + it * NTHR;
    const int r = i >> 3, u = i & 7;
    av[it] = u32x4_t{0, 0, 0, 0};
    bv[it] = av[it];
    if (i < LP * 8 && k0 + r < L) {
      av[it] = *reinterpret_cast<const u32x4_t*>(a + (row0 + k0 + r) * (size_t)ld_a + col0 + u * 8);
      bv[it] = *reinterpret_cast<const u32x4_t*>(b + (row0 + k0 + r) * (size_t)ld_b + col0 + u * 8);
    }
  }
#pragma unroll
  for (int it = 0; it < TRIPS; ++it) {
    const int i = tid + it * NTHR;
    const int r = i >> 3, u = i & 7;
    if (i < LP * 8) {
      *reinterpret_cast<u32x4_t*>(sA + k_off(r, u)) = av[it];
      *reinterpret_cast<u32x4_t*>(sB + k_off(r, u)) = bv[it];
    }
  }
}

// ---- forward ----
template <int NT, int NW, int SLOTS>
__global__ __launch_bounds__(64 * NW) void self_attn_b1_train_fwd_blocked_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
                                                                                 const bf16_t* __restrict__ V, int ld,
                                                                                 const int64_t* __restrict__ seg, bf16_t* __restrict__ Ob,
                                                                                 int ld_o, float* __restrict__ lse, int heads, int L,
                                                                                 float scale, DropP dr, int n_blocks) {
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
    {   // b1l_stage_block2 with V in the V image, kept here: through the helper (tried as a template flag) the 224-key instantiation
        // spills 8 VGPRs and the other two are scheduled differently
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
        const int q_row = sub * 16 + qn;
        f32x4_t s[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            const bf16x8_t kf = *reinterpret_cast<const bf16x8_t*>(sK + k_off(16 * t + qn, g + 4 * ks));
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, q[j][ks], acc, 0, 0, 0);
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
        l[j] = l[j] * alpha + sum;                     // the unrounded, un-dropped P~
        // the accumulator holds O[query 4g + r][..] in register r, the statistics belong to query (l & 15)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float a_r = __shfl(alpha, 4 * g + r, 64);
#pragma unroll
          for (int n = 0; n < 4; ++n) o[j][n][r] *= a_r;
        }
        if (dr.thr) {
          const uint64_t drow =
              (((uint64_t)b * heads + h) * L + (uint64_t)(q_row < L ? q_row : 0)) * mask_pitch(L) + (uint64_t)k0;
#pragma unroll
          for (int t = 0; t < NT; ++t) s[t] = drop_mul4v(dr, drow + 16 * t + 4 * g, s[t]);
        }
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
            o[j][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, vf, o[j][n], 0, 0, 0);
          }
        }
      }
    }
  }

  float* slab = sOut + wave * 16 * (HD + 4);        // private to the wave: no barrier from here on
#pragma unroll
  for (int j = 0; j < SLOTS; ++j) {
    const int sub = sub_first + j * sub_step;
    if (sub < n_sub) {
      const int q_row = sub * 16 + qn;
      const float inv = 1.0f / l[j];
      if (lse && g == 0 && q_row < L) lse[((size_t)b * heads + h) * L + q_row] = m[j] * LN2 + logf(l[j]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float inv_r = __shfl(inv, 4 * g + r, 64);
#pragma unroll
        for (int n = 0; n < 4; ++n) o[j][n][r] *= inv_r;
      }
      b1_store_tile(o[j], slab, lane, sub * 16, L, Ob, (size_t)ld_o, row0 * (size_t)ld_o + col0);
    }
  }
}

// ---- backward, part 1: dQ and the per-query statistics, two sweeps over the key blocks ----
template <int NT, int NW>
__global__ __launch_bounds__(64 * NW) void self_attn_b1_bwd_dq_blocked_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
                                                                              const bf16_t* __restrict__ V, int ld,
                                                                              const bf16_t* __restrict__ dO, int ld_do,
                                                                              const int64_t* __restrict__ seg, bf16_t* __restrict__ dQ,
                                                                              int ld_dq, float* __restrict__ lse, float* __restrict__ dsum,
                                                                              int heads, int L, float scale, DropP dr) {
  constexpr int LPB = 16 * NT;
  constexpr int PLANE = LPB * ROW_B;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sK = smem;
  char* sV = smem + PLANE;            // K image too: V is an A operand here
  float* sMask = reinterpret_cast<float*>(smem + 2 * PLANE);
  float* sOut = sMask + LPB;
  const int h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t row0 = (size_t)b * L;
  const int col0 = h * HD;
  const int qn = lane & 15, g = lane >> 4;
  const int sub = blockIdx.x * NW + wave;            // one 16-query sub-tile per wave (waves past the end idle through the barriers)
  const int q_row = sub * 16 + qn;
  const bool q_ok = q_row < L;
  bf16x8_t qf[2], gf[2];
  b1_load_frags(Q, (row0 + (q_ok ? q_row : 0)) * (size_t)ld + col0 + 8 * g, q_ok, qf);
  b1_load_frags(dO, (row0 + (q_ok ? q_row : 0)) * (size_t)ld_do + col0 + 8 * g, q_ok, gf);
  const uint64_t drow = (((uint64_t)b * heads + h) * L + (uint64_t)(q_ok ? q_row : 0)) * mask_pitch(L);

  auto stage = [&](int k0) {
    __syncthreads();                                 // the previous block's readers are done
    b1l_stage_block2<NT, 64 * NW>(K, ld, V, ld, row0, col0, k0, L, tid, sK, sV);
    for (int j = tid; j < LPB; j += 64 * NW) sMask[j] = k0 + j < L ? ((seg[row0 + k0 + j] > 0) ? 0.f : -10000.0f) : -INFINITY;
    __syncthreads();
  };
  // masked scores and dP = dPd o M of key tile t of the staged block (keys past L: P is 0 there, whatever the dropout mask says)
  auto tile = [&](int k0, int t, f32x4_t& sa, f32x4_t& d) {
    b1_s_dp_tile(sK, sV, t, lane, qf, gf, sa, d);      // S^T = K Q^T, dPd^T = V dO^T
    const float4 mk = *reinterpret_cast<const float4*>(sMask + 16 * t + 4 * g);
    sa[0] = sa[0] * scale + mk.x;
    sa[1] = sa[1] * scale + mk.y;
    sa[2] = sa[2] * scale + mk.z;
    sa[3] = sa[3] * scale + mk.w;
    if (dr.thr) d = drop_mul4v(dr, drow + (uint64_t)(k0 + 16 * t + 4 * g), d);
  };

  // ---- sweep 1: m, l = sum exp(s - m), a = sum exp(s - m) dP -> lse, D ----
  float m = -INFINITY, l = 0.f, a = 0.f;
#pragma unroll 1
  for (int k0 = 0; k0 < L; k0 += LPB) {
    stage(k0);
    // half a block at a time (NT / 2 score and NT / 2 dP tiles in registers); a half that is all padding leaves m, l, a as they are
#pragma unroll 1
    for (int t0 = 0; t0 < NT; t0 += NT / 2) {
      f32x4_t s[NT / 2], dp[NT / 2];
      float bm = -INFINITY;
#pragma unroll
      for (int t = 0; t < NT / 2; ++t) {
        tile(k0, t0 + t, s[t], dp[t]);
        bm = fmaxf(fmaxf(bm, fmaxf(s[t][0], s[t][1])), fmaxf(s[t][2], s[t][3]));
      }
      bm = fmaxf(bm, __shfl_xor(bm, 16, 64));
      bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
      const float m_new = fmaxf(m, bm);              // finite: key 0 is real, and m only grows
      const float corr = exp_fast(m - m_new);        // 0 on the first half of the first block (m = -inf)
      l *= corr;
      a *= corr;
#pragma unroll
      for (int t = 0; t < NT / 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = exp_fast(s[t][r] - m_new);
          l += e;
          a = __builtin_fmaf(e, dp[t][r], a);
        }
      m = m_new;
    }
  }
  l += __shfl_xor(l, 16, 64);                        // the lanes of one query hold disjoint key subsets
  l += __shfl_xor(l, 32, 64);
  a += __shfl_xor(a, 16, 64);
  a += __shfl_xor(a, 32, 64);
  const float lse_q = m + logf(l), dd = a / l;
  if (g == 0 && q_ok) {
    const size_t si = ((size_t)b * heads + h) * L + q_row;
    lse[si] = lse_q;
    dsum[si] = dd;
  }

  // ---- sweep 2: dS = P (dP - D) scale -> bf16, dQ += dS K, two key tiles at a time ----
  f32x4_t o[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) o[n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int k0 = 0; k0 < L; k0 += LPB) {
    stage(k0);
#pragma unroll 2
    for (int u = 0; u < NT / 2; ++u) {
      f32x4_t s0, s1, d0, d1;
      tile(k0, 2 * u, s0, d0);
      tile(k0, 2 * u + 1, s1, d1);
      float e[8];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        e[r] = exp_fast(s0[r] - lse_q) * (d0[r] - dd) * scale;
        e[4 + r] = exp_fast(s1[r] - lse_q) * (d1[r] - dd) * scale;
      }
      b1_accum_block(e, sK, u, lane, o);
    }
  }
  if (sub * 16 < L) b1_store_tile(o, sOut + wave * 16 * (HD + 4), lane, sub * 16, L, dQ, (size_t)ld_dq, row0 * (size_t)ld_dq + col0);
}

// ---- backward, part 2: dK, dV; the queries (Q, dO, lse, D) pass through LDS in blocks ----
template <int NT, int NW>
__global__ __launch_bounds__(64 * NW) void self_attn_b1_bwd_dkv_blocked_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
                                                                               const bf16_t* __restrict__ V, int ld,
                                                                               const bf16_t* __restrict__ dO, int ld_do,
                                                                               const int64_t* __restrict__ seg, bf16_t* __restrict__ dK,
                                                                               bf16_t* __restrict__ dV, int ld_dkv,
                                                                               const float* __restrict__ lse, const float* __restrict__ dsum,
                                                                               int heads, int L, float scale, DropP dr) {
  constexpr int LPB = 16 * NT;
  constexpr int PLANE = LPB * ROW_B;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sQ = smem;                    // K image: fragment reads (rows = queries) + transposed reads
  char* sG = smem + PLANE;            // dO
  float* sLse = reinterpret_cast<float*>(smem + 2 * PLANE);   // [LPB]
  float* sD = sLse + LPB;                                     // [LPB]
  float* sOut = sD + LPB;
  const int h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t row0 = (size_t)b * L;
  const int col0 = h * HD;
  const int kn = lane & 15, g = lane >> 4;
  const int sub = blockIdx.x * NW + wave;            // one 16-key sub-tile per wave (waves past the end idle through the barriers)
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
  const size_t si0 = ((size_t)b * heads + h) * L;
#pragma unroll 1
  for (int q0 = 0; q0 < L; q0 += LPB) {
    __syncthreads();                                 // the previous block's readers are done
    b1l_stage_block2<NT, 64 * NW>(Q, ld, dO, ld_do, row0, col0, q0, L, tid, sQ, sG);
    for (int j = tid; j < LPB; j += 64 * NW) {
      sLse[j] = q0 + j < L ? lse[si0 + q0 + j] : INFINITY;      // padded queries: P = exp(-inf) = 0
      sD[j] = q0 + j < L ? dsum[si0 + q0 + j] : 0.f;
    }
    __syncthreads();
#pragma unroll 1
    for (int u = 0; u < NT / 2; ++u) {
      float pd[8], ds[8];
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int t = 2 * u + half;
        f32x4_t sa, d;
        b1_s_dp_tile(sQ, sG, t, lane, kf, vf, sa, d);      // S[query q0 + 16t + 4g + r][key kn], dPd
        const float4 ls = *reinterpret_cast<const float4*>(sLse + 16 * t + 4 * g);
        const float4 dd = *reinterpret_cast<const float4*>(sD + 16 * t + 4 * g);
        const float lsv[4] = {ls.x, ls.y, ls.z, ls.w}, ddv[4] = {dd.x, dd.y, dd.z, dd.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = exp_fast(sa[r] * scale + kmask - lsv[r]);
          float mk = 1.0f;
          if (dr.thr) {
            const int q = q0 + 16 * t + 4 * g + r;
            mk = drop_mul(dr, (dbase + (uint64_t)(q < L ? q : 0)) * mask_pitch(L) + (uint64_t)(k_ok ? key : 0));
          }
          pd[4 * half + r] = p * mk;
          ds[4 * half + r] = p * (d[r] * mk - ddv[r]) * scale;
        }
      }
      b1_accum_block(pd, sG, u, lane, dv);      // dV += Pd^T dO
      b1_accum_block(ds, sQ, u, lane, dk);      // dK += dS^T Q
    }
  }
  if (sub * 16 < L) {
    float* slab = sOut + wave * 16 * (HD + 4);
    b1_store_tile(dk, slab, lane, sub * 16, L, dK, (size_t)ld_dkv, row0 * (size_t)ld_dkv + col0);
    b1_store_tile(dv, slab, lane, sub * 16, L, dV, (size_t)ld_dkv, row0 * (size_t)ld_dkv + col0);
  }
}

// ---- launchers ----
uint64_t g_b1l_launches[2] = {0, 0};     // forward, backward calls since load (lr2_self_attn_bf16_blocked_launch_counts)

// The block lengths of a call at this L: the launchers below and lr2_self_attn_bf16_blocked_plan both call it.
struct B1LPlan {
  int fwd_key_block, dq_key_block, dkv_query_block;
};
inline B1LPlan b1l_plan(int L) { return B1LPlan{16 * b1l_fwd_tiles(L), 16 * B1L_BWD_NT, 16 * B1L_BWD_NT}; }

template <int NT>
int b1l_launch_fwd(const B1Args& a, bf16_t* o, int ld_o, float* lse) {
  constexpr int LP = 16 * NT, NW = B1_NW, SLOTS = B1L_SLOTS;
  const size_t lds = (size_t)2 * LP * ROW_B + (size_t)LP * 4 + (size_t)NW * 16 * (HD + 4) * 4;
  static bool done = false;
  if (allow_lds_once(self_attn_b1_train_fwd_blocked_kernel<NT, NW, SLOTS>, lds, done, "self_attn_fwd_bf16_train_blocked")) return LR2_ERR_LAUNCH;
  const int n_sub = (a.L + 15) / 16;
  const int chunks = (n_sub + NW * SLOTS - 1) / (NW * SLOTS);
  LR2_LAUNCH((self_attn_b1_train_fwd_blocked_kernel<NT, NW, SLOTS>), dim3(chunks, a.heads, a.batch), dim3(64 * NW), lds, a.stream, a.q, a.k,
             a.v, a.ld, a.seg, o, ld_o, lse, a.heads, a.L, a.scale, a.dr, (a.L + LP - 1) / LP);
  return lr2_launch_status("lr2_self_attn_fwd_bf16_train_blocked");
}

template <int NT>
int b1l_launch_bwd(const B1Args& a, const bf16_t* go, int ld_do, bf16_t* dq, bf16_t* dk, bf16_t* dv, int ld_d, float* lse, float* dsum) {
  constexpr int LPB = 16 * NT, NW = B1_NW;
  const size_t lds1 = (size_t)2 * LPB * ROW_B + (size_t)LPB * 4 + (size_t)NW * 16 * (HD + 4) * 4;
  const size_t lds2 = (size_t)2 * LPB * ROW_B + (size_t)LPB * 8 + (size_t)NW * 16 * (HD + 4) * 4;
  static bool done1 = false, done2 = false;
  if (allow_lds_once(self_attn_b1_bwd_dq_blocked_kernel<NT, NW>, lds1, done1, "self_attn_bwd_bf16_blocked(dq)")) return LR2_ERR_LAUNCH;
  if (allow_lds_once(self_attn_b1_bwd_dkv_blocked_kernel<NT, NW>, lds2, done2, "self_attn_bwd_bf16_blocked(dkv)")) return LR2_ERR_LAUNCH;
  const int n_sub = (a.L + 15) / 16;
  const dim3 grid((n_sub + NW - 1) / NW, a.heads, a.batch);
  LR2_LAUNCH((self_attn_b1_bwd_dq_blocked_kernel<NT, NW>), grid, dim3(64 * NW), lds1, a.stream, a.q, a.k, a.v, a.ld, go, ld_do, a.seg, dq,
             ld_d, lse, dsum, a.heads, a.L, a.scale, a.dr);
  if (lr2_launch_status("lr2_self_attn_bwd_bf16_blocked(dq)")) return LR2_ERR_LAUNCH;
  LR2_LAUNCH((self_attn_b1_bwd_dkv_blocked_kernel<NT, NW>), grid, dim3(64 * NW), lds2, a.stream, a.q, a.k, a.v, a.ld, go, ld_do, a.seg, dk,
             dv, ld_d, (const float*)lse, (const float*)dsum, a.heads, a.L, a.scale, a.dr);
  return lr2_launch_status("lr2_self_attn_bwd_bf16_blocked(dkv)");
}

}  // namespace

extern "C" int lr2_self_attn_fwd_bf16_train_blocked(const void* q, const void* k, const void* v, int ld, const int64_t* seg, void* o_bf16,
                                                    int ld_o, void* lse, float drop_p, uint64_t drop_seed, uint32_t drop_site, int batch,
                                                    int heads, int L, int head_dim, float scale, void* stream) {
  if (!q || !k || !v || !seg || !o_bf16 || batch <= 0 || heads <= 0) return LR2_ERR_ARG;
  if (!(drop_p >= 0.f && drop_p < 1.f)) return LR2_ERR_ARG;
  if (!b1_aligned16(q) || !b1_aligned16(k) || !b1_aligned16(v) || ((uintptr_t)o_bf16 & 7)) return LR2_ERR_ARG;
  if (head_dim != HD || L < 1 || ld < heads * HD || ld_o < heads * HD || (ld % 8) || (ld_o % 8)) return LR2_ERR_SHAPE;
  const B1Args a{(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, ld, seg, batch, heads, L, scale,
                 make_drop(drop_p, drop_seed, drop_site), (hipStream_t)stream};
  const int block = b1l_plan(L).fwd_key_block;
  int rc;
  if (block == 160) rc = b1l_launch_fwd<10>(a, (bf16_t*)o_bf16, ld_o, (float*)lse);
  else if (block == 192) rc = b1l_launch_fwd<12>(a, (bf16_t*)o_bf16, ld_o, (float*)lse);
  else rc = b1l_launch_fwd<14>(a, (bf16_t*)o_bf16, ld_o, (float*)lse);
  if (rc == 0) ++g_b1l_launches[0];
  return rc;
}

extern "C" int lr2_self_attn_bwd_bf16_blocked(const void* q, const void* k, const void* v, int ld, const void* d_o, int ld_do,
                                              const int64_t* seg, void* dq, void* dk, void* dv, int ld_d, void* lse_ws, void* dsum_ws,
                                              float drop_p, uint64_t drop_seed, uint32_t drop_site, int batch, int heads, int L,
                                              int head_dim, float scale, void* stream) {
  if (!q || !k || !v || !d_o || !seg || !dq || !dk || !dv || !lse_ws || !dsum_ws || batch <= 0 || heads <= 0) return LR2_ERR_ARG;
  if (!(drop_p >= 0.f && drop_p < 1.f)) return LR2_ERR_ARG;
  if (!b1_aligned16(q) || !b1_aligned16(k) || !b1_aligned16(v) || !b1_aligned16(d_o) || ((uintptr_t)dq & 7) || ((uintptr_t)dk & 7) ||
      ((uintptr_t)dv & 7))
    return LR2_ERR_ARG;
  if (head_dim != HD || L < 1 || ld < heads * HD || ld_do < heads * HD || ld_d < heads * HD || (ld % 8) || (ld_do % 8) || (ld_d % 8))
    return LR2_ERR_SHAPE;
  const B1Args a{(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, ld, seg, batch, heads, L, scale,
                 make_drop(drop_p, drop_seed, drop_site), (hipStream_t)stream};
  // the block lengths are the plan's: one instantiation today, and a plan this dispatch does not know is an error, not another block
  const B1LPlan plan = b1l_plan(L);
  int rc = LR2_ERR_LAUNCH;
  if (plan.dq_key_block == 16 * B1L_BWD_NT && plan.dkv_query_block == 16 * B1L_BWD_NT)
    rc = b1l_launch_bwd<B1L_BWD_NT>(a, (const bf16_t*)d_o, ld_do, (bf16_t*)dq, (bf16_t*)dk, (bf16_t*)dv, ld_d, (float*)lse_ws,
                                    (float*)dsum_ws);
  if (rc == 0) ++g_b1l_launches[1];
  return rc;
}

extern "C" int lr2_self_attn_bf16_blocked_plan(int L, int* fwd_key_block, int* dq_key_block, int* dkv_query_block) {
  if (L < 1) return LR2_ERR_ARG;
  const B1LPlan p = b1l_plan(L);
  if (fwd_key_block) *fwd_key_block = p.fwd_key_block;
  if (dq_key_block) *dq_key_block = p.dq_key_block;
  if (dkv_query_block) *dkv_query_block = p.dkv_query_block;
  return 0;
}

extern "C" int lr2_self_attn_bf16_blocked_launch_counts(uint64_t counts[2]) {
  if (!counts) return LR2_ERR_ARG;
  counts[0] = g_b1l_launches[0];
  counts[1] = g_b1l_launches[1];
  return 0;
}
