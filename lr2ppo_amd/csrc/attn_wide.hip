// Wide form of the XiT cross-attention pair (attn.hip has the 16-key form): 1 <= Lk <= 64 image tokens, for --max_imgs above 16.
// Same formulas, same fp32 FMA arithmetic and exp_fast, same outputs (fp32 or hi/lo planes); no atomics, every sum in a fixed order.
//  * K/V of one (sequence, head) stay resident in LDS: NB key blocks of 16 rows x 96 floats each, NB = ceil(Lk / 16) a template
//    parameter, so 2 x NB x 6 KiB (48 KiB at 64 keys) -- the reason for the limit of 64.
//  * One lane owns one query row and keeps all 16 NB scores (the backward: scores and dL/dp, 2 x 16 NB) in registers; the loops over
//    keys are fully unrolled, so softmax still needs no cross-lane traffic and nothing is recomputed.
//  * The backward's dK / dV phase runs once per key block: the lanes put the block's dS and c p columns into sS / sP [256][16]
//    (32 KiB), thread <-> (column d, half of the query rows) accumulates 16 + 16 sums as in the 16-key kernel, the two halves meet in
//    sAcc [2][32][97] -- which takes the place of sS / sP once every thread has finished reading them -- and are added in a fixed
//    order.  LDS: 12 NB + 32 KiB (80 KiB at NB = 4: two workgroups per CU).
//  * This file is compiled with -fno-slp-vectorize (_native.EXTRA_FLAGS).  The SLP vectoriser pairs the keys' FMA chains into
//    v_pk_fma_f32 and pays for it with a v_mov transposition of every K / V row and 256 VGPRs + 56 AGPRs in the backward (one
//    workgroup per CU); measured at the PPO shape it made the backward 1.3x (32 keys) to 1.7x (64 keys) slower.  Scalar FMAs take
//    189 VGPRs at NB = 4 (forward 178), no AGPRs, no scratch.
#include "common.h"
#include "lr2ppo_hip.h"

namespace {

constexpr int KB = 16;          // keys per block
constexpr int MAX_NB = 4;       // key blocks: Lk <= 64
constexpr int MAX_HD = 96;

// K / V rows of (b, h) -> LDS, rows Lk .. NK - 1 zero
template <int NK>
__device__ __forceinline__ void load_kv(float (*sK)[MAX_HD], float (*sV)[MAX_HD], const float* __restrict__ K,
                                        const float* __restrict__ V, int b, int h, int E, int Lk, int hd, int t) {
  for (int idx = t; idx < NK * hd; idx += 256) {
    const int j = idx / hd, d = idx % hd;
    float kv = 0.f, vv = 0.f;
    if (j < Lk) {
      const size_t o = ((size_t)b * Lk + j) * E + (size_t)h * hd + d;
      kv = K[o];
      vv = V[o];
    }
    sK[j][d] = kv;
    sV[j][d] = vv;
  }
}

// ----------------------------------------------------------------------------------------------
template <int NB>
__global__ __launch_bounds__(256) void xattn_fwd_wide_kernel(const float* __restrict__ Q, const float* __restrict__ K,
                                                             const float* __restrict__ V, float* __restrict__ O, int o_planes,
                                                             size_t o_lo_off, int heads, int Lq, int Lk, int hd,
                                                             float post_scale) {
  constexpr int NK = NB * KB;
  __shared__ __attribute__((aligned(16))) float sK[NK][MAX_HD];
  __shared__ __attribute__((aligned(16))) float sV[NK][MAX_HD];
  const int b = blockIdx.x / heads, h = blockIdx.x % heads;
  const int E = heads * hd;
  const int t = threadIdx.x;
  load_kv<NK>(sK, sV, K, V, b, h, E, Lk, hd, t);
  __syncthreads();
  if (t >= Lq) return;
  const float* q = Q + ((size_t)b * Lq + t) * E + (size_t)h * hd;
  float s[NK];
#pragma unroll
  for (int j = 0; j < NK; ++j) s[j] = 0.f;
  for (int d = 0; d < hd; d += 4) {
    const float4 q4 = *reinterpret_cast<const float4*>(q + d);
#pragma unroll
    for (int j = 0; j < NK; ++j) {
      const float4 k4 = *reinterpret_cast<const float4*>(&sK[j][d]);
      s[j] += q4.x * k4.x + q4.y * k4.y + q4.z * k4.z + q4.w * k4.w;
    }
  }
  // only the last key block can hold rows past Lk (NB = ceil(Lk / 16)): their scores become -inf, their probabilities exactly 0
#pragma unroll
  for (int j = NK - KB; j < NK; ++j) s[j] = (j < Lk) ? s[j] : -INFINITY;
  float mx = s[0];
#pragma unroll
  for (int j = 1; j < NK; ++j) mx = fmaxf(mx, s[j]);
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < NK; ++j) {
    s[j] = exp_fast(s[j] - mx);
    sum += s[j];
  }
  const float inv = post_scale / sum;
#pragma unroll
  for (int j = 0; j < NK; ++j) s[j] *= inv;
  const size_t oo = ((size_t)b * Lq + t) * E + (size_t)h * hd;
  for (int d = 0; d < hd; d += 4) {
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < NK; ++j) {
      const float4 v4 = *reinterpret_cast<const float4*>(&sV[j][d]);
      a.x += s[j] * v4.x; a.y += s[j] * v4.y; a.z += s[j] * v4.z; a.w += s[j] * v4.w;
    }
    if (o_planes) store_planes4(reinterpret_cast<bf16_t*>(O) + oo + d, o_lo_off, a);
    else *reinterpret_cast<float4*>(O + oo + d) = a;
  }
}

// Backward, the formulas of attn.hip's xattn_bwd_kernel:
//   dPs_j = c (dO . V_j);  dS_j = p_j (dPs_j - sum_j' p_j' dPs_j');  dQ = sum_j dS_j K_j
//   dK_j = sum_q dS_qj Q_q;  dV_j = sum_q c p_qj dO_q
template <int NB>
__global__ __launch_bounds__(256) void xattn_bwd_wide_kernel(const float* __restrict__ Q, const float* __restrict__ K,
                                                             const float* __restrict__ V, const float* __restrict__ dO,
                                                             float* __restrict__ dQ, float* __restrict__ dK,
                                                             float* __restrict__ dV, int planes, size_t q_lo_off,
                                                             size_t kv_lo_off, int heads, int Lq, int Lk, int hd,
                                                             float post_scale) {
  constexpr int NK = NB * KB;
  extern __shared__ __attribute__((aligned(16))) float bwd_wide_smem[];
  typedef float RowK[MAX_HD];
  typedef float RowP[KB];
  typedef float RowA[MAX_HD + 1];
  RowK* sK = reinterpret_cast<RowK*>(bwd_wide_smem);                         // [NK][MAX_HD]
  RowK* sV = sK + NK;                                                        // [NK][MAX_HD]
  RowP* sP = reinterpret_cast<RowP*>(sV + NK);                               // [256][KB]  c * p of one key block
  RowP* sS = sP + 256;                                                       // [256][KB]  dS of one key block
  RowA (*sAcc)[2 * KB] = reinterpret_cast<RowA (*)[2 * KB]>(sP);             // [2][2*KB][MAX_HD+1], over sP / sS once they are read
  static_assert(2 * 2 * KB * (MAX_HD + 1) <= 2 * 256 * KB, "sAcc must fit into sP + sS");
  const int b = blockIdx.x / heads, h = blockIdx.x % heads;
  const int E = heads * hd;
  const int t = threadIdx.x;
  load_kv<NK>(sK, sV, K, V, b, h, E, Lk, hd, t);
  __syncthreads();
  float s[NK], dp[NK];          // after the first phase: c * p and dS of this lane's query row
  if (t < Lq) {
    const size_t ro = ((size_t)b * Lq + t) * E + (size_t)h * hd;
#pragma unroll
    for (int j = 0; j < NK; ++j) { s[j] = 0.f; dp[j] = 0.f; }
    for (int d = 0; d < hd; d += 4) {
      const float4 q4 = *reinterpret_cast<const float4*>(Q + ro + d);
      const float4 g4 = *reinterpret_cast<const float4*>(dO + ro + d);
#pragma unroll
      for (int j = 0; j < NK; ++j) {
        const float4 k4 = *reinterpret_cast<const float4*>(&sK[j][d]);
        const float4 v4 = *reinterpret_cast<const float4*>(&sV[j][d]);
        s[j] += q4.x * k4.x + q4.y * k4.y + q4.z * k4.z + q4.w * k4.w;
        dp[j] += g4.x * v4.x + g4.y * v4.y + g4.z * v4.z + g4.w * v4.w;
      }
    }
    // rows past Lk (last key block only): score -inf, probability exactly 0, as in the forward
#pragma unroll
    for (int j = NK - KB; j < NK; ++j) s[j] = (j < Lk) ? s[j] : -INFINITY;
    float mx = s[0];
#pragma unroll
    for (int j = 1; j < NK; ++j) mx = fmaxf(mx, s[j]);
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < NK; ++j) {
      s[j] = exp_fast(s[j] - mx);
      sum += s[j];
    }
    const float inv = 1.0f / sum;
    float dot = 0.f;
#pragma unroll
    for (int j = 0; j < NK; ++j) {
      s[j] *= inv;                 // p_j
      dp[j] *= post_scale;         // dL/dp_j
      dot += s[j] * dp[j];
    }
#pragma unroll
    for (int j = 0; j < NK; ++j) {
      dp[j] = s[j] * (dp[j] - dot);
      s[j] *= post_scale;
    }
    for (int d = 0; d < hd; d += 4) {
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int j = 0; j < NK; ++j) {
        const float4 k4 = *reinterpret_cast<const float4*>(&sK[j][d]);
        a.x += dp[j] * k4.x; a.y += dp[j] * k4.y; a.z += dp[j] * k4.z; a.w += dp[j] * k4.w;
      }
      if (planes) store_planes4(reinterpret_cast<bf16_t*>(dQ) + ro + d, q_lo_off, a);
      else *reinterpret_cast<float4*>(dQ + ro + d) = a;
    }
  }
  // dK / dV, one key block at a time: thread <-> (column d, half of the query rows); 16 + 16 accumulators per thread
  const int d = t & 127, part = t >> 7;
  const int half = (Lq + 1) / 2;
  const int q0 = part * half;
  const int q1 = (q0 + half < Lq) ? q0 + half : Lq;
#pragma unroll
  for (int kb = 0; kb < NB; ++kb) {
    if (t < Lq) {
#pragma unroll
      for (int j4 = 0; j4 < KB; j4 += 4) {
        *reinterpret_cast<float4*>(&sS[t][j4]) = make_float4(dp[kb * KB + j4], dp[kb * KB + j4 + 1], dp[kb * KB + j4 + 2], dp[kb * KB + j4 + 3]);
        *reinterpret_cast<float4*>(&sP[t][j4]) = make_float4(s[kb * KB + j4], s[kb * KB + j4 + 1], s[kb * KB + j4 + 2], s[kb * KB + j4 + 3]);
      }
    }
    __syncthreads();
    float ak[KB], av[KB];
#pragma unroll
    for (int j = 0; j < KB; ++j) { ak[j] = 0.f; av[j] = 0.f; }
    if (d < hd) {
      for (int q = q0; q < q1; ++q) {
        const size_t ro = ((size_t)b * Lq + q) * E + (size_t)h * hd + d;
        const float x = Q[ro], y = dO[ro];
#pragma unroll
        for (int j4 = 0; j4 < KB; j4 += 4) {
          const float4 ds4 = *reinterpret_cast<const float4*>(&sS[q][j4]);
          const float4 p4 = *reinterpret_cast<const float4*>(&sP[q][j4]);
          ak[j4 + 0] += ds4.x * x; ak[j4 + 1] += ds4.y * x; ak[j4 + 2] += ds4.z * x; ak[j4 + 3] += ds4.w * x;
          av[j4 + 0] += p4.x * y; av[j4 + 1] += p4.y * y; av[j4 + 2] += p4.z * y; av[j4 + 3] += p4.w * y;
        }
      }
    }
    __syncthreads();               // every read of sS / sP is done: sAcc may take their place
    if (d < hd) {
#pragma unroll
      for (int j = 0; j < KB; ++j) {
        sAcc[part][j][d] = ak[j];
        sAcc[part][KB + j][d] = av[j];
      }
    }
    __syncthreads();
    const int nj = (Lk - kb * KB < KB) ? Lk - kb * KB : KB;      // keys of this block (>= 1: NB = ceil(Lk / 16))
    for (int idx = t; idx < nj * (hd / 4); idx += 256) {
      const int j = idx / (hd / 4), c = (idx % (hd / 4)) * 4;
      const size_t o = ((size_t)b * Lk + kb * KB + j) * E + (size_t)h * hd + c;
      float4 gk, gv;
      gk.x = sAcc[0][j][c + 0] + sAcc[1][j][c + 0]; gk.y = sAcc[0][j][c + 1] + sAcc[1][j][c + 1];
      gk.z = sAcc[0][j][c + 2] + sAcc[1][j][c + 2]; gk.w = sAcc[0][j][c + 3] + sAcc[1][j][c + 3];
      gv.x = sAcc[0][KB + j][c + 0] + sAcc[1][KB + j][c + 0]; gv.y = sAcc[0][KB + j][c + 1] + sAcc[1][KB + j][c + 1];
      gv.z = sAcc[0][KB + j][c + 2] + sAcc[1][KB + j][c + 2]; gv.w = sAcc[0][KB + j][c + 3] + sAcc[1][KB + j][c + 3];
      if (planes) {
        store_planes4(reinterpret_cast<bf16_t*>(dK) + o, kv_lo_off, gk);
        store_planes4(reinterpret_cast<bf16_t*>(dV) + o, kv_lo_off, gv);
      } else {
        *reinterpret_cast<float4*>(dK + o) = gk;
        *reinterpret_cast<float4*>(dV + o) = gv;
      }
    }
    if (kb + 1 < NB) __syncthreads();      // the next block's sS / sP go over sAcc
  }
}

uint64_t g_wide_launches[2] = {0, 0};      // accepted forward / backward calls (host-side counters: lr2_xattn_wide_launch_counts)

constexpr size_t bwd_wide_lds(int nb) { return sizeof(float) * ((size_t)2 * nb * KB * MAX_HD + 2 * 256 * KB); }

template <int NB>
int launch_bwd_wide(const float* Q, const float* K, const float* V, const float* dO, float* dQ, float* dK, float* dV, int planes,
                    size_t q_lo_off, size_t kv_lo_off, int batch, int heads, int Lq, int Lk, int hd, float post_scale, hipStream_t stream) {
  static bool attr_set = false;
  if (!attr_set) {
    if (lr2_allow_dynamic_lds(xattn_bwd_wide_kernel<NB>, bwd_wide_lds(NB), "xattn_bwd_wide")) return LR2_ERR_LAUNCH;
    attr_set = true;
  }
  LR2_LAUNCH(xattn_bwd_wide_kernel<NB>, dim3(batch * heads), dim3(256), bwd_wide_lds(NB), stream, Q, K, V, dO, dQ, dK, dV, planes,
             q_lo_off, kv_lo_off, heads, Lq, Lk, hd, post_scale);
  return 0;
}

}  // namespace

extern "C" int lr2_xattn_wide_launch_counts(uint64_t counts[2]) {
  if (!counts) return LR2_ERR_ARG;
  counts[0] = g_wide_launches[0];
  counts[1] = g_wide_launches[1];
  return 0;
}

extern "C" int lr2_xattn_fwd_wide(const void* Q, const void* K, const void* V, void* O, int o_planes, uint64_t o_lo_off, int batch,
                                  int heads, int Lq, int Lk, int head_dim, float post_scale, void* stream) {
  if (!Q || !K || !V || !O || batch <= 0 || heads <= 0) return LR2_ERR_ARG;
  if (Lq < 1 || Lq > 256 || Lk < 1 || Lk > MAX_NB * KB || head_dim < 4 || head_dim > MAX_HD || head_dim % 4 != 0) return LR2_ERR_SHAPE;
  if (misaligned(Q, 16)) return LR2_ERR_SHAPE;                                  // float4 loads (K, V: element loads into LDS)
  if (o_planes ? (misaligned(O, 8) || o_lo_off % 4) : misaligned(O, 16)) return LR2_ERR_SHAPE;   // 4 x bf16 per plane / float4
#define LR2_FWD_WIDE(NB)                                                                                                        \
  LR2_LAUNCH(xattn_fwd_wide_kernel<NB>, dim3(batch * heads), dim3(256), 0, (hipStream_t)stream, (const float*)Q, (const float*)K, \
             (const float*)V, (float*)O, o_planes, (size_t)o_lo_off, heads, Lq, Lk, head_dim, post_scale)
  switch ((Lk + KB - 1) / KB) {
    case 1: LR2_FWD_WIDE(1); break;
    case 2: LR2_FWD_WIDE(2); break;
    case 3: LR2_FWD_WIDE(3); break;
    default: LR2_FWD_WIDE(4); break;
  }
#undef LR2_FWD_WIDE
  const int rc = lr2_launch_status(__func__);
  if (rc == 0) ++g_wide_launches[0];
  return rc;
}

extern "C" int lr2_xattn_bwd_wide(const void* Q, const void* K, const void* V, const void* dO, void* dQ, void* dK, void* dV,
                                  int planes, uint64_t q_lo_off, uint64_t kv_lo_off, int batch, int heads, int Lq, int Lk,
                                  int head_dim, float post_scale, void* stream) {
  if (!Q || !K || !V || !dO || !dQ || !dK || !dV || batch <= 0 || heads <= 0) return LR2_ERR_ARG;
  if (Lq < 1 || Lq > 256 || Lk < 1 || Lk > MAX_NB * KB || head_dim < 4 || head_dim > MAX_HD || head_dim % 4 != 0) return LR2_ERR_SHAPE;
  if (misaligned(Q, 16) || misaligned(dO, 16)) return LR2_ERR_SHAPE;            // float4 loads (K, V: element loads into LDS)
  if (planes ? (misaligned(dQ, 8) || misaligned(dK, 8) || misaligned(dV, 8) || q_lo_off % 4 || kv_lo_off % 4)
             : (misaligned(dQ, 16) || misaligned(dK, 16) || misaligned(dV, 16)))
    return LR2_ERR_SHAPE;                                                       // 4 x bf16 per plane / float4 stores
#define LR2_BWD_WIDE(NB)                                                                                                             \
  launch_bwd_wide<NB>((const float*)Q, (const float*)K, (const float*)V, (const float*)dO, (float*)dQ, (float*)dK, (float*)dV, planes, \
                      (size_t)q_lo_off, (size_t)kv_lo_off, batch, heads, Lq, Lk, head_dim, post_scale, (hipStream_t)stream)
  int rc;
  switch ((Lk + KB - 1) / KB) {
    case 1: rc = LR2_BWD_WIDE(1); break;
    case 2: rc = LR2_BWD_WIDE(2); break;
    case 3: rc = LR2_BWD_WIDE(3); break;
    default: rc = LR2_BWD_WIDE(4); break;
  }
#undef LR2_BWD_WIDE
  if (rc != 0) return rc;
  rc = lr2_launch_status(__func__);
  if (rc == 0) ++g_wide_launches[1];
  return rc;
}
