// Encoder self-attention, backward (autograd of TencentPretrain MultiHeadedAttention's core, head_dim 64; forward: selfattn_fwd.hip).
// Two kernels per call -- dQ (+ the per-query statistics), then dK / dV -- in three forms: recomputing one-block (L <= 256), recomputing
// over 128-row blocks (L > 256), and streaming persistent (given the forward's output and log-sum-exp, L <= 224, >= one pair per CU).
// lr2_self_attn_plan reports which form a shape takes.
#include "selfattn_common.h"

namespace {

// ---- what the one-block and the 128-row-blocked recomputing kernels share ----
// Rows r0 .. r0 + 16 NT - 1 of one head's operands A and B (K and V, or Q and dO), both planes, into LDS, both in the K image (each is
// read as row fragments AND transposed); rows >= L are zeros.  NTHR = threads of the workgroup.
template <int NT, int NTHR>
__device__ __forceinline__ void stage_rows2(const bf16_t* __restrict__ a_hi, size_t a_lo_off, int ld_a, const bf16_t* __restrict__ b_hi,
                                            size_t b_lo_off, int ld_b, size_t row0, int col0, int r0, int L, int tid, char* sA, char* sB) {
  constexpr int LP = 16 * NT, PLANE = LP * ROW_B;
  for (int i = tid; i < LP * 8; i += NTHR) {
    const int r = i >> 3, u = i & 7;
    u32x4_t ah = {0, 0, 0, 0}, al = ah, bh = ah, bl = ah;
    if (r0 + r < L) {
      const size_t oa = (row0 + r0 + r) * (size_t)ld_a + col0 + u * 8;
      const size_t ob = (row0 + r0 + r) * (size_t)ld_b + col0 + u * 8;
      ah = *reinterpret_cast<const u32x4_t*>(a_hi + oa);
      al = *reinterpret_cast<const u32x4_t*>(a_hi + oa + a_lo_off);
      bh = *reinterpret_cast<const u32x4_t*>(b_hi + ob);
      bl = *reinterpret_cast<const u32x4_t*>(b_hi + ob + b_lo_off);
    }
    *reinterpret_cast<u32x4_t*>(sA + k_off(r, u)) = ah;
    *reinterpret_cast<u32x4_t*>(sA + PLANE + k_off(r, u)) = al;
    *reinterpret_cast<u32x4_t*>(sB + k_off(r, u)) = bh;
    *reinterpret_cast<u32x4_t*>(sB + PLANE + k_off(r, u)) = bl;
  }
}
// the additive key mask of keys k0 .. k0 + 16 NT - 1 (natural-log domain)
template <int NT, int NTHR>
__device__ __forceinline__ void stage_key_mask(const int64_t* __restrict__ seg, size_t row0, int k0, int L, int tid, float* sMask) {
  for (int j = tid; j < 16 * NT; j += NTHR) sMask[j] = (k0 + j < L) ? ((seg[row0 + k0 + j] > 0) ? 0.f : -10000.0f) : -INFINITY;
}
// lse and D of queries q0 .. q0 + 16 NT - 1 (si0 = index of the head's query 0)
template <int NT, int NTHR>
__device__ __forceinline__ void stage_lse_d(const float* __restrict__ lse, const float* __restrict__ dsum, size_t si0, int q0, int L,
                                            int tid, float* sLse, float* sD) {
  for (int j = tid; j < 16 * NT; j += NTHR) {
    sLse[j] = (q0 + j < L) ? lse[si0 + q0 + j] : INFINITY;     // padded queries: P = exp(-inf) = 0
    sD[j] = (q0 + j < L) ? dsum[si0 + q0 + j] : 0.f;
  }
}
// Rows 16t .. 16t + 15 of the staged A and B (A fragments: row 16t + (l & 15)) against this lane's x and y fragments:
// a = A_t x^T, d = B_t y^T -- S^T and dPd^T in the dQ kernels (A, B = K, V), S and dPd in the dK / dV kernels (A, B = Q, dO).
template <int NT>
__device__ __forceinline__ void s_dp_tile(const char* sA, const char* sB, int t, int lane, const bf16x8_t (&xh)[2], const bf16x8_t (&xl)[2],
                                          const bf16x8_t (&yh)[2], const bf16x8_t (&yl)[2], f32x4_t& a, f32x4_t& d) {
  constexpr int PLANE = 16 * NT * ROW_B;
  a = f32x4_t{0.f, 0.f, 0.f, 0.f};
  d = a;
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const int o = k_off(16 * t + (lane & 15), (lane >> 4) + 4 * ks);
    a = mfma3(*reinterpret_cast<const bf16x8_t*>(sA + o), *reinterpret_cast<const bf16x8_t*>(sA + PLANE + o), xh[ks], xl[ks], a);
    d = mfma3(*reinterpret_cast<const bf16x8_t*>(sB + o), *reinterpret_cast<const bf16x8_t*>(sB + PLANE + o), yh[ks], yl[ks], d);
  }
}
// (The 32-query block of the two dK / dV kernels -- s_dp_tile, P and dS from lse / D / the dropout mask, two accum_block -- is written
// out in both: as one function the compiler contracts and vectorises its fp32 arithmetic differently, and dK / dV under dropout lose
// their bit-equality with what these kernels computed before.)
// acc += E^T X over rows 32u .. 32u + 31 of the staged X (transposed reads), E = this lane's 8 values of those rows, split in hi + lo
template <int NT>
__device__ __forceinline__ void accum_block(const float (&e)[8], const char* sX, int u, int lane, f32x4_t (&acc)[4]) {
  constexpr int PLANE = 16 * NT * ROW_B;
  const int tq = (lane & 15) >> 2, tp = lane & 3;
  bf16x8_t eh, el;
  split8(e, eh, el);
  const int ra = 32 * u + 4 * (lane >> 4) + tq, rb = ra + 16;
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int unit = 2 * n + (tp >> 1), half8 = 8 * (tp & 1);
    acc[n] = mfma3(eh, el, tr_pair_k(sX, ra, rb, unit, half8), tr_pair_k(sX + PLANE, ra, rb, unit, half8), acc[n]);
  }
}

// ---- backward, part 1: dQ (+ the per-query statistics part 2 needs) -------------------------------------------------
// Same decomposition as the forward: workgroup = (sequence, head, 64 queries), K and V of the head in LDS, everything
// in the transposed layout (lane = one query, 4 keys per 16-key tile):
//   S^T = K Q^T, P = softmax;  dPd^T = V dO^T;  dP = dPd o M;  D = sum_k dP P;  dS = P (dP - D) * scale;  dQ = dS K
// (M = dropout keep / (1 - p)).  dQ goes to columns [h*64, h*64+64) of the dQKV planes matrix.
template <int NT, int NW>
__global__ __launch_bounds__(64 * NW) void self_attn_bwd_dq_kernel(const bf16_t* __restrict__ Qh, const bf16_t* __restrict__ Kh,
                                                               const bf16_t* __restrict__ Vh, size_t lo_off, int ld,
                                                               const bf16_t* __restrict__ dOh, size_t do_lo_off, int ld_do,
                                                               const int64_t* __restrict__ seg, bf16_t* __restrict__ dQh,
                                                               size_t dq_lo_off, int ld_dq, float* __restrict__ lse,
                                                               float* __restrict__ dsum, int heads, int L, float scale,
                                                               DropP dr) {
  constexpr int LP = 16 * NT;
  constexpr int PLANE = LP * ROW_B;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sK = smem;
  char* sV = smem + 2 * PLANE;        // K layout too: V is an A operand here (rows = keys, contraction over hd)
  float* sMask = reinterpret_cast<float*>(smem + 4 * PLANE);
  float* sOut = sMask + LP;
  const int h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t row0 = (size_t)b * L;
  const int col0 = h * HD;
  stage_rows2<NT, 64 * NW>(Kh, lo_off, ld, Vh, lo_off, ld, row0, col0, 0, L, tid, sK, sV);
  stage_key_mask<NT, 64 * NW>(seg, row0, 0, L, tid, sMask);
  const int qn = lane & 15, g = lane >> 4;
  __syncthreads();
  const int n_sub = (L + 15) >> 4;
  for (int sub = blockIdx.x * NW + wave; sub < n_sub; sub += gridDim.x * NW) {
  const int q_row = sub * 16 + qn;
  const bool q_ok = q_row < L;
  bf16x8_t qh[2], ql[2], gh[2], gl[2];
  load_frags(Qh, lo_off, (row0 + (q_ok ? q_row : 0)) * (size_t)ld + col0 + 8 * g, q_ok, qh, ql);
  load_frags(dOh, do_lo_off, (row0 + (q_ok ? q_row : 0)) * (size_t)ld_do + col0 + 8 * g, q_ok, gh, gl);

  f32x4_t s[NT], dp[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    s_dp_tile<NT>(sK, sV, t, lane, qh, ql, gh, gl, s[t], dp[t]);      // S^T = K Q^T, dPd^T = V dO^T
  }
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
    accum_block<NT>(e, sK, u, lane, o);                                // dQ += dS K
  }
  store_tile_planes(o, sOut + wave * 16 * (HD + 4), lane, sub * 16, L, dQh, dq_lo_off, (size_t)ld_dq,
                    row0 * (size_t)ld_dq + col0);
  }  // sub-tile loop
}

// ---- backward, part 2: dK, dV ------------------------------------------------------------------------------------------
// Workgroup = (sequence, head, 64 keys); Q and dO of the head in LDS; each wave owns 16 keys (K, V fragments in
// registers) and walks over the queries in the NON-transposed layout (lane = one key, 4 queries per 16-query tile):
//   S = Q K^T, P = exp(S - lse[q]);  dPd = dO V^T;  Pd = P o M, dP = dPd o M, dS = P (dP - D[q]) * scale
//   dV = Pd^T dO,  dK = dS^T Q       (contraction over queries: P / dS tiles reused as A fragments, Q / dO transposed reads)
template <int NT, int NW>
__global__ __launch_bounds__(64 * NW) void self_attn_bwd_dkv_kernel(const bf16_t* __restrict__ Qh, const bf16_t* __restrict__ Kh,
                                                                const bf16_t* __restrict__ Vh, size_t lo_off, int ld,
                                                                const bf16_t* __restrict__ dOh, size_t do_lo_off, int ld_do,
                                                                const int64_t* __restrict__ seg, bf16_t* __restrict__ dKh,
                                                                bf16_t* __restrict__ dVh, size_t dkv_lo_off, int ld_dkv,
                                                                const float* __restrict__ lse, const float* __restrict__ dsum,
                                                                int heads, int L, float scale, DropP dr) {
  constexpr int LP = 16 * NT;
  constexpr int PLANE = LP * ROW_B;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sQ = smem;                    // K layout: fragment reads (rows = queries) + transposed reads
  char* sG = smem + 2 * PLANE;        // dO
  float* sLse = reinterpret_cast<float*>(smem + 4 * PLANE);   // [LP]
  float* sD = sLse + LP;                                      // [LP]
  float* sOut = sD + LP;
  const int h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t row0 = (size_t)b * L;
  const int col0 = h * HD;
  stage_rows2<NT, 64 * NW>(Qh, lo_off, ld, dOh, do_lo_off, ld_do, row0, col0, 0, L, tid, sQ, sG);
  stage_lse_d<NT, 64 * NW>(lse, dsum, ((size_t)b * heads + h) * L, 0, L, tid, sLse, sD);
  const int kn = lane & 15, g = lane >> 4;
  __syncthreads();
  const int n_sub = (L + 15) >> 4;
  for (int sub = blockIdx.x * NW + wave; sub < n_sub; sub += gridDim.x * NW) {
  const int key = sub * 16 + kn;
  const bool k_ok = key < L;
  bf16x8_t kh[2], kl[2], vh[2], vl[2];
  load_frags(Kh, lo_off, (row0 + (k_ok ? key : 0)) * (size_t)ld + col0 + 8 * g, k_ok, kh, kl);
  load_frags(Vh, lo_off, (row0 + (k_ok ? key : 0)) * (size_t)ld + col0 + 8 * g, k_ok, vh, vl);
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
      s_dp_tile<NT>(sQ, sG, t, lane, kh, kl, vh, vl, a, d);      // S[query 16t + 4g + r][key kn], dPd
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
    accum_block<NT>(pd, sG, u, lane, dv);      // dV += Pd^T dO
    accum_block<NT>(ds, sQ, u, lane, dk);      // dK += dS^T Q
  }
  float* slab = sOut + wave * 16 * (HD + 4);
  store_tile_planes(dk, slab, lane, sub * 16, L, dKh, dkv_lo_off, (size_t)ld_dkv, row0 * (size_t)ld_dkv + col0);
  store_tile_planes(dv, slab, lane, sub * 16, L, dVh, dkv_lo_off, (size_t)ld_dkv, row0 * (size_t)ld_dkv + col0);
  }  // sub-tile loop
}

// ---- persistent backward (round 4): the forward's log-sum-exp and output are inputs, nothing is recomputed twice ----
// With lse[q] from the forward, P = exp(S - lse) needs no row maximum / row sum, and D[q] = sum_k dP P = sum_d dO[q, d] O[q, d] needs
// no pass over the keys: both kernels STREAM over 32-row blocks of the resident operand -- one S / dP tile pair in registers at a time
// (the one-pair kernels above hold 14 S tiles and 14 dP tiles of a sub-tile) -- which fits 16-wave workgroups at <= 128 VGPRs:
//   * wave w < n_sub owns sub-tile w (16 queries in the dQ kernel, 16 keys in the dK / dV kernel) of every pair; waves 14, 15 move data;
//   * the resident planes (K, V / Q, dO: both in the d_off layout) are refilled IN HALVES while the other half is being used: a row
//     block is dead once every wave has passed it, so after block H1 - 1 (barrier "mid") the movers load rows [0, 32 H1) of the NEXT
//     pair and after the last block (barrier "end") the rest; a mover waits for its pieces (s_waitcnt vmcnt(0)) before the NEXT barrier,
//     i.e. half a pair later; no compute wave waits for memory except for its own 16-row fragments, requested before the stores.
// Arithmetic: dQ kernel  S^T = K Q^T, dPd^T = V dO^T, P = exp(S scale + mask - lse), dS = P (dPd o M - D) scale, dQ = dS K
//             dKV kernel S = Q K^T, dPd = dO V^T, Pd = P o M, dS as above, dV = Pd^T dO, dK = dS^T Q          (M = keep / (1 - p))
// replaces: autograd of tencentpretrain/layers/multi_headed_attn.py:61-74 (as the one-pair kernels do).
// eight bf16 (one fragment) -> fp32 sum of hi + lo products with another fragment pair: sum_i (ah + al)_i (bh + bl)_i
__device__ __forceinline__ float frag_dot(bf16x8_t ah, bf16x8_t al, bf16x8_t bh, bf16x8_t bl) {
  const u32x4_t a = __builtin_bit_cast(u32x4_t, ah), c = __builtin_bit_cast(u32x4_t, al);
  const u32x4_t b = __builtin_bit_cast(u32x4_t, bh), d = __builtin_bit_cast(u32x4_t, bl);
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float x0 = __uint_as_float(a[i] << 16) + __uint_as_float(c[i] << 16);
    const float x1 = __uint_as_float(a[i] & 0xffff0000u) + __uint_as_float(c[i] & 0xffff0000u);
    const float y0 = __uint_as_float(b[i] << 16) + __uint_as_float(d[i] << 16);
    const float y1 = __uint_as_float(b[i] & 0xffff0000u) + __uint_as_float(d[i] & 0xffff0000u);
    acc = __builtin_fmaf(x0, y0, acc);
    acc = __builtin_fmaf(x1, y1, acc);
  }
  return acc;
}

struct BwdArgs {
  const bf16_t *q, *k, *v;      // hi planes (lo plane lo_off elements behind), row stride ld
  size_t lo_off;
  int ld;
  const bf16_t* go;             // dO hi plane
  size_t do_lo_off;
  int ld_do;
  const bf16_t* o;              // forward output hi plane
  size_t o_lo_off;
  int ld_o;
  const int64_t* seg;
  bf16_t *dq, *dk, *dv;
  size_t d_lo_off;
  int ld_d;
  const float* lse;             // [batch, heads, L] from the forward
  float* dsum;                  // [batch, heads, L]: written by the dQ kernel, read by the dK / dV kernel
  int heads, L, n_pairs;
  float scale;
  DropP dr;
  uint32_t qkv_bytes, do_bytes; // descriptor spans from q / k / v and from go
};

// rows [0, 32 * H1) are the first half of the resident planes
template <int NT>
struct Halves {
  static constexpr int NB = NT / 2, H1 = (NB + 1) / 2, J_MID = 4 * H1, J_END = 2 * NT;
};

template <int NT, bool DROP>
__global__ __launch_bounds__(64 * PS_WAVES) void self_attn_bwd_dq_persist_kernel(BwdArgs A) {
  constexpr int LP = 16 * NT, PLANE = LP * ROW_B, NB = Halves<NT>::NB, H1 = Halves<NT>::H1;
  constexpr int MK = (LP + 64 * PS_MOVERS - 1) / (64 * PS_MOVERS);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sK = smem;
  char* sV = smem + 2 * PLANE;        // same layout: V is an A operand here (rows = keys, contraction over hd)
  float* sMask = reinterpret_cast<float*>(smem + 4 * PLANE);          // [LP], pre-multiplied by log2(e)
  float* sOut = sMask + LP;                                          // [PS_MAX_SUB waves][16][32 + 4]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int heads = A.heads, L = A.L, n_pairs = A.n_pairs;
  const int n_sub = (L + 15) >> 4;
  int p = blockIdx.x;
  if (p >= n_pairs) return;

  if (wave >= PS_MAX_SUB) {
    // ---- movers ----
    const __amdgpu_buffer_rsrc_t k_hi = buf_rsrc(A.k, A.qkv_bytes), k_lo = buf_rsrc(A.k + A.lo_off, A.qkv_bytes);
    const __amdgpu_buffer_rsrc_t v_hi = buf_rsrc(A.v, A.qkv_bytes), v_lo = buf_rsrc(A.v + A.lo_off, A.qkv_bytes);
    const int j0 = wave - PS_MAX_SUB, mtid = tid - 64 * PS_MAX_SUB;
    const uint32_t row_bytes = (uint32_t)A.ld * 2u;
    auto pair_off = [&](int pp) { const int b = pp / heads, h = pp - b * heads; return (uint32_t)(((size_t)b * L * A.ld + h * HD) * 2); };
    auto mask_of = [&](int pp, int j) -> float {
      const int b = pp / heads;
      return j < L ? ((A.seg[(size_t)b * L + j] > 0) ? 0.f : -10000.0f * LOG2E) : -INFINITY;
    };
    dma_rows<NT, IMG_D, 2>(k_hi, k_lo, sK, lane, j0, Halves<NT>::J_END, PS_MOVERS, pair_off(p), row_bytes, L);
    dma_rows<NT, IMG_D, 2>(v_hi, v_lo, sV, lane, j0, Halves<NT>::J_END, PS_MOVERS, pair_off(p), row_bytes, L);
    for (int j = mtid; j < LP; j += 64 * PS_MOVERS) sMask[j] = mask_of(p, j);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    phase_barrier();
    for (;;) {
      const int pn = p + gridDim.x;
      const bool more = pn < n_pairs;
      phase_barrier();                                   // mid: rows [0, 32 H1) of this pair are dead
      if (more) {
        dma_rows<NT, IMG_D, 2>(k_hi, k_lo, sK, lane, j0, Halves<NT>::J_MID, PS_MOVERS, pair_off(pn), row_bytes, L);
        dma_rows<NT, IMG_D, 2>(v_hi, v_lo, sV, lane, j0, Halves<NT>::J_MID, PS_MOVERS, pair_off(pn), row_bytes, L);
        float mk[MK];
#pragma unroll
        for (int i = 0; i < MK; ++i) mk[i] = mask_of(pn, mtid + i * 64 * PS_MOVERS);
#pragma unroll
        for (int i = 0; i < MK; ++i) {
          const int j = mtid + i * 64 * PS_MOVERS;
          if (j < 32 * H1) sMask[j] = mk[i];
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      phase_barrier();                                   // end: the rest is dead
      if (!more) break;
      dma_rows<NT, IMG_D, 2>(k_hi, k_lo, sK, lane, Halves<NT>::J_MID + j0, Halves<NT>::J_END, PS_MOVERS, pair_off(pn), row_bytes, L);
      dma_rows<NT, IMG_D, 2>(v_hi, v_lo, sV, lane, Halves<NT>::J_MID + j0, Halves<NT>::J_END, PS_MOVERS, pair_off(pn), row_bytes, L);
      {
        float mk[MK];
#pragma unroll
        for (int i = 0; i < MK; ++i) mk[i] = mask_of(pn, mtid + i * 64 * PS_MOVERS);
#pragma unroll
        for (int i = 0; i < MK; ++i) {
          const int j = mtid + i * 64 * PS_MOVERS;
          if (j >= 32 * H1 && j < LP) sMask[j] = mk[i];
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      p = pn;
    }
    return;
  }
  if (wave >= n_sub) {
    // ---- nothing to compute: keep the barriers company ----
    phase_barrier();
    for (;;) {
      phase_barrier();
      phase_barrier();
      p += gridDim.x;
      if (p >= n_pairs) break;
    }
    return;
  }

  // ---- compute waves: sub-tile `wave` = 16 queries of every pair ----
  const int sub = wave;
  const int qn = lane & 15, g = lane >> 4;
  const int q_row = sub * 16 + qn;
  const bool q_ok = q_row < L;
  float* slab = sOut + wave * 16 * (32 + 4);
  const float scale = A.scale, scale2 = A.scale * LOG2E;
  const uint32_t kb[2] = {lds_addr(sK + d_off(qn, g)), lds_addr(sK + d_off(qn, g + 4))};
  const uint32_t vbk[2] = {lds_addr(sV + d_off(qn, g)), lds_addr(sV + d_off(qn, g + 4))};
  const int i16 = lane & 15, tq = i16 >> 2, tp = i16 & 3;
  uint32_t ktb[4];                                        // transposed reads of K: rows 32u + 4g + tq (+ 16)
#pragma unroll
  for (int n = 0; n < 4; ++n) ktb[n] = lds_addr(sK + d_off(4 * g + tq, 2 * n + (tp >> 1)) + 8 * (tp & 1));

  bf16x8_t qh[2], ql[2], gh[2], gl[2];
  float dD = 0.f, lse2 = 0.f;
  // this wave's rows of pair pp: Q and dO fragments, D = sum_d dO O, lse
  auto fetch = [&](int pp) {
    const int b = pp / heads, h = pp - b * heads;
    const size_t row0_ = (size_t)b * L;
    const uint32_t lr = (uint32_t)(q_ok ? q_row : 0);
    bf16x8_t oh[2], ol[2];
    load_frags_u(A.q + row0_ * (size_t)A.ld + h * HD, A.lo_off, lr * (uint32_t)A.ld + 8u * g, q_ok, qh, ql);
    load_frags_u(A.go + row0_ * (size_t)A.ld_do + h * HD, A.do_lo_off, lr * (uint32_t)A.ld_do + 8u * g, q_ok, gh, gl);
    load_frags_u(A.o + row0_ * (size_t)A.ld_o + h * HD, A.o_lo_off, lr * (uint32_t)A.ld_o + 8u * g, q_ok, oh, ol);
    const size_t si0 = (size_t)pp * L;
    lse2 = q_ok ? A.lse[si0 + lr] * LOG2E : 0.f;
    float d = frag_dot(gh[0], gl[0], oh[0], ol[0]) + frag_dot(gh[1], gl[1], oh[1], ol[1]);
    d += __shfl_xor(d, 16, 64);
    d += __shfl_xor(d, 32, 64);
    dD = d;
    if (g == 0 && q_ok) A.dsum[si0 + lr] = d;
  };
  fetch(p);
  phase_barrier();
  for (;;) {
    const int b = p / heads, h = p - b * heads;
    const size_t row0 = (size_t)b * L;
    const uint64_t drow = (((uint64_t)b * heads + h) * L + (uint64_t)(q_ok ? q_row : 0)) * mask_pitch(L);
    f32x4_t o[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) o[n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      if (u == H1) phase_barrier();                      // mid
      float e[8];
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int t = 2 * u + half;
        f32x4_t a = {0.f, 0.f, 0.f, 0.f}, d = a;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          a = mfma3(lds_ld16(kb[ks] + 2048 * t), lds_ld16(kb[ks] + 2048 * t + PLANE), qh[ks], ql[ks], a);
          d = mfma3(lds_ld16(vbk[ks] + 2048 * t), lds_ld16(vbk[ks] + 2048 * t + PLANE), gh[ks], gl[ks], d);
        }
        const float4 mk = *reinterpret_cast<const float4*>(sMask + 16 * t + 4 * g);
        const float mkv[4] = {mk.x, mk.y, mk.z, mk.w};
        if (DROP && A.dr.thr) d = drop_mul4v(A.dr, drow + 16 * t + 4 * g, d);      // dP = dPd o M
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pr = __builtin_amdgcn_exp2f(__builtin_fmaf(a[r], scale2, mkv[r] - lse2));
          e[4 * half + r] = pr * (d[r] - dD) * scale;
        }
      }
      bf16x8_t eh, el;
      split8(e, eh, el);
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const uint32_t ad = ktb[n] + 4096 * u;
        o[n] = mfma3(eh, el, lds_tr_pair(ad, ad + 2048), lds_tr_pair(ad + PLANE, ad + 2048 + PLANE), o[n]);
      }
    }
    const int pn = p + gridDim.x;
    const bool more = pn < n_pairs;
    if (more) fetch(pn);                                 // the next pair's rows travel under the stores and the barrier
    store_tile_planes_half(o, slab, lane, sub * 16, L, A.dq, A.d_lo_off, (size_t)A.ld_d, row0 * (size_t)A.ld_d + h * HD);
    phase_barrier();                                     // end
    if (!more) break;
    p = pn;
  }
}

template <int NT, bool DROP>
__global__ __launch_bounds__(64 * PS_WAVES) void self_attn_bwd_dkv_persist_kernel(BwdArgs A) {
  constexpr int LP = 16 * NT, PLANE = LP * ROW_B, NB = Halves<NT>::NB, H1 = Halves<NT>::H1;
  constexpr int MK = (LP + 64 * PS_MOVERS - 1) / (64 * PS_MOVERS);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sQ = smem;                    // d_off layout: fragment reads (rows = queries) + transposed reads
  char* sG = smem + 2 * PLANE;        // dO
  float* sLse = reinterpret_cast<float*>(smem + 4 * PLANE);   // [LP] lse * log2(e); +inf for padded queries (P = 0)
  float* sD = sLse + LP;                                      // [LP]
  float* sOut = sD + LP;                                      // [PS_MAX_SUB waves][16][32 + 4]
  // DROP: the pair's dropout decisions, one byte per (sub-tile, 32-query block, lane) = the 8 (query, key) elements that lane owns in
  // that block, written by the mover waves one pair ahead (two buffers): the hashes cost the compute waves nothing -- neither issue
  // slots nor the registers their temporaries would need beside the fragments
  constexpr int KEEP_BYTES = PS_MAX_SUB * NB * 64;
  uint8_t* sKeep = reinterpret_cast<uint8_t*>(sOut + PS_MAX_SUB * 16 * (32 + 4));      // [2][KEEP_BYTES]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int heads = A.heads, L = A.L, n_pairs = A.n_pairs;
  const int n_sub = (L + 15) >> 4;
  int p = blockIdx.x;
  if (p >= n_pairs) return;

  if (wave >= PS_MAX_SUB) {
    // ---- movers ----
    const __amdgpu_buffer_rsrc_t q_hi = buf_rsrc(A.q, A.qkv_bytes), q_lo = buf_rsrc(A.q + A.lo_off, A.qkv_bytes);
    const __amdgpu_buffer_rsrc_t g_hi = buf_rsrc(A.go, A.do_bytes), g_lo = buf_rsrc(A.go + A.do_lo_off, A.do_bytes);
    const int j0 = wave - PS_MAX_SUB, mtid = tid - 64 * PS_MAX_SUB;
    const uint32_t q_row_bytes = (uint32_t)A.ld * 2u, g_row_bytes = (uint32_t)A.ld_do * 2u;
    auto q_off = [&](int pp) { const int b = pp / heads, h = pp - b * heads; return (uint32_t)(((size_t)b * L * A.ld + h * HD) * 2); };
    auto g_off = [&](int pp) { const int b = pp / heads, h = pp - b * heads; return (uint32_t)(((size_t)b * L * A.ld_do + h * HD) * 2); };
    // element index of (query q, key) of pair pp = pp L pitch + q pitch + key: pp L pitch is a multiple of 4 and the hash reads the low
    // 32 bits of (index >> 1) only, so everything per lane is 32-bit arithmetic (the same decisions as dropout_keep on the 64-bit index)
    auto write_keep = [&](int pp, uint8_t* dst) {
      const uint32_t pitch32 = (uint32_t)mask_pitch(L);
      const uint32_t pair_half32 = (uint32_t)(((uint64_t)pp * (uint64_t)L * mask_pitch(L)) >> 1);
      for (int i = mtid; i < n_sub * NB * 64; i += 64 * PS_MOVERS) {
        const int sub_ = i / (NB * 64), rem = i - sub_ * (NB * 64), u = rem >> 6, ln = rem & 63;
        const int key_ = sub_ * 16 + (ln & 15);
        const uint32_t col = (uint32_t)(key_ < L ? key_ : 0);
        uint32_t keep = 0;
#pragma unroll
        for (int e8 = 0; e8 < 8; ++e8) {
          const int q = 32 * u + 16 * (e8 >> 2) + 4 * (ln >> 4) + (e8 & 3);
          const uint32_t x = (uint32_t)(q < L ? q : 0) * pitch32 + col;
          const uint32_t hsh = dropout_hash(A.dr.key, (uint64_t)(pair_half32 + (x >> 1)));
          keep |= (uint32_t)(((x & 1) ? (hsh >> 16) : (hsh & 0xffffu)) >= A.dr.thr) << e8;
        }
        dst[i] = (uint8_t)keep;
      }
    };
    dma_rows<NT, IMG_D, 2>(q_hi, q_lo, sQ, lane, j0, Halves<NT>::J_END, PS_MOVERS, q_off(p), q_row_bytes, L);
    dma_rows<NT, IMG_D, 2>(g_hi, g_lo, sG, lane, j0, Halves<NT>::J_END, PS_MOVERS, g_off(p), g_row_bytes, L);
    if (DROP && A.dr.thr) write_keep(p, sKeep);
    for (int j = mtid; j < LP; j += 64 * PS_MOVERS) {
      const size_t si = (size_t)p * L + j;
      sLse[j] = j < L ? A.lse[si] * LOG2E : INFINITY;
      sD[j] = j < L ? A.dsum[si] : 0.f;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    phase_barrier();
    for (int it = 0;; ++it) {
      const int pn = p + gridDim.x;
      const bool more = pn < n_pairs;
      phase_barrier();                                   // mid
      if (more) {
        dma_rows<NT, IMG_D, 2>(q_hi, q_lo, sQ, lane, j0, Halves<NT>::J_MID, PS_MOVERS, q_off(pn), q_row_bytes, L);
        dma_rows<NT, IMG_D, 2>(g_hi, g_lo, sG, lane, j0, Halves<NT>::J_MID, PS_MOVERS, g_off(pn), g_row_bytes, L);
        if (DROP && A.dr.thr) write_keep(pn, sKeep + ((it + 1) & 1) * KEEP_BYTES);     // that buffer's readers finished a pair ago
        float l2[MK], dd[MK];
#pragma unroll
        for (int i = 0; i < MK; ++i) {
          const int j = mtid + i * 64 * PS_MOVERS;
          const size_t si = (size_t)pn * L + (j < L ? j : 0);
          l2[i] = j < L ? A.lse[si] * LOG2E : INFINITY;
          dd[i] = j < L ? A.dsum[si] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < MK; ++i) {
          const int j = mtid + i * 64 * PS_MOVERS;
          if (j < 32 * H1) { sLse[j] = l2[i]; sD[j] = dd[i]; }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      phase_barrier();                                   // end
      if (!more) break;
      dma_rows<NT, IMG_D, 2>(q_hi, q_lo, sQ, lane, Halves<NT>::J_MID + j0, Halves<NT>::J_END, PS_MOVERS, q_off(pn), q_row_bytes, L);
      dma_rows<NT, IMG_D, 2>(g_hi, g_lo, sG, lane, Halves<NT>::J_MID + j0, Halves<NT>::J_END, PS_MOVERS, g_off(pn), g_row_bytes, L);
      {
        float l2[MK], dd[MK];
#pragma unroll
        for (int i = 0; i < MK; ++i) {
          const int j = mtid + i * 64 * PS_MOVERS;
          const size_t si = (size_t)pn * L + (j < L ? j : 0);
          l2[i] = j < L ? A.lse[si] * LOG2E : INFINITY;
          dd[i] = j < L ? A.dsum[si] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < MK; ++i) {
          const int j = mtid + i * 64 * PS_MOVERS;
          if (j >= 32 * H1 && j < LP) { sLse[j] = l2[i]; sD[j] = dd[i]; }
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      p = pn;
    }
    return;
  }
  if (wave >= n_sub) {
    phase_barrier();
    for (;;) {
      phase_barrier();
      phase_barrier();
      p += gridDim.x;
      if (p >= n_pairs) break;
    }
    return;
  }

  // ---- compute waves: sub-tile `wave` = 16 keys of every pair ----
  const int sub = wave;
  const int kn = lane & 15, g = lane >> 4;
  const int key = sub * 16 + kn;
  const bool k_ok = key < L;
  float* slab = sOut + wave * 16 * (32 + 4);
  const float scale = A.scale, scale2 = A.scale * LOG2E;
  // fragment / transposed-read bases into sQ; the same row of sG is 2 * PLANE bytes further (added to the block's scalar offset)
  const uint32_t qb[2] = {lds_addr(sQ + d_off(kn, g)), lds_addr(sQ + d_off(kn, g + 4))};
  const uint32_t sq0 = lds_addr(sQ);
  bf16x8_t kh[2], kl[2], vh[2], vl[2];
  float kmask2 = 0.f;
  auto fetch = [&](int pp) {
    const int b = pp / heads, h = pp - b * heads;
    const size_t row0_ = (size_t)b * L;
    const int lane_ = opaque(lane);                       // addresses re-derived per pair, not kept live across the block loops
    const int key_ = sub * 16 + (lane_ & 15);
    const bool ok_ = key_ < L;
    const uint32_t lr = (uint32_t)(ok_ ? key_ : 0), lo8 = 8u * (uint32_t)(lane_ >> 4);
    load_frags_u(A.k + row0_ * (size_t)A.ld + h * HD, A.lo_off, lr * (uint32_t)A.ld + lo8, ok_, kh, kl);
    load_frags_u(A.v + row0_ * (size_t)A.ld + h * HD, A.lo_off, lr * (uint32_t)A.ld + lo8, ok_, vh, vl);
    kmask2 = ok_ ? ((A.seg[row0_ + lr] > 0) ? 0.f : -10000.0f * LOG2E) : -INFINITY;
  };
  fetch(p);
  phase_barrier();
  for (int it = 0;; ++it) {
    const int b = p / heads, h = p - b * heads;
    const size_t row0 = (size_t)b * L;
    const uint8_t* keep_buf = sKeep + (it & 1) * KEEP_BYTES;
    f32x4_t dv[4], dk[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) dv[n] = dk[n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    // one 32-query block: rolled loops (an unrolled pair lets the scheduler hoist seven blocks' worth of hashes and fragments)
    auto block = [&](int u) {
      const uint32_t uo = 4096u * (uint32_t)u, ug = uo + 2u * PLANE;          // block offsets into sQ / sG (uniform)
      // the block's 8 dropout decisions: one byte the mover waves left in LDS
      uint32_t keep = 0xffu;
      if (DROP && A.dr.thr) keep = keep_buf[(sub * NB + u) * 64 + opaque(lane)];
      float pd[8], ds[8];
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        f32x4_t a = {0.f, 0.f, 0.f, 0.f}, d = a;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const uint32_t aq = qb[ks] + uo + 2048 * half, ag = qb[ks] + ug + 2048 * half;
          a = mfma3(lds_ld16(aq), lds_ld16(aq + PLANE), kh[ks], kl[ks], a);   // S[query 32u + 16 half + 4g + r][key kn]
          d = mfma3(lds_ld16(ag), lds_ld16(ag + PLANE), vh[ks], vl[ks], d);   // dPd
        }
        const float4 ls = *reinterpret_cast<const float4*>(sLse + 32 * u + 16 * half + 4 * g);
        const float4 dd = *reinterpret_cast<const float4*>(sD + 32 * u + 16 * half + 4 * g);
        const float lsv[4] = {ls.x, ls.y, ls.z, ls.w}, ddv[4] = {dd.x, dd.y, dd.z, dd.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pr = __builtin_amdgcn_exp2f(__builtin_fmaf(a[r], scale2, kmask2 - lsv[r]));
          const float m = (DROP && A.dr.thr) ? (((keep >> (4 * half + r)) & 1u) ? A.dr.inv_keep : 0.0f) : 1.0f;
          pd[4 * half + r] = pr * m;
          ds[4 * half + r] = pr * (d[r] * m - ddv[r]) * scale;
        }
      }
      // transposed-read bases, re-derived per block from the lane number (a dozen integer instructions against four registers held
      // live across both loops): row 4g + tq of the block, 16-B unit 2n + (tp >> 1), 8-B half tp & 1
      uint32_t qtb[4];
      {
        const int lane_ = opaque(lane);
        const int tq = (lane_ >> 2) & 3, tp = lane_ & 3, rr = 4 * (lane_ >> 4) + tq;
#pragma unroll
        for (int n = 0; n < 4; ++n) qtb[n] = sq0 + (uint32_t)(d_off(rr, 2 * n + (tp >> 1)) + 8 * (tp & 1));
      }
      {
        bf16x8_t ph, pl;
        split8(pd, ph, pl);
#pragma unroll
        for (int n = 0; n < 4; ++n) {
          const uint32_t ag = qtb[n] + ug;
          dv[n] = mfma3(ph, pl, lds_tr_pair(ag, ag + 2048), lds_tr_pair(ag + PLANE, ag + 2048 + PLANE), dv[n]);
        }
      }
      {
        bf16x8_t eh, el;
        split8(ds, eh, el);
#pragma unroll
        for (int n = 0; n < 4; ++n) {
          const uint32_t aq = qtb[n] + uo;
          dk[n] = mfma3(eh, el, lds_tr_pair(aq, aq + 2048), lds_tr_pair(aq + PLANE, aq + 2048 + PLANE), dk[n]);
        }
      }
    };
#pragma unroll 1
    for (int u = 0; u < H1; ++u) block(u);
    phase_barrier();                                     // mid
#pragma unroll 1
    for (int u = H1; u < NB; ++u) block(u);
    const int pn = p + gridDim.x;
    const bool more = pn < n_pairs;
    if (more) fetch(pn);
    const size_t base = row0 * (size_t)A.ld_d + h * HD;
    store_tile_planes_half(dk, slab, opaque(lane), sub * 16, L, A.dk, A.d_lo_off, (size_t)A.ld_d, base);
    store_tile_planes_half(dv, slab, opaque(lane), sub * 16, L, A.dv, A.d_lo_off, (size_t)A.ld_d, base);
    phase_barrier();                                     // end
    if (!more) break;
    p = pn;
  }
}

// ---- backward for sequences beyond one LDS-resident block (L > 256): the same two kernels with a block loop ---------------
// dQ: the keys are walked in blocks of LPB = 16*NT, TWICE.  Sweep 1 keeps, per query, the running maximum m, the sum
// l = sum_k exp(s_k - m) and a = sum_k exp(s_k - m) dP_k (rescaled like the forward's accumulator when m grows), which give
// lse = m + log l and D = sum_k P_k dP_k = a / l without a second statistic pass; sweep 2 recomputes S and dP per block, forms
// dS = P (dP - D) * scale and accumulates dQ = dS K.  Five matrix products per (query, key) pair instead of three.
template <int NT>
__global__ __launch_bounds__(256) void self_attn_bwd_dq_blocked_kernel(
    const bf16_t* __restrict__ Qh, const bf16_t* __restrict__ Kh, const bf16_t* __restrict__ Vh, size_t lo_off, int ld,
    const bf16_t* __restrict__ dOh, size_t do_lo_off, int ld_do, const int64_t* __restrict__ seg, bf16_t* __restrict__ dQh,
    size_t dq_lo_off, int ld_dq, float* __restrict__ lse, float* __restrict__ dsum, int heads, int L, float scale, DropP dr) {
  constexpr int LPB = 16 * NT;
  constexpr int PLANE = LPB * ROW_B;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sK = smem;
  char* sV = smem + 2 * PLANE;        // K layout (V is an A operand here)
  float* sMask = reinterpret_cast<float*>(smem + 4 * PLANE);
  float* sOut = sMask + LPB;
  const int h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t row0 = (size_t)b * L;
  const int col0 = h * HD;
  const int qn = lane & 15, g = lane >> 4;
  const int sub = blockIdx.x * 4 + wave;             // one 16-query sub-tile per wave (waves past the end idle through the barriers)
  const int q_row = sub * 16 + qn;
  const bool q_ok = q_row < L;
  bf16x8_t qh[2], ql[2], gh[2], gl[2];
  load_frags(Qh, lo_off, (row0 + (q_ok ? q_row : 0)) * (size_t)ld + col0 + 8 * g, q_ok, qh, ql);
  load_frags(dOh, do_lo_off, (row0 + (q_ok ? q_row : 0)) * (size_t)ld_do + col0 + 8 * g, q_ok, gh, gl);
  const uint64_t drow = (((uint64_t)b * heads + h) * L + (uint64_t)(q_ok ? q_row : 0)) * mask_pitch(L);

  float m = -INFINITY, l = 0.f, a = 0.f, lse_q = 0.f, dd = 0.f;
  f32x4_t o[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) o[n] = f32x4_t{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
  for (int sweep = 0; sweep < 2; ++sweep) {
#pragma unroll 1
    for (int k0 = 0; k0 < L; k0 += LPB) {
      __syncthreads();                               // the previous block's readers are done
      stage_rows2<NT, 256>(Kh, lo_off, ld, Vh, lo_off, ld, row0, col0, k0, L, tid, sK, sV);
      stage_key_mask<NT, 256>(seg, row0, k0, L, tid, sMask);
      __syncthreads();

      f32x4_t s[NT], dp[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        f32x4_t sa, d;
        s_dp_tile<NT>(sK, sV, t, lane, qh, ql, gh, gl, sa, d);
        const float4 mk = *reinterpret_cast<const float4*>(sMask + 16 * t + 4 * g);
        sa[0] = sa[0] * scale + mk.x;
        sa[1] = sa[1] * scale + mk.y;
        sa[2] = sa[2] * scale + mk.z;
        sa[3] = sa[3] * scale + mk.w;
        // dP = dPd o M (keys past L: P is 0 there, whatever the mask says)
        if (dr.thr) d = drop_mul4v(dr, drow + (uint64_t)(k0 + 16 * t + 4 * g), d);
        s[t] = sa;
        dp[t] = d;
      }
      if (sweep == 0) {
        float bm = -INFINITY;
#pragma unroll
        for (int t = 0; t < NT; ++t) bm = fmaxf(fmaxf(bm, fmaxf(s[t][0], s[t][1])), fmaxf(s[t][2], s[t][3]));
        bm = fmaxf(bm, __shfl_xor(bm, 16, 64));
        bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
        const float m_new = fmaxf(m, bm);              // finite: every block holds at least one real key
        const float corr = exp_fast(m - m_new);        // 0 on the first block (m = -inf)
        l *= corr;
        a *= corr;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float e = exp_fast(s[t][r] - m_new);
            l += e;
            a = __builtin_fmaf(e, dp[t][r], a);
          }
        m = m_new;
      } else {
#pragma unroll
        for (int u = 0; u < NT / 2; ++u) {
          float e[8];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            e[r] = exp_fast(s[2 * u][r] - lse_q) * (dp[2 * u][r] - dd) * scale;
            e[4 + r] = exp_fast(s[2 * u + 1][r] - lse_q) * (dp[2 * u + 1][r] - dd) * scale;
          }
          accum_block<NT>(e, sK, u, lane, o);                          // dQ += dS K
        }
      }
    }
    if (sweep == 0) {                                  // per-query statistics (lanes of one query hold disjoint key subsets)
      l += __shfl_xor(l, 16, 64);
      l += __shfl_xor(l, 32, 64);
      a += __shfl_xor(a, 16, 64);
      a += __shfl_xor(a, 32, 64);
      lse_q = m + logf(l);
      dd = a / l;
      if (g == 0 && q_ok) {
        const size_t si = ((size_t)b * heads + h) * L + q_row;
        lse[si] = lse_q;
        dsum[si] = dd;
      }
    }
  }
  if (sub * 16 < L)
    store_tile_planes(o, sOut + wave * 16 * (HD + 4), lane, sub * 16, L, dQh, dq_lo_off, (size_t)ld_dq, row0 * (size_t)ld_dq + col0);
}

// dK, dV: each wave keeps its 16 keys' K / V fragments and accumulators while the queries (Q, dO, lse, D) pass through LDS in
// blocks of LPB.
template <int NT>
__global__ __launch_bounds__(256) void self_attn_bwd_dkv_blocked_kernel(
    const bf16_t* __restrict__ Qh, const bf16_t* __restrict__ Kh, const bf16_t* __restrict__ Vh, size_t lo_off, int ld,
    const bf16_t* __restrict__ dOh, size_t do_lo_off, int ld_do, const int64_t* __restrict__ seg, bf16_t* __restrict__ dKh,
    bf16_t* __restrict__ dVh, size_t dkv_lo_off, int ld_dkv, const float* __restrict__ lse, const float* __restrict__ dsum,
    int heads, int L, float scale, DropP dr) {
  constexpr int LPB = 16 * NT;
  constexpr int PLANE = LPB * ROW_B;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sQ = smem;
  char* sG = smem + 2 * PLANE;
  float* sLse = reinterpret_cast<float*>(smem + 4 * PLANE);
  float* sD = sLse + LPB;
  float* sOut = sD + LPB;
  const int h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t row0 = (size_t)b * L;
  const int col0 = h * HD;
  const int kn = lane & 15, g = lane >> 4;
  const int sub = blockIdx.x * 4 + wave;
  const int key = sub * 16 + kn;
  const bool k_ok = key < L;
  bf16x8_t kh[2], kl[2], vh[2], vl[2];
  load_frags(Kh, lo_off, (row0 + (k_ok ? key : 0)) * (size_t)ld + col0 + 8 * g, k_ok, kh, kl);
  load_frags(Vh, lo_off, (row0 + (k_ok ? key : 0)) * (size_t)ld + col0 + 8 * g, k_ok, vh, vl);
  const float kmask = k_ok ? ((seg[row0 + key] > 0) ? 0.f : -10000.0f) : -INFINITY;
  f32x4_t dv[4], dk[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) dv[n] = dk[n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const uint64_t dbase = ((uint64_t)b * heads + h) * (uint64_t)L;
#pragma unroll 1
  for (int q0 = 0; q0 < L; q0 += LPB) {
    __syncthreads();
    stage_rows2<NT, 256>(Qh, lo_off, ld, dOh, do_lo_off, ld_do, row0, col0, q0, L, tid, sQ, sG);
    stage_lse_d<NT, 256>(lse, dsum, ((size_t)b * heads + h) * L, q0, L, tid, sLse, sD);
    __syncthreads();
#pragma unroll 1
    for (int u = 0; u < NT / 2; ++u) {
      float pd[8], ds[8];
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int t = 2 * u + half;
        f32x4_t a, d;
        s_dp_tile<NT>(sQ, sG, t, lane, kh, kl, vh, vl, a, d);      // S[query 16t + 4g + r][key kn], dPd
        const float4 ls = *reinterpret_cast<const float4*>(sLse + 16 * t + 4 * g);
        const float4 dd = *reinterpret_cast<const float4*>(sD + 16 * t + 4 * g);
        const float lsv[4] = {ls.x, ls.y, ls.z, ls.w}, ddv[4] = {dd.x, dd.y, dd.z, dd.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = exp_fast(a[r] * scale + kmask - lsv[r]);
          float m = 1.0f;
          if (dr.thr) {
            const int q = q0 + 16 * t + 4 * g + r;
            m = drop_mul(dr, (dbase + (uint64_t)(q < L ? q : 0)) * mask_pitch(L) + (uint64_t)(k_ok ? key : 0));
          }
          pd[4 * half + r] = p * m;
          ds[4 * half + r] = p * (d[r] * m - ddv[r]) * scale;
        }
      }
      accum_block<NT>(pd, sG, u, lane, dv);      // dV += Pd^T dO
      accum_block<NT>(ds, sQ, u, lane, dk);      // dK += dS^T Q
    }
  }
  if (sub * 16 < L) {
    float* slab = sOut + wave * 16 * (HD + 4);
    store_tile_planes(dk, slab, lane, sub * 16, L, dKh, dkv_lo_off, (size_t)ld_dkv, row0 * (size_t)ld_dkv + col0);
    store_tile_planes(dv, slab, lane, sub * 16, L, dVh, dkv_lo_off, (size_t)ld_dkv, row0 * (size_t)ld_dkv + col0);
  }
}

template <int NT>
int launch_bwd_persist(const AttnArgs& a, const bf16_t* go, size_t do_lo_off, int ld_do, const bf16_t* o, size_t o_lo_off, int ld_o,
                       bf16_t* dq, bf16_t* dk, bf16_t* dv, size_t d_lo_off, int ld_d, const float* lse, float* dsum) {
  constexpr int LP = 16 * NT;
  const size_t lds1 = (size_t)4 * LP * ROW_B + (size_t)LP * 4 + (size_t)PS_MAX_SUB * 16 * (32 + 4) * 4;
  const size_t lds2 = (size_t)4 * LP * ROW_B + (size_t)LP * 8 + (size_t)PS_MAX_SUB * 16 * (32 + 4) * 4;
  const size_t lds2_drop = lds2 + (size_t)2 * PS_MAX_SUB * (NT / 2) * 64;       // + the dropout decision bytes of two pairs
  static bool done_dq[2] = {false, false}, done_dkv[2] = {false, false};
  static const char* const WHAT_DQ[2] = {"lr2_self_attn_bwd(dq, persistent)", "lr2_self_attn_bwd(dq, persistent, dropout)"};
  static const char* const WHAT_DKV[2] = {"lr2_self_attn_bwd(dkv, persistent)", "lr2_self_attn_bwd(dkv, persistent, dropout)"};
  BwdArgs A{};
  A.q = a.q; A.k = a.k; A.v = a.v; A.lo_off = a.lo_off; A.ld = a.ld;
  A.go = go; A.do_lo_off = do_lo_off; A.ld_do = ld_do;
  A.o = o; A.o_lo_off = o_lo_off; A.ld_o = ld_o;
  A.seg = a.seg; A.dq = dq; A.dk = dk; A.dv = dv; A.d_lo_off = d_lo_off; A.ld_d = ld_d;
  A.lse = lse; A.dsum = dsum; A.heads = a.heads; A.L = a.L; A.n_pairs = a.batch * a.heads; A.scale = a.scale; A.dr = a.dr;
  A.qkv_bytes = (uint32_t)operand_span_bytes(a.batch, a.L, a.ld, a.heads);
  A.do_bytes = (uint32_t)operand_span_bytes(a.batch, a.L, ld_do, a.heads);
  const bool drop = a.dr.thr != 0;
  const int grid = persist_grid(A.n_pairs);
  if (launch_drop_form(drop, self_attn_bwd_dq_persist_kernel<NT, false>, self_attn_bwd_dq_persist_kernel<NT, true>, lds1, lds1, done_dq,
                       WHAT_DQ, grid, a.stream, A))
    return LR2_ERR_LAUNCH;      // (the dK / dV kernel's LDS is allowed after the dQ launch, on the first call: host work only)
  return launch_drop_form(drop, self_attn_bwd_dkv_persist_kernel<NT, false>, self_attn_bwd_dkv_persist_kernel<NT, true>, lds2, lds2_drop,
                          done_dkv, WHAT_DKV, grid, a.stream, A);
}

template <int NT>
int launch_bwd(const AttnArgs& a, const bf16_t* go, size_t do_lo_off, int ld_do, bf16_t* dq, bf16_t* dk, bf16_t* dv,
               size_t d_lo_off, int ld_d, float* lse, float* dsum) {
  constexpr int LP = 16 * NT;
  constexpr int NW = NT <= 14 ? 8 : 4;          // two waves per SIMD where the K / V (Q / dO) planes + 8 output slabs fit the LDS
  const size_t lds1 = (size_t)4 * LP * ROW_B + (size_t)LP * 4 + (size_t)NW * 16 * (HD + 4) * 4;
  const size_t lds2 = (size_t)4 * LP * ROW_B + (size_t)LP * 8 + (size_t)NW * 16 * (HD + 4) * 4;
  static bool done1 = false, done2 = false;
  if (allow_lds_once(self_attn_bwd_dq_kernel<NT, NW>, lds1, done1, "self_attn_bwd_dq")) return LR2_ERR_LAUNCH;
  if (allow_lds_once(self_attn_bwd_dkv_kernel<NT, NW>, lds2, done2, "self_attn_bwd_dkv")) return LR2_ERR_LAUNCH;
  const int n_sub = (a.L + 15) / 16, max_chunks = (n_sub + NW - 1) / NW;
  int chunks = attn_chunks(a.batch, a.heads, a.L);
  if (chunks > max_chunks) chunks = max_chunks;
  const dim3 grid(chunks, a.heads, a.batch);
  LR2_LAUNCH((self_attn_bwd_dq_kernel<NT, NW>), grid, dim3(64 * NW), lds1, a.stream, a.q, a.k, a.v, a.lo_off, a.ld, go, do_lo_off,
             ld_do, a.seg, dq, d_lo_off, ld_d, lse, dsum, a.heads, a.L, a.scale, a.dr);
  if (lr2_launch_status("lr2_self_attn_bwd(dq)")) return LR2_ERR_LAUNCH;
  LR2_LAUNCH((self_attn_bwd_dkv_kernel<NT, NW>), grid, dim3(64 * NW), lds2, a.stream, a.q, a.k, a.v, a.lo_off, a.ld, go, do_lo_off,
             ld_do, a.seg, dk, dv, d_lo_off, ld_d, (const float*)lse, (const float*)dsum, a.heads, a.L, a.scale, a.dr);
  return lr2_launch_status("lr2_self_attn_bwd(dkv)");
}

// L > 256: query / key blocks of 128 rows through 64 KiB of LDS (two workgroups per CU)
int launch_bwd_blocked(const AttnArgs& a, const bf16_t* go, size_t do_lo_off, int ld_do, bf16_t* dq, bf16_t* dk, bf16_t* dv,
                       size_t d_lo_off, int ld_d, float* lse, float* dsum) {
  constexpr int NT = 8, LPB = 16 * NT;
  const size_t lds1 = (size_t)4 * LPB * ROW_B + (size_t)LPB * 4 + (size_t)4 * 16 * (HD + 4) * 4;
  const size_t lds2 = (size_t)4 * LPB * ROW_B + (size_t)LPB * 8 + (size_t)4 * 16 * (HD + 4) * 4;
  static bool done1 = false, done2 = false;
  if (allow_lds_once(self_attn_bwd_dq_blocked_kernel<NT>, lds1, done1, "self_attn_bwd_dq_blocked")) return LR2_ERR_LAUNCH;
  if (allow_lds_once(self_attn_bwd_dkv_blocked_kernel<NT>, lds2, done2, "self_attn_bwd_dkv_blocked")) return LR2_ERR_LAUNCH;
  const int n_sub = (a.L + 15) / 16;
  const dim3 grid((n_sub + 3) / 4, a.heads, a.batch);
  LR2_LAUNCH(self_attn_bwd_dq_blocked_kernel<NT>, grid, dim3(256), lds1, a.stream, a.q, a.k, a.v, a.lo_off, a.ld, go, do_lo_off,
             ld_do, a.seg, dq, d_lo_off, ld_d, lse, dsum, a.heads, a.L, a.scale, a.dr);
  if (lr2_launch_status("lr2_self_attn_bwd(dq, blocked)")) return LR2_ERR_LAUNCH;
  LR2_LAUNCH(self_attn_bwd_dkv_blocked_kernel<NT>, grid, dim3(256), lds2, a.stream, a.q, a.k, a.v, a.lo_off, a.ld, go, do_lo_off,
             ld_do, a.seg, dk, dv, d_lo_off, ld_d, (const float*)lse, (const float*)dsum, a.heads, a.L, a.scale, a.dr);
  return lr2_launch_status("lr2_self_attn_bwd(dkv, blocked)");
}

}  // namespace

#define LR2_SA_DISPATCH(L, CALL)  \
  if ((L) <= 64) return CALL(4);  \
  if ((L) <= 128) return CALL(8); \
  if ((L) <= 224) return CALL(14); \
  return CALL(16);

extern "C" int lr2_self_attn_bwd(const void* q_hi, const void* k_hi, const void* v_hi, uint64_t lo_off, int ld,
                                 const void* do_hi, uint64_t do_lo_off, int ld_do, const int64_t* seg, void* dq_hi, void* dk_hi,
                                 void* dv_hi, uint64_t d_lo_off, int ld_d, const void* o_hi, uint64_t o_lo_off, int ld_o,
                                 void* lse_ws, void* dsum_ws, float drop_p, uint64_t drop_seed, uint32_t drop_site, int batch,
                                 int heads, int L, int head_dim, float scale, void* stream) {
  if (!q_hi || !k_hi || !v_hi || !do_hi || !seg || !dq_hi || !dk_hi || !dv_hi || !lse_ws || !dsum_ws || batch <= 0 || heads <= 0)
    return LR2_ERR_ARG;
  if (head_dim != HD || L < 1 || ld % 8 || ld_do % 8 || ld_d % 8 || lo_off % 8 || do_lo_off % 8 || d_lo_off % 8)
    return LR2_ERR_SHAPE;
  if (o_hi && (ld_o % 8 || o_lo_off % 8)) return LR2_ERR_SHAPE;
  if (drop_p < 0.f || drop_p >= 1.f) return LR2_ERR_ARG;
  const AttnArgs a{(const bf16_t*)q_hi, (const bf16_t*)k_hi, (const bf16_t*)v_hi, (size_t)lo_off, ld, seg, batch, heads, L,
                   scale, make_drop(drop_p, drop_seed, drop_site), (hipStream_t)stream};
  if (L > 256)
    return launch_bwd_blocked(a, (const bf16_t*)do_hi, (size_t)do_lo_off, ld_do, (bf16_t*)dq_hi, (bf16_t*)dk_hi, (bf16_t*)dv_hi,
                              (size_t)d_lo_off, ld_d, (float*)lse_ws, (float*)dsum_ws);
  if (bwd_persist_ok(batch, heads, L, ld, ld_do, o_hi != nullptr)) {
#define CALLP(NT)                                                                                                                      \
  launch_bwd_persist<NT>(a, (const bf16_t*)do_hi, (size_t)do_lo_off, ld_do, (const bf16_t*)o_hi, (size_t)o_lo_off, ld_o, (bf16_t*)dq_hi, \
                         (bf16_t*)dk_hi, (bf16_t*)dv_hi, (size_t)d_lo_off, ld_d, (const float*)lse_ws, (float*)dsum_ws)
    if (L <= 64) return CALLP(4);
    if (L <= 128) return CALLP(8);
    return CALLP(14);
#undef CALLP
  }
#define CALL(NT)                                                                                                           \
  launch_bwd<NT>(a, (const bf16_t*)do_hi, (size_t)do_lo_off, ld_do, (bf16_t*)dq_hi, (bf16_t*)dk_hi, (bf16_t*)dv_hi,        \
                 (size_t)d_lo_off, ld_d, (float*)lse_ws, (float*)dsum_ws)
  LR2_SA_DISPATCH(L, CALL)
#undef CALL
}

// Which form of the attention kernels a call of this shape runs (a pure function of the shape and the device's CU count; the
// predicates are the ones the launchers of selfattn_fwd.hip and of this file call):
// *fwd_persistent / *bwd_persistent = 1 when lr2_self_attn_fwd / lr2_self_attn_bwd (the latter given o_hi) take the
// persistent kernels.  Tests assert on it; ld / ld_do as in the calls.
extern "C" int lr2_self_attn_plan(int batch, int heads, int L, int ld, int ld_do, int* fwd_persistent, int* bwd_persistent) {
  if (batch <= 0 || heads <= 0 || L < 1) return LR2_ERR_ARG;
  if (fwd_persistent) *fwd_persistent = fwd_persist_ok(batch, heads, L, ld);
  if (bwd_persistent) *bwd_persistent = bwd_persist_ok(batch, heads, L, ld, ld_do, true);
  return 0;
}
