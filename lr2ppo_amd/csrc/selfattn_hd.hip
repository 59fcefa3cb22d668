// Encoder self-attention, forward and backward, for head widths 32 .. 128 (head_dim % 16 == 0): the mathematics and the contract of
// selfattn_fwd.hip / selfattn_bwd.hip (which are written for 64 columns per head), templated on the padded head width
// HDP = head_dim rounded up to 32 = the K-step of v_mfma_f32_16x16x32_bf16, HDP in {32, 64, 96, 128}.
//
//   S = Q K^T * scale + (seg[key] > 0 ? 0 : -10000);  P = softmax(S) (fp32);  Pd = dropout(P);  O = Pd V, and the backward of that
//   replaces: tencentpretrain/layers/multi_headed_attn.py:61-74 + the mask of encoders/transformer_encoder.py:62-68 and their autograd
//
// One skeleton for every length: a workgroup is (sequence, head, 64 rows) = 4 waves x 16 rows, the OTHER operand passes through LDS in
// blocks of 64 rows (hi and lo planes, row pitch 2 HDP bytes), non-persistent, no LDS-DMA:
//   forward   queries in registers, K / V blocks in LDS, running maximum / sum and HDP / 16 output accumulators per wave
//             (self_attn_blocked_kernel's arithmetic);
//   dQ        queries and dO in registers, K / V blocks in LDS, walked twice: sweep 1 -> lse and D = sum_k P dP, sweep 2 -> dQ = dS K
//             (self_attn_bwd_dq_blocked_kernel's arithmetic);
//   dK / dV   keys (K, V fragments) in registers, Q / dO blocks in LDS, dK and dV accumulated in registers across the query blocks
//             (self_attn_bwd_dkv_blocked_kernel's arithmetic).
// Every sum has a fixed order, nothing is accumulated with atomics: the results are the same bits from run to run.
//
// The padding.  Columns [head_dim, HDP) of a head do not exist in memory: at that address are the next head's columns, the next row or
// the bytes behind the matrix.  They are never loaded -- a staged row's units beyond head_dim and a fragment's k-steps beyond head_dim
// are zeros written by the kernel (head_dim % 16 == 0: a 16-byte unit = 8 columns lies wholly inside or wholly outside the head) -- and
// never stored: the tile stores skip columns >= head_dim.  Zero columns add nothing to S = Q K^T and dP = dO V^T; the matching output
// columns of O, dQ, dK, dV come out as zeros and are dropped.
//
// The dropout mask's element index ((b * heads + h) * L + q) * mask_pitch(L) + key does not involve the head width: the stream is the
// one of the 64-column kernels (oracle.attention_keep_mask).
//
// LDS image of a staged plane: [64 rows][HDP / 8 units of 16 B], unit u of row r at u ^ ((r >> 1) & 3) -- selfattn_common.h's k_off
// assumes 128-byte rows and 8 units; an XOR of the two low unit bits stays inside every width's row (4, 8, 12 or 16 units).  One image
// serves the row-fragment reads (ds_read_b128) and the transposed reads (ds_read_b64_tr_b16); bank conflicts are accepted (DESIGN 4.5
// has the measured price against the 64-column kernels).

#include "selfattn_common.h"

namespace {

constexpr int HB = 64;            // rows of one staged block
constexpr int HT = HB / 16;       // ... in 16-row tiles
constexpr int HW = 4;             // waves per workgroup, 16 rows each

template <int HDP>
__device__ __forceinline__ int hd_off(int r, int u) { return r * (2 * HDP) + ((u ^ ((r >> 1) & 3)) << 4); }

// LDS bytes of a kernel: four planes (two operands, hi and lo), nstat per-row fp32 vectors, one 16 x (HDP + 4) fp32 slab per wave
constexpr size_t hd_lds(int hdp, int nstat) { return (size_t)4 * HB * 2 * hdp + (size_t)nstat * HB * 4 + (size_t)HW * 16 * (hdp + 4) * 4; }

// 16 rows x head_dim columns of one planes matrix as MFMA fragments (lane: row l & 15, columns 8 g + 32 ks ..); elem_off addresses
// column 8 g of the lane's row.  !ok or a k-step beyond the head: zeros, nothing is loaded.
template <int HDP>
__device__ __forceinline__ void load_frags_hd(const bf16_t* hi_plane, size_t lo_off, size_t elem_off, int g, int head_dim, bool ok,
                                              bf16x8_t (&fh)[HDP / 32], bf16x8_t (&fl)[HDP / 32]) {
#pragma unroll
  for (int ks = 0; ks < HDP / 32; ++ks) {
    u32x4_t a = {0, 0, 0, 0}, c = a;
    if (ok && 8 * g + 32 * ks < head_dim) {
      a = *reinterpret_cast<const u32x4_t*>(hi_plane + elem_off + 32 * ks);
      c = *reinterpret_cast<const u32x4_t*>(hi_plane + elem_off + 32 * ks + lo_off);
    }
    fh[ks] = __builtin_bit_cast(bf16x8_t, a);
    fl[ks] = __builtin_bit_cast(bf16x8_t, c);
  }
}

// Rows r0 .. r0 + 63 of one head's operands A and B (K and V, or Q and dO), both planes, into LDS; rows >= L and the units beyond
// head_dim are zeros.
template <int HDP>
__device__ __forceinline__ void stage_rows2_hd(const bf16_t* __restrict__ a_hi, size_t a_lo_off, int ld_a, const bf16_t* __restrict__ b_hi,
                                               size_t b_lo_off, int ld_b, size_t row0, int col0, int r0, int L, int head_dim, int tid,
                                               char* sA, char* sB) {
  constexpr int NU = HDP / 8, PLANE = HB * 2 * HDP;
  for (int i = tid; i < HB * NU; i += 64 * HW) {
    const int r = i / NU, u = i - r * NU;
    u32x4_t ah = {0, 0, 0, 0}, al = ah, bh = ah, bl = ah;
    if (r0 + r < L && 8 * u < head_dim) {
      const size_t oa = (row0 + r0 + r) * (size_t)ld_a + col0 + u * 8;
      const size_t ob = (row0 + r0 + r) * (size_t)ld_b + col0 + u * 8;
      ah = *reinterpret_cast<const u32x4_t*>(a_hi + oa);
      al = *reinterpret_cast<const u32x4_t*>(a_hi + oa + a_lo_off);
      bh = *reinterpret_cast<const u32x4_t*>(b_hi + ob);
      bl = *reinterpret_cast<const u32x4_t*>(b_hi + ob + b_lo_off);
    }
    const int o = hd_off<HDP>(r, u);
    *reinterpret_cast<u32x4_t*>(sA + o) = ah;
    *reinterpret_cast<u32x4_t*>(sA + PLANE + o) = al;
    *reinterpret_cast<u32x4_t*>(sB + o) = bh;
    *reinterpret_cast<u32x4_t*>(sB + PLANE + o) = bl;
  }
}
// the additive key mask of keys k0 .. k0 + 63 (natural-log domain); keys >= L: -inf
__device__ __forceinline__ void stage_key_mask_hd(const int64_t* __restrict__ seg, size_t row0, int k0, int L, int tid, float* sMask) {
  for (int j = tid; j < HB; j += 64 * HW) sMask[j] = (k0 + j < L) ? ((seg[row0 + k0 + j] > 0) ? 0.f : -10000.0f) : -INFINITY;
}
// lse and D of queries q0 .. q0 + 63 (si0 = index of the head's query 0); padded queries: P = exp(-inf) = 0
__device__ __forceinline__ void stage_lse_d_hd(const float* __restrict__ lse, const float* __restrict__ dsum, size_t si0, int q0, int L,
                                               int tid, float* sLse, float* sD) {
  for (int j = tid; j < HB; j += 64 * HW) {
    sLse[j] = (q0 + j < L) ? lse[si0 + q0 + j] : INFINITY;
    sD[j] = (q0 + j < L) ? dsum[si0 + q0 + j] : 0.f;
  }
}
// a = A_t x^T: rows 16 t .. 16 t + 15 of the staged A (A fragments: row 16 t + (l & 15)) against this lane's x fragments
template <int HDP>
__device__ __forceinline__ f32x4_t s_tile_hd(const char* sA, int t, int lane, const bf16x8_t (&xh)[HDP / 32],
                                             const bf16x8_t (&xl)[HDP / 32]) {
  constexpr int PLANE = HB * 2 * HDP;
  f32x4_t a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < HDP / 32; ++ks) {
    const int o = hd_off<HDP>(16 * t + (lane & 15), (lane >> 4) + 4 * ks);
    a = mfma3(*reinterpret_cast<const bf16x8_t*>(sA + o), *reinterpret_cast<const bf16x8_t*>(sA + PLANE + o), xh[ks], xl[ks], a);
  }
  return a;
}
// two ds_read_b64_tr_b16 (rows row_a and row_b of the lane's 4-row groups) = the B fragment of a product contracted over the rows
template <int HDP>
__device__ __forceinline__ bf16x8_t tr_pair_hd(const char* plane, int row_a, int row_b, int u, int half8) {
  const s16x4_t lo =
      __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(plane + hd_off<HDP>(row_a, u) + half8));
  const s16x4_t hi =
      __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(plane + hd_off<HDP>(row_b, u) + half8));
  typedef __attribute__((ext_vector_type(8))) short s16x8_t;
  const s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8_t, v);
}
// acc += E^T X over rows 32 u .. 32 u + 31 of the staged X (transposed reads), E = this lane's 8 values of those rows as hi + lo
// fragments (contraction slot (g, j) <-> row 4 g + j for j < 4, 16 + 4 g + j - 4 otherwise, as in selfattn_fwd.hip)
template <int HDP>
__device__ __forceinline__ void accum_block_hd(bf16x8_t eh, bf16x8_t el, const char* sX, int u, int lane, f32x4_t (&acc)[HDP / 16]) {
  constexpr int PLANE = HB * 2 * HDP;
  const int tq = (lane & 15) >> 2, tp = lane & 3;
  const int ra = 32 * u + 4 * (lane >> 4) + tq, rb = ra + 16;
#pragma unroll
  for (int n = 0; n < HDP / 16; ++n) {
    const int unit = 2 * n + (tp >> 1), half8 = 8 * (tp & 1);
    acc[n] = mfma3(eh, el, tr_pair_hd<HDP>(sX, ra, rb, unit, half8), tr_pair_hd<HDP>(sX + PLANE, ra, rb, unit, half8), acc[n]);
  }
}
// 16 x HDP accumulator tile (o[n][r] = X[row 4 g + r][col 16 n + (l & 15)], scaled per row by mul[r]) through the wave's LDS slab to
// row-contiguous stores of 4 columns: fp32 (O) and / or planes (Oh); rows >= rows_valid and columns >= head_dim are not stored.
template <int HDP>
__device__ __forceinline__ void store_tile_hd(const f32x4_t (&o)[HDP / 16], const float (&mul)[4], float* slab, int lane, int row_first,
                                              int rows_valid, int head_dim, float* __restrict__ O, bf16_t* __restrict__ Oh, size_t lo_off,
                                              size_t row_stride, size_t base) {
  constexpr int PITCH = HDP + 4, C4 = HDP / 4;
  const int qn = lane & 15, g = lane >> 4;
#pragma unroll
  for (int n = 0; n < HDP / 16; ++n)
#pragma unroll
    for (int r = 0; r < 4; ++r) slab[(4 * g + r) * PITCH + 16 * n + qn] = o[n][r] * mul[r];
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int pass = 0; pass < 16 * C4 / 64; ++pass) {
    const int idx = lane + 64 * pass;
    const int r = idx / C4, c = (idx - r * C4) * 4;
    if (row_first + r < rows_valid && c < head_dim) {
      const float4 v = *reinterpret_cast<const float4*>(slab + r * PITCH + c);
      const size_t off = base + (size_t)(row_first + r) * row_stride + c;
      if (O) *reinterpret_cast<float4*>(O + off) = v;
      if (Oh) store_planes4(Oh + off, lo_off, v);
    }
  }
  __builtin_amdgcn_wave_barrier();
}

// ---- forward ----
template <int HDP>
__global__ __launch_bounds__(64 * HW) void self_attn_hd_fwd_kernel(const bf16_t* __restrict__ Qh, const bf16_t* __restrict__ Kh,
                                                                   const bf16_t* __restrict__ Vh, size_t lo_off, int ld,
                                                                   const int64_t* __restrict__ seg, float* __restrict__ O,
                                                                   bf16_t* __restrict__ Oh, size_t o_lo_off, int ld_o, int heads, int L,
                                                                   int head_dim, float scale, float* __restrict__ lse, DropP dr) {
  constexpr int KS = HDP / 32, NO = HDP / 16, PLANE = HB * 2 * HDP;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sK = smem;                    // [hi | lo]
  char* sV = smem + 2 * PLANE;        // [hi | lo]
  float* sMask = reinterpret_cast<float*>(smem + 4 * PLANE);          // [HB]
  float* sOut = sMask + HB;                                          // [HW waves][16][HDP + 4]
  const int h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t row0 = (size_t)b * L;
  const int col0 = h * head_dim;
  const int qn = lane & 15, g = lane >> 4;
  const int sub = blockIdx.x * HW + wave;       // one 16-query sub-tile per wave (waves past the end idle through the barriers)
  const int q_row = sub * 16 + qn;
  const bool q_ok = q_row < L;
  bf16x8_t qh[KS], ql[KS];
  load_frags_hd<HDP>(Qh, lo_off, (row0 + (q_ok ? q_row : 0)) * (size_t)ld + col0 + 8 * g, g, head_dim, q_ok, qh, ql);
  const uint64_t drow = (((uint64_t)b * heads + h) * L + (uint64_t)(q_ok ? q_row : 0)) * mask_pitch(L);

  // online softmax over the key blocks: m' = max(m, max_j s_j); a = exp(m - m'); l = a l + sum_j exp(s_j - m'); O = a O + exp(s - m') V.
  // The dropout multiplies exp(s - m') before the P V product, l is the sum WITHOUT the mask.  Keys >= L carry -inf; every block holds
  // at least one real key (masked real keys carry -10000), so m' is finite from the first block on.
  float m = -INFINITY, l = 0.f;
  f32x4_t o[NO];
#pragma unroll
  for (int n = 0; n < NO; ++n) o[n] = f32x4_t{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
  for (int k0 = 0; k0 < L; k0 += HB) {
    __syncthreads();                               // the previous block's readers are done
    stage_rows2_hd<HDP>(Kh, lo_off, ld, Vh, lo_off, ld, row0, col0, k0, L, head_dim, tid, sK, sV);
    stage_key_mask_hd(seg, row0, k0, L, tid, sMask);
    __syncthreads();

    // S^T tiles: s[t][r] = S[query qn][key k0 + 16 t + 4 g + r]
    f32x4_t s[HT];
    float mx = m;
#pragma unroll
    for (int t = 0; t < HT; ++t) {
      s[t] = s_tile_hd<HDP>(sK, t, lane, qh, ql);
      const float4 mk = *reinterpret_cast<const float4*>(sMask + 16 * t + 4 * g);
      s[t][0] = s[t][0] * scale + mk.x;
      s[t][1] = s[t][1] * scale + mk.y;
      s[t][2] = s[t][2] * scale + mk.z;
      s[t][3] = s[t][3] * scale + mk.w;
      mx = fmaxf(fmaxf(mx, fmaxf(s[t][0], s[t][1])), fmaxf(s[t][2], s[t][3]));
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float alpha = exp_fast(m - mx);          // first block: exp(-inf) = 0
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < HT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[t][r] = exp_fast(s[t][r] - mx);
        sum += s[t][r];
      }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    m = mx;
    l = l * alpha + sum;
    // the accumulator holds O[query 4 g + r][..] in register r, the statistics belong to query l & 15
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float a_r = __shfl(alpha, 4 * g + r, 64);
#pragma unroll
      for (int n = 0; n < NO; ++n) o[n][r] *= a_r;
    }
#pragma unroll
    for (int u = 0; u < HT / 2; ++u) {
      float p[8];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        p[r] = s[2 * u][r];
        p[4 + r] = s[2 * u + 1][r];
      }
      if (dr.thr) {
        drop_mul4(dr, drow + (uint64_t)(k0 + 32 * u + 4 * g), p[0], p[1], p[2], p[3]);
        drop_mul4(dr, drow + (uint64_t)(k0 + 32 * u + 16 + 4 * g), p[4], p[5], p[6], p[7]);
      }
      bf16x8_t ph, pl;
      split8(p, ph, pl);
      accum_block_hd<HDP>(ph, pl, sV, u, lane, o);                   // O += P~ V
    }
  }

  const float inv = 1.0f / l;
  if (lse && g == 0 && q_ok) lse[((size_t)b * heads + h) * L + q_row] = m + logf(l);
  float inv_q[4];                           // 1 / sum of query 4 g + r (lane 4 g + r holds it: its own query is l & 15)
#pragma unroll
  for (int r = 0; r < 4; ++r) inv_q[r] = __shfl(inv, 4 * g + r, 64);
  if (sub * 16 < L)
    store_tile_hd<HDP>(o, inv_q, sOut + wave * 16 * (HDP + 4), lane, sub * 16, L, head_dim, O, Oh, o_lo_off, (size_t)ld_o,
                       row0 * (size_t)ld_o + col0);
}

// ---- backward, part 1: dQ (+ lse and D for part 2) ----
// The keys are walked in blocks TWICE.  Sweep 1 keeps, per query, the running maximum m, l = sum_k exp(s_k - m) and
// a = sum_k exp(s_k - m) dP_k (rescaled when m grows): lse = m + log l, D = sum_k P_k dP_k = a / l.  Sweep 2 recomputes S and dP per
// block, forms dS = P (dP - D) * scale and accumulates dQ = dS K.  dP = (dO V^T) o M, M = dropout keep / (1 - p).
template <int HDP>
__global__ __launch_bounds__(64 * HW) void self_attn_hd_bwd_dq_kernel(
    const bf16_t* __restrict__ Qh, const bf16_t* __restrict__ Kh, const bf16_t* __restrict__ Vh, size_t lo_off, int ld,
    const bf16_t* __restrict__ dOh, size_t do_lo_off, int ld_do, const int64_t* __restrict__ seg, bf16_t* __restrict__ dQh,
    size_t dq_lo_off, int ld_dq, float* __restrict__ lse, float* __restrict__ dsum, int heads, int L, int head_dim, float scale,
    DropP dr) {
  constexpr int KS = HDP / 32, NO = HDP / 16, PLANE = HB * 2 * HDP;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sK = smem;
  char* sV = smem + 2 * PLANE;        // V is an A operand here (rows = keys, contraction over the head's columns)
  float* sMask = reinterpret_cast<float*>(smem + 4 * PLANE);
  float* sOut = sMask + HB;
  const int h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t row0 = (size_t)b * L;
  const int col0 = h * head_dim;
  const int qn = lane & 15, g = lane >> 4;
  const int sub = blockIdx.x * HW + wave;
  const int q_row = sub * 16 + qn;
  const bool q_ok = q_row < L;
  bf16x8_t qh[KS], ql[KS], gh[KS], gl[KS];
  load_frags_hd<HDP>(Qh, lo_off, (row0 + (q_ok ? q_row : 0)) * (size_t)ld + col0 + 8 * g, g, head_dim, q_ok, qh, ql);
  load_frags_hd<HDP>(dOh, do_lo_off, (row0 + (q_ok ? q_row : 0)) * (size_t)ld_do + col0 + 8 * g, g, head_dim, q_ok, gh, gl);
  const uint64_t drow = (((uint64_t)b * heads + h) * L + (uint64_t)(q_ok ? q_row : 0)) * mask_pitch(L);

  float m = -INFINITY, l = 0.f, a = 0.f, lse_q = 0.f, dd = 0.f;
  f32x4_t o[NO];
#pragma unroll
  for (int n = 0; n < NO; ++n) o[n] = f32x4_t{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
  for (int sweep = 0; sweep < 2; ++sweep) {
#pragma unroll 1
    for (int k0 = 0; k0 < L; k0 += HB) {
      __syncthreads();                               // the previous block's readers are done
      stage_rows2_hd<HDP>(Kh, lo_off, ld, Vh, lo_off, ld, row0, col0, k0, L, head_dim, tid, sK, sV);
      stage_key_mask_hd(seg, row0, k0, L, tid, sMask);
      __syncthreads();

      f32x4_t s[HT], dp[HT];
#pragma unroll
      for (int t = 0; t < HT; ++t) {
        f32x4_t sa = s_tile_hd<HDP>(sK, t, lane, qh, ql);              // S^T = K Q^T
        f32x4_t d = s_tile_hd<HDP>(sV, t, lane, gh, gl);               // dPd^T = V dO^T
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
        for (int t = 0; t < HT; ++t) bm = fmaxf(fmaxf(bm, fmaxf(s[t][0], s[t][1])), fmaxf(s[t][2], s[t][3]));
        bm = fmaxf(bm, __shfl_xor(bm, 16, 64));
        bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
        const float m_new = fmaxf(m, bm);              // finite: every block holds at least one real key
        const float corr = exp_fast(m - m_new);        // 0 on the first block (m = -inf)
        l *= corr;
        a *= corr;
#pragma unroll
        for (int t = 0; t < HT; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float e = exp_fast(s[t][r] - m_new);
            l += e;
            a = __builtin_fmaf(e, dp[t][r], a);
          }
        m = m_new;
      } else {
#pragma unroll
        for (int u = 0; u < HT / 2; ++u) {
          float e[8];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            e[r] = exp_fast(s[2 * u][r] - lse_q) * (dp[2 * u][r] - dd) * scale;
            e[4 + r] = exp_fast(s[2 * u + 1][r] - lse_q) * (dp[2 * u + 1][r] - dd) * scale;
          }
          bf16x8_t eh, el;
          split8(e, eh, el);
          accum_block_hd<HDP>(eh, el, sK, u, lane, o);                 // dQ += dS K
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
  const float one[4] = {1.f, 1.f, 1.f, 1.f};
  if (sub * 16 < L)
    store_tile_hd<HDP>(o, one, sOut + wave * 16 * (HDP + 4), lane, sub * 16, L, head_dim, nullptr, dQh, dq_lo_off, (size_t)ld_dq,
                       row0 * (size_t)ld_dq + col0);
}

// ---- backward, part 2: dK, dV ----
// Each wave keeps its 16 keys' K / V fragments and the dK / dV accumulators while the queries (Q, dO, lse, D) pass through LDS in
// blocks, in the NON-transposed layout (lane = one key, 4 queries per 16-query tile):
//   S = Q K^T, P = exp(S - lse[q]);  dPd = dO V^T;  Pd = P o M, dS = P (dPd o M - D[q]) * scale;  dV = Pd^T dO,  dK = dS^T Q
template <int HDP>
__global__ __launch_bounds__(64 * HW) void self_attn_hd_bwd_dkv_kernel(
    const bf16_t* __restrict__ Qh, const bf16_t* __restrict__ Kh, const bf16_t* __restrict__ Vh, size_t lo_off, int ld,
    const bf16_t* __restrict__ dOh, size_t do_lo_off, int ld_do, const int64_t* __restrict__ seg, bf16_t* __restrict__ dKh,
    bf16_t* __restrict__ dVh, size_t dkv_lo_off, int ld_dkv, const float* __restrict__ lse, const float* __restrict__ dsum, int heads,
    int L, int head_dim, float scale, DropP dr) {
  constexpr int KS = HDP / 32, NO = HDP / 16, PLANE = HB * 2 * HDP;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sQ = smem;
  char* sG = smem + 2 * PLANE;        // dO
  float* sLse = reinterpret_cast<float*>(smem + 4 * PLANE);
  float* sD = sLse + HB;
  float* sOut = sD + HB;
  const int h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t row0 = (size_t)b * L;
  const int col0 = h * head_dim;
  const int kn = lane & 15, g = lane >> 4;
  const int sub = blockIdx.x * HW + wave;
  const int key = sub * 16 + kn;
  const bool k_ok = key < L;
  bf16x8_t kh[KS], kl[KS], vh[KS], vl[KS];
  load_frags_hd<HDP>(Kh, lo_off, (row0 + (k_ok ? key : 0)) * (size_t)ld + col0 + 8 * g, g, head_dim, k_ok, kh, kl);
  load_frags_hd<HDP>(Vh, lo_off, (row0 + (k_ok ? key : 0)) * (size_t)ld + col0 + 8 * g, g, head_dim, k_ok, vh, vl);
  const float kmask = k_ok ? ((seg[row0 + key] > 0) ? 0.f : -10000.0f) : -INFINITY;
  f32x4_t dv[NO], dk[NO];
#pragma unroll
  for (int n = 0; n < NO; ++n) dv[n] = dk[n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const uint64_t dbase = ((uint64_t)b * heads + h) * (uint64_t)L;
#pragma unroll 1
  for (int q0 = 0; q0 < L; q0 += HB) {
    __syncthreads();
    stage_rows2_hd<HDP>(Qh, lo_off, ld, dOh, do_lo_off, ld_do, row0, col0, q0, L, head_dim, tid, sQ, sG);
    stage_lse_d_hd(lse, dsum, ((size_t)b * heads + h) * L, q0, L, tid, sLse, sD);
    __syncthreads();
#pragma unroll 1
    for (int u = 0; u < HT / 2; ++u) {
      float pd[8], ds[8];
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int t = 2 * u + half;
        const f32x4_t sa = s_tile_hd<HDP>(sQ, t, lane, kh, kl);        // S[query q0 + 16 t + 4 g + r][key kn]
        const f32x4_t d = s_tile_hd<HDP>(sG, t, lane, vh, vl);         // dPd
        const float4 ls = *reinterpret_cast<const float4*>(sLse + 16 * t + 4 * g);
        const float4 dq = *reinterpret_cast<const float4*>(sD + 16 * t + 4 * g);
        const float lsv[4] = {ls.x, ls.y, ls.z, ls.w}, ddv[4] = {dq.x, dq.y, dq.z, dq.w};
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
      bf16x8_t eh, el;
      split8(pd, eh, el);
      accum_block_hd<HDP>(eh, el, sG, u, lane, dv);      // dV += Pd^T dO
      split8(ds, eh, el);
      accum_block_hd<HDP>(eh, el, sQ, u, lane, dk);      // dK += dS^T Q
    }
  }
  if (sub * 16 < L) {
    const float one[4] = {1.f, 1.f, 1.f, 1.f};
    float* slab = sOut + wave * 16 * (HDP + 4);
    const size_t base = row0 * (size_t)ld_dkv + col0;
    store_tile_hd<HDP>(dk, one, slab, lane, sub * 16, L, head_dim, nullptr, dKh, dkv_lo_off, (size_t)ld_dkv, base);
    store_tile_hd<HDP>(dv, one, slab, lane, sub * 16, L, head_dim, nullptr, dVh, dkv_lo_off, (size_t)ld_dkv, base);
  }
}

uint64_t g_hd_launches[2] = {0, 0};      // accepted forward / backward calls (host-side counters: lr2_self_attn_hd_launch_counts)

template <int HDP>
int launch_hd_fwd(const AttnArgs& a, int head_dim, float* o, bf16_t* oh, size_t o_lo_off, int ld_o, float* lse) {
  static bool done = false;
  if (allow_lds_once(self_attn_hd_fwd_kernel<HDP>, hd_lds(HDP, 1), done, "self_attn_hd_fwd")) return LR2_ERR_LAUNCH;
  LR2_LAUNCH(self_attn_hd_fwd_kernel<HDP>, dim3((a.L + HB - 1) / HB, a.heads, a.batch), dim3(64 * HW), hd_lds(HDP, 1), a.stream, a.q,
             a.k, a.v, a.lo_off, a.ld, a.seg, o, oh, o_lo_off, ld_o, a.heads, a.L, head_dim, a.scale, lse, a.dr);
  return lr2_launch_status("lr2_self_attn_hd_fwd");
}

template <int HDP>
int launch_hd_bwd(const AttnArgs& a, int head_dim, const bf16_t* go, size_t do_lo_off, int ld_do, bf16_t* dq, bf16_t* dk, bf16_t* dv,
                  size_t d_lo_off, int ld_d, float* lse, float* dsum) {
  static bool done1 = false, done2 = false;
  if (allow_lds_once(self_attn_hd_bwd_dq_kernel<HDP>, hd_lds(HDP, 1), done1, "self_attn_hd_bwd_dq")) return LR2_ERR_LAUNCH;
  if (allow_lds_once(self_attn_hd_bwd_dkv_kernel<HDP>, hd_lds(HDP, 2), done2, "self_attn_hd_bwd_dkv")) return LR2_ERR_LAUNCH;
  const dim3 grid((a.L + HB - 1) / HB, a.heads, a.batch);
  LR2_LAUNCH(self_attn_hd_bwd_dq_kernel<HDP>, grid, dim3(64 * HW), hd_lds(HDP, 1), a.stream, a.q, a.k, a.v, a.lo_off, a.ld, go,
             do_lo_off, ld_do, a.seg, dq, d_lo_off, ld_d, lse, dsum, a.heads, a.L, head_dim, a.scale, a.dr);
  if (lr2_launch_status("lr2_self_attn_hd_bwd(dq)")) return LR2_ERR_LAUNCH;
  LR2_LAUNCH(self_attn_hd_bwd_dkv_kernel<HDP>, grid, dim3(64 * HW), hd_lds(HDP, 2), a.stream, a.q, a.k, a.v, a.lo_off, a.ld, go,
             do_lo_off, ld_do, a.seg, dk, dv, d_lo_off, ld_d, (const float*)lse, (const float*)dsum, a.heads, a.L, head_dim, a.scale,
             a.dr);
  return lr2_launch_status("lr2_self_attn_hd_bwd(dkv)");
}

// the served widths: multiples of 16 from 32 to 128 (16: half of every K-step would be padding; lr2_self_attn_fwd's refusal stands)
inline bool hd_served(int head_dim) { return head_dim >= 32 && head_dim <= 128 && head_dim % 16 == 0; }

}  // namespace

extern "C" int lr2_self_attn_hd_launch_counts(uint64_t counts[2]) {
  if (!counts) return LR2_ERR_ARG;
  counts[0] = g_hd_launches[0];
  counts[1] = g_hd_launches[1];
  return 0;
}

#define LR2_HD_DISPATCH(head_dim, CALL)  \
  if ((head_dim) <= 32) rc = CALL(32);   \
  else if ((head_dim) <= 64) rc = CALL(64); \
  else if ((head_dim) <= 96) rc = CALL(96); \
  else rc = CALL(128);

extern "C" int lr2_self_attn_hd_fwd(const void* q_hi, const void* k_hi, const void* v_hi, uint64_t lo_off, int ld, const int64_t* seg,
                                    void* o, void* o_hi, uint64_t o_lo_off, int ld_o, void* lse, float drop_p, uint64_t drop_seed,
                                    uint32_t drop_site, int batch, int heads, int L, int head_dim, float scale, void* stream) {
  if (!q_hi || !k_hi || !v_hi || !seg || (!o && !o_hi) || batch <= 0 || heads <= 0 || L <= 0) return LR2_ERR_ARG;
  if (!(drop_p >= 0.f && drop_p < 1.f)) return LR2_ERR_ARG;
  if (!hd_served(head_dim) || ld % 8 || ld_o % 4 || lo_off % 8 || o_lo_off % 4) return LR2_ERR_SHAPE;
  const AttnArgs a{(const bf16_t*)q_hi, (const bf16_t*)k_hi, (const bf16_t*)v_hi, (size_t)lo_off, ld, seg, batch, heads, L,
                   scale, make_drop(drop_p, drop_seed, drop_site), (hipStream_t)stream};
  int rc;
#define CALL(HDP) launch_hd_fwd<HDP>(a, head_dim, (float*)o, (bf16_t*)o_hi, (size_t)o_lo_off, ld_o, (float*)lse)
  LR2_HD_DISPATCH(head_dim, CALL)
#undef CALL
  if (rc == 0) ++g_hd_launches[0];
  return rc;
}

// o_hi / o_lo_off / ld_o are accepted and checked as lr2_self_attn_bwd checks them, and not read: both kernels recompute (lse_ws and
// dsum_ws are written by the dQ kernel, whatever lse_ws held).
extern "C" int lr2_self_attn_hd_bwd(const void* q_hi, const void* k_hi, const void* v_hi, uint64_t lo_off, int ld, const void* do_hi,
                                    uint64_t do_lo_off, int ld_do, const int64_t* seg, void* dq_hi, void* dk_hi, void* dv_hi,
                                    uint64_t d_lo_off, int ld_d, const void* o_hi, uint64_t o_lo_off, int ld_o, void* lse_ws,
                                    void* dsum_ws, float drop_p, uint64_t drop_seed, uint32_t drop_site, int batch, int heads, int L,
                                    int head_dim, float scale, void* stream) {
  if (!q_hi || !k_hi || !v_hi || !do_hi || !seg || !dq_hi || !dk_hi || !dv_hi || !lse_ws || !dsum_ws || batch <= 0 || heads <= 0 ||
      L <= 0)
    return LR2_ERR_ARG;
  if (!(drop_p >= 0.f && drop_p < 1.f)) return LR2_ERR_ARG;
  if (!hd_served(head_dim) || ld % 8 || ld_do % 8 || ld_d % 8 || lo_off % 8 || do_lo_off % 8 || d_lo_off % 8) return LR2_ERR_SHAPE;
  if (o_hi && (ld_o % 8 || o_lo_off % 8)) return LR2_ERR_SHAPE;
  const AttnArgs a{(const bf16_t*)q_hi, (const bf16_t*)k_hi, (const bf16_t*)v_hi, (size_t)lo_off, ld, seg, batch, heads, L,
                   scale, make_drop(drop_p, drop_seed, drop_site), (hipStream_t)stream};
  int rc;
#define CALL(HDP)                                                                                                            \
  launch_hd_bwd<HDP>(a, head_dim, (const bf16_t*)do_hi, (size_t)do_lo_off, ld_do, (bf16_t*)dq_hi, (bf16_t*)dk_hi, (bf16_t*)dv_hi, \
                     (size_t)d_lo_off, ld_d, (float*)lse_ws, (float*)dsum_ws)
  LR2_HD_DISPATCH(head_dim, CALL)
#undef CALL
  if (rc == 0) ++g_hd_launches[1];
  return rc;
}
