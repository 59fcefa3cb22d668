// Encoder self-attention, forward, on the matrix cores (TencentPretrain MultiHeadedAttention core, head_dim 64, L <= 256).
//
//   S = Q K^T * scale + (seg[key] > 0 ? 0 : -10000);  P = softmax(S);  O = P V        (fp32 semantics)
//   replaces: tencentpretrain/layers/multi_headed_attn.py:61-74 + the mask of encoders/transformer_encoder.py:62-68
//
// Q, K, V arrive as bf16 hi/lo planes (the QKV GEMM's epilogue writes them), both products run as split-bf16 x3 on
// v_mfma_f32_16x16x32_bf16 with fp32 accumulation, the softmax is fp32.  One workgroup = one (sequence, head, 64 query
// rows); its 4 waves own 16 query rows each.  K and V of the head live in LDS as bf16 planes (4 x LP x 128 B).
//
// The score tile is computed TRANSPOSED, S^T = K Q^T: in the 16x16 accumulator layout a lane then holds, for ONE query
// (column l & 15), the keys 4*(l >> 4) + r of every 16-key tile -- exactly the shape of an MFMA A operand row.  Two
// adjacent key tiles give a lane 8 probabilities of its query: they are used directly as the A fragment of P V with the
// contraction index permuted (slot (g, j) <-> key 4g + j for j < 4, 16 + 4g + j - 4 otherwise); the V fragments are read
// with the same permutation by two ds_read_b64_tr_b16 (rows 4g .. 4g+3 and 16 + 4g .. 16 + 4g + 3 of the key block).
// P never touches LDS and no shuffle is needed between the two GEMMs.
//
// Three forms, chosen by lr2_self_attn_fwd from the shape: self_attn_mfma_kernel (one workgroup per pair, L <= 224),
// self_attn_persist_kernel (the same phases, one workgroup per CU walking over the pairs) and self_attn_blocked_kernel (L > 224: key
// blocks with a running max / sum).  The backward is selfattn_bwd.hip; what both share is selfattn_common.h.

#include "selfattn_common.h"

namespace {

// One 16-query sub-tile against the K / V planes resident in LDS, in two phases that touch different planes:
//   phase A (K, mask):  S^T = K Q^T (MFMA), fp32 softmax in the log2 domain -> the un-normalised probabilities as bf16 hi / lo
//                       fragments of the P V product + 1 / sum;
//   phase B (V):        O = (P~ V) / sum (MFMA), rows stored through the wave's LDS slab.
// qh / ql: the sub-tile's query fragments.
template <int NT, bool DROP = true>
__device__ __forceinline__ void attn_phase_a(const char* sK, const float* sMask, const bf16x8_t (&qh)[2], const bf16x8_t (&ql)[2],
                                             int sub, int lane, int L, int b, int h, int heads, float scale, float* __restrict__ lse,
                                             const DropP& dr, bf16x8_t (&ph)[NT / 2], bf16x8_t (&pl)[NT / 2], float& inv) {
  constexpr int PLANE = 16 * NT * ROW_B;
  const int qn = lane & 15, g = lane >> 4;
  const int q_row = sub * 16 + qn;
  // ---- S^T tiles: acc[t][r] = S[query qn][key 16t + 4g + r] ----
  const uint32_t kb[2] = {lds_addr(sK + k_off(qn, g)), lds_addr(sK + k_off(qn, g + 4))};
  f32x4_t s[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      // A fragment: key row 16t + (l & 15), hd 8g + 32ks ..: k_off(16t + qn, g + 4ks) = 2048 t + k_off(qn, g + 4ks)
      const bf16x8_t kh = lds_ld16(kb[ks] + 2048 * t);
      const bf16x8_t kl = lds_ld16(kb[ks] + 2048 * t + PLANE);
      acc = mfma3(kh, kl, qh[ks], ql[ks], acc);
    }
    s[t] = acc;
  }

  // ---- softmax over the keys of query qn: in-lane over (t, r), across the 4 lanes l, l^16, l^32, l^48 ----
  float mx = -INFINITY;
  const float scale2 = scale * LOG2E;
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
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      s[t][r] = __builtin_amdgcn_exp2f(s[t][r] - mx);     // padded keys: 2^(-inf) = 0
      sum += s[t][r];
    }
  }
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);
  inv = 1.0f / sum;
  if (lse && g == 0 && q_row < L) lse[((size_t)b * heads + h) * L + q_row] = mx * LN2 + logf(sum);
  const uint64_t drow = (((uint64_t)b * heads + h) * L + (uint64_t)(q_row < L ? q_row : 0)) * mask_pitch(L);

  // ---- P~ = the un-normalised exponentials in (0, 1], as the A fragments of P V: straight from the accumulators (permuted
  // contraction index: slot (g, j) <-> key 4g + j for j < 4, 16 + 4g + j - 4 otherwise, of each 32-key block) ----
#pragma unroll
  for (int u = 0; u < NT / 2; ++u) {
    float p[8];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      p[r] = s[2 * u][r];
      p[4 + r] = s[2 * u + 1][r];
    }
    if (DROP && dr.thr) {
      drop_mul4(dr, drow + 32 * u + 4 * g, p[0], p[1], p[2], p[3]);
      drop_mul4(dr, drow + 32 * u + 16 + 4 * g, p[4], p[5], p[6], p[7]);
    }
    const uint32_t h01 = cvt_pk_bf16(p[0], p[1]), h23 = cvt_pk_bf16(p[2], p[3]);
    const uint32_t h45 = cvt_pk_bf16(p[4], p[5]), h67 = cvt_pk_bf16(p[6], p[7]);
    const uint32_t l01 = cvt_pk_bf16(p[0] - __uint_as_float(h01 << 16), p[1] - __uint_as_float(h01 & 0xffff0000u));
    const uint32_t l23 = cvt_pk_bf16(p[2] - __uint_as_float(h23 << 16), p[3] - __uint_as_float(h23 & 0xffff0000u));
    const uint32_t l45 = cvt_pk_bf16(p[4] - __uint_as_float(h45 << 16), p[5] - __uint_as_float(h45 & 0xffff0000u));
    const uint32_t l67 = cvt_pk_bf16(p[6] - __uint_as_float(h67 << 16), p[7] - __uint_as_float(h67 & 0xffff0000u));
    ph[u] = __builtin_bit_cast(bf16x8_t, (u32x4_t{h01, h23, h45, h67}));
    pl[u] = __builtin_bit_cast(bf16x8_t, (u32x4_t{l01, l23, l45, l67}));
  }
}

// HALF_SLAB: the wave's LDS slab holds 16 rows x 32 columns (the 16-wave persistent kernel: 13-14 slabs beside the K / V planes);
// the output then leaves in two halves of 32 head columns.  Same values either way.
struct NoHook {
  __device__ __forceinline__ void operator()() const {}
};
// after_pv(): called between the last P V product and the output's way through the slab (the persistent kernel requests the next
// pair's query fragments there: the probability registers are dead by then).
template <int NT, bool HALF_SLAB = false, typename Hook = NoHook>
__device__ __forceinline__ void attn_phase_b(const char* sV, float* slab, const bf16x8_t (&ph)[NT / 2], const bf16x8_t (&pl)[NT / 2],
                                             float inv, int sub, int lane, int L, size_t row0, int col0, float* __restrict__ O,
                                             bf16_t* __restrict__ Oh, size_t o_lo_off, int ld_o, Hook after_pv = Hook()) {
  constexpr int PLANE = 16 * NT * ROW_B;
  const int qn = lane & 15, g = lane >> 4;
  const int i16 = lane & 15, tq = i16 >> 2, tp = i16 & 3;
  // transposed V reads: lane (tq, tp) of a 16-lane group supplies row 32u + 4g + tq (and that row + 16), hd 16n + 4tp .. +3:
  // v_off(32u + 4g + tq (+ 16), unit) = 4096 u (+ 2048) + v_off(4g + tq, unit)
  uint32_t vb[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) vb[n] = lds_addr(sV + v_off(4 * g + tq, 2 * n + (tp >> 1)) + 8 * (tp & 1));
  if constexpr (HALF_SLAB) {
    // 32 head columns at a time: 8 accumulator registers + the V fragments of two column groups beside the probabilities (a
    // 128-register wave); each half leaves through the 16 x 32 slab as soon as it is complete
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      f32x4_t o[2] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int u = 0; u < NT / 2; ++u) {
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          const uint32_t a = vb[2 * half + n] + 4096 * u;
          const bf16x8_t vh = lds_tr_pair(a, a + 2048);
          const bf16x8_t vl = lds_tr_pair(a + PLANE, a + 2048 + PLANE);
          o[n] = mfma3(ph[u], pl[u], vh, vl, o[n]);
        }
      }
      if (half == 1) after_pv();
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) slab[(4 * g + r) * (32 + 4) + 16 * n + qn] = o[n][r] * __shfl(inv, 4 * g + r, 64);
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int pass = 0; pass < 2; ++pass) {
        const int r = pass * 8 + (lane >> 3), c = (lane & 7) * 4;
        const int qr = sub * 16 + r;
        if (qr < L) {
          const float4 v = *reinterpret_cast<const float4*>(slab + r * (32 + 4) + c);
          // uniform 64-bit base + 32-bit lane offset: the stores take the scalar-base form (no 64-bit address registers per lane)
          const size_t ubase = row0 * (size_t)ld_o + col0 + 32 * half;
          const uint32_t loff = (uint32_t)qr * (uint32_t)ld_o + (uint32_t)c;
          if (O) *reinterpret_cast<float4*>(O + ubase + loff) = v;
          if (Oh) store_planes4(Oh + ubase + loff, o_lo_off, v);
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
    return;
  }
  // ---- O = (P~ V) / sum over 32-key blocks; the 1 / sum goes onto the 16 output values instead of the NT * 4 probabilities
  f32x4_t o[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) o[n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < NT / 2; ++u) {
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const bf16x8_t vh = lds_tr_pair(vb[n] + 4096 * u, vb[n] + 4096 * u + 2048);
      const bf16x8_t vl = lds_tr_pair(vb[n] + 4096 * u + PLANE, vb[n] + 4096 * u + 2048 + PLANE);
      o[n] = mfma3(ph[u], pl[u], vh, vl, o[n]);
    }
  }

  after_pv();
  // ---- o[n][r] = O[query 4g + r][hd 16n + (l & 15)] -> LDS slab -> 16-B row-contiguous stores ----
  float inv_q[4];                         // 1 / sum of query 4g + r (lane 4g + r holds it: its own query is l & 15)
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
    if (qr < L) {
      const float4 v = *reinterpret_cast<const float4*>(slab + r * (HD + 4) + c);
      const size_t off = (row0 + qr) * (size_t)ld_o + col0 + c;
      if (O) *reinterpret_cast<float4*>(O + off) = v;
      if (Oh) store_planes4(Oh + off, o_lo_off, v);
    }
  }
  __builtin_amdgcn_wave_barrier();
}

template <int NT>
__device__ __forceinline__ void attn_subtile_fwd(const char* sK, const char* sV, const float* sMask, float* slab,
                                                 const bf16x8_t (&qh)[2], const bf16x8_t (&ql)[2], int sub, int lane, int L, int b,
                                                 int h, int heads, size_t row0, int col0, float scale, float* __restrict__ lse,
                                                 const DropP& dr, float* __restrict__ O, bf16_t* __restrict__ Oh, size_t o_lo_off,
                                                 int ld_o) {
  bf16x8_t ph[NT / 2], pl[NT / 2];
  float inv;
  attn_phase_a<NT>(sK, sMask, qh, ql, sub, lane, L, b, h, heads, scale, lse, dr, ph, pl, inv);
  attn_phase_b<NT>(sV, slab, ph, pl, inv, sub, lane, L, row0, col0, O, Oh, o_lo_off, ld_o);
}

template <int NT, int NW>   // NT = key tiles of 16 (even), LP = 16 * NT padded keys; NW = waves per workgroup
__global__ __launch_bounds__(64 * NW) void self_attn_mfma_kernel(const bf16_t* __restrict__ Qh, const bf16_t* __restrict__ Kh,
                                                             const bf16_t* __restrict__ Vh, size_t lo_off, int ld,
                                                             const int64_t* __restrict__ seg, float* __restrict__ O,
                                                             bf16_t* __restrict__ Oh, size_t o_lo_off, int ld_o, int heads,
                                                             int L, float scale, float* __restrict__ lse, DropP dr) {
  constexpr int LP = 16 * NT;
  constexpr int PLANE = LP * ROW_B;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sK = smem;                    // [hi | lo]
  char* sV = smem + 2 * PLANE;        // [hi | lo]
  float* sMask = reinterpret_cast<float*>(smem + 4 * PLANE);          // [LP]
  float* sOut = sMask + LP;                                          // [NW waves][16][HD + 4]
  const int h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t row0 = (size_t)b * L;
  const int col0 = h * HD;

  const int qn = lane & 15, g = lane >> 4;
  const int n_sub = (L + 15) >> 4;
  // Query fragments of a 16-row sub-tile: B operand of S^T = K Q^T (lane: query l & 15, hd 8*(l >> 4) + 32*ks ..).
  // Requested one sub-tile ahead -- the first one before K / V are staged -- so that the HBM latency of the 64 x 4 x 16 B
  // never sits between two MFMA phases.
  auto load_q = [&](int sub_, bf16x8_t (&fh)[2], bf16x8_t (&fl)[2]) {
    const int q_row_ = sub_ * 16 + qn;
    const bool ok = sub_ < n_sub && q_row_ < L;
    load_frags(Qh, lo_off, (row0 + (ok ? q_row_ : 0)) * (size_t)ld + col0 + 8 * g, ok, fh, fl);
  };
  const int sub_first = blockIdx.x * NW + wave, sub_step = gridDim.x * NW;
  bf16x8_t qh[2], ql[2], qh_next[2], ql_next[2];
  load_q(sub_first, qh_next, ql_next);

  // ---- stage K, V (both planes) and the additive key mask: every request first, then the LDS writes (one HBM latency
  // for the whole 4 x LP x 128 B instead of one per loop trip) ----
  {
    constexpr int TRIPS = (LP * 8 + 64 * NW - 1) / (64 * NW);
    u32x4_t kh[TRIPS], kl[TRIPS], vh[TRIPS], vl[TRIPS];
#pragma unroll
    for (int it = 0; it < TRIPS; ++it) {
      const int i = tid + it * 64 * NW;
      const int r = i >> 3, u = i & 7;
      kh[it] = u32x4_t{0, 0, 0, 0};
      kl[it] = kh[it]; vh[it] = kh[it]; vl[it] = kh[it];
      if (i < LP * 8 && r < L) {
        const size_t o = (row0 + r) * (size_t)ld + col0 + u * 8;
        kh[it] = *reinterpret_cast<const u32x4_t*>(Kh + o);
        kl[it] = *reinterpret_cast<const u32x4_t*>(Kh + o + lo_off);
        vh[it] = *reinterpret_cast<const u32x4_t*>(Vh + o);
        vl[it] = *reinterpret_cast<const u32x4_t*>(Vh + o + lo_off);
      }
    }
#pragma unroll
    for (int it = 0; it < TRIPS; ++it) {
      const int i = tid + it * 64 * NW;
      const int r = i >> 3, u = i & 7;
      if (i < LP * 8) {
        *reinterpret_cast<u32x4_t*>(sK + k_off(r, u)) = kh[it];
        *reinterpret_cast<u32x4_t*>(sK + PLANE + k_off(r, u)) = kl[it];
        *reinterpret_cast<u32x4_t*>(sV + v_off(r, u)) = vh[it];
        *reinterpret_cast<u32x4_t*>(sV + PLANE + v_off(r, u)) = vl[it];
      }
    }
  }
  // additive key mask, pre-multiplied by log2(e): the softmax below works on t = s * scale * log2(e) + mask * log2(e)
  // (2^(t - max t) = e^(s' - max s')), one fma + one v_exp_f32 per score instead of fma, multiply and v_exp_f32
  for (int j = tid; j < LP; j += 64 * NW) sMask[j] = j < L ? ((seg[row0 + j] > 0) ? 0.f : -10000.0f * LOG2E) : -INFINITY;

  __syncthreads();
  // K / V stay resident; each wave walks over 16-query sub-tiles (blockIdx.x strides them when the grid splits the queries)
  for (int sub = sub_first; sub < n_sub; sub += sub_step) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) { qh[ks] = qh_next[ks]; ql[ks] = ql_next[ks]; }
  load_q(sub + sub_step, qh_next, ql_next);     // next sub-tile's queries travel while this one is computed

  attn_subtile_fwd<NT>(sK, sV, sMask, sOut + wave * 16 * (HD + 4), qh, ql, sub, lane, L, b, h, heads, row0, col0, scale, lse, dr,
                       O, Oh, o_lo_off, ld_o);
  }  // sub-tile loop
}

// ---- persistent forward: one workgroup per CU walks over (sequence, head) pairs, K / V travel by LDS-DMA under the compute; the
// protocol (who loads what when, the two barriers per pair, the hazards) is written out in selfattn_common.h.  Same arithmetic, same
// bits as self_attn_mfma_kernel (both call attn_phase_a / attn_phase_b). ----
template <int NT, bool DROP>
__global__ __launch_bounds__(64 * PS_WAVES) void self_attn_persist_kernel(const bf16_t* __restrict__ Qh, const bf16_t* __restrict__ Kh,
                                                                          const bf16_t* __restrict__ Vh, size_t lo_off, int ld,
                                                                          const int64_t* __restrict__ seg, float* __restrict__ O,
                                                                          bf16_t* __restrict__ Oh, size_t o_lo_off, int ld_o, int heads,
                                                                          int L, float scale, float* __restrict__ lse, DropP dr,
                                                                          int n_pairs, uint32_t kv_bytes) {
  constexpr int LP = 16 * NT;
  constexpr int PLANE = LP * ROW_B;
  constexpr int MK = (LP + 64 * PS_MOVERS - 1) / (64 * PS_MOVERS);     // mask values per mover thread
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sK = smem;                    // [hi | lo]
  char* sV = smem + 2 * PLANE;        // [hi | lo]
  float* sMask = reinterpret_cast<float*>(smem + 4 * PLANE);          // [2][LP]: pair number it reads half it & 1
  float* sOut = sMask + 2 * LP;                                      // [PS_MAX_SUB waves][16][32 + 4]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool mover = wave >= PS_MAX_SUB;
  const int mtid = tid - 64 * PS_MAX_SUB;                             // thread number among the movers
  const int qn = lane & 15, g = lane >> 4;
  const int n_sub = (L + 15) >> 4;
  const bool computes = wave < n_sub;
  float* slab = sOut + (mover ? 0 : wave) * 16 * (32 + 4);
  const uint32_t row_bytes = (uint32_t)ld * 2u;

  int p = blockIdx.x;
  if (p >= n_pairs) return;
  int b = p / heads, h = p - b * heads;
  size_t row0 = (size_t)b * L;
  int col0 = h * HD;

  if (mover) {
    // ---- the two mover waves ----
    const __amdgpu_buffer_rsrc_t k_hi = buf_rsrc(Kh, kv_bytes), k_lo = buf_rsrc(Kh + lo_off, kv_bytes);
    const __amdgpu_buffer_rsrc_t v_hi = buf_rsrc(Vh, kv_bytes), v_lo = buf_rsrc(Vh + lo_off, kv_bytes);
    const int j0 = wave - PS_MAX_SUB;
    dma_rows<NT, IMG_K, 2>(k_hi, k_lo, sK, lane, j0, 2 * NT, PS_MOVERS, (uint32_t)((row0 * ld + col0) * 2), row_bytes, L);
    // additive key mask, pre-multiplied by log2(e) (see self_attn_mfma_kernel)
    for (int j = mtid; j < LP; j += 64 * PS_MOVERS) sMask[j] = j < L ? ((seg[row0 + j] > 0) ? 0.f : -10000.0f * LOG2E) : -INFINITY;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    phase_barrier();
    for (int it = 0;; ++it) {
      // phase A of pair p: its V planes travel
      dma_rows<NT, IMG_V, 2>(v_hi, v_lo, sV, lane, j0, 2 * NT, PS_MOVERS, (uint32_t)((row0 * ld + col0) * 2), row_bytes, L);
      const int pn = p + gridDim.x;
      const bool more = pn < n_pairs;
      const int bn = pn / heads, hn = pn - bn * heads;
      const size_t row0n = (size_t)bn * L;
      float mk[MK];
      if (more) {
#pragma unroll
        for (int i = 0; i < MK; ++i) {
          const int j = mtid + i * 64 * PS_MOVERS;
          mk[i] = j < L ? ((seg[row0n + j] > 0) ? 0.f : -10000.0f * LOG2E) : -INFINITY;
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                // V of this pair has landed
      phase_barrier();
      if (!more) break;
      // phase B of pair p: K and the mask of the next pair travel
      dma_rows<NT, IMG_K, 2>(k_hi, k_lo, sK, lane, j0, 2 * NT, PS_MOVERS, (uint32_t)((row0n * ld + hn * HD) * 2), row_bytes, L);
      float* mnext = sMask + ((it + 1) & 1) * LP;
#pragma unroll
      for (int i = 0; i < MK; ++i) {
        const int j = mtid + i * 64 * PS_MOVERS;
        if (j < LP) mnext[j] = mk[i];
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                // K of the next pair has landed
      phase_barrier();
      p = pn; row0 = row0n; col0 = hn * HD;
    }
    return;
  }

  if (!computes) {
    // ---- waves n_sub .. 13: nothing to compute, they only keep the barriers company ----
    phase_barrier();
    for (;;) {
      phase_barrier();
      p += gridDim.x;
      if (p >= n_pairs) break;
      phase_barrier();
    }
    return;
  }

  // ---- compute waves ----
  const int sub = wave;
  // query fragments of this wave's sub-tile of the pair whose first row is row0_ (B operand of S^T = K Q^T).  load_frags_u's body, kept
  // here: called through the shared helper the loop below compiles to different instructions (selfattn_common.h, "left alone")
  auto load_q = [&](size_t row0_, int col0_, bf16x8_t (&fh)[2], bf16x8_t (&fl)[2]) {
    const int lane_ = opaque(lane);
    const int q_row_ = sub * 16 + (lane_ & 15);
    const bool ok = q_row_ < L;
    const bf16_t* ub = Qh + row0_ * (size_t)ld + col0_;                      // uniform
    const uint32_t o = (uint32_t)(ok ? q_row_ : 0) * (uint32_t)ld + 8u * (uint32_t)(lane_ >> 4);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      u32x4_t a = {0, 0, 0, 0}, c = a;
      if (ok) {
        a = *reinterpret_cast<const u32x4_t*>(ub + o + 32 * ks);
        c = *reinterpret_cast<const u32x4_t*>(ub + lo_off + o + 32 * ks);
      }
      fh[ks] = __builtin_bit_cast(bf16x8_t, a);
      fl[ks] = __builtin_bit_cast(bf16x8_t, c);
    }
  };
  bf16x8_t qh[2], ql[2];
  load_q(row0, col0, qh, ql);
  phase_barrier();
  for (int it = 0;; ++it) {
    const float* mask = sMask + (it & 1) * LP;
    bf16x8_t ph[NT / 2], pl[NT / 2];
    float inv = 0.f;
    attn_phase_a<NT, DROP>(sK, mask, qh, ql, sub, opaque(lane), L, b, h, heads, scale, lse, dr, ph, pl, inv);
    phase_barrier();
    const int pn = p + gridDim.x;
    const bool more = pn < n_pairs;
    const int bn = pn / heads, hn = pn - bn * heads;
    const size_t row0n = (size_t)bn * L;
    // the next pair's queries are requested once the probability registers are dead; they travel under the output's stores and the
    // wait at the barrier
    auto next_q = [&]() { if (more) load_q(row0n, hn * HD, qh, ql); };
    attn_phase_b<NT, true>(sV, slab, ph, pl, inv, sub, opaque(lane), L, row0, col0, O, Oh, o_lo_off, ld_o, next_q);
    if (!more) break;
    phase_barrier();
    p = pn; b = bn; h = hn; row0 = row0n; col0 = hn * HD;
  }
}

// ---- forward for sequences longer than one LDS-resident key block (L > 256: ViT-L/14's 257 tokens, RoBERTa's 514) ----
// Same arithmetic and fragment layout as self_attn_mfma_kernel, with the keys walked in blocks of LP = 16 * NT: K / V of
// ONE block live in LDS; every wave keeps, for each of its (up to SLOTS) 16-query sub-tiles, the running row maximum m,
// the running sum l and the un-normalised output accumulator across the blocks (online softmax):
//     m' = max(m, max_j s_j);  a = exp(m - m');  l = a l + sum_j exp(s_j - m');  O = a O + exp(s - m') V_block
// and normalises by l at the end.  Probability dropout multiplies exp(s - m') by mask / keep before the P V product; l is
// the sum WITHOUT the mask, so O / l equals dropout(softmax(S)) V exactly as in the one-block kernel.
// Padding keys (index >= L) carry -inf; every block holds at least one real key (real keys masked by seg get -10000,
// as upstream), so m' is finite from the first block on.
template <int SLOTS>
struct AttnState {
  f32x4_t o[SLOTS][4];
  float m[SLOTS], l[SLOTS];
};

template <int NT, int NW, int SLOTS, int J>
__device__ __forceinline__ void blocked_subtiles(AttnState<SLOTS>& st, const bf16_t* __restrict__ Qh, size_t lo_off, int ld,
                                                 size_t row0, int col0, const char* sK, const char* sV, const float* sMask,
                                                 int sub_first, int sub_step, int n_sub, int L, int k0, float scale, int heads,
                                                 int b, int h, const DropP& dr, int lane) {
  constexpr int LP = 16 * NT;
  constexpr int PLANE = LP * ROW_B;
  const int qn = lane & 15, g = lane >> 4;
  const int sub = sub_first + J * sub_step;
  if (sub < n_sub) {            // wave-uniform
    const int q_row = sub * 16 + qn;
    bf16x8_t qh[2], ql[2];
    {   // load_frags' body, kept here: called through the helper this kernel compiles to other instructions (selfattn_common.h)
      const bool ok = q_row < L;
      const size_t o = (row0 + (ok ? q_row : 0)) * (size_t)ld + col0 + 8 * g;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        u32x4_t a = {0, 0, 0, 0}, c = a;
        if (ok) {
          a = *reinterpret_cast<const u32x4_t*>(Qh + o + 32 * ks);
          c = *reinterpret_cast<const u32x4_t*>(Qh + o + 32 * ks + lo_off);
        }
        qh[ks] = __builtin_bit_cast(bf16x8_t, a);
        ql[ks] = __builtin_bit_cast(bf16x8_t, c);
      }
    }
    f32x4_t s[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int r = 16 * t + qn;
        const bf16x8_t kh = *reinterpret_cast<const bf16x8_t*>(sK + k_off(r, g + 4 * ks));
        const bf16x8_t kl = *reinterpret_cast<const bf16x8_t*>(sK + PLANE + k_off(r, g + 4 * ks));
        acc = mfma3(kh, kl, qh[ks], ql[ks], acc);
      }
      s[t] = acc;
    }
    float mx = st.m[J];
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
    const float alpha = exp_fast(st.m[J] - mx);     // first block: exp(-inf) = 0
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
    st.m[J] = mx;
    st.l[J] = st.l[J] * alpha + sum;
    // the output accumulator holds O[query 4g + r][..] in register r, the statistics belong to query (l & 15): fetch the
    // rescale factor of query 4g + r from the lane that owns it
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float a_r = __shfl(alpha, 4 * g + r, 64);
#pragma unroll
      for (int n = 0; n < 4; ++n) st.o[J][n][r] *= a_r;
    }
    const uint64_t drow = (((uint64_t)b * heads + h) * L + (uint64_t)(q_row < L ? q_row : 0)) * mask_pitch(L) + (uint64_t)k0;
    const int i16 = lane & 15, tq = i16 >> 2, tp = i16 & 3;
#pragma unroll
    for (int u = 0; u < NT / 2; ++u) {
      float p[8];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        p[r] = s[2 * u][r];
        p[4 + r] = s[2 * u + 1][r];
      }
      if (dr.thr) {
        drop_mul4(dr, drow + 32 * u + 4 * g, p[0], p[1], p[2], p[3]);
        drop_mul4(dr, drow + 32 * u + 16 + 4 * g, p[4], p[5], p[6], p[7]);
      }
      const uint32_t h01 = cvt_pk_bf16(p[0], p[1]), h23 = cvt_pk_bf16(p[2], p[3]);
      const uint32_t h45 = cvt_pk_bf16(p[4], p[5]), h67 = cvt_pk_bf16(p[6], p[7]);
      const uint32_t l01 = cvt_pk_bf16(p[0] - __uint_as_float(h01 << 16), p[1] - __uint_as_float(h01 & 0xffff0000u));
      const uint32_t l23 = cvt_pk_bf16(p[2] - __uint_as_float(h23 << 16), p[3] - __uint_as_float(h23 & 0xffff0000u));
      const uint32_t l45 = cvt_pk_bf16(p[4] - __uint_as_float(h45 << 16), p[5] - __uint_as_float(h45 & 0xffff0000u));
      const uint32_t l67 = cvt_pk_bf16(p[6] - __uint_as_float(h67 << 16), p[7] - __uint_as_float(h67 & 0xffff0000u));
      const bf16x8_t ph = __builtin_bit_cast(bf16x8_t, (u32x4_t{h01, h23, h45, h67}));
      const bf16x8_t pl = __builtin_bit_cast(bf16x8_t, (u32x4_t{l01, l23, l45, l67}));
      const int ra = 32 * u + 4 * g + tq, rb = ra + 16;
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const int unit = 2 * n + (tp >> 1), half8 = 8 * (tp & 1);
        const bf16x8_t vh = tr_pair(sV, ra, rb, unit, half8);
        const bf16x8_t vl = tr_pair(sV + PLANE, ra, rb, unit, half8);
        st.o[J][n] = mfma3(ph, pl, vh, vl, st.o[J][n]);
      }
    }
  }
  if constexpr (J + 1 < SLOTS)
    blocked_subtiles<NT, NW, SLOTS, J + 1>(st, Qh, lo_off, ld, row0, col0, sK, sV, sMask, sub_first, sub_step, n_sub, L, k0, scale,
                                           heads, b, h, dr, lane);
}

template <int SLOTS, int J>
__device__ __forceinline__ void blocked_finish(AttnState<SLOTS>& st, float* slab, int sub_first, int sub_step, int n_sub, int L,
                                               size_t row0, int col0, float* __restrict__ O, bf16_t* __restrict__ Oh,
                                               size_t o_lo_off, int ld_o, float* __restrict__ lse, int heads, int b, int h, int lane) {
  const int qn = lane & 15, g = lane >> 4;
  const int sub = sub_first + J * sub_step;
  if (sub < n_sub) {
    const float inv = 1.0f / st.l[J];
    const int q_row = sub * 16 + qn;
    if (lse && g == 0 && q_row < L) lse[((size_t)b * heads + h) * L + q_row] = st.m[J] + logf(st.l[J]);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float inv_r = __shfl(inv, 4 * g + r, 64);
#pragma unroll
      for (int n = 0; n < 4; ++n) slab[(4 * g + r) * (HD + 4) + 16 * n + qn] = st.o[J][n][r] * inv_r;
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
      const int r = pass * 4 + (lane >> 4), c = (lane & 15) * 4;
      const int qr = sub * 16 + r;
      if (qr < L) {
        const float4 v = *reinterpret_cast<const float4*>(slab + r * (HD + 4) + c);
        const size_t off = (row0 + qr) * (size_t)ld_o + col0 + c;
        if (O) *reinterpret_cast<float4*>(O + off) = v;
        if (Oh) store_planes4(Oh + off, o_lo_off, v);
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
  if constexpr (J + 1 < SLOTS)
    blocked_finish<SLOTS, J + 1>(st, slab, sub_first, sub_step, n_sub, L, row0, col0, O, Oh, o_lo_off, ld_o, lse, heads, b, h, lane);
}

template <int NT, int NW, int SLOTS>
__global__ __launch_bounds__(64 * NW) void self_attn_blocked_kernel(const bf16_t* __restrict__ Qh, const bf16_t* __restrict__ Kh,
                                                                const bf16_t* __restrict__ Vh, size_t lo_off, int ld,
                                                                const int64_t* __restrict__ seg, float* __restrict__ O,
                                                                bf16_t* __restrict__ Oh, size_t o_lo_off, int ld_o, int heads,
                                                                int L, float scale, float* __restrict__ lse, DropP dr,
                                                                int n_blocks) {
  constexpr int LP = 16 * NT;
  constexpr int PLANE = LP * ROW_B;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sK = smem;
  char* sV = smem + 2 * PLANE;
  float* sMask = reinterpret_cast<float*>(smem + 4 * PLANE);
  float* sOut = sMask + LP;
  const int h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t row0 = (size_t)b * L;
  const int col0 = h * HD;
  const int n_sub = (L + 15) >> 4;
  const int sub_first = blockIdx.x * NW + wave, sub_step = gridDim.x * NW;   // host: sub_first + SLOTS * sub_step >= n_sub
  AttnState<SLOTS> st;
#pragma unroll
  for (int j = 0; j < SLOTS; ++j) {
    st.m[j] = -INFINITY;
    st.l[j] = 0.f;
#pragma unroll
    for (int n = 0; n < 4; ++n) st.o[j][n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }
  for (int blk = 0; blk < n_blocks; ++blk) {
    const int k0 = blk * LP;
    if (blk) __syncthreads();                       // every wave is done reading the previous block
    constexpr int TRIPS = (LP * 8 + 64 * NW - 1) / (64 * NW);
    u32x4_t kh[TRIPS], kl[TRIPS], vh[TRIPS], vl[TRIPS];
#pragma unroll
    for (int it = 0; it < TRIPS; ++it) {
      const int i = tid + it * 64 * NW;
      const int r = i >> 3, u = i & 7;
      kh[it] = u32x4_t{0, 0, 0, 0};
      kl[it] = kh[it]; vh[it] = kh[it]; vl[it] = kh[it];
      if (i < LP * 8 && k0 + r < L) {
        const size_t o = (row0 + k0 + r) * (size_t)ld + col0 + u * 8;
        kh[it] = *reinterpret_cast<const u32x4_t*>(Kh + o);
        kl[it] = *reinterpret_cast<const u32x4_t*>(Kh + o + lo_off);
        vh[it] = *reinterpret_cast<const u32x4_t*>(Vh + o);
        vl[it] = *reinterpret_cast<const u32x4_t*>(Vh + o + lo_off);
      }
    }
#pragma unroll
    for (int it = 0; it < TRIPS; ++it) {
      const int i = tid + it * 64 * NW;
      const int r = i >> 3, u = i & 7;
      if (i < LP * 8) {
        *reinterpret_cast<u32x4_t*>(sK + k_off(r, u)) = kh[it];
        *reinterpret_cast<u32x4_t*>(sK + PLANE + k_off(r, u)) = kl[it];
        *reinterpret_cast<u32x4_t*>(sV + v_off(r, u)) = vh[it];
        *reinterpret_cast<u32x4_t*>(sV + PLANE + v_off(r, u)) = vl[it];
      }
    }
    for (int j = tid; j < LP; j += 64 * NW) sMask[j] = (k0 + j < L) ? ((seg[row0 + k0 + j] > 0) ? 0.f : -10000.0f) : -INFINITY;
    __syncthreads();
    blocked_subtiles<NT, NW, SLOTS, 0>(st, Qh, lo_off, ld, row0, col0, sK, sV, sMask, sub_first, sub_step, n_sub, L, k0, scale, heads,
                                       b, h, dr, lane);
  }
  blocked_finish<SLOTS, 0>(st, sOut + wave * 16 * (HD + 4), sub_first, sub_step, n_sub, L, row0, col0, O, Oh, o_lo_off, ld_o, lse,
                           heads, b, h, lane);
}

template <int NT>
int launch_fwd_persist(const AttnArgs& a, float* o, bf16_t* oh, size_t o_lo_off, int ld_o, float* lse) {
  constexpr int LP = 16 * NT;
  const size_t lds = (size_t)4 * LP * ROW_B + (size_t)2 * LP * 4 + (size_t)PS_MAX_SUB * 16 * (32 + 4) * 4;
  static bool done[2] = {false, false};
  static const char* const PERSIST_WHAT[2] = {"lr2_self_attn_fwd(persistent)", "lr2_self_attn_fwd(persistent, dropout)"};
  const int n_pairs = a.batch * a.heads;
  return launch_drop_form(a.dr.thr != 0, self_attn_persist_kernel<NT, false>, self_attn_persist_kernel<NT, true>, lds, lds, done,
                          PERSIST_WHAT, persist_grid(n_pairs), a.stream, a.q, a.k, a.v, a.lo_off, a.ld, a.seg, o, oh,
                          o_lo_off, ld_o, a.heads, a.L, a.scale, lse, a.dr, n_pairs,
                          (uint32_t)operand_span_bytes(a.batch, a.L, a.ld, a.heads));
}

// The one-pair forward: 8 waves per workgroup (2 per SIMD) hide the LDS-read latency of the dependent tile chains; a 256-key
// variant would keep 4 (its K/V planes + 8 output slabs would not fit the 160 KiB of LDS).
template <int NT>
int launch_fwd(const AttnArgs& a, float* o, bf16_t* oh, size_t o_lo_off, int ld_o, float* lse) {
  constexpr int LP = 16 * NT;
  constexpr int NW = NT <= 14 ? 8 : 4;
  if constexpr (NT <= 14)
    if (fwd_persist_ok(a.batch, a.heads, a.L, a.ld)) return launch_fwd_persist<NT>(a, o, oh, o_lo_off, ld_o, lse);
  const size_t lds = (size_t)4 * LP * ROW_B + (size_t)LP * 4 + (size_t)NW * 16 * (HD + 4) * 4;
  static bool done = false;
  if (allow_lds_once(self_attn_mfma_kernel<NT, NW>, lds, done, "self_attn_fwd")) return LR2_ERR_LAUNCH;
  const int n_sub = (a.L + 15) / 16, max_chunks = (n_sub + NW - 1) / NW;
  int chunks = attn_chunks(a.batch, a.heads, a.L);
  if (chunks > max_chunks) chunks = max_chunks;
  LR2_LAUNCH((self_attn_mfma_kernel<NT, NW>), dim3(chunks, a.heads, a.batch), dim3(64 * NW), lds, a.stream, a.q, a.k, a.v,
             a.lo_off, a.ld, a.seg, o, oh, o_lo_off, ld_o, a.heads, a.L, a.scale, lse, a.dr);
  return lr2_launch_status("lr2_self_attn_fwd");
}

// L > 256: key blocks of 16 * NT keys, nb = ceil(L / 224) blocks of equal (rounded) size; SLOTS sub-tiles of 16 queries per
// wave, the query range split over gridDim.x workgroups when a sequence has more than 8 * SLOTS sub-tiles.
template <int NT, int SLOTS>
int launch_fwd_blocked(const AttnArgs& a, float* o, bf16_t* oh, size_t o_lo_off, int ld_o, float* lse, int n_blocks) {
  constexpr int LP = 16 * NT, NW = 8;
  const size_t lds = (size_t)4 * LP * ROW_B + (size_t)LP * 4 + (size_t)NW * 16 * (HD + 4) * 4;
  static bool done = false;
  if (allow_lds_once(self_attn_blocked_kernel<NT, NW, SLOTS>, lds, done, "self_attn_fwd(blocked)")) return LR2_ERR_LAUNCH;
  const int n_sub = (a.L + 15) / 16;
  const int chunks = (n_sub + NW * SLOTS - 1) / (NW * SLOTS);
  LR2_LAUNCH((self_attn_blocked_kernel<NT, NW, SLOTS>), dim3(chunks, a.heads, a.batch), dim3(64 * NW), lds, a.stream, a.q, a.k, a.v,
             a.lo_off, a.ld, a.seg, o, oh, o_lo_off, ld_o, a.heads, a.L, a.scale, lse, a.dr, n_blocks);
  return lr2_launch_status("lr2_self_attn_fwd(blocked)");
}

// (tests/attn_cases.py::fwd_block restates this choice of the block length for the mask patterns of tests/test_attention_edges_gpu.py
// and DESIGN.md 4.5 tabulates it: keep the three in step.)
static int fwd_blocked_dispatch(const AttnArgs& a, float* o, bf16_t* oh, size_t o_lo_off, int ld_o, float* lse) {
  const int nb = (a.L + 223) / 224;
  const int tiles = (((a.L + nb - 1) / nb) + 15) / 16;       // key tiles per block
  const int n_sub = (a.L + 15) / 16;
  const bool few = n_sub <= 8 * 3;                           // 3 sub-tile slots per wave are enough (L <= 384); else 4 (+ query chunks)
#define BLK(NT)                                                                                        \
  return few ? launch_fwd_blocked<NT, 3>(a, o, oh, o_lo_off, ld_o, lse, (a.L + 16 * NT - 1) / (16 * NT)) \
             : launch_fwd_blocked<NT, 4>(a, o, oh, o_lo_off, ld_o, lse, (a.L + 16 * NT - 1) / (16 * NT));
  if (tiles <= 10) { BLK(10) }
  if (tiles <= 12) { BLK(12) }
  // 14 key tiles: 3 query sub-tiles per wave always (the 4-slot variant needs 11 VGPRs more than the 256 of two waves per SIMD)
  return launch_fwd_blocked<14, 3>(a, o, oh, o_lo_off, ld_o, lse, (a.L + 16 * 14 - 1) / (16 * 14));
#undef BLK
}

}  // namespace

extern "C" int lr2_self_attn_fwd(const void* q_hi, const void* k_hi, const void* v_hi, uint64_t lo_off, int ld,
                                 const int64_t* seg, void* o, void* o_hi, uint64_t o_lo_off, int ld_o, void* lse, float drop_p,
                                 uint64_t drop_seed, uint32_t drop_site, int batch, int heads, int L, int head_dim, float scale,
                                 void* stream) {
  if (!q_hi || !k_hi || !v_hi || !seg || (!o && !o_hi) || batch <= 0 || heads <= 0) return LR2_ERR_ARG;
  if (head_dim != HD || L < 1 || ld % 8 || ld_o % 4 || lo_off % 8 || o_lo_off % 4) return LR2_ERR_SHAPE;
  if (drop_p < 0.f || drop_p >= 1.f) return LR2_ERR_ARG;
  const AttnArgs a{(const bf16_t*)q_hi, (const bf16_t*)k_hi, (const bf16_t*)v_hi, (size_t)lo_off, ld, seg, batch, heads, L,
                   scale, make_drop(drop_p, drop_seed, drop_site), (hipStream_t)stream};
  // L > 224: key blocks with a running max / sum.  (A one-block kernel for 225 <= L <= 256 -- 16 key tiles, 4 waves -- needs
  // 512 VGPRs + 710 spilled: the two-block walk of the blocked kernel is the forward for those lengths.)
  if (L > 224) return fwd_blocked_dispatch(a, (float*)o, (bf16_t*)o_hi, (size_t)o_lo_off, ld_o, (float*)lse);
  if (L <= 64) return launch_fwd<4>(a, (float*)o, (bf16_t*)o_hi, (size_t)o_lo_off, ld_o, (float*)lse);
  if (L <= 128) return launch_fwd<8>(a, (float*)o, (bf16_t*)o_hi, (size_t)o_lo_off, ld_o, (float*)lse);
  return launch_fwd<14>(a, (float*)o, (bf16_t*)o_hi, (size_t)o_lo_off, ld_o, (float*)lse);
}
