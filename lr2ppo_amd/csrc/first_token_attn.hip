// ---------------------------------------------------------------------------------------------------------------------
// Attention for the FIRST query of every sequence only (the [CLS] row): what pooling 'first' (utils/misc.py:23-35 upstream)
// keeps of the last encoder layer.  One workgroup per (sequence, head): scores of the one query against all L keys,
// fp32 softmax with the same additive key mask and the same exp as the full kernels, then P V.  K / V rows are read as
// whole 128-B hi and lo rows (bf16 planes, x = hi + lo).  ~0.2 % of the full layer's attention work: a vector kernel.
// ---------------------------------------------------------------------------------------------------------------------

#include "selfattn_common.h"

namespace {

constexpr int FT_THREADS = 256;
constexpr int FT_MAXL = 4096;

__device__ __forceinline__ float bf_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf_hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }

__global__ __launch_bounds__(FT_THREADS) void first_token_attn_kernel(const float* __restrict__ q, int ld_q,
                                                                       const bf16_t* __restrict__ k_hi,
                                                                       const bf16_t* __restrict__ v_hi, size_t lo_off, int ld,
                                                                       const int64_t* __restrict__ seg, float* __restrict__ o,
                                                                       int ld_o, int heads, int L, float scale) {
  // Round 4: 8 threads per key row (16 B of the hi plane + 16 B of the lo plane each: the 128-byte row segment of a head is one
  // coalesced request), 32 rows per sweep of the workgroup, for the scores AND for P V -- the first version read a row per thread
  // (64 cache lines per wave instruction) and V two bytes per lane: 245 us at 512 x 12 x 197 = 2.5 TB/s.
  __shared__ float sq[HD];
  __shared__ float sp[FT_MAXL];
  __shared__ float red[FT_THREADS / 64];
  __shared__ float so[FT_THREADS / 8][HD + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int rr = tid >> 3, c8 = (tid & 7) * 8;            // row within a sweep, first of this thread's 8 head columns
  const int b = blockIdx.x / heads, h = blockIdx.x % heads;
  const size_t row0 = (size_t)b * L;
  if (tid < HD) sq[tid] = q[(size_t)b * ld_q + h * HD + tid];
  __syncthreads();
  float qv[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) qv[i] = sq[c8 + i];
  float mx = -INFINITY;
  for (int j0 = 0; j0 < L; j0 += FT_THREADS / 8) {
    const int j = j0 + rr;
    float acc = 0.f;
    if (j < L) {
      const bf16_t* kr = k_hi + (row0 + j) * (size_t)ld + h * HD + c8;
      const u32x4_t hv = *reinterpret_cast<const u32x4_t*>(kr);
      const u32x4_t lv = *reinterpret_cast<const u32x4_t*>(kr + lo_off);
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        acc = __builtin_fmaf(qv[2 * w], bf_lo(hv[w]) + bf_lo(lv[w]), acc);
        acc = __builtin_fmaf(qv[2 * w + 1], bf_hi(hv[w]) + bf_hi(lv[w]), acc);
      }
    }
    // the row's 8 partial sums sit in 8 consecutive lanes
    acc += __shfl_xor(acc, 1, 64);
    acc += __shfl_xor(acc, 2, 64);
    acc += __shfl_xor(acc, 4, 64);
    if (j < L) {
      const float sc = acc * scale + ((seg[row0 + j] > 0) ? 0.f : -10000.0f);
      if ((tid & 7) == 0) sp[j] = sc;
      mx = fmaxf(mx, sc);
    }
  }
  mx = wave_max(mx);
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float sum = 0.f;
  for (int j = tid; j < L; j += FT_THREADS) {
    const float e = exp_fast(sp[j] - mx);
    sp[j] = e;
    sum += e;
  }
  sum = wave_sum(sum);
  if (lane == 0) red[wave] = sum;
  __syncthreads();
  sum = (red[0] + red[1]) + (red[2] + red[3]);
  // O = P V: thread (rr, c8) sums its 8 columns over the rows rr, rr + 32, ...; the 32 row groups are combined through LDS
  float ov[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) ov[i] = 0.f;
  for (int j = rr; j < L; j += FT_THREADS / 8) {
    const bf16_t* vr = v_hi + (row0 + j) * (size_t)ld + h * HD + c8;
    const u32x4_t hv = *reinterpret_cast<const u32x4_t*>(vr);
    const u32x4_t lv = *reinterpret_cast<const u32x4_t*>(vr + lo_off);
    const float pj = sp[j];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      ov[2 * w] = __builtin_fmaf(pj, bf_lo(hv[w]) + bf_lo(lv[w]), ov[2 * w]);
      ov[2 * w + 1] = __builtin_fmaf(pj, bf_hi(hv[w]) + bf_hi(lv[w]), ov[2 * w + 1]);
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) so[rr][c8 + i] = ov[i];
  __syncthreads();
  if (tid < HD) {
    float t = 0.f;
#pragma unroll
    for (int r = 0; r < FT_THREADS / 8; ++r) t += so[r][tid];
    o[(size_t)b * ld_o + h * HD + tid] = t / sum;
  }
}

}  // namespace

extern "C" int lr2_first_token_attn(const void* q, int ld_q, const void* k_hi, const void* v_hi, uint64_t lo_off, int ld,
                                    const int64_t* seg, void* o, int ld_o, int batch, int heads, int L, int head_dim,
                                    float scale, void* stream) {
  if (!q || !k_hi || !v_hi || !seg || !o || batch <= 0 || heads <= 0) return LR2_ERR_ARG;
  if (head_dim != HD || L < 1 || L > FT_MAXL || ld % 8 || lo_off % 8) return LR2_ERR_SHAPE;
  LR2_LAUNCH(first_token_attn_kernel, dim3(batch * heads), dim3(FT_THREADS), 0, (hipStream_t)stream, (const float*)q, ld_q,
             (const bf16_t*)k_hi, (const bf16_t*)v_hi, (size_t)lo_off, ld, seg, (float*)o, ld_o, heads, L, scale);
  return lr2_launch_status(__func__);
}
