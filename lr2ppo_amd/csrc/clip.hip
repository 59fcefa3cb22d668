// Global gradient-norm clipping on the device (torch.nn.utils.clip_grad_norm_, norm_type = 2, error_if_nonfinite = False):
//
//   sumsq     one workgroup per chunk of the AdamW chunk table: sum of g^2 in fp64 -> one partial per chunk.
//   gram_dot  sum_ij A_ij B_ij of two fp32 [n, n] matrices in fp64, times a by-value factor -> one slot.  With the Gram matrices of
//             the two thin factors of out_layer.fc1's gradient (dW = alpha dzo^T flat) this is ||dW||_F^2 = alpha^2 sum_ij
//             (dzo dzo^T)_ij (flat flat^T)_ij: the 2 GB gradient the fused update never writes is not needed for its norm.
//   coef      one workgroup adds the partials and slots in index order; total_norm and min(1, max_norm / (total_norm + 1e-6)) leave as
//             two fp32 values, formed in fp64 and rounded once.
//   adamw_multi_scaled   the multi-tensor AdamW on g * coef (one fp32 multiply of its own, then common.h::adam_update).
//
// Every sum has a fixed order (a thread's own elements in index order, lane tree, waves in index order, as adafactor.hip's
// block_sum): no atomics, equal bits from run to run.  Squares and products of fp32 values are exact in fp64; only the additions round.
// 16-byte loads where a chunk's pointers allow them, element loads (still 256 B per wave instruction) otherwise.
#include "common.h"
#include "lr2ppo_hip.h"

namespace {

constexpr int NT = 256, NW = NT / 64;

struct Chunk {
  float* p;
  const float* g;
  float* m;
  float* v;
  uint64_t count;
  float wd;
  float pad;
};
static_assert(sizeof(Chunk) == sizeof(lr2_adamw_chunk), "chunk layout");

__device__ __forceinline__ double wave_sum_f64(double v) {      // xor tree: every lane ends with the same bits
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
// sum over the workgroup, waves in index order; every thread gets the result.  red: NW doubles
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
  v = wave_sum_f64(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) s += red[w];
  return s;
}
__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

__global__ __launch_bounds__(NT) void clip_sumsq_kernel(const Chunk* __restrict__ table, double* __restrict__ partials) {
  __shared__ double red[NW];
  const float* __restrict__ g = table[blockIdx.x].g;
  const uint64_t count = table[blockIdx.x].count;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  uint64_t done = 0;
  if (aligned16(g)) {           // uniform over the workgroup
    const uint64_t n4 = count / 4;
    const float4* g4 = reinterpret_cast<const float4*>(g);
    for (uint64_t i = threadIdx.x; i < n4; i += NT) {
      const float4 x = g4[i];
      a0 += (double)x.x * (double)x.x;
      a1 += (double)x.y * (double)x.y;
      a2 += (double)x.z * (double)x.z;
      a3 += (double)x.w * (double)x.w;
    }
    done = n4 * 4;
  }
  for (uint64_t i = done + threadIdx.x; i < count; i += NT) {
    const double x = (double)g[i];
    a0 += x * x;
  }
  const double s = block_sum_f64((a0 + a1) + (a2 + a3), red);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(NT) void clip_gram_dot_kernel(const float* __restrict__ A, const float* __restrict__ B, int n, int ld_a,
                                                           int ld_b, double factor, double* __restrict__ slot) {
  __shared__ double red[NW];
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if ((n % 4) == 0 && (ld_a % 4) == 0 && (ld_b % 4) == 0 && aligned16(A) && aligned16(B)) {
    const uint64_t q_row = (uint64_t)(n / 4), total = q_row * (uint64_t)n;
    for (uint64_t q = threadIdx.x; q < total; q += NT) {
      const uint64_t r = q / q_row, c = (q % q_row) * 4;
      const float4 x = *reinterpret_cast<const float4*>(A + r * (uint64_t)ld_a + c);
      const float4 y = *reinterpret_cast<const float4*>(B + r * (uint64_t)ld_b + c);
      a0 += (double)x.x * (double)y.x;
      a1 += (double)x.y * (double)y.y;
      a2 += (double)x.z * (double)y.z;
      a3 += (double)x.w * (double)y.w;
    }
  } else {
    const uint64_t total = (uint64_t)n * (uint64_t)n;
    for (uint64_t i = threadIdx.x; i < total; i += NT) {
      const uint64_t r = i / (uint64_t)n, c = i % (uint64_t)n;
      a0 += (double)A[r * (uint64_t)ld_a + c] * (double)B[r * (uint64_t)ld_b + c];
    }
  }
  const double s = block_sum_f64((a0 + a1) + (a2 + a3), red);
  if (threadIdx.x == 0) *slot = factor * s;
}

// slots[0..n) added in index order: staged through LDS 256 at a time (parallel loads), added by one thread (a few thousand
// dependent fp64 additions, once per step).  out[0] = total_norm, out[1] = coef.
__global__ __launch_bounds__(NT) void clip_coef_kernel(const double* __restrict__ slots, int n, double max_norm,
                                                       float* __restrict__ out) {
  __shared__ double buf[NT];
  double s = 0.0;
  for (int base = 0; base < n; base += NT) {
    const int here = min(NT, n - base);
    if ((int)threadIdx.x < here) buf[threadIdx.x] = slots[base + threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0)
      for (int i = 0; i < here; ++i) s += buf[i];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double total = sqrt(s);
    const double c = max_norm / (total + 1e-6);
    const double coef = c < 1.0 ? c : (c != c ? c : 1.0);       // clamp(c, max = 1): a NaN stays a NaN
    out[0] = (float)total;
    out[1] = (float)coef;
  }
}

__global__ __launch_bounds__(NT) void adamw_scaled_kernel(const Chunk* __restrict__ table, float lr_host, float b1, float b2, float ob1,
                                                          float ob2, float eps, const float* __restrict__ lr_dev,
                                                          const float* __restrict__ gscale_dev) {
  const float lr = lr_dev ? scalar_load_f32(lr_dev) : lr_host;
  const float coef = scalar_load_f32(gscale_dev);
  const Chunk c = table[blockIdx.x];
#define ADAM1(P, G, M, V) adam_update(P, __fmul_rn(G, coef), M, V, lr, b1, b2, ob1, ob2, eps, c.wd);
  uint64_t done = 0;
  if (aligned16(c.p) && aligned16(c.g) && aligned16(c.m) && aligned16(c.v)) {
    const uint64_t n4 = c.count / 4;
    float4* p4 = reinterpret_cast<float4*>(c.p);
    const float4* g4 = reinterpret_cast<const float4*>(c.g);
    float4* m4 = reinterpret_cast<float4*>(c.m);
    float4* v4 = reinterpret_cast<float4*>(c.v);
    for (uint64_t i = threadIdx.x; i < n4; i += NT) {
      float4 p = p4[i], g = g4[i], m = m4[i], v = v4[i];
      ADAM1(p.x, g.x, m.x, v.x) ADAM1(p.y, g.y, m.y, v.y) ADAM1(p.z, g.z, m.z, v.z) ADAM1(p.w, g.w, m.w, v.w)
      p4[i] = p; m4[i] = m; v4[i] = v;
    }
    done = n4 * 4;
  }
  for (uint64_t i = done + threadIdx.x; i < c.count; i += NT) {
    float p = c.p[i], g = c.g[i], m = c.m[i], v = c.v[i];
    ADAM1(p, g, m, v)
    c.p[i] = p; c.m[i] = m; c.v[i] = v;
  }
#undef ADAM1
}

}  // namespace

#define CHECK_LAUNCH() return lr2_launch_status(__func__)

extern "C" int lr2_clip_sumsq(const lr2_adamw_chunk* table_dev, int n_chunks, void* partials_dev, void* stream) {
  if (!table_dev || n_chunks <= 0 || !partials_dev || misaligned(partials_dev, 8)) return LR2_ERR_ARG;
  LR2_LAUNCH(clip_sumsq_kernel, dim3(n_chunks), dim3(NT), 0, (hipStream_t)stream, (const Chunk*)table_dev, (double*)partials_dev);
  CHECK_LAUNCH();
}

extern "C" int lr2_clip_gram_dot(const void* A, const void* B, int n, int ld_a, int ld_b, double factor, void* slot_dev,
                                 void* stream) {
  if (!A || !B || n <= 0 || ld_a < n || ld_b < n || !slot_dev || misaligned(slot_dev, 8) || misaligned(A, 4) || misaligned(B, 4))
    return LR2_ERR_ARG;
  LR2_LAUNCH(clip_gram_dot_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, (const float*)A, (const float*)B, n, ld_a, ld_b, factor,
             (double*)slot_dev);
  CHECK_LAUNCH();
}

extern "C" int lr2_clip_coef(const void* slots_dev, int n, double max_norm, void* out_dev, void* stream) {
  if (!slots_dev || n <= 0 || !out_dev || misaligned(slots_dev, 8) || misaligned(out_dev, 4) || !(max_norm >= 0.0)) return LR2_ERR_ARG;
  LR2_LAUNCH(clip_coef_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, (const double*)slots_dev, n, max_norm, (float*)out_dev);
  CHECK_LAUNCH();
}

extern "C" int lr2_adamw_multi_scaled(const lr2_adamw_chunk* table_dev, int n_chunks, double lr, double beta1, double beta2,
                                      double eps, const void* lr_dev, const void* gscale_dev, void* stream) {
  if (!table_dev || n_chunks <= 0 || !gscale_dev || misaligned(gscale_dev, 4)) return LR2_ERR_ARG;
  // the same double -> float conversions as lr2_adamw_multi
  LR2_LAUNCH(adamw_scaled_kernel, dim3(n_chunks), dim3(NT), 0, (hipStream_t)stream, (const Chunk*)table_dev, (float)lr, (float)beta1,
             (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, (const float*)lr_dev, (const float*)gscale_dev);
  CHECK_LAUNCH();
}
