// Operands of the MX-FP8 training mode (FeatureExtractor(precision="mxfp8_train")): the backward's products reduce over the token axis
// (weight gradients dW = dY^T . X) or over output features (input gradients dX = dY . W), so their MX blocks run down COLUMNS of the
// matrices the forward and the backward produce.
//
//   lr2_quant_mxfp8_t   : x [rows, cols] (fp32, or bf16 hi / lo planes) -> MX-FP8 of x^T [cols, rows_pad] (+ the row-blocked MX-FP8 of x,
//                         + the column sums of x), with an optional GELU / GELU' prologue.  One read of x feeds both products.
//   lr2_dropout_residual: out = resid + dropout(y) -- the split-bf16 products' fused dropout + residual epilogue, after an MX product.
#include "common.h"
#include "lr2ppo_hip.h"

namespace {

// 32 values -> 32 e4m3fn bytes by common.h's block rule, four per word in element order
__device__ __forceinline__ void mx_pack32(const float (&v)[32], float inv, int (&w)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) w[j] = mx_pack4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3], inv);
}

struct QuantTParams {
  const float* x;          // fp32 input [rows, ld] ...
  const bf16_t* hi;        // ... or bf16 hi / lo planes (lo plane lo_off elements behind hi), row stride ld
  size_t lo_off;
  int ld;
  const float* z;          // act 2: GELU'(z) factor, z [rows, ld_z]
  int ld_z, act;           // act 0: x; 1: GELU(x); 2: x * GELU'(z)
  uint8_t* qt;             // optional [cols, rows_pad] e4m3 bytes of x^T ...
  uint8_t* st;             // ... and [cols, rows_pad / 32] scale bytes
  uint8_t* q;              // optional [rows, cols] row-blocked bytes ...
  uint8_t* s;              // ... and [rows, cols / 32] scales
  float* partials;         // optional [rows_pad / 128, cols]: per 128-row tile column sums
  int rows, cols, rows_pad;
};

// One workgroup per 128 rows x 64 columns tile, staged through LDS as fp32 after the prologue.  Column-blocked: thread (column
// tid & 63, 32-row block tid >> 6) quantises 32 values down its column and stores 32 consecutive bytes of a row of x^T.  Row-blocked:
// thread (row tid >> 1, 32-column half tid & 1) quantises along the row exactly as quant_mxfp8_kernel does.  Rows past `rows` are
// zeros: zero bytes, scale byte 0.
__global__ __launch_bounds__(256) void quant_mxfp8_t_kernel(QuantTParams p) {
  __shared__ float tile[128][65];
  __shared__ float red[4][64];
  const int tid = threadIdx.x;
  const int c0 = blockIdx.x * 64, r0 = blockIdx.y * 128;
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    const int r = 16 * it + (tid >> 4), c = 4 * (tid & 15), gr = r0 + r;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (gr < p.rows) {
      if (p.x) {
        v = *reinterpret_cast<const float4*>(p.x + (size_t)gr * p.ld + c0 + c);
      } else {
        const bf16_t* h = p.hi + (size_t)gr * p.ld + c0 + c;
        const uint2 hv = *reinterpret_cast<const uint2*>(h), lv = *reinterpret_cast<const uint2*>(h + p.lo_off);
        v = make_float4(bf2f((bf16_t)(hv.x & 0xFFFF)) + bf2f((bf16_t)(lv.x & 0xFFFF)), bf2f((bf16_t)(hv.x >> 16)) + bf2f((bf16_t)(lv.x >> 16)),
                        bf2f((bf16_t)(hv.y & 0xFFFF)) + bf2f((bf16_t)(lv.y & 0xFFFF)), bf2f((bf16_t)(hv.y >> 16)) + bf2f((bf16_t)(lv.y >> 16)));
      }
      if (p.act == 1) {
        v = make_float4(gelu_erf(v.x), gelu_erf(v.y), gelu_erf(v.z), gelu_erf(v.w));
      } else if (p.act == 2) {
        const float4 z = *reinterpret_cast<const float4*>(p.z + (size_t)gr * p.ld_z + c0 + c);
        v.x *= gelu_erf_grad(z.x); v.y *= gelu_erf_grad(z.y); v.z *= gelu_erf_grad(z.z); v.w *= gelu_erf_grad(z.w);
      }
    }
    tile[r][c] = v.x; tile[r][c + 1] = v.y; tile[r][c + 2] = v.z; tile[r][c + 3] = v.w;
  }
  __syncthreads();
  if (p.qt || p.partials) {
    const int c = tid & 63, b = tid >> 6;
    float v[32];
    float amax = 0.f, sum = 0.f;
#pragma unroll
    for (int k = 0; k < 32; ++k) {
      v[k] = tile[32 * b + k][c];
      amax = fmaxf(amax, fabsf(v[k]));
      sum += v[k];
    }
    if (p.qt) {
      const int e = mx_exponent(amax);
      int w[8];
      mx_pack32(v, mx_inverse(e), w);
      int4* dq = reinterpret_cast<int4*>(p.qt + (size_t)(c0 + c) * p.rows_pad + r0 + 32 * b);
      dq[0] = make_int4(w[0], w[1], w[2], w[3]);
      dq[1] = make_int4(w[4], w[5], w[6], w[7]);
      p.st[(size_t)(c0 + c) * (p.rows_pad / 32) + r0 / 32 + b] = (uint8_t)(e + 127);
    }
    if (p.partials) red[b][c] = sum;
  }
  if (p.q) {
    const int r = tid >> 1, hf = tid & 1, gr = r0 + r;
    if (gr < p.rows) {
      float v[32];
      float amax = 0.f;
#pragma unroll
      for (int k = 0; k < 32; ++k) {
        v[k] = tile[r][32 * hf + k];
        amax = fmaxf(amax, fabsf(v[k]));
      }
      const int e = mx_exponent(amax);
      int w[8];
      mx_pack32(v, mx_inverse(e), w);
      int4* dq = reinterpret_cast<int4*>(p.q + (size_t)gr * p.cols + c0 + 32 * hf);
      dq[0] = make_int4(w[0], w[1], w[2], w[3]);
      dq[1] = make_int4(w[4], w[5], w[6], w[7]);
      p.s[(size_t)gr * (p.cols / 32) + c0 / 32 + hf] = (uint8_t)(e + 127);
    }
  }
  if (p.partials) {
    __syncthreads();
    if (tid < 64) p.partials[(size_t)blockIdx.y * p.cols + c0 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
  }
}

__global__ __launch_bounds__(256) void dropout_residual_kernel(const float* __restrict__ y, const float* __restrict__ resid,
                                                               float* __restrict__ out, size_t n4, float scale, uint32_t thr, uint64_t key) {
#pragma clang fp contract(off)
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    float4 v = dropout_apply4(key, (uint64_t)i * 4, thr, scale, reinterpret_cast<const float4*>(y)[i]);
    const float4 r = reinterpret_cast<const float4*>(resid)[i];
    v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
    reinterpret_cast<float4*>(out)[i] = v;
  }
}

}  // namespace

extern "C" int lr2_quant_mxfp8_t(const void* x, int is_planes, uint64_t lo_off, int ldx, const void* z, int ld_z, int act, void* qt,
                                 void* st, void* q, void* scales, void* colsum, void* partials, int accumulate, int rows, int cols,
                                 void* stream) {
  if (!x || (!qt && !q) || rows <= 0 || cols <= 0 || act < 0 || act > 2 || (is_planes != 0 && is_planes != 1) ||
      (accumulate != 0 && accumulate != 1))
    return LR2_ERR_ARG;
  if ((qt != nullptr) != (st != nullptr) || (q != nullptr) != (scales != nullptr) || (colsum != nullptr) != (partials != nullptr) ||
      (act == 2 && !z))
    return LR2_ERR_ARG;
  if (cols % 64 || ldx < cols || ldx % 4 || (is_planes && lo_off % 4) || (act == 2 && (ld_z < cols || ld_z % 4))) return LR2_ERR_SHAPE;
  // vector accesses: x / z as float4 (planes: 4 x bf16 = 8 bytes per plane), 16-byte stores of e4m3 bytes
  if ((uintptr_t)x % (is_planes ? 8 : 16) || (act == 2 && (uintptr_t)z % 16) || (uintptr_t)qt % 16 || (uintptr_t)q % 16)
    return LR2_ERR_SHAPE;
  const int rows_pad = (rows + 127) / 128 * 128;
  QuantTParams p{is_planes ? nullptr : (const float*)x, is_planes ? (const bf16_t*)x : nullptr, (size_t)lo_off, ldx, (const float*)z,
                 ld_z, act, (uint8_t*)qt, (uint8_t*)st, (uint8_t*)q, (uint8_t*)scales, (float*)partials, rows, cols, rows_pad};
  LR2_LAUNCH(quant_mxfp8_t_kernel, dim3(cols / 64, rows_pad / 128), dim3(256), 0, (hipStream_t)stream, p);
  if (lr2_launch_status(__func__)) return LR2_ERR_LAUNCH;
  if (colsum) return lr2_colsum_partials_finish(partials, rows_pad / 128, cols, cols, colsum, accumulate, stream);
  return 0;
}

extern "C" int lr2_dropout_residual(const void* y, const void* resid, void* out, uint64_t n, float drop_p, uint64_t drop_seed,
                                    uint32_t drop_site, void* stream) {
  if (!y || !resid || !out || n == 0 || drop_p <= 0.f || drop_p >= 1.f) return LR2_ERR_ARG;
  if (n % 4 || (uintptr_t)y % 16 || (uintptr_t)resid % 16 || (uintptr_t)out % 16) return LR2_ERR_SHAPE;
  size_t blocks = (n / 4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  LR2_LAUNCH(dropout_residual_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const float*)y, (const float*)resid,
             (float*)out, (size_t)(n / 4), 1.0f / (1.0f - drop_p), dropout_threshold(drop_p),
             (((uint64_t)drop_site) << 40) ^ (drop_seed * 0x9E3779B97F4A7C15ull));
  return lr2_launch_status(__func__);
}
