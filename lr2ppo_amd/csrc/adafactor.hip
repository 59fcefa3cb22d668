// Multi-tensor Adafactor (tencentpretrain/utils/optimizers.py:518-603 with relative_step=False, scale_parameter=False, beta1=None):
// the factored second moment of 2-D tensors, the plain one of 1-D tensors, the per-tensor RMS clip, decay and update, in four
// table-driven launches per param group whatever the number of tensors (lr2_adafactor_multi in include/lr2ppo_hip.h).
//
//   stats     u = g*g + eps0; a workgroup owns one 512 x 1024 tile: a wave takes one row at a time (16 elements per lane), keeps
//             the 16 column sums of its lanes in fp64 registers and reduces the row sum across its lanes; the 8 waves' column sums
//             meet in LDS.  Partials leave as fp32: [col tiles][rows] and [row tiles][cols] -- 5.9 MB at [3072, 162816].
//   finalise  partials summed in tile order in fp64, the EMA into row / col, mean(row).
//   update^2  U = g * rsqrt(row / mean(row))[i] * rsqrt(col)[j]; sum of U^2 per tile in fp64.
//   apply     the tensor's partials summed in tile order -> rms -> clip; p += (-wd*lr) p; p -= lr * U / clip.
//
// Every sum has a fixed order (lane tree, then waves / tiles in index order): no atomics, equal bits from run to run.  Traffic of a
// 2-D tensor: g three times, p in and out = 20 B per parameter.  16-byte accesses only for tensors whose pointers are 16-byte
// aligned and whose cols % 4 == 0 (every row then starts aligned); element accesses (still 256 B per wave instruction) otherwise.
#include "common.h"
#include "lr2ppo_hip.h"

namespace {

constexpr int TR = LR2_ADAFACTOR_TILE_ROWS, TC = LR2_ADAFACTOR_TILE_COLS, CH1 = LR2_ADAFACTOR_CHUNK_1D;
constexpr int NT = 512, NW = NT / 64, PER = TC / 64;   // threads, waves, elements per lane and row
static_assert(PER == 16 && CH1 == NT * PER, "a lane owns 16 elements of a tile row / a thread 16 of a 1-D chunk");

struct Tensor {
  float* p;
  const float* g;
  float* row;
  float* col;
  uint64_t rows, cols, ws_row, ws_col, ws_mean, ws_sq;
  uint32_t n_tiles, n_ct, n_rt, pad;
  double wd;
};
struct Tile {
  uint32_t tensor, index;
};
struct Fin {
  uint32_t tensor, kind;
  uint64_t start;
};
static_assert(sizeof(Tensor) == sizeof(lr2_adafactor_tensor) && sizeof(Tile) == sizeof(lr2_adafactor_tile) &&
                  sizeof(Fin) == sizeof(lr2_adafactor_fin), "table layouts");

// column (within the tile) of slot k of a lane: four float4 per lane in the aligned form, 16 strided elements otherwise
template <bool VEC>
__device__ __forceinline__ uint32_t slot_col(int lane, int k) {
  return VEC ? 256u * (k >> 2) + 4u * lane + (k & 3) : 64u * k + lane;
}
template <bool VEC>
__device__ __forceinline__ void load_row(const float* __restrict__ src, uint32_t ncols, int lane, float (&x)[PER]) {
  if (VEC) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t c = 256u * q + 4u * lane;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c < ncols) v = *reinterpret_cast<const float4*>(src + c);     // ncols % 4 == 0: a float4 is inside or outside as a whole
      x[4 * q] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const uint32_t c = 64u * k + lane;
      x[k] = c < ncols ? src[c] : 0.f;
    }
  }
}
template <bool VEC>
__device__ __forceinline__ void store_row(float* __restrict__ dst, uint32_t ncols, int lane, const float (&x)[PER]) {
  if (VEC) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t c = 256u * q + 4u * lane;
      if (c < ncols) *reinterpret_cast<float4*>(dst + c) = make_float4(x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const uint32_t c = 64u * k + lane;
      if (c < ncols) dst[c] = x[k];
    }
  }
}

__device__ __forceinline__ double wave_sum(double v) {      // xor tree: every lane ends with the same bits
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
// sum over the workgroup, waves in index order; every thread gets the result.  red: NW doubles
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum(v);
  __syncthreads();                                          // red may still be read from an earlier call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) s += red[w];
  return s;
}

__device__ __forceinline__ float rsqrt_ref(float x) { return 1.0f / sqrtf(x); }      // torch's CPU rsqrt: two rounded operations
__device__ __forceinline__ float ema(float old, float b2, float omb, float m) {       // old.mul_(b2).add_(omb * m)
  return __fadd_rn(__fmul_rn(old, b2), __fmul_rn(omb, m));
}

struct Geom {
  uint64_t i0, j0;
  uint32_t nrows, ncols;
};
__device__ __forceinline__ Geom tile_geom(const Tensor& t, uint32_t index) {
  Geom g;
  g.i0 = (uint64_t)(index / t.n_ct) * TR;
  g.j0 = (uint64_t)(index % t.n_ct) * TC;
  g.nrows = (uint32_t)(t.rows - g.i0 < (uint64_t)TR ? t.rows - g.i0 : (uint64_t)TR);
  g.ncols = (uint32_t)(t.cols - g.j0 < (uint64_t)TC ? t.cols - g.j0 : (uint64_t)TC);
  return g;
}
__device__ __forceinline__ bool aligned16(const void* a, uint64_t cols) { return (((uintptr_t)a) & 15) == 0 && (cols & 3) == 0; }

// 1-D chunk: element e of thread tid is start + tid + NT * k
struct Chunk {
  uint64_t start;
  uint32_t n;
};
__device__ __forceinline__ Chunk chunk_geom(const Tensor& t, uint32_t index) {
  Chunk c;
  c.start = (uint64_t)index * CH1;
  c.n = (uint32_t)(t.cols - c.start < (uint64_t)CH1 ? t.cols - c.start : (uint64_t)CH1);
  return c;
}

// ------------------------------------------------------------------------------------------------ 1: stats
template <bool VEC>
__device__ __forceinline__ void stats_tile(const Tensor& t, uint32_t index, char* ws, float eps0, float* sCol) {
  const Geom gm = tile_geom(t, index);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double cacc[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) cacc[k] = 0.0;
  float* rowpart = reinterpret_cast<float*>(ws + t.ws_row) + (uint64_t)(index % t.n_ct) * t.rows + gm.i0;
  for (uint32_t r = wave; r < gm.nrows; r += NW) {
    float x[PER];
    load_row<VEC>(t.g + (gm.i0 + r) * t.cols + gm.j0, gm.ncols, lane, x);
    double racc = 0.0;
#pragma unroll
    for (int k = 0; k < PER; ++k)
      if (slot_col<VEC>(lane, k) < gm.ncols) {
        const double u = (double)__fadd_rn(__fmul_rn(x[k], x[k]), eps0);
        cacc[k] += u;
        racc += u;
      }
    racc = wave_sum(racc);
    if (lane == 0) rowpart[r] = (float)racc;
  }
#pragma unroll
  for (int k = 0; k < PER; ++k) sCol[wave * TC + k * 64 + lane] = (float)cacc[k];
  __syncthreads();
  float* colpart = reinterpret_cast<float*>(ws + t.ws_col) + (uint64_t)(index / t.n_ct) * t.cols + gm.j0;
  for (int s = threadIdx.x; s < TC; s += NT) {
    const uint32_t c = slot_col<VEC>(s & 63, s >> 6);
    if (c < gm.ncols) {
      double a = 0.0;
#pragma unroll
      for (int w = 0; w < NW; ++w) a += (double)sCol[w * TC + s];
      colpart[c] = (float)a;
    }
  }
}

__global__ __launch_bounds__(NT) void adafactor_stats_kernel(const Tensor* __restrict__ tensors, const Tile* __restrict__ tiles,
                                                             char* __restrict__ ws, float eps0, float b2, float omb) {
  __shared__ float sCol[NW * TC];
  __shared__ double red[NW];
  const Tile tl = tiles[blockIdx.x];
  const Tensor t = tensors[tl.tensor];
  if (t.rows == 0) {      // 1-D: the second moment itself, and this chunk's share of sum U^2
    const Chunk c = chunk_geom(t, tl.index);
    double acc = 0.0;
    for (uint32_t e = threadIdx.x; e < c.n; e += NT) {
      const float g = t.g[c.start + e];
      const float v = ema(t.row[c.start + e], b2, omb, __fadd_rn(__fmul_rn(g, g), eps0));
      t.row[c.start + e] = v;
      const float U = __fmul_rn(rsqrt_ref(v), g);
      acc += (double)U * (double)U;
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) reinterpret_cast<double*>(ws + t.ws_sq)[tl.index] = acc;
    return;
  }
  if (aligned16(t.g, t.cols)) stats_tile<true>(t, tl.index, ws, eps0, sCol);
  else stats_tile<false>(t, tl.index, ws, eps0, sCol);
}

// ------------------------------------------------------------------------------------------------ 2: finalise
constexpr int FT = 1024;
static_assert(LR2_ADAFACTOR_FIN_COLS == FT, "one column per thread");
__global__ __launch_bounds__(FT) void adafactor_finalize_kernel(const Tensor* __restrict__ tensors, const Fin* __restrict__ fins,
                                                                char* __restrict__ ws, float b2, float omb) {
  __shared__ double red[FT];
  const Fin f = fins[blockIdx.x];
  const Tensor t = tensors[f.tensor];
  const uint32_t tid = threadIdx.x;
  if (f.kind == 1) {
    const uint64_t j = f.start + tid;
    if (j < t.cols) {
      const float* part = reinterpret_cast<const float*>(ws + t.ws_col) + j;
      double a = 0.0;
      for (uint32_t rt = 0; rt < t.n_rt; ++rt) a += (double)part[(uint64_t)rt * t.cols];
      t.col[j] = ema(t.col[j], b2, omb, (float)(a / (double)t.rows));
    }
    return;
  }
  // all rows of one tensor, 256 at a time; the four threads of a row take a quarter of the column tiles each (joined in order)
  const uint32_t q = tid >> 8, rr = tid & 255;
  const uint32_t per = (t.n_ct + 3) / 4;
  const uint32_t lo = q * per < t.n_ct ? q * per : t.n_ct, hi = lo + per < t.n_ct ? lo + per : t.n_ct;
  const float* part = reinterpret_cast<const float*>(ws + t.ws_row);
  double msum = 0.0;
  for (uint64_t i0 = 0; i0 < t.rows; i0 += 256) {
    const uint64_t i = i0 + rr;
    double a = 0.0;
    if (i < t.rows)
      for (uint32_t ct = lo; ct < hi; ++ct) a += (double)part[(uint64_t)ct * t.rows + i];
    red[tid] = a;
    __syncthreads();
    if (q == 0 && i < t.rows) {
      const double s = ((red[rr] + red[256 + rr]) + red[512 + rr]) + red[768 + rr];
      const float nv = ema(t.row[i], b2, omb, (float)(s / (double)t.cols));
      t.row[i] = nv;
      msum += (double)nv;
    }
    __syncthreads();
  }
  red[tid] = q == 0 ? msum : 0.0;
  __syncthreads();
  for (uint32_t s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) *reinterpret_cast<float*>(ws + t.ws_mean) = (float)(red[0] / (double)t.rows);
}

// rsqrt(row / mean(row)) of the tile's rows and rsqrt(col) of its columns -> LDS
__device__ __forceinline__ void tile_factors(const Tensor& t, const Geom& gm, const char* ws, float* sR, float* sC) {
  const float mean = *reinterpret_cast<const float*>(ws + t.ws_mean);
  for (uint32_t r = threadIdx.x; r < gm.nrows; r += NT) sR[r] = rsqrt_ref(t.row[gm.i0 + r] / mean);
  for (uint32_t c = threadIdx.x; c < gm.ncols; c += NT) sC[c] = rsqrt_ref(t.col[gm.j0 + c]);
  __syncthreads();
}

// ------------------------------------------------------------------------------------------------ 3: sum of U^2
template <bool VEC>
__device__ __forceinline__ double usq_tile(const Tensor& t, const Geom& gm, const float* sR, const float* sC) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double acc = 0.0;
  for (uint32_t r = wave; r < gm.nrows; r += NW) {
    float x[PER];
    load_row<VEC>(t.g + (gm.i0 + r) * t.cols + gm.j0, gm.ncols, lane, x);
    const float rf = sR[r];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const uint32_t c = slot_col<VEC>(lane, k);
      if (c < gm.ncols) {
        const float U = __fmul_rn(__fmul_rn(rf, sC[c]), x[k]);
        acc += (double)U * (double)U;
      }
    }
  }
  return acc;
}

__global__ __launch_bounds__(NT) void adafactor_usq_kernel(const Tensor* __restrict__ tensors, const Tile* __restrict__ tiles,
                                                           char* __restrict__ ws) {
  __shared__ float sR[TR];
  __shared__ float sC[TC];
  __shared__ double red[NW];
  const Tile tl = tiles[blockIdx.x];
  const Tensor t = tensors[tl.tensor];
  if (t.rows == 0) return;      // 1-D chunks left their partial in the stats launch
  const Geom gm = tile_geom(t, tl.index);
  tile_factors(t, gm, ws, sR, sC);
  double acc = aligned16(t.g, t.cols) ? usq_tile<true>(t, gm, sR, sC) : usq_tile<false>(t, gm, sR, sC);
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) reinterpret_cast<double*>(ws + t.ws_sq)[tl.index] = acc;
}

// ------------------------------------------------------------------------------------------------ 4: apply
struct Step {
  float div;            // max(1, rms / clip_threshold)
  float lr;
  float alpha;          // -weight_decay * lr
  bool decay;
};
__device__ __forceinline__ float apply_one(float p, float U, const Step& s) {
  if (s.div != 1.0f) U = U / s.div;                 // update.div_(...): x / 1 is x
  U = __fmul_rn(U, s.lr);                           // update.mul_(lr)
  if (s.decay) p = __fadd_rn(p, __fmul_rn(s.alpha, p));   // p.add_(-wd*lr, p)
  return __fsub_rn(p, U);                           // p.add_(-update)
}
template <bool VEC>
__device__ __forceinline__ void apply_tile(const Tensor& t, const Geom& gm, const float* sR, const float* sC, const Step& s) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint32_t r = wave; r < gm.nrows; r += NW) {
    const uint64_t off = (gm.i0 + r) * t.cols + gm.j0;
    float x[PER], y[PER];
    load_row<VEC>(t.g + off, gm.ncols, lane, x);
    load_row<VEC>(t.p + off, gm.ncols, lane, y);
    const float rf = sR[r];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const uint32_t c = slot_col<VEC>(lane, k);
      if (c < gm.ncols) y[k] = apply_one(y[k], __fmul_rn(__fmul_rn(rf, sC[c]), x[k]), s);
    }
    store_row<VEC>(t.p + off, gm.ncols, lane, y);
  }
}

__global__ __launch_bounds__(NT) void adafactor_apply_kernel(const Tensor* __restrict__ tensors, const Tile* __restrict__ tiles,
                                                             const char* __restrict__ ws, double lr_host, double clip,
                                                             const float* __restrict__ lr_dev) {
  __shared__ float sR[TR];
  __shared__ float sC[TC];
  __shared__ double red[NW];
  const Tile tl = tiles[blockIdx.x];
  const Tensor t = tensors[tl.tensor];
  // the tensor's sum of U^2: thread i takes partials i, i + NT, ...; then the fixed-order workgroup sum -- the same bits in every tile
  const double* part = reinterpret_cast<const double*>(ws + t.ws_sq);
  double tot = 0.0;
  for (uint32_t i = threadIdx.x; i < t.n_tiles; i += NT) tot += part[i];
  tot = block_sum(tot, red);
  const double numel = t.rows ? (double)t.rows * (double)t.cols : (double)t.cols;
  const double lr = lr_dev ? (double)*lr_dev : lr_host;
  Step s;
  s.div = (float)fmax(1.0, sqrt(tot / numel) / clip);
  s.lr = (float)lr;
  s.alpha = (float)(-t.wd * lr);
  s.decay = t.wd != 0.0;
  if (t.rows == 0) {
    const Chunk c = chunk_geom(t, tl.index);
    for (uint32_t e = threadIdx.x; e < c.n; e += NT) {
      const float g = t.g[c.start + e];
      t.p[c.start + e] = apply_one(t.p[c.start + e], __fmul_rn(rsqrt_ref(t.row[c.start + e]), g), s);
    }
    return;
  }
  const Geom gm = tile_geom(t, tl.index);
  tile_factors(t, gm, ws, sR, sC);
  if (aligned16(t.g, t.cols) && aligned16(t.p, t.cols)) apply_tile<true>(t, gm, sR, sC, s);
  else apply_tile<false>(t, gm, sR, sC, s);
}

uint64_t g_adafactor_counts[2] = {0, 0};      // accepted calls / kernel launches (host-side counters: lr2_adafactor_launch_counts)

}  // namespace

extern "C" int lr2_adafactor_launch_counts(uint64_t counts[2]) {
  if (!counts) return LR2_ERR_ARG;
  counts[0] = g_adafactor_counts[0];
  counts[1] = g_adafactor_counts[1];
  return 0;
}

extern "C" int lr2_adafactor_multi(const lr2_adafactor_tensor* tensors_dev, const lr2_adafactor_tile* tiles_dev, int n_tiles,
                                   const lr2_adafactor_fin* fin_dev, int n_fin, void* ws_dev, double lr, double beta2t, double eps0,
                                   double clip_threshold, const void* lr_dev, void* stream) {
  if (!tensors_dev || !tiles_dev || !ws_dev || n_tiles <= 0 || n_fin < 0 || (n_fin && !fin_dev)) return LR2_ERR_ARG;
  if (!(clip_threshold > 0.0) || misaligned(ws_dev, 8) || misaligned(lr_dev, 4)) return LR2_ERR_ARG;
  const hipStream_t st = (hipStream_t)stream;
  const Tensor* tn = (const Tensor*)tensors_dev;
  const Tile* tl = (const Tile*)tiles_dev;
  // beta2t and (1 - beta2t) are formed in double like the reference's Python scalars, then rounded once to fp32
  const float b2 = (float)beta2t, omb = (float)(1.0 - beta2t);
  int rc;
  LR2_LAUNCH(adafactor_stats_kernel, dim3(n_tiles), dim3(NT), 0, st, tn, tl, (char*)ws_dev, (float)eps0, b2, omb);
  if ((rc = lr2_launch_status("adafactor_stats"))) return rc;
  // a group of 1-D tensors only has nothing to finalise; the update^2 launch stays (its workgroups return at once) so that the
  // number of launches depends on nothing but this
  if (n_fin) {
    LR2_LAUNCH(adafactor_finalize_kernel, dim3(n_fin), dim3(FT), 0, st, tn, (const Fin*)fin_dev, (char*)ws_dev, b2, omb);
    if ((rc = lr2_launch_status("adafactor_finalize"))) return rc;
  }
  LR2_LAUNCH(adafactor_usq_kernel, dim3(n_tiles), dim3(NT), 0, st, tn, tl, (char*)ws_dev);
  if ((rc = lr2_launch_status("adafactor_usq"))) return rc;
  LR2_LAUNCH(adafactor_apply_kernel, dim3(n_tiles), dim3(NT), 0, st, tn, tl, (const char*)ws_dev, lr, clip_threshold,
             (const float*)lr_dev);
  if ((rc = lr2_launch_status("adafactor_apply"))) return rc;
  g_adafactor_counts[0] += 1;
  g_adafactor_counts[1] += n_fin ? LR2_ADAFACTOR_LAUNCHES : LR2_ADAFACTOR_LAUNCHES - 1;
  return 0;
}
