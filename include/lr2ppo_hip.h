/* lr2ppo_hip.h -- C ABI of the MI355X (gfx950) kernels behind the LR2PPO hot path.
 *
 * The reference (ChazzyGordon/LR2PPO) is pure Python/PyTorch and has no FFI of its own:
 * every entry point below replaces a group of ATen/cuBLAS ops that the reference reaches through
 * nn.Module calls.  The "replaces" note on each function cites that reference call site
 * (paths relative to the reference repo root).  INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference would add.
 *
 * Conventions: raw device pointers + sizes; `stream` is a hipStream_t passed as void*; every call is
 * stream-ordered and asynchronous (no internal sync, no allocation, graph-capturable); no ownership is
 * transferred; return 0 on success or a negative LR2_ERR_* code (no exceptions cross the ABI).
 * All tensors are fp32 in HBM exactly as in the reference (indices int64/int32); bf16 exists only inside
 * the GEMM kernel (LDS images of split operands).  All reductions/accumulators are fp32.
 */
#ifndef LR2PPO_HIP_H
#define LR2PPO_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LR2_ERR_ARG (-1)    /* null pointer / inconsistent arguments */
#define LR2_ERR_SHAPE (-2)  /* shape not supported by the kernel's tiling */
#define LR2_ERR_LAUNCH (-3) /* HIP launch failure */

#define LR2_ABI_VERSION 27
int lr2_abi_version(void);
/* Fills name[0..len) with the HIP device name and returns the CU count (or <0). */
int lr2_device_info(char* name, int len);

/* Fused GEMM epilogue, applied per element (m, n) in this order:
 *   v = acc*alpha (+bias[n]); act==1: z=v (stored to out_z if set), v=gelu_erf(v);
 *   drop_p>0: v = keep(seed,site,m*N+n) ? v/(1-p) : 0;  act==2: v *= gelu_erf'(aux_z[m,n]);
 *   resid: v += resid[m,n];  accumulate: v += out[m,n];  out[m,n] = v (fp32) and/or (out_hi, out_lo)[m,n] = split(v). */
typedef struct lr2_epilogue {
  const void* bias;   /* [N] or NULL */
  const void* resid;  /* [M, ld_resid] or NULL */
  const void* aux_z;  /* [M, ld_aux], required when act == 2 */
  void* out;          /* [M, ld_out] fp32 or NULL (then out_hi must be set) */
  void* out_z;        /* [M, ld_z] pre-activation (act == 1) or NULL */
  void* out_hi;       /* bf16 hi plane [M, ld_planes] or NULL: result ALSO/INSTEAD written as split planes */
  uint64_t out_lo_off; /* elements from the hi plane to the lo plane; 0 (ABI 21): ONE bf16 plane, round to nearest even */
  int32_t ld_planes;
  int32_t ld_resid, ld_aux, ld_out, ld_z;
  int32_t act;        /* 0 none, 1 GELU(erf), 2 multiply by GELU'(aux_z) */
  int32_t accumulate; /* 1: out += result */
  float alpha;
  float drop_p;       /* 0 disables dropout */
  uint32_t drop_site;
  /* Global gradient-norm clipping of the fused optimizer step (adam_p): when non-NULL the result g[m,n] is multiplied by
   * *adam_gscale_dev (device float, the coefficient lr2_clip_coef writes) as ONE fp32 multiply of its own before the AdamW update --
   * the bits of lr2_adamw_multi_scaled on the materialised gradient.  NULL: the unscaled update, as before.  The pointer lies in
   * what used to be 8 bytes of padding in front of drop_seed (a uint32 _pad and the compiler's fill; zero in every caller that
   * zeroes the struct): sizeof and every other offset are unchanged. */
  const void* adam_gscale_dev;
  uint64_t drop_seed;
  /* Fused optimizer step (weight-gradient GEMMs): when adam_p is set the result g[m,n] (after alpha) is not stored but
   * consumed by the AdamW update of lr2_adamw_multi on (adam_p, adam_m, adam_v)[m, ld_out*m + n]; `out` may be NULL.
   * The 2 GB gradient of out_layer.fc1.weight is then never written to or read back from HBM.  drop_p must be 0 with adam_p
   * (the update consumes the result: there is nothing to mask; LR2_ERR_ARG otherwise).
   * replaces: the fc1.weight slice of optimizers.py:344-402 + the .grad write of loss.backward(). */
  void* adam_p;
  void* adam_m;
  void* adam_v;
  double adam_lr, adam_beta1, adam_beta2, adam_eps, adam_weight_decay;
  /* (1,1) form only -- the weight gradient dW = dY^T X of an nn.Linear: when colsum is set, colsum[m] = sum over k of A[k, m]
   * (the gradient of the layer's BIAS, db = sum of dY rows) is produced by the same call.  On the 256 x 256 kernel (block_m =
   * 256) the sums are accumulated from the A fragments the product stages anyway -- dY is not read a second time; otherwise a
   * column-sum pass runs behind the product.  colsum_ws: fp32 scratch, max(128, splits * ceil(N / 256)) * M floats.
   * replaces: autograd of the bias of nn.Linear (tencentpretrain/layers/position_ffn.py:12-15, multi_headed_attn.py:55-76). */
  void* colsum;
  void* colsum_ws;
  /* Device-resident dropout seed (HIP-graph capture of a training step: a seed passed by value would be frozen into the graph):
   * when non-NULL, the mask stream's seed is *drop_seed_dev + drop_seed (device uint64, read by the kernel at run time);
   * drop_site must then be below 65536. */
  const void* drop_seed_dev;
  /* Device-resident learning rate of the fused optimizer step (same reason: a scheduler changes it every step): when non-NULL the
   * update uses *adam_lr_dev (device float) and adam_lr is ignored. */
  const void* adam_lr_dev;
} lr2_epilogue;

/* C[M,N] = op(A).op(B), fp32 in / fp32 out, computed on bf16 MFMA with fp32 accumulation.
 *   passes=3: split-bf16 (x = hi + lo; lo*hi + hi*lo + hi*hi): fp32-grade results (rel. err ~2^-17)
 *   passes=1: single bf16 pass (inputs rounded to bf16)
 *   trans_a=0: A is [M][K] (lda>=K);  trans_a=1: A is [K][M] (lda>=M)
 *   trans_b=0: B is [N][K] (nn.Linear weight);  trans_b=1: B is [K][N]
 * Supported forms: (0,0) forward, (0,1) input gradient, (1,1) weight gradient.
 * Constraints: K%64==0 unless both operands are strided (1,1); lda,ldb %4==0 (16-byte rows); buffers < 4 GiB.
 * M, N and (in the (1,1) form) K may be ragged.
 * Operand formats: a_planes / b_planes = 0: fp32 matrix (split into bf16 hi+lo inside the kernel);
 *   = 1: pre-split "planes" tensor: bf16 hi plane at the pointer, bf16 lo plane a_lo_off / b_lo_off BYTES later, both
 *   with the matrix's row-major shape and leading dimension (elements); streamed by LDS-DMA, no conversion work.
 *   Supported: (fp32, fp32), (planes, planes), (planes A, fp32 B).  Planes are produced by the epilogue's out_hi,
 *   by lr2_split_planes(_multi) and by the LayerNorm / attention kernels' planes outputs.
 * a_bytes/b_bytes: bytes addressable from A/B, per plane (rows past the end read as zero: ragged M, ragged K in (1,1)).
 *   In the (1,1) form the kernels never compare a row with K: the caller passes the extent of K ROWS (K * ld elements, or what is
 *   addressable when that is less), not of the allocation -- rows K and later that lie inside a_bytes / b_bytes are added into the
 *   product.  Whole rows: operands are read 16 bytes at a time and a load that crosses the extent reads as zero.
 * LR2_ERR_ARG: act outside 0..2, act == 2 without aux_z.  LR2_ERR_SHAPE: a leading dimension smaller than the row it addresses
 *   (lda < K, or < M when trans_a; ldb likewise; ld_out / ld_z / ld_resid / ld_aux / ld_planes < N when the pointer is set; ld_out
 *   for adam_p) -- lr2_gemm_bf16 and lr2_gemm_bf16_train refuse the same.  Nothing is launched by a rejected call.
 * splits>1 uses split-K through splitk_ws (fp32 [splits][M][N]).  block_m: 128 or 64, or 256 = the 256 x 256 ping-pong kernel for
 *   planes x planes operands with passes = 3: the (0,0) form (whole 32-deep K steps, splits = 1) and the (1,1) form (any K, any
 *   splits: tiles x splits workgroups, the weight-gradient kernel of round 3); other combinations fall back to the 128-row family.
 * replaces: nn.Linear / F.linear + bias + nn.GELU + nn.Dropout + residual add in
 *   finetune/ppo.py:164-170 (Mlp), finetune/xit.py:103-110,118-122,147,
 *   tencentpretrain/layers/{multi_headed_attn.py:55-58,75, position_ffn.py:12-15} and their autograd backward. */
int lr2_gemm(const void* A, const void* B, int M, int N, int K, int lda, int ldb, int trans_a, int trans_b,
             uint64_t a_bytes, uint64_t b_bytes, int a_planes, uint64_t a_lo_off, int b_planes, uint64_t b_lo_off,
             const lr2_epilogue* epi, void* splitk_ws, int splits, int block_m, int passes, void* stream);

/* Round 4 (ABI 18).  How lr2_gemm schedules a large (0,0) product of planes asked for with block_m = 256 and no fused dropout mask:
 * *rows_256 = the leading rows that run on the 256 x 256 kernel as WHOLE rounds of one workgroup per CU (0 = one launch, no row
 * split); the remaining rows run on the general kernel with *tail_block_m-row tiles (2-3 workgroups per CU), so that a last round
 * less than half full does not hold the chip for a full tile time.  Pure host arithmetic; lr2_gemm follows this plan.
 * LR2_GEMM_ROWSPLIT=0 (read once per process) switches the split off.  Same nn.Linear call sites as lr2_gemm. */
int lr2_gemm_row_split_plan(int M, int N, int K, int* rows_256, int* tail_block_m);
/* Diagnostic: launches issued by lr2_gemm since the library was loaded -- counts[0] the 256 x 256 NT kernel, counts[1] its TN form,
 * counts[2] the general kernel family (tests assert which kernels a call reached; no device call). */
int lr2_gemm_launch_counts(uint64_t counts[3]);
/* Diagnostic (ABI 26): *rows = the tile height, 256 or 192, that the launchers of the 256 x 256 NT kernels (lr2_gemm, lr2_gemm_bf16,
 * lr2_gemm_bf16_train at block_m == 256) pick for a launch of M rows and N columns: 192 when one round of 256-row tiles would leave
 * CUs idle that a round of 192-row tiles fills.  Pure host arithmetic (no device call); tests assert which form a shape reaches. */
int lr2_gemm256_tile_rows(int M, int N, int* rows);

/* Row gather: dst[b, j, :] = src[b, clamp(index[b, j]), :]  (rows of row_elems fp32; strides in elements; index NULL: index[b, j] = j).
 * An index outside [0, t_in) is CLAMPED into it (below 0 -> row 0, t_in and above -> row t_in - 1): never an out-of-bounds read, and
 * with index NULL and t_in = 1 every output row is the one source row.  lr2_gather_rows_bwd applies the same clamp, so the pair is
 * adjoint for every index tensor.
 * LR2_ERR_ARG: a NULL src / dst, B / t_in / t_out <= 0, row_elems == 0.  LR2_ERR_SHAPE: row_elems or a stride % 4, src or dst not
 * 16-byte aligned (float4 accesses).
 * replaces: text_emb[batch_index, index] / img_emb[batch_index, index] (finetune/ppo.py:268-271,321-324). */
int lr2_gather_rows(const void* src, const int64_t* index, void* dst, int B, int t_in, int t_out, uint64_t row_elems,
                    uint64_t src_bstride, uint64_t src_tstride, void* stream);
/* Gradient of lr2_gather_rows with tight strides: dsrc[b, t, :] = sum over the j with clamp(index[b, j]) == t of ddst[b, j, :], in j
 * order.  EVERY row of dsrc [B, t_in, row_elems] is overwritten (a row that no j selects becomes zeros): no zero-initialisation,
 * no accumulation into dsrc.  The clamp is lr2_gather_rows'.  Refusals as in lr2_gather_rows (ddst and dsrc 16-byte aligned). */
int lr2_gather_rows_bwd(const void* ddst, const int64_t* index, void* dsrc, int B, int t_in, int t_out,
                        uint64_t row_elems, void* stream);
/* Strided row copy: dst[(r / group)*dst_gstride + (r % group)*D + dst_off + c] = src[r*D + c].
 * dst_planes=1: dst is a bf16 planes tensor (same element offsets, lo plane dst_lo_off elements later).
 * LR2_ERR_ARG: NULL src / dst, rows / D / group <= 0.  LR2_ERR_SHAPE: D, dst_gstride or dst_off % 4; src not 16-byte aligned; dst not
 * 16-byte aligned (fp32) or not 8-byte aligned / dst_lo_off % 4 (planes).
 * replaces: torch.cat([x, img_feature], dim=1) (finetune/ppo.py:224). */
int lr2_copy_rows(const void* src, void* dst, int dst_planes, uint64_t dst_lo_off, int rows, int D, int group,
                  uint64_t dst_gstride, uint64_t dst_off, void* stream);
/* fp32 -> bf16 planes: dst_hi[i] = bf16(src[i]), dst_hi[lo_off + i] = bf16(src[i] - hi) for i < n (n % 4 == 0).
 * Vector accesses: src 16-byte aligned, dst_hi 8-byte aligned, lo_off % 4 == 0 (the lo plane 8-byte aligned too), else
 * LR2_ERR_SHAPE. */
int lr2_split_planes(const void* src, void* dst_hi, uint64_t lo_off, uint64_t n, void* stream);
/* Transposing split: src fp32 [R][C] -> planes [C][R] (hi at dst_hi, lo lo_off elements behind).  An nn.Linear weight
 * [out, in] re-laid as [in, out] lets its forward x.W^T run as the (0,1) form of lr2_gemm, the fastest of the three on wide
 * outputs; nothing in the reference corresponds to it (layout choice of this build).  Element-wise accesses only: no alignment
 * beyond the element types', any lo_off. */
int lr2_split_planes_t(const void* src, void* dst_hi, uint64_t lo_off, int R, int C, void* stream);
/* planes of dropout_mask(src) / (1 - p), mask element index = flat element index (the gradient entering a dropped branch).
 * drop_p in [0, 1) (0: lr2_split_planes); n % 4 == 0; src 16-byte aligned, dst_hi 8-byte aligned, lo_off % 4 == 0, else LR2_ERR_SHAPE.
 * replaces: autograd of nn.Dropout at tencentpretrain/layers/transformer.py:55,58,65,72 on the pre-LN residual paths. */
int lr2_dropout_planes(const void* src, void* dst_hi, uint64_t lo_off, uint64_t n, float drop_p, uint64_t drop_seed,
                       uint32_t drop_site, void* stream);
/* lr2_split_planes for many tensors in one launch (weights after an optimizer step). table: DEVICE array of chunks.  The table
 * lives on the device, so the chunks are NOT checked: each must meet lr2_split_planes' rules (src 16-byte aligned, dst_hi 8-byte
 * aligned, lo_off % 4 == 0, count % 4 == 0). */
typedef struct lr2_split_chunk {
  const void* src;
  void* dst_hi;
  uint64_t lo_off; /* elements */
  uint64_t count;  /* elements, multiple of 4 */
} lr2_split_chunk;
int lr2_split_planes_multi(const lr2_split_chunk* table_dev, int n_chunks, void* stream);

/* LayerNorm forward over rows of length D (D%4==0, D<=1024).
 *   mode 0: nn.LayerNorm (biased variance, eps inside sqrt)      -- finetune/xit.py:37,74,93-94
 *   mode 1: TencentPretrain LayerNorm gamma*(x-mu)/(std_unbiased+eps)+beta -- tencentpretrain/layers/layer_norm.py:16-21
 * Output row r is written at out + (r / group)*group_stride + (r % group)*D (group<=0: dense), which lets the
 * final XiT LayerNorm write straight into the concat buffer of finetune/ppo.py:224.
 * out (fp32) and/or out_hi (bf16 planes, lo plane out_lo_off elements later, same row mapping) receive the result.
 * out_lo_off == 0 (ABI 21): out_hi is ONE bf16 plane (round to nearest even -- the hi plane of the planes output and nothing else:
 * 2 bytes written per element), the A operand of lr2_gemm_bf16.
 * mean/rstd (fp32 [rows]) may be NULL when no backward is needed. */
int lr2_layernorm_fwd(const void* x, const void* gamma, const void* beta, void* out, void* out_hi, uint64_t out_lo_off,
                      void* mean, void* rstd, int rows, int D, float eps, int mode, int group, uint64_t group_stride,
                      void* stream);

/* LayerNorm backward, both semantics (mode / eps as in the forward).  dy uses the same (group, stride) row mapping as the forward output.
 * dx = LN'(dy) (+ resid_grad) -> dx (fp32); optional dxm_hi = bf16 planes of dropout_mask(dx)/(1-p) (the gradient of
 * y = dropout(a) + res with respect to a, finetune/xit.py:34,40; p = 0: planes of dx), the next GEMMs' operand.  dgamma/dbeta are accumulated per block
 * into partials [nblocks][2][D]; finish with lr2_colsum_partials_finish.  drop_seed_dev (may be NULL): device uint64 added to drop_seed at run
 * time, as in lr2_epilogue.
 * replaces: autograd of nn.LayerNorm + the in-place residual adds of finetune/xit.py:45-55,77-86, and of the
 * TencentPretrain LayerNorm (tencentpretrain/layers/layer_norm.py:16-21) in the encoder layers. */
int lr2_layernorm_bwd(const void* dy, int group, uint64_t group_stride, const void* x, const void* gamma, const void* mean,
                      const void* rstd, const void* resid_grad, void* dx, void* dxm_hi, uint64_t dxm_lo_off, float drop_p,
                      uint64_t drop_seed, uint32_t drop_site, const void* drop_seed_dev, void* partials, int nblocks, int rows, int D,
                      int mode, float eps, void* stream);
/* lr2_layernorm_fwd for rows of up to 1536 columns (the same kernel with six float4 per lane instead of four; every argument, both
 * modes and every output form as there; D % 4 == 0, 4 <= D <= 1536).  lr2_layernorm_fwd keeps its refusal of D > 1024.
 * replaces: the TencentPretrain LayerNorm (tencentpretrain/layers/layer_norm.py:5-21) of a tower wider than 1024 (ViT-H/14: 1280). */
int lr2_layernorm_fwd_wide(const void* x, const void* gamma, const void* beta, void* out, void* out_hi, uint64_t out_lo_off,
                           void* mean, void* rstd, int rows, int D, float eps, int mode, int group, uint64_t group_stride,
                           void* stream);
/* lr2_layernorm_bwd for rows of up to 1536 columns, every argument as there (partials: [nblocks, 2 D]).
 * replaces: autograd of the TencentPretrain LayerNorm (tencentpretrain/layers/layer_norm.py:16-21) of a tower wider than 1024. */
int lr2_layernorm_bwd_wide(const void* dy, int group, uint64_t group_stride, const void* x, const void* gamma, const void* mean,
                           const void* rstd, const void* resid_grad, void* dx, void* dxm_hi, uint64_t dxm_lo_off, float drop_p,
                           uint64_t drop_seed, uint32_t drop_site, const void* drop_seed_dev, void* partials, int nblocks, int rows,
                           int D, int mode, float eps, void* stream);
/* out[c] (+)= sum_b partials[b*ld + c] for c < cols (deterministic second stage of column reductions; accumulate != 0 adds to out).
 * ld >= cols, else LR2_ERR_SHAPE. */
int lr2_colsum_partials_finish(const void* partials, int nblocks, int cols, int ld, void* out, int accumulate,
                               void* stream);
/* Column sums of a [rows, cols] matrix (fp32, or bf16 planes with the lo plane lo_off elements after the hi plane; is_planes == 2
 * (ABI 22): ONE bf16 plane, lo_off unused) -> fp32 [cols] (bias gradients); partials: workspace [nblocks][cols].
 * cols % 4 == 0, ld % 4 == 0, ld >= cols, else LR2_ERR_SHAPE.
 * replaces: autograd of the nn.Linear bias add. */
int lr2_colsum(const void* x, int is_planes, uint64_t lo_off, int rows, int cols, int ld, void* partials, int nblocks,
               void* out, void* stream);

/* XiT multi-head attention core, per (sequence b, head h): S = Q K^T (no pre-scale), P = softmax(S) * post_scale,
 * O = P V.  Q/O: [batch*Lq, heads*hd]; K/V: [batch*Lk, heads*hd].  Lq<=256, Lk<=16, hd<=96, hd%4==0.
 * o_planes=1: O is written as bf16 planes (hi at O, lo o_lo_off elements later) for the projection GEMM.
 * LR2_ERR_SHAPE: Lq outside [1, 256], Lk outside [1, 16], head_dim outside [4, 96] or % 4; Q not 16-byte aligned; O not 16-byte
 * aligned (fp32) or not 8-byte aligned / o_lo_off % 4 (planes).
 * replaces: finetune/xit.py:133-146 (einsum, softmax, "/ scaling", einsum). */
int lr2_xattn_fwd(const void* Q, const void* K, const void* V, void* O, int o_planes, uint64_t o_lo_off, int batch,
                  int heads, int Lq, int Lk, int head_dim, float post_scale, void* stream);
/* Backward of lr2_xattn_fwd: recomputes P; writes dQ [batch*Lq, E], dK, dV [batch*Lk, E] (fp32, or bf16 planes when
 * planes=1: lo planes q_lo_off / kv_lo_off elements after the hi planes).  Shape rules of the forward; Q and dO 16-byte aligned;
 * dQ / dK / dV 16-byte aligned (fp32) or 8-byte aligned with q_lo_off % 4 == 0 and kv_lo_off % 4 == 0 (planes), else LR2_ERR_SHAPE. */
int lr2_xattn_bwd(const void* Q, const void* K, const void* V, const void* dO, void* dQ, void* dK, void* dV,
                  int planes, uint64_t q_lo_off, uint64_t kv_lo_off, int batch, int heads, int Lq, int Lk, int head_dim,
                  float post_scale, void* stream);
/* The wide form of the pair above, for more than 16 image tokens (--max_imgs up to 64): the argument lists, formulas, fp32 FMA
 * arithmetic, output forms and alignment rules of lr2_xattn_fwd / lr2_xattn_bwd with 1 <= Lk <= 64 (K / V of one (sequence, head) stay
 * resident in LDS, 48 KiB at 64 keys: the reason for the limit).  No atomics, every sum in a fixed order: two calls give the same bits.
 * At Lk <= 16 the results meet the narrow pair's bounds but are not bit-equal to it (the backward adds in another order).
 * LR2_ERR_ARG: a NULL pointer, batch or heads not positive.  LR2_ERR_SHAPE: Lq outside [1, 256], Lk outside [1, 64], head_dim outside
 * [4, 96] or % 4, a pointer or plane offset off the narrow pair's alignment.  A refused call launches nothing.
 * replaces: finetune/xit.py:133-146 at max_imgs > 16 (the reference accepts any number of image tokens). */
int lr2_xattn_fwd_wide(const void* Q, const void* K, const void* V, void* O, int o_planes, uint64_t o_lo_off, int batch,
                       int heads, int Lq, int Lk, int head_dim, float post_scale, void* stream);
int lr2_xattn_bwd_wide(const void* Q, const void* K, const void* V, const void* dO, void* dQ, void* dK, void* dV,
                       int planes, uint64_t q_lo_off, uint64_t kv_lo_off, int batch, int heads, int Lq, int Lk, int head_dim,
                       float post_scale, void* stream);
/* Diagnostic: counts[0] = accepted lr2_xattn_fwd_wide calls, counts[1] = accepted lr2_xattn_bwd_wide calls (host counters, not
 * synchronised; a refused call moves neither).
 * replaces: nothing (a test hook, as lr2_gemm_f16_launch_counts: which form a dispatch ran). */
int lr2_xattn_wide_launch_counts(uint64_t counts[2]);

/* TencentPretrain self-attention core, per (sequence, head): S = Q K^T * scale + (seg[key]>0 ? 0 : -10000),
 * P = softmax(S), O = P V -- both products on the matrix cores (split-bf16 x3), softmax in fp32.
 * q_hi / k_hi / v_hi: bf16 hi planes of Q, K, V, element (row, h*64 + d) at ptr[row*ld + h*64 + d], the lo plane lo_off
 * ELEMENTS behind each (one fused QKV matrix [batch*L, 3*heads*64] with ld = 3*heads*64 is the intended producer);
 * seg int64 [batch*L]; o fp32 [batch*L, ld_o] and/or o_hi planes (lo plane o_lo_off elements behind); hd == 64; any L (one
 * LDS-resident key block up to 256 keys, a key-block loop with running max / sum beyond).
 * A sequence with no valid key: softmax over the -10000-shifted scores, as upstream; accurate to the fp32 grid at 10^4.
 * replaces: tencentpretrain/layers/multi_headed_attn.py:61-74 and the mask of encoders/transformer_encoder.py:62-68. */
int lr2_self_attn_fwd(const void* q_hi, const void* k_hi, const void* v_hi, uint64_t lo_off, int ld, const int64_t* seg,
                      void* o, void* o_hi, uint64_t o_lo_off, int ld_o, void* lse, float drop_p, uint64_t drop_seed,
                      uint32_t drop_site, int batch, int heads, int L, int head_dim, float scale, void* stream);
/* (above) lse: optional fp32 [batch, heads, L] log-sum-exp of the masked scores; drop_p > 0 applies the counter-based
 * dropout to the probabilities (element index ((b*heads + h)*L + q)*L + key, multi_headed_attn.py:72). */

/* Self-attention for the FIRST query row of every sequence only: o[b, h*64 + d] = sum_j softmax_j(q[b] . K[b*L + j] * scale +
 * (seg>0 ? 0 : -10000)) V[b*L + j] -- what pooling 'first' keeps of the last encoder layer (the [CLS] feature of the image
 * encoder), so that layer's output projection and feed-forward run on `batch` rows instead of batch*L.
 * q fp32 [batch, ld_q] (already projected, bias included); k_hi / v_hi bf16 hi planes of K and V over ALL rows, element
 * (row, h*64 + d) at ptr[row*ld + h*64 + d], lo plane lo_off ELEMENTS behind; seg int64 [batch*L]; o fp32 [batch, ld_o];
 * L <= 4096, head_dim == 64.
 * replaces: tencentpretrain/layers/multi_headed_attn.py:61-74 restricted to query 0 (utils/misc.py:23-35 'first' pooling,
 * as consumed at finetune/ppo.py:120-127). */
int lr2_first_token_attn(const void* q, int ld_q, const void* k_hi, const void* v_hi, uint64_t lo_off, int ld,
                         const int64_t* seg, void* o, int ld_o, int batch, int heads, int L, int head_dim, float scale,
                         void* stream);

/* Backward of lr2_self_attn_fwd: from Q, K, V planes and dO planes (same layout rules) to dQ, dK, dV planes
 * (dq_hi / dk_hi / dv_hi: hi planes, element (row, h*64 + d) at ptr[row*ld_d + h*64 + d], lo plane d_lo_off elements behind --
 * three column blocks of one dQKV matrix are the intended target).  Two kernels: dQ per 16-query sub-tile, then dK, dV per 16-key
 * sub-tile; pass the forward's drop_p / seed / site to replay its mask.
 *   o_hi == NULL: everything is recomputed from Q, K, V -- the dQ kernel writes the per-query log-sum-exp and sum_k dP*P into lse_ws /
 *     dsum_ws (fp32 [batch*heads*L] each, scratch).  L > 256: both kernels walk the other dimension in blocks of 128 rows; the dQ
 *     kernel sweeps the keys twice (running max / sum / sum of exp * dP first).
 *   o_hi != NULL (ABI 19): the forward's output planes (element (row, h*64 + d) at o_hi[row*ld_o + h*64 + d], lo plane o_lo_off elements
 *     behind) and, in lse_ws, the log-sum-exp lr2_self_attn_fwd wrote (an INPUT then): P = exp(S - lse) and D = sum_d dO O need no
 *     pass over the keys, both kernels stream over 32-row blocks and -- with at least one (sequence, head) pair per CU, L <= 224 -- run
 *     as persistent 16-wave workgroups whose K / V (Q / dO) planes are refilled by LDS-DMA under the compute (lr2_self_attn_plan
 *     says which form a shape takes).  Shapes the persistent form does not cover fall back to the recomputing kernels, which
 *     OVERWRITE lse_ws with their own (equal up to rounding) values.
 * A sequence with no valid key: softmax over the -10000-shifted scores, as upstream; accurate to the fp32 grid at 10^4.
 * replaces: autograd of tencentpretrain/layers/multi_headed_attn.py:61-74. */
int lr2_self_attn_bwd(const void* q_hi, const void* k_hi, const void* v_hi, uint64_t lo_off, int ld, const void* do_hi,
                      uint64_t do_lo_off, int ld_do, const int64_t* seg, void* dq_hi, void* dk_hi, void* dv_hi,
                      uint64_t d_lo_off, int ld_d, const void* o_hi, uint64_t o_lo_off, int ld_o, void* lse_ws, void* dsum_ws,
                      float drop_p, uint64_t drop_seed, uint32_t drop_site, int batch, int heads, int L, int head_dim, float scale,
                      void* stream);
/* (ABI 19) Which form of the attention kernels a call of this shape runs on this device: *fwd_persistent / *bwd_persistent = 1 when
 * lr2_self_attn_fwd / lr2_self_attn_bwd (given o_hi) take the persistent kernels (a pure function of the shape, the CU count and the
 * LR2_ATTN_PERSIST switch; either pointer may be NULL).  No reference counterpart: a test hook of this library's own scheduling. */
int lr2_self_attn_plan(int batch, int heads, int L, int ld, int ld_do, int* fwd_persistent, int* bwd_persistent);

/* lr2_self_attn_fwd for head widths other than 64: head_dim % 16 == 0, 32 <= head_dim <= 128 (ViT-H/14: 80), every argument as there
 * with h*head_dim + d in place of h*64 + d.  The width is padded to a multiple of 32 inside the kernel: the padding columns are zeros the
 * kernel writes, never loaded and never stored.  One key-blocked kernel (64-key blocks, running max / sum) for every L; results are the
 * same bits from run to run.  head_dim == 64 is accepted (tests set this skeleton against lr2_self_attn_fwd; dispatch never sends it).
 * LR2_ERR_ARG: a NULL pointer, batch, heads or L not positive, drop_p outside [0, 1).  LR2_ERR_SHAPE: another head_dim, or
 * lr2_self_attn_fwd's alignment rules.  A refused call launches nothing.
 * replaces: tencentpretrain/layers/multi_headed_attn.py:61-74 and the mask of encoders/transformer_encoder.py:62-68. */
int lr2_self_attn_hd_fwd(const void* q_hi, const void* k_hi, const void* v_hi, uint64_t lo_off, int ld, const int64_t* seg,
                         void* o, void* o_hi, uint64_t o_lo_off, int ld_o, void* lse, float drop_p, uint64_t drop_seed,
                         uint32_t drop_site, int batch, int heads, int L, int head_dim, float scale, void* stream);
/* lr2_self_attn_bwd for the head widths of lr2_self_attn_hd_fwd, every argument as there.  Always the recomputing form: a dQ kernel
 * (two sweeps over 64-key blocks; writes lse_ws and dsum_ws) and a dK / dV kernel (64-query blocks, accumulators in registers); o_hi is
 * checked as lr2_self_attn_bwd checks it and not read, lse_ws is overwritten.  Errors as lr2_self_attn_hd_fwd.
 * replaces: autograd of tencentpretrain/layers/multi_headed_attn.py:61-74. */
int lr2_self_attn_hd_bwd(const void* q_hi, const void* k_hi, const void* v_hi, uint64_t lo_off, int ld, const void* do_hi,
                         uint64_t do_lo_off, int ld_do, const int64_t* seg, void* dq_hi, void* dk_hi, void* dv_hi,
                         uint64_t d_lo_off, int ld_d, const void* o_hi, uint64_t o_lo_off, int ld_o, void* lse_ws, void* dsum_ws,
                         float drop_p, uint64_t drop_seed, uint32_t drop_site, int batch, int heads, int L, int head_dim, float scale,
                         void* stream);
/* Diagnostic: counts[0] = accepted lr2_self_attn_hd_fwd calls, counts[1] = accepted lr2_self_attn_hd_bwd calls (host counters, not
 * synchronised; a refused call moves neither).
 * replaces: nothing (a test hook, as lr2_xattn_wide_launch_counts). */
int lr2_self_attn_hd_launch_counts(uint64_t counts[2]);

/* y[r] = dot(x[row(r)], w) + b for r < rows, row(r) = r*row_step + row_off.
 * replaces: self.head = nn.Linear(768, 1) and the last-position select (finetune/ppo.py:228-232,293-295). */
int lr2_head_fwd(const void* x, const void* w, const void* b, void* y, int rows, int D, int row_step, int row_off,
                 void* stream);
/* dx[total_rows, D] = 0 except dx[row(r)] = dy[r]*w for r < rows (total_rows may exceed rows*row_step: the rows beyond are 0);
 * dw = sum_r dy[r]*x[row(r)];  db = sum_r dy[r].  dx may be NULL; dw and db are written together or not at all. */
int lr2_head_bwd(const void* x, const void* w, const void* dy, void* dx, void* dw, void* db, int rows, int D,
                 int row_step, int row_off, int total_rows, void* stream);

/* out[r, :] = x[r, :] + table[r % period, :].  replaces: x + pos_emb (finetune/ppo.py:286-289,339-342). */
int lr2_add_period_rows(const void* x, const void* table, void* out, int rows, int D, int period, void* stream);
/* dtable[t, :] = sum over rows r with r % period == t of dy[r, :]  (t < period; other rows of dtable untouched). */
int lr2_period_rows_grad(const void* dy, void* dtable, int rows, int D, int period, void* stream);

/* Fused PPO losses + analytic gradients for one minibatch (T = tags per item, T <= 8, B <= 1024).
 * Inputs fp32: scores[B,T] (new), old_scores[B,T], rewards[B], old_value[B], value[B]; int64 next_state[B,ns_len]
 * (its last rank_len entries give the actor's descending order; the reference hard-codes 2, ppo.py:565-567).
 * Outputs fp32:
 *   scalars[0]=policy loss, [1]=value loss, [2]=rank loss, [3]=positive-hinge count;
 *   per_item[4][B] = kl, entropy, rewards (r - w_kl*kl), advantages; dscores[B,T]; dvalue[B].
 * Data-parallel form (RankLoss is one scalar over the GLOBAL batch): call once with stats_out (fp32[3]) set -- only
 * {hinge sum, positive-hinge count, sum |A|} of this rank are written -- all-reduce(sum) those three floats over the
 * `world` ranks, then call again with global_stats = the reduced sums: R, 1/count and mean |A| are then global and
 * dscores is scaled so that the rank AVERAGE of the parameter gradients equals the gradient of the global-batch loss.
 * stats_out == NULL and global_stats == NULL: the single-rank form.
 * replaces: finetune/ppo.py:544-584 (KL, entropy, advantage, flipped order, RankLoss :43-55, clipped value
 * loss :494-498) and their autograd backward. */
int lr2_ppo_loss(const void* scores, const void* old_scores, const void* rewards, const void* old_value,
                 const void* value, const int64_t* next_state, int ns_len, int rank_len, int B, int T, float kl_w,
                 float ent_w, float value_clip, float margin, float adv_eps, void* scalars, void* per_item,
                 void* dscores, void* dvalue, void* stats_out, const void* global_stats, int world, void* stream);

/* mode = 'cls' (C classes, C <= 8): the 768 -> C head, y[r, c] = x[r, :] . w[c, :] + b[c], and its backward
 * (dx[r, :] = sum_c dy[r, c] w[c, :]; dw[c, :] = sum_r dy[r, c] x[r, :]; db[c] = sum_r dy[r, c]; dx or dw/db may be NULL).
 * D % 4 == 0; x and w (forward), w and dx (backward, when dx is given) 16-byte aligned, else LR2_ERR_SHAPE.
 * replaces: nn.Linear(768, labels_num) of finetune/ppo.py:209-210,228-230 and its autograd. */
int lr2_cls_head_fwd(const void* x, const void* w, const void* b, void* y, int rows, int D, int C, void* stream);
int lr2_cls_head_bwd(const void* x, const void* w, const void* dy, void* dx, void* dw, void* db, int rows, int D, int C,
                     void* stream);
/* probs[r, :] = softmax(logits[r, :]) (use_softmax = 1) or logits[r, :] (0: evaluate(), ppo.py:641-643); scores[r] =
 * sum_k k * probs[r, k] (the expected label the PPO loop ranks by); probs may be NULL.
 * replaces: finetune/ppo.py:532-537 / :859-863 / :641-643. */
int lr2_cls_scores(const void* logits, void* probs, void* scores, int rows, int C, int use_softmax, void* stream);
/* dlogits[r, c] = dscores[r] * probs[r, c] * (c - scores[r]): autograd of the softmax form of lr2_cls_scores. */
int lr2_cls_scores_bwd(const void* probs, const void* scores, const void* dscores, void* dlogits, int rows, int C, void* stream);
/* loss[0] = mean_r (logsumexp(logits[r, :]) - logits[r, tgts[r]]); dlogits (may be NULL) = its gradient.
 * replaces: nn.NLLLoss()(nn.LogSoftmax(dim=-1)(logits), tgts) of finetune/ppo.py:239-241 and its autograd. */
int lr2_nll_loss(const void* logits, const int64_t* tgts, int rows, int C, void* loss, void* dlogits, void* stream);

/* SmoothL1(beta) mean loss + gradient (dpred may be NULL).  replaces: nn.SmoothL1Loss(beta=0.3) (finetune/ppo.py:236). */
int lr2_smooth_l1(const void* pred, const void* target, int n, float beta, void* loss, void* dpred, void* stream);

/* Pairwise hinge of the stage-2 reward training: scores = [chosen(bs) ; reject(bs)];
 * loss_acc[0] = mean relu(margin - (chosen - reject)), loss_acc[1] = mean (chosen > reject); dscores (may be NULL) = d loss / d scores.
 * replaces: finetune/reward_pair_dataloader.py:356-359 (+ the autograd of that expression). */
int lr2_pair_hinge(const void* scores, int bs, float margin, void* loss_acc, void* dscores, void* stream);

/* One chunk of the multi-tensor AdamW: `count` fp32 elements starting at p/g/m/v. */
typedef struct lr2_adamw_chunk {
  void* p;
  const void* g;
  void* m;
  void* v;
  uint64_t count;
  float weight_decay;
  float _pad;
} lr2_adamw_chunk;
/* table: DEVICE array of n_chunks lr2_adamw_chunk (one workgroup per chunk).  Update (correct_bias=False):
 *   m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; p -= lr * m/(sqrt(v)+eps); then p -= lr*wd*p.
 * replaces: tencentpretrain/utils/optimizers.py:344-402 (AdamW.step), including its decay-after-update order. */
int lr2_adamw_multi(const lr2_adamw_chunk* table_dev, int n_chunks, double lr, double beta1, double beta2,
                    double eps, const void* lr_dev, void* stream);
/* lr_dev (may be NULL): device float read by the kernel in place of `lr` -- a captured HIP graph of a training step then follows
 * the scheduler without re-capture. */

/* Global gradient-norm clipping (added within ABI 27: new entry points; lr2_epilogue.adam_gscale_dev took the place of padding).
 * The rule is torch.nn.utils.clip_grad_norm_ with norm_type = 2 and error_if_nonfinite = False:
 *   total_norm = sqrt(sum of g^2 over every gradient), coef = min(1, max_norm / (total_norm + 1e-6)), g <- g * coef.
 * Everything stays on the device; every sum has a fixed order (a thread's elements in index order, lane tree, waves in index
 * order -- no atomics), so results are bit-reproducible.  Four pieces:
 *   lr2_clip_sumsq    partials[i] = sum over chunk i of g^2, fp64 (squares formed and added in fp64), one workgroup per chunk of the
 *                     table lr2_adamw_multi reads (only g and count are used).  16-byte loads for a chunk whose g is 16-byte
 *                     aligned, element loads otherwise.
 *   lr2_clip_gram_dot *slot = factor * sum_ij A[i,j] * B[i,j] of two fp32 [n, n] matrices (rows ld_a / ld_b floats apart), fp64, one
 *                     workgroup.  With A = dY dY^T and B = X X^T this is the squared Frobenius norm of dW = alpha dY^T X
 *                     (factor = alpha^2) -- the gradient of out_layer.fc1.weight, which the fused update never materialises.
 *   lr2_clip_coef     one workgroup adds slots[0..n) in index order (fp64) and writes out[0] = total_norm, out[1] = coef as fp32,
 *                     both formed in fp64 and rounded once.  A NaN sum gives NaN, NaN; an infinite one gives inf, 0.
 *   lr2_adamw_multi_scaled   lr2_adamw_multi on g * *gscale_dev (device float; one fp32 multiply of its own, then the same update):
 *                     gradients in memory stay unscaled.  16-byte accesses for a chunk whose four pointers are 16-byte aligned,
 *                     element accesses otherwise.
 * LR2_ERR_ARG: a NULL pointer (lr_dev excepted), n_chunks / n <= 0, ld < n, a partials / slot pointer that is not 8-byte aligned,
 * an out / gscale_dev pointer that is not 4-byte aligned, max_norm < 0 or NaN.
 * replaces: nothing in the reference (it has no clip); torch.nn.utils.clip_grad_norm_ is what a user of it would call. */
int lr2_clip_sumsq(const lr2_adamw_chunk* table_dev, int n_chunks, void* partials_dev, void* stream);
int lr2_clip_gram_dot(const void* A, const void* B, int n, int ld_a, int ld_b, double factor, void* slot_dev, void* stream);
int lr2_clip_coef(const void* slots_dev, int n, double max_norm, void* out_dev, void* stream);
int lr2_adamw_multi_scaled(const lr2_adamw_chunk* table_dev, int n_chunks, double lr, double beta1, double beta2, double eps,
                           const void* lr_dev, const void* gscale_dev, void* stream);

/* Added within ABI 27 (purely additive: no signature or struct changes).  Multi-tensor Adafactor with an external learning rate
 * (relative_step=False, scale_parameter=False, beta1=None -- what every launcher passes), fp32, for 2-D (factored second moment)
 * and 1-D tensors.  A 2-D tensor [rows, cols] is cut into tiles of LR2_ADAFACTOR_TILE_ROWS x LR2_ADAFACTOR_TILE_COLS (row-major tile
 * order: index = row_tile * n_col_tiles + col_tile); a 1-D tensor (rows == 0) into chunks of LR2_ADAFACTOR_CHUNK_1D elements.
 * One call issues LR2_ADAFACTOR_LAUNCHES kernel launches whatever the number of tensors (one fewer, no finalise, when n_fin == 0):
 *   1 stats     (grid n_tiles): u = g*g + eps0; per tile the row sums and column sums of u -> workspace partials (fp32, summed in
 *               fp64).  1-D chunks: v = beta2t v + (1-beta2t) u, U = g rsqrt(v), sum U^2 -> the chunk's partial.
 *   2 finalise  (grid n_fin): per tensor the partials summed in tile order (fp64), row = beta2t row + (1-beta2t) mean_j(u),
 *               col likewise with mean_i(u); the rows entry of a tensor also stores mean(row).
 *   3 update^2  (grid n_tiles): U = g * rsqrt(row / mean(row))[i] * rsqrt(col)[j]; sum U^2 per tile -> partial (fp64).
 *   4 apply     (grid n_tiles): rms = sqrt(sum of the tensor's partials in tile order / numel); U /= max(1, rms / clip_threshold);
 *               U *= lr; p += (-weight_decay*lr) * p; p -= U.
 * No atomics: every sum has a fixed order, results are bit-reproducible.  Nothing returns to the host.  p / g / the state vectors
 * need 4-byte alignment only: 16-byte accesses are used for a tensor whose pointers are 16-byte aligned and whose cols % 4 == 0,
 * element accesses otherwise.  Offsets are 64-bit throughout.
 * HBM traffic of a 2-D tensor: g three times, p once in and once out = 20 B per parameter. */
#define LR2_ADAFACTOR_TILE_ROWS 512
#define LR2_ADAFACTOR_TILE_COLS 1024
#define LR2_ADAFACTOR_CHUNK_1D 8192
#define LR2_ADAFACTOR_FIN_COLS 1024 /* columns per finalise entry of kind 1 */
#define LR2_ADAFACTOR_LAUNCHES 4
typedef struct lr2_adafactor_tensor {
  void* p;
  const void* g;
  void* row;        /* 2-D: exp_avg_sq_row [rows]; 1-D: exp_avg_sq [cols] */
  void* col;        /* 2-D: exp_avg_sq_col [cols]; 1-D: unused */
  uint64_t rows;    /* 0: a 1-D tensor of `cols` elements */
  uint64_t cols;
  uint64_t ws_row;  /* BYTE offsets into the workspace: fp32 row partials [n_col_tiles][rows] */
  uint64_t ws_col;  /* fp32 column partials [n_row_tiles][cols] */
  uint64_t ws_mean; /* fp32 mean(row) */
  uint64_t ws_sq;   /* fp64 sum-of-U^2 partials [n_tiles], 8-byte aligned */
  uint32_t n_tiles; /* tiles (2-D) or chunks (1-D) of this tensor */
  uint32_t n_col_tiles;
  uint32_t n_row_tiles;
  uint32_t _pad;
  double weight_decay;
} lr2_adafactor_tensor;
typedef struct lr2_adafactor_tile {
  uint32_t tensor; /* index into the tensor table */
  uint32_t index;  /* tile / chunk number within that tensor */
} lr2_adafactor_tile;
typedef struct lr2_adafactor_fin {
  uint32_t tensor;
  uint32_t kind;  /* 0: all rows of the tensor (one entry per 2-D tensor); 1: LR2_ADAFACTOR_FIN_COLS columns from `start` */
  uint64_t start;
} lr2_adafactor_fin;
/* tensors / tiles / fin: DEVICE tables (every tile of every tensor exactly once; one kind-0 entry and ceil(cols / FIN_COLS) kind-1
 * entries per 2-D tensor; n_fin may be 0 when every tensor is 1-D).  ws: DEVICE workspace the offsets point into, 8-byte aligned.
 * beta2t = 1 - step^decay_rate, eps0 and clip_threshold by value (formed in double on the host, like the reference's math.pow);
 * lr as lr2_adamw_multi's (lr_dev, may be NULL: device float read in its place).
 * replaces: tencentpretrain/utils/optimizers.py:518-603 (Adafactor.step) for relative_step=False, scale_parameter=False,
 * beta1=None. */
int lr2_adafactor_multi(const lr2_adafactor_tensor* tensors_dev, const lr2_adafactor_tile* tiles_dev, int n_tiles,
                        const lr2_adafactor_fin* fin_dev, int n_fin, void* ws_dev, double lr, double beta2t, double eps0,
                        double clip_threshold, const void* lr_dev, void* stream);
/* Diagnostic: counts[0] = accepted lr2_adafactor_multi calls, counts[1] = kernel launches they issued (host counters, not
 * synchronised; a refused call moves neither).
 * replaces: nothing (a test hook, as lr2_xattn_wide_launch_counts). */
int lr2_adafactor_launch_counts(uint64_t counts[2]);

/*
 * The per-step scalars such a graph reads -- dst_dev[0..7] = seed (uint64, the dropout seed of lr2_epilogue.drop_seed_dev /
 * lr2_layernorm_bwd), dst_dev[8 + 4 i ..] = lrs[i] (float, i < n_lrs <= 14) -- are written by ONE small kernel whose arguments
 * carry the values: no host buffer has to outlive the call, so steps can be enqueued ahead of the device. */
#define LR2_STEP_SCALARS_BYTES 64
#define LR2_STEP_SCALARS_MAX_LRS 14
int lr2_step_scalars_store(void* dst_dev, uint64_t seed, const float* lrs_host, int n_lrs, void* stream);

/* Tokens -> embeddings: out[r,:] = word[src[r]] + pos[r % L] + seg_table[seg[r]].  Ids outside [0, vocab) / [0, n_seg) never
 * index memory: the row is taken from index 0 and *err_flag (device int, may be NULL) gets bit 0 (token) / bit 1 (segment)
 * OR-ed in, for the host to raise the IndexError nn.Embedding would.  The sum is (word + pos) + seg in fp32.
 * LR2_ERR_ARG: a NULL pointer (err_flag excepted), rows / L / D / vocab / n_seg <= 0.  LR2_ERR_SHAPE: D % 4; word, pos, seg_table or
 * out not 16-byte aligned (float4 accesses).
 * replaces: tencentpretrain/embeddings/{word,pos,seg}_embedding.py forward sums (embedding.py:19-30). */
int lr2_text_embed(const int64_t* src, const int64_t* seg, const void* word, const void* pos, const void* seg_table,
                   void* out, int rows, int L, int D, int64_t vocab, int n_seg, int* err_flag, void* stream);
/* Backward of lr2_text_embed's word / segment gathers (the position table's gradient is lr2_period_rows_grad), deterministic:
 * `order` = stable argsort of the token ids, `sorted_ids` = ids in that order; dword[tok, :] = sum of dx rows carrying tok (rows of
 * dword for PRESENT tokens are overwritten, rows for absent tokens are NOT written: zero the table first).  A run of equal ids is
 * summed in original row order inside pieces of LR2_TEXT_EMBED_BWD_WORD_SEG sorted positions, the pieces of a long run (the padding
 * id) in piece order through `word_partials` (fp32 scratch, 2 * ceil(rows / LR2_TEXT_EMBED_BWD_WORD_SEG) * D floats) -- a fixed
 * order, and no single workgroup walks a long run alone.  dseg[s, :] = sum of dx rows with segment s via `seg_partials` (fp32
 * scratch, ceil(rows / LR2_TEXT_EMBED_BWD_ROWS_PER_BLOCK) * n_seg * D floats).  No atomics.  Rows whose token id is outside [0, vocab)
 * or whose segment id is outside [0, n_seg) are dropped from the respective sum.
 * LR2_ERR_ARG: a NULL pointer, rows / D / vocab <= 0.  LR2_ERR_SHAPE: D % 4, n_seg outside [1, 4]; dx, dword or word_partials not
 * 16-byte aligned (float4 accesses).
 * replaces: autograd of nn.Embedding in tencentpretrain/embeddings/{word,seg}_embedding.py. */
#define LR2_TEXT_EMBED_BWD_ROWS_PER_BLOCK 64
#define LR2_TEXT_EMBED_BWD_WORD_SEG 256
int lr2_text_embed_bwd(const void* dx, const int64_t* sorted_ids, const int64_t* order, const int64_t* seg, void* dword,
                       void* dseg, void* seg_partials, void* word_partials, int rows, int D, int64_t vocab, int n_seg,
                       void* stream);
/* dst = dropout_mask(src) / (1 - p), fp32, mask element index = flat element index (src == dst allowed).
 * drop_p in (0, 1); n % 4 == 0; src and dst 16-byte aligned, else LR2_ERR_SHAPE.
 * replaces: self.dropout of tencentpretrain/embeddings/embedding.py:33 and its autograd. */
int lr2_dropout_apply(const void* src, void* dst, uint64_t n, float drop_p, uint64_t drop_seed, uint32_t drop_site,
                      void* stream);
/* Image -> patch rows: out[(b*P + p), c*ps*ps + i*ps + j] = img[b, c, py*ps+i, px*ps+j].
 * LR2_ERR_ARG: NULL img / out, B / C / H / W / ps <= 0.  LR2_ERR_SHAPE: H or W % ps.
 * replaces: the unfold implied by nn.Conv2d(k=s=patch) in tencentpretrain/embeddings/patch_embedding.py:18,27. */
int lr2_patchify(const void* img, void* out, int B, int C, int H, int W, int ps, void* stream);
/* Image -> patch rows as bf16 hi/lo planes (the A operand of the patch-projection GEMM); element layout of lr2_patchify with row
 * stride ld >= C*ps*ps (columns past C*ps*ps are written as zeros: ViT-L/14's 588 -> 640 so the GEMM sees whole K tiles); ps even.
 * img: fp32 [B,C,H,W] (is_u8 = 0) or uint8 frames [B,C,H,W] (is_u8 = 1); with is_u8 and mean3/std3 (HOST float[3]) given, pixels
 * are normalised on the fly: (x / 255 - mean[c]) / std[c].
 * LR2_ERR_ARG: NULL img / out_hi, B / C / H / W / ps <= 0.  LR2_ERR_SHAPE: H or W % ps, C > 3, ps odd, ld < C*ps*ps, ld % 4, lo_off
 * odd; out_hi not 8-byte aligned when ps % 4 == 0 and lo_off % 4 == 0 (4 x bf16 stores per plane), not 4-byte aligned otherwise
 * (2 x bf16 stores); img not 16-byte aligned when ps == 16, ld == C*ps*ps and lo_off % 4 == 0 (the strip kernel's 16-byte loads).
 * replaces: ZeroOneNormalize + transforms.Normalize (tencentpretrain/utils/dataloader.py:559-561) + the unfold implied by
 * nn.Conv2d(k=s=patch) (embeddings/patch_embedding.py:18,27). */
int lr2_patchify_planes(const void* img, int is_u8, void* out_hi, uint64_t lo_off, int ld, int B, int C, int H, int W, int ps,
                        const float* mean3, const float* std3, void* stream);
/* NDCG@ks[q] per ragged item i (elements offsets[i] .. offsets[i+1], at most 64): sort by score descending (stable), gain
 * 2^rel - 1, discount disc[j] (= log2(j + 2), device fp32 table supplied by the caller), sequential fp32 sums, 1 when the ideal
 * DCG <= 1e-6.  out: fp32 [n_items, n_k].  An item with more than 64 elements, or with a label outside [0, 62] (2^rel - 1 in
 * int64), gets a row of NaN -- never a truncated or wrapped value (the entry point cannot see device-side sizes without a sync).
 * replaces: finetune/ppo.py:651-659 + ndcg.py:28-65 (AverageNDCGMeter.return_ndcg_at_k). */
int lr2_ndcg(const void* scores, const int64_t* gold, const int64_t* offsets, const void* disc, const int64_t* ks, int n_k,
             void* out, int n_items, void* stream);
/* ViT embedding assembly: out[b,0,:] = cls + pos[0]; out[b,1+p,:] = patch_proj[b*P+p,:] + pos[1+p].
 * LR2_ERR_ARG: a NULL pointer, B / P / D <= 0.  LR2_ERR_SHAPE: D % 4; patch_proj, cls, pos or out not 16-byte aligned (float4).
 * replaces: patch_embedding.py:28-29 (cls concat) + pos_embedding.py:30-35 + embedding.py:27-30. */
int lr2_vit_assemble(const void* patch_proj, const void* cls, const void* pos, void* out, int B, int P, int D,
                     void* stream);

/* MX-FP8 products on gfx950's block-scaled matrix instruction (BASELINE.json configs[4]: "fp8 MFMA"; an inference-only fast mode,
 * NOT the parity path: e4m3 keeps 3 mantissa bits).  Format: OCP MX v1.0 -- e4m3fn elements, one E8M0 scale byte (2^(s - 127)) per 32
 * consecutive elements of a row, shared exponent floor(log2(amax)) - 8, round-to-nearest-even, saturating at +-448.
 *   lr2_quant_mxfp8: x fp32 [rows, K] (row stride ldx) -> q uint8 [rows, K], scales uint8 [rows, K / 32].  K % 32 == 0.
 *   lr2_gemm_mxfp8 : out[M, N] fp32 = A_q . B_q^T (+ bias[N]) (act 1: GELU) (+ resid[M, ld_resid]); A_q [M, K], B_q [N, K] and their
 *                    scales as written by lr2_quant_mxfp8.  N % 128 == 0, K % 128 == 0, any M.  out_q / out_scales (both or neither;
 *                    out may then be NULL): the result also / instead quantised to MX-FP8 [M, N] + [M, N / 32] by the same rule --
 *                    the A operand of the next product without an fp32 round trip.  out_hi / out_lo_off / ld_planes: the result also /
 *                    instead as bf16 hi / lo planes (the operand format of lr2_self_attn_fwd and of the split-bf16 products);
 *                    out_lo_off == 0 (ABI 18): ONE bf16 plane (round to nearest even), the operand format of lr2_self_attn_fwd_bf16.
 * Every producer of the format in this library (these two, lr2_layernorm_fwd_mxfp8, lr2_quant_mxfp8_t, lr2_self_attn_fwd_bf16 and its
 * blocked form) writes the same bytes for the same fp32 row: scale byte = max(exponent field of amax - 8, 0): 0 for amax below 2^-118, 247 for
 * amax = Inf; a NaN element takes no part in amax and becomes 0xFE (-448), +-Inf +-448, -0 and negative values
 * that round to zero 0x80; fp32 denormals are not flushed (tests/test_mx_edges_gpu.py).
 * LR2_ERR_ARG: a NULL operand; no destination; act other than 0 / 1; out_q without out_scales or the reverse; non-positive sizes.
 * LR2_ERR_SHAPE: lr2_quant_mxfp8: K % 32, ldx < K, ldx % 4; lr2_gemm_mxfp8: N % 128, K % 128, ld_out or ld_resid below N or no multiple
 * of 4 (where the pointer is given), ld_planes below N or no multiple of 4, out_lo_off % 4.  A refused call writes nothing.
 * replaces: nn.Linear forward (tencentpretrain/layers/position_ffn.py:12-15, multi_headed_attn.py:55-76) in that mode. */
int lr2_quant_mxfp8(const void* x, int ldx, void* q, void* scales, int rows, int K, void* stream);
/* LayerNorm (lr2_layernorm_fwd's semantics, modes 0 / 1) whose result leaves as MX-FP8 [rows, D] + [rows, D / 32] (and as fp32 when out is
 * given): the A operand of the projection that follows, without an fp32 round trip.  D % 32 == 0. */
int lr2_layernorm_fwd_mxfp8(const void* x, const void* gamma, const void* beta, void* out, void* out_q, void* out_scales, int rows,
                            int D, float eps, int mode, void* stream);
int lr2_gemm_mxfp8(const void* a_q, const void* a_scales, const void* b_q, const void* b_scales, void* out, int ld_out,
                   const void* bias, const void* resid, int ld_resid, int act, void* out_q, void* out_scales, void* out_hi,
                   uint64_t out_lo_off, int ld_planes, int M, int N, int K, void* stream);
/* Round 4 (ABI 18).  Encoder self-attention of the MX-FP8 mode: q / k / v are ONE bf16 plane each (row stride ld elements; what
 * lr2_gemm_mxfp8 writes with out_lo_off = 0 -- q, k, v = the three column blocks of one [rows, 3E] matrix), single-pass bf16 products,
 * fp32 softmax, key mask -10000 * (seg <= 0) after the scale; the context rows leave as fp32 (o_f32 [batch * L, ld_o]) and / or as
 * MX-FP8 (o_q [batch * L, ld_o] bytes + o_scales [batch * L, ld_o / 32]: the A operand of the output projection, no fp32 round trip, no
 * quantise pass) and / or (ABI 21) as ONE bf16 plane (o_bf16 [batch * L, ld_o], round to nearest even of the fp32 context: the A
 * operand of lr2_gemm_bf16).  head_dim 64, L <= 288, inference only (no dropout).  NOT the parity path: lr2_self_attn_fwd stays the
 * default.
 * replaces: tencentpretrain/layers/multi_headed_attn.py:60-74 in those modes. */
int lr2_self_attn_fwd_bf16(const void* q, const void* k, const void* v, int ld, const int64_t* seg, void* o_f32, void* o_q,
                           void* o_scales, void* o_bf16, int ld_o, int batch, int heads, int L, int head_dim, float scale, void* stream);
/* (ABI 21) *persistent = 1 when lr2_self_attn_fwd_bf16 runs a call of this shape as persistent workgroups (at least one (sequence,
 * head) pair per CU), 0 for one workgroup per pair.  A test hook of this library's own scheduling; no reference counterpart. */
int lr2_self_attn_fwd_bf16_plan(int batch, int heads, int L, int ld, int* persistent);

/* ABI 21.  Single-pass bf16 product, the "bf16" inference mode (BASELINE.json configs[2]; FeatureExtractor(precision="bf16")):
 * C[M, N] = A[M, K] . B[N, K]^T with A and B ONE bf16 plane each (row strides lda / ldb elements, a_bytes / b_bytes addressable from
 * each pointer: rows past the end read as zero), one v_mfma_f32_16x16x32_bf16 product per tile pair, fp32 accumulate.  NOT the parity
 * path: an operand keeps 8 mantissa bits.  Epilogue: alpha, bias, act 0 / 1 (GELU), resid; the result goes to out (fp32) and / or
 * out_hi -- hi / lo planes, or ONE bf16 plane (round to nearest even) when out_lo_off == 0, the convention of lr2_gemm_mxfp8.
 * Inference only: dropout, act 2, accumulate, out_z, the fused optimizer step and column sums are LR2_ERR_ARG.
 * K % 64 == 0, lda / ldb % 8 == 0, N % 4 == 0 (else LR2_ERR_SHAPE); M and N may be ragged.
 * block_m == 256: the 256 x 256 single-pass ping-pong kernel (csrc/gemm256_b1.hip) at ANY M (large products follow
 * lr2_gemm_row_split_plan as lr2_gemm does); 128 / 64: the general kernel family at passes = 1.
 * replaces: nn.Linear forward (tencentpretrain/layers/position_ffn.py:12-15, multi_headed_attn.py:55-76) in that mode. */
int lr2_gemm_bf16(const void* A, const void* B, int M, int N, int K, int lda, int ldb, uint64_t a_bytes, uint64_t b_bytes,
                  const lr2_epilogue* epi, int block_m, void* stream);
/* Diagnostic: launches issued by lr2_gemm_bf16 since the library was loaded -- counts[0] the 256 x 256 single-pass kernel, counts[1]
 * the general kernel family (no device call).  Plain host counters, as lr2_gemm_launch_counts': not synchronised -- meaningful when one
 * thread issues the launches, which is how tests read them. */
int lr2_gemm_bf16_launch_counts(uint64_t counts[2]);

/* ABI 22.  Single-pass bf16 products of encoder TRAINING (FeatureExtractor(precision="bf16_train")): A and B ONE bf16 plane
 * each, one v_mfma_f32_16x16x32_bf16 product per tile pair, fp32 accumulate.  NOT the parity path (lr2_gemm at passes = 3 stays it).
 *   (trans_a, trans_b) == (0, 0):  C[M, N] = A[M, K] . B[N, K]^T -- lr2_gemm_bf16's product with lr2_gemm's TRAINING epilogue: alpha, bias,
 *       act 0 / 1 (GELU; out_z keeps the pre-activation) / 2 (multiply by the EXACT GELU'(aux_z): x * (Phi(z) + z phi(z)) formed in fp64
 *       with one rounding, on kernels of its own; no split-K), the dropout mask (drop_*), resid, accumulate; the
 *       result goes to out (fp32) and / or out_hi (hi / lo planes, or ONE plane when out_lo_off == 0).  K % 64 == 0.  block_m == 256: the
 *       256 x 256 single-pass kernel (csrc/gemm256_b1.hip) when at most one of {aux_z, resid, accumulate} asks for a value per element
 *       and splits <= 1, following lr2_gemm_row_split_plan unless a dropout mask is fused (lr2_gemm's rule); else the general family at
 *       passes = 1 (block_m 128 / 64).  An input gradient runs in this form on the weight's transpose (lr2_split_planes_t).
 *   (1, 1):  C[M, N] = A[K, M]^T . B[K, N] -- the weight gradient dW[N_out, N_in] = dY[T, N_out]^T X[T, N_in] (M = N_out, N = N_in, K = T;
 *       any K: rows past a_bytes / b_bytes -- the extents of K WHOLE rows, lr2_gemm's rule -- read as zero).  Plain epilogue (alpha -> out).  colsum (with
 *       colsum_ws of max(128, splits * ceil(N / 256)) * M floats; M % 4 == 0): the bias gradient db[m] = sum_k A[k, m], the column sums
 *       of the bf16 plane AS THE PRODUCT SEES IT (not of the fp32 gradient it was rounded from).  block_m == 256: the 256 x 256
 *       single-pass TN kernel (csrc/gemm256_tn_b1.hip; 64-row K steps, tiles x splits workgroups, column sums from the same launch);
 *       else the general family at passes = 1 and lr2_colsum.  splits > 1 leaves fp32 slabs [splits, M, N] in splitk_ws, summed in
 *       split order by one more launch: the same bits on every run.
 * LR2_ERR_ARG: NULL operands / epilogue / no output; act == 2 without aux_z; adam_p (no fused optimizer); accumulate or a training
 * epilogue (bias, act, dropout, resid, out_z, out_hi) with the (1,1) form; colsum with the (0,0) form or without colsum_ws; (1,0) / (0,1);
 * splits > 1 without splitk_ws or with act == 2.  LR2_ERR_SHAPE: lda / ldb % 8, N % 4, an epilogue leading dimension % 4, K % 64 in the (0,0) form,
 * M % 4 with colsum, a_bytes / b_bytes >= 4 GiB, a leading dimension smaller than the row it addresses.  Nothing is launched by a rejected call.
 * replaces: nn.Linear forward and autograd's input / weight / bias gradients of it (tencentpretrain/layers/position_ffn.py:12-15,
 * multi_headed_attn.py:55-76) in that mode. */
int lr2_gemm_bf16_train(const void* A, const void* B, int M, int N, int K, int lda, int ldb, int trans_a, int trans_b, uint64_t a_bytes,
                        uint64_t b_bytes, const lr2_epilogue* epi, void* splitk_ws, int splits, int block_m, void* stream);
/* Diagnostic, as lr2_gemm_bf16_launch_counts: launches issued by lr2_gemm_bf16_train -- counts[0] the 256 x 256 single-pass NT kernel,
 * counts[1] the 256 x 256 single-pass TN kernel, counts[2] the general kernel family. */
int lr2_gemm_bf16_train_launch_counts(uint64_t counts[3]);

/* ABI 23.  Encoder self-attention of the single-pass bf16 TRAINING mode (FeatureExtractor(precision="bf16_train", bf16_attention=True),
 * DESIGN 4.6; csrc/selfattn_b1_train.hip): every operand and every output ONE bf16 plane, element (row, h * 64 + d) at
 * ptr[row * ld + h * 64 + d]; q / k / v are the three column blocks of one [batch * L, 3E] plane, dq / dk / dv likewise; one
 * v_mfma_f32_16x16x32_bf16 product per tile pair, fp32 softmax, key mask -10000 * (seg <= 0) after the scale.  One workgroup per
 * (sequence, head) (small batches: up to 4), head_dim 64, 1 <= L <= 288.  NOT the parity path: lr2_self_attn_fwd / lr2_self_attn_bwd
 * stay the default.
 *   lr2_self_attn_fwd_bf16_train: lr2_self_attn_fwd_bf16's arithmetic with training's two additions.  The un-normalised probabilities
 *       p~ = exp2(s - max) are summed in fp32 BEFORE dropout; p~ * (keep ? 1 / (1 - p) : 0) -- lr2_self_attn_fwd's mask stream:
 *       element ((b * heads + h) * L + q) * pitch(L) + key of (drop_seed, drop_site), pitch = L rounded up to 4 -- is rounded to
 *       bf16 (nearest even) as the A operand of P V, the accumulator is multiplied by 1 / sum, the context leaves as one bf16 plane
 *       o_bf16 [batch * L, ld_o].  lse (optional): fp32 [batch, heads, L], the natural-log log-sum-exp of the masked scores (before
 *       dropout).  drop_p == 0: o_bf16 is byte-equal to lr2_self_attn_fwd_bf16's.
 *   lr2_self_attn_bwd_bf16: the recomputing backward, two launches.  dQ: S^T = K Q^T, dPd^T = V dO^T, P = softmax, dP = dPd o M,
 *       D = sum_k dP P, dS = P (dP - D) scale rounded to bf16, dQ = dS K; writes lse_ws and dsum_ws (fp32 [batch, heads, L] each,
 *       workspaces: the dK / dV launch reads them).  dK / dV: P = exp(S scale + mask - lse), Pd = P o M and dS rounded to bf16,
 *       dV = Pd^T dO, dK = dS^T Q.  Outputs: round to nearest even of the fp32 accumulators.  Neither the forward's lse nor its
 *       output is read; the same (drop_p, drop_seed, drop_site) as the forward replays its mask.  No atomics: two calls give the same
 *       bytes.
 * LR2_ERR_ARG: a NULL pointer (lse of the forward excepted), q / k / v / d_o not 16-byte or an output not 8-byte aligned, drop_p
 * outside [0, 1).  LR2_ERR_SHAPE: head_dim != 64, L < 1 or L > 288, a leading dimension that is no multiple of 8 or smaller than
 * heads * 64.  Nothing is launched by a rejected call.
 * replaces: tencentpretrain/layers/multi_headed_attn.py:61-74 (scores, mask, softmax, dropout, context) and its autograd, in that
 * mode. */
int lr2_self_attn_fwd_bf16_train(const void* q, const void* k, const void* v, int ld, const int64_t* seg, void* o_bf16, int ld_o,
                                 void* lse, float drop_p, uint64_t drop_seed, uint32_t drop_site, int batch, int heads, int L,
                                 int head_dim, float scale, void* stream);
int lr2_self_attn_bwd_bf16(const void* q, const void* k, const void* v, int ld, const void* d_o, int ld_do, const int64_t* seg,
                           void* dq, void* dk, void* dv, int ld_d, void* lse_ws, void* dsum_ws, float drop_p, uint64_t drop_seed,
                           uint32_t drop_site, int batch, int heads, int L, int head_dim, float scale, void* stream);
/* Diagnostic, as lr2_gemm_bf16_launch_counts: counts[0] = accepted lr2_self_attn_fwd_bf16_train calls, counts[1] = accepted
 * lr2_self_attn_bwd_bf16 calls since the library was loaded.
 * replaces: nothing (a test hook: which attention a schedule ran; multi_headed_attn.py:61-74 has no counterpart). */
int lr2_self_attn_bf16_train_launch_counts(uint64_t counts[2]);

/* ABI 24.  The same attention for sequences longer than one LDS-resident head (FeatureExtractor(precision="bf16_train",
 * bf16_attention=True, bf16_attention_long=True); csrc/selfattn_b1_blocked.hip): the argument lists, the layout, the
 * arithmetic contract, the key mask, the dropout mask stream and the rounding sites of lr2_self_attn_fwd_bf16_train /
 * lr2_self_attn_bwd_bf16, with the keys (forward, dQ) or the queries (dK / dV) walked in blocks through LDS; head_dim 64, any L >= 1
 * (so 1 <= L <= 288 can be run in both forms), one workgroup of 8 waves per (sequence, head, chunk of query or key sub-tiles).
 *   lr2_self_attn_fwd_bf16_train_blocked: K and V of one key block in LDS (lr2_self_attn_fwd's blocked rule: ceil(L / 224) equal rounded
 *       blocks of 160, 192 or 224 keys); per 16-query sub-tile a running maximum m, the sum l of the unrounded, un-dropped
 *       p~ = exp2(s - m) and the un-normalised accumulator, both rescaled by exp2(m - m') in fp32 when m grows; p~ * mask is rounded to
 *       bf16 as the A operand of P V; o_bf16 = accumulator / l as one bf16 plane; lse (optional) = m + log l in natural-log units.
 *   lr2_self_attn_bwd_bf16_blocked: two launches.  dQ, two sweeps over key blocks of 256: sweep 1 keeps m, l and a = sum exp(s - m) dP
 *       and writes lse_ws = m + log l and dsum_ws = D = a / l; sweep 2 forms dS = P (dP - D) scale, rounds it to bf16, dQ += dS K.
 *       dK / dV: a wave holds 16 keys' K and V fragments and accumulators while Q, dO, lse and D pass through LDS in blocks of 256
 *       queries; Pd = P o M and dS are rounded to bf16.  Outputs: round to nearest even of the fp32 accumulators.  No atomics.
 * Errors as the two calls above with L >= 1 as the only length rule; nothing is launched by a rejected call.
 * replaces: tencentpretrain/layers/multi_headed_attn.py:61-74 (scores, mask, softmax, dropout, context) and its autograd, in that mode
 * at the sequence lengths the one-block kernels do not serve. */
int lr2_self_attn_fwd_bf16_train_blocked(const void* q, const void* k, const void* v, int ld, const int64_t* seg, void* o_bf16, int ld_o,
                                         void* lse, float drop_p, uint64_t drop_seed, uint32_t drop_site, int batch, int heads, int L,
                                         int head_dim, float scale, void* stream);
int lr2_self_attn_bwd_bf16_blocked(const void* q, const void* k, const void* v, int ld, const void* d_o, int ld_do, const int64_t* seg,
                                   void* dq, void* dk, void* dv, int ld_d, void* lse_ws, void* dsum_ws, float drop_p, uint64_t drop_seed,
                                   uint32_t drop_site, int batch, int heads, int L, int head_dim, float scale, void* stream);
/* Host only: the block lengths the two calls above use at this L (each launcher calls the helper this does): *fwd_key_block keys per
 * block of the forward, *dq_key_block keys per block of the dQ launch, *dkv_query_block queries per block of the dK / dV launch; NULL
 * pointers are skipped.  LR2_ERR_ARG for L < 1.
 * replaces: nothing (tests lay their masks on these blocks; multi_headed_attn.py:61-74 has no counterpart). */
int lr2_self_attn_bf16_blocked_plan(int L, int* fwd_key_block, int* dq_key_block, int* dkv_query_block);
/* Diagnostic: counts[0] = accepted lr2_self_attn_fwd_bf16_train_blocked calls, counts[1] = accepted lr2_self_attn_bwd_bf16_blocked calls
 * since the library was loaded.
 * replaces: nothing (a test hook, as lr2_self_attn_bf16_train_launch_counts). */
int lr2_self_attn_bf16_blocked_launch_counts(uint64_t counts[2]);

/* ABI 25.  lr2_self_attn_fwd_bf16 for sequences longer than one LDS-resident head (FeatureExtractor(precision="bf16" | "mxfp8",
 * attention_long=True); csrc/selfattn_mx_blocked.hip): that call's argument list, layout, key mask and three outputs -- q / k /
 * v ONE bf16 plane each (row stride ld), the context rows out as fp32 (o_f32 [batch * L, ld_o]) and / or as MX-FP8 (o_q [batch * L, ld_o]
 * bytes + o_scales [batch * L, ld_o / 32], lr2_quant_mxfp8's rule) and / or as ONE bf16 plane (o_bf16 [batch * L, ld_o], round to nearest
 * even of the fp32 context); any subset -- with the keys walked in blocks through LDS by lr2_self_attn_fwd_bf16_train_blocked's loop:
 * lr2_self_attn_bf16_blocked_plan's fwd_key_block keys per block, per 16-query sub-tile a running maximum m, the fp32 sum l of the
 * unrounded p~ = exp2(s - m) and the un-normalised accumulator, both rescaled by exp2(m - m') when m grows; p~ rounded to bf16 as the A
 * operand of P V; context = accumulator / l.  No dropout, no lse: o_bf16 is byte-equal to lr2_self_attn_fwd_bf16_train_blocked's at
 * drop_p = 0.  head_dim 64, any L >= 1 (so 1 <= L <= 288 can be run in both forms), one workgroup of 8 waves per (sequence, head, chunk
 * of 512 queries).  Inference only.  NOT the parity path: lr2_self_attn_fwd stays the default, and lr2_self_attn_fwd_bf16 is unchanged.
 * LR2_ERR_ARG: a NULL q / k / v / seg; no output at all; o_q without o_scales or the reverse; q / k / v / o_f32 not 16-byte, o_bf16 not
 * 8-byte or o_q not 4-byte aligned; batch or heads <= 0.  LR2_ERR_SHAPE: head_dim != 64; L < 1; ld or ld_o below heads * 64 or no
 * multiple of 8; ld_o % 32 when o_q is given.  Nothing is launched by a rejected call.
 * replaces: tencentpretrain/layers/multi_headed_attn.py:60-74 in those modes at the sequence lengths lr2_self_attn_fwd_bf16 does not
 * serve. */
int lr2_self_attn_fwd_bf16_blocked(const void* q, const void* k, const void* v, int ld, const int64_t* seg, void* o_f32, void* o_q,
                                   void* o_scales, void* o_bf16, int ld_o, int batch, int heads, int L, int head_dim, float scale,
                                   void* stream);
/* Diagnostic: *count = accepted lr2_self_attn_fwd_bf16_blocked calls since the library was loaded (a plain host counter, not
 * synchronised).  LR2_ERR_ARG for a NULL count.
 * replaces: nothing (a test hook, as lr2_self_attn_bf16_blocked_launch_counts: which attention a schedule ran). */
int lr2_self_attn_fwd_bf16_blocked_launch_count(uint64_t* count);

/* ABI 27.  The single-pass f16 inference mode (FeatureExtractor(precision="f16")): the "bf16" mode's entry points with
 * every single plane in IEEE binary16 -- 11 significand bits per operand instead of 8, the same bytes, the same matrix rate
 * (v_mfma_f32_16x16x32_f16).  NOT the parity path.  An f16 plane is written by ONE rule everywhere: clamp to +-65504 (an outlier
 * saturates, it does not become inf), round to nearest even, NaN stays NaN, results below 2^-14 are IEEE subnormals.
 *
 * lr2_gemm_f16: C[M, N] = A[M, K] . B[N, K]^T with A and B ONE f16 plane each (row strides lda / ldb elements, a_bytes / b_bytes
 * addressable from each pointer: rows past the end read as zero), fp32 accumulate; lr2_gemm_bf16's inference contract: alpha, bias,
 * act 0 / 1 (GELU), resid; the result goes to out (fp32) and / or out_hi -- ONE f16 plane when out_lo_off == 0, bf16 hi / lo planes (as
 * ever: the operands of lr2_self_attn_fwd) otherwise.  It runs on the 256 x 256 kernel of csrc/gemm256_f16.hip (the tile rule of
 * lr2_gemm256_tile_rows) at every size.  LR2_ERR_ARG: NULL operands / epilogue, no destination, dropout, act 2, accumulate, out_z, the
 * fused optimizer step, column sums.  LR2_ERR_SHAPE: K % 64, lda / ldb % 8, N % 4, an epilogue leading dimension % 4 or smaller than N,
 * lda / ldb < K, a_bytes / b_bytes > 4 GiB - 768 B.  Nothing is launched (and nothing counted) by a rejected call.
 * replaces: nn.Linear forward (tencentpretrain/layers/position_ffn.py:12-15, multi_headed_attn.py:55-76) in that mode. */
int lr2_gemm_f16(const void* A, const void* B, int M, int N, int K, int lda, int ldb, uint64_t a_bytes, uint64_t b_bytes,
                 const lr2_epilogue* epi, void* stream);
/* Diagnostic: *count = accepted lr2_gemm_f16 and lr2_gemm_f16_tiled calls since the library was loaded, one per call (a plain host
 * counter, not synchronised).
 * replaces: nothing (a test hook, as lr2_gemm_bf16_launch_counts). */
int lr2_gemm_f16_launch_count(uint64_t* count);
/* Added within ABI 27 (purely additive: no signature or struct changes).  lr2_gemm_f16's product with lr2_gemm_bf16's parameter list
 * and dispatch: the same operands, epilogue contract, argument checks and return codes as lr2_gemm_f16, and
 *   block_m == 256: the 256 x 256 f16 kernel under lr2_gemm_row_split_plan, as lr2_gemm_bf16 does it -- the leading whole rounds of the
 *       chip on csrc/gemm256_f16.hip, the remaining rows on the 128- / 64-row f16 kernels (A and every set epilogue pointer advanced by
 *       the plan's rows of its own leading dimension); no plan: lr2_gemm_f16's single launch.  LR2_ERR_SHAPE for a_bytes / b_bytes
 *       > 4 GiB - 768 B (that kernel's limit; only this block_m checks it).
 *   block_m == 128 / 64: the whole product on the f16 instantiations of the general kernel family (csrc/gemm.hip: 128 x 128 / 64 x 128
 *       tiles, 4 waves, one v_mfma_f32_16x16x32_f16 product per tile pair); any other block_m is treated as 128 (the family's rule).
 *       LR2_ERR_SHAPE for a_bytes / b_bytes >= 4 GiB (lr2_gemm_bf16's rule).
 * Each accumulator runs through k in ascending 32-wide MFMA steps in either kernel and the epilogue code is shared, so the tile height
 * changes no result bit (tests assert it).  lr2_gemm_f16_launch_count counts the accepted calls of lr2_gemm_f16 AND of this entry point,
 * one per call.  Nothing is launched (and nothing counted) by a rejected call.
 * replaces: nn.Linear forward (tencentpretrain/layers/position_ffn.py:12-15, multi_headed_attn.py:55-76) in that mode, at the sizes
 * where a launch is not many whole rounds of 256-row tiles; lr2_gemm_f16 is unchanged. */
int lr2_gemm_f16_tiled(const void* A, const void* B, int M, int N, int K, int lda, int ldb, uint64_t a_bytes, uint64_t b_bytes,
                       const lr2_epilogue* epi, int block_m, void* stream);
/* Diagnostic (added within ABI 27): kernel launches issued by lr2_gemm_f16 and lr2_gemm_f16_tiled since the library was loaded --
 * counts[0] the 256 x 256 f16 kernel, counts[1] the f16 kernels of the general family; a row-split call adds one to each (no device
 * call; plain host counters, not synchronised).
 * replaces: nothing (a test hook, as lr2_gemm_bf16_launch_counts). */
int lr2_gemm_f16_launch_counts(uint64_t counts[2]);
/* lr2_layernorm_fwd with the single plane in f16: the arguments of its out_lo_off = 0 form (out fp32 and / or out_f16, optional mean /
 * rstd, mode 0 = nn.LayerNorm / 1 = the TencentPretrain LayerNorm, the group / group_stride row map).  D % 4 == 0, D <= 1024.
 * replaces: tencentpretrain/layers/layer_norm.py:5-21 (and nn.LayerNorm, finetune/xit.py:37) in front of a product of that mode. */
int lr2_layernorm_fwd_f16(const void* x, const void* gamma, const void* beta, void* out, void* out_f16, void* mean, void* rstd, int rows,
                          int D, float eps, int mode, int group, uint64_t group_stride, void* stream);
/* dst[i] = f16(src[i]), n fp32 elements -> ONE f16 plane by the rule above: the mode's weights (once per weight refresh), its post-LN
 * first-layer operand, the context of its fallback attention.  n % 4 == 0; src 16-byte, dst 8-byte aligned (else LR2_ERR_SHAPE).
 * replaces: the .half() casts of the 16-bit configuration (BASELINE.json configs[2]; tencentpretrain/utils/ has no kernel of its own). */
int lr2_round_f16(const void* src, void* dst, uint64_t n, void* stream);
/* lr2_self_attn_fwd_bf16 on f16 planes (csrc/selfattn_mx.hip): q / k / v ONE f16 plane each (row stride ld elements; the three column
 * blocks of the [rows, 3E] plane lr2_gemm_f16 writes), S and O on the f16 MFMA, fp32 softmax with the row sum of the unrounded
 * probabilities, the un-normalised probabilities rounded to f16 as the A operand of P V, key mask -10000 * (seg <= 0) after the scale;
 * the context rows leave as fp32 (o_f32 [batch * L, ld_o]) and / or as ONE f16 plane (o_f16 [batch * L, ld_o]: the A operand of
 * lr2_gemm_f16).  No MX-FP8 outputs.  One workgroup per (sequence, head), or persistent workgroups under lr2_self_attn_fwd_bf16_plan's
 * rule.  head_dim 64, 1 <= L <= 288, inference only.  LR2_ERR_ARG: a NULL q / k / v / seg, no output, batch / heads / L <= 0.
 * LR2_ERR_SHAPE: head_dim != 64, L > 288, ld % 8, ld or ld_o below heads * 64, ld_o % 4.  Nothing is launched by a rejected call.
 * replaces: tencentpretrain/layers/multi_headed_attn.py:60-74 in that mode. */
int lr2_self_attn_fwd_f16(const void* q, const void* k, const void* v, int ld, const int64_t* seg, void* o_f32, void* o_f16, int ld_o,
                          int batch, int heads, int L, int head_dim, float scale, void* stream);
/* Diagnostic: *count = accepted lr2_self_attn_fwd_f16 calls since the library was loaded.
 * replaces: nothing (a test hook, as lr2_self_attn_fwd_bf16_blocked_launch_count: which attention a schedule ran). */
int lr2_self_attn_fwd_f16_launch_count(uint64_t* count);
/* Added within ABI 27 (purely additive: no signature or struct changes).  lr2_self_attn_fwd_f16 for sequences longer than one
 * LDS-resident head (FeatureExtractor(precision="f16", f16_attention_long=True); csrc/selfattn_mx_blocked.hip): that call's
 * argument list, layout, key mask and two outputs -- q / k / v ONE f16 plane each (row stride ld), the context rows out as fp32 (o_f32
 * [batch * L, ld_o]) and / or as ONE f16 plane (o_f16 [batch * L, ld_o]: clamp to +-65504, round to nearest even of the fp32 context);
 * any non-empty subset -- with the keys walked in blocks through LDS by lr2_self_attn_fwd_bf16_blocked's loop on the f16 MFMA:
 * lr2_self_attn_bf16_blocked_plan's fwd_key_block keys per block, per 16-query sub-tile a running maximum m, the fp32 sum l of the
 * unrounded p~ = exp2(s - m) and the un-normalised accumulator, both rescaled by exp2(m - m') when m grows; p~ (in (0, 1]) rounded to
 * f16 (nearest even, subnormals kept) as the A operand of P V; context = accumulator / l.  No dropout, no lse, no MX-FP8 outputs.
 * head_dim 64, any L >= 1 (so 1 <= L <= 288 can be run in both forms), one workgroup of 8 waves per (sequence, head, chunk of 512
 * queries).  Inference only.  NOT the parity path: lr2_self_attn_fwd stays the default, and lr2_self_attn_fwd_f16 is unchanged (it still
 * answers LR2_ERR_SHAPE at L = 289).
 * LR2_ERR_ARG: a NULL q / k / v / seg; no output at all; q / k / v / o_f32 not 16-byte or o_f16 not 8-byte aligned; batch or heads <= 0.
 * LR2_ERR_SHAPE: head_dim != 64; L < 1; ld % 8; ld_o % 4; ld or ld_o below heads * 64.  Nothing is launched (and nothing counted) by a
 * rejected call.
 * replaces: tencentpretrain/layers/multi_headed_attn.py:60-74 in that mode at the sequence lengths lr2_self_attn_fwd_f16 does not
 * serve. */
int lr2_self_attn_fwd_f16_blocked(const void* q, const void* k, const void* v, int ld, const int64_t* seg, void* o_f32, void* o_f16,
                                  int ld_o, int batch, int heads, int L, int head_dim, float scale, void* stream);
/* Diagnostic (added within ABI 27): *count = accepted lr2_self_attn_fwd_f16_blocked calls since the library was loaded (a plain host
 * counter, not synchronised).  LR2_ERR_ARG for a NULL count.
 * replaces: nothing (a test hook, as lr2_self_attn_fwd_f16_launch_count: which attention a schedule ran). */
int lr2_self_attn_fwd_f16_blocked_launch_count(uint64_t* count);

/* ABI 20.  MX-FP8 encoder training (FeatureExtractor(precision="mxfp8_train")): the backward's operands, blocked along the axis its
 * products reduce over, and a K-sliced weight-gradient product.
 *   lr2_quant_mxfp8_t: x [rows, cols] -- fp32 (is_planes 0) or bf16 hi / lo planes with the lo plane lo_off elements behind (is_planes 1),
 *                      row stride ldx -- through the prologue act (0: x; 1: GELU(x); 2: x * GELU'(z), z fp32 [rows, ld_z]) -> qt / st
 *                      (both or neither): MX-FP8 of x^T, [cols, rows_pad] bytes + [cols, rows_pad / 32] scales (rows_pad = rows rounded
 *                      up to 128, padding zero bytes); q / scales (both or neither; qt or q required): the row-blocked MX-FP8 of the same values, byte-identical to
 *                      lr2_quant_mxfp8; colsum / partials (both or neither): fp32 column sums [cols] written (accumulate 0) or added
 *                      (1), deterministic, through partials [rows_pad / 128, cols].  cols % 64 == 0; x, z, qt, q 16-byte aligned (planes:
 *                      8-byte), else LR2_ERR_SHAPE.
 * replaces: the split into bf16 planes of the backward's operands (lr2_split_planes / lr2_split_planes_t) and lr2_colsum, in that mode. */
int lr2_quant_mxfp8_t(const void* x, int is_planes, uint64_t lo_off, int ldx, const void* z, int ld_z, int act, void* qt, void* st,
                      void* q, void* scales, void* colsum, void* partials, int accumulate, int rows, int cols, void* stream);
/*   lr2_gemm_mxfp8_wgrad: out[M, ld_out] (+)= A_q . B_q^T with A_q [M, K], B_q [N, K] as lr2_quant_mxfp8_t writes them (K = the padded
 *                      token count); `splits` K slices (capped at K / 128) leave fp32 partials in workspace [splits, M, N] that one more
 *                      launch sums in slice order: the same bits on every run.  splits == 1: no workspace.  M, N, K % 128 == 0;
 *                      out and workspace 16-byte aligned.  LR2_ERR_SHAPE: M, N or K % 128, ld_out < N, ld_out % 4, alignment;
 *                      LR2_ERR_ARG: a NULL operand or out, splits < 1, more than one (capped) slice without a workspace; a refused
 *                      call writes nothing.
 * replaces: the TN weight-gradient products of planes (lr2_gemm with trans_a = trans_b = 1), in that mode. */
int lr2_gemm_mxfp8_wgrad(const void* a_q, const void* a_scales, const void* b_q, const void* b_scales, void* out, int ld_out,
                         int accumulate, void* workspace, int splits, int M, int N, int K, void* stream);
/*   lr2_dropout_residual: out[n] = resid + dropout_mask(y) / (1 - p), the mask of lr2_dropout_apply (element index = flat index);
 *                      y, resid, out 16-byte aligned.
 * replaces: the fused dropout + residual epilogue of lr2_gemm behind an MX-FP8 product (dropout_1 / dropout_2 of a layer). */
int lr2_dropout_residual(const void* y, const void* resid, void* out, uint64_t n, float drop_p, uint64_t drop_seed, uint32_t drop_site,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LR2PPO_HIP_H */
