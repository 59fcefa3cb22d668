"""Thin torch-tensor wrappers over the C ABI (include/lr2ppo_hip.h).

PyTorch is used for device memory and streams only: every wrapper passes raw device pointers and the
current HIP stream to the native library.  All tensors are fp32, contiguous, on a HIP device.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
import os
from typing import Optional

import torch

from . import _native as _nat

# GEMM precision: 3 = split-bf16 (fp32-grade, parity mode, default); 1 = single bf16 pass.
_PASSES = 3


def set_gemm_passes(p: int):
    global _PASSES
    if p not in (1, 3):
        raise ValueError("passes must be 1 or 3")
    _PASSES = p


def get_gemm_passes() -> int:
    return _PASSES


# ---- optional per-launch timing (bench.py): HIP events on the launch stream around selected entry points ----
_PROF = None
_PROF_ONLY = None

# Kernels of this package write parameters through raw pointers (the optimizer), which torch's tensor version counters do not see:
# every parameter such a kernel updates gets its own write counter bumped (mark_params_written), and caches of derived data (weight
# planes) compare it next to p._version.  Per parameter, not global: the PPO heads' optimizer steps must not invalidate the frozen
# encoders' weight planes (round 2's single global epoch re-split both stacks' weights on every step of the composed loop).
def mark_params_written(params):
    for p in params:
        p._lr2_writes = getattr(p, "_lr2_writes", 0) + 1


def param_write_count(p) -> int:
    return getattr(p, "_lr2_writes", 0)


def profile_start(only=None):
    """Start collecting (start, end) HIP events per kernel signature; see profile_stop().  `only`: a collection of
    signatures to restrict the collection to (two event records per launch cost ~25 us of host time; with ~120 timed
    launches per PPO step that alone can make the step host-bound)."""
    global _PROF, _PROF_ONLY
    _PROF = {}
    _PROF_ONLY = None if only is None else frozenset(only)


def profile_stop():
    """-> {key: {"ms": total, "n": launches, "flops": per-launch, "bytes": per-launch}} (synchronises)."""
    global _PROF
    prof, _PROF = _PROF, None
    torch.cuda.synchronize()
    out = {}
    for key, rec in (prof or {}).items():
        ms = sum(s.elapsed_time(e) for s, e in rec["ev"])
        out[key] = {"ms": ms, "n": len(rec["ev"]), "flops": rec["flops"], "bytes": rec["bytes"]}
    return out


class _Timed:
    __slots__ = ("key", "flops", "bytes", "s")

    def __init__(self, key, flops=0, nbytes=0):
        self.key, self.flops, self.bytes = key, flops, nbytes

    def __enter__(self):
        self.s = None
        if _PROF is not None and (_PROF_ONLY is None or self.key in _PROF_ONLY):
            self.s = torch.cuda.Event(enable_timing=True)
            self.s.record()
        return self

    def __exit__(self, *exc):
        if self.s is not None and _PROF is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            rec = _PROF.setdefault(self.key, {"ev": [], "flops": self.flops, "bytes": self.bytes})
            rec["ev"].append((self.s, e))
        return False


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _stream():
    # torch.cuda.current_stream() builds a Stream object through several Python layers (~8 us, 300 launches per PPO
    # step); the raw handle of the same stream comes straight from the C++ side in ~0.3 us
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())


def _chk_f32(*ts):
    for t in ts:
        if t is None:
            continue
        if t.dtype != torch.float32 or not t.is_cuda:
            raise TypeError(f"expected a float32 HIP tensor, got {t.dtype} on {t.device}")


class Drop:
    """Dropout spec for one site: p, seed, site id (see csrc/common.h::dropout_keep).  seed_dev: int64[1] device tensor whose
    value the kernels ADD to `seed` at run time (HIP-graph capture of a training step, StepScalars)."""
    __slots__ = ("p", "seed", "site", "seed_dev")

    def __init__(self, p: float, seed: int, site: int, seed_dev: Optional[torch.Tensor] = None):
        self.p, self.seed, self.site, self.seed_dev = float(p), int(seed), int(site), seed_dev

    def seed_dev_ptr(self):
        return self.seed_dev.data_ptr() if self.seed_dev is not None else None


class StepScalars:
    """The per-step scalars of a captured training step, in device memory (lr2_step_scalars_store): the dropout seed and up to
    14 learning rates.  store() is one small launch whose kernel arguments carry the values."""
    MAX_LRS = 14

    def __init__(self, device):
        self.buf = torch.zeros(8, dtype=torch.int64, device=device)
        self.seed = self.buf[0:1]
        self._lr_view = self.buf.view(torch.float32)
        self._lrs = (C.c_float * self.MAX_LRS)()
        self.n_lrs = 0

    def new_lr(self) -> int:
        if self.n_lrs >= self.MAX_LRS:
            raise ValueError("StepScalars holds at most 14 learning rates")
        self.n_lrs += 1
        return self.n_lrs - 1

    def lr_tensor(self, slot: int) -> torch.Tensor:
        return self._lr_view[2 + slot:3 + slot]

    def store(self, seed: int, lrs):
        for i, v in enumerate(lrs):
            self._lrs[i] = v
        _nat.check(_nat.lib().lr2_step_scalars_store(self.buf.data_ptr(), int(seed) & 0xFFFFFFFFFFFFFFFF, self._lrs, len(lrs),
                                                     _stream()), "lr2_step_scalars_store")


class Planes:
    """A matrix stored as two bf16 planes [hi | lo] (x = hi + lo) -- the operand format of the split-bf16 GEMM.
    Same bytes as the fp32 [rows, cols] tensor it replaces.  `lo_off` = elements from the hi plane to the lo plane."""
    __slots__ = ("buf", "rows", "cols", "lo_off", "transposed")

    def __init__(self, buf: torch.Tensor, rows: int, cols: int, lo_off: Optional[int] = None):
        self.transposed = False      # True: this is W^T [in, out] of an nn.Linear weight (see split_planes_t)
        if buf.dtype != torch.int16 or not buf.is_cuda:
            raise TypeError("Planes storage must be an int16 HIP tensor")
        self.buf, self.rows, self.cols = buf, rows, cols
        self.lo_off = rows * cols if lo_off is None else lo_off
        if buf.numel() < self.lo_off + rows * cols:
            raise ValueError("Planes storage too small")

    @staticmethod
    def empty(rows: int, cols: int, device) -> "Planes":
        return Planes(torch.empty(2 * rows * cols, dtype=torch.int16, device=device), rows, cols)

    def data_ptr(self) -> int:
        return self.buf.data_ptr()

    def plane_bytes(self) -> int:
        return self.rows * self.cols * 2

    def to_float(self) -> torch.Tensor:
        """hi + lo as fp32 (tests / debugging only)."""
        n = self.rows * self.cols
        hi = self.buf[:n].view(torch.bfloat16).float()
        lo = self.buf[self.lo_off:self.lo_off + n].view(torch.bfloat16).float()
        return (hi + lo).view(self.rows, self.cols)


def split_planes(src: torch.Tensor, dst: Planes):
    _chk_f32(src)
    n = src.numel()
    _nat.check(_nat.lib().lr2_split_planes(src.data_ptr(), dst.data_ptr(), dst.lo_off, n, _stream()), "lr2_split_planes")
    return dst


def split_planes_t(src: torch.Tensor, dst: Planes):
    """dst [C, R] planes = transpose of the fp32 matrix src [R, C]; marks dst as a transposed weight."""
    _chk_f32(src)
    R, C = src.shape
    if dst.rows != C or dst.cols != R or not src.is_contiguous():
        raise ValueError("split_planes_t: dst must be [C, R] planes of a contiguous [R, C] matrix")
    _nat.check(_nat.lib().lr2_split_planes_t(src.data_ptr(), dst.data_ptr(), dst.lo_off, R, C, _stream()), "lr2_split_planes_t")
    dst.transposed = True
    return dst


def dropout_planes(src: torch.Tensor, dst: Planes, drop: Optional[Drop]):
    """dst = planes of dropout_mask(src) / (1 - p) (drop None / p = 0: plain split)."""
    _chk_f32(src)
    p, seed, site = (drop.p, drop.seed, drop.site) if drop is not None else (0.0, 0, 0)
    _nat.check(_nat.lib().lr2_dropout_planes(src.data_ptr(), dst.data_ptr(), dst.lo_off, src.numel(), p, seed, site, _stream()),
               "lr2_dropout_planes")
    return dst


def dropout_apply(src: torch.Tensor, dst: torch.Tensor, drop: Optional[Drop]):
    """dst = dropout_mask(src) / (1 - p) (fp32; drop None / p = 0: copy)."""
    _chk_f32(src, dst)
    if drop is None or drop.p <= 0.0:
        if dst.data_ptr() != src.data_ptr():
            dst.copy_(src)
        return dst
    _nat.check(_nat.lib().lr2_dropout_apply(src.data_ptr(), dst.data_ptr(), src.numel(), drop.p, drop.seed, drop.site, _stream()),
               "lr2_dropout_apply")
    return dst


def text_embed_bwd(dx, src, seg, dword, dseg, *, rows, D):
    """dword[t] = sum of dx rows whose token is t (rows of tokens PRESENT in src are overwritten, all others left as they are:
    zero the table first; a caller accumulating into a live table must add the result itself); dseg[s] = sum of dx rows with
    segment s.  Deterministic: rows are grouped by token with a stable device sort, summed in row order inside pieces of 256
    sorted positions and the pieces of a long run (the padding id) in piece order (no float atomics)."""
    _chk_f32(dx, dword, dseg)
    if src.dtype != torch.int64 or seg.dtype != torch.int64:
        raise TypeError("src / seg must be int64")
    sorted_ids, order = torch.sort(src.view(-1), stable=True)
    rpb, wseg = 64, 256                                          # LR2_TEXT_EMBED_BWD_ROWS_PER_BLOCK / _WORD_SEG
    n_seg = dseg.shape[0]
    partials = torch.empty(((rows + rpb - 1) // rpb) * n_seg * D, dtype=torch.float32, device=dx.device)
    wpart = torch.empty(2 * ((rows + wseg - 1) // wseg) * D, dtype=torch.float32, device=dx.device)
    _nat.check(_nat.lib().lr2_text_embed_bwd(dx.data_ptr(), sorted_ids.data_ptr(), order.data_ptr(), seg.data_ptr(),
                                             dword.data_ptr(), dseg.data_ptr(), partials.data_ptr(), wpart.data_ptr(), rows, D,
                                             dword.shape[0], n_seg, _stream()), "lr2_text_embed_bwd")


def split_planes_multi(table_dev: torch.Tensor, n_chunks: int):
    _nat.check(_nat.lib().lr2_split_planes_multi(table_dev.data_ptr(), n_chunks, _stream()), "lr2_split_planes_multi")


class AdamArgs:
    """AdamW step fused into a weight-gradient GEMM (lr2_epilogue.adam_*): the GEMM result is the gradient of `p` and is
    consumed on the fly -- m, v, p are updated exactly as lr2_adamw_multi would, the gradient never reaches HBM."""
    __slots__ = ("p", "m", "v", "lr", "beta1", "beta2", "eps", "weight_decay", "lr_dev", "gscale_dev", "norm_slot")

    def __init__(self, p, m, v, lr, beta1, beta2, eps, weight_decay, lr_dev: Optional[torch.Tensor] = None,
                 gscale_dev: Optional[torch.Tensor] = None, norm_slot: Optional[torch.Tensor] = None):
        self.lr_dev = lr_dev        # float32[1] device tensor read by the kernel in place of lr (captured steps)
        # gradient-norm clipping (AdamW.set_grad_clip): float32[1] device tensor the gradient is multiplied by before the update, and
        # the float64[1] slot the producer of the gradient owes its squared norm to before the coefficient is formed
        self.gscale_dev, self.norm_slot = gscale_dev, norm_slot
        _chk_f32(p, m, v)
        if not (p.is_contiguous() and m.is_contiguous() and v.is_contiguous() and p.shape == m.shape == v.shape):
            raise ValueError("AdamArgs: p, m, v must be contiguous and of one shape")
        self.p, self.m, self.v = p, m, v
        self.lr, self.beta1, self.beta2, self.eps, self.weight_decay = lr, beta1, beta2, eps, weight_decay


def use_gemm256(M: int, N: int, K: int) -> bool:
    return _use_gemm256(M, N, K, _PASSES)


@functools.lru_cache(maxsize=4096)
def _use_gemm256(M: int, N: int, K: int, passes: int) -> bool:
    """True when an NT product of planes should run on the 256 x 256 ping-pong kernel (csrc/gemm256.hip): whole 32-deep K
    steps and enough 256 x 256 tiles that the last round of one-workgroup-per-CU rounds is well filled.  Measured on
    MI355X (tools/gemm_bench.py --planes): M = 100864 (ViT-B/16 over 512 frames) 355-385 TFLOP/s at K = 768 and ~460 at
    K = 3072 against 310-325 / 355 for the 128-row kernels; at M = 12544 (0.6-2.3 rounds) the two are level."""
    if K % 32 or passes != 3:
        return False
    tiles = ((M + 255) // 256) * ((N + 255) // 256)
    rounds = -(-tiles // 256)
    if tiles >= 256 and tiles >= 0.85 * rounds * 256:
        return True
    # round 4 (tools/dbg/rowsplit_ab.py): more than one round with a last round LESS than half full -- lr2_gemm then sends the rows of
    # the whole rounds to the 256 x 256 kernel and the remaining rows to the 128- / 64-row kernels (row split: two launches, no
    # reduction): M = 12544, N = 3072, K = 768 (588 tiles) 166 us against 199 (NN on 128-row tiles) / 184 (three rounds of 256 x 256)
    if 256 < tiles < 5 * 256 and 0 < tiles % 256 < 128 and K % 64 == 0:
        return True
    # one partial round, long contraction (M = 12544, N = 768, K = 3072: 147 tiles): each CU runs one tile at the 256 x 256 kernel's
    # main-loop rate and the epilogue is amortised over 96 K steps -- 182 us against 197 (64-row tiles) / 212 (128-row), round 3;
    # round 4: also three quarters of a round at K >= 1024 (M = 12544, N = 1024, K = 1024: 196 tiles, 77 us against 86)
    if (128 <= tiles <= 256 and K >= 2304) or (192 <= tiles <= 256 and K >= 1024):
        return True
    # round 4, late: the kernel's 192-row tile (gemm256.hip, MIH = 3; the launcher takes it when a round of 192-row tiles fills CUs a
    # round of 256-row tiles leaves idle): M = 12544, N = 768: 147 -> 198 workgroups -- K = 768: 50 us against 56 (64-row tiles),
    # K = 1536: 80 against 94 (profiles/experiments/README.md F.6)
    t192 = ((M + 191) // 192) * ((N + 255) // 256)
    return tiles < 256 and 192 <= t192 <= 256 and t192 > tiles and K >= 768


@functools.lru_cache(maxsize=4096)
def _gemm256_tn_splits(M: int, N: int, K: int, passes: int) -> int:
    """K-split count when the TN product C[M, N] = A[K, M]^T B[K, N] of planes should run on the TN form of the 256 x 256 kernel
    (csrc/gemm256.hip::gemm256_tn_kernel), else 0.  Weight gradients at thousands of token rows: few output tiles (768 x 3072 =
    36), a long contraction; tiles x splits fill ONE round of the 256 CUs, each workgroup runs >= 16 K steps of 32 rows."""
    if passes != 3 or K < 4096 or os.environ.get("LR2_GEMM_256_TN", "1") == "0":
        return 0
    tiles = ((M + 255) // 256) * ((N + 255) // 256)
    if tiles > 128 or M * N < 0.85 * tiles * 65536:
        return 0
    steps = (K + 31) // 32
    return max(1, min(256 // tiles, steps // 16))


@functools.lru_cache(maxsize=4096)
def choose_tiling(M: int, N: int, K: int, trans_a: bool, trans_b: bool = False):
    """(block_m, splits).  256 CUs hold 2 (BM=128) or 3 (BM=64) workgroups each; pick the split-K factor that minimises
    rounds x (K-tiles per workgroup + fixed prologue/epilogue cost) + the cost of writing/reading the partial slabs, so
    that skinny GEMMs fill the chip without wave-quantisation tails (576 workgroups on 512 slots = 2 rounds)."""
    if not trans_a and not trans_b and use_gemm256(M, N, K):
        return 256, 1        # honoured for planes x planes operands only (lr2_gemm falls back to 128-row tiles otherwise)
    if trans_a and trans_b:
        sp256 = _gemm256_tn_splits(M, N, K, _PASSES)
        if sp256:
            return 256, sp256    # planes x planes only, as above
    return _general_tiling(M, N, K, trans_a, trans_b)


@functools.lru_cache(maxsize=4096)
def _general_tiling(M: int, N: int, K: int, trans_a: bool, trans_b: bool):
    """choose_tiling's answer for the 128- / 64-row kernel family alone."""
    bm = 64 if (M <= 64 and not trans_a) else 128
    tiles = ((M + bm - 1) // bm) * ((N + 127) // 128)
    if bm == 128 and not trans_a and not trans_b and tiles < 1536:
        # NT with fewer than three rounds of 128-row tiles (512 resident workgroups): when the last round is poorly filled
        # it costs more than the lower intensity of 64-row tiles.  Measured with tools/gemm_bench.py: M=12544 N=768
        # (588 tiles) +9..15 %, M=6304 N=768 K=768 (300) +17 %, M=6304 N=3072 (1200) +17 %; full rounds (4096^3: 1024
        # tiles) and M=12544 N=3072 (2352) are 10-25 % faster with 128-row tiles.
        last = tiles % 512
        if (tiles > 512 and 0 < last <= 128) or (256 < tiles <= 512 and K < 1536):
            return 64, 1
    k_tiles = (K + 63) // 64
    slots = 768 if bm == 64 else 512
    if bm == 128 and not trans_a and tiles < 512 and K <= 1024 and ((M + 63) // 64) * ((N + 127) // 128) >= 64:
        # small short-K GEMMs (image tokens: M = 1024, K = 768): one pass of 64-row tiles beats split-K + its reduce launch
        # (NT 1024x768x768: 16.6 vs 19.0 us, NN 1024x3072x768: 21.9 vs 28.7 us)
        return 64, 1
    if tiles >= slots or k_tiles < 8:
        return bm, 1
    slab_cost = M * N * 6.4e-7            # one fp32 slab written + read, in units of one K-tile step (~2.5 us)
    best, best_cost = 1, None
    for s in range(1, min(k_tiles // 2, 64) + 1):
        per = -(-k_tiles // s)
        s_eff = -(-k_tiles // per)
        rounds = -(-(tiles * s_eff) // slots)
        cost = rounds * (per + 3.0) + (s_eff * slab_cost if s_eff > 1 else 0.0)
        if best_cost is None or cost < best_cost - 1e-9:
            best, best_cost = s_eff, cost
    return bm, best


def _LIB_GEMM(*args):
    """Bound on first use (the library is loaded lazily so that importing ops never needs the GPU)."""
    global _LIB_GEMM
    _LIB_GEMM = _nat.lib().lr2_gemm
    return _LIB_GEMM(*args)


def gemm(a, b, out: Optional[torch.Tensor], M: int, N: int, K: int, *, trans_a=False, trans_b=False,
         lda: Optional[int] = None, ldb: Optional[int] = None, ld_out: Optional[int] = None,
         bias: Optional[torch.Tensor] = None, act: int = 0, out_z: Optional[torch.Tensor] = None,
         aux_z: Optional[torch.Tensor] = None, resid: Optional[torch.Tensor] = None, drop: Optional[Drop] = None,
         accumulate: bool = False, alpha: float = 1.0, out_planes: Optional[Planes] = None,
         splitk_ws: Optional[torch.Tensor] = None, splits: Optional[int] = None, block_m: Optional[int] = None,
         passes: Optional[int] = None, adam: Optional[AdamArgs] = None, colsum: Optional[torch.Tensor] = None,
         colsum_ws: Optional[torch.Tensor] = None):
    """out[M,N] = op(a) @ op(b) with the fused epilogue; a / b are fp32 tensors or Planes; the result goes to `out`
    (fp32) and/or `out_planes`, or -- with `adam` -- straight into the AdamW update of adam.p[M,N].
    See lr2_gemm in include/lr2ppo_hip.h."""
    a_pl, b_pl = isinstance(a, Planes), isinstance(b, Planes)
    _chk_f32(None if a_pl else a, None if b_pl else b, out, bias, out_z, aux_z, resid)
    if lda is None:
        lda = M if trans_a else K
    if ldb is None:
        ldb = N if trans_b else K
    if ld_out is None:
        ld_out = N
    if block_m is None or splits is None:
        bm, sp = choose_tiling(M, N, K, trans_a, trans_b)
    if block_m is not None:
        bm = block_m
    if splits is not None:
        sp = splits
    if sp > 1:
        need = sp * M * N
        if splitk_ws is None or splitk_ws.numel() < need:
            raise ValueError(f"split-K workspace too small: need {need} floats")
    e = _nat.Epilogue()
    e.bias, e.resid, e.aux_z, e.out, e.out_z = _ptr(bias), _ptr(resid), _ptr(aux_z), _ptr(out), _ptr(out_z)
    e.ld_resid, e.ld_aux, e.ld_out, e.ld_z = _ld(resid, N), _ld(aux_z, N), ld_out, _ld(out_z, N)
    if out_planes is not None:
        e.out_hi, e.out_lo_off, e.ld_planes = out_planes.data_ptr(), out_planes.lo_off, out_planes.cols
    e.act, e.accumulate, e.alpha = act, 1 if accumulate else 0, alpha
    if drop is not None and drop.p > 0.0:
        e.drop_p, e.drop_seed, e.drop_site, e.drop_seed_dev = drop.p, drop.seed, drop.site, drop.seed_dev_ptr()
    if adam is not None:
        if out is not None or out_planes is not None or adam.p.numel() != M * N or ld_out != N:
            raise ValueError("gemm(adam=...): the result is consumed by the update; p must be [M, N] and out/out_planes None")
        e.adam_p, e.adam_m, e.adam_v = adam.p.data_ptr(), adam.m.data_ptr(), adam.v.data_ptr()
        e.adam_lr, e.adam_beta1, e.adam_beta2 = adam.lr, adam.beta1, adam.beta2
        e.adam_eps, e.adam_weight_decay = adam.eps, adam.weight_decay
        e.adam_lr_dev = adam.lr_dev.data_ptr() if adam.lr_dev is not None else None
        if adam.gscale_dev is not None:
            _chk_f32(adam.gscale_dev)
            e.adam_gscale_dev = adam.gscale_dev.data_ptr()
    if colsum is not None:
        # weight-gradient form: colsum[m] = sum_k A[k, m] (the bias gradient) from the same launch (lr2_epilogue.colsum)
        _chk_f32(colsum, colsum_ws)
        if not (trans_a and trans_b) or colsum.numel() != M or colsum_ws is None \
                or colsum_ws.numel() < max(128, sp * ((N + 255) // 256)) * M:
            raise ValueError("gemm(colsum=...): TN form only; colsum [M], colsum_ws >= max(128, splits * ceil(N / 256)) * M floats")
        e.colsum, e.colsum_ws = colsum.data_ptr(), colsum_ws.data_ptr()
    a_bytes = a.plane_bytes() if a_pl else a.numel() * 4
    b_bytes = b.plane_bytes() if b_pl else b.numel() * 4
    if trans_a and trans_b:
        # the kernels never compare a row with K: rows past it read as zero only because the extent ends there, so an operand that is
        # the first K rows of a taller buffer (a workspace, a Planes view) passes the extent of K rows, not of the allocation.  Whole
        # rows: an extent that ends inside a 16-byte load of row K - 1 would zero that row's last columns.
        a_bytes = min(a_bytes, K * lda * (2 if a_pl else 4))
        b_bytes = min(b_bytes, K * ldb * (2 if b_pl else 4))
    args = (a.data_ptr(), b.data_ptr(), M, N, K, lda, ldb, 1 if trans_a else 0, 1 if trans_b else 0, a_bytes, b_bytes,
            1 if a_pl else 0, a.lo_off * 2 if a_pl else 0, 1 if b_pl else 0, b.lo_off * 2 if b_pl else 0, C.byref(e),
            _ptr(splitk_ws), sp, bm, passes or _PASSES, _stream())
    if _PROF is None:               # the steady-state path: no label formatting, no event objects
        rc = _LIB_GEMM(*args)
    else:
        form = "TN" if trans_a else ("NN" if trans_b else "NT")
        src = ("p" if a_pl else "f") + ("p" if b_pl else "f")
        label = f"gemm_{form}_{src}_M{M}_N{N}_K{K}" + ("_adamw" if adam is not None else "")
        alg_bytes = 4.0 * (M * K + N * K) + (24.0 if adam is not None else 4.0) * M * N
        with _Timed(label, 2.0 * M * N * K, alg_bytes):
            rc = _LIB_GEMM(*args)
    if rc:
        _nat.check(rc, f"lr2_gemm(M={M},N={N},K={K},ta={trans_a},tb={trans_b},planes a={a_pl} b={b_pl})")
    return out if out is not None else out_planes


def _ld(t: Optional[torch.Tensor], default: int) -> int:
    return default if t is None else t.shape[-1]


def layernorm_fwd(x, gamma, beta, out, mean=None, rstd=None, *, rows, D, eps=1e-5, mode=0, group=0, group_stride=0,
                  out_planes: Optional[Planes] = None, out_plane: Optional[torch.Tensor] = None):
    """out (fp32) and/or out_planes receive LN(x); both use the (group, group_stride) row mapping.
    out_plane (instead of out_planes): the result as ONE bf16 plane (a 2-byte HIP tensor of rows * D elements, round to nearest
    even): the A operand of gemm_bf16."""
    _chk_f32(x, gamma, beta, out, mean, rstd)
    hi, lo_off = (out_planes.data_ptr(), out_planes.lo_off) if out_planes is not None else (None, 0)
    if out_plane is not None:
        if out_planes is not None:
            raise ValueError("layernorm_fwd: out_plane excludes out_planes")
        hi = _plane_ptr(out_plane, rows * D, "layernorm_fwd: out_plane")
    with _Timed(f"lnfwd_R{rows}_D{D}", 0.0, (6.0 if out_plane is not None else 8.0) * rows * D):
        name = "lr2_layernorm_fwd_wide" if D > 1024 else "lr2_layernorm_fwd"        # rows wider than four float4 per lane
        rc = getattr(_nat.lib(), name)(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(out), hi, lo_off, _ptr(mean),
                                       _ptr(rstd), rows, D, eps, mode, group, group_stride, _stream())
    _nat.check(rc, name)
    return out if out is not None else (out_planes if out_planes is not None else out_plane)


def _plane_ptr(t: torch.Tensor, numel: int, what: str) -> int:
    """data pointer of ONE bf16 plane: a 2-byte HIP tensor (int16 / bfloat16) of at least `numel` elements."""
    if t.element_size() != 2 or not t.is_cuda or t.numel() < numel:
        raise TypeError(f"{what} must be a 2-byte HIP tensor of at least {numel} elements")
    return t.data_ptr()


@functools.lru_cache(maxsize=4096)
def use_gemm256_b1(M: int, N: int, K: int) -> bool:
    """True when a single-pass bf16 product should run on the 256 x 256 ping-pong kernel (csrc/gemm256_b1.hip) rather than on the
    128- / 64-row family at passes = 1.  Fitted to tools/gemm_bench.py --bf16 --bm {256,128,64} on MI355X (us; 256 / 128 / 64 rows):
      M = 100864: N 3072 K 768  752 / 772 / -;  N 768 K 3072  481 / 672 / -;  N 2304 K 768  580 / 678 / -
      M = 12544:  N 3072 K 768  112 / 130 / -  (588 tiles: row split);  N 768 K 3072  85 / 119 / -  (147 tiles: 192-row tiles);
                  N 2304 K 768  83 / 102 / 87  (441 tiles);  N 768 K 768  34.8 / 48.6 / 35.0  (147 tiles)
      M = 6304:   N 2304 K 768  43.8 / 52.5 / 48.2  (225 tiles);  N 3072 K 768  67.9 / 74.1 / 65.4  (300 tiles);
                  N 768 K 768  32.6 / 25.5 / 20.6  (75 tiles);  N 768 K 3072  75.7 / 61.3 / 52.7  (75 tiles)
    -> the 256 x 256 kernel from half a round of tiles up, except just over one round (256 < tiles < 384: a second round less than
    half full, where the 64-row tiles are level or ahead)."""
    if K % 64:
        return False
    tiles = ((M + 255) // 256) * ((N + 255) // 256)
    return tiles >= 128 and not 256 < tiles < 384


def _bf16_fallback_block_m(M: int, N: int) -> int:
    """Tile height of the general family for a single-pass product the 256 x 256 kernel does not take: 64 rows below three rounds of
    128-row tiles (choose_tiling's threshold; ahead of 128 rows on every shape measured above), else 128."""
    return 64 if ((M + 127) // 128) * ((N + 127) // 128) < 1536 else 128


def gemm_bf16(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor], M: int, N: int, K: int, *,
              lda: Optional[int] = None, ldb: Optional[int] = None, ld_out: Optional[int] = None, bias: Optional[torch.Tensor] = None,
              act: int = 0, resid: Optional[torch.Tensor] = None, alpha: float = 1.0, out_plane: Optional[torch.Tensor] = None,
              out_planes: Optional[Planes] = None, planes_col: int = 0, block_m: Optional[int] = None):
    """out[M, N] = a[M, K] @ b[N, K]^T (+ bias) (act 1: GELU) (+ resid) as ONE bf16 pass (lr2_gemm_bf16): a, b are single bf16 planes
    (2-byte HIP tensors; a Planes matrix contributes its hi plane = bf16(x)).  The result goes to `out` (fp32) and / or ONE bf16
    plane `out_plane` (round to nearest even) or hi / lo `out_planes`.  Inference only: the bf16 mode, never the parity path.
    planes_col: the result's N columns go to columns [planes_col, planes_col + N) of a wider `out_planes` matrix [M, >= planes_col + N].
    block_m: 256 = the 256 x 256 single-pass kernel (any M), 128 / 64 = the general family; None: by size (use_gemm256_b1)."""
    _chk_f32(out, bias, resid)
    lda = K if lda is None else lda
    ldb = K if ldb is None else ldb
    if isinstance(a, Planes):
        a = a.buf[:a.rows * a.cols]
    if isinstance(b, Planes):
        b = b.buf[:b.rows * b.cols]
    a_ptr = _plane_ptr(a, (M - 1) * lda + K, "gemm_bf16: a")
    b_ptr = _plane_ptr(b, (N - 1) * ldb + K, "gemm_bf16: b")
    if out_plane is not None and out_planes is not None:
        raise ValueError("gemm_bf16: out_plane excludes out_planes")
    e = _nat.Epilogue()
    e.bias, e.resid, e.out = _ptr(bias), _ptr(resid), _ptr(out)
    e.ld_resid, e.ld_out = _ld(resid, N), (N if ld_out is None else ld_out)
    if out_plane is not None:
        e.out_hi, e.out_lo_off, e.ld_planes = _plane_ptr(out_plane, M * N, "gemm_bf16: out_plane"), 0, N
    elif out_planes is not None:
        if out_planes.rows != M or planes_col < 0 or planes_col % 4 or planes_col + N > out_planes.cols:
            raise ValueError("gemm_bf16: out_planes must be [M, >= planes_col + N], planes_col a multiple of 4")
        e.out_hi, e.out_lo_off, e.ld_planes = out_planes.data_ptr() + 2 * planes_col, out_planes.lo_off, out_planes.cols
    e.act, e.alpha = act, alpha
    if block_m is None:
        block_m = 256 if use_gemm256_b1(M, N, K) else _bf16_fallback_block_m(M, N)
    with _Timed(f"gemm_bf16_M{M}_N{N}_K{K}", 2.0 * M * N * K, 2.0 * (M * K + N * K) + (4.0 if out is not None else 2.0) * M * N):
        rc = _nat.lib().lr2_gemm_bf16(a_ptr, b_ptr, M, N, K, lda, ldb, a.numel() * 2, b.numel() * 2, C.byref(e), block_m, _stream())
    if rc:
        _nat.check(rc, f"lr2_gemm_bf16(M={M},N={N},K={K},block_m={block_m})")
    return out if out is not None else (out_plane if out_plane is not None else out_planes)


def gemm_bf16_launch_counts():
    """(launches of the 256 x 256 single-pass kernel, launches of the general family) by gemm_bf16 since the library was loaded."""
    c = (C.c_uint64 * 2)()
    _nat.check(_nat.lib().lr2_gemm_bf16_launch_counts(c), "lr2_gemm_bf16_launch_counts")
    return int(c[0]), int(c[1])


# ---- the single-pass f16 inference mode (FeatureExtractor(precision="f16")): the bf16 mode's ops with every single plane in f16 ------
def gemm_f16(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor], M: int, N: int, K: int, *,
             lda: Optional[int] = None, ldb: Optional[int] = None, ld_out: Optional[int] = None, bias: Optional[torch.Tensor] = None,
             act: int = 0, resid: Optional[torch.Tensor] = None, alpha: float = 1.0, out_plane: Optional[torch.Tensor] = None,
             out_planes: Optional[Planes] = None, planes_col: int = 0, block_m: Optional[int] = None):
    """out[M, N] = a[M, K] @ b[N, K]^T (+ bias) (act 1: GELU) (+ resid) as ONE f16 pass (lr2_gemm_f16): a, b are single f16 planes
    (2-byte HIP tensors: what round_f16, layernorm_fwd_f16, self_attn_fwd_f16 and this product write).  The result goes to `out`
    (fp32) and / or ONE f16 plane `out_plane` (clamped to +-65504, round to nearest even) or bf16 hi / lo `out_planes` (the operands of
    the 3-pass attention kernels).  Inference only: the f16 mode, never the parity path.
    block_m: None = lr2_gemm_f16, the 256 x 256 kernel at every size; 256 = that kernel under the row split of gemm_bf16 (whole rounds
    of the chip there, the remaining rows on short tiles), 128 / 64 = the f16 kernels of the general family (lr2_gemm_f16_tiled).  The
    tile height changes no result bit; f16_block_m is the measured rule the schedule follows.
    planes_col: as gemm_bf16."""
    _chk_f32(out, bias, resid)
    lda = K if lda is None else lda
    ldb = K if ldb is None else ldb
    a_ptr = _plane_ptr(a, (M - 1) * lda + K, "gemm_f16: a")
    b_ptr = _plane_ptr(b, (N - 1) * ldb + K, "gemm_f16: b")
    if out_plane is not None and out_planes is not None:
        raise ValueError("gemm_f16: out_plane excludes out_planes")
    e = _nat.Epilogue()
    e.bias, e.resid, e.out = _ptr(bias), _ptr(resid), _ptr(out)
    e.ld_resid, e.ld_out = _ld(resid, N), (N if ld_out is None else ld_out)
    if out_plane is not None:
        e.out_hi, e.out_lo_off, e.ld_planes = _plane_ptr(out_plane, M * N, "gemm_f16: out_plane"), 0, N
    elif out_planes is not None:
        if out_planes.rows != M or planes_col < 0 or planes_col % 4 or planes_col + N > out_planes.cols:
            raise ValueError("gemm_f16: out_planes must be [M, >= planes_col + N], planes_col a multiple of 4")
        e.out_hi, e.out_lo_off, e.ld_planes = out_planes.data_ptr() + 2 * planes_col, out_planes.lo_off, out_planes.cols
    e.act, e.alpha = act, alpha
    with _Timed(f"gemm_f16_M{M}_N{N}_K{K}", 2.0 * M * N * K, 2.0 * (M * K + N * K) + (4.0 if out is not None else 2.0) * M * N):
        if block_m is None:
            rc = _nat.lib().lr2_gemm_f16(a_ptr, b_ptr, M, N, K, lda, ldb, a.numel() * 2, b.numel() * 2, C.byref(e), _stream())
        else:
            if block_m not in (256, 128, 64):
                raise ValueError("gemm_f16: block_m is None, 256, 128 or 64")
            rc = _nat.lib().lr2_gemm_f16_tiled(a_ptr, b_ptr, M, N, K, lda, ldb, a.numel() * 2, b.numel() * 2, C.byref(e), block_m,
                                               _stream())
    if rc:
        _nat.check(rc, f"lr2_gemm_f16(M={M},N={N},K={K},block_m={block_m})")
    return out if out is not None else (out_plane if out_plane is not None else out_planes)


def gemm_f16_launch_count() -> int:
    """Accepted lr2_gemm_f16 and lr2_gemm_f16_tiled calls since the library was loaded (one per call)."""
    c = C.c_uint64(0)
    _nat.check(_nat.lib().lr2_gemm_f16_launch_count(C.byref(c)), "lr2_gemm_f16_launch_count")
    return int(c.value)


def gemm_f16_launch_counts():
    """(launches of the 256 x 256 f16 kernel, launches of the f16 kernels of the general family) by gemm_f16 since the library was
    loaded; a row-split call adds one to each."""
    c = (C.c_uint64 * 2)()
    _nat.check(_nat.lib().lr2_gemm_f16_launch_counts(c), "lr2_gemm_f16_launch_counts")
    return int(c[0]), int(c[1])


_F16_FORCE_256 = False


@contextlib.contextmanager
def f16_force_256():
    """Inside the block f16_block_m is bypassed: the f16 schedule (TransformerEncoder.forward_f16) passes block_m = None, i.e. every
    product is one lr2_gemm_f16 call on the 256 x 256 kernel (what tests compare the dispatched schedule with, bit for bit)."""
    global _F16_FORCE_256
    prev, _F16_FORCE_256 = _F16_FORCE_256, True
    try:
        yield
    finally:
        _F16_FORCE_256 = prev


def f16_schedule_block_m(M: int, N: int, K: int) -> Optional[int]:
    """The block_m the f16 schedule passes to gemm_f16: f16_block_m's, or None inside f16_force_256()."""
    return None if _F16_FORCE_256 else f16_block_m(M, N, K)


@functools.lru_cache(maxsize=4096)
def f16_block_m(M: int, N: int, K: int) -> int:
    """Tile height (256, 128 or 64) of a single-pass f16 product: the block_m gemm_f16 gets from the f16 schedule.  256 = the 256 x 256
    kernel under the row split (lr2_gemm_row_split_plan), 128 / 64 = the f16 kernels of the general family.  The tile height changes no
    result bit (tests/test_f16_tiles_gpu.py), so the rule is about time only.
    Fitted to tools/gemm_bench.py --f16 --f16-schedule-epilogues {--f16-unsplit, --bm 256, --bm 128, --bm 64} --iters 200 on MI355X --
    every product with the epilogue and destination forward_f16 gives it (N = 4 K: bias, GELU -> one f16 plane; N = 3 K: bias -> one
    f16 plane; else bias + residual -> fp32) --, a fresh process per run, the four variants alternating, each twice; us, mean of the
    two runs: lr2_gemm_f16 (one launch of the 256 x 256 kernel: what every product paid before) / block_m 256 (the row split where the
    plan has one) / 128 / 64 -> the rule's answer:
      M=100864 N=3072 K=768: 624.6 / 623.5 / 735.9 / 799.0 -> 256
      M=100864 N=768 K=3072: 484.8 / 485.2 / 713.9 / 761.9 -> 256
      M=100864 N=2304 K=768: 399.6 / 398.0 / 496.4 / 562.1 -> 256
      M=12544 N=3072 K=768: 102.3 / 96.5 / 112.9 / 115.8 -> 256     (588 tiles = 2.3 rounds: the row split, 10 752 rows + 1792 on 64-row tiles)
      M=12544 N=768 K=3072: 74.4 / 74.0 / 112.1 / 91.2 -> 256       (147 tiles: 192-row tiles)
      M=12544 N=2304 K=768: 59.1 / 58.8 / 73.8 / 72.9 -> 256        (441 tiles)
      M=12544 N=768 K=768: 28.9 / 28.8 / 43.9 / 34.7 -> 256         (147 tiles)
      M=6304 N=2304 K=768: 30.1 / 30.1 / 38.6 / 41.4 -> 256         (225 tiles)
      M=6304 N=3072 K=768: 62.0 / 53.7 / 58.7 / 59.0 -> 256         (300 tiles = 1.2 rounds: the row split, 5376 rows + 928 on 64-row tiles)
      M=6304 N=768 K=768: 24.4 / 24.4 / 23.8 / 19.1 -> 64           (75 tiles)
      M=6304 N=768 K=3072: 64.0 / 64.3 / 55.9 / 46.6 -> 64          (75 tiles)
    Spread between the two runs of one variant: at most 2.8 % (73.9 / 71.9), typically 0.3 %.  A shape class leaves lr2_gemm_f16's single
    launch only where the other form is ahead by more than that: the row split wherever the plan has one (- 6 % and - 13 %), 64-row
    tiles below half a round of 256 x 256 tiles (- 22 % and - 27 %); 128-row tiles win nowhere.  This is NOT use_gemm256_b1's rule: with
    the result leaving as one 2-byte plane the 256 x 256 kernel is 25-35 % faster than with an fp32 result and the short tiles gain
    less, so just over one round (256 < tiles < 384) the row split beats whole launches of 64-row tiles here.  (With a bare fp32 result
    -- the same command without --f16-schedule-epilogues -- M = 6304, N = 3072 reads 79.7 / 66.8 / 70.9 / 61.4: 64 rows would win by 8 %;
    the schedule never asks for that form at that width.  DESIGN 4 has that table.)  The 128-tile boundary is use_gemm256_b1's: measured on
    either side of it (75 and 147 tiles), not at it.
    K % 64 != 0 (never in the schedule; either kernel refuses it): a short tile, never the ring."""
    if K % 64:
        return 64                                       # (refused by either kernel; never the 256 x 256 ring)
    tiles = ((M + 255) // 256) * ((N + 255) // 256)
    return 256 if tiles >= 128 else 64


def layernorm_fwd_f16(x, gamma, beta, rows, D, eps, mode, *, group=0, group_stride=0, out=None, mean=None, rstd=None,
                      out_plane: Optional[torch.Tensor] = None):
    """layernorm_fwd with the single plane in f16 (lr2_layernorm_fwd_f16): LN(x) to `out` (fp32) and / or ONE f16 plane `out_plane` (a
    2-byte HIP tensor of rows * D elements: the A operand of gemm_f16); the (group, group_stride) row mapping as layernorm_fwd."""
    _chk_f32(x, gamma, beta, out, mean, rstd)
    if out is None and out_plane is None:
        raise ValueError("layernorm_fwd_f16: out and / or out_plane")
    hp = _plane_ptr(out_plane, rows * D, "layernorm_fwd_f16: out_plane") if out_plane is not None else None
    with _Timed(f"lnfwd_f16_R{rows}_D{D}", 0.0, (6.0 if out is None else 10.0 if out_plane is not None else 8.0) * rows * D):
        rc = _nat.lib().lr2_layernorm_fwd_f16(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(out), hp, _ptr(mean), _ptr(rstd),
                                              rows, D, eps, mode, group, group_stride, _stream())
    _nat.check(rc, "lr2_layernorm_fwd_f16")
    return out if out is not None else out_plane


def round_f16(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """dst = f16(src): an fp32 HIP tensor -> ONE f16 plane (a 2-byte HIP tensor of at least src.numel() elements) by the mode's plane
    writer (clamp to +-65504, round to nearest even; lr2_round_f16)."""
    _chk_f32(src)
    n = src.numel()
    with _Timed(f"round_f16_{n}", 0.0, 6.0 * n):
        rc = _nat.lib().lr2_round_f16(src.data_ptr(), _plane_ptr(dst, n, "round_f16: dst"), n, _stream())
    _nat.check(rc, "lr2_round_f16")
    return dst


def self_attn_fwd_f16(qkv: torch.Tensor, seg, *, batch, heads, L, head_dim, scale, out: Optional[torch.Tensor] = None,
                      out_plane: Optional[torch.Tensor] = None):
    """Encoder self-attention of the f16 mode (lr2_self_attn_fwd_f16).  qkv: ONE f16 plane [batch * L, 3E] = [Q | K | V] (a 2-byte HIP
    tensor: what gemm_f16(out_plane=...) writes); the context as fp32 `out` [batch * L, E] and / or as ONE f16 plane `out_plane` (a
    2-byte HIP tensor [batch * L, E])."""
    E = heads * head_dim
    if qkv.element_size() != 2 or not qkv.is_cuda or qkv.numel() < batch * L * 3 * E:
        raise TypeError("self_attn_fwd_f16: qkv is a 2-byte HIP tensor [batch * L, 3 * heads * head_dim]")
    if seg.dtype != torch.int64:
        raise TypeError("seg must be int64")
    _chk_f32(out)
    if out is None and out_plane is None:
        raise ValueError("self_attn_fwd_f16: out and / or out_plane")
    ob = _plane_ptr(out_plane, batch * L * E, "self_attn_fwd_f16: out_plane") if out_plane is not None else None
    base = qkv.data_ptr()
    with _Timed(f"selfattn_f16_B{batch}_H{heads}_L{L}", 4.0 * batch * heads * L * L * head_dim, 7.0 * batch * L * E):
        _nat.check(_nat.lib().lr2_self_attn_fwd_f16(base, base + 2 * E, base + 4 * E, 3 * E, seg.data_ptr(), _ptr(out), ob, E, batch,
                                                    heads, L, head_dim, scale, _stream()), "lr2_self_attn_fwd_f16")
    return out if out is not None else out_plane


def self_attn_fwd_f16_launch_count() -> int:
    """Accepted lr2_self_attn_fwd_f16 calls since the library was loaded."""
    c = C.c_uint64(0)
    _nat.check(_nat.lib().lr2_self_attn_fwd_f16_launch_count(C.byref(c)), "lr2_self_attn_fwd_f16_launch_count")
    return int(c.value)


def self_attn_fwd_f16_blocked(qkv: torch.Tensor, seg, *, batch, heads, L, head_dim, scale, out: Optional[torch.Tensor] = None,
                              out_plane: Optional[torch.Tensor] = None):
    """self_attn_fwd_f16 with the keys walked in blocks through LDS (lr2_self_attn_fwd_f16_blocked, csrc/selfattn_mx_blocked.hip): the
    same arguments, checks and outputs at any L >= 1 -- what the f16 inference schedule runs above 288 tokens with
    TransformerEncoder.f16_attention_long."""
    E = heads * head_dim
    if qkv.element_size() != 2 or not qkv.is_cuda or qkv.numel() < batch * L * 3 * E:
        raise TypeError("self_attn_fwd_f16_blocked: qkv is a 2-byte HIP tensor [batch * L, 3 * heads * head_dim]")
    if seg.dtype != torch.int64:
        raise TypeError("seg must be int64")
    _chk_f32(out)
    if out is None and out_plane is None:
        raise ValueError("self_attn_fwd_f16_blocked: out and / or out_plane")
    ob = _plane_ptr(out_plane, batch * L * E, "self_attn_fwd_f16_blocked: out_plane") if out_plane is not None else None
    base = qkv.data_ptr()
    with _Timed(f"selfattn_f16l_B{batch}_H{heads}_L{L}", 4.0 * batch * heads * L * L * head_dim, 7.0 * batch * L * E):
        _nat.check(_nat.lib().lr2_self_attn_fwd_f16_blocked(base, base + 2 * E, base + 4 * E, 3 * E, seg.data_ptr(), _ptr(out), ob, E,
                                                            batch, heads, L, head_dim, scale, _stream()), "lr2_self_attn_fwd_f16_blocked")
    return out if out is not None else out_plane


def self_attn_fwd_f16_blocked_launch_count() -> int:
    """Accepted self_attn_fwd_f16_blocked calls since the library was loaded (a test hook: which attention a schedule ran)."""
    c = C.c_uint64(0)
    _nat.check(_nat.lib().lr2_self_attn_fwd_f16_blocked_launch_count(C.byref(c)), "lr2_self_attn_fwd_f16_blocked_launch_count")
    return int(c.value)


# ---- single-pass bf16 products of encoder training (the "bf16_train" mode) --------------------------------------------
_BF16_TRAIN_FORCE_256 = False


@contextlib.contextmanager
def bf16_train_force_256():
    """Tests: inside the block every product of gemm_bf16_train that names no block_m goes to the 256 x 256 single-pass kernels,
    whatever its size (the encoder stacks of the tests are too small for the dispatch rule to send anything there)."""
    global _BF16_TRAIN_FORCE_256
    prev, _BF16_TRAIN_FORCE_256 = _BF16_TRAIN_FORCE_256, True
    try:
        yield
    finally:
        _BF16_TRAIN_FORCE_256 = prev


@functools.lru_cache(maxsize=4096)
def gemm256_tn_b1_splits(M: int, N: int, K: int) -> int:
    """K-split count when the single-pass weight gradient C[M, N] = A[K, M]^T B[K, N] should run on the 256 x 256 TN kernel
    (csrc/gemm256_tn_b1.hip), else 0 (the 128-row family at passes = 1).  _gemm256_tn_splits' rule for the 3-pass kernel -- few output
    tiles, a long contraction, tiles x splits in ONE round of the 256 CUs -- with K steps of 64 rows, at least 8 of them per workgroup.
    Fitted to tools/gemm_bench.py --bf16 --tn on MI355X, bias gradient included (us; this kernel at the rule's splits / the 128-row family
    at passes = 1 + its column-sum pass / the 3-pass 256 x 256 TN kernel), (N_out, N_in):
      T = 100864: (768, 3072) 553 / 724 / 1081;  (3072, 768) 490 / 773 / 1084;  (2304, 768) 377 / 620 / 824;  (768, 768) 146 / 248 / 296
      T = 12544:  (768, 3072) 85 / 98 / 149;     (3072, 768) 88 / 100 / 152;    (2304, 768) 74 / 78 / 122;    (768, 768) 43 / 46 / 60
    and to --bm 256 --splits {3, 4, 7, 9, 14, 18, 28, 56}: one full round is the optimum on every shape (36 tiles: 7 splits 554 us, 4
    694, 14 583; 27 tiles: 9 splits 385, 7 433, 18 407; 9 tiles: 28 splits 137, 14 208, 56 169; at T = 12544 24 splits 43, 14 46).
    -> the kernel wins all eight shapes; the rule is the 3-pass kernel's."""
    if K < 4096:
        return 0
    tiles = ((M + 255) // 256) * ((N + 255) // 256)
    if tiles > 128 or M * N < 0.85 * tiles * 65536:
        return 0
    steps = (K + 63) // 64
    return max(1, min(256 // tiles, steps // 8))


def bf16_train_tn_tiling(M: int, N: int, K: int):
    """(block_m, splits) of a single-pass weight gradient: the 256 x 256 TN kernel by gemm256_tn_b1_splits, else the general family."""
    sp = gemm256_tn_b1_splits(M, N, K)
    if _BF16_TRAIN_FORCE_256:
        return 256, max(1, sp)
    return (256, sp) if sp else _general_tiling(M, N, K, True, True)


def _one_plane(t, numel: int, what: str):
    """A single bf16 plane as (pointer, elements addressable): a 2-byte HIP tensor, or the hi plane (= bf16(x)) of a Planes matrix."""
    if isinstance(t, Planes):
        t = t.buf[:t.rows * t.cols]
    return _plane_ptr(t, numel, what), t.numel()


def gemm_bf16_train(a, b, out: Optional[torch.Tensor], M: int, N: int, K: int, *, trans: bool = False, lda: Optional[int] = None,
                    ldb: Optional[int] = None, ld_out: Optional[int] = None, bias: Optional[torch.Tensor] = None, act: int = 0,
                    out_z: Optional[torch.Tensor] = None, aux_z: Optional[torch.Tensor] = None, resid: Optional[torch.Tensor] = None,
                    drop: Optional[Drop] = None, accumulate: bool = False, alpha: float = 1.0, out_plane: Optional[torch.Tensor] = None,
                    out_planes: Optional[Planes] = None, splitk_ws: Optional[torch.Tensor] = None, splits: Optional[int] = None,
                    block_m: Optional[int] = None, colsum: Optional[torch.Tensor] = None, colsum_ws: Optional[torch.Tensor] = None):
    """One bf16 pass with the training epilogue (lr2_gemm_bf16_train); a, b: single bf16 planes (2-byte HIP tensors; a Planes matrix
    contributes its hi plane).  NOT the parity path.
    trans=False: out[M, N] = a[M, K] @ b[N, K]^T -- alpha, bias, act 0 / 1 (GELU, out_z keeps the pre-activation) / 2 (x GELU'(aux_z)),
      drop, resid, accumulate -> `out` (fp32) and / or ONE plane `out_plane` or hi / lo `out_planes`.  block_m None: use_gemm256_b1.
    trans=True: out[M, N] = a[K, M]^T @ b[K, N] (the weight gradient; K = token rows, any count) -> `out`; colsum [M] receives the column
      sums of a (the bias gradient, of the bf16 plane as the product sees it).  block_m / splits None: bf16_train_tn_tiling."""
    _chk_f32(out, bias, out_z, aux_z, resid, colsum, colsum_ws)
    if lda is None:
        lda = M if trans else K
    if ldb is None:
        ldb = N if trans else K
    if trans:
        a_ptr, a_n = _one_plane(a, (K - 1) * lda + M, "gemm_bf16_train: a")
        b_ptr, b_n = _one_plane(b, (K - 1) * ldb + N, "gemm_bf16_train: b")
        # the extents of K WHOLE rows: rows >= K read as zero.  (Not (K - 1) * ld + M: an extent that ends inside a 16-byte load zeroes
        # the last columns of row K - 1 whenever M or N is no multiple of 8.)
        a_n, b_n = min(a_n, K * lda), min(b_n, K * ldb)
        if block_m is None or splits is None:
            bm, sp = bf16_train_tn_tiling(M, N, K)
            block_m = bm if block_m is None else block_m
            splits = sp if splits is None else splits
    else:
        a_ptr, a_n = _one_plane(a, (M - 1) * lda + K, "gemm_bf16_train: a")
        b_ptr, b_n = _one_plane(b, (N - 1) * ldb + K, "gemm_bf16_train: b")
        if block_m is None:
            block_m = 256 if (_BF16_TRAIN_FORCE_256 or use_gemm256_b1(M, N, K)) else _bf16_fallback_block_m(M, N)
        splits = 1 if splits is None else splits
    if splits > 1 and (splitk_ws is None or splitk_ws.numel() < splits * M * N):
        raise ValueError(f"split-K workspace too small: need {splits * M * N} floats")
    if out_plane is not None and out_planes is not None:
        raise ValueError("gemm_bf16_train: out_plane excludes out_planes")
    e = _nat.Epilogue()
    e.bias, e.resid, e.aux_z, e.out, e.out_z = _ptr(bias), _ptr(resid), _ptr(aux_z), _ptr(out), _ptr(out_z)
    e.ld_resid, e.ld_aux, e.ld_out, e.ld_z = _ld(resid, N), _ld(aux_z, N), (N if ld_out is None else ld_out), _ld(out_z, N)
    if out_plane is not None:
        e.out_hi, e.out_lo_off, e.ld_planes = _plane_ptr(out_plane, M * N, "gemm_bf16_train: out_plane"), 0, N
    elif out_planes is not None:
        if out_planes.rows != M or out_planes.cols != N:
            raise ValueError("gemm_bf16_train: out_planes must be [M, N]")
        e.out_hi, e.out_lo_off, e.ld_planes = out_planes.data_ptr(), out_planes.lo_off, N
    e.act, e.accumulate, e.alpha = act, 1 if accumulate else 0, alpha
    if drop is not None and drop.p > 0.0:
        e.drop_p, e.drop_seed, e.drop_site, e.drop_seed_dev = drop.p, drop.seed, drop.site, drop.seed_dev_ptr()
    if colsum is not None:
        if not trans or colsum.numel() != M or colsum_ws is None or colsum_ws.numel() < max(128, splits * ((N + 255) // 256)) * M:
            raise ValueError("gemm_bf16_train(colsum=...): trans=True only; colsum [M], colsum_ws >= max(128, splits * ceil(N / 256)) * M floats")
        e.colsum, e.colsum_ws = colsum.data_ptr(), colsum_ws.data_ptr()
    t = 1 if trans else 0
    with _Timed(f"gemm_bf16t_{'TN' if trans else 'NT'}_M{M}_N{N}_K{K}", 2.0 * M * N * K, 2.0 * (M * K + N * K) + 4.0 * M * N):
        rc = _nat.lib().lr2_gemm_bf16_train(a_ptr, b_ptr, M, N, K, lda, ldb, t, t, a_n * 2, b_n * 2, C.byref(e), _ptr(splitk_ws),
                                            splits, block_m, _stream())
    if rc:
        _nat.check(rc, f"lr2_gemm_bf16_train(M={M},N={N},K={K},trans={trans},block_m={block_m},splits={splits})")
    return out if out is not None else (out_plane if out_plane is not None else out_planes)


def gemm_bf16_train_launch_counts():
    """(256 x 256 NT kernel, 256 x 256 TN kernel, general family) launches by gemm_bf16_train since the library was loaded."""
    c = (C.c_uint64 * 3)()
    _nat.check(_nat.lib().lr2_gemm_bf16_train_launch_counts(c), "lr2_gemm_bf16_train_launch_counts")
    return int(c[0]), int(c[1]), int(c[2])


# workgroups of the LayerNorm backward (each leaves one partial row of d gamma / d beta): 4 per CU.  With one per CU (round 2) the
# kernel kept 24 KB of loads in flight per CU and ran at 3.4 TB/s on the encoders' [100864, 768] rows (rocprofv3, profiles/r03_*).
LN_BWD_BLOCKS = 512       # workgroups of 4 rows-at-a-time waves: 2 per CU measured best at the encoder shapes (tools/dbg/ln_bwd_time.py)


def layernorm_bwd(dy, x, gamma, mean, rstd, dx, partials, dgamma, dbeta, *, rows, D, group=0, group_stride=0,
                  resid_grad=None, dx_planes: Optional[Planes] = None, drop: Optional[Drop] = None, nblocks=LN_BWD_BLOCKS, mode=0,
                  eps=1e-5):
    """dx (fp32) = LN'(dy) + resid_grad; dx_planes = planes of dropout_mask(dx)/(1-p) (p = 0: of dx).
    mode / eps: the forward's (0 = nn.LayerNorm, 1 = TencentPretrain LayerNorm)."""
    _chk_f32(dy, x, gamma, mean, rstd, dx, partials, dgamma, dbeta, resid_grad)
    nb = min(nblocks, (rows + 3) // 4)
    if partials.numel() < nb * 2 * D:
        raise ValueError("layernorm_bwd partials workspace too small")
    p, seed, site = (drop.p, drop.seed, drop.site) if drop is not None else (0.0, 0, 0)
    L = _nat.lib()
    name = "lr2_layernorm_bwd_wide" if D > 1024 else "lr2_layernorm_bwd"
    rc = getattr(L, name)(dy.data_ptr(), group, group_stride, x.data_ptr(), gamma.data_ptr(), mean.data_ptr(),
                          rstd.data_ptr(), _ptr(resid_grad), _ptr(dx),
                          dx_planes.data_ptr() if dx_planes is not None else None,
                          dx_planes.lo_off if dx_planes is not None else 0, p, seed, site,
                          drop.seed_dev_ptr() if drop is not None else None, partials.data_ptr(), nb, rows, D, mode, eps, _stream())
    _nat.check(rc, name)
    if dbeta.data_ptr() == dgamma.data_ptr() + 4 * D:       # [d gamma | d beta] adjacent (flat gradient buffers): one finishing launch
        _nat.check(L.lr2_colsum_partials_finish(partials.data_ptr(), nb, 2 * D, 2 * D, dgamma.data_ptr(), 0, _stream()), "finish")
        return
    _nat.check(L.lr2_colsum_partials_finish(partials.data_ptr(), nb, D, 2 * D, dgamma.data_ptr(), 0, _stream()), "finish")
    _nat.check(L.lr2_colsum_partials_finish(partials.data_ptr() + 4 * D, nb, D, 2 * D, dbeta.data_ptr(), 0, _stream()),
               "finish")


def colsum(x, out, partials, *, rows, cols, ld=None, nblocks=128):
    """Column sums of an fp32 matrix or a Planes matrix -> fp32 [cols]."""
    is_pl = isinstance(x, Planes)
    _chk_f32(None if is_pl else x, out, partials)
    nb = min(nblocks, rows)
    if partials.numel() < nb * cols:
        raise ValueError("colsum partials workspace too small")
    rc = _nat.lib().lr2_colsum(x.data_ptr(), 1 if is_pl else 0, x.lo_off if is_pl else 0, rows, cols, ld or cols,
                               partials.data_ptr(), nb, out.data_ptr(), _stream())
    _nat.check(rc, "lr2_colsum")
    return out


XATTN_NARROW_LK = 16     # keys of the 16-key XiT attention pair (csrc/attn.hip)
XATTN_MAX_LK = 64        # ... of the wide pair (csrc/attn_wide.hip: K / V of one (sequence, head) resident in LDS) = the largest max_imgs


def check_max_imgs(max_imgs):
    """The heads' limit in words, at construction: the XiT cross-attention serves 1 .. XATTN_MAX_LK image tokens."""
    if not 1 <= int(max_imgs) <= XATTN_MAX_LK:
        raise ValueError(f"max_imgs = {max_imgs}: the XiT cross-attention kernels serve 1 to {XATTN_MAX_LK} image tokens "
                         f"(K / V of one sequence and head stay resident in LDS)")


def _xattn_wide(Lk, wide):
    """Which form runs: the 16-key pair up to 16 keys (its results keep their bits), the wide pair for 17 .. 64 or when forced."""
    if Lk > XATTN_MAX_LK:
        raise ValueError(f"XiT attention: Lk = {Lk} keys, the kernels serve at most {XATTN_MAX_LK} (for the heads: --max_imgs <= {XATTN_MAX_LK})")
    return bool(wide) or Lk > XATTN_NARROW_LK


def xattn_fwd(q, k, v, o, *, batch, heads, Lq, Lk, head_dim, post_scale, wide=False):
    """o: fp32 tensor or Planes.  wide=True forces the wide kernel at any Lk <= 64 (tests compare the two forms at Lk <= 16)."""
    name = "lr2_xattn_fwd_wide" if _xattn_wide(Lk, wide) else "lr2_xattn_fwd"      # raises at Lk > 64, before anything else
    o_pl = isinstance(o, Planes)
    _chk_f32(q, k, v, None if o_pl else o)
    _nat.check(getattr(_nat.lib(), name)(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), 1 if o_pl else 0,
                                         o.lo_off if o_pl else 0, batch, heads, Lq, Lk, head_dim, post_scale, _stream()), name)
    return o


def xattn_bwd(q, k, v, do, dq, dk, dv, *, batch, heads, Lq, Lk, head_dim, post_scale, wide=False):
    """dq / dk / dv: all fp32 tensors or all Planes.  wide: as xattn_fwd."""
    name = "lr2_xattn_bwd_wide" if _xattn_wide(Lk, wide) else "lr2_xattn_bwd"
    pl = isinstance(dq, Planes)
    _chk_f32(q, k, v, do)
    if not pl:
        _chk_f32(dq, dk, dv)
    _nat.check(getattr(_nat.lib(), name)(q.data_ptr(), k.data_ptr(), v.data_ptr(), do.data_ptr(), dq.data_ptr(), dk.data_ptr(),
                                         dv.data_ptr(), 1 if pl else 0, dq.lo_off if pl else 0, dk.lo_off if pl else 0, batch,
                                         heads, Lq, Lk, head_dim, post_scale, _stream()), name)


def xattn_wide_launch_counts():
    """(forward, backward) calls the wide XiT attention pair has accepted (a test hook: which form a dispatch ran)."""
    c = (C.c_uint64 * 2)()
    _nat.check(_nat.lib().lr2_xattn_wide_launch_counts(c), "lr2_xattn_wide_launch_counts")
    return int(c[0]), int(c[1])


def _qkv_ptrs(qkv, E):
    base = qkv.data_ptr()
    return base, base + 2 * E, base + 4 * E


def _self_attn_hd(head_dim: int) -> bool:
    """Whether the head-width-general kernels (selfattn_hd.hip) serve this width: multiples of 16 from 32 to 128 except 64, which stays
    with the 64-column kernels (the same call, the same bits as before); every other width goes to those too and is refused there."""
    return head_dim != 64 and 32 <= head_dim <= 128 and head_dim % 16 == 0


def self_attn_hd_launch_counts():
    """(forward, backward) calls the head-width-general attention pair has accepted (a test hook: which form a dispatch ran)."""
    c = (C.c_uint64 * 2)()
    _nat.check(_nat.lib().lr2_self_attn_hd_launch_counts(c), "lr2_self_attn_hd_launch_counts")
    return int(c[0]), int(c[1])


def self_attn_fwd(qkv: "Planes", seg, o, *, batch, heads, L, head_dim, scale, lse=None, drop: Optional[Drop] = None):
    """Encoder self-attention on the matrix cores.  qkv: Planes [batch*L, 3*heads*head_dim] = [Q | K | V] (what one fused
    QKV GEMM writes); seg: int64 [batch*L]; o: fp32 tensor or Planes [batch*L, heads*head_dim]; lse: optional fp32
    [batch*heads*L]; drop: dropout on the probabilities.  head_dim 64: lr2_self_attn_fwd; 32 .. 128 in steps of 16 otherwise:
    lr2_self_attn_hd_fwd."""
    E = heads * head_dim
    if not isinstance(qkv, Planes) or qkv.cols != 3 * E or qkv.rows != batch * L:
        raise TypeError("self_attn_fwd: qkv must be a Planes matrix [batch*L, 3*heads*head_dim]")
    if seg.dtype != torch.int64:
        raise TypeError("seg must be int64")
    o_pl = isinstance(o, Planes)
    _chk_f32(None if o_pl else o, lse)
    q, k, v = _qkv_ptrs(qkv, E)
    p, seed, site = (drop.p, drop.seed, drop.site) if drop is not None else (0.0, 0, 0)
    name = "lr2_self_attn_hd_fwd" if _self_attn_hd(head_dim) else "lr2_self_attn_fwd"
    with _Timed(f"selfattn_B{batch}_H{heads}_L{L}", 4.0 * batch * heads * L * L * head_dim, 16.0 * batch * L * E):
        _nat.check(getattr(_nat.lib(), name)(q, k, v, qkv.lo_off, qkv.cols, seg.data_ptr(),
                                             None if o_pl else o.data_ptr(), o.data_ptr() if o_pl else None,
                                             o.lo_off if o_pl else 0, E, _ptr(lse), p, seed, site, batch, heads, L, head_dim,
                                             scale, _stream()), name)
    return o


def first_token_attn(q: torch.Tensor, kv: "Planes", seg, o: torch.Tensor, *, batch, heads, L, head_dim, scale):
    """Attention of query row 0 of every sequence against all keys (lr2_first_token_attn).  q: fp32 [batch, E] (projected);
    kv: Planes [batch*L, 2E] = [K | V]; seg: int64 [batch*L]; o: fp32 [batch, E]."""
    E = heads * head_dim
    if not isinstance(kv, Planes) or kv.cols != 2 * E or kv.rows != batch * L:
        raise TypeError("first_token_attn: kv must be a Planes matrix [batch*L, 2*heads*head_dim]")
    if seg.dtype != torch.int64:
        raise TypeError("seg must be int64")
    _chk_f32(q, o)
    if q.shape != (batch, E) or o.shape != (batch, E) or not q.is_contiguous() or not o.is_contiguous():
        raise ValueError("first_token_attn: q / o must be contiguous [batch, heads*head_dim]")
    _nat.check(_nat.lib().lr2_first_token_attn(q.data_ptr(), E, kv.data_ptr(), kv.data_ptr() + 2 * E, kv.lo_off, 2 * E,
                                               seg.data_ptr(), o.data_ptr(), E, batch, heads, L, head_dim, scale, _stream()),
               "lr2_first_token_attn")
    return o


def self_attn_bwd(qkv: "Planes", do: "Planes", seg, dqkv: "Planes", lse_ws, dsum_ws, *, batch, heads, L, head_dim, scale,
                  drop: Optional[Drop] = None, o: Optional["Planes"] = None):
    """dQKV (Planes [batch*L, 3E]) from QKV and dO (Planes [batch*L, E]); lse_ws / dsum_ws: fp32 [batch*heads*L].  Without `o` both are
    scratch (everything is recomputed).  With `o` = the forward's output planes [batch*L, E], lse_ws must hold the log-sum-exp
    self_attn_fwd(..., lse=lse_ws) wrote for the same inputs: the streaming / persistent kernels (lr2_self_attn_bwd, ABI 19)."""
    E = heads * head_dim
    for name, t, cols in (("qkv", qkv, 3 * E), ("do", do, E), ("dqkv", dqkv, 3 * E)) + ((("o", o, E),) if o is not None else ()):
        if not isinstance(t, Planes) or t.cols != cols or t.rows != batch * L:
            raise TypeError(f"self_attn_bwd: {name} must be a Planes matrix [batch*L, {cols}]")
    if seg.dtype != torch.int64:
        raise TypeError("seg must be int64")
    _chk_f32(lse_ws, dsum_ws)
    if lse_ws.numel() < batch * heads * L or dsum_ws.numel() < batch * heads * L:
        raise ValueError("self_attn_bwd: statistics workspaces too small")
    q, k, v = _qkv_ptrs(qkv, E)
    dq, dk, dv = _qkv_ptrs(dqkv, E)
    p, seed, site = (drop.p, drop.seed, drop.site) if drop is not None else (0.0, 0, 0)
    name = "lr2_self_attn_hd_bwd" if _self_attn_hd(head_dim) else "lr2_self_attn_bwd"
    with _Timed(f"selfattnbwd_B{batch}_H{heads}_L{L}", 14.0 * batch * heads * L * L * head_dim, 32.0 * batch * L * E):
        _nat.check(getattr(_nat.lib(), name)(q, k, v, qkv.lo_off, qkv.cols, do.data_ptr(), do.lo_off, do.cols, seg.data_ptr(),
                                             dq, dk, dv, dqkv.lo_off, dqkv.cols, o.data_ptr() if o is not None else None,
                                             o.lo_off if o is not None else 0, o.cols if o is not None else 0,
                                             lse_ws.data_ptr(), dsum_ws.data_ptr(), p, seed, site, batch, heads, L, head_dim, scale,
                                             _stream()), name)
    return dqkv


def self_attn_plan(batch: int, heads: int, L: int, ld: Optional[int] = None, ld_do: Optional[int] = None):
    """(forward persistent?, backward persistent?) for a call of this shape (lr2_self_attn_plan): which form of the kernels runs."""
    import ctypes
    E = heads * 64
    f, b = ctypes.c_int(), ctypes.c_int()
    _nat.check(_nat.lib().lr2_self_attn_plan(batch, heads, L, 3 * E if ld is None else ld, E if ld_do is None else ld_do,
                                             ctypes.byref(f), ctypes.byref(b)), "lr2_self_attn_plan")
    return bool(f.value), bool(b.value)


def gather_rows(src, index, dst, *, B, t_in, t_out, row_elems, src_bstride=None, src_tstride=None):
    """dst[b, j] = src[b, clamp(index[b, j])]; index None: j.  An index outside [0, t_in) is clamped into it (lr2_gather_rows)."""
    _chk_f32(src, dst)
    if index is not None and index.dtype != torch.int64:
        raise TypeError("index must be int64")
    _nat.check(_nat.lib().lr2_gather_rows(src.data_ptr(), _ptr(index), dst.data_ptr(), B, t_in, t_out, row_elems,
                                    src_bstride if src_bstride is not None else t_in * row_elems,
                                    src_tstride if src_tstride is not None else row_elems, _stream()), "lr2_gather_rows")
    return dst


def gather_rows_bwd(ddst, index, dsrc, *, B, t_in, t_out, row_elems):
    """dsrc[b, t] = sum of ddst[b, j] over the j whose clamped index is t (the forward's clamp): every row of dsrc is overwritten."""
    _chk_f32(ddst, dsrc)
    _nat.check(_nat.lib().lr2_gather_rows_bwd(ddst.data_ptr(), _ptr(index), dsrc.data_ptr(), B, t_in, t_out, row_elems,
                                        _stream()), "lr2_gather_rows_bwd")
    return dsrc


def copy_rows(src, dst, *, rows, D, group, dst_gstride, dst_off):
    """dst: fp32 tensor or Planes (the concat buffer of finetune/ppo.py:224)."""
    pl = isinstance(dst, Planes)
    _chk_f32(src, None if pl else dst)
    _nat.check(_nat.lib().lr2_copy_rows(src.data_ptr(), dst.data_ptr(), 1 if pl else 0, dst.lo_off if pl else 0, rows, D,
                                        group, dst_gstride, dst_off, _stream()), "lr2_copy_rows")
    return dst


def head_fwd(x, w, b, y, *, rows, D, row_step=1, row_off=0):
    _chk_f32(x, w, b, y)
    _nat.check(_nat.lib().lr2_head_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), rows, D, row_step, row_off,
                                 _stream()), "lr2_head_fwd")
    return y


def head_bwd(x, w, dy, dx, dw, db, *, rows, D, row_step=1, row_off=0, total_rows=None):
    _chk_f32(x, w, dy, dx, dw, db)
    _nat.check(_nat.lib().lr2_head_bwd(x.data_ptr(), w.data_ptr(), dy.data_ptr(), _ptr(dx), _ptr(dw), _ptr(db), rows, D,
                                 row_step, row_off, total_rows if total_rows is not None else rows * row_step, _stream()),
            "lr2_head_bwd")


def add_period_rows(x, table, out, *, rows, D, period):
    _chk_f32(x, table, out)
    _nat.check(_nat.lib().lr2_add_period_rows(x.data_ptr(), table.data_ptr(), out.data_ptr(), rows, D, period, _stream()),
            "lr2_add_period_rows")
    return out


def period_rows_grad(dy, dtable, *, rows, D, period):
    _chk_f32(dy, dtable)
    _nat.check(_nat.lib().lr2_period_rows_grad(dy.data_ptr(), dtable.data_ptr(), rows, D, period, _stream()),
            "lr2_period_rows_grad")
    return dtable


def ppo_loss(scores, old_scores, rewards, old_value, value, next_state, scalars, per_item, dscores, dvalue, *, B, T,
             kl_w, ent_w, value_clip, margin=0.01, adv_eps=-0.1, rank_len=2, stats_out=None, global_stats=None, world=1):
    """stats_out (fp32[3]): write only this rank's {hinge sum, positive count, sum |A|} (pass 1 of the data-parallel form);
    global_stats (fp32[3], all-reduced) + world: use the global RankLoss statistics (pass 2); see lr2_ppo_loss."""
    _chk_f32(scores, old_scores, rewards, old_value, value, scalars, per_item, dscores, dvalue, stats_out, global_stats)
    if next_state.dtype != torch.int64 or not next_state.is_contiguous():
        raise TypeError("next_state must be contiguous int64")
    _nat.check(_nat.lib().lr2_ppo_loss(scores.data_ptr(), old_scores.data_ptr(), rewards.data_ptr(), old_value.data_ptr(),
                                 value.data_ptr(), next_state.data_ptr(), next_state.shape[1], rank_len, B, T, kl_w, ent_w,
                                 value_clip, margin, adv_eps, _ptr(scalars), _ptr(per_item), _ptr(dscores), _ptr(dvalue),
                                 _ptr(stats_out), _ptr(global_stats), world, _stream()), "lr2_ppo_loss")


def cls_head_fwd(x, w, b, y, *, rows, D, C):
    _chk_f32(x, w, b, y)
    _nat.check(_nat.lib().lr2_cls_head_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), rows, D, C, _stream()),
               "lr2_cls_head_fwd")
    return y


def cls_head_bwd(x, w, dy, dx, dw, db, *, rows, D, C):
    _chk_f32(x, w, dy, dx, dw, db)
    _nat.check(_nat.lib().lr2_cls_head_bwd(x.data_ptr(), w.data_ptr(), dy.data_ptr(), _ptr(dx), _ptr(dw), _ptr(db), rows, D, C,
                                           _stream()), "lr2_cls_head_bwd")


def cls_scores(logits, probs, scores, *, rows, C, softmax=True):
    """scores[r] = sum_k k * (softmax(logits[r]) if softmax else logits[r])_k; probs (optional) receives the distribution."""
    _chk_f32(logits, probs, scores)
    _nat.check(_nat.lib().lr2_cls_scores(logits.data_ptr(), _ptr(probs), scores.data_ptr(), rows, C, 1 if softmax else 0,
                                         _stream()), "lr2_cls_scores")
    return scores


def cls_scores_bwd(probs, scores, dscores, dlogits, *, rows, C):
    _chk_f32(probs, scores, dscores, dlogits)
    _nat.check(_nat.lib().lr2_cls_scores_bwd(probs.data_ptr(), scores.data_ptr(), dscores.data_ptr(), dlogits.data_ptr(), rows,
                                             C, _stream()), "lr2_cls_scores_bwd")
    return dlogits


def nll_loss(logits, tgts, loss, dlogits=None, *, rows, C):
    _chk_f32(logits, loss, dlogits)
    if tgts.dtype != torch.int64:
        raise TypeError("tgts must be int64")
    _nat.check(_nat.lib().lr2_nll_loss(logits.data_ptr(), tgts.data_ptr(), rows, C, loss.data_ptr(), _ptr(dlogits), _stream()),
               "lr2_nll_loss")
    return loss


def smooth_l1(pred, target, loss, dpred=None, *, n, beta=0.3):
    _chk_f32(pred, target, loss, dpred)
    _nat.check(_nat.lib().lr2_smooth_l1(pred.data_ptr(), target.data_ptr(), n, beta, loss.data_ptr(), _ptr(dpred), _stream()),
            "lr2_smooth_l1")
    return loss


def pair_hinge(scores, loss_acc, dscores=None, *, bs, margin=1.0):
    """scores: [2*bs] = chosen then reject; loss_acc: [2] (loss, accuracy); dscores: [2*bs] or None."""
    _chk_f32(scores, loss_acc, dscores)
    if scores.numel() != 2 * bs or loss_acc.numel() < 2 or (dscores is not None and dscores.numel() != 2 * bs):
        raise ValueError("pair_hinge: scores/dscores must hold 2*bs elements, loss_acc 2")
    _nat.check(_nat.lib().lr2_pair_hinge(scores.data_ptr(), bs, margin, loss_acc.data_ptr(), _ptr(dscores), _stream()),
               "lr2_pair_hinge")
    return loss_acc


def adamw_multi(table_dev: torch.Tensor, n_chunks: int, lr: float, beta1: float, beta2: float, eps: float,
                n_params: int = 0, lr_dev: Optional[torch.Tensor] = None):
    with _Timed(f"adamw_{n_params}", 0.0, 28.0 * n_params):
        _nat.check(_nat.lib().lr2_adamw_multi(table_dev.data_ptr(), n_chunks, lr, beta1, beta2, eps,
                                              lr_dev.data_ptr() if lr_dev is not None else None, _stream()), "lr2_adamw_multi")


def _chk_f64(t: torch.Tensor, what: str):
    if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous():
        raise TypeError(f"{what}: expected a contiguous float64 HIP tensor, got {t.dtype} on {t.device}")


def clip_sumsq(table_dev: torch.Tensor, n_chunks: int, partials: torch.Tensor, n_params: int = 0):
    """partials[i] (float64) = sum of g^2 over chunk i of an AdamW chunk table (lr2_clip_sumsq: fixed order, no atomics)."""
    _chk_f64(partials, "clip_sumsq")
    if partials.numel() < n_chunks:
        raise ValueError("clip_sumsq: one float64 partial per chunk")
    with _Timed(f"clip_sumsq_{n_params}", 0.0, 4.0 * n_params):
        _nat.check(_nat.lib().lr2_clip_sumsq(table_dev.data_ptr(), n_chunks, partials.data_ptr(), _stream()), "lr2_clip_sumsq")
    return partials


def clip_gram_dot(a: torch.Tensor, b: torch.Tensor, slot: torch.Tensor, *, n: int, factor: float = 1.0, ld_a: Optional[int] = None,
                  ld_b: Optional[int] = None):
    """slot[0] (float64) = factor * sum_ij a[i, j] * b[i, j] over the leading [n, n] of two fp32 matrices (lr2_clip_gram_dot)."""
    _chk_f32(a, b)
    _chk_f64(slot, "clip_gram_dot")
    ld_a, ld_b = ld_a or a.shape[-1], ld_b or b.shape[-1]
    if a.numel() < (n - 1) * ld_a + n or b.numel() < (n - 1) * ld_b + n or slot.numel() < 1:
        raise ValueError("clip_gram_dot: a / b must hold n rows of n floats, ld apart; slot one float64")
    _nat.check(_nat.lib().lr2_clip_gram_dot(a.data_ptr(), b.data_ptr(), n, ld_a, ld_b, factor, slot.data_ptr(), _stream()),
               "lr2_clip_gram_dot")
    return slot


def clip_coef(slots: torch.Tensor, n: int, max_norm: float, out: torch.Tensor):
    """out[0] = total_norm = sqrt(slots[0] + ... + slots[n - 1]), out[1] = min(1, max_norm / (total_norm + 1e-6)) (float32, formed in
    float64): the rule of torch.nn.utils.clip_grad_norm_ (lr2_clip_coef)."""
    _chk_f64(slots, "clip_coef")
    _chk_f32(out)
    if slots.numel() < n or out.numel() < 2 or not out.is_contiguous():
        raise ValueError("clip_coef: slots must hold n float64 values, out two float32")
    _nat.check(_nat.lib().lr2_clip_coef(slots.data_ptr(), n, max_norm, out.data_ptr(), _stream()), "lr2_clip_coef")
    return out


def adamw_multi_scaled(table_dev: torch.Tensor, n_chunks: int, lr: float, beta1: float, beta2: float, eps: float,
                       gscale_dev: torch.Tensor, n_params: int = 0, lr_dev: Optional[torch.Tensor] = None):
    """adamw_multi on g * gscale_dev[0] (float32 device scalar); the gradients in memory stay as they are."""
    _chk_f32(gscale_dev)
    with _Timed(f"adamw_{n_params}", 0.0, 28.0 * n_params):
        _nat.check(_nat.lib().lr2_adamw_multi_scaled(table_dev.data_ptr(), n_chunks, lr, beta1, beta2, eps,
                                                     lr_dev.data_ptr() if lr_dev is not None else None, gscale_dev.data_ptr(),
                                                     _stream()), "lr2_adamw_multi_scaled")


def adafactor_multi(tensors_dev: torch.Tensor, tiles_dev: torch.Tensor, n_tiles: int, fin_dev: Optional[torch.Tensor], n_fin: int,
                    ws_dev: torch.Tensor, lr: float, beta2t: float, eps0: float, clip_threshold: float, n_params: int = 0,
                    n_bytes: float = 0.0, lr_dev: Optional[torch.Tensor] = None):
    """One Adafactor step over the tensors of the device tables (lr2_adafactor_multi: _native.ADAFACTOR_LAUNCHES launches whatever
    their number).  n_bytes: the HBM traffic the caller counted (20 B per element of a 2-D tensor, 28 B of a 1-D one)."""
    with _Timed(f"adafactor_{n_params}", 0.0, n_bytes):
        _nat.check(_nat.lib().lr2_adafactor_multi(tensors_dev.data_ptr(), tiles_dev.data_ptr(), n_tiles, _ptr(fin_dev), n_fin,
                                                  ws_dev.data_ptr(), lr, beta2t, eps0, clip_threshold,
                                                  lr_dev.data_ptr() if lr_dev is not None else None, _stream()), "lr2_adafactor_multi")


def adafactor_launch_counts():
    """(accepted lr2_adafactor_multi calls, kernel launches they issued) since the library was loaded (a test hook)."""
    c = (C.c_uint64 * 2)()
    _nat.check(_nat.lib().lr2_adafactor_launch_counts(c), "lr2_adafactor_launch_counts")
    return int(c[0]), int(c[1])


class Mx8:
    """A matrix in MX-FP8 (OCP MX v1.0: e4m3fn bytes + one E8M0 scale byte per 32 consecutive elements of a row) -- the operand
    format of gemm_mxfp8, the inference-only fp8 fast mode (csrc/fp8.hip; NOT the parity path)."""
    __slots__ = ("q", "s", "rows", "cols")

    def __init__(self, q: torch.Tensor, s: torch.Tensor, rows: int, cols: int):
        if q.dtype != torch.uint8 or s.dtype != torch.uint8 or not q.is_cuda or q.numel() < rows * cols or s.numel() < rows * (cols // 32):
            raise TypeError("Mx8: uint8 HIP tensors [rows, cols] and [rows, cols / 32]")
        self.q, self.s, self.rows, self.cols = q, s, rows, cols

    @staticmethod
    def empty(rows: int, cols: int, device) -> "Mx8":
        return Mx8(torch.empty(rows * cols, dtype=torch.uint8, device=device), torch.empty(rows * (cols // 32), dtype=torch.uint8, device=device),
                   rows, cols)

    def to_float(self) -> torch.Tensor:
        """Dequantised fp32 matrix (tests / debugging)."""
        v = self.q[:self.rows * self.cols].view(torch.float8_e4m3fn).float().view(self.rows, self.cols // 32, 32)
        sc = torch.exp2(self.s[:self.rows * (self.cols // 32)].float() - 127.0).view(self.rows, self.cols // 32, 1)
        return (v * sc).view(self.rows, self.cols)


def quant_mxfp8(x: torch.Tensor, dst: Optional[Mx8] = None) -> Mx8:
    """x fp32 [rows, K] (rows may be strided, K % 32 == 0) -> Mx8 (lr2_quant_mxfp8)."""
    _chk_f32(x)
    if x.dim() != 2 or x.stride(1) != 1 or x.shape[1] % 32:
        raise ValueError("quant_mxfp8: a 2-D fp32 matrix with contiguous rows and K % 32 == 0")
    R, K = x.shape
    dst = dst or Mx8.empty(R, K, x.device)
    if dst.rows != R or dst.cols != K:
        raise ValueError("quant_mxfp8: destination shape")
    _nat.check(_nat.lib().lr2_quant_mxfp8(x.data_ptr(), x.stride(0), dst.q.data_ptr(), dst.s.data_ptr(), R, K, _stream()), "lr2_quant_mxfp8")
    return dst


def layernorm_fwd_mxfp8(x, gamma, beta, dst: Mx8, out: Optional[torch.Tensor] = None, *, rows, D, eps=1e-5, mode=0) -> Mx8:
    """LN(x) as MX-FP8 (and as fp32 when `out` is given) -- lr2_layernorm_fwd_mxfp8."""
    _chk_f32(x, gamma, beta, out)
    if dst.rows != rows or dst.cols != D:
        raise ValueError("layernorm_fwd_mxfp8: destination shape")
    with _Timed(f"lnfwd_mx_R{rows}_D{D}", 0.0, 5.0 * rows * D):
        _nat.check(_nat.lib().lr2_layernorm_fwd_mxfp8(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(out), dst.q.data_ptr(),
                                                      dst.s.data_ptr(), rows, D, eps, mode, _stream()), "lr2_layernorm_fwd_mxfp8")
    return dst


def gemm_mxfp8(a: Mx8, b: Mx8, out: Optional[torch.Tensor], *, bias=None, resid=None, act: int = 0, out_mx: Optional[Mx8] = None,
               out_planes: Optional[Planes] = None, out_bf16: Optional[torch.Tensor] = None):
    """out[M, N] fp32 = a . b^T (+ bias) (act 1: GELU) (+ resid) with a [M, K], b [N, K] in MX-FP8 (lr2_gemm_mxfp8).
    out_mx: the result also (out given) or only (out None) as MX-FP8 -- the next product's A operand.
    out_bf16: the result as ONE bf16 plane (an int16 / bfloat16 tensor of M * N elements): the operands of self_attn_fwd_bf16."""
    _chk_f32(out, bias, resid)
    M, N, K = a.rows, b.rows, a.cols
    if out_bf16 is not None:
        if out_planes is not None or out_bf16.element_size() != 2 or not out_bf16.is_cuda or out_bf16.numel() < M * N:
            raise ValueError("gemm_mxfp8: out_bf16 is a 2-byte HIP tensor of M * N elements, and excludes out_planes")
        out_planes = Planes.__new__(Planes)       # a single plane: lo_off = 0 (see include/lr2ppo_hip.h)
        out_planes.buf, out_planes.rows, out_planes.cols, out_planes.lo_off, out_planes.transposed = out_bf16, M, N, 0, False
    if b.cols != K or (out is None and out_mx is None and out_planes is None):
        raise ValueError("gemm_mxfp8: a [M, K], b [N, K], out [M, N] and / or out_mx / out_planes / out_bf16")
    if out_planes is not None and (out_planes.rows != M or out_planes.cols != N):
        raise ValueError("gemm_mxfp8: out_planes must be [M, N]")
    if out is not None and (out.dim() != 2 or out.shape[0] != M or out.shape[1] != N or out.stride(1) != 1):
        raise ValueError("gemm_mxfp8: out must be [M, N] with contiguous rows")
    if out_mx is not None and (out_mx.rows != M or out_mx.cols != N):
        raise ValueError("gemm_mxfp8: out_mx must be [M, N]")
    with _Timed(f"gemm_mxfp8_M{M}_N{N}_K{K}", 2.0 * M * N * K, float(M * K + N * K + 4 * M * N)):
        _nat.check(_nat.lib().lr2_gemm_mxfp8(a.q.data_ptr(), a.s.data_ptr(), b.q.data_ptr(), b.s.data_ptr(), _ptr(out),
                                             out.stride(0) if out is not None else N, _ptr(bias), _ptr(resid),
                                             resid.stride(0) if resid is not None else 0, act,
                                             out_mx.q.data_ptr() if out_mx is not None else None,
                                             out_mx.s.data_ptr() if out_mx is not None else None,
                                             out_planes.data_ptr() if out_planes is not None else None,
                                             out_planes.lo_off if out_planes is not None else 0,
                                             out_planes.cols if out_planes is not None else 0, M, N, K, _stream()), "lr2_gemm_mxfp8")
    return out if out is not None else (out_mx if out_mx is not None else out_planes)


def quant_mxfp8_t(x, *, rows_out: Optional[Mx8] = None, row_blocked: bool = False, colsum: Optional[torch.Tensor] = None,
                  accumulate: bool = False, act: int = 0, z: Optional[torch.Tensor] = None, dst: Optional[Mx8] = None,
                  partials: Optional[torch.Tensor] = None, transposed: bool = True):
    """x [rows, cols] -- fp32 (rows may be strided) or Planes -- through the prologue `act` (0: x; 1: GELU(x); 2: x * GELU'(z)) ->
    (Mx8 of x^T [cols, rows_pad] (MX blocks down the columns of x; rows_pad = rows rounded up to 128, padding zeros),
     the row-blocked Mx8 [rows, cols] (rows_out, or a new one with row_blocked=True; byte-identical to quant_mxfp8), else None,
     colsum: fp32 [cols] column sums written (accumulate: added), else None) -- lr2_quant_mxfp8_t.  partials: workspace of
    rows_pad / 128 * cols floats for the column sums (allocated when not given).  transposed=False: no x^T (first item None; a
    forward that keeps nothing for a backward), rows_out / row_blocked then required."""
    pl = isinstance(x, Planes)
    if pl:
        R, K, ld = x.rows, x.cols, x.cols
    else:
        _chk_f32(x)
        if x.dim() != 2 or x.stride(1) != 1:
            raise ValueError("quant_mxfp8_t: a 2-D fp32 matrix with contiguous rows, or Planes")
        R, K = x.shape
        ld = x.stride(0)
    if K % 64:
        raise ValueError("quant_mxfp8_t: cols % 64 == 0")
    if act == 2:
        _chk_f32(z)
        if z is None or z.dim() != 2 or tuple(z.shape) != (R, K) or z.stride(1) != 1:
            raise ValueError("quant_mxfp8_t: act 2 needs z [rows, cols] with contiguous rows")
    Rp = -(-R // 128) * 128
    dev = x.buf.device if pl else x.device
    if transposed:
        dst = dst or Mx8.empty(K, Rp, dev)
        if dst.rows != K or dst.cols != Rp:
            raise ValueError("quant_mxfp8_t: destination must be [cols, rows_pad]")
    elif dst is not None or (rows_out is None and not row_blocked):
        raise ValueError("quant_mxfp8_t(transposed=False): no dst, and a row-blocked output")
    if rows_out is None and row_blocked:
        rows_out = Mx8.empty(R, K, dev)
    if rows_out is not None and (rows_out.rows != R or rows_out.cols != K):
        raise ValueError("quant_mxfp8_t: rows_out must be [rows, cols]")
    if colsum is not None:
        _chk_f32(colsum, partials)
        if colsum.numel() != K:
            raise ValueError("quant_mxfp8_t: colsum [cols]")
        if partials is None:
            partials = torch.empty((Rp // 128) * K, device=dev)
        elif partials.numel() < (Rp // 128) * K:
            raise ValueError("quant_mxfp8_t: partials workspace too small")
    out_bytes = (1.04 if transposed else 0.0) + (1.03 if rows_out is not None else 0.0)
    with _Timed(f"quant_mxfp8_t_R{R}_C{K}", 0.0, float((8 if act == 2 else 4) * R * K + out_bytes * Rp * K)):
        _nat.check(_nat.lib().lr2_quant_mxfp8_t(x.data_ptr(), 1 if pl else 0, x.lo_off if pl else 0, ld, _ptr(z),
                                                z.stride(0) if z is not None else 0, act, _ptr(dst.q) if transposed else None,
                                                _ptr(dst.s) if transposed else None,
                                                rows_out.q.data_ptr() if rows_out is not None else None,
                                                rows_out.s.data_ptr() if rows_out is not None else None, _ptr(colsum),
                                                _ptr(partials) if colsum is not None else None, 1 if accumulate else 0, R, K,
                                                _stream()), "lr2_quant_mxfp8_t")
    return dst, rows_out, colsum


@functools.lru_cache(maxsize=4096)
def mxfp8_wgrad_splits(M: int, N: int, K: int) -> int:
    """K slices of the weight-gradient product C[M, N] over K (padded) tokens: enough that tiles x slices fill the 256 CUs' 512
    workgroup slots (two 64-KiB-LDS workgroups per CU) once, and every slice keeps >= 4 K steps of 128."""
    tiles = (M // 128) * (N // 128)
    return max(1, min(-(-512 // tiles), K // 512))


def gemm_mxfp8_wgrad(a_t: Mx8, b_t: Mx8, out: torch.Tensor, *, splits: Optional[int] = None, accumulate: bool = False,
                     workspace: Optional[torch.Tensor] = None):
    """out[M, N] (+)= a_t . b_t^T with a_t [M, K], b_t [N, K] blocked along K (quant_mxfp8_t of dY and X: a weight gradient dY^T X),
    out with contiguous rows (any row stride: a view of a flat gradient buffer).  K-sliced (lr2_gemm_mxfp8_wgrad): workspace holds
    splits * M * N floats; the slices are summed in a fixed order, so the bits do not depend on timing."""
    _chk_f32(out, workspace)
    M, N, K = a_t.rows, b_t.rows, a_t.cols
    if b_t.cols != K or out.dim() != 2 or tuple(out.shape) != (M, N) or out.stride(1) != 1:
        raise ValueError("gemm_mxfp8_wgrad: a_t [M, K], b_t [N, K], out [M, N] with contiguous rows")
    sp = splits or mxfp8_wgrad_splits(M, N, K)
    sp = max(1, min(sp, K // 128))
    if sp > 1 and (workspace is None or workspace.numel() < sp * M * N):
        raise ValueError(f"gemm_mxfp8_wgrad: workspace too small: need {sp * M * N} floats")
    with _Timed(f"gemm_mxfp8_wgrad_M{M}_N{N}_K{K}", 2.0 * M * N * K, float(M * K + N * K + (8 * sp + 4) * M * N)):
        _nat.check(_nat.lib().lr2_gemm_mxfp8_wgrad(a_t.q.data_ptr(), a_t.s.data_ptr(), b_t.q.data_ptr(), b_t.s.data_ptr(), out.data_ptr(),
                                                   out.stride(0), 1 if accumulate else 0, _ptr(workspace) if sp > 1 else None, sp,
                                                   M, N, K, _stream()), "lr2_gemm_mxfp8_wgrad")
    return out


def dropout_residual(y: torch.Tensor, resid: torch.Tensor, out: torch.Tensor, drop: Drop):
    """out = resid + dropout_mask(y) / (1 - p) over contiguous fp32 tensors of one shape (lr2_dropout_residual)."""
    _chk_f32(y, resid, out)
    if not (y.is_contiguous() and resid.is_contiguous() and out.is_contiguous()) or y.numel() != resid.numel() or y.numel() != out.numel():
        raise ValueError("dropout_residual: contiguous tensors of one size")
    with _Timed(f"dropout_residual_{y.numel()}", 0.0, 12.0 * y.numel()):
        _nat.check(_nat.lib().lr2_dropout_residual(y.data_ptr(), resid.data_ptr(), out.data_ptr(), y.numel(), drop.p, drop.seed, drop.site,
                                                   _stream()), "lr2_dropout_residual")
    return out


def self_attn_fwd_bf16(qkv: torch.Tensor, seg, *, batch, heads, L, head_dim, scale, out: Optional[torch.Tensor] = None,
                       out_mx: Optional[Mx8] = None, out_plane: Optional[torch.Tensor] = None):
    """Encoder self-attention of the MX-FP8 and bf16 modes (lr2_self_attn_fwd_bf16).  qkv: ONE bf16 plane [batch * L, 3E] = [Q | K | V]
    (a 2-byte HIP tensor: what gemm_mxfp8(out_bf16=...) / gemm_bf16(out_plane=...) write); the context as fp32 `out` [batch * L, E]
    and / or as MX-FP8 `out_mx` and / or as ONE bf16 plane `out_plane` (a 2-byte HIP tensor [batch * L, E])."""
    E = heads * head_dim
    if qkv.element_size() != 2 or not qkv.is_cuda or qkv.numel() < batch * L * 3 * E:
        raise TypeError("self_attn_fwd_bf16: qkv is a 2-byte HIP tensor [batch * L, 3 * heads * head_dim]")
    if seg.dtype != torch.int64:
        raise TypeError("seg must be int64")
    _chk_f32(out)
    if out is None and out_mx is None and out_plane is None:
        raise ValueError("self_attn_fwd_bf16: out and / or out_mx and / or out_plane")
    ob = _plane_ptr(out_plane, batch * L * E, "self_attn_fwd_bf16: out_plane") if out_plane is not None else None
    if out_mx is not None and (out_mx.rows != batch * L or out_mx.cols != E):
        raise ValueError("self_attn_fwd_bf16: out_mx must be [batch * L, heads * head_dim]")
    base = qkv.data_ptr()
    with _Timed(f"selfattn_bf16_B{batch}_H{heads}_L{L}", 4.0 * batch * heads * L * L * head_dim, 7.0 * batch * L * E):
        _nat.check(_nat.lib().lr2_self_attn_fwd_bf16(base, base + 2 * E, base + 4 * E, 3 * E, seg.data_ptr(), _ptr(out),
                                                     out_mx.q.data_ptr() if out_mx is not None else None,
                                                     out_mx.s.data_ptr() if out_mx is not None else None, ob, E, batch, heads, L,
                                                     head_dim, scale, _stream()), "lr2_self_attn_fwd_bf16")
    return out if out is not None else (out_mx if out_mx is not None else out_plane)


def self_attn_fwd_bf16_blocked(qkv: torch.Tensor, seg, *, batch, heads, L, head_dim, scale, out: Optional[torch.Tensor] = None,
                               out_mx: Optional[Mx8] = None, out_plane: Optional[torch.Tensor] = None):
    """self_attn_fwd_bf16 with the keys walked in blocks through LDS (lr2_self_attn_fwd_bf16_blocked, csrc/selfattn_mx_blocked.hip): the
    same arguments, checks and outputs at any L >= 1 -- what the bf16 and MX-FP8 inference schedules run above 288 tokens with
    TransformerEncoder.infer_attention_long.  The plane is byte-equal to self_attn_fwd_bf16_train's at the same L without dropout."""
    E = heads * head_dim
    if qkv.element_size() != 2 or not qkv.is_cuda or qkv.numel() < batch * L * 3 * E:
        raise TypeError("self_attn_fwd_bf16_blocked: qkv is a 2-byte HIP tensor [batch * L, 3 * heads * head_dim]")
    if seg.dtype != torch.int64:
        raise TypeError("seg must be int64")
    _chk_f32(out)
    if out is None and out_mx is None and out_plane is None:
        raise ValueError("self_attn_fwd_bf16_blocked: out and / or out_mx and / or out_plane")
    ob = _plane_ptr(out_plane, batch * L * E, "self_attn_fwd_bf16_blocked: out_plane") if out_plane is not None else None
    if out_mx is not None and (out_mx.rows != batch * L or out_mx.cols != E):
        raise ValueError("self_attn_fwd_bf16_blocked: out_mx must be [batch * L, heads * head_dim]")
    base = qkv.data_ptr()
    with _Timed(f"selfattn_bf16l_B{batch}_H{heads}_L{L}", 4.0 * batch * heads * L * L * head_dim, 7.0 * batch * L * E):
        _nat.check(_nat.lib().lr2_self_attn_fwd_bf16_blocked(base, base + 2 * E, base + 4 * E, 3 * E, seg.data_ptr(), _ptr(out),
                                                             out_mx.q.data_ptr() if out_mx is not None else None,
                                                             out_mx.s.data_ptr() if out_mx is not None else None, ob, E, batch, heads,
                                                             L, head_dim, scale, _stream()), "lr2_self_attn_fwd_bf16_blocked")
    return out if out is not None else (out_mx if out_mx is not None else out_plane)


def self_attn_fwd_bf16_blocked_launch_count() -> int:
    """Accepted self_attn_fwd_bf16_blocked calls since the library was loaded (a test hook: which attention a schedule ran)."""
    c = C.c_uint64()
    _nat.check(_nat.lib().lr2_self_attn_fwd_bf16_blocked_launch_count(C.byref(c)), "lr2_self_attn_fwd_bf16_blocked_launch_count")
    return int(c.value)


def self_attn_bf16_plan(batch: int, heads: int, L: int, ld: Optional[int] = None) -> bool:
    """True when self_attn_fwd_bf16 runs a call of this shape as persistent workgroups (lr2_self_attn_fwd_bf16_plan)."""
    f = C.c_int()
    _nat.check(_nat.lib().lr2_self_attn_fwd_bf16_plan(batch, heads, L, 3 * heads * 64 if ld is None else ld, C.byref(f)),
               "lr2_self_attn_fwd_bf16_plan")
    return bool(f.value)


def _attn_plane_args(what: str, seg, batch, heads, L, head_dim, planes):
    """Checks shared by the two single-plane training attention calls: every (name, tensor, columns) of `planes` is ONE bf16 plane
    [batch * L, columns]; seg is int64.  Returns E."""
    E = heads * head_dim
    if seg.dtype != torch.int64:
        raise TypeError("seg must be int64")
    for name, t, cols in planes:
        _plane_ptr(t, batch * L * cols, f"{what}: {name}")
    return E


def self_attn_fwd_bf16_train(qkv: torch.Tensor, seg, out_plane: torch.Tensor, *, batch, heads, L, head_dim, scale,
                             lse: Optional[torch.Tensor] = None, drop: Optional[Drop] = None):
    """Encoder self-attention of the bf16_train mode, forward (lr2_self_attn_fwd_bf16_train).  qkv: ONE bf16 plane [batch * L, 3E] =
    [Q | K | V] (what gemm_bf16_train(out_plane=...) writes); out_plane: the context as ONE bf16 plane [batch * L, E]; lse: optional
    fp32 [batch * heads * L]; drop: dropout on the probabilities (self_attn_fwd's mask stream).  head_dim 64; L <= 288 runs the
    one-block kernels, a longer sequence the key-blocked ones (lr2_self_attn_fwd_bf16_train_blocked: the same arithmetic contract)."""
    E = _attn_plane_args("self_attn_fwd_bf16_train", seg, batch, heads, L, head_dim, (("qkv", qkv, 3 * heads * head_dim),
                                                                                     ("out_plane", out_plane, heads * head_dim)))
    _chk_f32(lse)
    if lse is not None and lse.numel() < batch * heads * L:
        raise ValueError("self_attn_fwd_bf16_train: lse too small")
    q, k, v = _qkv_ptrs(qkv, E)
    p, seed, site = (drop.p, drop.seed, drop.site) if drop is not None else (0.0, 0, 0)
    with _Timed(f"selfattn_b1t_B{batch}_H{heads}_L{L}", 4.0 * batch * heads * L * L * head_dim, 8.0 * batch * L * E):
        name = "lr2_self_attn_fwd_bf16_train" if L <= 288 else "lr2_self_attn_fwd_bf16_train_blocked"
        _nat.check(getattr(_nat.lib(), name)(q, k, v, 3 * E, seg.data_ptr(), out_plane.data_ptr(), E, _ptr(lse), p, seed, site, batch,
                                             heads, L, head_dim, scale, _stream()), name)
    return out_plane


def self_attn_bwd_bf16(qkv: torch.Tensor, do: torch.Tensor, seg, dqkv: torch.Tensor, lse_ws, dsum_ws, *, batch, heads, L, head_dim,
                       scale, drop: Optional[Drop] = None):
    """dQKV (ONE bf16 plane [batch * L, 3E]) from QKV [batch * L, 3E] and dO [batch * L, E] (ONE bf16 plane each) by the recomputing
    single-plane backward (lr2_self_attn_bwd_bf16; L > 288: lr2_self_attn_bwd_bf16_blocked); lse_ws / dsum_ws: fp32
    [batch * heads * L] scratch at any L.  `drop` as in the forward replays its mask; the forward's output and log-sum-exp are not
    needed."""
    E = _attn_plane_args("self_attn_bwd_bf16", seg, batch, heads, L, head_dim, (("qkv", qkv, 3 * heads * head_dim),
                                                                               ("do", do, heads * head_dim),
                                                                               ("dqkv", dqkv, 3 * heads * head_dim)))
    _chk_f32(lse_ws, dsum_ws)
    if lse_ws.numel() < batch * heads * L or dsum_ws.numel() < batch * heads * L:
        raise ValueError("self_attn_bwd_bf16: statistics workspaces too small")
    q, k, v = _qkv_ptrs(qkv, E)
    dq, dk, dv = _qkv_ptrs(dqkv, E)
    p, seed, site = (drop.p, drop.seed, drop.site) if drop is not None else (0.0, 0, 0)
    with _Timed(f"selfattnbwd_b1t_B{batch}_H{heads}_L{L}", 14.0 * batch * heads * L * L * head_dim, 16.0 * batch * L * E):
        name = "lr2_self_attn_bwd_bf16" if L <= 288 else "lr2_self_attn_bwd_bf16_blocked"
        _nat.check(getattr(_nat.lib(), name)(q, k, v, 3 * E, do.data_ptr(), E, seg.data_ptr(), dq, dk, dv, 3 * E, lse_ws.data_ptr(),
                                             dsum_ws.data_ptr(), p, seed, site, batch, heads, L, head_dim, scale, _stream()), name)
    return dqkv


def self_attn_bf16_train_launch_counts():
    """(forward, backward) calls of the single-plane training attention since the library was loaded."""
    c = (C.c_uint64 * 2)()
    _nat.check(_nat.lib().lr2_self_attn_bf16_train_launch_counts(c), "lr2_self_attn_bf16_train_launch_counts")
    return int(c[0]), int(c[1])


def self_attn_bf16_blocked_plan(L: int):
    """(forward key block, dQ key block, dK / dV query block): the block lengths the blocked single-plane training attention uses at
    this L (lr2_self_attn_bf16_blocked_plan; host only)."""
    f, q, kv = C.c_int(), C.c_int(), C.c_int()
    _nat.check(_nat.lib().lr2_self_attn_bf16_blocked_plan(L, C.byref(f), C.byref(q), C.byref(kv)), "lr2_self_attn_bf16_blocked_plan")
    return f.value, q.value, kv.value


def self_attn_bf16_blocked_launch_counts():
    """(forward, backward) calls of the BLOCKED single-plane training attention since the library was loaded."""
    c = (C.c_uint64 * 2)()
    _nat.check(_nat.lib().lr2_self_attn_bf16_blocked_launch_counts(c), "lr2_self_attn_bf16_blocked_launch_counts")
    return int(c[0]), int(c[1])


def text_embed(src, seg, word, pos, seg_table, out, *, rows, L, D, err: Optional[torch.Tensor] = None):
    """err: optional int32[1] device word; bit 0 / bit 1 are set when a token / segment id is out of range."""
    _chk_f32(word, pos, seg_table, out)
    if src.dtype != torch.int64 or seg.dtype != torch.int64:
        raise TypeError("src / seg must be int64")
    if L > pos.shape[0]:
        raise IndexError(f"sequence length {L} exceeds the position table ({pos.shape[0]} rows)")
    _nat.check(_nat.lib().lr2_text_embed(src.data_ptr(), seg.data_ptr(), word.data_ptr(), pos.data_ptr(), seg_table.data_ptr(),
                                         out.data_ptr(), rows, L, D, word.shape[0], seg_table.shape[0], _ptr(err), _stream()),
               "lr2_text_embed")
    return out


CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)     # tencentpretrain/utils/dataloader.py:561
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def patchify_planes(img, out: Planes, *, B, Cc, H, W, ps, mean=None, std=None):
    """Patch rows of `img` as planes [B*P, Cc*ps*ps].  img: fp32 [B,Cc,H,W], or uint8 frames (then normalised on the fly
    with mean / std per channel when both are given: (x / 255 - mean) / std)."""
    is_u8 = img.dtype == torch.uint8
    if not is_u8:
        _chk_f32(img)
    if not img.is_cuda or not img.is_contiguous():
        raise TypeError("patchify_planes: img must be a contiguous HIP tensor")
    P = (H // ps) * (W // ps)
    if out.rows != B * P or out.cols < Cc * ps * ps:
        raise ValueError("patchify_planes: out must be [B*P, >= C*ps*ps] planes (extra columns are zero-filled)")
    m3 = s3 = None
    if is_u8 and mean is not None and std is not None:
        m3, s3 = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
    _nat.check(_nat.lib().lr2_patchify_planes(img.data_ptr(), 1 if is_u8 else 0, out.data_ptr(), out.lo_off, out.cols, B, Cc, H, W,
                                              ps, m3, s3, _stream()), "lr2_patchify_planes")
    return out


_NDCG_TABLES = {}


def ndcg(scores, gold, offsets, ks=(1, 3, 5, 10, 20, 100000000)):
    """-> fp32 [n_items, len(ks)] NDCG@k of ragged items (scores / gold flat, offsets int64 [n_items + 1]), on the device."""
    _chk_f32(scores)
    if gold.dtype != torch.int64 or offsets.dtype != torch.int64:
        raise TypeError("gold / offsets must be int64")
    dev = scores.device
    key = (str(dev), tuple(ks))
    if key not in _NDCG_TABLES:
        # discount table computed exactly as the reference does (torch.log2 of an int64 tensor on the host, ndcg.py:31)
        disc = torch.log2(torch.arange(64, dtype=torch.int64) + 2).to(dev)
        _NDCG_TABLES[key] = (disc, torch.tensor(list(ks), dtype=torch.int64, device=dev))
    disc, ks_t = _NDCG_TABLES[key]
    n_items = offsets.numel() - 1
    out = torch.empty(n_items, len(ks), dtype=torch.float32, device=dev)
    if n_items > 0:
        _nat.check(_nat.lib().lr2_ndcg(scores.data_ptr(), gold.data_ptr(), offsets.data_ptr(), disc.data_ptr(), ks_t.data_ptr(),
                                       len(ks), out.data_ptr(), n_items, _stream()), "lr2_ndcg")
    return out


def patchify(img, out, *, B, Cc, H, W, ps):
    _chk_f32(img, out)
    _nat.check(_nat.lib().lr2_patchify(img.data_ptr(), out.data_ptr(), B, Cc, H, W, ps, _stream()), "lr2_patchify")
    return out


def vit_assemble(proj, cls, pos, out, *, B, P, D):
    _chk_f32(proj, cls, pos, out)
    _nat.check(_nat.lib().lr2_vit_assemble(proj.data_ptr(), cls.data_ptr(), pos.data_ptr(), out.data_ptr(), B, P, D, _stream()),
            "lr2_vit_assemble")
    return out
