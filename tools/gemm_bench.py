#!/usr/bin/env python3
"""Micro-benchmark of lr2_gemm on the shapes of the LR2PPO head (run on the GPU box).
usage: python tools/gemm_bench.py [--passes 3] [--iters 20]
       python tools/gemm_bench.py --bf16 [--bm 256|128] [--only ...]: the single-pass bf16 product (lr2_gemm_bf16) on the NT shapes
       python tools/gemm_bench.py --f16 [--bm 256|128|64] [--only ...]: the single-pass f16 product (lr2_gemm_f16_tiled) on the NT shapes;
           --bm 256: the 256 x 256 kernel under the row split, 128 / 64: the f16 short tiles; without --bm: ops.f16_block_m's choice;
           --f16-unsplit: lr2_gemm_f16 itself (one launch of the 256 x 256 kernel whatever the size: the baseline of the dispatch)
       python tools/gemm_bench.py --bf16 --tn [--bm 256|128] [--splits S] [--only ...]: the single-pass weight gradient
           (lr2_gemm_bf16_train, TN) on TN_B1_SHAPES, bias gradient included; without --bm each shape is timed on the 256 x 256 TN
           kernel, on the 128-row family at passes = 1 and on the 3-pass 256 x 256 TN kernel, in that order"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from lr2ppo_amd import ops  # noqa: E402

SHAPES = [  # (form, M, N, K) as ops.gemm sees them
    ("NT", 12544, 3072, 768), ("NT", 12544, 768, 3072), ("NT", 12544, 768, 768), ("NN", 12544, 768, 3072),
    ("NN", 12544, 3072, 768), ("TN", 3072, 768, 12544), ("TN", 768, 3072, 12544), ("TN", 768, 768, 12544),
    ("NT", 64, 3072, 162816), ("NN", 64, 162816, 3072), ("TN", 3072, 162816, 64), ("NT", 1024, 3072, 768),
    ("NT", 4096, 4096, 4096),
    # dual-encoder forward at batch 32 (M = 32 * 197)
    ("NT", 6304, 2304, 768), ("NT", 6304, 768, 768), ("NT", 6304, 3072, 768), ("NT", 6304, 768, 3072),
    # NT vs NN (forward on W or on W^T) at the encoder's shapes
    ("NN", 6304, 2304, 768), ("NN", 6304, 3072, 768), ("NT", 100864, 2304, 768), ("NN", 100864, 2304, 768),
    ("NT", 100864, 3072, 768), ("NN", 100864, 3072, 768),
    # small GEMMs of the PPO step (image tokens, tail, out_layer.fc2): where split-K + its reduce launch compete with one pass
    ("NT", 1024, 768, 768), ("NN", 1024, 3072, 768), ("NT", 1024, 768, 3072), ("NT", 64, 768, 3072), ("NT", 256, 768, 768),
    ("TN", 768, 768, 1024), ("TN", 3072, 768, 1024), ("NN", 1024, 768, 3072),
    # 31..: ViT-B/16 forward over 512 frames (M = 512 * 197) and the pointwise head at 20 tags (M = 640 * 196)
    ("NT", 100864, 768, 768), ("NT", 100864, 768, 3072), ("NT", 125440, 3072, 768), ("NT", 125440, 768, 3072),
    ("NT", 8192, 8192, 8192),
    # 36: the QKV product of RoBERTa-base over 64 sequences (the M = 12 544 twin of shape 19)
    ("NT", 12544, 2304, 768),
]


# (N_out, N_in, T): the encoders' weight gradients over 512 frames x 197 tokens and over 64 sequences x 196 tokens
TN_B1_SHAPES = [(768, 3072, 100864), (3072, 768, 100864), (2304, 768, 100864), (768, 768, 100864),
                (768, 3072, 12544), (3072, 768, 12544), (2304, 768, 12544), (768, 768, 12544)]


def _time(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def bench_tn_b1(a, dev, g):
    """dW [N_out, N_in] = dY^T X and db = colsum(dY) as the bf16_train schedule calls them (engine.linear_wgrad_bf16)"""
    for si, (M, N, K) in enumerate(TN_B1_SHAPES):
        if a.only is not None and si not in a.only:
            continue
        A = torch.randn(K, M, device=dev, generator=g)
        B = torch.randn(K, N, device=dev, generator=g)
        Ap, Bp = ops.split_planes(A, ops.Planes.empty(K, M, dev)), ops.split_planes(B, ops.Planes.empty(K, N, dev))
        out, db = torch.empty(M, N, device=dev), torch.empty(M, device=dev)
        rule = ops.gemm256_tn_b1_splits(M, N, K)
        gbm, gsp = ops._general_tiling(M, N, K, True, True)
        cases = []
        if a.bm in (None, 256):
            cases.append(("bf16x1 256x256", 256, a.splits or max(1, rule), 1))
        if a.bm in (None, 128, 64):
            cases.append(("bf16x1 general", a.bm or gbm, a.splits or gsp, 1))
        if a.bm is None:
            bm3, sp3 = ops.choose_tiling(M, N, K, True, True)
            cases.append(("split-bf16 x3 ", bm3, sp3, 3))
        for label, bm, sp, passes in cases:
            ws = torch.empty(sp * M * N, device=dev) if sp > 1 else None
            cs_ws = torch.empty(max(128, sp * ((N + 255) // 256)) * M, device=dev)
            if passes == 1:
                fn = lambda: ops.gemm_bf16_train(Ap, Bp, out, M, N, K, trans=True, block_m=bm, splits=sp, splitk_ws=ws, colsum=db,  # noqa: E731
                                                 colsum_ws=cs_ws)
            else:
                fn = lambda: ops.gemm(Ap, Bp, out, M, N, K, trans_a=True, trans_b=True, lda=M, ldb=N, splitk_ws=ws, splits=sp,     # noqa: E731
                                      block_m=bm, passes=3, colsum=db, colsum_ws=cs_ws)
            ms = _time(fn, a.iters)
            print(f"{label} TN N_out={M:5d} N_in={N:5d} T={K:6d} bm={bm:3d} splits={sp:3d} (rule {rule:3d}): {ms * 1e3:8.1f} us  "
                  f"{2.0 * M * N * K / ms / 1e9:7.1f} TFLOP/s", flush=True)
        del A, B, Ap, Bp, out


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", type=int, nargs="*", default=None, help="indices into SHAPES")
    ap.add_argument("--planes", action="store_true", help="operands as pre-split bf16 hi/lo planes (LDS-DMA path)")
    ap.add_argument("--bm", type=int, default=None, help="override block_m")
    ap.add_argument("--splits", type=int, default=None, help="override split-K factor")
    ap.add_argument("--bf16", action="store_true", help="ONE bf16 plane per operand, one pass (ops.gemm_bf16; NT shapes only); "
                    "--bm 256: the 256 x 256 single-pass kernel, --bm 128: the 128-row family at passes = 1; default: by size")
    ap.add_argument("--f16", action="store_true", help="ONE f16 plane per operand, one pass (ops.gemm_f16; NT shapes only); "
                    "--bm 256: the 256 x 256 kernel under the row split, --bm 128 / 64: the f16 kernels of the 128- / 64-row family; "
                    "default: by size (ops.f16_block_m)")
    ap.add_argument("--f16-unsplit", action="store_true", help="with --f16: ops.gemm_f16(block_m=None) = lr2_gemm_f16, ONE launch of the "
                    "256 x 256 kernel at every size, no row split (excludes --bm)")
    ap.add_argument("--f16-schedule-epilogues", action="store_true", help="with --f16: each product with the epilogue and destination "
                    "TransformerEncoder.forward_f16 gives it -- N = 4 K (FFN-1): bias, GELU -> ONE f16 plane; N = 3 K (QKV): bias -> ONE "
                    "f16 plane; otherwise (wo, FFN-2): bias + residual -> fp32 -- instead of a bare fp32 result")
    ap.add_argument("--tn", action="store_true", help="with --bf16: the single-pass weight gradient (ops.gemm_bf16_train, TN) on TN_B1_SHAPES")
    a = ap.parse_args(argv)
    if a.f16 and (a.bf16 or a.tn):
        ap.error("--f16 is a mode of its own: it excludes --bf16 and --tn")
    if a.f16 and a.bm not in (None, 256, 128, 64):
        ap.error("--f16 --bm takes 256, 128 or 64")
    if a.f16_schedule_epilogues and not a.f16:
        ap.error("--f16-schedule-epilogues is a switch of --f16")
    if a.f16_unsplit and (not a.f16 or a.bm is not None):
        ap.error("--f16-unsplit is a switch of --f16 and excludes --bm")
    if a.tn and not a.bf16:
        ap.error("--tn is the weight-gradient form of the single-pass product: give --bf16")
    return a


def main():
    a = parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    if a.tn:
        return bench_tn_b1(a, dev, g)
    for si, (form, M, N, K) in enumerate(SHAPES):
        if a.only is not None and si not in a.only:
            continue
        ta, tb = form == "TN", form in ("NN", "TN")
        if a.f16:
            if form != "NT" or K % 64:
                continue
            A = torch.randn(M, K, device=dev, generator=g).to(torch.float16)
            B = torch.randn(N, K, device=dev, generator=g).to(torch.float16)
            out = torch.empty(M, N, device=dev)
            bm = None if a.f16_unsplit else (a.bm or ops.f16_block_m(M, N, K))
            kw, dst, epi = {}, out, "fp32"
            if a.f16_schedule_epilogues:
                kw["bias"] = torch.randn(N, device=dev, generator=g)
                if N in (3 * K, 4 * K):
                    epi = "bias+gelu->plane" if N == 4 * K else "bias->plane"
                    kw.update(act=1 if N == 4 * K else 0, out_plane=torch.empty(M * N, dtype=torch.float16, device=dev))
                    dst = None
                else:
                    epi = "bias+resid->fp32"
                    kw["resid"] = torch.randn(M, N, device=dev, generator=g)
            ms = _time(lambda: ops.gemm_f16(A, B, dst, M, N, K, block_m=bm, **kw), a.iters)
            print(f"f16x1 NT M={M:6d} N={N:6d} K={K:6d} {epi} bm={bm or 'unsplit'}: {ms:8.4f} ms  {2.0 * M * N * K / ms / 1e9:7.1f} TFLOP/s", flush=True)
            del A, B, out
            continue
        if a.bf16:
            if form != "NT" or K % 64:
                continue
            A = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
            B = torch.randn(N, K, device=dev, generator=g).to(torch.bfloat16)
            out = torch.empty(M, N, device=dev)
            bm = a.bm or (256 if ops.use_gemm256_b1(M, N, K) else ops._bf16_fallback_block_m(M, N))
            for _ in range(3):
                ops.gemm_bf16(A, B, out, M, N, K, block_m=bm)
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.iters):
                ops.gemm_bf16(A, B, out, M, N, K, block_m=bm)
            e.record()
            torch.cuda.synchronize()
            ms = s.elapsed_time(e) / a.iters
            print(f"bf16x1 NT M={M:6d} N={N:6d} K={K:6d} bm={bm}: {ms:8.4f} ms  {2.0 * M * N * K / ms / 1e9:7.1f} TFLOP/s", flush=True)
            del A, B, out
            continue
        A = torch.randn((K, M) if ta else (M, K), device=dev, generator=g)
        B = torch.randn((K, N) if tb else (N, K), device=dev, generator=g)
        out = torch.empty(M, N, device=dev)
        if a.planes:
            big_b = (M == 64 and K > 100000) or (N > 100000 and form == "NN")   # out_layer.fc1 weight: stays fp32
            Ap = ops.Planes.empty(*A.shape, dev)
            ops.split_planes(A, Ap)
            A = Ap
            if not big_b:
                Bp = ops.Planes.empty(*B.shape, dev)
                ops.split_planes(B, Bp)
                B = Bp
        bm, sp = ops.choose_tiling(M, N, K, ta, tb)
        bm = a.bm or bm
        sp = a.splits or sp
        ws = torch.empty(max(1, sp) * M * N, device=dev) if sp > 1 else None
        for _ in range(3):
            ops.gemm(A, B, out, M, N, K, trans_a=ta, trans_b=tb, splitk_ws=ws, passes=a.passes, block_m=bm, splits=sp)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.iters):
            ops.gemm(A, B, out, M, N, K, trans_a=ta, trans_b=tb, splitk_ws=ws, passes=a.passes, block_m=bm, splits=sp)
        e.record()
        torch.cuda.synchronize()
        ms = s.elapsed_time(e) / a.iters
        tf = 2.0 * M * N * K / ms / 1e9
        gbs = 4.0 * (M * K + N * K + M * N) / ms / 1e6
        print(f"{form} M={M:6d} N={N:6d} K={K:6d} bm={bm} splits={sp:2d}: {ms:8.4f} ms  {tf:7.1f} TFLOP/s  {gbs:7.0f} GB/s(alg)", flush=True)
        del A, B, out, ws


if __name__ == "__main__":
    main()
