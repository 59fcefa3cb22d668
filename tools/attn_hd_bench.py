"""Times of the head-width-general self-attention pair (csrc/selfattn_hd.hip) and of the ViT-H/14 tower.

Kernels, each launch between its own pair of HIP events, the median / minimum / maximum of `--iters` launches after `--warmup`:
  * width 64 through lr2_self_attn_hd_fwd / lr2_self_attn_hd_bwd against lr2_self_attn_fwd / lr2_self_attn_bwd (no `o_hi`: the
    recomputing backward) at (batch, heads, L) = (64, 16, 257) -- the 64-column forward is its key-blocked, non-persistent kernel there --
    and at (64, 12, 197), where the 64-column forward takes its persistent form (one pair per CU); its non-persistent one-block form is
    timed at (21, 12, 197) = 252 pairs, below the CU count, beside the new pair at the same shape: that ratio is the like-for-like one;
  * width 80 at (64 frames x 16 heads, L = 257): ViT-H/14's own attention.
Tower: lr2ppo_amd/configs/vit_huge_14_224.json, 32 layers, random weights, 64 frames x 257 tokens: the inference forward, and one
training forward + backward of the tower alone (split-bf16, dropout as configured), `--steps` repetitions each.  The fraction of the
nominal MFMA rate counts 3 passes over the algorithmic flops at 2.5 PFLOP/s, the attention at the PADDED width 96 stated separately.
Prints one JSON line.  Usage: python tools/attn_hd_bench.py [--iters 30] [--warmup 5] [--steps 20] [--no-tower]"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 2.5e15          # nominal dense bf16 MFMA rate


def _timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median_us": round(statistics.median(ms) * 1e3, 1), "min_us": round(min(ms) * 1e3, 1), "max_us": round(max(ms) * 1e3, 1)}


def time_kernels(ops, lib, dev, iters, warmup):
    out = {}
    g = torch.Generator(device=dev).manual_seed(1)
    for batch, heads, L, hd, names in ((64, 16, 257, 64, ("hd", "w64")), (64, 12, 197, 64, ("hd", "w64")),
                                       (21, 12, 197, 64, ("hd", "w64")), (64, 16, 257, 80, ("hd",))):
        E, n = heads * hd, batch * L
        qkv = ops.split_planes(torch.randn(n, 3 * E, device=dev, generator=g), ops.Planes.empty(n, 3 * E, dev))
        do = ops.split_planes(torch.randn(n, E, device=dev, generator=g), ops.Planes.empty(n, E, dev))
        o, dqkv = ops.Planes.empty(n, E, dev), ops.Planes.empty(n, 3 * E, dev)
        seg = torch.ones(n, dtype=torch.int64, device=dev)
        lse, ws1, ws2 = (torch.empty(batch * heads * L, device=dev) for _ in range(3))
        scale = 1.0 / math.sqrt(hd)
        base, dbase = qkv.data_ptr(), dqkv.data_ptr()

        def fwd(entry):
            rc = getattr(lib, entry)(base, base + 2 * E, base + 4 * E, qkv.lo_off, 3 * E, seg.data_ptr(), None, o.data_ptr(), o.lo_off, E,
                                     lse.data_ptr(), 0.0, 0, 0, batch, heads, L, hd, scale, None)
            assert rc == 0, (entry, rc)

        def bwd(entry):
            rc = getattr(lib, entry)(base, base + 2 * E, base + 4 * E, qkv.lo_off, 3 * E, do.data_ptr(), do.lo_off, E, seg.data_ptr(),
                                     dbase, dbase + 2 * E, dbase + 4 * E, dqkv.lo_off, 3 * E, None, 0, 0, ws1.data_ptr(), ws2.data_ptr(),
                                     0.0, 0, 0, batch, heads, L, hd, scale, None)
            assert rc == 0, (entry, rc)

        key = f"B{batch}_H{heads}_L{L}_hd{hd}"
        out[key] = {}
        for nm in names:
            suffix = "_hd" if nm == "hd" else ""
            out[key][f"{nm}_fwd"] = _timed(lambda: fwd(f"lr2_self_attn{suffix}_fwd"), iters, warmup)
            out[key][f"{nm}_bwd"] = _timed(lambda: bwd(f"lr2_self_attn{suffix}_bwd"), iters, warmup)
        if "w64" in names:
            for d in ("fwd", "bwd"):
                out[key][f"{d}_ratio_hd_over_w64"] = round(out[key][f"hd_{d}"]["median_us"] / out[key][f"w64_{d}"]["median_us"], 3)
        else:
            # algorithmic flops of the padded width: 2 products forward, 7 backward (5 in the two-sweep dQ kernel, 4 in dK / dV,
            # S and dP recomputed: 9 executed) of 2 L^2 HDP each, 3 passes
            hdp = (hd + 31) // 32 * 32
            per = 2.0 * batch * heads * L * L
            out[key]["fwd_frac_nominal"] = round(3 * 2 * per * hd / (out[key]["hd_fwd"]["median_us"] * 1e-6) / PEAK, 4)
            out[key]["fwd_frac_nominal_padded"] = round(3 * 2 * per * hdp / (out[key]["hd_fwd"]["median_us"] * 1e-6) / PEAK, 4)
            out[key]["bwd_frac_nominal"] = round(3 * 5 * per * hd / (out[key]["hd_bwd"]["median_us"] * 1e-6) / PEAK, 4)
            out[key]["bwd_frac_nominal_padded_executed"] = round(3 * 9 * per * hdp / (out[key]["hd_bwd"]["median_us"] * 1e-6) / PEAK, 4)
    return out


def time_tower(dev, steps, frames=64):
    from lr2ppo_amd import runtime
    from lr2ppo_amd.finetune.features import IMAGE_TOWERS, encoder_args
    from lr2ppo_amd.tencentpretrain.encoders import str2encoder
    a = encoder_args(IMAGE_TOWERS["vit_huge_14_224"])
    enc = str2encoder["transformer"](a).to(dev)
    g = torch.Generator(device=dev).manual_seed(2)
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if "gamma" not in n and "beta" not in n:
                p.normal_(0, 0.02, generator=g)
    L, E, F, H = a.max_seq_length, a.hidden_size, a.feedforward_size, a.heads_num
    emb = torch.randn(frames, L, E, device=dev, generator=g)
    dout = torch.randn(frames, L, E, device=dev, generator=g) * 0.1
    seg = torch.ones(frames, L, dtype=torch.int64, device=dev)
    M = frames * L
    gemm = 2.0 * M * (4 * E * E + 2 * E * F) * a.layers_num              # QKV, output projection, two feed-forward products
    attn = lambda hd: 2.0 * 2 * frames * H * L * L * hd * a.layers_num    # noqa: E731  (Q K^T and P V)
    hd, hdp = E // H, (E // H + 31) // 32 * 32
    enc.eval()
    with torch.no_grad():
        fwd = _timed(lambda: enc(emb, seg), steps, 2)
    enc.train()
    runtime.set_dropout_seed(1234)

    def train():
        out, saved = enc._forward_train(emb, seg)
        enc._backward_train(saved, dout)

    trn = _timed(train, steps, 2)
    t_f, t_t = fwd["median_us"] * 1e-6, trn["median_us"] * 1e-6
    return {"frames": frames, "tokens": L, "layers": a.layers_num, "forward": fwd, "train_fwd_bwd": trn,
            "forward_algorithmic_tflop": round((gemm + attn(hd)) / 1e12, 2),
            "forward_frac_nominal": round(3 * (gemm + attn(hd)) / t_f / PEAK, 4),
            "forward_frac_nominal_padded_attention": round(3 * (gemm + attn(hdp)) / t_f / PEAK, 4),
            "train_frac_nominal": round(3 * 3 * (gemm + attn(hd)) / t_t / PEAK, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--no-tower", action="store_true", help="kernel times only")
    a = ap.parse_args()
    if a.iters < 20 or a.steps < 20:
        raise SystemExit("at least 20 timed launches per figure")
    from lr2ppo_amd import _native, ops
    dev = torch.device("cuda:0")
    out = {"kernels": time_kernels(ops, _native.lib(), dev, a.iters, a.warmup)}
    if not a.no_tower:
        out["vit_huge_14_224"] = time_tower(dev, a.steps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
