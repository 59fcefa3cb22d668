"""Dual-encoder forward micro-benchmark (ViT-B/16 + RoBERTa-base, random weights, batch 32 of the repo's default shapes).
Prints ms per forward, algorithmic TFLOP/s (2MNK of the GEMMs + 4 L^2 d of attention) and a per-kernel-class breakdown
from HIP events.  python tools/encoder_bench.py [--batch 32] [--iters 10] [--passes 3]
--train [--precision mxfp8_train | bf16_train [--bf16-attention [--bf16-attention-long]]] [--recompute]: forward + backward per step, and
the step's peak device memory.  --text-seq L / --only text | image: the text tower at another sequence length / one tower alone.
--ppo-shapes --precision bf16 | f16 | mxfp8 with --text-seq / --only: the per-tower loop on that inference schedule (forward_bf16 /
forward_f16 / forward_fp8);
[--attention-long]: sequences longer than 288 on the key-blocked single-plane attention (TransformerEncoder.infer_attention_long);
[--f16-attention-long] (--precision f16): the same on the key-blocked f16 kernel (TransformerEncoder.f16_attention_long)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lr2ppo_amd import ops  # noqa: E402
from lr2ppo_amd.tencentpretrain.encoders import str2encoder  # noqa: E402
from lr2ppo_amd.tencentpretrain.opts import finetune_opts, tokenizer_opts  # noqa: E402

VIT = dict(emb_size=768, feedforward_size=3072, hidden_size=768, hidden_act="gelu", heads_num=12, layers_num=12, dropout=0.1,
           max_seq_length=197, encoder="transformer", mask="fully_visible", layernorm_positioning="pre")
ROBERTA = dict(emb_size=768, feedforward_size=3072, hidden_size=768, hidden_act="gelu", heads_num=12, layers_num=12,
               max_seq_length=514, dropout=0.1, encoder="transformer", mask="fully_visible")


def _args(**over):
    p = argparse.ArgumentParser()
    finetune_opts(p)
    tokenizer_opts(p)
    d = vars(p.parse_args([]))
    d.update(over)
    return argparse.Namespace(**d)


def flops(B, L, E=768, F=3072, layers=12, heads=12, first_token_only=False):
    """Matrix flops of one encoder forward.  first_token_only: the last layer as TransformerEncoder.forward_first_token runs
    it (keys / values for every row; query, scores, projection and feed-forward for row 0 of each sequence)."""
    M = B * L
    gemm = 2.0 * M * E * (3 * E + E + 2 * F)
    attn = 4.0 * B * heads * L * L * (E // heads)
    if not first_token_only:
        return layers * (gemm + attn)
    last = 2.0 * M * E * (2 * E) + 2.0 * B * E * (E + E + 2 * F) + 4.0 * B * heads * L * (E // heads)
    return (layers - 1) * (gemm + attn) + last


def measure_forward(batch_items=32, tags=2, n_img=16, iters=3, passes=3, dev=None, precision="split_bf16"):
    """Dual-encoder forward at the PPO step's feature-extraction shapes: ViT-B/16 over batch_items*n_img frames
    [*, 197, 768], RoBERTa-base over batch_items*tags label sequences [*, 196, 768]; random N(0, 0.02) weights.
    -> {"ms", "algorithmic_tflop", "tflops", "mfma_issue_frac"} (MFMA issue fraction = passes * flops / time / 2.5 PF).
    precision: "split_bf16" (enc.forward), "bf16" (enc.forward_bf16: one pass), "f16" (enc.forward_f16: one pass) or "mxfp8"
    (enc.forward_fp8)."""
    dev = dev or torch.device("cuda:0")
    ops.set_gemm_passes(passes)
    if precision != "split_bf16":
        passes = 1
    total_ms, total_fl, parts = 0.0, 0.0, {}
    for name, cfg, B, L in (("vit-b/16", VIT, batch_items * n_img, 197), ("roberta-base", ROBERTA, batch_items * tags, 196)):
        enc = str2encoder["transformer"](_args(**cfg))
        with torch.no_grad():
            for n, p in enc.named_parameters():
                if "gamma" not in n and "beta" not in n:
                    p.normal_(0, 0.02)
        enc = enc.to(dev).eval()
        emb = torch.randn(B, L, 768, device=dev)
        seg = torch.ones(B, L, dtype=torch.int64, device=dev)
        fwd = {"split_bf16": enc, "bf16": enc.forward_bf16, "f16": enc.forward_f16, "mxfp8": enc.forward_fp8}[precision]
        with torch.no_grad():
            fwd(emb, seg)
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(iters):
                fwd(emb, seg)
            e.record()
            torch.cuda.synchronize()
        ms = s.elapsed_time(e) / iters
        fl = flops(B, L)
        parts[name] = {"batch": B, "seq": L, "ms": round(ms, 3), "tflops": round(fl / ms / 1e9, 1)}
        total_ms += ms
        total_fl += fl
        del enc, emb
        torch.cuda.empty_cache()
    return {"ms": round(total_ms, 3), "algorithmic_tflop": round(total_fl / 1e12, 2), "tflops": round(total_fl / total_ms / 1e9, 1),
            "mfma_issue_frac": round(passes * total_fl / total_ms / 1e9 / 2500.0, 4), "passes": passes, "precision": precision, "parts": parts}


def parse_args(argv=None):
    """The command line, checked (argparse's error exit on a combination that means nothing); no device is touched."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--ppo-shapes", action="store_true", help="ViT over batch*16 frames, RoBERTa over batch*2 sequences")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--detail", action="store_true", help="per-signature launch averages")
    ap.add_argument("--train", action="store_true", help="time forward + backward (train mode, dropout 0.1) instead; with "
                    "--ppo-shapes: both towers at the PPO sizes (ViT over batch*16 frames, RoBERTa over batch*2 sequences)")
    ap.add_argument("--precision", choices=("split_bf16", "mxfp8_train", "bf16_train", "bf16", "f16", "mxfp8"), default="split_bf16",
                    help="--train: the encoders' training precision (split_bf16 | mxfp8_train | bf16_train); "
                         "--ppo-shapes without --train: the inference precision (split_bf16 | bf16 | f16 | mxfp8)")
    ap.add_argument("--recompute", action="store_true",
                    help="--train: keep each layer's input only and re-run a layer's forward in front of its backward "
                         "(TransformerEncoder.recompute); the peak-memory figure shows what that buys, the step time what it costs")
    ap.add_argument("--bf16-attention", action="store_true",
                    help="--train --precision bf16_train: the attention core on ONE bf16 plane per operand too "
                         "(TransformerEncoder.bf16_attention)")
    ap.add_argument("--bf16-attention-long", action="store_true",
                    help="--bf16-attention: sequences longer than 288 on the blocked single-plane kernels too "
                         "(TransformerEncoder.bf16_attention_long)")
    ap.add_argument("--attention-long", action="store_true",
                    help="--precision bf16 | mxfp8 (inference): sequences longer than 288 on the key-blocked single-plane attention "
                         "(TransformerEncoder.infer_attention_long) instead of the 3-pass kernels")
    ap.add_argument("--f16-attention-long", action="store_true",
                    help="--ppo-shapes --precision f16 (inference): sequences longer than 288 on the key-blocked single-plane f16 "
                         "attention (TransformerEncoder.f16_attention_long) instead of the 3-pass kernels")
    ap.add_argument("--f16-force-256", action="store_true",
                    help="--ppo-shapes --precision f16 (inference): every product on the 256 x 256 f16 kernel (ops.f16_force_256: the "
                         "schedule before the short f16 tiles) -- the other side of an A/B against ops.f16_block_m's dispatch")
    ap.add_argument("--text-seq", type=int, default=196, help="sequence length of the text tower (at most 514)")
    ap.add_argument("--only", choices=("both", "image", "text"), default="both", help="run one tower alone")
    a = ap.parse_args(argv)
    if a.bf16_attention_long and not a.bf16_attention:
        ap.error("--bf16-attention-long is a switch of --bf16-attention")
    if not 1 <= a.text_seq <= ROBERTA["max_seq_length"]:
        ap.error("--text-seq: 1 .. %d" % ROBERTA["max_seq_length"])
    if a.attention_long and (a.train or a.precision not in ("bf16", "mxfp8")):
        ap.error("--attention-long is a switch of the inference modes: give --precision bf16 | mxfp8, not --train "
                 "(--precision f16 has --f16-attention-long)")
    if a.f16_attention_long and (a.train or not a.ppo_shapes or a.precision != "f16"):
        ap.error("--f16-attention-long is a switch of the f16 inference mode: give --ppo-shapes --precision f16, not --train")
    if a.f16_force_256 and (a.train or not a.ppo_shapes or a.precision != "f16"):
        ap.error("--f16-force-256 is a switch of the f16 inference mode: give --ppo-shapes --precision f16, not --train")
    if (a.text_seq != 196 or a.only != "both") and a.ppo_shapes and not a.train and a.precision not in ("bf16", "f16", "mxfp8"):
        ap.error("--text-seq / --only are switches of the per-tower loop: not of --ppo-shapes without --train "
                 "(--precision bf16 | f16 | mxfp8 excepted: they then run the per-tower loop on their own schedule)")
    if a.bf16_attention and not (a.train and a.precision == "bf16_train"):
        ap.error("--bf16-attention is a switch of --train --precision bf16_train")
    if a.recompute and not a.train:
        ap.error("--recompute is a switch of the training schedule: give --train")
    if a.precision == "bf16_train" and not a.train:
        ap.error("--precision bf16_train is a training precision: give --train")
    if a.precision in ("bf16", "f16", "mxfp8") and (a.train or not a.ppo_shapes):
        ap.error("--precision bf16 / f16 / mxfp8 are inference modes: give --ppo-shapes, not --train")
    return a


def main():
    a = parse_args()
    if a.f16_force_256:
        with ops.f16_force_256():
            return _run(a)
    return _run(a)


def _run(a):
    dev = torch.device("cuda:0")
    ops.set_gemm_passes(a.passes)
    torch.manual_seed(0)
    infer = a.precision if a.precision in ("bf16", "f16", "mxfp8") else None          # (parse_args: never with --train)
    per_tower = infer is not None and (a.text_seq != 196 or a.only != "both" or a.attention_long or a.f16_attention_long)
    if a.ppo_shapes and not a.train and not per_tower:
        prec = "split_bf16" if a.precision == "mxfp8_train" else a.precision      # (a training precision: ignored without --train)
        print(measure_forward(a.batch, iters=a.iters, passes=a.passes, dev=dev, precision=prec))
        return
    total_ms, total_fl = 0.0, 0.0
    passes = 1 if infer else a.passes
    towers = [t for t in (("vit-b/16", VIT, 197), ("roberta-base", ROBERTA, a.text_seq))
              if a.only == "both" or t[0].startswith("vit") == (a.only == "image")]
    for name, cfg, L in towers:
        enc = str2encoder["transformer"](_args(**cfg))
        with torch.no_grad():
            for n, p in enc.named_parameters():
                if "gamma" not in n and "beta" not in n:
                    p.normal_(0, 0.02)
        enc = enc.to(dev)
        enc = enc.train() if a.train else enc.eval()
        enc.fp8_train = a.train and a.precision == "mxfp8_train"
        enc.bf16_train = a.train and a.precision == "bf16_train"
        enc.bf16_attention = a.bf16_attention
        enc.bf16_attention_long = a.bf16_attention_long
        enc.recompute = a.recompute
        enc.infer_attention_long = a.attention_long
        enc.f16_attention_long = a.f16_attention_long
        infer_fwd = {"bf16": enc.forward_bf16, "f16": enc.forward_f16, "mxfp8": enc.forward_fp8, None: enc}[infer]
        B = (a.batch * 16 if name.startswith("vit") else a.batch * 2) if a.ppo_shapes else a.batch
        emb = torch.randn(B, L, 768, device=dev, requires_grad=a.train)
        seg = torch.ones(B, L, dtype=torch.int64, device=dev)
        dout = torch.randn(B, L, 768, device=dev)

        def run():
            if a.train:
                enc(emb, seg).backward(dout)
            else:
                with torch.no_grad():
                    infer_fwd(emb, seg)
        for _ in range(2):
            run()
        torch.cuda.synchronize()
        resident = torch.cuda.memory_allocated()                      # parameters, gradients, workspace, inputs
        torch.cuda.reset_peak_memory_stats()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.iters):
            run()
        e.record()
        torch.cuda.synchronize()
        ms = s.elapsed_time(e) / a.iters
        peak = torch.cuda.max_memory_allocated()
        fl = flops(B, L) * (3.0 if a.train else 1.0)
        total_ms += ms
        total_fl += fl
        ops.profile_start()
        run()
        prof = ops.profile_stop()
        classes = {}
        for k, v in prof.items():
            c = k.split("_")[0] + ("_" + k.split("_")[1] if k.startswith("gemm") else "")
            classes[c] = classes.get(c, 0.0) + v["ms"]
        print(f"{name:13s} B={B} L={L} {a.precision if a.train or infer else ''}{' attention-long' if a.attention_long else ''}{' f16-attention-long' if a.f16_attention_long else ''}: {ms:7.3f} ms/{'step' if a.train else 'forward'}  {fl / ms / 1e9:7.1f} TFLOP/s (algorithmic)  "
              f"frac of 2.5 PF bf16 dense x{passes} passes: {passes * fl / ms / 1e9 / 2500:.3f}", flush=True)
        if a.train:
            print(f"    recompute {'on' if a.recompute else 'off'}: peak memory {peak / 2 ** 30:.2f} GiB ({(peak - resident) / 2 ** 30:.2f} GiB above "
                  f"the resident {resident / 2 ** 30:.2f}); saved activations by the formula {enc.saved_activation_bytes(B, L) / 2 ** 30:.2f} GiB",
                  flush=True)
        print("    events:", {k: round(v, 3) for k, v in sorted(classes.items(), key=lambda kv: -kv[1])}, flush=True)
        if a.detail:
            for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"]):
                tf = v["flops"] / (v["ms"] / v["n"]) / 1e9 if v["flops"] else 0.0
                print(f"      {k:40s} n={v['n']:3d} avg {v['ms'] / v['n'] * 1e3:8.1f} us  {tf:7.1f} TFLOP/s", flush=True)
    print(f"dual encoder: {total_ms:.3f} ms  {total_fl / total_ms / 1e9:.1f} TFLOP/s algorithmic, "
          f"MFMA issue fraction {passes * total_fl / total_ms / 1e9 / 2500:.3f}")


if __name__ == "__main__":
    main()
