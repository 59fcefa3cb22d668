"""HIP-event time of ONE optimizer step() over an Actor-sized parameter set (max_imgs = 16: about 0.52 G parameters, 96 % of them
out_layer.fc1.weight [3072, 162816]) for Adafactor (lr2_adafactor_multi) and for AdamW's unfused step (lr2_adamw_multi over every
tensor, what train_model runs with fuse_fc1_update=False), with the bytes each moves and the rate on its own byte count.

    python tools/optimizer_bench.py [--steps 20] [--warmup 5] [--max_imgs 16] [--phases]

Gradients are set once (seeded normals); the optimizers run in the order adamw, adafactor, adamw, adafactor on the same parameters so
that a drift of the machine shows as a difference between the two rounds.  --phases adds the Adafactor step over three parts of the
set alone (out_layer.fc1.weight, the other 2-D tensors, the 1-D tensors); events around step() cannot tell the four launches apart:
their times come from `rocprofv3 --kernel-trace --stats -- python tools/optimizer_bench.py` (kernel names adafactor_*_kernel).
Also reports the bytes of optimizer state either optimizer keeps for the set.  Prints one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--max_imgs", type=int, default=16)
    ap.add_argument("--phases", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optimizer_bench: needs the GPU (a CPU run gives no time)")
    from lr2ppo_amd.finetune import ppo
    from lr2ppo_amd.tencentpretrain.utils.optimizers import Adafactor, AdamW
    dev = torch.device("cuda:0")
    margs = argparse.Namespace(mode="reg", labels_num=3, seq_length=196, max_imgs=a.max_imgs, visual_feat_dim=768)
    torch.manual_seed(7)
    actor = ppo.Actor(margs, None).to(dev)
    gen = torch.Generator(device=dev).manual_seed(11)
    with torch.no_grad():
        for p in actor.parameters():
            p.normal_(0, 0.02, generator=gen)
            p.grad = torch.randn(p.shape, device=dev, generator=gen) * 0.1
    named = list(actor.named_parameters())
    groups = lambda ps: ppo._grouped(ps)                                   # noqa: E731
    n2 = sum(p.numel() for _, p in named if p.dim() == 2)
    n1 = sum(p.numel() for _, p in named if p.dim() == 1)
    out = {"max_imgs": a.max_imgs, "params": n1 + n2, "params_2d": n2, "params_1d": n1, "tensors": len(named),
           "adamw_bytes": 28 * (n1 + n2), "adafactor_bytes": 20 * n2 + 28 * n1}
    adamw = AdamW(groups(named), lr=1e-4, correct_bias=False)
    ada = Adafactor(groups(named), lr=1e-4, scale_parameter=False, relative_step=False)
    for rnd in (1, 2):
        for name, opt in (("adamw", adamw), ("adafactor", ada)):
            med, lo, hi = timed(opt.step, a.steps, a.warmup)
            out[f"{name}_ms_round{rnd}"] = round(med, 4)
            out[f"{name}_ms_min_max_round{rnd}"] = [round(lo, 4), round(hi, 4)]
            out[f"{name}_TBps_round{rnd}"] = round(out[f"{name}_bytes"] / (med * 1e-3) / 1e12, 3)
    out["adafactor_over_adamw"] = round(min(out["adafactor_ms_round1"], out["adafactor_ms_round2"])
                                        / min(out["adamw_ms_round1"], out["adamw_ms_round2"]), 4)
    out["state_bytes_adamw"] = 8 * (n1 + n2)
    out["state_bytes_adafactor"] = sum(4 * (p.shape[0] + p.shape[1]) if p.dim() == 2 else 4 * p.numel() for _, p in named)
    if a.phases:
        fc1 = [(n, p) for n, p in named if n.endswith("out_layer.fc1.weight")]
        rest2 = [(n, p) for n, p in named if p.dim() == 2 and not n.endswith("out_layer.fc1.weight")]
        only1 = [(n, p) for n, p in named if p.dim() == 1]
        for tag, ps in (("fc1", fc1), ("other_2d", rest2), ("1d", only1)):
            o = Adafactor([{"params": [p for _, p in ps], "weight_decay": 0.01}], lr=1e-4, scale_parameter=False, relative_step=False)
            med, _, _ = timed(o.step, a.steps, a.warmup)
            out[f"adafactor_{tag}_ms"] = round(med, 4)
            out[f"adafactor_{tag}_params"] = sum(p.numel() for _, p in ps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
