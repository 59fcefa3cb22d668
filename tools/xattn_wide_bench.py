"""Times of the two forms of the XiT cross-attention pair and of the head-only PPO step at several --max_imgs.

Kernels, at the PPO shape (64 pairs, 8 heads, Lq 196, head_dim 96): the 16-key pair at Lk 16, the wide pair at Lk 16 / 32 / 48 / 64,
forward and backward, HIP events around `--iters` back-to-back launches after `--warmup` launches, one process, one session.
Head-only step (bench.py's: rollout + update_minibatch, 32 items x 2 tags, pre-extracted features) at max_imgs 16 / 32 / 64.
Prints one JSON line.  Usage: python tools/xattn_wide_bench.py [--iters 200] [--warmup 20] [--steps 10] [--no-step]"""
import argparse
import json
import math
import os
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def time_kernels(ops, dev, iters, warmup):
    batch, heads, Lq, hd = 64, 8, 196, 96
    E = heads * hd
    g = torch.Generator(device=dev).manual_seed(1)
    out = {}
    for Lk, wide in ((16, False), (16, True), (32, True), (48, True), (64, True)):
        q, do = (torch.randn(batch * Lq, E, device=dev, generator=g) * 0.5 for _ in range(2))
        k, v = (torch.randn(batch * Lk, E, device=dev, generator=g) * 0.5 for _ in range(2))
        o, dq = ops.Planes.empty(batch * Lq, E, dev), ops.Planes.empty(batch * Lq, E, dev)       # planes: what the heads ask for
        dk, dv = ops.Planes.empty(batch * Lk, E, dev), ops.Planes.empty(batch * Lk, E, dev)
        kw = dict(batch=batch, heads=heads, Lq=Lq, Lk=Lk, head_dim=hd, post_scale=1.0 / math.sqrt(E), wide=wide)
        fns = {"fwd": lambda: ops.xattn_fwd(q, k, v, o, **kw), "bwd": lambda: ops.xattn_bwd(q, k, v, do, dq, dk, dv, **kw)}
        for name, fn in fns.items():
            for _ in range(warmup):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[f"{'wide' if wide else 'narrow'}_k{Lk}_{name}_us"] = round(e0.elapsed_time(e1) / iters * 1e3, 2)
    return out


def time_step(dev, max_imgs, steps, warmup, batch=32, tags=2):
    from lr2ppo_amd import runtime
    from lr2ppo_amd.finetune import ppo
    margs = argparse.Namespace(mode="reg", labels_num=3, seq_length=196, max_imgs=max_imgs, visual_feat_dim=768, is_master=True,
                               kl_div_loss_weight=0.001, entropy_weight=0.001, value_clip=0.5, optimizer="adamw", scheduler="linear",
                               learning_rate=1e-3, critic_learning_rate=1e-3, train_steps=1000, warmup=0.1, device=dev,
                               fuse_fc1_update=True)
    torch.manual_seed(7)
    model = ppo.ActorCritic(margs, None).to(dev)
    reward = ppo.Reward(margs, None).to(dev).eval()
    with torch.no_grad():
        for p in list(model.parameters()) + list(reward.parameters()):
            p.normal_(0, 0.02)
    opt, copt, sch, csch = ppo.build_optimizer(margs, model)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(20):
            sch.step(), csch.step()
    model.actor.bind_grads(), model.critic.bind_grads()
    runtime.set_dropout_seed(1234)
    g = torch.Generator(device=dev).manual_seed(1000)
    data = [(torch.randn(batch, tags, 196, 768, device=dev, generator=g), torch.randn(batch, max_imgs, 768, device=dev, generator=g),
             torch.randint(0, 3, (batch, tags), device=dev, generator=g)) for _ in range(4)]

    def step(i):
        text, img, tgts = data[i % 4]
        model.eval()
        rec = ppo.rollout_step(model, reward, text, img, tgts)
        model.train()
        return ppo.update_minibatch(margs, model, opt, copt, rec)

    for i in range(warmup):
        m = step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        m = step(warmup + i)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    if not torch.isfinite(m).all():
        raise SystemExit("non-finite PPO metrics")
    return round(dt * 1e3, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-step", action="store_true", help="kernel times only")
    ap.add_argument("--lib", default=None, help="another build of the kernel library (A/B timing of one session)")
    a = ap.parse_args()
    if a.lib:
        from lr2ppo_amd import _native
        _native.use_library(a.lib)
    from lr2ppo_amd import ops
    dev = torch.device("cuda:0")
    out = {"kernels_us": time_kernels(ops, dev, a.iters, a.warmup)}
    if not a.no_step:
        out["head_only_step_ms"] = {}
        for max_imgs in (16, 32, 64):
            out["head_only_step_ms"][f"max_imgs_{max_imgs}"] = time_step(dev, max_imgs, a.steps, 3)
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
