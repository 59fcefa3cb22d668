"""HIP-event time of one stage-3 PPO update (ppo.update_minibatch: actor + critic forward, loss, backward, optimizer steps) at the
bench's head-only shape (batch 32 x 2 tags, max_imgs 16) in three variants on the same models and the same rollout record:

    unclipped       the default path (out_layer.fc1 update fused into its weight-gradient GEMM)
    clip_fused      --max_grad_norm on the fused route: the fc1 gradient's norm from its factors' two Gram products
    clip_plain      --max_grad_norm with fuse_fc1_update=False: the 2 GB gradient written, read for the norm, read for the update

    python tools/clip_bench.py [--rounds 7] [--steps 5] [--warmup 3] [--batch 32] [--max_imgs 16] [--max_norm 1.0]

The variants are alternated in one process after warm-up (round r runs all three, `steps` updates each inside one event pair), so a
drift of the machine shows in all of them; per variant the median per-step time over the rounds and the spread (min, max).  Prints
one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--tags", type=int, default=2)
    ap.add_argument("--max_imgs", type=int, default=16)
    ap.add_argument("--max_norm", type=float, default=1.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_bench: needs the GPU (a CPU run gives no time)")
    from lr2ppo_amd import runtime
    from lr2ppo_amd.finetune import ppo
    dev = torch.device("cuda:0")

    def args_of(**kw):
        return argparse.Namespace(mode="reg", labels_num=3, seq_length=196, max_imgs=a.max_imgs, visual_feat_dim=768, is_master=True,
                                  kl_div_loss_weight=0.001, entropy_weight=0.001, value_clip=0.5, optimizer="adamw",
                                  scheduler="constant", learning_rate=1e-5, critic_learning_rate=1e-5, train_steps=1000, warmup=0.1,
                                  device=dev, **kw)

    with torch.device(dev):
        model, reward = ppo.ActorCritic(args_of(), None), ppo.Reward(args_of(), None)
    torch.manual_seed(7)
    ppo._init_normal(model), ppo._init_normal(reward)
    reward.eval()
    gen = torch.Generator().manual_seed(11)
    text = torch.randn(a.batch, a.tags, 196, 768, generator=gen).to(dev)
    img = torch.randn(a.batch, a.max_imgs, 768, generator=gen).to(dev)
    tgts = torch.randint(0, 3, (a.batch, a.tags), generator=gen).to(dev)
    runtime.set_dropout_seed(3)
    model.eval()
    record = ppo.rollout_step(model, reward, text, img, tgts)
    model.train()
    model.actor.bind_grads(), model.critic.bind_grads()
    variants = {}
    for name, kw in (("unclipped", {}), ("clip_fused", {"max_grad_norm": a.max_norm}),
                     ("clip_plain", {"max_grad_norm": a.max_norm, "fuse_fc1_update": False})):
        args = args_of(**kw)
        opt, copt, _, _ = ppo.build_optimizer(args, model)
        variants[name] = (args, opt, copt)

    def run(name, n):
        args, opt, copt = variants[name]
        for _ in range(n):
            ppo.update_minibatch(args, model, opt, copt, record)

    for name in variants:
        run(name, a.warmup)
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(a.rounds):
        for name in variants:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            run(name, a.steps)
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e) / a.steps)
    out = {"batch": a.batch, "tags": a.tags, "max_imgs": a.max_imgs, "rounds": a.rounds, "steps": a.steps, "max_norm": a.max_norm}
    for name, ts in times.items():
        ts = sorted(ts)
        out[f"{name}_ms"] = round(ts[len(ts) // 2], 4)
        out[f"{name}_ms_min_max"] = [round(ts[0], 4), round(ts[-1], 4)]
    for name in ("clip_fused", "clip_plain"):
        out[f"{name}_minus_unclipped_ms"] = round(out[f"{name}_ms"] - out["unclipped_ms"], 4)
        _, opt, copt = variants[name]
        out[f"{name}_total_norm"] = [round(float(opt.total_norm), 6), round(float(copt.total_norm), 6)]
        out[f"{name}_coef"] = [round(float(opt.clip_coef), 6), round(float(copt.clip_coef), 6)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
