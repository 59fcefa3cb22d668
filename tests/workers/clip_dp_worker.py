"""Fresh child process: gradient-norm clipping under the data-parallel exchange path, ONE RCCL rank on cuda:0 with the exchange forced
(LR2_DP_FORCE=1).  The norm of out_layer.fc1's gradient then comes from the GATHERED factors with alpha = 1 / world, after the tail
all-reduce has been waited for; every collective is the identity at world 1, so two rollout + update steps must leave the bits of
the plain clipped step (weights, first moments, metrics, norms and coefficients), on one stream and on two."""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

_INIT = {}


def run(force: bool, streams: str, dev):
    from lr2ppo_amd import runtime
    from lr2ppo_amd.finetune import ppo
    os.environ["LR2_DP_FORCE"] = "1" if force else "0"
    os.environ["LR2_PPO_STREAMS"] = streams
    args = argparse.Namespace(mode="reg", labels_num=3, seq_length=196, max_imgs=16, visual_feat_dim=768, is_master=True,
                              kl_div_loss_weight=0.001, entropy_weight=0.001, value_clip=0.5, optimizer="adamw", scheduler="linear",
                              learning_rate=1e-3, critic_learning_rate=1e-3, train_steps=41, warmup=0.1, device=dev,
                              max_grad_norm=0.02)
    with torch.device(dev):
        model, reward = ppo.ActorCritic(args, None), ppo.Reward(args, None)
    if not _INIT:
        torch.manual_seed(5)
        for m in (model, reward):
            ppo._init_normal(m)
        _INIT["model"] = {k: v.detach().clone() for k, v in model.state_dict().items()}
        _INIT["reward"] = {k: v.detach().clone() for k, v in reward.state_dict().items()}
    else:
        model.load_state_dict(_INIT["model"], strict=True)
        reward.load_state_dict(_INIT["reward"], strict=True)
    reward.eval()
    opt, copt, sch, csch = ppo.build_optimizer(args, model)
    assert opt.max_grad_norm == 0.02 and copt.max_grad_norm == 0.02
    for _ in range(3):
        sch.step(), csch.step()
    model.actor.bind_grads(), model.critic.bind_grads()
    runtime.set_dropout_seed(99)
    dp = ppo._DataParallel()
    assert dp.active == force and dp.world == 1 and dp.backend == "nccl"
    gen = torch.Generator().manual_seed(23)
    mets, clips = [], []
    for _ in range(2):
        text, img = torch.randn(4, 2, 196, 768, generator=gen).to(dev), torch.randn(4, 16, 768, generator=gen).to(dev)
        tg = torch.randint(0, 3, (4, 2), generator=gen).to(dev)
        model.eval()
        rec = ppo.rollout_step(model, reward, text, img, tg)
        model.train()
        mets.append(ppo.update_minibatch(args, model, opt, copt, rec, dp).clone())
        clips.append(torch.cat([opt.total_norm, opt.clip_coef, copt.total_norm, copt.clip_coef]).clone())
        sch.step(), csch.step()
    torch.cuda.synchronize()
    clips = torch.stack(clips)
    assert float(clips[1, 1]) < 1.0 and float(clips[1, 3]) < 1.0, clips.tolist()        # the clip is active
    state = {n: p.detach().clone() for n, p in model.named_parameters() if p.numel() < 3_000_000}
    for tag, head, o in (("actor", model.actor, opt), ("critic", model.critic, copt)):
        w = head.out_layer.fc1.weight
        state[tag + ".fc1.sample"] = w.detach().view(-1)[::4099].clone()
        state[tag + ".fc1.sum"] = w.detach().double().sum().view(1)
        state[tag + ".fc1.m.sample"] = o.state[w]["exp_avg"].view(-1)[::4099].clone()
    state["metrics"], state["clips"] = torch.stack(mets), clips
    del model, reward, opt, copt
    torch.cuda.empty_cache()
    return state


def main():
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%s" % os.environ.get("MASTER_PORT", "29647"), rank=0, world_size=1)
    base = run(False, "0", dev)
    for streams in ("0", "1"):
        got = run(True, streams, dev)
        bad = [k for k in base if not torch.equal(base[k], got[k])]
        assert not bad, f"clipped step under the forced exchange (streams={streams}) differs from the plain clipped step in {bad[:6]}"
        print(f"CLIP_DP_BITEQUAL streams={streams}", flush=True)
    dist.destroy_process_group()
    print("CLIP_DP_OK", flush=True)


if __name__ == "__main__":
    main()
