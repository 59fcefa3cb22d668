"""Gradient-norm clipping outside the single-GPU PPO update: under the data-parallel exchange path (one RCCL rank, forced), through
encoder fine-tuning (finetune_pointwise_step: the head's optimizer and the encoders' each clip their own list) and in
pointwise_2data_trad, whose unused projection is neither stepped nor part of the norm."""
import argparse
import os
import subprocess
import sys

import pytest
import torch

from conftest import REPO

pytestmark = pytest.mark.gpu

REL22 = 2.0 ** -22


def _norm64(tensors):
    return float(sum(float(torch.linalg.vector_norm(t.detach().cpu(), 2, dtype=torch.float64)) ** 2 for t in tensors) ** 0.5)


def test_clipped_step_under_the_forced_exchange_is_the_plain_clipped_step(dev):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29647", HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, os.path.join(REPO, "tests", "workers", "clip_dp_worker.py")], env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "CLIP_DP_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-4000:]
    assert out.stdout.count("CLIP_DP_BITEQUAL") == 2


def test_encoder_finetuning_clips_head_and_encoders_separately(dev):
    """One layer per tower, finetune_pointwise_step with --max_grad_norm: the encoder optimizer's total_norm is the fp64 norm over
    fx.grad_flats() (gradients in memory stay unscaled), the head's the norm over its flat buffer (unfused route), both clips bite."""
    from lr2ppo_amd import runtime
    from lr2ppo_amd.finetune import ppo
    from lr2ppo_amd.finetune.features import (TEXT_CONFIG, VIT_CONFIG, FeatureExtractor, build_encoder_optimizer, encoder_args,
                                              finetune_pointwise_step, synthetic_raw_batch)
    args = argparse.Namespace(mode="reg", labels_num=3, seq_length=196, max_imgs=4, visual_feat_dim=768, is_master=True,
                              kl_div_loss_weight=0.001, entropy_weight=0.001, value_clip=0.5, optimizer="adamw", scheduler="linear",
                              learning_rate=1e-3, critic_learning_rate=1e-3, train_steps=41, warmup=0.1, device=dev,
                              max_grad_norm=1e-3)
    frames, ids, seg, tgts = (t.to(dev) for t in synthetic_raw_batch(1, 2, n_img=4, generator=torch.Generator().manual_seed(3)))
    fx = FeatureExtractor(encoder_args(VIT_CONFIG, layers_num=1), encoder_args(TEXT_CONFIG, layers_num=1))
    fx.init_normal(generator=torch.Generator().manual_seed(8))
    fx = fx.to(dev).train()
    with torch.device(dev):
        model = ppo.ActorCritic(args, None)
    torch.manual_seed(5)
    ppo._init_normal(model)
    model.train()
    opt, copt, sch, csch = ppo.build_optimizer(args, model)
    eopt, esch = build_encoder_optimizer(args, fx)
    assert opt.max_grad_norm == eopt.max_grad_norm == 1e-3
    sch.step(), csch.step(), esch.step()
    before = [p.detach().clone() for p in fx.parameters()]
    runtime.set_dropout_seed(31)
    loss = finetune_pointwise_step(args, fx, model.actor, opt, sch, eopt, esch, frames, ids, seg, tgts)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    for name, o, flats in (("encoders", eopt, fx.grad_flats()), ("head", opt, [model.actor._flat_grad])):
        want, got, coef = _norm64(flats), float(o.total_norm), float(o.clip_coef)
        print(f"{name}: total_norm {got:.9g}, fp64 {want:.9g}, coef {coef:.6g}")
        assert abs(got - want) <= REL22 * want, (name, got, want)
        assert 0.0 < coef < 1.0 and abs(coef - 1e-3 / (want + 1e-6)) <= 4 * REL22 * coef, (name, coef)
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, fx.parameters()))        # and the encoders trained


def test_pointwise_2data_trad_leaves_the_unused_projection_out_of_step_and_norm(dev):
    from lr2ppo_amd.finetune import pointwise_2data_trad as p2
    args = argparse.Namespace(mode="reg", labels_num=3, optimizer="adamw", scheduler="linear", learning_rate=1e-3, train_steps=21,
                              warmup=0.1, max_grad_norm=1e-2)
    model = p2.Classifier(args, None)
    torch.manual_seed(47)
    for n, p in model.named_parameters():
        if "gamma" not in n and "beta" not in n:
            p.data.normal_(0, 0.02)
    model = model.to(dev).train()
    opt, sch = p2.build_optimizer(args, model)
    assert opt.max_grad_norm == 1e-2
    sch.step()
    gen = torch.Generator().manual_seed(9)
    for width, unused in ((136, "text_proj."), (46, "text_proj3."), (136, "text_proj.")):
        feats, tgts = torch.randn(2, 5, width, generator=gen).to(dev), torch.randint(0, 3, (2, 5), generator=gen).to(dev)
        frozen = {n: p.detach().clone() for n, p in model.named_parameters() if n.startswith(unused)}
        for n, g in model.grad_buffers().items():          # whatever lies in the unused projection's buffers must not count
            if n.startswith(unused):
                g.fill_(1e3)
        p2.train_model(args, model, opt, sch, feats, None, tgts)
        torch.cuda.synchronize()
        used = [p.grad for n, p in model.named_parameters() if not n.startswith(unused)]
        assert len(frozen) == 4 and all(g is not None for g in used)
        for n, p in model.named_parameters():
            if n.startswith(unused):
                assert p.grad is None and torch.equal(p.detach(), frozen[n]), n
        want, got, coef = _norm64(used), float(opt.total_norm), float(opt.clip_coef)
        assert abs(got - want) <= REL22 * want and got < 100.0, (width, got, want)
        assert 0.0 < coef < 1.0, (width, coef)
