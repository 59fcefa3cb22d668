"""The heads at more than 16 image tokens (--max_imgs 17 .. 64, served by the wide XiT cross-attention pair of csrc/attn_wide.hip) on a
real MI355X: Actor and Critic against the CPU oracle at max_imgs = 32 (per-tag and shared image tokens) and 17, one rollout +
update_minibatch at 32 with the size-independent properties of test_head_gpu.py::test_full_batch_properties, the captured step, the
stage-1 / stage-2 Classifiers, and a stage-3 launcher started WITHOUT --max_imgs (the parser's default, 32).

Bars: those test_head_gpu.py applies to the same quantities at 16 -- logits / values 1e-4 (TOL), parameter gradients
1e-7 + 2e-3 max |ref| -- and, for the input gradients, the 2e-3 relative norm of test_ppo_finetune_gpu.py.  out_layer.fc1.weight
((196 + max_imgs) * 768 columns) is compared on sampled rows, whole rows, so the columns of every image token are in."""
import argparse
import copy
import json
import os
import subprocess
import sys

import pytest
import torch

from oracle import lr2ppo_oracle as O

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4            # test_head_gpu.py
REL = 2e-3            # test_ppo_finetune_gpu.py: relative norm of the input gradients
FC1_ROWS = (0, 1, 777, 1536, 3070, 3071)
CHECK = ["text_proj.fc1.weight", "text_proj.fc2.bias", "img_proj.fc2.weight", "out_layer.fc1.bias", "out_layer.fc2.weight", "head.weight",
         "head.bias"]


def _ns(max_imgs, **kw):
    return argparse.Namespace(mode="reg", labels_num=3, seq_length=196, max_imgs=max_imgs, visual_feat_dim=768, **kw)


def _train_args(max_imgs, dev):
    return _ns(max_imgs, is_master=False, kl_div_loss_weight=0.001, entropy_weight=0.001, value_clip=0.5, optimizer="adamw",
               scheduler="linear", learning_rate=1e-3, critic_learning_rate=1e-3, train_steps=100, warmup=0.1, device=dev)


def _maxerr(a, b):
    return (a.detach().double().cpu() - b.detach().double().cpu()).abs().max().item()


def _rel(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _check_grads(G, Pg, names, who):
    for n in names:
        ref_g = Pg[n].grad
        err = _maxerr(G[n], ref_g)
        assert err < 1e-7 + 2e-3 * float(ref_g.abs().max()), f"{who} grad {n}: err {err} scale {float(ref_g.abs().max())}"
    rows = torch.tensor(FC1_ROWS)
    ref_g = Pg["out_layer.fc1.weight"].grad[rows]
    err = _maxerr(G["out_layer.fc1.weight"][rows.to(G["out_layer.fc1.weight"].device)], ref_g)
    assert float(ref_g[:, 196 * 768:].abs().max()) > 0            # the image tokens' columns carry gradient
    assert err < 1e-7 + 2e-3 * float(ref_g.abs().max()), f"{who} grad out_layer.fc1.weight rows: err {err}"


def _device_init(module, dev, seed):
    """normal_(0, 0.02) on the device (the reference's initialiser; half a billion normals take seconds on the host)."""
    module = module.to(dev)
    g = torch.Generator(device=dev).manual_seed(seed)
    with torch.no_grad():
        for p in module.parameters():
            p.normal_(0, 0.02, generator=g)
    return module


def _inputs(seed, bs, tags, max_imgs, layout):
    """text [bs, tags, 196, 768]; img as the head gets it (per_tag: [bs, tags, n, 768], shared: [bs, n, 768]); oracle_img(leaf) -> the
    [bs, tags, n, 768] the oracle takes."""
    text, img4, _ = O.seeded_head_inputs(seed, bs, tags, n_img=max_imgs)
    if layout == "shared":
        return text, img4[:, 0].contiguous(), lambda leaf: leaf.unsqueeze(1).repeat(1, tags, 1, 1)
    return text, img4, lambda leaf: leaf


CASES = [(32, 2, "per_tag"), (32, 2, "shared"), (17, 1, "per_tag")]


@pytest.mark.parametrize("max_imgs, bs, layout", CASES, ids=[f"imgs{m}-bs{b}-{l}" for m, b, l in CASES])
def test_actor_matches_oracle(dev, max_imgs, bs, layout):
    """Eval forward, then train-mode forward + backward (dropout 0.1, pinned seed) with input gradients, against the oracle's forward
    and autograd: logits, every XiT parameter gradient, sampled rows of out_layer.fc1.weight, d text_emb and d img_emb."""
    from lr2ppo_amd import ops, runtime
    from lr2ppo_amd.finetune import ppo
    tags = 2
    text, img, oracle_img = _inputs(155 + max_imgs, bs, tags, max_imgs, layout)
    wlog = torch.randn(bs * tags, generator=torch.Generator().manual_seed(56))
    P = O.seeded_params(O.head_param_spec("actor", max_imgs=max_imgs), seed=7)
    actor = ppo.Actor(_ns(max_imgs), None)
    actor.load_state_dict(P, strict=True)
    actor = actor.to(dev).eval()
    before = ops.xattn_wide_launch_counts()
    with torch.no_grad():
        ev = actor(text.to(dev), img.to(dev), None)
        ref_ev = O.actor_forward(P, text, oracle_img(img), None)
    assert ops.xattn_wide_launch_counts()[0] == before[0] + 1          # the wide forward served it
    assert _maxerr(ev, ref_ev) < TOL
    actor.train()
    runtime.set_dropout_seed(2024, calls=5)
    seed = runtime.peek_drop_seed()
    logits = actor.engine_forward(text.to(dev), img.to(dev), save=True)
    d_text, d_img = actor.engine_backward(wlog.to(dev), input_grads=True)
    assert ops.xattn_wide_launch_counts() == (before[0] + 2, before[1] + 1)
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    tl, il = text.clone().requires_grad_(True), img.clone().requires_grad_(True)
    ref_logits = O.actor_forward(Pg, tl, oracle_img(il), None, drop={"p": 0.1, "seed": seed, "site_base": 0})
    (ref_logits * wlog).sum().backward()
    assert _maxerr(logits, ref_logits) < TOL
    _check_grads(actor.grad_buffers(), Pg, CHECK + [n for n in P if n.startswith("xit.")], "actor")
    assert d_text.shape == text.shape and d_img.shape == img.shape
    assert _rel(d_text, tl.grad) < REL, _rel(d_text, tl.grad)
    assert _rel(d_img, il.grad) < REL, _rel(d_img, il.grad)
    # the same step without input gradients: the parameter gradients meet the same bars
    runtime.set_dropout_seed(2024, calls=5)
    actor.engine_forward(text.to(dev), img.to(dev), save=True)
    actor.engine_backward(wlog.to(dev))
    _check_grads(actor.grad_buffers(), Pg, CHECK + [n for n in P if n.startswith("xit.")], "actor (no input gradients)")


@pytest.mark.parametrize("max_imgs, bs", [(32, 2), (17, 1)], ids=["imgs32-bs2", "imgs17-bs1"])
def test_critic_matches_oracle(dev, max_imgs, bs):
    """Critic (trunk + pos_emb + xitt + last-position head) with a non-identity index: eval value, then train-mode value, parameter
    gradients of both XiT blocks and the input gradients against the oracle."""
    from lr2ppo_amd import runtime
    from lr2ppo_amd.finetune import ppo
    tags = 2
    text, img, _ = _inputs(255 + max_imgs, bs, tags, max_imgs, "per_tag")
    wval = torch.randn(bs, generator=torch.Generator().manual_seed(57))
    index = torch.tensor([[1, 0], [0, 1]])[:bs]
    P = O.seeded_params(O.head_param_spec("critic", max_imgs=max_imgs), seed=8)
    critic = ppo.Critic(_ns(max_imgs), None)
    critic.load_state_dict(P, strict=True)
    critic = critic.to(dev).eval()
    with torch.no_grad():
        ev = critic.engine_forward(text.to(dev), img.to(dev), index.to(dev), save=False)
        assert _maxerr(ev, O.critic_forward(P, text, img, index)) < TOL
    critic.train()
    runtime.set_dropout_seed(2025, calls=1)
    seed = runtime.peek_drop_seed()
    value = critic.engine_forward(text.to(dev), img.to(dev), index.to(dev), save=True)
    d_text, d_img = critic.engine_backward(wval.to(dev), input_grads=True)
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    tl, il = text.clone().requires_grad_(True), img.clone().requires_grad_(True)
    ref_v = O.critic_forward(Pg, tl, il, index, drop={"p": 0.1, "seed": seed, "site_base": 0})
    (ref_v * wval).sum().backward()
    assert _maxerr(value, ref_v) < TOL
    _check_grads(critic.grad_buffers(), Pg, CHECK + ["pos_emb.weight"] + [n for n in P if n.startswith(("xit.", "xitt."))], "critic")
    assert _rel(d_text, tl.grad) < REL, _rel(d_text, tl.grad)
    assert _rel(d_img, il.grad) < REL, _rel(d_img, il.grad)


def test_reward_and_stage2_classifier_run_at_32(dev):
    """Reward (4 fixed positions) against the oracle at max_imgs = 32; the stage-2 Classifier is the Reward: from the same weights it
    gives the same bits."""
    from lr2ppo_amd.finetune import ppo, reward_pair_dataloader
    bs, tags, max_imgs = 2, 2, 32
    text, img, tgts = O.seeded_head_inputs(355, bs, tags, n_img=max_imgs)
    index = torch.tensor([[0, 1, 1, 0], [1, 0, 0, 1]])
    P = O.seeded_params(O.head_param_spec("reward", max_imgs=max_imgs), seed=9)
    reward = ppo.Reward(_ns(max_imgs), None)
    reward.load_state_dict(P, strict=True)
    reward = reward.to(dev).eval()
    with torch.no_grad():
        r = reward(text.to(dev), img.to(dev), tgts.to(dev), index.to(dev))
        assert _maxerr(r, O.reward_forward(P, text, img, index)) < TOL
        s2 = reward_pair_dataloader.Classifier(_ns(max_imgs), None)
        s2.load_state_dict(P, strict=True)
        assert torch.equal(s2.to(dev).eval()(text.to(dev), img.to(dev), tgts.to(dev), index.to(dev)), r)


def test_stage1_classifier_runs_at_32(dev):
    """The stage-1 Classifier (the Actor with targets) at max_imgs = 32: SmoothL1 loss and logits against the oracle."""
    from lr2ppo_amd.finetune import pointwise
    bs, tags, max_imgs = 2, 2, 32
    text, img, tgts = O.seeded_head_inputs(356, bs, tags, n_img=max_imgs)
    with torch.no_grad():
        s1 = _device_init(pointwise.Classifier(_ns(max_imgs), None), dev, 11).eval()
        loss, logits = s1(text.to(dev), img.to(dev), tgts.to(dev))
        Pa = {k: v.detach().cpu() for k, v in s1.state_dict().items()}
        ref_loss, ref_logits = O.actor_forward(Pa, text, img, tgts)
        assert _maxerr(logits, ref_logits) < TOL and abs(float(loss) - float(ref_loss)) < TOL


def test_rollout_update_and_captured_step_at_32(dev, monkeypatch):
    """One rollout + update_minibatch at max_imgs = 32, bs 2, with the property checks of test_full_batch_properties: (1) the same
    rollout twice gives the same bits; (2) permuting the items permutes the record; (3) an update at lr = 0 leaves every weight; (4)
    the fused and the separate out_layer.fc1 update (K = (196 + 32) * 768) agree bit for bit; (5) so do the multi-stream and the
    single-stream schedule; and (6) the step captured in a HIP graph (GraphedPPOStep) gives the eager step's metrics bit for bit."""
    from lr2ppo_amd import runtime
    from lr2ppo_amd.finetune import ppo
    bs, tags, max_imgs = 2, 2, 32
    args = _train_args(max_imgs, dev)
    model, reward = _device_init(ppo.ActorCritic(args, None), dev, 3).eval(), _device_init(ppo.Reward(args, None), dev, 5).eval()
    g = torch.Generator().manual_seed(4)
    text = torch.randn(bs, tags, 196, 768, generator=g).to(dev)
    img = torch.randn(bs, max_imgs, 768, generator=g).to(dev)
    tgts = torch.randint(0, 3, (bs, tags), generator=g).to(dev)
    rec = ppo.rollout_step(model, reward, text, img, tgts)
    rec2 = ppo.rollout_step(model, reward, text, img, tgts)
    for a, b in zip(rec[1:5], rec2[1:5]):
        assert torch.equal(a, b)                                           # (1)
    monkeypatch.setenv("LR2_PPO_STREAMS", "0")
    rec1s = ppo.rollout_step(model, reward, text, img, tgts)
    monkeypatch.delenv("LR2_PPO_STREAMS")
    for a, b in zip(rec[1:5], rec1s[1:5]):
        assert torch.equal(a, b)                                           # (5) rollout
    perm = torch.tensor([1, 0], device=dev)
    recp = ppo.rollout_step(model, reward, text[perm].contiguous(), img[perm].contiguous(), tgts[perm].contiguous())
    for a, b in zip(rec[1:5], recp[1:5]):
        assert torch.equal(a[perm], b)                                     # (2)
    opt, copt, sch, csch = ppo.build_optimizer(args, model)                # LambdaLR: lr = 0 until the first scheduler.step()
    before = {n: p.detach().clone() for n, p in model.named_parameters() if "fc1.weight" not in n or "out_layer" not in n}
    probe = model.actor.out_layer.fc1.weight[:8, -256:].clone()            # columns of the last image token
    model.train()
    out = ppo.train_model(args, model, opt, copt, sch, csch, [rec], 1)
    assert all(v == v and abs(v) < 1e6 for v in out)
    for n, p in model.named_parameters():
        if n in before:
            assert torch.equal(p.detach(), before[n]), n                   # (3)
    assert torch.equal(probe, model.actor.out_layer.fc1.weight[:8, -256:])
    state = copy.deepcopy({"m": model.state_dict(), "o": opt.state_dict(), "c": copt.state_dict()})

    def restore():
        model.load_state_dict(state["m"])
        opt.load_state_dict(copy.deepcopy(state["o"])), copt.load_state_dict(copy.deepcopy(state["c"]))

    results = []
    for fuse, streams in ((True, "1"), (False, "1"), (True, "0")):
        restore()
        args.fuse_fc1_update = fuse
        monkeypatch.setenv("LR2_PPO_STREAMS", streams)
        runtime.set_dropout_seed(77)
        metrics = ppo.update_minibatch(args, model, opt, copt, rec)
        results.append((model.actor.out_layer.fc1.weight[:64, -512:].clone(), model.critic.out_layer.fc1.weight[-64:, -512:].clone(),
                        model.actor.head.weight.clone(), model.critic.head.weight.clone(), metrics.clone()))
    monkeypatch.delenv("LR2_PPO_STREAMS")
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert torch.equal(a, b)                                       # (4), (5) update
    assert not torch.equal(results[0][0][:8, -256:], probe)                 # and the step did move the image tokens' columns
    # (6) eager steps, then the same steps through GraphedPPOStep (call 1 eager, call 2 captures, call 3 replays)
    args.fuse_fc1_update = True

    def eager():
        model.eval()
        r = ppo.rollout_step(model, reward, text, img, tgts)
        model.train()
        return ppo.update_minibatch(args, model, opt, copt, r).clone()

    restore()
    runtime.set_dropout_seed(99)
    ref = [eager() for _ in range(3)]
    w_ref = model.actor.out_layer.fc1.weight[:64, -512:].clone()
    restore()
    runtime.set_dropout_seed(99)
    model.actor.bind_grads(), model.critic.bind_grads()
    step = ppo.GraphedPPOStep(args, model, reward, opt, copt)
    got = [step(text, img, tgts).clone() for _ in range(3)]
    torch.cuda.synchronize()
    assert step.graph is not None
    for i, (x, y) in enumerate(zip(got, ref)):
        assert torch.equal(x, y), f"metrics of step {i} differ: {x.tolist()} vs {y.tolist()}"
    assert torch.equal(model.actor.out_layer.fc1.weight[:64, -512:], w_ref)
    step.release()


def test_stage3_launcher_without_max_imgs(dev, tmp_path):
    """`python -m lr2ppo_amd.finetune.ppo` on synthetic items with no --max_imgs: the parser's default (32, the reference's) applies,
    one update cycle runs and the validation reaches its NDCG line."""
    from lr2ppo_amd.finetune import ppo
    assert ppo.build_parser().get_default("max_imgs") == 32
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps({"emb_size": 768, "hidden_size": 768}))
    out = tmp_path / "model.bin"
    cmd = [sys.executable, "-m", "lr2ppo_amd.finetune.ppo", "--config_path", str(cfg), "--output_model_path", str(out),
           "--synthetic_items", "2", "--synthetic_val_items", "1", "--batch_size", "2", "--seq_length", "196", "--visual_feat_dim", "768",
           "--learning_rate", "1e-4", "--mode", "reg", "--max_cycles", "1", "--max_timesteps", "1", "--update_timesteps", "1",
           "--epochs_num", "2"]
    assert "--max_imgs" not in cmd
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONPATH=REPO))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    log = r.stdout + r.stderr
    assert "NDCG@3=" in log, log[-3000:]
