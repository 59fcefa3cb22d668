"""Global gradient-norm clipping through the full PPO heads (batch 4 x 2 tags, max_imgs 1 and 16, modes 'reg' and 'cls'): off means
the plain step bit for bit; the plain (materialised) route against an fp64 norm on the CPU and against torch pre-scaling the
gradients; the fused route -- the norm of out_layer.fc1's never-written gradient from its factors' Gram matrices -- against both; and
the captured step against the eager one.

One model pair per configuration is built on the device and reset to the same initial weights before every run; a run is one
ppo.update_minibatch on a fixed hand-made rollout record (no reward model needed) from the same dropout seed."""
import argparse
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

BS, TAGS = 4, 2
REL22 = 2.0 ** -22
# Fused route, measured on MI355X with fused_route_figures below over 8 record seeds (1000 .. 1007) x max_imgs {1, 16}, mode 'reg'
# (DESIGN.md 4.8): worst relative distance of total_norm from the fp64 norm of the materialised gradients 6.38e-6 (max_imgs 16;
# 1.43e-6 at max_imgs 1 -- the split-bf16 x 3 Gram products leave out the lo x lo terms, a bias that grows with the factors' width);
# of the step from the plain clipped route's, relative L2: parameter deltas 3.10e-6, out_layer.fc1's exp_avg 6.40e-6.  The plain
# route's own total_norm was within 5.8e-8.  Bounds = 8 x the worst measured value (conditioning varies with the data); the norm's
# may not pass 1e-4, where the coefficient would differ visibly from torch's.
FUSED_NORM_BOUND = 8 * 6.38e-6
FUSED_DELTA_BOUND = 8 * 3.10e-6
FUSED_EXP_AVG_BOUND = 8 * 6.40e-6
assert FUSED_NORM_BOUND <= 1e-4


def _args(dev, mode, max_imgs, **kw):
    return argparse.Namespace(mode=mode, labels_num=3, seq_length=196, max_imgs=max_imgs, visual_feat_dim=768, is_master=True,
                              kl_div_loss_weight=0.001, entropy_weight=0.001, value_clip=0.5, optimizer="adamw",
                              scheduler="linear", learning_rate=1e-3, critic_learning_rate=1e-3, train_steps=41, warmup=0.1,
                              device=dev, **kw)


def make_record(dev, max_imgs, seed):
    gen = torch.Generator().manual_seed(seed)
    text, img = torch.randn(BS, TAGS, 196, 768, generator=gen), torch.randn(BS, max_imgs, 768, generator=gen)
    tgts = torch.randint(0, 3, (BS, TAGS), generator=gen)
    state = torch.arange(TAGS).unsqueeze(0).repeat(BS, 1)
    order = torch.stack([torch.randperm(TAGS, generator=gen) for _ in range(BS)])
    next_state = torch.cat([torch.arange(2).unsqueeze(0).repeat(BS, 1), torch.gather(state, 1, order)], dim=1)
    old_scores, rewards, old_value = torch.rand(BS, TAGS, generator=gen) * 2, torch.randn(BS, generator=gen), torch.randn(BS, generator=gen)
    return [t.to(dev) for t in (state, next_state, old_scores, rewards, old_value, text, img, tgts)]


def _counts():
    from lr2ppo_amd import _native, ops
    c = (ctypes.c_uint64 * 3)()
    assert _native.lib().lr2_gemm_launch_counts(c) == 0
    return tuple(int(x) for x in c), ops.adafactor_launch_counts()


class Rig:
    """ActorCritic of one configuration on the device + its initial weights; run() = reset, fresh optimizers, one update."""

    def __init__(self, dev, mode, max_imgs):
        from lr2ppo_amd.finetune import ppo
        self.dev, self.mode, self.max_imgs = dev, mode, max_imgs
        with torch.device(dev):
            self.model = ppo.ActorCritic(_args(dev, mode, max_imgs), None)
        torch.manual_seed(5)
        ppo._init_normal(self.model)
        self.init = [p.detach().clone() for p in self.model.parameters()]
        self.model.train()

    def run(self, record, *, fuse=True, flag="absent", clip=None, prescale=None, steps=1):
        from lr2ppo_amd import runtime
        from lr2ppo_amd.finetune import ppo
        kw = {} if flag == "absent" else {"max_grad_norm": flag}
        args = _args(self.dev, self.mode, self.max_imgs, fuse_fc1_update=fuse, **kw)
        with torch.no_grad():
            for p, q in zip(self.model.parameters(), self.init):
                p.copy_(q)
        opt, copt, sch, csch = ppo.build_optimizer(args, self.model)
        self.model.actor.bind_grads(), self.model.critic.bind_grads()
        for _ in range(3):                  # leave the lr-0 first cycle
            sch.step(), csch.step()
        if clip is not None:
            opt.set_grad_clip(clip[0]), copt.set_grad_clip(clip[1])
        if prescale is not None:            # an unclipped step fed gradients that torch multiplied by the coefficient
            for o, head, c in ((opt, self.model.actor, prescale[0]), (copt, self.model.critic, prescale[1])):
                def step(real=o.step, head=head, c=c):
                    head._flat_grad.mul_(c)
                    return real()
                o.step = step
        runtime.set_dropout_seed(99)
        before = _counts()
        for _ in range(steps):
            metrics = ppo.update_minibatch(args, self.model, opt, copt, record)
        torch.cuda.synchronize()
        after = _counts()
        out = dict(metrics=metrics.clone(), opt=opt, copt=copt,
                   gemm=tuple(a - b for a, b in zip(after[0], before[0])), adafactor=tuple(a - b for a, b in zip(after[1], before[1])))
        if opt.max_grad_norm is not None:
            out["norm"] = (float(opt.total_norm), float(copt.total_norm))
            out["coef"] = (opt.clip_coef.clone(), copt.clip_coef.clone())
        return out

    def weights(self):
        return [p.detach().clone() for p in self.model.parameters()]

    def moments(self, out):
        return [out[k].state[p][s].clone() for k in ("opt", "copt") for g in out[k].param_groups for p in g["params"]
                for s in ("exp_avg", "exp_avg_sq")]

    def cpu_norms(self):
        """fp64 norms of the materialised gradients (plain route: every gradient sits in the flat buffers), on the CPU."""
        return tuple(float(torch.linalg.vector_norm(h._flat_grad.cpu(), 2, dtype=torch.float64)) for h in (self.model.actor, self.model.critic))


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def rel_l2(a, b):
    """||a - b|| / ||b|| over lists of tensors, in fp64."""
    num = sum(float((x.double() - y.double()).pow(2).sum()) for x, y in zip(a, b))
    den = sum(float(y.double().pow(2).sum()) for y in b)
    return (num / den) ** 0.5


def fused_route_figures(rig, record):
    """One configuration and record -> the figures the plain-route and fused-route checks assert on (and the bounds above were measured with)."""
    fc1 = [rig.model.actor.out_layer.fc1.weight, rig.model.critic.out_layer.fc1.weight]
    rig.run(record, fuse=False)
    ref = rig.cpu_norms()
    clip = (0.25 * ref[0], 0.25 * ref[1])
    plain = rig.run(record, fuse=False, clip=clip)
    w_plain = rig.weights()
    m_plain = [plain[k].state[p]["exp_avg"].clone() for k, p in zip(("opt", "copt"), fc1)]
    fused = rig.run(record, fuse=True, clip=clip)
    w_fused = rig.weights()
    m_fused = [fused[k].state[p]["exp_avg"] for k, p in zip(("opt", "copt"), fc1)]
    d_plain = [w - i for w, i in zip(w_plain, rig.init)]
    d_fused = [w - i for w, i in zip(w_fused, rig.init)]
    return dict(ref=ref, clip=clip, plain=plain, fused=fused, w_plain=w_plain,
                norm_err_plain=max(abs(n - r) / r for n, r in zip(plain["norm"], ref)),
                norm_err_fused=max(abs(n - r) / r for n, r in zip(fused["norm"], ref)),
                delta_err=rel_l2(d_fused, d_plain), exp_avg_err=rel_l2(m_fused, m_plain))


@pytest.fixture(scope="module", params=[(1, "reg"), (1, "cls"), (16, "reg"), (16, "cls")], ids=lambda p: f"imgs{p[0]}-{p[1]}")
def rig(request, dev):
    r = Rig(dev, request.param[1], request.param[0])
    yield r
    del r
    torch.cuda.empty_cache()


def test_off_is_the_plain_step_bit_for_bit(rig):
    """Flag absent, 0, or max_norm = 1e9 (on, never active): weights, moments and metrics of the plain step on both routes.  The launch
    counters: flag absent / 0 launch what the plain step launches; 1e9 launches no further GEMM on the plain route and exactly the
    two Gram products per model on the fused route; no Adafactor launch anywhere."""
    record = make_record(rig.dev, rig.max_imgs, 23)
    for fuse in (True, False):
        base = rig.run(record, fuse=fuse)
        w, m = rig.weights(), rig.moments(base)
        assert base["opt"].max_grad_norm is None and base["adafactor"] == (0, 0)
        for flag in (0.0, 1e9):
            got = rig.run(record, fuse=fuse, flag=flag)
            assert (got["opt"].max_grad_norm, got["copt"].max_grad_norm) == ((None, None) if flag == 0.0 else (1e9, 1e9))
            assert torch.equal(got["metrics"], base["metrics"]), (fuse, flag)
            assert _same(rig.weights(), w) and _same(rig.moments(got), m), (fuse, flag)
            extra = tuple(a - b for a, b in zip(got["gemm"], base["gemm"]))
            assert got["adafactor"] == (0, 0)
            assert sum(extra) == (4 if (flag and fuse) else 0) and extra[1] == 0, (fuse, flag, extra)
            if flag:
                assert float(got["coef"][0]) == 1.0 and float(got["coef"][1]) == 1.0
        del w, m, base


def test_plain_and_fused_routes_clip_like_torch(rig):
    record = make_record(rig.dev, rig.max_imgs, 23)
    f = fused_route_figures(rig, record)
    print(f"max_imgs {rig.max_imgs} {rig.mode}: fp64 norms {f['ref']}; total_norm rel. error plain {f['norm_err_plain']:.3e}, fused "
          f"{f['norm_err_fused']:.3e}; fused vs plain step: deltas {f['delta_err']:.3e}, fc1 exp_avg {f['exp_avg_err']:.3e}")
    # route 2 (plain): the clip is active, the norm is the fp64 norm, the step is torch's pre-scaled one
    for out in (f["plain"], f["fused"]):
        assert all(0.0 < float(c) < 1.0 for c in out["coef"])
    assert f["norm_err_plain"] <= REL22
    pre = rig.run(record, fuse=False, prescale=f["plain"]["coef"])
    assert pre["opt"].max_grad_norm is None and _same(rig.weights(), f["w_plain"])
    assert torch.equal(pre["metrics"], f["plain"]["metrics"])
    # route 3 (fused): the same norm from the factors, the same step
    assert f["norm_err_fused"] <= FUSED_NORM_BOUND
    assert f["delta_err"] <= FUSED_DELTA_BOUND and f["exp_avg_err"] <= FUSED_EXP_AVG_BOUND
    assert sum(f["fused"]["gemm"]) - sum(f["plain"]["gemm"]) == 4              # the two Gram products per model, nothing else


def test_graphed_step_with_clipping_equals_the_eager_clipped_step(dev):
    """GraphedPPOStep captures norm, coefficient and scaled updates as they stand: bits of the eager clipped step over 4 batches
    while the scheduler moves."""
    from lr2ppo_amd import runtime
    from lr2ppo_amd.finetune import ppo
    args = _args(dev, "cls", 16, max_grad_norm=0.02)

    def build(src=None):
        with torch.device(dev):
            model, reward = ppo.ActorCritic(args, None), ppo.Reward(args, None)
        if src is None:
            torch.manual_seed(5)
            ppo._init_normal(model), ppo._init_normal(reward)
        else:
            model.load_state_dict(src[0].state_dict()), reward.load_state_dict(src[1].state_dict())
        reward.eval()
        opt, copt, sch, csch = ppo.build_optimizer(args, model)
        model.actor.bind_grads(), model.critic.bind_grads()
        for _ in range(3):
            sch.step(), csch.step()
        return model, reward, opt, copt, sch, csch

    A = build()
    B = build(A)
    gen = torch.Generator().manual_seed(23)
    batches = [(torch.randn(BS, TAGS, 196, 768, generator=gen).to(dev), torch.randn(BS, 16, 768, generator=gen).to(dev),
                torch.randint(0, 3, (BS, TAGS), generator=gen).to(dev)) for _ in range(4)]
    runtime.set_dropout_seed(99)
    model, reward, opt, copt, sch, csch = A
    ref, coefs = [], []
    for b in batches:
        model.eval()
        rec = ppo.rollout_step(model, reward, *b)
        model.train()
        ref.append(ppo.update_minibatch(args, model, opt, copt, rec).clone())
        coefs.append((float(opt.clip_coef), float(copt.clip_coef), float(opt.total_norm), float(copt.total_norm)))
        sch.step(), csch.step()
    # the critic's clip bites in every step, the actor's in some: an update right after its rollout starts at probability ratio 1,
    # and on some batches the actor's gradient is ~1e-5, where no clip can bite
    assert all(0.0 < c[1] < 1.0 for c in coefs) and any(0.0 < c[0] < 1.0 for c in coefs) and all(0.0 < c[0] <= 1.0 for c in coefs), coefs
    runtime.set_dropout_seed(99)
    model, reward, opt, copt, sch, csch = B
    step = ppo.GraphedPPOStep(args, model, reward, opt, copt)
    for i, b in enumerate(batches):
        got = step(*b).clone()
        assert torch.equal(got, ref[i]), f"metrics of step {i} differ"
        assert (float(opt.clip_coef), float(copt.clip_coef), float(opt.total_norm), float(copt.total_norm)) == coefs[i], i
        sch.step(), csch.step()
    assert step.graph is not None
    for (n, p), (_, q) in zip(B[0].named_parameters(), A[0].named_parameters()):
        assert torch.equal(p, q), f"parameter {n} differs after 4 steps"
    step.release()
