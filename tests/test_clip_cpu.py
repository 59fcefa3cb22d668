"""Global gradient-norm clipping, the parts that need no GPU: the C ABI of csrc/clip.hip, AdamW.set_grad_clip's argument checks, the
refusal of Adafactor, and --max_grad_norm on every training launcher."""
import argparse
import ctypes
import os
import re

import pytest
import torch

from lr2ppo_amd import _native as native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"lr2_clip_sumsq": 4, "lr2_clip_gram_dot": 8, "lr2_clip_coef": 5, "lr2_adamw_multi_scaled": 9}


def test_header_signatures_sources_and_layout_agree():
    header = open(os.path.join(REPO, "include", "lr2ppo_hip.h")).read()
    src = open(os.path.join(native.CSRC, "clip.hip")).read()
    assert "clip.hip" in native.SOURCES
    lib = native.lib()
    for name, n_args in NEW.items():
        decl = re.search(r"^int %s\(([^;]*)\);" % name, header, flags=re.M | re.S)
        assert decl, name
        assert len(decl.group(1).split(",")) == n_args == len(native.SIGNATURES[name]), name
        assert re.search(r'extern "C" int %s\(' % name, src), name
        assert hasattr(lib, name)
    # lr2_adamw_multi keeps its signature; the scaled entry point is that plus one pointer in front of the stream
    assert native.SIGNATURES["lr2_adamw_multi_scaled"] == native.SIGNATURES["lr2_adamw_multi"][:-1] + [ctypes.c_void_p] * 2
    # the coefficient's pointer has a field of its own in lr2_epilogue, in what was padding: no size or offset moved
    assert "adam_gscale_dev" in header
    E = native.Epilogue
    assert E.adam_gscale_dev.offset == 96 and E.adam_gscale_dev.size == 8
    assert E.drop_site.offset == 92 and E.drop_seed.offset == 104 and E.adam_lr_dev.offset == 200 and ctypes.sizeof(E) == 208
    assert native.Epilogue().adam_gscale_dev is None


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = native.lib()
    A = 64                                                                   # any non-NULL, 8-byte aligned address: never dereferenced
    assert lib.lr2_clip_sumsq(None, 1, A, None) == -1 and lib.lr2_clip_sumsq(A, 0, A, None) == -1
    assert lib.lr2_clip_sumsq(A, 1, None, None) == -1 and lib.lr2_clip_sumsq(A, 1, A + 4, None) == -1
    g = lib.lr2_clip_gram_dot
    assert g(None, A, 4, 4, 4, 1.0, A, None) == -1 and g(A, None, 4, 4, 4, 1.0, A, None) == -1
    assert g(A, A, 0, 4, 4, 1.0, A, None) == -1 and g(A, A, 4, 3, 4, 1.0, A, None) == -1 and g(A, A, 4, 4, 3, 1.0, A, None) == -1
    assert g(A, A, 4, 4, 4, 1.0, None, None) == -1 and g(A, A, 4, 4, 4, 1.0, A + 4, None) == -1
    c = lib.lr2_clip_coef
    assert c(None, 1, 1.0, A, None) == -1 and c(A, 0, 1.0, A, None) == -1 and c(A, 1, 1.0, None, None) == -1
    assert c(A, 1, -1.0, A, None) == -1 and c(A, 1, float("nan"), A, None) == -1 and c(A + 4, 1, 1.0, A, None) == -1
    s = lib.lr2_adamw_multi_scaled
    assert s(None, 1, 1e-3, 0.9, 0.999, 1e-6, None, A, None) == -1 and s(A, 0, 1e-3, 0.9, 0.999, 1e-6, None, A, None) == -1
    assert s(A, 1, 1e-3, 0.9, 0.999, 1e-6, None, None, None) == -1
    # the fused step: a coefficient without adam_p, or together with the GELU' input whose slot it travels in, is refused
    e = native.Epilogue()
    e.out, e.ld_out, e.alpha, e.adam_gscale_dev = A, 128, 1.0, A
    assert lib.lr2_gemm(A, A, 128, 128, 64, 64, 64, 0, 0, 1 << 20, 1 << 20, 0, 0, 0, 0, ctypes.byref(e), None, 1, 128, 3, None) == -1


def test_set_grad_clip_argument_checks():
    from lr2ppo_amd.tencentpretrain.utils import optimizers as OPT
    lin = torch.nn.Linear(4, 3)
    opt = OPT.AdamW(lin.parameters(), lr=1e-3, correct_bias=False)
    assert opt.max_grad_norm is None and opt.total_norm is None and opt.clip_coef is None
    for bad in (-1.0, float("nan"), float("inf"), -0.5):
        with pytest.raises(ValueError, match="max_norm"):
            opt.set_grad_clip(bad)
    with pytest.raises((TypeError, ValueError)):
        opt.set_grad_clip("tight")
    opt.set_grad_clip(0.5)
    assert opt.max_grad_norm == 0.5
    opt.set_grad_clip(2)
    assert opt.max_grad_norm == 2.0 and isinstance(opt.max_grad_norm, float)
    for off in (None, 0, 0.0):
        opt.set_grad_clip(1.0)
        opt.set_grad_clip(off)
        assert opt.max_grad_norm is None
    assert "unscaled" in OPT.AdamW.set_grad_clip.__doc__.lower()
    assert not hasattr(OPT.Adafactor, "set_grad_clip")


def test_max_grad_norm_with_adafactor_is_a_value_error():
    from lr2ppo_amd.tencentpretrain.utils import optimizers as OPT
    from lr2ppo_amd.finetune import pointwise, pointwise_trad, ppo, reward_pair_dataloader
    lin = torch.nn.Linear(4, 3)
    ada = OPT.Adafactor(lin.parameters(), lr=1e-3, relative_step=False, scale_parameter=False)
    adam = OPT.AdamW(lin.parameters(), lr=1e-3, correct_bias=False)
    with pytest.raises(ValueError, match="invariant to the gradient's scale"):
        OPT.apply_grad_clip(argparse.Namespace(max_grad_norm=1.0), ada)
    with pytest.raises(ValueError, match="clips its own update"):
        OPT.apply_grad_clip(argparse.Namespace(max_grad_norm=1.0), adam, ada)
    assert adam.max_grad_norm is None                     # refused as a whole: nothing was switched on
    with pytest.raises(ValueError, match=">= 0"):
        OPT.apply_grad_clip(argparse.Namespace(max_grad_norm=-1.0), adam)
    OPT.apply_grad_clip(argparse.Namespace(max_grad_norm=0.0), ada)           # off: Adafactor runs as before
    OPT.apply_grad_clip(argparse.Namespace(), ada)                            # flag absent (programmatic callers)
    OPT.apply_grad_clip(argparse.Namespace(max_grad_norm=0.75), adam)
    assert adam.max_grad_norm == 0.75

    class ActorCritic(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.actor, self.critic = torch.nn.Linear(4, 3), torch.nn.Linear(4, 1)

    base = dict(scheduler="constant", learning_rate=1e-3, critic_learning_rate=1e-3, train_steps=10, warmup=0.1)
    for mod, model in ((pointwise, lin), (pointwise_trad, lin), (reward_pair_dataloader, lin), (ppo, ActorCritic())):
        with pytest.raises(ValueError, match="Adafactor"):
            mod.build_optimizer(argparse.Namespace(optimizer="adafactor", max_grad_norm=1.0, **base), model)
        out = mod.build_optimizer(argparse.Namespace(optimizer="adafactor", max_grad_norm=0.0, **base), model)
        assert isinstance(out[0], OPT.Adafactor)
        out = mod.build_optimizer(argparse.Namespace(optimizer="adamw", max_grad_norm=1.5, **base), model)
        opts = [o for o in out if isinstance(o, OPT.AdamW)]
        assert len(opts) == (2 if mod is ppo else 1) and all(o.max_grad_norm == 1.5 for o in opts)
        out = mod.build_optimizer(argparse.Namespace(optimizer="adamw", **base), model)
        assert all(o.max_grad_norm is None for o in out if isinstance(o, OPT.AdamW))


def test_flag_parses_on_every_training_launcher_with_default_zero():
    from lr2ppo_amd.finetune import pointwise, pointwise_trad, ppo, reward_pair_dataloader
    # ppo_trad / reward_trad / pointwise_2data_trad parse with ppo's / reward_pair_dataloader's / pointwise_trad's parser
    for mod in (ppo, pointwise, pointwise_trad, reward_pair_dataloader):
        parser = mod.build_parser()
        assert parser.parse_args([]).max_grad_norm == 0.0, mod.__name__
        got = parser.parse_args(["--max_grad_norm", "0.5"]).max_grad_norm
        assert got == 0.5 and isinstance(got, float), mod.__name__
    src = {m: open(os.path.join(REPO, "lr2ppo_amd", "finetune", m + ".py")).read() for m in ("ppo_trad", "reward_trad", "pointwise_2data_trad")}
    assert "ppo.build_parser()" in src["ppo_trad"] and "rp.build_parser()" in src["reward_trad"]
    # the tables of the reference's option groups stay the reference's
    assert "max_grad_norm" not in open(os.path.join(REPO, "lr2ppo_amd", "tencentpretrain", "opts.py")).read()
