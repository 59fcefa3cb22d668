"""The CPU half of the Adafactor suite (test_adafactor_gpu.py): registries against the parsers, the eight schedules against the
reference's recorded tables (tests/golden/sched_all.json), the constructor contract, the seven launchers' build_optimizer, the C ABI
(still 27; names in the header, SIGNATURES, INTEGRATION.md, SOURCES) and the tile / workspace plan against a brute-force count."""
import argparse
import ctypes
import json
import os
import re

import pytest
import torch

from conftest import GOLD, REPO

from lr2ppo_amd import _native as native
from lr2ppo_amd.tencentpretrain import opts
from lr2ppo_amd.tencentpretrain.utils import optimizers as OPT

NEW_SYMBOLS = ("lr2_adafactor_multi", "lr2_adafactor_launch_counts")


def _choices(flag):
    p = argparse.ArgumentParser()
    opts.optimization_opts(p)
    return next(a.choices for a in p._actions if flag in a.option_strings)


def test_registries_carry_every_parser_choice():
    assert set(_choices("--optimizer")) == set(OPT.str2optimizer) == {"adamw", "adafactor"}
    assert set(_choices("--scheduler")) == set(OPT.str2scheduler) == {
        "linear", "cosine", "cosine_with_restarts", "polynomial", "constant", "constant_with_warmup", "inverse_sqrt", "tri_stage"}
    assert OPT.str2optimizer["adafactor"] is OPT.Adafactor


def test_schedule_tables_match_the_reference():
    with open(os.path.join(GOLD, "sched_all.json")) as f:
        s = json.load(f)
    T, w, d = s["train_steps"], s["warmup"], s["decay"]
    assert set(s["lrs"]) == set(OPT.str2scheduler)
    for name, want in s["lrs"].items():
        o = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=s["base_lr"])
        fn = OPT.str2scheduler[name]
        if name == "constant":
            sch = fn(o)
        elif name == "constant_with_warmup":
            sch = fn(o, T * w)
        elif name == "tri_stage":                      # trainer.py:585-586
            sch = fn(o, T * w, T * d, T)
        else:
            sch = fn(o, T * w, T)
        got = [o.param_groups[0]["lr"]]
        for _ in range(len(want) - 1):
            o.step()
            sch.step()
            got.append(o.param_groups[0]["lr"])
        assert len(got) == len(want) >= T + 1
        assert max(abs(a - b) for a, b in zip(got, want)) <= 1e-12, name


def test_constructor_contract():
    p = [torch.nn.Parameter(torch.zeros(3, 4))]
    with pytest.raises(ValueError, match="Cannot combine manual lr and relative_step"):
        OPT.Adafactor(p, lr=1e-3)
    with pytest.raises(ValueError, match="warmup_init requires relative_step=True"):
        OPT.Adafactor(p, lr=None, relative_step=False, warmup_init=True)
    for kw in (dict(lr=None), dict(lr=1e-3, relative_step=False), dict(lr=1e-3, relative_step=False, scale_parameter=False, beta1=0.9),
               dict(lr=None, relative_step=False, scale_parameter=False)):
        with pytest.raises(NotImplementedError, match="relative_step=False"):
            OPT.Adafactor(p, **kw)
    for bad in ((2, 3, 4), (768, 3, 16, 16), ()):
        with pytest.raises(NotImplementedError, match="1-D and 2-D"):
            OPT.Adafactor([torch.nn.Parameter(torch.zeros(bad))], lr=1e-3, relative_step=False, scale_parameter=False)
    o = OPT.Adafactor(p, lr=1e-3, relative_step=False, scale_parameter=False)
    d = o.defaults
    assert d["eps"] == (1e-30, 1e-3) and d["clip_threshold"] == 1.0 and d["decay_rate"] == -0.8 and d["beta1"] is None \
        and d["weight_decay"] == 0.0 and d["warmup_init"] is False
    assert not hasattr(o, "external_update")            # the step functions then take the unfused out_layer.fc1 route
    # host-side refusal of what the kernels cannot read: a CPU parameter with a gradient
    p[0].grad = torch.zeros(3, 4)
    with pytest.raises(RuntimeError, match="contiguous float32 HIP parameters and gradients"):
        o.step()
    assert all(st.get("step", 0) == 0 for st in o.state.values())      # a refused step() moves no step count


class _Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, groups, **kw):
        self.calls.append((groups, kw))
        return torch.optim.SGD([{"params": g["params"]} for g in groups if g["params"]], lr=kw["lr"])


@pytest.mark.parametrize("launcher", ["ppo", "pointwise", "reward_pair_dataloader", "pointwise_trad", "pointwise_2data_trad",
                                      "reward_trad", "ppo_trad"])
def test_build_optimizer_reaches_adafactor_with_the_reference_arguments(launcher, monkeypatch):
    import importlib
    mod = importlib.import_module("lr2ppo_amd.finetune." + launcher)
    rec = _Recorder()
    reg = dict(OPT.str2optimizer, adafactor=rec)
    owner = importlib.import_module(mod.build_optimizer.__module__)
    monkeypatch.setattr(owner, "str2optimizer", reg)
    args = argparse.Namespace(optimizer="adafactor", scheduler="constant_with_warmup", learning_rate=3e-4, critic_learning_rate=7e-4,
                              train_steps=10, warmup=0.1)
    lin = lambda: torch.nn.Linear(4, 3)                   # noqa: E731
    two = owner.__name__.endswith((".ppo",))
    if two:
        model = torch.nn.Module()
        model.actor, model.critic = lin(), lin()
    else:
        model = lin()
    out = mod.build_optimizer(args, model)
    assert len(out) == (4 if two else 2)
    want = [3e-4, 7e-4] if two else [3e-4]
    assert [kw for _, kw in rec.calls] == [dict(lr=lr, scale_parameter=False, relative_step=False) for lr in want]
    for groups, _ in rec.calls:
        assert [g["weight_decay"] for g in groups] == [0.01, 0.0]
        assert [tuple(p.shape) for p in groups[0]["params"]] == [(3, 4)] and [tuple(p.shape) for p in groups[1]["params"]] == [(3,)]
    # adamw keeps its branch
    rec2 = _Recorder()
    monkeypatch.setattr(owner, "str2optimizer", dict(reg, adamw=rec2))
    args.optimizer = "adamw"
    mod.build_optimizer(args, model)
    assert [kw for _, kw in rec2.calls] == [dict(lr=lr, correct_bias=False) for lr in want]


def test_the_two_refusals():
    from lr2ppo_amd.finetune import features, ppo
    args = argparse.Namespace(optimizer="adafactor", scheduler="linear", learning_rate=1e-3, train_steps=10, warmup=0.1)
    with pytest.raises(NotImplementedError, match="4-D"):
        features.build_encoder_optimizer(args, torch.nn.Linear(2, 2))
    lin = torch.nn.Linear(4, 3)
    ada = OPT.Adafactor(lin.parameters(), lr=1e-3, relative_step=False, scale_parameter=False)
    adam = OPT.AdamW(lin.parameters(), lr=1e-3, correct_bias=False)
    for pair in ((ada, ada), (adam, ada), (ada, adam)):
        with pytest.raises(NotImplementedError, match="beta2t"):
            ppo.GraphedPPOStep(args, None, None, *pair)


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------
def test_abi_stays_27_and_the_new_names_are_everywhere():
    header = open(os.path.join(REPO, "include", "lr2ppo_hip.h")).read()
    assert native.ABI_VERSION == 27 and re.search(r"#define LR2_ABI_VERSION 27\b", header)
    lib = native.lib()
    assert lib.lr2_abi_version() == 27
    integration = open(os.path.join(REPO, "INTEGRATION.md")).read()
    src = open(os.path.join(native.CSRC, "adafactor.hip")).read()
    assert "adafactor.hip" in native.SOURCES
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in native.SIGNATURES and name in integration, name
        assert re.search(r'extern "C" int %s\(' % name, src), name
        assert hasattr(lib, name)
    for macro, value in (("TILE_ROWS", native.ADAFACTOR_TILE_ROWS), ("TILE_COLS", native.ADAFACTOR_TILE_COLS),
                         ("CHUNK_1D", native.ADAFACTOR_CHUNK_1D), ("FIN_COLS", native.ADAFACTOR_FIN_COLS),
                         ("LAUNCHES", native.ADAFACTOR_LAUNCHES)):
        assert int(re.search(r"#define LR2_ADAFACTOR_%s (\d+)" % macro, header).group(1)) == value, macro
    # the ctypes mirrors have the header's layouts (x86-64: natural alignment)
    assert ctypes.sizeof(native.AdafactorTensor) == 4 * 8 + 6 * 8 + 4 * 4 + 8 == 104
    assert ctypes.sizeof(native.AdafactorTile) == 8 and ctypes.sizeof(native.AdafactorFin) == 16
    assert native.AdafactorTensor.weight_decay.offset == 96 and native.AdafactorTensor.n_tiles.offset == 80
    # existing layouts are untouched
    assert ctypes.sizeof(native.AdamChunk) == 48 and ctypes.sizeof(native.Epilogue) == 208


def test_argument_contract_refuses_before_any_launch():
    lib = native.lib()
    c = (ctypes.c_uint64 * 2)()
    assert lib.lr2_adafactor_launch_counts(None) == -1 and lib.lr2_adafactor_launch_counts(c) == 0
    before = (int(c[0]), int(c[1]))
    A = 64
    f = lib.lr2_adafactor_multi      # (tensors, tiles, n_tiles, fin, n_fin, ws, lr, beta2t, eps0, clip, lr_dev, stream)
    assert f(None, A, 1, A, 1, A, 1e-3, 0.0, 1e-30, 1.0, None, None) == -1
    assert f(A, None, 1, A, 1, A, 1e-3, 0.0, 1e-30, 1.0, None, None) == -1
    assert f(A, A, 0, A, 1, A, 1e-3, 0.0, 1e-30, 1.0, None, None) == -1
    assert f(A, A, 1, None, 1, A, 1e-3, 0.0, 1e-30, 1.0, None, None) == -1
    assert f(A, A, 1, A, -1, A, 1e-3, 0.0, 1e-30, 1.0, None, None) == -1
    assert f(A, A, 1, A, 1, None, 1e-3, 0.0, 1e-30, 1.0, None, None) == -1
    assert f(A, A, 1, A, 1, A + 4, 1e-3, 0.0, 1e-30, 1.0, None, None) == -1      # fp64 partials: 8-byte workspace
    assert f(A, A, 1, A, 1, A, 1e-3, 0.0, 1e-30, 0.0, None, None) == -1          # clip_threshold > 0
    assert f(A, A, 1, A, 1, A, 1e-3, 0.0, 1e-30, 1.0, A + 2, None) == -1
    assert lib.lr2_adafactor_launch_counts(c) == 0 and (int(c[0]), int(c[1])) == before


# ---- the plan against a brute-force count -------------------------------------------------------------------------------------------
PLAN_SHAPES = [(1, 1), (1, 7), (7, 1), (3, 5), (4, 768), (513, 1025), (1024, 1023), (511, 3077), (3072, 162816), (1,), (3,), (8192,),
               (8193,), (4097,), (768,)]


def test_plan_against_brute_force():
    TR, TC, CH, FC = native.ADAFACTOR_TILE_ROWS, native.ADAFACTOR_TILE_COLS, native.ADAFACTOR_CHUNK_1D, native.ADAFACTOR_FIN_COLS
    tensors, tiles, fin, ws = OPT.adafactor_plan(PLAN_SHAPES)
    assert len(tensors) == len(PLAN_SHAPES)
    regions = []
    for ti, (shape, t) in enumerate(zip(PLAN_SHAPES, tensors)):
        mine = [idx for tt, idx in tiles if tt == ti]
        assert mine == list(range(t["n_tiles"]))                      # every tile exactly once, in order
        if len(shape) == 2:
            R, Cc = shape
            cover = set()
            if R * Cc <= 4_000_000:                                   # brute force: every element lies in exactly one tile
                for idx in mine:
                    i0, j0 = (idx // t["n_col_tiles"]) * TR, (idx % t["n_col_tiles"]) * TC
                    assert i0 < R and j0 < Cc
                    cells = {(i, j) for i in range(i0, min(i0 + TR, R), 97) for j in range(j0, min(j0 + TC, Cc), 89)}
                    assert not (cells & cover)
                    cover |= cells
                assert cover == {(i, j) for i in range(R) for j in range(Cc)
                                 if (i % TR) % 97 == 0 and (j % TC) % 89 == 0}
            assert t["n_row_tiles"] == len(range(0, R, TR)) and t["n_col_tiles"] == len(range(0, Cc, TC))
            assert t["n_tiles"] == t["n_row_tiles"] * t["n_col_tiles"] and (t["rows"], t["cols"]) == (R, Cc)
            f = [(k, s) for tt, k, s in fin if tt == ti]
            assert f == [(0, 0)] + [(1, s) for s in range(0, Cc, FC)]
            regions += [(t["ws_row"], 4 * t["n_col_tiles"] * R), (t["ws_col"], 4 * t["n_row_tiles"] * Cc), (t["ws_mean"], 4)]
        else:
            assert (t["rows"], t["cols"]) == (0, shape[0]) and t["n_tiles"] == len(range(0, shape[0], CH))
            assert not [1 for tt, _, _ in fin if tt == ti]
        assert t["ws_sq"] % 8 == 0
        regions.append((t["ws_sq"], 8 * t["n_tiles"]))
    regions.sort()
    assert regions[0][0] == 0
    for (a, n), (b, _) in zip(regions, regions[1:]):
        assert a + n == b                                            # no overlap, no hole
    assert regions[-1][0] + regions[-1][1] == ws
    fc1 = tensors[PLAN_SHAPES.index((3072, 162816))]
    assert (fc1["n_row_tiles"], fc1["n_col_tiles"]) == (6, 159)
    part = 4 * (159 * 3072 + 6 * 162816) + 8 * 954 + 4
    assert part < 6 * 2 ** 20                                        # "a few MB" at the fc1 shape: 5.9 MB
    with pytest.raises(NotImplementedError):
        OPT.adafactor_plan([(2, 3, 4)])
