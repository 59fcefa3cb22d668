"""Key-blocked f16 attention above 288 tokens for the f16 inference mode (FeatureExtractor(precision="f16", f16_attention_long=True);
csrc/selfattn_mx_blocked.hip), the parts that need no GPU: lr2_self_attn_fwd_f16_blocked rejects bad arguments with the code its header
names before launching anything, the switch's combinations at the constructor, the launchers' flag and tools/encoder_bench.py's command
line, and the ABI number, which the two additive entry points leave at 27."""
import argparse
import ctypes
import os
import re
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 4096          # a stand-in device address, aligned for every operand (nothing is dereferenced: every call here fails)


def _count(lib):
    c = ctypes.c_uint64(12345)
    assert lib.lr2_self_attn_fwd_f16_blocked_launch_count(ctypes.byref(c)) == 0
    return c.value


def test_entry_point_validates_before_launching():
    from lr2ppo_amd import _native as native
    from lr2ppo_amd import ops
    lib = native.lib()
    before = _count(lib)
    assert ops.self_attn_fwd_f16_blocked_launch_count() == before

    def call(*, q=A, k=A, v=A, seg=A, o_f32=A, o_f16=A, ld=384, ld_o=128, batch=2, heads=2, L=320, hd=64):
        return lib.lr2_self_attn_fwd_f16_blocked(q, k, v, ld, seg, o_f32, o_f16, ld_o, batch, heads, L, hd, 0.125, None)

    ARG, SHAPE = -1, -2
    # LR2_ERR_ARG
    for name in ("q", "k", "v", "seg"):
        assert call(**{name: None}) == ARG, name
    assert call(o_f32=None, o_f16=None) == ARG                                         # no output at all
    for name in ("q", "k", "v", "o_f32"):                                              # 16-byte alignment
        assert call(**{name: A + 8}) == ARG, name
        assert call(**{name: A + 4}) == ARG, name
    assert call(o_f16=A + 4) == ARG and call(o_f16=A + 2) == ARG                       # 8-byte alignment of the plane
    assert call(o_f32=None, o_f16=A + 4) == ARG
    assert call(batch=0) == ARG and call(batch=-1) == ARG and call(heads=0) == ARG and call(heads=-3) == ARG
    # LR2_ERR_SHAPE
    assert call(hd=32) == SHAPE and call(hd=128) == SHAPE
    assert call(L=0) == SHAPE and call(L=-5) == SHAPE
    assert call(ld=120) == SHAPE and call(ld=388) == SHAPE                             # below heads * 64; no multiple of 8
    assert call(ld_o=120) == SHAPE and call(ld_o=130) == SHAPE                         # below heads * 64; no multiple of 4
    for outs in (dict(o_f32=None), dict(o_f16=None)):                                  # the same at either single output
        assert call(hd=32, **outs) == SHAPE and call(L=0, **outs) == SHAPE and call(ld=388, **outs) == SHAPE
        assert call(ld_o=130, **outs) == SHAPE and call(ld_o=120, **outs) == SHAPE
    with pytest.raises(native.NativeError, match="LR2_ERR_SHAPE"):
        native.check(call(L=0), "lr2_self_attn_fwd_f16_blocked")
    with pytest.raises(native.NativeError, match="LR2_ERR_ARG"):
        native.check(call(q=None), "lr2_self_attn_fwd_f16_blocked")
    # a call that looks accepted but for one argument leaves the count where it was: nothing was launched
    assert _count(lib) == before and ops.self_attn_fwd_f16_blocked_launch_count() == before
    assert lib.lr2_self_attn_fwd_f16_blocked_launch_count(None) == ARG


def test_the_one_block_entry_point_is_unchanged():
    """lr2_self_attn_fwd_f16 still answers LR2_ERR_SHAPE at L = 289, and counts nothing for it"""
    from lr2ppo_amd import _native as native
    from lr2ppo_amd import ops
    lib = native.lib()
    c0, b0 = ops.self_attn_fwd_f16_launch_count(), _count(lib)
    assert lib.lr2_self_attn_fwd_f16(A, A, A, 384, A, A, A, 128, 2, 2, 289, 64, 0.125, None) == -2
    assert ops.self_attn_fwd_f16_launch_count() == c0 and _count(lib) == b0


def _towers():
    from lr2ppo_amd.finetune.features import TEXT_CONFIG, VIT_CONFIG, encoder_args
    return encoder_args(VIT_CONFIG, layers_num=1), encoder_args(TEXT_CONFIG, layers_num=1)


def test_defaults():
    from lr2ppo_amd.finetune.features import FeatureExtractor
    from lr2ppo_amd.tencentpretrain.encoders.transformer_encoder import TransformerEncoder
    assert TransformerEncoder.f16_attention_long is False
    with torch.device("meta"):
        fx = FeatureExtractor(*_towers(), precision="f16")
    assert fx.f16_attention_long is False
    assert fx.image.encoder.f16_attention_long is False and fx.text.encoder.f16_attention_long is False


def test_extractor_switch():
    from lr2ppo_amd.finetune.features import FeatureExtractor
    with torch.device("meta"):
        fx = FeatureExtractor(*_towers(), precision="f16", f16_attention_long=True)
        assert fx.f16_attention_long and fx.image.encoder.f16_attention_long and fx.text.encoder.f16_attention_long
        assert not fx.attention_long and not fx.text.encoder.infer_attention_long          # the bf16 / MX-FP8 modes' switch: untouched
        assert not fx.text.encoder.bf16_attention_long                                     # training's switch: untouched
        for prec in FeatureExtractor.PRECISIONS:
            if prec == "f16":
                continue
            with pytest.raises(ValueError, match="f16_attention_long"):
                FeatureExtractor(*_towers(), precision=prec, f16_attention_long=True)
            off = FeatureExtractor(*_towers(), precision=prec)
            assert not off.f16_attention_long and not off.image.encoder.f16_attention_long and not off.text.encoder.f16_attention_long
        with pytest.raises(ValueError, match="key-blocked"):                               # as before: the bf16 kernel's switch is refused
            FeatureExtractor(*_towers(), precision="f16", attention_long=True)
        with pytest.raises(ValueError, match="key-blocked"):
            FeatureExtractor(*_towers(), precision="f16", attention_long=True, f16_attention_long=True)


def _args(**kw):
    from lr2ppo_amd.finetune.features import raw_input_opts
    p = raw_input_opts(argparse.ArgumentParser())
    a = p.parse_args(["--raw_inputs", "--encoder_layers", "1"] + [f"--{k}" for k, v in kw.items() if v])
    a.seq_length, a.visual_feat_dim, a.device = 304, 768, "meta"
    return a


def test_flag_is_on_all_three_launchers():
    import importlib
    for name in ("ppo", "pointwise", "reward_pair_dataloader"):      # the launchers that take raw_input_opts
        mod = importlib.import_module(f"lr2ppo_amd.finetune.{name}")
        text = mod.build_parser().format_help()
        assert "--f16_attention_long" in text and "--f16_features" in text, name


def test_f16_attention_long_flag():
    from lr2ppo_amd.finetune.features import build_extractor
    assert _args(f16_attention_long=True).f16_attention_long and not _args().f16_attention_long
    with pytest.raises(ValueError, match="needs --f16_features"):
        build_extractor(_args(f16_attention_long=True))
    for other in ("bf16_features", "fp8_features"):
        with pytest.raises(ValueError):
            build_extractor(_args(f16_attention_long=True, **{other: True}))
    for mode in ("bf16_finetune", "fp8_finetune"):                                         # no training mode takes it
        with pytest.raises(ValueError, match="f16_attention_long"):
            build_extractor(_args(f16_attention_long=True, **{mode: True}), trainable=True)
        with pytest.raises(ValueError):
            build_extractor(_args(f16_attention_long=True, f16_features=True, **{mode: True}), trainable=True)
    with pytest.raises(ValueError):
        build_extractor(_args(f16_attention_long=True, f16_features=True), trainable=True)
    with pytest.raises(ValueError, match="features_attention_long"):                       # as before
        build_extractor(_args(features_attention_long=True, f16_features=True))
    with pytest.raises(ValueError, match="features_attention_long"):
        build_extractor(_args(features_attention_long=True, f16_features=True, f16_attention_long=True))
    fx = build_extractor(_args(f16_features=True, f16_attention_long=True))
    assert fx.precision == "f16" and fx.f16_attention_long and not fx.attention_long
    assert fx.image.encoder.f16_attention_long and fx.text.encoder.f16_attention_long
    off = build_extractor(_args(f16_features=True))
    assert not off.f16_attention_long and not off.text.encoder.f16_attention_long and not off.image.encoder.f16_attention_long


def test_encoder_bench_command_line(capsys):
    tools = os.path.join(REPO, "tools")
    sys.path.insert(0, tools)
    try:
        import encoder_bench
    finally:
        sys.path.remove(tools)
    long = ["--only", "text", "--text-seq", "512", "--ppo-shapes"]
    a = encoder_bench.parse_args(long + ["--precision", "f16", "--f16-attention-long"])
    assert a.f16_attention_long and not a.attention_long and a.precision == "f16" and a.text_seq == 512 and a.only == "text"
    assert not encoder_bench.parse_args(long + ["--precision", "f16"]).f16_attention_long
    for bad in (long + ["--precision", "bf16", "--f16-attention-long"], long + ["--precision", "mxfp8", "--f16-attention-long"],
                ["--ppo-shapes", "--f16-attention-long"], ["--f16-attention-long"],
                ["--ppo-shapes", "--precision", "f16", "--f16-attention-long", "--train"],
                ["--train", "--precision", "bf16_train", "--f16-attention-long"],
                ["--precision", "f16", "--f16-attention-long"]):                           # without --ppo-shapes
        with pytest.raises(SystemExit):
            encoder_bench.parse_args(bad)
        capsys.readouterr()
    with pytest.raises(SystemExit):                                                        # as before: the bf16 kernel's switch
        encoder_bench.parse_args(long + ["--precision", "f16", "--attention-long"])


def test_abi_number_stays_27_and_the_names_are_bound():
    from lr2ppo_amd import _native as native
    hdr = open(os.path.join(REPO, "include", "lr2ppo_hip.h")).read()
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert native.ABI_VERSION == 27 == int(re.search(r"#define LR2_ABI_VERSION (\d+)", hdr).group(1))
    assert int(re.search(r"lr2_abi_version\(\) == (\d+)", doc).group(1)) == 27 and native.lib().lr2_abi_version() == 27
    for name in ("lr2_self_attn_fwd_f16_blocked", "lr2_self_attn_fwd_f16_blocked_launch_count"):
        assert name in native.SIGNATURES and re.search(r"\bint %s\(" % name, hdr), name
        assert getattr(native.lib(), name) is not None
    assert native.SIGNATURES["lr2_self_attn_fwd_f16_blocked"] == native.SIGNATURES["lr2_self_attn_fwd_f16"]
    defining = [s for s in os.listdir(native.CSRC) if s.endswith(".hip")
                and 'extern "C" int lr2_self_attn_fwd_f16_blocked(' in open(os.path.join(native.CSRC, s)).read()]
    assert len(defining) == 1 and defining[0] in native.SOURCES, defining
