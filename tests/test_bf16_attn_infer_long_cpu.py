"""Single-plane bf16 attention above 288 tokens for the bf16 and MX-FP8 inference modes (FeatureExtractor(precision="bf16" | "mxfp8",
attention_long=True); csrc/selfattn_mx_blocked.hip), the parts that need no GPU: lr2_self_attn_fwd_bf16_blocked rejects bad arguments
with the code its header names before launching anything, and the switch's combinations at the constructor, the launchers' flag and
tools/encoder_bench.py's command line."""
import argparse
import ctypes
import os
import sys

import pytest

A = 4096          # a stand-in device address, aligned for every operand (nothing is dereferenced: every call here fails)


def _count(lib):
    c = ctypes.c_uint64(12345)
    assert lib.lr2_self_attn_fwd_bf16_blocked_launch_count(ctypes.byref(c)) == 0
    return c.value


def test_entry_point_validates_before_launching():
    from lr2ppo_amd import _native as native
    from lr2ppo_amd import ops
    lib = native.lib()
    before = _count(lib)
    assert ops.self_attn_fwd_bf16_blocked_launch_count() == before

    def call(*, q=A, k=A, v=A, seg=A, o_f32=A, o_q=A, o_s=A, o_b=A, ld=384, ld_o=128, batch=2, heads=2, L=320, hd=64):
        return lib.lr2_self_attn_fwd_bf16_blocked(q, k, v, ld, seg, o_f32, o_q, o_s, o_b, ld_o, batch, heads, L, hd, 0.125, None)

    ARG, SHAPE = -1, -2
    # LR2_ERR_ARG
    for name in ("q", "k", "v", "seg"):
        assert call(**{name: None}) == ARG, name
    assert call(o_f32=None, o_q=None, o_s=None, o_b=None) == ARG                       # no output at all
    assert call(o_s=None) == ARG and call(o_q=None) == ARG                             # o_q without o_scales, and the reverse
    assert call(o_f32=None, o_b=None, o_s=None) == ARG and call(o_f32=None, o_b=None, o_q=None) == ARG
    for name in ("q", "k", "v", "o_f32"):                                              # 16-byte alignment
        assert call(**{name: A + 8}) == ARG, name
    assert call(o_b=A + 4) == ARG and call(o_b=A + 2) == ARG                           # 8-byte alignment of the plane
    assert call(o_q=A + 2) == ARG and call(o_q=A + 1) == ARG                           # 4-byte alignment of the MX bytes
    assert call(batch=0) == ARG and call(batch=-1) == ARG and call(heads=0) == ARG and call(heads=-3) == ARG
    # LR2_ERR_SHAPE
    assert call(hd=32) == SHAPE and call(hd=128) == SHAPE
    assert call(L=0) == SHAPE and call(L=-5) == SHAPE
    assert call(ld=120) == SHAPE and call(ld=388) == SHAPE                             # below heads * 64; no multiple of 8
    assert call(ld_o=120) == SHAPE and call(ld_o=132) == SHAPE
    assert call(ld_o=136) == SHAPE                                                     # ld_o % 32 with o_q given
    with pytest.raises(native.NativeError, match="LR2_ERR_SHAPE"):
        native.check(call(L=0), "lr2_self_attn_fwd_bf16_blocked")
    with pytest.raises(native.NativeError, match="LR2_ERR_ARG"):
        native.check(call(q=None), "lr2_self_attn_fwd_bf16_blocked")
    # a call that looks accepted but for one argument leaves the count where it was: nothing was launched
    assert _count(lib) == before and ops.self_attn_fwd_bf16_blocked_launch_count() == before
    assert lib.lr2_self_attn_fwd_bf16_blocked_launch_count(None) == ARG


def test_ld_o_rule_depends_on_the_mx_output():
    """ld_o = 136 (a multiple of 8, not of 32) is a shape error only when o_q is given; without it the call passes validation, which
    is not tried here (it would launch).  The other way round is testable: with o_q the code is LR2_ERR_SHAPE at any other output set."""
    from lr2ppo_amd import _native as native
    lib = native.lib()
    before = _count(lib)
    for o_f32, o_b in ((A, A), (None, A), (A, None), (None, None)):
        assert lib.lr2_self_attn_fwd_bf16_blocked(A, A, A, 384, A, o_f32, A, A, o_b, 136, 2, 2, 320, 64, 0.125, None) == -2
    assert _count(lib) == before


def _towers():
    from lr2ppo_amd.finetune.features import TEXT_CONFIG, VIT_CONFIG, encoder_args
    return encoder_args(VIT_CONFIG, layers_num=1), encoder_args(TEXT_CONFIG, layers_num=1)


def test_extractor_switch():
    from lr2ppo_amd.finetune.features import FeatureExtractor
    from lr2ppo_amd.tencentpretrain.encoders.transformer_encoder import TransformerEncoder
    assert TransformerEncoder.infer_attention_long is False
    for prec in ("split_bf16", "bf16_train", "mxfp8_train"):
        with pytest.raises(ValueError, match="attention_long"):
            FeatureExtractor(*_towers(), precision=prec, attention_long=True)
        off = FeatureExtractor(*_towers(), precision=prec)
        assert not off.attention_long and not off.image.encoder.infer_attention_long and not off.text.encoder.infer_attention_long
    for prec in ("bf16", "mxfp8"):
        fx = FeatureExtractor(*_towers(), precision=prec, attention_long=True)
        assert fx.attention_long and fx.image.encoder.infer_attention_long and fx.text.encoder.infer_attention_long
        assert not fx.image.encoder.bf16_attention_long and not fx.text.encoder.bf16_attention_long          # training's switch: untouched
        off = FeatureExtractor(*_towers(), precision=prec)
        assert not off.attention_long and not off.image.encoder.infer_attention_long and not off.text.encoder.infer_attention_long


def _args(**kw):
    from lr2ppo_amd.finetune.features import raw_input_opts
    p = raw_input_opts(argparse.ArgumentParser())
    a = p.parse_args(["--raw_inputs", "--encoder_layers", "1"] + [f"--{k}" for k, v in kw.items() if v])
    a.seq_length, a.visual_feat_dim, a.device = 304, 768, "meta"
    return a


def test_features_attention_long_flag():
    from lr2ppo_amd.finetune.features import build_extractor
    assert _args(features_attention_long=True).features_attention_long and not _args().features_attention_long
    with pytest.raises(ValueError, match="needs --bf16_features or --fp8_features"):
        build_extractor(_args(features_attention_long=True))
    with pytest.raises(ValueError, match="needs --bf16_features or --fp8_features"):
        build_extractor(_args(features_attention_long=True, bf16_finetune=True), trainable=True)
    for mode, prec in (("bf16_features", "bf16"), ("fp8_features", "mxfp8")):
        fx = build_extractor(_args(features_attention_long=True, **{mode: True}))
        assert fx.precision == prec and fx.attention_long
        assert fx.image.encoder.infer_attention_long and fx.text.encoder.infer_attention_long
        off = build_extractor(_args(**{mode: True}))
        assert not off.attention_long and not off.text.encoder.infer_attention_long


def test_encoder_bench_command_line(capsys):
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    sys.path.insert(0, tools)
    try:
        import encoder_bench
    finally:
        sys.path.remove(tools)
    for bad in (["--attention-long", "--train"], ["--attention-long", "--train", "--precision", "bf16_train"],
                ["--attention-long", "--precision", "split_bf16"], ["--attention-long"],
                ["--attention-long", "--ppo-shapes", "--precision", "split_bf16"]):
        with pytest.raises(SystemExit):
            encoder_bench.parse_args(bad)
        assert "--attention-long" in capsys.readouterr().err
    for prec in ("bf16", "mxfp8"):
        a = encoder_bench.parse_args(["--only", "text", "--text-seq", "512", "--batch", "32", "--ppo-shapes", "--precision", prec,
                                      "--attention-long"])
        assert a.attention_long and a.precision == prec and a.text_seq == 512
        assert not encoder_bench.parse_args(["--only", "text", "--text-seq", "512", "--ppo-shapes", "--precision", prec]).attention_long
    with pytest.raises(SystemExit):                                   # as before: the split-bf16 forward has no per-tower --ppo-shapes loop
        encoder_bench.parse_args(["--only", "text", "--text-seq", "512", "--ppo-shapes"])
