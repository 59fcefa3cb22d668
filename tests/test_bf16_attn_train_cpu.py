"""Single-plane bf16 attention of the bf16_train mode (FeatureExtractor(precision="bf16_train", bf16_attention=True)), the parts that
need no GPU: the two entry points reject bad arguments before launching anything, the --bf16_attention flag's combinations, the
attribute on both towers and the activation bookkeeping of the branch."""
import argparse
import ctypes

import pytest


def test_entry_points_validate_before_launching():
    from lr2ppo_amd import _native as native
    from lr2ppo_amd import ops
    lib = native.lib()
    A = 16          # a stand-in device address (nothing is dereferenced: every call fails)
    before = ops.self_attn_bf16_train_launch_counts()

    def fwd(*, q=A, o=A, seg=A, ld=384, ld_o=128, p=0.0, L=64, hd=64):
        return lib.lr2_self_attn_fwd_bf16_train(q, A, A, ld, seg, o, ld_o, None, p, 0, 0, 2, 2, L, hd, 0.125, None)

    def bwd(*, q=A, do=A, dq=A, ws=A, ld=384, ld_do=128, ld_d=384, p=0.0, L=64, hd=64):
        return lib.lr2_self_attn_bwd_bf16(q, A, A, ld, do, ld_do, A, dq, A, A, ld_d, ws, A, p, 0, 0, 2, 2, L, hd, 0.125, None)

    for call in (fwd, bwd):
        for kw in (dict(L=289), dict(hd=32), dict(ld=388), dict(p=1.0)):          # the four refusals, through _nat.check
            with pytest.raises(native.NativeError):
                native.check(call(**kw), call.__name__)
        assert call(L=289) == -2 and call(L=0) == -2 and call(hd=32) == -2 and call(hd=128) == -2
        assert call(ld=388) == -2
        assert call(p=1.0) == -1 and call(p=-0.1) == -1 and call(p=float("nan")) == -1
        assert call(q=None) == -1
    assert fwd(ld_o=132) == -2 and fwd(o=None) == -1 and fwd(seg=None) == -1
    assert bwd(ld_do=132) == -2 and bwd(ld_d=388) == -2
    assert bwd(do=None) == -1 and bwd(dq=None) == -1 and bwd(ws=None) == -1
    assert ops.self_attn_bf16_train_launch_counts() == before                        # nothing was launched
    assert lib.lr2_self_attn_bf16_train_launch_counts(None) == -1
    counts = (ctypes.c_uint64 * 2)()
    assert lib.lr2_self_attn_bf16_train_launch_counts(counts) == 0 and tuple(counts) == before


def _args(**kw):
    from lr2ppo_amd.finetune.features import raw_input_opts
    p = raw_input_opts(argparse.ArgumentParser())
    a = p.parse_args(["--raw_inputs"] + [f"--{k}" for k, v in kw.items() if v])
    a.seq_length, a.visual_feat_dim, a.device = 196, 768, "meta"
    return a


def test_bf16_attention_flag():
    from lr2ppo_amd.finetune.features import build_extractor
    assert _args(bf16_finetune=True, bf16_attention=True).bf16_attention and not _args(bf16_finetune=True).bf16_attention
    with pytest.raises(ValueError, match="bf16_finetune"):
        build_extractor(_args(bf16_attention=True), trainable=True)
    with pytest.raises(ValueError, match="bf16_finetune"):
        build_extractor(_args(bf16_attention=True, fp8_finetune=True), trainable=True)


def test_extractor_sets_the_switch_on_both_towers():
    from lr2ppo_amd.finetune.features import TEXT_CONFIG, VIT_CONFIG, FeatureExtractor, encoder_args
    towers = lambda: (encoder_args(VIT_CONFIG, layers_num=1), encoder_args(TEXT_CONFIG, layers_num=1))          # noqa: E731
    fx = FeatureExtractor(*towers(), precision="bf16_train", bf16_attention=True)
    assert fx.bf16_attention and fx.image.encoder.bf16_attention and fx.text.encoder.bf16_attention
    assert fx.image.encoder.bf16_train and fx.text.encoder.bf16_train
    off = FeatureExtractor(*towers(), precision="bf16_train")
    assert not off.bf16_attention and not off.image.encoder.bf16_attention and not off.text.encoder.bf16_attention
    for prec in ("split_bf16", "mxfp8_train", "bf16", "mxfp8"):
        with pytest.raises(ValueError, match="bf16_attention"):
            FeatureExtractor(*towers(), precision=prec, bf16_attention=True)


@pytest.mark.parametrize("pre", [True, False], ids=["pre_ln", "post_ln"])
def test_saved_activation_bytes(pre):
    """Q | K | V ([M, 3E]) and the context ([M, E]) are kept as ONE bf16 plane instead of hi / lo planes and the log-sum-exp
    ([B, H, L] fp32) is not kept at all: 8 M E + 4 B H L bytes less per layer, either LayerNorm placement; nothing else changes."""
    from lr2ppo_amd.finetune.features import TEXT_CONFIG, VIT_CONFIG, encoder_args
    from lr2ppo_amd.tencentpretrain.encoders import str2encoder
    layers = 3
    enc = str2encoder["transformer"](encoder_args(VIT_CONFIG if pre else TEXT_CONFIG, layers_num=layers))
    E, H = enc.hidden_size, enc.heads_num
    B, L = 5, 197
    M = B * L
    split = enc.saved_activation_bytes(B, L)
    enc.bf16_attention = True
    assert enc.saved_activation_bytes(B, L) == split                                # a switch of bf16_train only
    enc.bf16_train = True
    on = enc.saved_activation_bytes(B, L)
    on_rc = enc.saved_activation_bytes(B, L, recompute=True)
    enc.bf16_attention = False
    assert enc.saved_activation_bytes(B, L) - on == layers * (8 * M * E + 4 * B * H * L)
    assert enc.saved_activation_bytes(B, L, recompute=True) == on_rc                # each layer's fp32 input, whatever the branch
    enc.bf16_attention = True
    assert enc.saved_activation_bytes(B, 300) == _without(enc, B, 300)              # L > 288: today's branch, today's bytes


def _without(enc, B, L):
    enc.bf16_attention = False
    try:
        return enc.saved_activation_bytes(B, L)
    finally:
        enc.bf16_attention = True
