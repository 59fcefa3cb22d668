"""Single-plane bf16 training attention for sequences longer than 288 (FeatureExtractor(precision="bf16_train", bf16_attention=True,
bf16_attention_long=True); csrc/selfattn_b1_blocked.hip), the parts that need no GPU: the two blocked entry points reject bad arguments
before launching anything, the plan entry point's block lengths over L = 1 .. 1100, the --bf16_attention_long flag's and the
constructor's combinations on both towers, and the activation bookkeeping of the branch."""
import argparse
import ctypes

import pytest

import attn_cases as AC


def test_blocked_entry_points_validate_before_launching():
    from lr2ppo_amd import _native as native
    from lr2ppo_amd import ops
    lib = native.lib()
    A = 16          # a stand-in device address (nothing is dereferenced: every call fails)
    before = ops.self_attn_bf16_blocked_launch_counts()
    before_one_block = ops.self_attn_bf16_train_launch_counts()

    def fwd(*, q=A, k=A, v=A, o=A, seg=A, ld=384, ld_o=128, p=0.0, L=320, hd=64):
        return lib.lr2_self_attn_fwd_bf16_train_blocked(q, k, v, ld, seg, o, ld_o, None, p, 0, 0, 2, 2, L, hd, 0.125, None)

    def bwd(*, q=A, k=A, v=A, do=A, seg=A, dq=A, dk=A, dv=A, ws=A, ws2=A, ld=384, ld_do=128, ld_d=384, p=0.0, L=320, hd=64):
        return lib.lr2_self_attn_bwd_bf16_blocked(q, k, v, ld, do, ld_do, seg, dq, dk, dv, ld_d, ws, ws2, p, 0, 0, 2, 2, L, hd, 0.125,
                                                  None)

    for call in (fwd, bwd):
        for kw in (dict(L=0), dict(hd=32), dict(ld=388), dict(p=1.0)):          # through _nat.check
            with pytest.raises(native.NativeError):
                native.check(call(**kw), call.__name__)
        assert call(L=0) == -2 and call(L=-5) == -2 and call(hd=32) == -2 and call(hd=128) == -2
        assert call(ld=388) == -2
        assert call(p=1.0) == -1 and call(p=-0.1) == -1 and call(p=float("nan")) == -1
        for name in ("q", "k", "v", "seg"):
            assert call(**{name: None}) == -1, name
        assert call(q=8) == -1                                                  # 16-byte alignment of the operands
    assert fwd(ld_o=132) == -2 and fwd(o=None) == -1
    assert bwd(ld_do=132) == -2 and bwd(ld_d=388) == -2
    for name in ("do", "dq", "dk", "dv", "ws", "ws2"):
        assert bwd(**{name: None}) == -1, name
    assert ops.self_attn_bf16_blocked_launch_counts() == before                  # nothing was launched
    assert ops.self_attn_bf16_train_launch_counts() == before_one_block
    assert lib.lr2_self_attn_bf16_blocked_launch_counts(None) == -1
    counts = (ctypes.c_uint64 * 2)()
    assert lib.lr2_self_attn_bf16_blocked_launch_counts(counts) == 0 and tuple(counts) == before


def test_plan():
    from lr2ppo_amd import _native as native
    from lr2ppo_amd import ops
    assert native.lib().lr2_self_attn_bf16_blocked_plan(0, None, None, None) == -1
    assert native.lib().lr2_self_attn_bf16_blocked_plan(300, None, None, None) == 0          # NULL outputs are skipped
    for L in range(1, 1101):
        plan = ops.self_attn_bf16_blocked_plan(L)
        assert len(plan) == 3
        for block in plan:
            assert block > 0 and block % 16 == 0, (L, plan)
            n_blocks = -(-L // block)
            assert n_blocks >= 1 and all(j * block < L for j in range(n_blocks)), (L, plan)          # no block without a row
        if L > 224:
            assert plan[0] == AC.fwd_block(L), (L, plan)
        assert plan[0] <= 224


def _args(**kw):
    from lr2ppo_amd.finetune.features import raw_input_opts
    p = raw_input_opts(argparse.ArgumentParser())
    a = p.parse_args(["--raw_inputs"] + [f"--{k}" for k, v in kw.items() if v])
    a.seq_length, a.visual_feat_dim, a.device = 196, 768, "meta"
    return a


def test_bf16_attention_long_flag():
    from lr2ppo_amd.finetune.features import build_extractor
    assert _args(bf16_finetune=True, bf16_attention=True, bf16_attention_long=True).bf16_attention_long
    assert not _args(bf16_finetune=True, bf16_attention=True).bf16_attention_long
    with pytest.raises(ValueError, match="needs --bf16_attention"):
        build_extractor(_args(bf16_finetune=True, bf16_attention_long=True), trainable=True)
    with pytest.raises(ValueError, match="bf16_finetune"):                       # --bf16_attention's own rule comes first
        build_extractor(_args(bf16_attention=True, bf16_attention_long=True), trainable=True)


def test_extractor_sets_the_long_switch_on_both_towers():
    from lr2ppo_amd.finetune.features import TEXT_CONFIG, VIT_CONFIG, FeatureExtractor, encoder_args
    towers = lambda: (encoder_args(VIT_CONFIG, layers_num=1), encoder_args(TEXT_CONFIG, layers_num=1))          # noqa: E731
    fx = FeatureExtractor(*towers(), precision="bf16_train", bf16_attention=True, bf16_attention_long=True)
    assert fx.bf16_attention_long and fx.image.encoder.bf16_attention_long and fx.text.encoder.bf16_attention_long
    assert fx.image.encoder.bf16_attention and fx.text.encoder.bf16_attention
    for enc in (fx.image.encoder, fx.text.encoder):
        assert enc._b1_attention(64, 300) and enc._b1_attention(64, 288) and not enc._b1_attention(32, 300)
    off = FeatureExtractor(*towers(), precision="bf16_train", bf16_attention=True)
    assert not off.bf16_attention_long and not off.image.encoder.bf16_attention_long and not off.text.encoder.bf16_attention_long
    assert off.text.encoder._b1_attention(64, 288) and not off.text.encoder._b1_attention(64, 289)
    with pytest.raises(ValueError, match="bf16_attention"):
        FeatureExtractor(*towers(), precision="bf16_train", bf16_attention_long=True)
    for prec in ("split_bf16", "mxfp8_train", "bf16", "mxfp8"):
        with pytest.raises(ValueError, match="bf16_attention"):
            FeatureExtractor(*towers(), precision=prec, bf16_attention=True, bf16_attention_long=True)
        with pytest.raises(ValueError, match="bf16_attention"):
            FeatureExtractor(*towers(), precision=prec, bf16_attention_long=True)


@pytest.mark.parametrize("pre", [True, False], ids=["pre_ln", "post_ln"])
def test_saved_activation_bytes(pre):
    """At L = 514 the long switch takes Q | K | V and the context to ONE plane each and drops the kept log-sum-exp: 8 M E + 4 B H L
    bytes less per layer; recompute=True keeps each layer's fp32 input either way; without the switch L = 300 keeps today's bytes."""
    from lr2ppo_amd.finetune.features import TEXT_CONFIG, VIT_CONFIG, encoder_args
    from lr2ppo_amd.tencentpretrain.encoders import str2encoder
    layers = 3
    enc = str2encoder["transformer"](encoder_args(VIT_CONFIG if pre else TEXT_CONFIG, layers_num=layers))
    E, H = enc.hidden_size, enc.heads_num
    B, L = 5, 514
    M = B * L
    enc.bf16_train = True
    three_pass = enc.saved_activation_bytes(B, L)
    three_pass_300 = enc.saved_activation_bytes(B, 300)
    enc.bf16_attention = True
    assert enc.saved_activation_bytes(B, L) == three_pass                           # the long switch is off: the 3-pass branch's bytes
    assert enc.saved_activation_bytes(B, 300) == three_pass_300
    off_rc = enc.saved_activation_bytes(B, L, recompute=True)
    enc.bf16_attention_long = True
    assert three_pass - enc.saved_activation_bytes(B, L) == layers * (8 * M * E + 4 * B * H * L)
    assert enc.saved_activation_bytes(B, L, recompute=True) == off_rc
    assert three_pass_300 - enc.saved_activation_bytes(B, 300) == layers * (8 * B * 300 * E + 4 * B * H * 300)
    enc.bf16_attention = False                                                      # the long switch alone changes nothing
    assert enc.saved_activation_bytes(B, L) == three_pass
    enc.bf16_attention, enc.bf16_train = True, False                                # a switch of bf16_train only
    enc.bf16_attention_long = False
    split = enc.saved_activation_bytes(B, L)
    enc.bf16_attention_long = True
    assert enc.saved_activation_bytes(B, L) == split
