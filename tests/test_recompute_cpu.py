"""Per-layer activation recomputation, the parts that need no GPU: the saved-activation arithmetic (the formula the training
forward allocates its arena with) and the flag's plumbing."""
import argparse

import pytest


def _encoder(config, **over):
    from lr2ppo_amd.finetune.features import encoder_args
    from lr2ppo_amd.tencentpretrain.encoders import str2encoder
    return str2encoder["transformer"](encoder_args(config, **over))


@pytest.mark.parametrize("tower,batch,L", [("vit", 512, 197), ("roberta", 640, 196)])
def test_saved_activation_bytes_is_the_arena_formula(tower, batch, L):
    from lr2ppo_amd.finetune.features import TEXT_CONFIG, VIT_CONFIG
    pre = tower == "vit"
    enc = _encoder(VIT_CONFIG if pre else TEXT_CONFIG)
    layers, E, F, H = 12, 768, 3072, 12
    assert (enc.layers_num, enc.hidden_size, enc.heads_num) == (layers, E, H) and (enc.layernorm_positioning == "pre") == pre
    M = batch * L
    final = 4 * M * E + 8 * M + 8 * 256
    plain = layers * ((32 if pre else 40) * M * E + 8 * M * F + 16 * M + 4 * batch * H * L + 20 * 256) + final
    assert not enc.recompute
    assert enc.saved_activation_bytes(batch, L) == plain == enc.saved_activation_bytes(batch, L, recompute=False)
    rc = enc.saved_activation_bytes(batch, L, recompute=True)
    # each layer's input only (the post-LN input planes are re-split from it, not kept), the final LayerNorm's part, per-layer constants
    assert layers * 4 * M * E <= rc <= layers * (4 * M * E + 20 * 256) + final
    enc.recompute = True                                                # recompute=None: the encoder's own setting
    assert enc.saved_activation_bytes(batch, L) == rc and enc.saved_activation_bytes(batch, L, recompute=False) == plain
    # exactly: one [M, E] fp32 tensor per layer in a 256-byte aligned piece, and the final LayerNorm's two statistics (pre-LN)
    assert rc == layers * (4 * M * E + 256) + (8 * M + 8 * 256 if pre else 0)
    enc.recompute, enc.fp8_train = False, True                          # MX-FP8 keeps less than split-bf16, recompute the same few
    assert rc < enc.saved_activation_bytes(batch, L) < plain and enc.saved_activation_bytes(batch, L, recompute=True) == rc


def test_extractor_sums_the_two_towers():
    from lr2ppo_amd.finetune.features import TEXT_CONFIG, VIT_CONFIG, FeatureExtractor, encoder_args
    for rc in (False, True):
        fx = FeatureExtractor(encoder_args(VIT_CONFIG, layers_num=2), encoder_args(TEXT_CONFIG, layers_num=3), recompute=rc)
        assert fx.recompute == fx.image.encoder.recompute == fx.text.encoder.recompute == rc
        want = fx.image.encoder.saved_activation_bytes(4 * 16, 197) + fx.text.encoder.saved_activation_bytes(4 * 20, 196)
        assert fx.saved_activation_bytes((4, 16, 3, 224, 224), (4, 20, 196)) == want
    assert not FeatureExtractor(encoder_args(VIT_CONFIG, layers_num=1), encoder_args(TEXT_CONFIG, layers_num=1)).recompute


def _args(**kw):
    from lr2ppo_amd.finetune.features import raw_input_opts
    p = raw_input_opts(argparse.ArgumentParser())
    a = p.parse_args(["--raw_inputs"] + [f"--{k}" for k, v in kw.items() if v])
    a.seq_length, a.visual_feat_dim, a.device = 196, 768, "meta"
    return a


def test_recompute_flag_needs_finetune_encoders():
    from lr2ppo_amd.finetune.features import TEXT_CONFIG, VIT_CONFIG, FeatureExtractor, build_extractor, encoder_args
    assert _args(recompute_activations=True).recompute_activations and not _args().recompute_activations
    with pytest.raises(ValueError, match="finetune_encoders"):
        build_extractor(_args(recompute_activations=True), trainable=False)
    with pytest.raises(ValueError, match="inference"):
        FeatureExtractor(encoder_args(VIT_CONFIG, layers_num=1), encoder_args(TEXT_CONFIG, layers_num=1), precision="mxfp8",
                         recompute=True)
    fx = FeatureExtractor(encoder_args(VIT_CONFIG, layers_num=1), encoder_args(TEXT_CONFIG, layers_num=1), precision="mxfp8_train",
                          recompute=True)
    assert fx.image.encoder.recompute and fx.image.encoder.fp8_train
