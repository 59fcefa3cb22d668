"""Single-pass bf16 encoder training (FeatureExtractor(precision="bf16_train")), the parts that need no GPU: lr2_gemm_bf16_train rejects
bad arguments before launching anything, the --bf16_finetune flag's combinations, and the activation bookkeeping of the mode."""
import argparse
import ctypes

import pytest


def test_gemm_bf16_train_validates_before_launching():
    from lr2ppo_amd import _native as native
    lib = native.lib()
    A = 16          # a stand-in device address (nothing is dereferenced: every call fails)

    def epi(**kw):
        e = native.Epilogue()
        e.out, e.ld_out, e.alpha = A, 256, 1.0
        for k, v in kw.items():
            setattr(e, k, v)
        return ctypes.byref(e)

    def call(a, b, M, N, K, e, bm, *, t=0, tb=None, ws=None, splits=1, lda=None, ldb=None, a_bytes=None, b_bytes=None):
        tb = t if tb is None else tb
        lda = (M if t else K) if lda is None else lda
        ldb = (N if t else K) if ldb is None else ldb
        return lib.lr2_gemm_bf16_train(a, b, M, N, K, lda, ldb, t, tb, M * K * 2 if a_bytes is None else a_bytes,
                                       N * K * 2 if b_bytes is None else b_bytes, e, ws, splits, bm, None)

    before = (ctypes.c_uint64 * 3)()
    assert lib.lr2_gemm_bf16_train_launch_counts(before) == 0
    for t in (0, 1):
        assert call(None, None, 256, 256, 64, epi(), 256, t=t) == -1              # null operands
        assert call(A, None, 256, 256, 64, epi(), 256, t=t) == -1
        assert call(A, A, 256, 256, 64, None, 256, t=t) == -1                     # no epilogue
        assert call(A, A, 256, 256, 64, epi(out=None), 256, t=t) == -1            # no destination
        for bm in (256, 128):
            assert call(A, A, 256, 256, 64, epi(out=None, adam_p=A, adam_m=A, adam_v=A), bm, t=t) == -1   # the fused optimizer
            assert call(A, A, 256, 256, 64, epi(adam_p=A, adam_m=A, adam_v=A), bm, t=t) == -1
            assert call(A, A, 256, 256, 128, epi(), bm, t=t, splits=2) == -1      # several splits, no workspace
        # alignment and leading dimensions (lr2_gemm_bf16's rules), the 4 GiB limits
        assert call(A, A, 256, 256, 64, epi(), 256, t=t, lda=260) == -2
        assert call(A, A, 256, 256, 64, epi(), 256, t=t, ldb=260) == -2
        assert call(A, A, 256, 254, 64, epi(), 256, t=t, ldb=256) == -2           # N % 4
        assert call(A, A, 256, 256, 64, epi(ld_out=258), 256, t=t) == -2
        assert call(A, A, 256, 256, 64, epi(), 256, t=t, a_bytes=1 << 32) == -2
        assert call(A, A, 256, 256, 64, epi(), 128, t=t, b_bytes=1 << 32) == -2
    assert call(A, A, 256, 256, 64, epi(), 256, t=1, tb=0) == -1                  # (1,0) / (0,1) are not forms of the entry
    assert call(A, A, 256, 256, 64, epi(), 256, t=0, tb=1) == -1
    # the (0,0) form: GELU' needs its input; whole 64-deep K steps; leading dimensions of the epilogue's tensors
    assert call(A, A, 256, 256, 64, epi(act=2), 256) == -1
    assert call(A, A, 256, 256, 64, epi(act=2), 128) == -1
    assert call(A, A, 256, 256, 64, epi(act=3), 256) == -1
    assert call(A, A, 256, 256, 128, epi(act=2, aux_z=A, ld_aux=256), 128, ws=A, splits=2) == -1   # the exact-GELU' kernels take no split-K
    assert call(A, A, 256, 256, 64, epi(out_z=A, ld_z=256), 256) == -1            # a kept pre-activation without GELU
    assert call(A, A, 256, 256, 96, epi(), 256) == -2
    assert call(A, A, 256, 256, 32, epi(), 128) == -2
    assert call(A, A, 256, 256, 64, epi(act=2, aux_z=A, ld_aux=258), 256) == -2
    assert call(A, A, 256, 256, 64, epi(resid=A, ld_resid=258), 256) == -2
    assert call(A, A, 256, 256, 64, epi(act=1, out_z=A, ld_z=258), 256) == -2
    assert call(A, A, 256, 256, 64, epi(out_hi=A, ld_planes=258), 256) == -2
    assert call(A, A, 256, 256, 64, epi(colsum=A, colsum_ws=A), 256) == -1        # column sums belong to the weight-gradient form
    assert call(A, A, 256, 256, 64, epi(out=None, out_hi=A, ld_planes=256, accumulate=1), 256) == -1   # nothing to accumulate into
    # the (1,1) form: a plain epilogue, no accumulate, column sums need their workspace and M % 4
    assert call(A, A, 256, 256, 4096, epi(accumulate=1), 256, t=1) == -1
    assert call(A, A, 256, 256, 4096, epi(accumulate=1), 128, t=1) == -1
    assert call(A, A, 256, 256, 4096, epi(bias=A), 256, t=1) == -1
    assert call(A, A, 256, 256, 4096, epi(act=1), 256, t=1) == -1
    assert call(A, A, 256, 256, 4096, epi(drop_p=0.1), 256, t=1) == -1
    assert call(A, A, 256, 256, 4096, epi(resid=A, ld_resid=256), 256, t=1) == -1
    assert call(A, A, 256, 256, 4096, epi(out_hi=A, ld_planes=256), 256, t=1) == -1
    assert call(A, A, 256, 256, 4096, epi(colsum=A), 256, t=1) == -1
    assert call(A, A, 258, 256, 4096, epi(colsum=A, colsum_ws=A), 256, t=1, lda=264) == -2
    counts = (ctypes.c_uint64 * 3)()
    assert lib.lr2_gemm_bf16_train_launch_counts(counts) == 0 and list(counts) == list(before)      # nothing was launched
    assert lib.lr2_gemm_bf16_train_launch_counts(None) == -1


def _args(**kw):
    from lr2ppo_amd.finetune.features import raw_input_opts
    p = raw_input_opts(argparse.ArgumentParser())
    a = p.parse_args(["--raw_inputs"] + [f"--{k}" for k, v in kw.items() if v])
    a.seq_length, a.visual_feat_dim, a.device = 196, 768, "meta"
    return a


def test_bf16_finetune_flag():
    from lr2ppo_amd.finetune.features import FeatureExtractor, build_extractor
    assert "bf16_train" in FeatureExtractor.PRECISIONS and "bf16_train" not in FeatureExtractor.INFERENCE_ONLY
    assert _args(bf16_finetune=True).bf16_finetune and not _args().bf16_finetune
    with pytest.raises(ValueError, match="finetune_encoders"):
        build_extractor(_args(bf16_finetune=True), trainable=False)
    for other in ("fp8_finetune", "fp8_features", "bf16_features"):
        with pytest.raises(ValueError):
            build_extractor(_args(bf16_finetune=True, **{other: True}), trainable=True)
    with pytest.raises(ValueError):
        FeatureExtractor(precision="bf16_training")


def test_extractor_sets_the_mode_on_both_towers():
    from lr2ppo_amd.finetune.features import TEXT_CONFIG, VIT_CONFIG, FeatureExtractor, encoder_args
    fx = FeatureExtractor(encoder_args(VIT_CONFIG, layers_num=1), encoder_args(TEXT_CONFIG, layers_num=1), precision="bf16_train",
                          recompute=True)
    assert fx.image.encoder.bf16_train and fx.text.encoder.bf16_train and not fx.image.encoder.fp8_train
    assert fx.image.encoder.recompute and fx.text.encoder.recompute
    ref = FeatureExtractor(encoder_args(VIT_CONFIG, layers_num=1), encoder_args(TEXT_CONFIG, layers_num=1))
    assert not ref.image.encoder.bf16_train and not ref.text.encoder.bf16_train


@pytest.mark.parametrize("pre", [True, False], ids=["pre_ln", "post_ln"])
def test_saved_activation_bytes(pre):
    """The LayerNorm outputs (two [M, E] tensors per layer) and GELU(z) ([M, F]) are kept as ONE bf16 plane instead of hi / lo planes:
    2 bytes less per element, 4 M E + 2 M F per layer, either LayerNorm placement; nothing else changes."""
    from lr2ppo_amd.finetune.features import TEXT_CONFIG, VIT_CONFIG, encoder_args
    from lr2ppo_amd.tencentpretrain.encoders import str2encoder
    layers = 3
    enc = str2encoder["transformer"](encoder_args(VIT_CONFIG if pre else TEXT_CONFIG, layers_num=layers))
    E, F = enc.hidden_size, enc.transformer[0].feed_forward.linear_1.out_features
    B, L = 5, 197
    M = B * L
    split = enc.saved_activation_bytes(B, L)
    split_rc = enc.saved_activation_bytes(B, L, recompute=True)
    enc.bf16_train = True
    assert split - enc.saved_activation_bytes(B, L) == layers * (4 * M * E + 2 * M * F)
    assert enc.saved_activation_bytes(B, L, recompute=True) == split_rc        # each layer's fp32 input, whatever the precision


def test_tn_dispatch_rule():
    from lr2ppo_amd import ops
    # the encoders' weight gradients at the PPO sizes: few tiles, a long contraction -> one round of the chip
    for n_out, n_in in ((768, 3072), (3072, 768), (2304, 768), (768, 768)):
        for T in (100864, 12544):
            sp = ops.gemm256_tn_b1_splits(n_out, n_in, T)
            tiles = ((n_out + 255) // 256) * ((n_in + 255) // 256)
            assert sp == 0 or (1 <= sp and tiles * sp <= 256), (n_out, n_in, T, sp)
    assert ops.gemm256_tn_b1_splits(768, 768, 394) == 0           # a short contraction: the general family
    assert ops.bf16_train_tn_tiling(768, 768, 394)[0] in (64, 128)
    with ops.bf16_train_force_256():
        assert ops.bf16_train_tn_tiling(768, 768, 394) == (256, 1)
    assert ops.bf16_train_tn_tiling(768, 768, 394)[0] in (64, 128)
