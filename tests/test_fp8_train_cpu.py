"""MX-FP8 encoder training, the parts that need no GPU: the new C entry points reject bad arguments before launching anything, and
the --fp8_finetune flag's combinations."""
import argparse

import pytest


def test_entry_points_validate_before_launching():
    from lr2ppo_amd import _native as native
    lib = native.lib()
    A = 16          # a stand-in device address with the alignment the kernels need (nothing is dereferenced: every call fails)
    # lr2_quant_mxfp8_t: NULL input / outputs, cols not a multiple of 64, a row stride below cols, half of an optional pair
    assert lib.lr2_quant_mxfp8_t(None, 0, 0, 64, None, 0, 0, None, None, None, None, None, None, 0, 1, 64, None) == -1
    assert lib.lr2_quant_mxfp8_t(A, 0, 0, 64, None, 0, 0, None, None, None, None, None, None, 0, 1, 64, None) == -1   # no output
    assert lib.lr2_quant_mxfp8_t(A, 0, 0, 96, None, 0, 0, A, A, None, None, None, None, 0, 1, 96, None) == -2
    assert lib.lr2_quant_mxfp8_t(A, 0, 0, 64, None, 0, 0, A, A, None, None, None, None, 0, 1, 128, None) == -2
    assert lib.lr2_quant_mxfp8_t(A, 0, 0, 64, None, 0, 0, A, A, A, None, None, None, 0, 1, 64, None) == -1
    assert lib.lr2_quant_mxfp8_t(A, 0, 0, 64, None, 0, 0, A, None, A, A, None, None, 0, 1, 64, None) == -1
    assert lib.lr2_quant_mxfp8_t(A, 0, 0, 64, None, 0, 2, A, A, None, None, None, None, 0, 1, 64, None) == -1   # GELU' without z
    assert lib.lr2_quant_mxfp8_t(A, 0, 0, 64, None, 0, 3, A, A, None, None, None, None, 0, 1, 64, None) == -1
    # ... and misaligned vector operands: fp32 input / z / outputs off 16 bytes, planes off 8
    assert lib.lr2_quant_mxfp8_t(A + 4, 0, 0, 64, None, 0, 0, A, A, None, None, None, None, 0, 1, 64, None) == -2
    assert lib.lr2_quant_mxfp8_t(A + 4, 1, 0, 64, None, 0, 0, A, A, None, None, None, None, 0, 1, 64, None) == -2
    assert lib.lr2_quant_mxfp8_t(A, 0, 0, 64, A + 8, 64, 2, A, A, None, None, None, None, 0, 1, 64, None) == -2
    assert lib.lr2_quant_mxfp8_t(A, 0, 0, 64, None, 0, 0, A + 1, A, None, None, None, None, 0, 1, 64, None) == -2
    assert lib.lr2_quant_mxfp8_t(A, 0, 0, 64, None, 0, 0, None, None, A + 8, A, None, None, 0, 1, 64, None) == -2
    # lr2_gemm_mxfp8_wgrad: NULL operands, shapes off the 128 grid, a short leading dimension, several slices without a workspace,
    # misaligned destination / workspace
    assert lib.lr2_gemm_mxfp8_wgrad(None, None, None, None, None, 128, 0, None, 1, 128, 128, 128, None) == -1
    assert lib.lr2_gemm_mxfp8_wgrad(A, A, A, A, A, 128, 0, None, 1, 100, 128, 128, None) == -2
    assert lib.lr2_gemm_mxfp8_wgrad(A, A, A, A, A, 128, 0, None, 1, 128, 128, 200, None) == -2
    assert lib.lr2_gemm_mxfp8_wgrad(A, A, A, A, A, 64, 0, None, 1, 128, 128, 128, None) == -2
    assert lib.lr2_gemm_mxfp8_wgrad(A, A, A, A, A, 128, 0, None, 2, 128, 128, 256, None) == -1
    assert lib.lr2_gemm_mxfp8_wgrad(A, A, A, A, A, 128, 2, None, 1, 128, 128, 128, None) == -1
    assert lib.lr2_gemm_mxfp8_wgrad(A, A, A, A, A + 4, 128, 0, A, 2, 128, 128, 256, None) == -2
    assert lib.lr2_gemm_mxfp8_wgrad(A, A, A, A, A, 128, 0, A + 4, 2, 128, 128, 256, None) == -2
    # lr2_dropout_residual: NULL, p outside (0, 1), n not a multiple of 4, misaligned tensors
    assert lib.lr2_dropout_residual(None, None, None, 4, 0.1, 0, 0, None) == -1
    assert lib.lr2_dropout_residual(A, A, A, 4, 0.0, 0, 0, None) == -1
    assert lib.lr2_dropout_residual(A, A, A, 6, 0.1, 0, 0, None) == -2
    assert lib.lr2_dropout_residual(A, A + 4, A, 4, 0.1, 0, 0, None) == -2


def _args(**kw):
    from lr2ppo_amd.finetune.features import raw_input_opts
    p = raw_input_opts(argparse.ArgumentParser())
    a = p.parse_args(["--raw_inputs"] + [f"--{k}" for k, v in kw.items() if v])
    a.seq_length, a.visual_feat_dim, a.device = 196, 768, "meta"
    return a


def test_fp8_finetune_flag_needs_finetune_encoders():
    from lr2ppo_amd.finetune.features import FeatureExtractor, build_extractor
    assert _args(fp8_finetune=True).fp8_finetune and not _args().fp8_finetune
    with pytest.raises(ValueError, match="finetune_encoders"):
        build_extractor(_args(fp8_finetune=True), trainable=False)
    with pytest.raises(ValueError):
        build_extractor(_args(fp8_features=True), trainable=True)          # unchanged
    assert "mxfp8_train" in FeatureExtractor.PRECISIONS and "mxfp8" in FeatureExtractor.PRECISIONS
