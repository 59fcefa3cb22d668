"""The single-pass bf16 inference mode, the parts that need no GPU: the precision and its launcher flag, the combinations they refuse,
and lr2_gemm_bf16's argument checks (nothing is launched by a rejected call)."""
import argparse
import ctypes

import pytest
import torch


def _args(**kw):
    from lr2ppo_amd.finetune.features import raw_input_opts
    p = raw_input_opts(argparse.ArgumentParser())
    a = p.parse_args(["--raw_inputs"] + [f"--{k}" for k, v in kw.items() if v])
    a.seq_length, a.visual_feat_dim, a.device = 196, 768, "meta"
    return a


def test_bf16_is_a_precision_and_a_launcher_flag():
    from lr2ppo_amd.finetune.features import FeatureExtractor
    assert "bf16" in FeatureExtractor.PRECISIONS
    assert _args(bf16_features=True).bf16_features and not _args().bf16_features


@pytest.mark.parametrize("other, trainable", [("fp8_features", False), (None, True), ("fp8_finetune", True)])
def test_bf16_features_excludes_the_other_modes(other, trainable):
    from lr2ppo_amd.finetune.features import build_extractor
    kw = {"bf16_features": True}
    if other:
        kw[other] = True
    with pytest.raises(ValueError):
        build_extractor(_args(**kw), trainable=trainable)


def test_bf16_precision_refuses_recompute():
    from lr2ppo_amd.finetune.features import FeatureExtractor
    assert "bf16" in FeatureExtractor.PRECISIONS                # (an unknown precision is a ValueError too)
    with torch.device("meta"):
        with pytest.raises(ValueError, match="inference only"):
            FeatureExtractor(precision="bf16", recompute=True)


def test_gemm_bf16_validates_before_launching():
    from lr2ppo_amd import _native as native
    lib = native.lib()
    A = 16          # a stand-in device address (nothing is dereferenced: every call fails)

    def epi(**kw):
        e = native.Epilogue()
        e.out, e.ld_out, e.alpha = A, 256, 1.0
        for k, v in kw.items():
            setattr(e, k, v)
        return ctypes.byref(e)

    def call(a, b, M, N, K, e, bm):
        return lib.lr2_gemm_bf16(a, b, M, N, K, K, K, M * K * 2, N * K * 2, e, bm, None)

    before = (ctypes.c_uint64 * 2)()
    assert lib.lr2_gemm_bf16_launch_counts(before) == 0
    assert call(None, None, 256, 256, 64, epi(), 256) == -1                       # null operands
    assert call(A, None, 256, 256, 64, epi(), 256) == -1
    assert call(A, A, 256, 256, 64, None, 256) == -1                              # no epilogue
    assert call(A, A, 256, 256, 64, epi(out=None), 256) == -1                     # no destination
    # K must be whole 64-deep steps: neither the 256 x 256 kernel nor the 128- / 64-row family at one pass has another form
    assert call(A, A, 256, 256, 96, epi(), 256) == -2
    assert call(A, A, 256, 256, 32, epi(), 128) == -2
    # inference only
    assert call(A, A, 256, 256, 64, epi(drop_p=0.1), 256) == -1                   # dropout
    assert call(A, A, 256, 256, 64, epi(out=None, adam_p=A, adam_m=A, adam_v=A), 256) == -1   # the fused optimizer
    assert call(A, A, 256, 256, 64, epi(adam_p=A, adam_m=A, adam_v=A), 128) == -1
    assert call(A, A, 256, 256, 64, epi(act=2, aux_z=A, ld_aux=256), 256) == -1   # GELU'
    assert call(A, A, 256, 256, 64, epi(accumulate=1), 256) == -1
    assert call(A, A, 256, 256, 64, epi(colsum=A, colsum_ws=A), 256) == -1
    counts = (ctypes.c_uint64 * 2)()
    assert lib.lr2_gemm_bf16_launch_counts(counts) == 0 and list(counts) == list(before)      # nothing was launched
    assert lib.lr2_gemm_bf16_launch_counts(None) == -1


def test_default_dispatch_rule():
    from lr2ppo_amd import ops
    assert ops.use_gemm256_b1(100864, 3072, 768) and ops.use_gemm256_b1(100864, 768, 3072)   # the ViT token products at 512 frames
    assert ops.use_gemm256_b1(12544, 3072, 768)                   # 2.3 rounds: the row split
    assert ops.use_gemm256_b1(12544, 768, 3072) and ops.use_gemm256_b1(12544, 2304, 768)     # 147 / 441 tiles: measured ahead
    assert not ops.use_gemm256_b1(6304, 3072, 768) and not ops.use_gemm256_b1(6304, 768, 768)   # 300 / 75 tiles: 64-row tiles
    assert not ops.use_gemm256_b1(100864, 3072, 800)              # no whole 64-deep steps
    assert not ops.use_gemm256_b1(394, 768, 256)                  # a handful of tiles: the 128-row family
