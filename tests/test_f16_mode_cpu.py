"""The single-pass f16 inference mode, the parts that need no GPU: the precision and its launcher flag, the combinations they refuse,
and the argument checks of lr2_gemm_f16 / lr2_self_attn_fwd_f16 (nothing is launched, and nothing counted, by a rejected call)."""
import argparse
import ctypes
import os
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(**kw):
    from lr2ppo_amd.finetune.features import raw_input_opts
    p = raw_input_opts(argparse.ArgumentParser())
    a = p.parse_args(["--raw_inputs"] + [f"--{k}" for k, v in kw.items() if v])
    a.seq_length, a.visual_feat_dim, a.device = 196, 768, "meta"
    return a


def test_f16_is_a_precision_and_a_launcher_flag():
    from lr2ppo_amd.finetune.features import FeatureExtractor
    assert "f16" in FeatureExtractor.PRECISIONS and "f16" in FeatureExtractor.INFERENCE_ONLY
    assert _args(f16_features=True).f16_features and not _args().f16_features
    from lr2ppo_amd.finetune import pointwise, ppo, reward_pair_dataloader           # the flag is on all three launchers
    for mod in (pointwise, ppo, reward_pair_dataloader):
        assert "--f16_features" in mod.build_parser().format_help(), mod.__name__


@pytest.mark.parametrize("other, trainable", [("bf16_features", False), ("fp8_features", False), (None, True), ("fp8_finetune", True),
                                              ("bf16_finetune", True), ("fp8_finetune", False), ("bf16_finetune", False),
                                              ("features_attention_long", False)])
def test_f16_features_excludes_the_other_modes(other, trainable):
    from lr2ppo_amd.finetune.features import build_extractor
    kw = {"f16_features": True}
    if other:
        kw[other] = True
    with pytest.raises(ValueError):
        build_extractor(_args(**kw), trainable=trainable)


def test_f16_precision_refuses_recompute_and_attention_long():
    from lr2ppo_amd.finetune.features import FeatureExtractor
    with torch.device("meta"):
        with pytest.raises(ValueError, match="inference only"):
            FeatureExtractor(precision="f16", recompute=True)
        with pytest.raises(ValueError, match="key-blocked"):
            FeatureExtractor(precision="f16", attention_long=True)
        with pytest.raises(ValueError):
            FeatureExtractor(precision="f16", bf16_attention=True)
        fx = FeatureExtractor(precision="f16")
    with torch.no_grad():
        assert fx.precision == "f16" and fx.eval()._fast_now() == "forward_f16"
        with pytest.raises(NotImplementedError):                    # dropout: an inference mode
            fx.train()._fast_now()
    with pytest.raises(NotImplementedError):                        # gradients
        fx.eval()._fast_now()


def test_gemm_f16_validates_before_launching():
    from lr2ppo_amd import _native as native
    lib = native.lib()
    A = 16          # a stand-in device address (nothing is dereferenced: every call fails)

    def epi(**kw):
        e = native.Epilogue()
        e.out, e.ld_out, e.alpha = A, 256, 1.0
        for k, v in kw.items():
            setattr(e, k, v)
        return ctypes.byref(e)

    def call(a, b, M, N, K, e):
        return lib.lr2_gemm_f16(a, b, M, N, K, K, K, M * K * 2, N * K * 2, e, None)

    before = ctypes.c_uint64(0)
    assert lib.lr2_gemm_f16_launch_count(ctypes.byref(before)) == 0
    # lr2_gemm_bf16's status codes
    assert call(None, None, 256, 256, 64, epi()) == -1                       # null operands
    assert call(A, None, 256, 256, 64, epi()) == -1
    assert call(None, A, 256, 256, 64, epi()) == -1
    assert call(A, A, 256, 256, 64, None) == -1                              # no epilogue
    assert call(A, A, 256, 256, 64, epi(out=None)) == -1                     # no destination
    assert call(A, A, 256, 256, 96, epi()) == -2                             # K must be whole 64-deep steps
    assert call(A, A, 256, 256, 32, epi()) == -2
    assert call(A, A, 256, 254, 64, epi()) == -2                             # N % 4
    assert call(A, A, 256, 256, 64, epi(ld_out=128)) == -2                   # a leading dimension smaller than the row
    # inference only: every training epilogue request
    assert call(A, A, 256, 256, 64, epi(drop_p=0.1)) == -1                   # dropout
    assert call(A, A, 256, 256, 64, epi(out=None, adam_p=A, adam_m=A, adam_v=A)) == -1   # the fused optimizer
    assert call(A, A, 256, 256, 64, epi(adam_p=A, adam_m=A, adam_v=A)) == -1
    assert call(A, A, 256, 256, 64, epi(act=2, aux_z=A, ld_aux=256)) == -1   # GELU'
    assert call(A, A, 256, 256, 64, epi(accumulate=1)) == -1
    assert call(A, A, 256, 256, 64, epi(out_z=A, ld_z=256, act=1)) == -1     # the kept pre-activation
    assert call(A, A, 256, 256, 64, epi(colsum=A, colsum_ws=A)) == -1
    after = ctypes.c_uint64(0)
    assert lib.lr2_gemm_f16_launch_count(ctypes.byref(after)) == 0 and after.value == before.value      # nothing was launched
    assert lib.lr2_gemm_f16_launch_count(None) == -1


def test_self_attn_fwd_f16_validates_before_launching():
    from lr2ppo_amd import _native as native
    lib = native.lib()
    A = 16

    def call(q=A, k=A, v=A, seg=A, o32=A, o16=A, L=16, hd=64, ld=768, ld_o=256, batch=2, heads=4):
        return lib.lr2_self_attn_fwd_f16(q, k, v, ld, seg, o32, o16, ld_o, batch, heads, L, hd, 0.125, None)

    before = ctypes.c_uint64(0)
    assert lib.lr2_self_attn_fwd_f16_launch_count(ctypes.byref(before)) == 0
    assert call(L=289) == -2                                        # one LDS-resident head: 288 keys at most
    assert call(hd=32) == -2                                        # head width 64 only
    assert call(o32=None, o16=None) == -1                           # no output
    assert call(q=None) == -1 and call(k=None) == -1 and call(v=None) == -1 and call(seg=None) == -1
    assert call(L=0) == -1 and call(batch=0) == -1 and call(heads=0) == -1
    assert call(ld=772) == -2 and call(ld=128) == -2                # 16-byte rows; a row holds every head
    assert call(ld_o=128) == -2 and call(ld_o=258) == -2
    after = ctypes.c_uint64(0)
    assert lib.lr2_self_attn_fwd_f16_launch_count(ctypes.byref(after)) == 0 and after.value == before.value
    assert lib.lr2_self_attn_fwd_f16_launch_count(None) == -1


def test_layernorm_and_round_f16_validate_before_launching():
    from lr2ppo_amd import _native as native
    lib = native.lib()
    A = 64
    assert lib.lr2_layernorm_fwd_f16(A, A, A, None, None, None, None, 4, 768, 1e-6, 1, 0, 0, None) == -1       # no output
    assert lib.lr2_layernorm_fwd_f16(None, A, A, A, A, None, None, 4, 768, 1e-6, 1, 0, 0, None) == -1
    assert lib.lr2_layernorm_fwd_f16(A, A, A, A, A, None, None, 0, 768, 1e-6, 1, 0, 0, None) == -1
    assert lib.lr2_layernorm_fwd_f16(A, A, A, A, A, None, None, 4, 770, 1e-6, 1, 0, 0, None) == -2             # D % 4
    assert lib.lr2_layernorm_fwd_f16(A, A, A, A, A, None, None, 4, 2048, 1e-6, 1, 0, 0, None) == -2            # D <= 1024
    assert lib.lr2_round_f16(None, A, 64, None) == -1 and lib.lr2_round_f16(A, None, 64, None) == -1
    assert lib.lr2_round_f16(A, A, 0, None) == -1
    assert lib.lr2_round_f16(A, A, 66, None) == -2                  # whole groups of 4
    assert lib.lr2_round_f16(A + 4, A, 64, None) == -2 and lib.lr2_round_f16(A, A + 2, 64, None) == -2         # alignment


def test_abi_numbers_agree_and_the_tools_take_the_mode():
    import re

    from lr2ppo_amd import _native as native
    hdr = open(os.path.join(REPO, "include", "lr2ppo_hip.h")).read()
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert native.ABI_VERSION == 27 == int(re.search(r"#define LR2_ABI_VERSION (\d+)", hdr).group(1))
    assert int(re.search(r"lr2_abi_version\(\) == (\d+)", doc).group(1)) == 27 and native.lib().lr2_abi_version() == 27
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import encoder_bench
    a = encoder_bench.parse_args(["--ppo-shapes", "--precision", "f16", "--only", "text", "--text-seq", "128"])
    assert a.precision == "f16" and a.only == "text" and a.text_seq == 128
    for bad in (["--precision", "f16"], ["--ppo-shapes", "--precision", "f16", "--train"],
                ["--ppo-shapes", "--precision", "f16", "--attention-long"]):
        with pytest.raises(SystemExit):
            encoder_bench.parse_args(bad)
