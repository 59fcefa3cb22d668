"""The CPU half of the head-width suite (test_selfattn_hd_gpu.py, test_encoder_head_widths_gpu.py): the additive C ABI of
csrc/selfattn_hd.hip (three symbols inside ABI 27; header, SIGNATURES, SOURCES), the argument contract of
lr2_self_attn_hd_fwd / lr2_self_attn_hd_bwd (every refusal returns before anything is launched: nothing is dereferenced and the launch
counters stay), the routing of lr2ppo_amd.ops by head width, the free-width fp64 reference against tests/attn_cases.py's, and the
ViT-H/14 configuration behind --image_tower vit_huge_14_224."""
import ctypes
import os
import re

import pytest
import torch

import attn_cases as AC
import attn_hd_cases as HC
from conftest import REPO

from lr2ppo_amd import _native as native

A = 64          # a stand-in device address (nothing is dereferenced: every call below is refused, or stubbed)
ARG, SHAPE = -1, -2
NEW_SYMBOLS = ("lr2_self_attn_hd_fwd", "lr2_self_attn_hd_bwd", "lr2_self_attn_hd_launch_counts")
SERVED = (32, 48, 64, 80, 96, 112, 128)
REFUSED = (16, 24, 40, 136, 144)


@pytest.fixture(scope="module")
def lib():
    return native.lib()


def _counts(lib):
    c = (ctypes.c_uint64 * 2)()
    assert lib.lr2_self_attn_hd_launch_counts(c) == 0
    return int(c[0]), int(c[1])


def _decl_args(header, name):
    """Number of parameters of `int name(...)` in the header."""
    m = re.search(r"\bint %s\(([^;]*?)\);" % name, header, re.S)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_abi_stays_27_and_the_new_names_are_everywhere(lib):
    header = open(os.path.join(REPO, "include", "lr2ppo_hip.h")).read()
    assert native.ABI_VERSION == 27 and re.search(r"#define LR2_ABI_VERSION 27\b", header) and lib.lr2_abi_version() == 27
    integration = open(os.path.join(REPO, "INTEGRATION.md")).read()
    src = open(os.path.join(native.CSRC, "selfattn_hd.hip")).read()
    assert "selfattn_hd.hip" in native.SOURCES
    for name in NEW_SYMBOLS:
        assert name in native.SIGNATURES and name in integration, name
        assert re.search(r'extern "C" int %s\(' % name, src), name
        assert hasattr(lib, name)
        assert _decl_args(header, name) == len(native.SIGNATURES[name]), name
    # the argument lists of the 64-column twins
    assert native.SIGNATURES["lr2_self_attn_hd_fwd"] == native.SIGNATURES["lr2_self_attn_fwd"]
    assert native.SIGNATURES["lr2_self_attn_hd_bwd"] == native.SIGNATURES["lr2_self_attn_bwd"]
    assert _decl_args(header, "lr2_self_attn_hd_fwd") == _decl_args(header, "lr2_self_attn_fwd")
    assert _decl_args(header, "lr2_self_attn_hd_bwd") == _decl_args(header, "lr2_self_attn_bwd")


def _fwd(lib, *, q=A, k=A, v=A, lo_off=1024, ld=384, seg=A, o=A, o_hi=None, o_lo_off=0, ld_o=128, lse=None, p=0.0, batch=2, heads=2,
         L=17, hd=80):
    return lib.lr2_self_attn_hd_fwd(q, k, v, lo_off, ld, seg, o, o_hi, o_lo_off, ld_o, lse, p, 0, 0, batch, heads, L, hd, 0.125, None)


def _bwd(lib, *, q=A, k=A, v=A, lo_off=1024, ld=384, do=A, do_lo_off=1024, ld_do=128, seg=A, dq=A, dk=A, dv=A, d_lo_off=1024, ld_d=384,
         o=None, o_lo_off=0, ld_o=0, ws=A, ws2=A, p=0.0, batch=2, heads=2, L=17, hd=80):
    return lib.lr2_self_attn_hd_bwd(q, k, v, lo_off, ld, do, do_lo_off, ld_do, seg, dq, dk, dv, d_lo_off, ld_d, o, o_lo_off, ld_o, ws, ws2,
                                    p, 0, 0, batch, heads, L, hd, 0.125, None)


def test_refusals_return_before_any_launch(lib):
    assert lib.lr2_self_attn_hd_launch_counts(None) == ARG
    before = _counts(lib)
    for call in (_fwd, _bwd):
        for hd in REFUSED + (0, -80, 72, 256):
            assert call(lib, hd=hd) == SHAPE, hd
        assert call(lib, L=0) == ARG and call(lib, L=-3) == ARG
        assert call(lib, batch=0) == ARG and call(lib, heads=0) == ARG
        assert call(lib, p=1.0) == ARG and call(lib, p=-0.1) == ARG and call(lib, p=float("nan")) == ARG
        for name in ("q", "k", "v", "seg"):
            assert call(lib, **{name: None}) == ARG, name
        # the alignment rules of the 64-column twins
        assert call(lib, ld=388) == SHAPE and call(lib, lo_off=1028) == SHAPE
    assert _fwd(lib, o=None, o_hi=None) == ARG                                      # neither output
    assert _fwd(lib, ld_o=130) == SHAPE and _fwd(lib, o=None, o_hi=A, o_lo_off=1026) == SHAPE
    for name in ("do", "dq", "dk", "dv", "ws", "ws2"):
        assert _bwd(lib, **{name: None}) == ARG, name
    assert _bwd(lib, ld_do=132) == SHAPE and _bwd(lib, ld_d=388) == SHAPE
    assert _bwd(lib, do_lo_off=1028) == SHAPE and _bwd(lib, d_lo_off=1028) == SHAPE
    assert _bwd(lib, o=A, ld_o=132, o_lo_off=1024) == SHAPE and _bwd(lib, o=A, ld_o=128, o_lo_off=1028) == SHAPE
    # the twins keep their range: the new pair is an addition, not a widening
    assert lib.lr2_self_attn_fwd(A, A, A, 1024, 384, A, A, None, 0, 128, None, 0.0, 0, 0, 2, 2, 17, 80, 0.125, None) == SHAPE
    assert lib.lr2_self_attn_bwd(A, A, A, 1024, 384, A, 1024, 128, A, A, A, A, 1024, 384, None, 0, 0, A, A, 0.0, 0, 0, 2, 2, 17, 80,
                                 0.125, None) == SHAPE
    assert _counts(lib) == before, "a refused call moved a launch counter"


class _Recorder:
    """Stands in for the loaded library: records the entry point a call names and accepts it."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append(name)
            return 0
        return fn


class _FakePlanes:
    def __init__(self, rows, cols):
        self.rows, self.cols, self.lo_off = rows, cols, rows * cols

    def data_ptr(self):
        return A


@pytest.mark.parametrize("hd,fwd,bwd", [(64, "lr2_self_attn_fwd", "lr2_self_attn_bwd"), (16, "lr2_self_attn_fwd", "lr2_self_attn_bwd"),
                                        (40, "lr2_self_attn_fwd", "lr2_self_attn_bwd"), (144, "lr2_self_attn_fwd", "lr2_self_attn_bwd")]
                         + [(w, "lr2_self_attn_hd_fwd", "lr2_self_attn_hd_bwd") for w in SERVED if w != 64])
def test_ops_routes_by_head_width(monkeypatch, hd, fwd, bwd):
    """64 and every width the new pair does not serve go to the 64-column entry points (which refuse all but 64: width 16 keeps raising),
    the served widths to the new ones."""
    from lr2ppo_amd import ops
    rec = _Recorder()
    monkeypatch.setattr(ops._nat, "lib", lambda: rec)
    monkeypatch.setattr(ops, "Planes", _FakePlanes)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(ops, "_chk_f32", lambda *ts: None)          # "a float32 HIP tensor": there is no device here
    B, H, L = 2, 3, 5
    E = H * hd
    seg = torch.ones(B * L, dtype=torch.int64)
    ws = torch.zeros(B * H * L)
    qkv, o, do, dqkv = _FakePlanes(B * L, 3 * E), _FakePlanes(B * L, E), _FakePlanes(B * L, E), _FakePlanes(B * L, 3 * E)
    ops.self_attn_fwd(qkv, seg, o, batch=B, heads=H, L=L, head_dim=hd, scale=0.1)
    ops.self_attn_bwd(qkv, do, seg, dqkv, ws, ws, batch=B, heads=H, L=L, head_dim=hd, scale=0.1)
    assert rec.calls == [fwd, bwd]


def test_free_width_reference_equals_attn_cases_at_64():
    B, H, L = 2, 2, 37
    c = HC.random_case(B, H, L, 64, seed=3)
    seg = AC.masks(B, L, 64)["suffix"]
    assert torch.equal(seg, HC.suffix_seg(B, L))
    keep = torch.rand(B, H, L, L, generator=torch.Generator().manual_seed(4)) > 0.1
    a = AC.reference(c["q"], c["k"], c["v"], seg, 0.125, keep=keep.numpy(), p=0.1, do=c["do"])
    b = HC.reference(c["q"], c["k"], c["v"], seg, 0.125, keep=keep.numpy(), p=0.1, do=c["do"])
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    m = HC.pack(c["q"], c["k"], c["v"])
    assert torch.equal(m, AC.pack(c["q"], c["k"], c["v"]))
    for x, y in zip(HC.unpack(m, B, H, L, 64), (c["q"], c["k"], c["v"])):
        assert torch.equal(x, y)
    # at another width: head h of part j sits in columns j E + h hd ..
    c = HC.random_case(B, 3, 5, 80, seed=5)
    m = HC.pack(c["q"], c["k"])
    assert m.shape == (B * 5, 2 * 240) and torch.equal(m[5 + 2, 240 + 80:240 + 160], c["k"][1, 1, 2])


def test_vit_huge_config_and_projection():
    from lr2ppo_amd.finetune.features import IMAGE_TOWERS, TEXT_CONFIG, FeatureExtractor, encoder_args
    a = encoder_args(IMAGE_TOWERS["vit_huge_14_224"])
    assert (a.hidden_size, a.emb_size, a.heads_num, a.layers_num, a.feedforward_size) == (1280, 1280, 16, 32, 5120)
    assert a.hidden_size // a.heads_num == 80 and a.hidden_size % a.heads_num == 0
    assert a.patch_size == 14 and a.image_height == a.image_width == 224
    assert a.max_seq_length == (224 // 14) ** 2 + 1 == 257
    assert a.layernorm_positioning == "pre" and a.remove_embedding_layernorm and a.embedding == ["patch", "pos"]
    large = encoder_args(IMAGE_TOWERS["vit_large_14_224"])
    assert set(vars(a)) == set(vars(large))                                       # the shape of the ViT-L/14 file
    fx = FeatureExtractor(encoder_args(IMAGE_TOWERS["vit_huge_14_224"], layers_num=1), encoder_args(TEXT_CONFIG, layers_num=1))
    assert fx.visual_projection is not None
    assert (fx.visual_projection.in_features, fx.visual_projection.out_features) == (1280, 768)
    assert tuple(fx.visual_projection.weight.shape) == (768, 1280)


def test_image_tower_flag_on_the_three_launchers():
    from lr2ppo_amd.finetune import pointwise, ppo, reward_pair_dataloader
    for mod in (pointwise, reward_pair_dataloader, ppo):
        parser = mod.build_parser()
        assert "vit_huge_14_224" in parser.format_help(), mod.__name__
        a = parser.parse_args(["--config_path", "c.json", "--output_model_path", "o.bin", "--raw_inputs", "--image_tower",
                               "vit_huge_14_224"])
        assert a.image_tower == "vit_huge_14_224"


def test_wide_layernorm_entries_and_the_narrow_refusal(lib):
    """lr2_layernorm_fwd_wide / lr2_layernorm_bwd_wide (ViT-H/14's 1280-wide rows) carry their twins' argument lists; the twins keep
    refusing D > 1024, the wide pair refuses D > 1536 -- all before any launch."""
    header = open(os.path.join(REPO, "include", "lr2ppo_hip.h")).read()
    integration = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for wide, narrow in (("lr2_layernorm_fwd_wide", "lr2_layernorm_fwd"), ("lr2_layernorm_bwd_wide", "lr2_layernorm_bwd")):
        assert native.SIGNATURES[wide] == native.SIGNATURES[narrow] and wide in integration
        assert _decl_args(header, wide) == _decl_args(header, narrow) == len(native.SIGNATURES[wide])

    def fwd(name, D, rows=4, x=A):
        return getattr(lib, name)(x, A, A, A, None, 0, A, A, rows, D, 1e-6, 1, 0, 0, None)

    def bwd(name, D, rows=4, dy=A):
        return getattr(lib, name)(dy, 0, 0, A, A, A, A, None, A, None, 0, 0.0, 0, 0, None, A, 8, rows, D, 1, 1e-6, None)

    for call, narrow, wide in ((fwd, "lr2_layernorm_fwd", "lr2_layernorm_fwd_wide"), (bwd, "lr2_layernorm_bwd", "lr2_layernorm_bwd_wide")):
        for D in (1028, 1280, 1536, 2048):
            assert call(narrow, D) == SHAPE, D
        for D in (1540, 2048, 1282, 0, -4):
            assert call(wide, D) == SHAPE, D
        assert call(wide, 1280, rows=0) == ARG
    assert fwd("lr2_layernorm_fwd_wide", 1280, x=None) == ARG and bwd("lr2_layernorm_bwd_wide", 1280, dy=None) == ARG
