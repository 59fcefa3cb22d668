"""Single-pass bf16 encoder training (FeatureExtractor(precision="bf16_train")): the 256 x 256 TN weight-gradient kernel
(csrc/gemm256_tn_b1.hip) on exact and random data, the training epilogues on the 256 x 256 NT kernel (csrc/gemm256_b1.hip through
lr2_gemm_bf16_train), the schedule's gradients against split-bf16 and against a torch emulation of its rounding points, and the
FeatureExtractor routes."""
import argparse
import importlib.util
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def _plane(x):
    """fp32 values that ARE bf16 numbers -> the int16 plane"""
    return x.to(torch.bfloat16).view(torch.int16).contiguous()


def _bf16(x):
    return x.to(torch.bfloat16).float()


# ---- 1. the TN kernel on exact data -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_out, n_in, T, splits", [
    (256, 256, 64, 1),            # one K step
    (256, 256, 96, 1),            # the second k-half of the last (only) step wholly out of range
    (256, 512, 4096, 1), (256, 512, 4096, 3), (256, 512, 4096, 7),      # 64 steps: 22 + 22 + 20, 10 x 6 + 4; tiles_n = 2
    (200, 328, 4100, 1), (200, 328, 4100, 5),                            # all three extents ragged
])
def test_tn_kernel_exact(dev, n_out, n_in, T, splits):
    from lr2ppo_amd import ops
    g = torch.Generator().manual_seed(n_out + n_in + T)
    a = torch.randint(-4, 5, (T, n_out), generator=g).float().to(dev)
    b = torch.randint(-4, 5, (T, n_in), generator=g).float().to(dev)
    want = a.double().t() @ b.double()                  # |sum| <= 16 T < 2^24: exact in fp32 whatever the order
    want_cs = a.double().sum(0)
    a_p, b_p = _plane(a), _plane(b)
    nan = float("nan")
    outs = []
    for _ in range(2):
        out = torch.full((n_out, n_in), nan, device=dev)
        cs = torch.full((n_out,), nan, device=dev)
        ws = torch.full((max(1, splits) * n_out * n_in,), nan, device=dev)
        cs_ws = torch.full((max(128, splits * ((n_in + 255) // 256)) * n_out,), nan, device=dev)
        c0 = ops.gemm_bf16_train_launch_counts()
        ops.gemm_bf16_train(a_p, b_p, out, n_out, n_in, T, trans=True, block_m=256, splits=splits, splitk_ws=ws, colsum=cs,
                            colsum_ws=cs_ws)
        c1 = ops.gemm_bf16_train_launch_counts()
        assert (c1[0] - c0[0], c1[1] - c0[1], c1[2] - c0[2]) == (0, 1, 0)          # the 256 x 256 TN kernel, nothing else
        outs.append((out, cs))
    out, cs = outs[0]
    assert torch.equal(out.double(), want)
    assert torch.equal(cs.double(), want_cs)
    assert torch.equal(out.view(torch.int32), outs[1][0].view(torch.int32)) and torch.equal(cs.view(torch.int32), outs[1][1].view(torch.int32))


# ---- 2. the TN kernel on random data -----------------------------------------------------------------------------------------------
def test_tn_kernel_random(dev):
    """|error| <= T * 2^-24 * sum_k |a_k b_k| against the fp64 product of the planes (every bf16 x bf16 product is exact in fp32; T
    fp32 additions of at most half an ulp of a partial sum that never exceeds sum |a_k b_k|) -- the bound tests/test_bf16_mode_gpu.py
    uses for the NT product."""
    from lr2ppo_amd import ops
    n_out, n_in, T = 768, 256, 12544
    g = torch.Generator().manual_seed(5)
    a = _bf16(torch.randn(T, n_out, generator=g)).to(dev)
    b = _bf16(torch.randn(T, n_in, generator=g)).to(dev)
    want = a.double().t() @ b.double()
    bound = T * 2.0 ** -24 * (a.double().abs().t() @ b.double().abs())
    a_p, b_p = _plane(a), _plane(b)
    sp = ops.gemm256_tn_b1_splits(n_out, n_in, T)
    assert sp >= 1 and ops.bf16_train_tn_tiling(n_out, n_in, T) == (256, sp)      # the shipped rule sends this shape to the kernel
    out, cs = torch.full((n_out, n_in), float("nan"), device=dev), torch.full((n_out,), float("nan"), device=dev)
    ws, cs_ws = torch.empty(sp * n_out * n_in, device=dev), torch.empty(max(128, sp) * n_out, device=dev)
    c0 = ops.gemm_bf16_train_launch_counts()
    ops.gemm_bf16_train(a_p, b_p, out, n_out, n_in, T, trans=True, splitk_ws=ws, colsum=cs, colsum_ws=cs_ws)      # the rule's own tiling
    assert ops.gemm_bf16_train_launch_counts()[1] == c0[1] + 1
    err = (out.double() - want).abs()
    print(f"\n[TN 256 x 256, splits {sp}] worst |error| / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    cs_bound = T * 2.0 ** -24 * a.double().abs().sum(0)
    assert bool(((cs.double() - a.double().sum(0)).abs() <= cs_bound).all())
    # the 128-row family at passes = 1 on the same planes
    bm, sp2 = ops._general_tiling(n_out, n_in, T, True, True)
    ref, cs2 = torch.full((n_out, n_in), float("nan"), device=dev), torch.full((n_out,), float("nan"), device=dev)
    ops.gemm_bf16_train(a_p, b_p, ref, n_out, n_in, T, trans=True, block_m=bm, splits=sp2, splitk_ws=torch.empty(sp2 * n_out * n_in, device=dev),
                        colsum=cs2, colsum_ws=cs_ws)
    assert ops.gemm_bf16_train_launch_counts()[2] == c0[2] + 1
    assert bool(((out.double() - ref.double()).abs() <= 2 * bound).all())
    assert bool(((cs2.double() - a.double().sum(0)).abs() <= cs_bound).all())


# ---- 3. the training epilogues on the 256 x 256 NT kernel ---------------------------------------------------------------------------
def _nt_case(dev, M, N, K=128):
    g = torch.Generator().manual_seed(M + N)
    a = _bf16(torch.randn(M, K, generator=g)).to(dev)
    b = _bf16(torch.randn(N, K, generator=g) * 0.1).to(dev)
    bias = torch.randn(N, generator=g).to(dev) * 0.1
    resid = torch.randn(M, N, generator=g).to(dev)
    z = torch.randn(M, N, generator=g).to(dev)
    return _plane(a), _plane(b), bias, resid, z


def _counts_delta(ops, c0):
    c1 = ops.gemm_bf16_train_launch_counts()
    return tuple(x - y for x, y in zip(c1, c0))


SHAPES = [(512, 256), (300, 260)]          # interior slabs (the per-slab fast forms, where there are any) / edge slabs


@pytest.mark.parametrize("bm", [256, 64])
@pytest.mark.parametrize("M, N", SHAPES)
def test_epilogue_dropout_residual(dev, M, N, bm):
    """(i) residual + dropout(product + bias): the zero pattern is ops.dropout_planes' on an all-ones [M, N] matrix with the same seed
    and site; a kept element is the undropped product x 1 / (1 - p) (+ the residual), within one fp32 rounding."""
    from lr2ppo_amd import ops
    K = 128
    a, b, bias, resid, _ = _nt_case(dev, M, N)
    plain = torch.full((M, N), float("nan"), device=dev)
    c0 = ops.gemm_bf16_train_launch_counts()
    ops.gemm_bf16_train(a, b, plain, M, N, K, bias=bias, block_m=bm)
    assert _counts_delta(ops, c0) == ((1, 0, 0) if bm == 256 else (0, 0, 1))
    drop = ops.Drop(0.1, 991, 7)
    got = torch.full((M, N), float("nan"), device=dev)
    ops.gemm_bf16_train(a, b, got, M, N, K, bias=bias, resid=resid, drop=drop, block_m=bm)
    keep = ops.dropout_planes(torch.ones(M, N, device=dev), ops.Planes.empty(M, N, dev), drop).to_float() != 0
    assert 0.85 < float(keep.float().mean()) < 0.95
    assert torch.equal(got[~keep], resid[~keep])                         # a dropped element: the residual alone
    one = torch.ones((), dtype=torch.float32, device=dev)
    scale = one / (one - torch.tensor(0.1, dtype=torch.float32, device=dev))       # the kernel's 1.0f / (1.0f - p)
    want = plain * scale + resid
    ulp = torch.maximum(want.abs(), (plain * scale).abs()) * 2.0 ** -23
    assert bool(((got - want).abs()[keep] <= ulp[keep]).all())
    # no residual: exact zeros where dropped
    got2 = torch.full((M, N), float("nan"), device=dev)
    ops.gemm_bf16_train(a, b, got2, M, N, K, bias=bias, drop=drop, block_m=bm)
    assert torch.equal(got2 != 0, keep & (plain != 0))


@pytest.mark.parametrize("bm", [256, 64])
@pytest.mark.parametrize("M, N", SHAPES)
def test_epilogue_kept_preactivation_and_gelu_plane(dev, M, N, bm):
    """(ii) FFN-1: out_z is the act = 0 product bit for bit; the ONE plane is round-to-nearest-even of the GELU the same kernel writes
    as fp32."""
    from lr2ppo_amd import ops
    K = 128
    a, b, bias, _, _ = _nt_case(dev, M, N)
    plain, z = torch.full((M, N), float("nan"), device=dev), torch.full((M, N), float("nan"), device=dev)
    plane = torch.full((M * N,), -1, dtype=torch.int16, device=dev)
    g32 = torch.full((M, N), float("nan"), device=dev)
    ops.gemm_bf16_train(a, b, plain, M, N, K, bias=bias, block_m=bm)
    ops.gemm_bf16_train(a, b, None, M, N, K, bias=bias, act=1, out_z=z, out_plane=plane, block_m=bm)
    ops.gemm_bf16_train(a, b, g32, M, N, K, bias=bias, act=1, block_m=bm)
    assert torch.equal(z.view(torch.int32), plain.view(torch.int32))
    assert torch.equal(plane.view(M, N), g32.to(torch.bfloat16).view(torch.int16))


@pytest.mark.parametrize("bm", [256, 64])
@pytest.mark.parametrize("M, N", SHAPES)
def test_epilogue_residual_and_planes(dev, M, N, bm):
    """(iv) residual -> fp32 AND hi / lo planes: the planes are split_planes of the fp32 output; ONE plane is its hi plane."""
    from lr2ppo_amd import ops
    K = 128
    a, b, bias, resid, _ = _nt_case(dev, M, N)
    out = torch.full((M, N), float("nan"), device=dev)
    pl = ops.Planes(torch.full((2 * M * N,), -1, dtype=torch.int16, device=dev), M, N)
    ops.gemm_bf16_train(a, b, out, M, N, K, bias=bias, resid=resid, out_planes=pl, block_m=bm)
    plain = torch.full((M, N), float("nan"), device=dev)
    ops.gemm_bf16_train(a, b, plain, M, N, K, bias=bias, block_m=bm)
    assert bool(((out - (plain + resid)).abs() <= (plain + resid).abs() * 2.0 ** -23).all())
    want = ops.split_planes(out, ops.Planes.empty(M, N, dev))
    assert torch.equal(pl.buf[:2 * M * N], want.buf[:2 * M * N])
    # planes alone (QKV in front of the 3-pass attention), and ONE plane
    pl2 = ops.Planes(torch.full((2 * M * N,), -1, dtype=torch.int16, device=dev), M, N)
    ops.gemm_bf16_train(a, b, None, M, N, K, bias=bias, out_planes=pl2, block_m=bm)
    want2 = ops.split_planes(plain, ops.Planes.empty(M, N, dev))
    assert torch.equal(pl2.buf[:2 * M * N], want2.buf[:2 * M * N])
    one = torch.full((M * N,), -1, dtype=torch.int16, device=dev)
    ops.gemm_bf16_train(a, b, None, M, N, K, bias=bias, out_plane=one, block_m=bm)
    assert torch.equal(one, want2.buf[:M * N])


def _gelu_grad64(z):
    z = z.double()
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


@pytest.mark.parametrize("bm", [256, 64])
@pytest.mark.parametrize("M, N", SHAPES)
def test_epilogue_gelu_grad(dev, M, N, bm):
    """(iii) FFN-2 input gradient: product x GELU'(aux_z) within 2 ulp of the fp64 evaluation, rounded; hi / lo planes and ONE plane of it.
    GELU' is an O(1) factor (-0.13 .. 1.13), so an ulp here is the fp32 spacing at max(|expected|, |product|).  lr2_gemm_bf16_train's
    act == 2 kernels form x * GELU'(z) in fp64 with one rounding (gemm_common.h::mul_gelu_grad_exact): gelu_erf_grad of the other paths
    is up to 2.7 x 2^-23 from the exact GELU' (erf_fast) and measured 2.25-2.37 ulp here."""
    from lr2ppo_amd import ops
    K = 128
    a, b, _, _, z = _nt_case(dev, M, N)
    plain, got = torch.full((M, N), float("nan"), device=dev), torch.full((M, N), float("nan"), device=dev)
    ops.gemm_bf16_train(a, b, plain, M, N, K, block_m=bm)
    pl = ops.Planes(torch.full((2 * M * N,), -1, dtype=torch.int16, device=dev), M, N)
    ops.gemm_bf16_train(a, b, got, M, N, K, act=2, aux_z=z, out_planes=pl, block_m=bm)
    one = torch.full((M * N,), -1, dtype=torch.int16, device=dev)
    ops.gemm_bf16_train(a, b, None, M, N, K, act=2, aux_z=z, out_plane=one, block_m=bm)
    want_pl = ops.split_planes(got, ops.Planes.empty(M, N, dev))
    assert torch.equal(pl.buf[:2 * M * N], want_pl.buf[:2 * M * N]) and torch.equal(one, want_pl.buf[:M * N])
    want = (plain.double() * _gelu_grad64(z)).float()
    ulp = torch.maximum(want.abs(), plain.abs()) * 2.0 ** -23
    worst = float(((got - want).abs() / ulp.clamp_min(1e-45)).max())
    print(f"\n[act = 2, {M} x {N}, block_m {bm}] worst |error| {worst:.2f} ulp")
    assert worst <= 2.0


@pytest.mark.parametrize("M, N", SHAPES)
def test_epilogue_gelu_grad_same_bits_on_both_kernel_families(dev, M, N):
    """The 256 x 256 kernel's per-element epilogue and the general family's apply the same function in the same order."""
    from lr2ppo_amd import ops
    K = 128
    a, b, bias, resid, z = _nt_case(dev, M, N)
    for kw in (dict(act=2, aux_z=z), dict(bias=bias, act=1), dict(bias=bias, resid=resid, drop=ops.Drop(0.1, 5, 3))):
        outs = []
        for bm in (256, 64):
            o = torch.full((M, N), float("nan"), device=dev)
            ops.gemm_bf16_train(a, b, o, M, N, K, block_m=bm, **kw)
            outs.append(o)
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), sorted(kw)


# ---- 4. gradients against split-bf16 -----------------------------------------------------------------------------------------------
def _small_encoder(pre, dev, seed, layers=2):
    from lr2ppo_amd.finetune.features import TEXT_CONFIG, VIT_CONFIG, encoder_args
    from lr2ppo_amd.tencentpretrain.encoders import str2encoder
    a = encoder_args(VIT_CONFIG if pre else TEXT_CONFIG, layers_num=layers, hidden_size=256, emb_size=256, feedforward_size=1024, heads_num=4,
                     dropout=0.1)
    g = torch.Generator().manual_seed(seed)
    enc = str2encoder["transformer"](a)
    for n, p in enc.named_parameters():
        if "gamma" in n:
            p.data.uniform_(0.8, 1.2, generator=g)
        else:
            p.data.normal_(0, 0.05, generator=g)
    return enc.to(dev).train()


def _grads(enc, bf16, emb, seg, dout):
    from lr2ppo_amd import runtime
    enc.bf16_train = bf16
    runtime.set_dropout_seed(1234)
    out, saved = enc._forward_train(emb, seg)
    demb, G = enc._backward_train(saved, dout)
    return out, demb.clone(), {n: G[p].clone() for n, p in enc.named_parameters()}


# relative L2 distance of bf16_train from split_bf16, measured on one MI355X with the inputs below (pre-LN, post-LN), the larger of the
# run forced to the 256 x 256 kernels and the run with the dispatch as shipped: the gates are 1.5 x these, floored at 1e-3
# (the print resolution of a 0.0000).  The key bias's true gradient is 0: measured against the query bias's gradient.
MEASURED = {
    "output": (0.0029, 0.0032),
    "d_emb": (0.0034, 0.0037),
    "transformer.0.self_attn.linear_layers.0.weight": (0.0059, 0.0062),
    "transformer.0.self_attn.linear_layers.0.bias": (0.0058, 0.0062),
    "transformer.0.self_attn.linear_layers.1.weight": (0.0058, 0.0062),
    "transformer.0.self_attn.linear_layers.1.bias": (0.0015, 0.0014),
    "transformer.0.self_attn.linear_layers.2.weight": (0.0051, 0.0053),
    "transformer.0.self_attn.linear_layers.2.bias": (0.0042, 0.0043),
    "transformer.0.self_attn.final_linear.weight": (0.0047, 0.0052),
    "transformer.0.self_attn.final_linear.bias": (0.0036, 0.0041),
    "transformer.0.feed_forward.linear_1.weight": (0.0044, 0.0046),
    "transformer.0.feed_forward.linear_1.bias": (0.0042, 0.0044),
    "transformer.0.feed_forward.linear_2.weight": (0.0041, 0.0043),
    "transformer.0.feed_forward.linear_2.bias": (0.0031, 0.0032),
    "transformer.0.layer_norm_1.gamma": (0.0055, 0.0038),
    "transformer.0.layer_norm_1.beta": (0.0043, 0.0041),
    "transformer.0.layer_norm_2.gamma": (0.0046, 0.0031),
    "transformer.0.layer_norm_2.beta": (0.0042, 0.0029),
    "transformer.1.self_attn.linear_layers.0.weight": (0.0064, 0.0069),
    "transformer.1.self_attn.linear_layers.0.bias": (0.0052, 0.0062),
    "transformer.1.self_attn.linear_layers.1.weight": (0.0063, 0.0068),
    "transformer.1.self_attn.linear_layers.1.bias": (0.0014, 0.0015),
    "transformer.1.self_attn.linear_layers.2.weight": (0.0040, 0.0040),
    "transformer.1.self_attn.linear_layers.2.bias": (0.0034, 0.0031),
    "transformer.1.self_attn.final_linear.weight": (0.0042, 0.0042),
    "transformer.1.self_attn.final_linear.bias": (0.0030, 0.0029),
    "transformer.1.feed_forward.linear_1.weight": (0.0046, 0.0046),
    "transformer.1.feed_forward.linear_1.bias": (0.0037, 0.0035),
    "transformer.1.feed_forward.linear_2.weight": (0.0041, 0.0041),
    "transformer.1.feed_forward.linear_2.bias": (0.0018, 0.0017),
    "transformer.1.layer_norm_1.gamma": (0.0041, 0.0031),
    "transformer.1.layer_norm_1.beta": (0.0036, 0.0025),
    "transformer.1.layer_norm_2.gamma": (0.0047, 0.0031),
    "transformer.1.layer_norm_2.beta": (0.0044, 0.0000),
    "layer_norm.gamma": (0.0028, None),
    "layer_norm.beta": (0.0000, None),
}


def _fp8_measured():
    """the mxfp8_train figures for the same tensors (tests/test_fp8_train_gpu.py, the table DESIGN 4.3 summarises)"""
    spec = importlib.util.spec_from_file_location("_fp8_train_gpu", os.path.join(os.path.dirname(__file__), "test_fp8_train_gpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.MEASURED


def test_measured_values_are_a_quarter_of_mxfp8s():
    """Five more mantissa bits predict 1/32 of the MX-FP8 distance; a measured value above a quarter of it would mean a wrong operand,
    not a coarse format.  Exempt: the key bias (true gradient zero) and tensors whose MX-FP8 figure is itself 0.0000 (no product's
    rounding reaches them: the last layer's output-side gradients)."""
    fp8 = _fp8_measured()
    assert MEASURED and set(MEASURED) == set(fp8)
    for n, vals in MEASURED.items():
        for col in (0, 1):
            if vals[col] is None or n.endswith("linear_layers.1.bias") or fp8[n][col] < 1e-3:
                continue
            assert vals[col] < 0.25 * fp8[n][col], (n, col, vals[col], fp8[n][col])


def _gate(measured):
    return max(1.5 * measured, 1e-3)


@pytest.mark.parametrize("forced", [True, False], ids=["forced_256", "as_shipped"])
@pytest.mark.parametrize("pre", [True, False], ids=["pre_ln", "post_ln"])
def test_gradients_against_split_bf16(dev, pre, forced):
    import contextlib
    from lr2ppo_amd import ops
    B, L = (4, 197) if pre else (4, 196)
    col = 0 if pre else 1
    enc = _small_encoder(pre, dev, 3)
    g = torch.Generator().manual_seed(4)
    emb = torch.randn(B, L, 256, generator=g).to(dev)
    seg = torch.ones(B, L, dtype=torch.int64)
    if not pre:
        seg[1, 150:] = 0
        seg[3, 40:] = 0
    seg = seg.to(dev)
    dout = torch.randn(B, L, 256, generator=g).to(dev) * 0.1
    ref_out, ref_demb, ref = _grads(enc, False, emb, seg, dout)
    c0 = ops.gemm_bf16_train_launch_counts()
    with (ops.bf16_train_force_256() if forced else contextlib.nullcontext()):
        out, demb, got = _grads(enc, True, emb, seg, dout)
    d = _counts_delta(ops, c0)
    assert (d[0] > 0 and d[1] > 0 and d[2] == 0) if forced else (d[2] > 0)
    rel = lambda a, b: float((a - b).norm() / b.norm().clamp_min(1e-30))            # noqa: E731
    res = {"output": rel(out, ref_out), "d_emb": rel(demb, ref_demb)}
    for n in ref:
        if n.endswith("linear_layers.1.bias"):
            res[n] = float((got[n] - ref[n]).norm() / ref[n.replace(".1.bias", ".0.bias")].norm())
        else:
            res[n] = rel(got[n], ref[n])
    print(f"\n[bf16_train vs split_bf16, {'pre' if pre else 'post'}-LN, {'forced 256' if forced else 'as shipped'}]")
    for n, r in res.items():
        print(f"  BF16T {col} {n} {r:.6f}")
    bad = [n for n, r in res.items() if n not in MEASURED or not r <= _gate(MEASURED[n][col])]
    assert not bad, bad
    for n in ref:
        if n.endswith("weight"):
            assert float(torch.nn.functional.cosine_similarity(got[n].flatten(), ref[n].flatten(), dim=0)) > 0.999, n


# ---- 5. the schedule against a torch emulation ---------------------------------------------------------------------------------------
def _r(x):
    """what a plane holds: the fp32 value rounded to bf16 (nearest even)"""
    return x.detach().float().to(torch.bfloat16).double()


class _BLinear(torch.autograd.Function):
    """y = x W^T + b as the bf16 schedule computes it: every operand of the forward, the input-gradient and the weight-gradient product
    rounded to bf16; the bias gradient is the sum of the rounded dY (the operand as the weight-gradient product sees it)."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return _r(x) @ _r(w).t() + b

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        return _r(dy) @ _r(w), _r(dy).t() @ _r(x), _r(dy).sum(0)


def _emulated_layer(P, emb, seg, pre, heads, eps, drop):
    """one encoder layer (+ the pre-LN stack's final LayerNorm) in fp64: the bf16 schedule's rounding points, attention and LayerNorm
    exact, the dropout masks of the HIP kernels (oracle.lr2ppo_oracle)"""
    from oracle import lr2ppo_oracle as O
    B, L, E = emb.shape
    M, hd = B * L, E // heads
    mask = (1.0 - (seg > 0).double().view(B, 1, 1, L)) * -10000.0
    t = "transformer.0"
    ln = lambda x, k: O.layernorm_tp(x, P[f"{t}.{k}.gamma"], P[f"{t}.{k}.beta"], eps)          # noqa: E731
    lin = lambda x, k: _BLinear.apply(x, P[f"{t}.{k}.weight"], P[f"{t}.{k}.bias"])            # noqa: E731

    def attention(x):
        w = torch.cat([P[f"{t}.self_attn.linear_layers.{j}.weight"] for j in range(3)], 0)
        b = torch.cat([P[f"{t}.self_attn.linear_layers.{j}.bias"] for j in range(3)], 0)
        q, k, v = _BLinear.apply(x, w, b).view(B, L, 3, heads, hd).permute(2, 0, 3, 1, 4)
        p = torch.softmax(q @ k.transpose(-2, -1) / hd ** 0.5 + mask, dim=-1)
        o = (O._apply_dropout(p, drop, 0, pitch4=True) @ v).transpose(1, 2).reshape(M, E)
        return O._apply_dropout(lin(o, "self_attn.final_linear"), drop, 1)

    def ffn(x):
        return O._apply_dropout(lin(O.gelu_erf(lin(x, "feed_forward.linear_1")), "feed_forward.linear_2"), drop, 2)

    h = emb.reshape(M, E)
    if pre:
        t1 = h + attention(ln(h, "layer_norm_1"))
        hn = t1 + ffn(ln(t1, "layer_norm_2"))
        hn = O.layernorm_tp(hn, P["layer_norm.gamma"], P["layer_norm.beta"], eps)
    else:
        inter = ln(h + attention(h), "layer_norm_1")
        hn = ln(inter + ffn(inter), "layer_norm_2")
    return hn.view(B, L, E)


# worst relative L2 over output, d emb and every parameter gradient, measured on one MI355X (pre-LN, post-LN); the gate is 3 x it
EMULATION_WORST = (1.43e-3, 1.61e-3)


@pytest.mark.parametrize("pre", [True, False], ids=["pre_ln", "post_ln"])
def test_schedule_against_a_torch_emulation(dev, pre):
    """Plumbing: the schedule against the same rounding points emulated in torch (fp64 products of bf16-rounded operands, fp64 attention
    and LayerNorm, the kernels' dropout masks).  A transposed operand, a wrong dropout site or a bias gradient from the wrong tensor is
    O(1).  What separates the two otherwise: fp32 accumulation, the fp32 intermediate tensors, and the bf16 roundings those flip."""
    from lr2ppo_amd import runtime
    B, L = 2, 197 if pre else 196
    enc = _small_encoder(pre, dev, 11, layers=1)
    g = torch.Generator().manual_seed(12)
    emb = torch.randn(B, L, 256, generator=g)
    seg = torch.ones(B, L, dtype=torch.int64)
    if not pre:
        seg[1, 120:] = 0
    dout = torch.randn(B, L, 256, generator=g) * 0.1
    enc.bf16_train = True
    runtime.set_dropout_seed(4321)
    out, saved = enc._forward_train(emb.to(dev), seg.to(dev))
    p, seed = saved["drop"]
    demb, G = enc._backward_train(saved, dout.to(dev))
    P = {n: q.detach().double().cpu().requires_grad_() for n, q in enc.named_parameters()}
    e64 = emb.double().requires_grad_()
    ln_eps = enc.transformer[0].layer_norm_1.eps
    ref = _emulated_layer(P, e64, seg, pre, 4, ln_eps, {"p": p, "seed": seed, "site_base": 0})
    (ref * dout.double()).sum().backward()
    rel = lambda a, b: float((a.double().cpu() - b).norm() / b.norm())          # noqa: E731
    errs = {"output": rel(out, ref.detach()), "d_emb": rel(demb, e64.grad)}
    for n, q in enc.named_parameters():
        if n.endswith("linear_layers.1.bias"):      # true gradient 0: against the query bias's gradient
            errs[n] = float((G[q].double().cpu() - P[n].grad).norm() / P[n.replace(".1.bias", ".0.bias")].grad.norm())
        else:
            errs[n] = rel(G[q], P[n].grad)
    print(f"\n[bf16_train vs torch emulation, {'pre' if pre else 'post'}-LN] EMUL {0 if pre else 1} worst {max(errs.values()):.3e}")
    for n, r in errs.items():
        print(f"  {n:50s} rel L2 {r:.4e}")
    gate = EMULATION_WORST[0 if pre else 1]
    assert gate is not None and max(errs.values()) <= 3 * gate, max(errs.values())


# ---- 6. interface ---------------------------------------------------------------------------------------------------------------------
def _fx(dev, precision, **kw):
    from lr2ppo_amd.finetune.features import TEXT_CONFIG, VIT_CONFIG, FeatureExtractor, encoder_args
    fx = FeatureExtractor(encoder_args(VIT_CONFIG, layers_num=1), encoder_args(TEXT_CONFIG, layers_num=1), precision=precision, **kw)
    fx.init_normal(generator=torch.Generator().manual_seed(8))
    return fx.to(dev)


def _batch(dev):
    from lr2ppo_amd.finetune.features import synthetic_raw_batch
    frames, ids, seg, tgts = synthetic_raw_batch(1, 2, n_img=4, generator=torch.Generator().manual_seed(3))
    return frames.to(dev), ids.to(dev), seg.to(dev), tgts.to(dev)


def test_interface_routes(dev):
    from lr2ppo_amd import runtime
    fx = _fx(dev, "bf16_train")
    assert fx.image.encoder.bf16_train and fx.text.encoder.bf16_train
    frames, ids, seg, tgts = _batch(dev)
    # extract() = forward_train's features with dropout off, bit for bit
    t0, i0 = fx.extract(frames, ids, seg)
    fx.eval()
    t1, i1, _ = fx.forward_train(frames, ids, seg)
    assert torch.equal(t0, t1) and torch.equal(i0, i1)
    # autograd route = explicit route, bit for bit (train mode: dropout on, same seeds); two identical steps: identical bits
    fx.train()
    gt = torch.randn(t0.shape, generator=torch.Generator().manual_seed(1)).to(dev) * 0.01
    gi = torch.randn(i0.shape, generator=torch.Generator().manual_seed(2)).to(dev) * 0.01
    runtime.set_dropout_seed(77)
    te, ie = fx(frames, ids, seg)
    fx.zero_grad(set_to_none=True)
    ((te * gt).sum() + (ie * gi).sum()).backward()
    auto = {n: p.grad.clone() for n, p in fx.named_parameters() if p.grad is not None}

    def explicit(f):
        runtime.set_dropout_seed(77)
        te2, ie2, ctx = f.forward_train(frames, ids, seg)
        f.zero_grad(set_to_none=True)
        f.bind_grads()
        f.backward_train(ctx, gt, gi)
        return te2, ie2, {n: p.grad.clone() for n, p in f.named_parameters()}

    te2, ie2, expl = explicit(fx)
    assert torch.equal(te, te2) and torch.equal(ie, ie2)
    enc_names = [n for n in expl if ".encoder." in n]
    assert enc_names and all(torch.equal(auto[n], expl[n]) for n in enc_names)
    te3, ie3, again = explicit(fx)
    assert torch.equal(te2, te3) and torch.equal(ie2, ie3) and all(torch.equal(expl[n], again[n]) for n in expl)
    # recompute=True: the same bits as the plain path
    rc = _fx(dev, "bf16_train", recompute=True).train()
    rc.load_state_dict(fx.state_dict())
    te4, ie4, rce = explicit(rc)
    assert torch.equal(te2, te4) and torch.equal(ie2, ie4)
    diff = [n for n in expl if not torch.equal(expl[n], rce[n])]
    assert not diff, diff
    # grad_flats() sizes do not depend on the precision
    ref = _fx(dev, "split_bf16")
    assert [t.numel() for t in fx.grad_flats()] == [t.numel() for t in ref.grad_flats()]
    # the inference-only precisions still refuse the training forward
    for prec in ("bf16", "mxfp8"):
        with pytest.raises(NotImplementedError):
            _fx(dev, prec).forward_train(frames, ids, seg)


def test_interface_steps_and_weight_cache(dev):
    from lr2ppo_amd.finetune import ppo
    from lr2ppo_amd.finetune.features import build_encoder_optimizer, finetune_pointwise_step, finetune_ppo_step
    fx = _fx(dev, "bf16_train")
    frames, ids, seg, tgts = _batch(dev)
    args = argparse.Namespace(mode="reg", labels_num=3, seq_length=196, max_imgs=4, visual_feat_dim=768, is_master=True,
                              kl_div_loss_weight=0.001, entropy_weight=0.001, value_clip=0.5, optimizer="adamw", scheduler="linear",
                              learning_rate=1e-3, critic_learning_rate=1e-3, train_steps=41, warmup=0.1, device=dev)
    enc = fx.text.encoder
    fx.extract(frames, ids, seg)
    n0 = enc.bf16_weight_splits
    fx.forward_train(frames, ids, seg)
    fx.extract(frames, ids, seg)
    assert enc.bf16_weight_splits == n0                           # no parameter write: no re-split
    model = ppo.ActorCritic(args, None)
    ppo._init_normal(model.critic)
    model = model.to(dev)
    reward = ppo.Reward(args, None)
    ppo._init_normal(reward)
    reward = reward.to(dev).eval()
    opt, copt, sch, csch = ppo.build_optimizer(args, model)
    eopt, esch = build_encoder_optimizer(args, fx)
    sch.step(), csch.step(), esch.step()
    before = {n: p.detach().clone() for n, p in fx.named_parameters()}
    loss = finetune_pointwise_step(args, fx, model.actor, opt, sch, eopt, esch, frames, ids, seg, tgts)
    assert torch.isfinite(loss)
    fx.extract(frames, ids, seg)
    n1 = enc.bf16_weight_splits
    assert n1 == n0 + 1                                            # one optimizer write since: one re-split
    fx.extract(frames, ids, seg)
    assert enc.bf16_weight_splits == n1
    metrics = finetune_ppo_step(args, fx, model, reward, opt, copt, eopt, frames, ids, seg, tgts)
    assert bool(torch.isfinite(torch.as_tensor(metrics)).all())
    moved = {n for n, p in fx.named_parameters() if not torch.equal(before[n], p.detach())}
    stuck = [n for n in before if ".encoder." in n and n not in moved]
    assert not stuck, stuck
