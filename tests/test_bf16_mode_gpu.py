"""The single-pass bf16 inference mode on a real MI355X: the 256 x 256 single-pass product (csrc/gemm256_b1.hip) and its 128-row
fallback against exact and fp64 references, the single-plane outputs of the product / LayerNorm / attention byte for byte against
round-to-nearest-even of the fp32 results, TransformerEncoder.forward_bf16 against an fp64 emulation that rounds where the schedule
writes a plane, and FeatureExtractor(precision="bf16") against the split-bf16 path of the same weights."""
import argparse
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(256, 256, 64), (300, 256, 128), (257, 320, 192), (512, 264, 448), (1, 256, 64)]
U = 2.0 ** -24


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def _operands(M, N, K, dev, ints, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    if ints:
        a = torch.randint(-8, 9, (M, K), device=dev, generator=g).to(torch.bfloat16)
        b = torch.randint(-8, 9, (N, K), device=dev, generator=g).to(torch.bfloat16)
    else:
        a = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
        b = torch.randn(N, K, device=dev, generator=g).to(torch.bfloat16)
    return a, b


def _ran_on(block_m, before, after):
    """the launch counters say which kernel a call reached"""
    d = (after[0] - before[0], after[1] - before[1])
    assert d == ((1, 0) if block_m == 256 else (0, 1)), (block_m, d)


@pytest.mark.parametrize("block_m", [256, 128])
@pytest.mark.parametrize("M, N, K", SHAPES)
def test_product_exact_on_integers_and_within_the_fp32_accumulation_bound(dev, M, N, K, block_m):
    from lr2ppo_amd import ops
    # (a) integers in [-8, 8]: every partial sum is an integer below 2^24 -- the result is exact
    a, b = _operands(M, N, K, dev, True, 1)
    out = torch.full((M, N), float("nan"), device=dev)
    c0 = ops.gemm_bf16_launch_counts()
    ops.gemm_bf16(a, b, out, M, N, K, block_m=block_m)
    _ran_on(block_m, c0, ops.gemm_bf16_launch_counts())
    ref = a.double() @ b.double().T
    assert torch.equal(out.double(), ref)
    # (b) normal data rounded to bf16 against the fp64 product of those values: |err| <= K * 2^-24 * sum_k |a_k b_k|
    a, b = _operands(M, N, K, dev, False, 2)
    out.fill_(float("nan"))
    ops.gemm_bf16(a, b, out, M, N, K, block_m=block_m)
    ref = a.double() @ b.double().T
    bound = K * U * (a.double().abs() @ b.double().abs().T)
    err = (out.double() - ref).abs()
    print(f"\n{M}x{N}x{K} block_m={block_m}: max err / bound = {(err / bound).max().item():.3e}")
    assert (err <= bound).all()


@pytest.mark.parametrize("block_m", [256, 128])
@pytest.mark.parametrize("M, N, K", SHAPES)
def test_product_with_bias_gelu_residual(dev, M, N, K, block_m):
    from lr2ppo_amd import ops
    a, b = _operands(M, N, K, dev, False, 3)
    g = torch.Generator(device=dev).manual_seed(4)
    bias = torch.randn(N, device=dev, generator=g)
    resid = torch.randn(M, N, device=dev, generator=g)
    out = torch.full((M, N), float("nan"), device=dev)
    ops.gemm_bf16(a, b, out, M, N, K, bias=bias, act=1, resid=resid, block_m=block_m)
    z = a.double() @ b.double().T + bias.double()
    gz = 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))
    ref = gz + resid.double()
    # product bound + the fp32 rounding of z, through GELU (|GELU'| <= 1.13); the kernel's documented 6e-7 erf error (x 0.5 |z|);
    # the fp32 roundings of the GELU's three operations and of the residual add
    zb = K * U * (a.double().abs() @ b.double().abs().T) + 2 * U * z.abs()
    tol = 1.13 * zb + 3e-7 * z.abs() + 4 * U * (gz.abs() + z.abs()) + 2 * U * (resid.double().abs() + ref.abs())
    err = (out.double() - ref).abs()
    print(f"\n{M}x{N}x{K} block_m={block_m} bias+GELU+resid: max err / tol = {(err / tol).max().item():.3e}")
    assert (err <= tol).all()
    # alpha, and a residual without the activation
    ops.gemm_bf16(a, b, out, M, N, K, bias=bias, resid=resid, alpha=0.5, block_m=block_m)
    ref = 0.5 * (a.double() @ b.double().T) + bias.double() + resid.double()
    tol = 0.5 * K * U * (a.double().abs() @ b.double().abs().T) + 4 * U * (ref.abs() + resid.double().abs() + bias.double().abs())
    assert ((out.double() - ref).abs() <= tol).all()


@pytest.mark.parametrize("block_m", [256, 128])
@pytest.mark.parametrize("M, N, K", SHAPES)
def test_product_plane_is_rne_of_the_fp32_result(dev, M, N, K, block_m):
    from lr2ppo_amd import ops
    a, b = _operands(M, N, K, dev, False, 5)
    bias = torch.randn(N, device=dev, generator=torch.Generator(device=dev).manual_seed(6))
    for act in (0, 1):
        out = torch.empty(M, N, device=dev)
        both = torch.zeros(M * N + 8, dtype=torch.bfloat16, device=dev)
        alone = torch.zeros(M * N + 8, dtype=torch.bfloat16, device=dev)
        ops.gemm_bf16(a, b, out, M, N, K, bias=bias, act=act, out_plane=both, block_m=block_m)       # both outputs, one launch
        ops.gemm_bf16(a, b, None, M, N, K, bias=bias, act=act, out_plane=alone, block_m=block_m)     # the plane alone
        want = out.to(torch.bfloat16).view(-1).view(torch.int16)
        assert torch.equal(both[:M * N].view(torch.int16), want)
        assert torch.equal(alone[:M * N].view(torch.int16), want)
        assert (both[M * N:] == 0).all() and (alone[M * N:] == 0).all()                              # nothing behind the plane
    # hi / lo planes out of the same kernel: the QKV product in front of the 3-pass attention kernels
    pl = ops.Planes.empty(M, N, dev)
    out = torch.empty(M, N, device=dev)
    ops.gemm_bf16(a, b, out, M, N, K, bias=bias, out_planes=pl, block_m=block_m)
    hi = out.to(torch.bfloat16)
    assert torch.equal(pl.buf[:M * N], hi.view(-1).view(torch.int16))
    assert torch.equal(pl.buf[M * N:].view(torch.bfloat16), (out - hi.float()).to(torch.bfloat16).view(-1))


def test_large_product_follows_the_row_split_plan(dev):
    """M = 12 544, N = 3072 (588 tiles of 256 x 256 = 2.3 rounds): whole rounds on the 256 x 256 kernel, the rest on short tiles --
    every row computed once, the same bits as the 128-row family gives (both accumulate 64-deep steps in k order)."""
    from lr2ppo_amd import ops
    M, N, K = 12544, 3072, 256
    a, b = _operands(M, N, K, dev, True, 7)
    out = torch.full((M, N), float("nan"), device=dev)
    c0 = ops.gemm_bf16_launch_counts()
    ops.gemm_bf16(a, b, out, M, N, K)
    c1 = ops.gemm_bf16_launch_counts()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, 1)
    assert torch.equal(out, (a.float() @ b.float().T))              # integers: exact in fp32 whatever the order


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("D", [768, 100])
@pytest.mark.parametrize("rows", [1, 5, 300])
def test_layernorm_plane_is_the_hi_plane(dev, rows, D, mode):
    from lr2ppo_amd import ops
    g = torch.Generator(device=dev).manual_seed(8)
    x = torch.randn(rows, D, device=dev, generator=g) * 3 + 1
    gamma, beta = torch.randn(D, device=dev, generator=g), torch.randn(D, device=dev, generator=g)
    pl = ops.Planes.empty(rows, D, dev)
    ops.layernorm_fwd(x, gamma, beta, None, rows=rows, D=D, eps=1e-6, mode=mode, out_planes=pl)
    one = torch.zeros(rows * D + 8, dtype=torch.int16, device=dev)
    f32 = torch.empty(rows, D, device=dev)
    ops.layernorm_fwd(x, gamma, beta, f32, rows=rows, D=D, eps=1e-6, mode=mode, out_plane=one)
    assert torch.equal(one[:rows * D], pl.buf[:rows * D])
    assert torch.equal(one[:rows * D], f32.to(torch.bfloat16).view(-1).view(torch.int16))
    assert (one[rows * D:] == 0).all()                            # the lo store is gone: nothing written behind the plane


@pytest.mark.parametrize("batch, heads", [(2, 4), (64, 4)])
@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("L", [1, 16, 197, 288])
def test_attention_plane_is_rne_of_the_fp32_context(dev, L, padded, batch, heads):
    from lr2ppo_amd import _native, ops
    cus = _native.lib().lr2_device_info(None, 0)
    persistent = ops.self_attn_bf16_plan(batch, heads, L)
    assert persistent == (batch * heads >= cus)                  # (2, 4): one workgroup per pair; (64, 4): the persistent form
    E = heads * 64
    g = torch.Generator(device=dev).manual_seed(9)
    qkv = torch.randn(batch * L, 3 * E, device=dev, generator=g).to(torch.bfloat16)
    seg = torch.ones(batch, L, dtype=torch.int64, device=dev)
    if padded:
        seg[:, max(1, (2 * L) // 3):] = 0
    o32 = torch.full((batch * L, E), float("nan"), device=dev)
    both = torch.zeros(batch * L * E, dtype=torch.bfloat16, device=dev)
    alone = torch.zeros(batch * L * E, dtype=torch.bfloat16, device=dev)
    kw = dict(batch=batch, heads=heads, L=L, head_dim=64, scale=0.125)
    ops.self_attn_fwd_bf16(qkv, seg.view(-1), out=o32, out_plane=both, **kw)
    ops.self_attn_fwd_bf16(qkv, seg.view(-1), out_plane=alone, **kw)
    assert torch.isfinite(o32).all()
    want = o32.to(torch.bfloat16).view(-1).view(torch.int16)
    assert torch.equal(both.view(torch.int16), want) and torch.equal(alone.view(torch.int16), want)
    # ... and the fp32 context is the attention of those operands (single-pass products: P and the operands keep 8 mantissa bits)
    q, k, v = (t.float().view(batch, L, heads, 64).transpose(1, 2).double() for t in qkv.split(E, dim=1))
    s = q @ k.transpose(-1, -2) * 0.125 + (seg <= 0).double()[:, None, None, :] * -10000.0
    ref = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(batch * L, E)
    assert _rel(o32, ref) < 1e-2


# ---- the schedule against an fp64 emulation that rounds to bf16 where forward_bf16 writes a plane ---------------------------------
def _enc_args(**over):
    from lr2ppo_amd.tencentpretrain.opts import finetune_opts, tokenizer_opts
    p = argparse.ArgumentParser()
    finetune_opts(p)
    tokenizer_opts(p)
    d = vars(p.parse_args([]))
    d.update(dict(emb_size=256, feedforward_size=1024, hidden_size=256, hidden_act="gelu", heads_num=4, layers_num=1, dropout=0.0,
                  max_seq_length=514, embedding=["word", "pos", "seg"], encoder="transformer", mask="fully_visible"))
    d.update(over)
    return argparse.Namespace(**d)


def _bf(x):
    return x.float().to(torch.bfloat16).double()


def _ln(x, m):
    mean = x.mean(-1, keepdim=True)
    std = x.std(-1, unbiased=True, keepdim=True)
    return m.gamma.double() * (x - mean) / (std + m.eps) + m.beta.double()


def _emulate(enc, emb, seg, rounded=True):
    """(rounded=False: the encoder in plain fp64, no rounding anywhere -- the reference where the split-bf16 path cannot run.)
    forward_bf16 in fp64, rounded to bf16 (via fp32, as the kernels hold fp32 values) exactly where the schedule writes a plane:
    the LayerNorm output / the post-LN hidden state in front of QKV, Q | K | V, the context, the LayerNorm output in front of FFN-1,
    GELU(z); the weights are bf16(W); inside the attention kernel the un-normalised probabilities are bf16, their sum is not."""
    _bf = globals()["_bf"] if rounded else (lambda x: x)
    B, L, E = emb.shape
    H = enc.heads_num
    pre = enc.layernorm_positioning == "pre"
    h = emb.double().view(B * L, E)
    mask = (seg <= 0).double()[:, None, None, :] * -10000.0
    lin = lambda x, m: x @ _bf(m.weight.double()).T + m.bias.double()
    for layer in enc.transformer:
        att, ffn = layer.self_attn, layer.feed_forward
        x = _bf(_ln(h, layer.layer_norm_1)) if pre else _bf(h)
        q, k, v = (_bf(lin(x, m)).view(B, L, H, E // H).transpose(1, 2) for m in att.linear_layers)
        s = q @ k.transpose(-1, -2) / math.sqrt(E // H) + mask
        p = torch.exp(s - s.max(-1, keepdim=True).values)
        o = _bf(((_bf(p) @ v) / p.sum(-1, keepdim=True)).transpose(1, 2).reshape(B * L, E))
        h2 = lin(o, att.final_linear) + h
        gelu = lambda z: 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))
        if pre:
            t = _bf(_ln(h2, layer.layer_norm_2))
            h = lin(_bf(gelu(lin(t, ffn.linear_1))), ffn.linear_2) + h2
        else:
            xn = _ln(h2, layer.layer_norm_1)
            y = lin(_bf(gelu(lin(_bf(xn), ffn.linear_1))), ffn.linear_2) + xn
            h = _ln(y, layer.layer_norm_2)
    if enc.final_layernorm:
        h = _ln(h, enc.layer_norm)
    return h.view(B, L, E)


# Measured on MI355X (this file's own prints), each against the reference its test names:
#   plumbing, vs the rounding emulation: pre-LN 4.686e-4, post-LN 1.711e-4           -> gate 3 x the worst (cap 3e-2)
#   first_only vs row 0 of the full call: 2.107e-3 / 2.105e-3                         -> gate 1.5 x
#   accuracy vs split-bf16, 2 layers, E = 256: text 5.749e-4, image 3.183e-3          -> gates 1.5 x each (cap 1.5e-2)
#   E = 768 (ViT-B/16 + RoBERTa-base, 2 layers): text 1.768e-3, image 4.195e-3, Actor max |d logit| 2.070e-3   -> 1.5 x each
#   L = 304 (3-pass attention fallback) vs split-bf16: 2.527e-4; head width 32 vs plain fp64: 2.576e-4         -> 1.5 x each
PLUMBING_GATE = 3 * 4.686e-4
FIRST_ONLY_GATE = 1.5 * 2.107e-3
ACCURACY_GATE = {"text": 1.5 * 5.749e-4, "image": 1.5 * 3.183e-3}
ACCURACY_GATE_768 = {"text": 1.5 * 1.768e-3, "image": 1.5 * 4.195e-3, "logit": 1.5 * 2.070e-3}
LONG_SEQ_GATE = 1.5 * 2.527e-4
HEAD32_GATE = 1.5 * 2.576e-4
assert PLUMBING_GATE <= 3e-2 and max(ACCURACY_GATE.values()) <= 1.5e-2 and max(ACCURACY_GATE_768.values()) <= 1.5e-2


@pytest.mark.parametrize("placement, L, padded", [("pre", 197, False), ("post", 196, True)])
def test_forward_bf16_matches_the_rounding_emulation(dev, placement, L, padded):
    """One layer, B = 2, E = 256, F = 1024, 4 heads.  A transposed or mis-sliced operand, the wrong plane, a missing bias or residual
    is O(1); rounding ties that fall differently (the emulation's fp64 sums against the kernels' fp32 ones) are all that may differ.
    Gate: 3 x the measured worst relative L2, capped at 3e-2 (the cap tests/test_fp8_train_gpu.py uses for the same kind of check).
    Measured on MI355X: 4.686e-4 (pre-LN, L = 197) and 1.711e-4 (post-LN, L = 196, padded) -> PLUMBING_GATE = 1.41e-3; first_only
    against row 0 of the full call 2.107e-3 / 2.105e-3 -> FIRST_ONLY_GATE = 3.16e-3 (1.5 x: the result is deterministic)."""
    from lr2ppo_amd.tencentpretrain.encoders import str2encoder
    torch.manual_seed(11)
    enc = str2encoder["transformer"](_enc_args(layernorm_positioning=placement))
    for n, p in enc.named_parameters():
        p.data.normal_(0, 0.05) if "gamma" not in n else p.data.normal_(1.0, 0.1)
    enc = enc.to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(12)
    emb = torch.randn(2, L, 256, device=dev, generator=g)
    seg = torch.ones(2, L, dtype=torch.int64, device=dev)
    if padded:
        seg[1, 150:] = 0
    got = enc.forward_bf16(emb, seg)
    ref = _emulate(enc, emb, seg)
    r = _rel(got, ref)
    r3 = _rel(got, enc(emb, seg))
    print(f"\nforward_bf16 {placement}-LN L={L}: vs emulation {r:.3e}; vs the split-bf16 forward {r3:.3e}")
    assert torch.isfinite(got).all() and r < PLUMBING_GATE
    first = enc.forward_bf16(emb, seg, first_only=True)
    # the pruned last layer runs its row-0 products in split-bf16 on hi / lo K | V planes of a bf16 product, the full call in one
    # bf16 pass: the two differ by what the mode differs from the parity path over one layer (measured, FIRST_ONLY_GATE)
    r0 = _rel(first, got[:, 0, :])
    print(f"first_only vs row 0 of the full call {r0:.3e}")
    assert first.shape == (2, 256) and torch.isfinite(first).all() and r0 < FIRST_ONLY_GATE


def _small_extractor(dev, **over):
    from lr2ppo_amd.finetune.features import TEXT_CONFIG, VIT_CONFIG, FeatureExtractor, encoder_args
    kw = dict(layers_num=2, hidden_size=256, emb_size=256, feedforward_size=1024, heads_num=4)
    kw.update(over)
    torch.manual_seed(13)
    fx = FeatureExtractor(encoder_args(VIT_CONFIG, **kw), encoder_args(TEXT_CONFIG, **kw), feat_dim=kw["hidden_size"], precision="bf16")
    fx.init_normal()
    return fx.to(dev).eval()


def test_bf16_mode_accuracy_against_split_bf16(dev):
    """Two-layer towers at E = 256: relative L2 of text_emb / img_emb between precision="bf16" and the split-bf16 path of the same
    module.  Gate: 1.5 x measured per tensor (the result is deterministic; the margin covers the choice of seed), capped at 1.5e-2 --
    above that the mode would be no better than MX-FP8's 2.2e-2 on the text tower.  Measured on MI355X: text 5.749e-4, image 3.183e-3 -> gates
    8.62e-4 and 4.77e-3 (DESIGN.md 2 sets them beside the emulation's 4-7e-3 at full depth).
    (The Actor's logits are not compared here: the heads take 768-wide features only, these towers are 256 wide.)"""
    from lr2ppo_amd.finetune.features import synthetic_raw_batch
    fx = _small_extractor(dev)
    frames, ids, seg, _ = synthetic_raw_batch(2, 2, n_img=4, device=dev, generator=torch.Generator(device=dev).manual_seed(14))
    fx.precision = "split_bf16"
    t0, i0 = fx.extract(frames, ids, seg)
    fx.precision = "bf16"
    t1, i1 = fx.extract(frames, ids, seg)
    fx.precision = "split_bf16"
    t2, i2 = fx.extract(frames, ids, seg)
    assert torch.equal(t0, t2) and torch.equal(i0, i2)            # the mode shares the weight planes and must not disturb them
    rt, ri = _rel(t1, t0), _rel(i1, i0)
    print(f"\nbf16 vs split-bf16, 2 layers, E = 256: text {rt:.3e}, image {ri:.3e}")
    assert torch.isfinite(t1).all() and torch.isfinite(i1).all()
    assert 1e-5 < rt < ACCURACY_GATE["text"] and 1e-5 < ri < ACCURACY_GATE["image"]       # really another precision, and close
    fx.precision = "bf16"
    with pytest.raises(NotImplementedError):
        fx.forward_train(frames, ids, seg)
    with pytest.raises(NotImplementedError):
        fx.train()(frames, ids, seg)


def test_bf16_mode_actor_logit_shift_at_768(dev):
    """The figure test 5 cannot give at E = 256 (the heads take 768-wide features only): ViT-B/16 + RoBERTa-base, two layers each,
    seeded Actor; max |d logit| between the bf16 features and the split-bf16 ones, printed beside the feature errors (DESIGN.md 2 sets
    it beside the full-depth emulation's 8.5e-3).  Measured on MI355X: text 1.768e-3, image 4.195e-3, max |d logit| 2.070e-3; gates
    1.5 x each (deterministic; the margin covers the seed)."""
    import argparse as ap

    from lr2ppo_amd.finetune import ppo
    from lr2ppo_amd.finetune.features import synthetic_raw_batch
    from oracle import lr2ppo_oracle as O
    fx = _small_extractor(dev, hidden_size=768, emb_size=768, feedforward_size=3072, heads_num=12)
    args = ap.Namespace(mode="reg", labels_num=3, seq_length=196, max_imgs=16, visual_feat_dim=768, is_master=True, device=dev)
    actor = ppo.Actor(args, None)
    actor.load_state_dict(O.seeded_params(O.head_param_spec("actor"), seed=7), strict=True)
    actor = actor.to(dev).eval()
    frames, ids, seg, _ = synthetic_raw_batch(2, 2, device=dev, generator=torch.Generator(device=dev).manual_seed(19))
    fx.precision = "split_bf16"
    t0, i0 = fx.extract(frames, ids, seg)
    fx.precision = "bf16"
    t1, i1 = fx.extract(frames, ids, seg)
    with torch.no_grad():
        d = (actor(t1, i1, None) - actor(t0, i0, None)).abs().max().item()
    rt, ri = _rel(t1, t0), _rel(i1, i0)
    print(f"\nbf16 vs split-bf16, 2 layers, E = 768: text {rt:.3e}, image {ri:.3e}, Actor max |d logit| {d:.3e}")
    assert rt < ACCURACY_GATE_768["text"] and ri < ACCURACY_GATE_768["image"] and d < ACCURACY_GATE_768["logit"]


def test_long_sequences_take_the_three_pass_attention(dev):
    """L = 304 > 288 at head width 64: the QKV product writes hi / lo planes, the 3-pass attention kernels run, the context goes
    through split_planes -- inside the accuracy gate against the split-bf16 forward."""
    from lr2ppo_amd.tencentpretrain.encoders import str2encoder
    torch.manual_seed(15)
    enc = str2encoder["transformer"](_enc_args(layers_num=2, hidden_size=128, emb_size=128, feedforward_size=512, heads_num=2))
    for n, p in enc.named_parameters():
        if "gamma" not in n and "beta" not in n:
            p.data.normal_(0, 0.02)
    enc = enc.to(dev).eval()
    emb = torch.randn(2, 304, 128, device=dev, generator=torch.Generator(device=dev).manual_seed(16))
    seg = torch.ones(2, 304, dtype=torch.int64, device=dev)
    got, ref = enc.forward_bf16(emb, seg), enc(emb, seg)
    r = _rel(got, ref)
    print(f"\nL = 304 fallback: bf16 vs split-bf16 {r:.3e}")
    assert torch.isfinite(got).all() and r < LONG_SEQ_GATE            # measured 2.527e-4, x 1.5


def test_head_width_32_takes_the_three_pass_attention(dev):
    """The issue's fallback case: E = 128, 4 heads (head width 32).  The attention kernels are built for head width 64, so
    forward_bf16 zero-pads every head to 64 columns (one small bf16 product per head and Q / K / V block into a zeroed planes matrix)
    and runs the 3-pass kernels on that.  The split-bf16 forward refuses this head width
    (tests/test_encoder_gpu.py::test_small_encoder_both_layernorm_placements), so the reference is the same encoder in plain fp64
    (4e-6 from the split-bf16 path where both exist); the gate is 1.5 x the measured 2.576e-4, far inside test 5's."""
    from lr2ppo_amd.tencentpretrain.encoders import str2encoder
    torch.manual_seed(17)
    enc = str2encoder["transformer"](_enc_args(layers_num=2, hidden_size=128, emb_size=128, feedforward_size=512, heads_num=4))
    for n, p in enc.named_parameters():
        if "gamma" not in n and "beta" not in n:
            p.data.normal_(0, 0.02)
    enc = enc.to(dev).eval()
    emb = torch.randn(2, 64, 128, device=dev, generator=torch.Generator(device=dev).manual_seed(18))
    seg = torch.ones(2, 64, dtype=torch.int64, device=dev)
    seg[1, 50:] = 0
    got = enc.forward_bf16(emb, seg)
    r = _rel(got, _emulate(enc, emb, seg, rounded=False))
    print(f"\nhead width 32: bf16 vs fp64 {r:.3e}")
    assert torch.isfinite(got).all() and 1e-5 < r < HEAD32_GATE       # measured 2.576e-4, x 1.5
