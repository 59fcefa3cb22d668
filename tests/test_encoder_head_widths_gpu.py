"""TransformerEncoder and FeatureExtractor at head widths other than 64 (csrc/selfattn_hd.hip behind ops.self_attn_fwd / self_attn_bwd):
two-layer towers of head width 32, 80, 96 and 128 in both LayerNorm placements -- inference, forward_first_token, the split-bf16
training schedule, recompute, bf16_train and mxfp8_train -- against oracle.transformer_encoder and its autograd; the ViT-H/14 tower
(hidden 1280, 16 heads of 80, 257 tokens) at full width behind FeatureExtractor and --image_tower vit_huge_14_224; and the proof that a
width-64 tower launches none of the new kernels.

Bars: forward max error < 1e-3 max|ref| (the north-star bar of tests/test_encoder_gpu.py; expected ~1e-5); gradients relative L2 < REL =
2e-3 (tests/test_round3_gpu.py); recompute: torch.equal (the mode's contract); bf16_train / mxfp8_train against the split-bf16 schedule:
the per-tensor tables MEASURED and the rule _gate of tests/test_bf16_train_gpu.py (max(1.5 x measured, 1e-3)) and
tests/test_fp8_train_gpu.py (min(0.15, max(1.5 x measured, 1e-3))), which those files apply to the same comparison on the same inputs at
4 heads of 64."""
import argparse

import pytest
import torch

from oracle import lr2ppo_oracle as O

pytestmark = pytest.mark.gpu

REL = 2e-3          # the gradient bar of the encoder-backward tests (tests/test_round3_gpu.py: REL = 2e-3)
SIZES = ((32, 128, 4), (80, 320, 4), (96, 192, 2), (128, 256, 2))          # (head width, hidden size E, heads)
B, L = 2, 33


def _rel(a, b) -> float:
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _tower(dev, E, heads, pre, seed):
    """A two-layer tower with dropout 0 and the oracle's parameter dict for it."""
    from lr2ppo_amd.finetune.features import TEXT_CONFIG, VIT_CONFIG, encoder_args
    from lr2ppo_amd.tencentpretrain.encoders import str2encoder
    a = encoder_args(VIT_CONFIG if pre else TEXT_CONFIG, layers_num=2, hidden_size=E, emb_size=E, feedforward_size=4 * E, heads_num=heads,
                     dropout=0.0)
    P = O.seeded_params(O.encoder_param_spec(2, E, 4 * E, pre), seed=seed, std=0.05)
    enc = str2encoder["transformer"](a)
    enc.load_state_dict(P, strict=True)
    return enc.to(dev), P


def _inputs(E, seed):
    g = torch.Generator().manual_seed(seed)
    emb = torch.randn(B, L, E, generator=g)
    w = torch.randn(B, L, E, generator=g)
    seg = torch.ones(B, L, dtype=torch.long)
    seg[1, 20:] = 0                                                     # a padded tail in sequence 1
    return emb, seg, w


@pytest.mark.parametrize("pre", [True, False], ids=["pre_ln", "post_ln"])
@pytest.mark.parametrize("hd,E,heads", SIZES)
def test_forward_and_first_token_match_oracle(dev, hd, E, heads, pre):
    from lr2ppo_amd import ops
    enc, P = _tower(dev, E, heads, pre, seed=300 + hd)
    enc.eval()
    emb, seg, _ = _inputs(E, seed=hd)
    with torch.no_grad():
        ref = O.transformer_encoder(P, emb, seg, 2, heads, pre)
        before = ops.self_attn_hd_launch_counts()
        h = enc(emb.to(dev), seg.to(dev))
        assert ops.self_attn_hd_launch_counts() == (before[0] + 2, before[1])          # one forward per layer, on the new kernels
        h0 = enc.forward_first_token(emb.to(dev), seg.to(dev))
    bar = 1e-3 * float(ref.abs().max())
    err = float((h.cpu() - ref).abs().max())
    print(f"  width {hd}, {'pre' if pre else 'post'}-LN: forward max err {err:.3e} (bar {bar:.3e})")
    assert err < bar
    assert h0.shape == (B, E) and float((h0.cpu() - ref[:, 0]).abs().max()) < bar
    assert _rel(h0, h[:, 0]) < 1e-5


@pytest.mark.parametrize("pre", [True, False], ids=["pre_ln", "post_ln"])
@pytest.mark.parametrize("hd,E,heads", SIZES)
def test_training_gradients_match_oracle_autograd_and_recompute_gives_the_same_bits(dev, hd, E, heads, pre):
    enc, P = _tower(dev, E, heads, pre, seed=400 + hd)
    enc.train()
    emb, seg, w = _inputs(E, seed=10 + hd)

    def run():
        for p in enc.parameters():
            p.grad = None
        e = emb.to(dev).requires_grad_(True)
        h = enc(e, seg.to(dev))
        (h * w.to(dev)).sum().backward()
        return h.detach().clone(), e.grad.clone(), {n: p.grad.clone() for n, p in enc.named_parameters()}

    out, demb, G = run()
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    e64 = emb.clone().requires_grad_(True)
    ref = O.transformer_encoder(Pg, e64, seg, 2, heads, pre)
    (ref * w).sum().backward()
    assert float((out.cpu() - ref.detach()).abs().max()) < 1e-3 * float(ref.abs().max())
    assert _rel(demb, e64.grad) < REL, _rel(demb, e64.grad)
    worst = 0.0
    for n, g in G.items():
        r = Pg[n].grad
        if n.endswith("linear_layers.1.bias"):          # the key bias: analytically zero (softmax is shift-invariant), DESIGN.md 6
            assert float(g.abs().max()) < 1e-4 * float(Pg[n.replace(".1.bias", ".0.bias")].grad.abs().max()) + 1e-6, n
            continue
        worst = max(worst, _rel(g, r))
        assert _rel(g, r) < REL, (n, _rel(g, r))
    print(f"  width {hd}, {'pre' if pre else 'post'}-LN: worst parameter-gradient rel L2 {worst:.3e}, d_emb {_rel(demb, e64.grad):.3e}")
    enc.recompute = True
    out2, demb2, G2 = run()
    assert torch.equal(out, out2) and torch.equal(demb, demb2)
    for n in G:
        assert torch.equal(G[n], G2[n]), n


def _small_encoder_two_heads(pre, dev, seed):
    """tests/test_bf16_train_gpu.py::_small_encoder (= test_fp8_train_gpu.py's) with 2 heads of 128 instead of 4 of 64."""
    from lr2ppo_amd.finetune.features import TEXT_CONFIG, VIT_CONFIG, encoder_args
    from lr2ppo_amd.tencentpretrain.encoders import str2encoder
    a = encoder_args(VIT_CONFIG if pre else TEXT_CONFIG, layers_num=2, hidden_size=256, emb_size=256, feedforward_size=1024, heads_num=2,
                     dropout=0.1)
    g = torch.Generator().manual_seed(seed)
    enc = str2encoder["transformer"](a)
    for n, p in enc.named_parameters():
        if "gamma" in n:
            p.data.uniform_(0.8, 1.2, generator=g)
        else:
            p.data.normal_(0, 0.05, generator=g)
    return enc.to(dev).train()


@pytest.mark.parametrize("mode", ["bf16_train", "mxfp8_train"])
@pytest.mark.parametrize("pre", [True, False], ids=["pre_ln", "post_ln"])
def test_single_pass_training_modes_against_split_bf16_at_width_128(dev, mode, pre):
    """One training step at E = 256 with 2 heads of 128 on the inputs of test_gradients_against_split_bf16 (both files), gated by those
    files' own MEASURED tables and _gate rules (module docstring)."""
    import test_bf16_train_gpu as TB
    import test_fp8_train_gpu as TF
    from lr2ppo_amd import ops
    T = TB if mode == "bf16_train" else TF
    Bt, Lt = (4, 197) if pre else (4, 196)
    col = 0 if pre else 1
    enc = _small_encoder_two_heads(pre, dev, 3)
    g = torch.Generator().manual_seed(4)
    emb = torch.randn(Bt, Lt, 256, generator=g).to(dev)
    seg = torch.ones(Bt, Lt, dtype=torch.int64)
    if not pre:
        seg[1, 150:] = 0
        seg[3, 40:] = 0
    seg = seg.to(dev)
    dout = torch.randn(Bt, Lt, 256, generator=g).to(dev) * 0.1
    ref_out, ref_demb, ref = T._grads(enc, False, emb, seg, dout)
    before = ops.self_attn_hd_launch_counts()
    out, demb, got = T._grads(enc, True, emb, seg, dout)
    assert ops.self_attn_hd_launch_counts() == (before[0] + 2, before[1] + 2)         # the 3-pass attention of both layers: the new pair
    enc.bf16_train = enc.fp8_train = False
    rel = lambda a, b: float((a - b).norm() / b.norm().clamp_min(1e-30))            # noqa: E731
    res = {"output": rel(out, ref_out), "d_emb": rel(demb, ref_demb)}
    for n in ref:
        if n.endswith("linear_layers.1.bias"):
            res[n] = float((got[n] - ref[n]).norm() / ref[n.replace(".1.bias", ".0.bias")].norm())
        else:
            res[n] = rel(got[n], ref[n])
    print(f"\n[{mode} vs split_bf16 at width 128, {'pre' if pre else 'post'}-LN]")
    for n, r in res.items():
        print(f"  HD128 {mode} {col} {n} {r:.6f} (gate {T._gate(T.MEASURED[n][col]):.6f})")
    bad = [(n, r) for n, r in res.items() if not r <= T._gate(T.MEASURED[n][col])]
    assert not bad, bad


def _vit_h_extractor(dev, vit_layers=2, text_layers=1):
    from lr2ppo_amd.finetune.features import IMAGE_TOWERS, TEXT_CONFIG, FeatureExtractor, encoder_args
    fx = FeatureExtractor(encoder_args(IMAGE_TOWERS["vit_huge_14_224"], layers_num=vit_layers, dropout=0.0),
                          encoder_args(TEXT_CONFIG, layers_num=text_layers, dropout=0.0))
    assert fx.visual_projection is not None and tuple(fx.visual_projection.weight.shape) == (768, 1280)
    assert fx.vit_args.hidden_size // fx.vit_args.heads_num == 80 and fx.vit_args.max_seq_length == 257
    pv = {**{"embedding." + k: v for k, v in O.seeded_params(O.vit_embedding_spec(1280, 3, 14, 257), seed=291).items()},
          **{"encoder." + k: v for k, v in O.seeded_params(O.encoder_param_spec(vit_layers, 1280, 5120, True), seed=292).items()}}
    pt = {**{"embedding." + k: v for k, v in O.seeded_params(O.text_embedding_spec(768, 50265, 514), seed=64).items()},
          **{"encoder." + k: v for k, v in O.seeded_params(O.encoder_param_spec(text_layers, 768, 3072, False), seed=65).items()}}
    wp = torch.randn(768, 1280, generator=torch.Generator().manual_seed(293)) * 1280 ** -0.5      # CLIP's initialiser for `proj`
    fx.image.load_state_dict(pv, strict=True)
    fx.text.load_state_dict(pt, strict=True)
    fx.visual_projection.load_state_dict({"weight": wp}, strict=True)
    return fx.to(dev), pv, pt, wp


def test_vit_h14_full_width_two_layers_extract_and_train_match_oracle(dev):
    """ViT-H/14 at full width (2 of its 32 layers) + the 1280 -> 768 projection + RoBERTa-base (1 layer), one item x 2 frames x 1 tag:
    extract() within 1e-3 of the oracle chain (embedding -> encoder -> pooling 'first' -> projection), as smoke() asks of ViT-B; then one
    forward_train + backward_train: every gradient finite, the projection's against the oracle's autograd at REL."""
    from lr2ppo_amd import ops
    from lr2ppo_amd.finetune.features import synthetic_raw_batch
    fx, pv, pt, wp = _vit_h_extractor(dev)
    frames, ids, seg, _ = synthetic_raw_batch(1, 1, n_img=2, generator=torch.Generator().manual_seed(41))
    fx.eval()
    before = ops.self_attn_hd_launch_counts()
    text_emb, img_emb = fx.extract(frames.to(dev), ids.to(dev), seg.to(dev))
    assert ops.self_attn_hd_launch_counts()[0] == before[0] + 2                         # both ViT-H layers; RoBERTa's heads are 64 wide
    assert text_emb.shape == (1, 1, 196, 768) and img_emb.shape == (1, 2, 768)
    pvg = {k: v.clone().requires_grad_(True) for k, v in pv.items()}
    wpg = wp.clone().requires_grad_(True)
    text_ref, img_ref = O.feature_chain(pvg, pt, frames, ids, seg, patch=14, vit_layers=2, vit_heads=16, text_layers=1, proj=wpg)
    assert (text_emb.cpu() - text_ref.detach()).abs().max().item() < 1e-3 * max(1.0, float(text_ref.abs().max()))
    err = (img_emb.cpu() - img_ref.detach()).abs().max().item()
    print(f"  ViT-H/14 (2 layers) img_emb max err {err:.3e}, max|ref| {float(img_ref.abs().max()):.3e}")
    assert err < 1e-3 * max(1.0, float(img_ref.abs().max()))
    # ---- one training step's forward and backward (dropout 0: train mode computes what eval mode does) ----
    fx.train()
    fx.bind_grads()
    g = torch.Generator().manual_seed(42)
    d_text, d_img = torch.randn(text_emb.shape, generator=g), torch.randn(img_emb.shape, generator=g)
    t2, i2, ctx = fx.forward_train(frames.to(dev), ids.to(dev), seg.to(dev))
    assert (i2.cpu() - img_ref.detach()).abs().max().item() < 1e-3 * max(1.0, float(img_ref.abs().max()))
    fx.backward_train(ctx, d_text.to(dev), d_img.to(dev))
    for n, p in fx.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    (img_ref * d_img).sum().backward()
    r = _rel(fx.visual_projection.weight.grad, wpg.grad)
    print(f"  visual_projection.weight.grad rel L2 {r:.3e}")
    assert r < REL
    for n in ("encoder.transformer.0.self_attn.linear_layers.0.weight", "encoder.transformer.1.self_attn.final_linear.weight",
              "embedding.patch.projection.weight"):
        q = dict(fx.image.named_parameters())[n]
        assert _rel(q.grad, pvg[n].grad) < REL, (n, _rel(q.grad, pvg[n].grad))


def test_image_tower_flag_runs_one_stage1_step(dev):
    """`--raw_inputs --finetune_encoders --image_tower vit_huge_14_224 --encoder_layers 1 --batch_size 1` as the stage-1 launcher parses
    it -> build_extractor -> one finetune_pointwise_step (called directly: a launcher subprocess spends its time starting up)."""
    from lr2ppo_amd import ops
    from lr2ppo_amd.finetune import pointwise, ppo, reward_pair_dataloader
    from lr2ppo_amd.finetune.features import build_encoder_optimizer, build_extractor, finetune_pointwise_step, synthetic_raw_batch
    argv = ["--config_path", "c.json", "--output_model_path", "o.bin", "--raw_inputs", "--image_tower", "vit_huge_14_224",
            "--encoder_layers", "1", "--batch_size", "1", "--max_imgs", "2", "--max_tags", "1", "--seq_length", "196",
            "--visual_feat_dim", "768", "--mode", "reg"]
    for mod in (pointwise, reward_pair_dataloader, ppo):
        assert mod.build_parser().parse_args(argv).image_tower == "vit_huge_14_224", mod.__name__
    d = vars(pointwise.build_parser().parse_args(argv + ["--finetune_encoders"]))
    d.update(labels_num=3, is_master=True, optimizer="adamw", scheduler="linear", learning_rate=1e-4, train_steps=20, warmup=0.1,
             device=dev)
    args = argparse.Namespace(**d)
    torch.manual_seed(5)
    fx = build_extractor(args, trainable=True)
    assert len(fx.image.encoder.transformer) == 1 and fx.vit_args.hidden_size == 1280 and fx.visual_projection is not None
    model = pointwise.Classifier(args, None).to(dev).train()
    fx.train()
    opt, sch = pointwise.build_optimizer(args, model)
    eopt, esch = build_encoder_optimizer(args, fx)
    sch.step(), esch.step()                                                   # leave lambda(0) = 0
    frames, ids, seg, tgts = synthetic_raw_batch(1, 1, n_img=2, generator=torch.Generator().manual_seed(33))
    w0 = fx.image.encoder.transformer[0].self_attn.linear_layers[0].weight.detach().clone()
    before = ops.self_attn_hd_launch_counts()
    loss = finetune_pointwise_step(args, fx, model, opt, sch, eopt, esch, frames.to(dev), ids.to(dev), seg.to(dev), tgts.to(dev))
    after = ops.self_attn_hd_launch_counts()
    assert after[0] > before[0] and after[1] > before[1]
    assert bool(torch.isfinite(loss).all())
    w1 = fx.image.encoder.transformer[0].self_attn.linear_layers[0].weight.detach()
    assert bool(torch.isfinite(w1).all()) and not torch.equal(w0, w1)          # the tower behind the new attention was trained


def test_width_64_tower_launches_none_of_the_new_kernels(dev):
    from lr2ppo_amd import ops
    enc, _ = _tower(dev, 128, 2, True, seed=9)
    emb, seg, w = _inputs(128, seed=9)
    before = ops.self_attn_hd_launch_counts()
    enc.eval()
    with torch.no_grad():
        enc(emb.to(dev), seg.to(dev))
        enc.forward_first_token(emb.to(dev), seg.to(dev))
    enc.train()
    e = emb.to(dev).requires_grad_(True)
    (enc(e, seg.to(dev)) * w.to(dev)).sum().backward()
    assert bool(torch.isfinite(e.grad).all())
    assert ops.self_attn_hd_launch_counts() == before


@pytest.mark.parametrize("D", [1028, 1280, 1536])
def test_layernorm_wider_than_1024_columns_matches_fp64(dev, D):
    """ViT-H/14's rows are 1280 wide: lr2_layernorm_fwd_wide / lr2_layernorm_bwd_wide behind ops.layernorm_fwd / layernorm_bwd (six
    float4 per lane; 1028 = one element past the narrow kernels' range, 1536 = the last width served), through the LayerNorm module
    and its autograd, against the oracle's expression in fp64.  Rows: more than one workgroup's four, and no multiple of four."""
    from lr2ppo_amd.tencentpretrain.layers.layer_norm import LayerNorm
    g = torch.Generator().manual_seed(D)
    x, w = torch.randn(2, 11, D, generator=g) * 3 + 0.5, torch.randn(2, 11, D, generator=g)
    ln = LayerNorm(D).to(dev)
    with torch.no_grad():
        ln.gamma.copy_(torch.rand(D, generator=g) + 0.5)
        ln.beta.copy_(torch.randn(D, generator=g))
    xd = x.to(dev).requires_grad_(True)
    y = ln(xd)
    (y * w.to(dev)).sum().backward()
    x64 = x.double().requires_grad_(True)
    g64, b64 = ln.gamma.detach().double().cpu().requires_grad_(True), ln.beta.detach().double().cpu().requires_grad_(True)
    ref = O.layernorm_tp(x64, g64, b64)
    (ref * w.double()).sum().backward()
    assert _rel(y, ref) < 1e-6 and _rel(xd.grad, x64.grad) < 1e-5
    assert _rel(ln.gamma.grad, g64.grad) < 1e-5 and _rel(ln.beta.grad, b64.grad) < 1e-5
