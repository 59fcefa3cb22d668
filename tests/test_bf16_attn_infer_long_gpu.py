"""Single-plane bf16 attention above 288 tokens for the bf16 and MX-FP8 inference modes: lr2_self_attn_fwd_bf16_blocked
(csrc/selfattn_mx_blocked.hip) at the kernel level through ops.self_attn_fwd_bf16_blocked, TransformerEncoder.infer_attention_long in
forward_bf16 / forward_fp8 above it, and FeatureExtractor(precision="bf16", attention_long=True) at the top.

Method, inputs and reference are test_bf16_attn_train_gpu.py's (loaded as a module: _check, _slack, H8, NAN16): attn_cases.exact_qkv at
scale 1/8 -- bf16 numbers whose scores are exact in fp32 -- against attn_cases.reference in fp64, masks laid on the forward key block
read from ops.self_attn_bf16_blocked_plan(L)[0].  The gate on the fp32 context is that module's derived O gate without its last term (an
fp32 output has no plane rounding):

    |O - ref| <= 1.5 * 2^-8 * (P |V|) + slack          slack = 2^-18 max(1, max|ref|), P from the fp64 reference

The bf16 plane is checked byte for byte against round-to-nearest-even of the fp32 output, the MX-FP8 bytes and scales against
ops.quant_mxfp8 of it, and the plane against the training twin's (ops.self_attn_fwd_bf16_train without dropout: above 288 the blocked
training kernel this one restates; at 257 / 288 that entry point called directly).  Every output buffer starts as a NaN pattern (0x7FC0
for the plane, 0xFF bytes for MX-FP8: neither the saturating e4m3 conversion nor a scale byte e + 127 <= 254 produces 0xFF) with a canary
region behind it.

The schedule test has no derived bound; it measures against code this change does not touch, in the same run (one MI355X):

    forward_bf16 vs the split-bf16 forward, rel. L2:   e288 (one-block kernel)        e304 (switch on)        gate e304 <= 2 e288
        pre-LN                                         2.521e-4                       2.547e-4  (off: 2.545e-4)
        post-LN                                        2.514e-4                       2.533e-4  (off: 2.530e-4)
    forward_fp8, single-plane vs 3-pass attention:     d288 (LR2_FP8_ATTN 1 vs 0)     d304 (switch on vs off) gate d304 <= 2 d288
        pre-LN                                         4.669e-4                       4.643e-4
        post-LN                                        4.607e-4                       4.202e-4

(the factor 2: both paths round at the same sites; it allows for the difference in sequence length and draw).  In the same run the
fp32 context reached at most 0.59 of its derived gate (86 checks), the all-padding sequence |O - 1| = 1.3e-3 (gate 5.9e-3), and
no plane element differed from the training twin's at any of the 17 lengths.
"""
import argparse
import importlib.util
import os

import pytest
import torch

import attn_cases as AC

pytestmark = pytest.mark.gpu

def _one_block_tests():
    """tests/test_bf16_attn_train_gpu.py as a module: _check, _slack and the constants"""
    spec = importlib.util.spec_from_file_location("_bf16_attn_train_gpu", os.path.join(os.path.dirname(__file__), "test_bf16_attn_train_gpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _one_block_tests()
_check, _slack, H8, NAN16 = G._check, G._slack, G.H8, G.NAN16
SCALE, SMALL = 0.125, (2, 2)
LONG_L = (289, 320, 321, 384, 385, 448, 449, 512, 513, 514, 577, 768, 769, 1024, 1025)
SHORT_L = (1, 17, 160, 161, 257, 288)          # accepted by the entry point below its schedule's range
EDGE_L = LONG_L + SHORT_L
PEAKED_L = (289, 385, 449, 514)


def _block(L):
    from lr2ppo_amd import ops
    return ops.self_attn_bf16_blocked_plan(L)[0]


class Infer:
    """One problem on the device as ONE bf16 plane [Q | K | V], and lr2_self_attn_fwd_bf16_blocked on it.  Every output starts as a NaN
    pattern and has a canary region behind it; every call checks that the outputs asked for are written everywhere and that the canaries
    and the outputs not asked for are untouched."""

    def __init__(self, dev, c, seg):
        from lr2ppo_amd import ops
        self.ops, self.dev = ops, dev
        self.B, self.H, self.L, _ = c["q"].shape
        self.E = self.H * 64
        self.n = self.B * self.L
        self.seg = seg.reshape(-1).to(dev)
        x = AC.pack(c["q"], c["k"], c["v"])
        self.qkv = x.to(torch.bfloat16).to(dev).contiguous()
        assert torch.equal(self.qkv.float().cpu(), x), "the plane holds the reference's numbers"
        self.kw = dict(batch=self.B, heads=self.H, L=self.L, head_dim=64, scale=SCALE)

    def run(self, which=("out", "mx", "plane")):
        """-> dict: "out" fp32 [n, E], "plane" int16 [n * E], "q" uint8 [n * E], "s" uint8 [n * E / 32] for the outputs asked for"""
        n, E, dev = self.n, self.E, self.dev
        f = torch.full((n * E + E,), float("nan"), device=dev)
        p = torch.full((n * E + E,), NAN16, dtype=torch.int16, device=dev)
        q = torch.full((n * E + E,), 0xFF, dtype=torch.uint8, device=dev)
        s = torch.full((n * (E // 32) + E,), 0xFF, dtype=torch.uint8, device=dev)
        mx = self.ops.Mx8(q[:n * E], s[:n * (E // 32)], n, E)
        self.ops.self_attn_fwd_bf16_blocked(self.qkv, self.seg, out=f[:n * E].view(n, E) if "out" in which else None,
                                            out_mx=mx if "mx" in which else None, out_plane=p[:n * E] if "plane" in which else None,
                                            **self.kw)
        torch.cuda.synchronize()
        assert bool(torch.isnan(f[n * E:]).all()) and bool((p[n * E:] == NAN16).all()), "written behind the last row"
        assert bool((q[n * E:] == 0xFF).all()) and bool((s[n * (E // 32):] == 0xFF).all()), "written behind the last row (MX-FP8)"
        res = {}
        if "out" in which:
            assert bool(torch.isfinite(f[:n * E]).all()), "out: an element was not written"
            res["out"] = f[:n * E].view(n, E)
        else:
            assert bool(torch.isnan(f).all()), "out: written without being asked for"
        if "plane" in which:
            assert not bool((p[:n * E] == NAN16).any()), "plane: an element was not written"
            res["plane"] = p[:n * E]
        else:
            assert bool((p == NAN16).all()), "plane: written without being asked for"
        if "mx" in which:
            assert not bool((q[:n * E] == 0xFF).any()) and not bool((s[:n * (E // 32)] == 0xFF).any()), "mx: an element was not written"
            res["q"], res["s"] = q[:n * E], s[:n * (E // 32)]
        else:
            assert bool((q == 0xFF).all()) and bool((s == 0xFF).all()), "mx: written without being asked for"
        return res

    def unheads(self, out):
        return AC.unpack(out.float().cpu().view(self.n, self.E), self.B, self.H, self.L)[0]


def _gate_check(what, o, c, seg, seqs=None):
    """the fp32 context of the sequences `seqs` against fp64 under the derived gate (module docstring)"""
    sel = slice(None) if seqs is None else seqs
    q, k, v, sg = (t[sel] for t in (c["q"], c["k"], c["v"], seg))
    o_ref, _ = AC.reference(q, k, v, sg, SCALE)
    nb, L = q.shape[0], q.shape[2]
    s = q.double() @ k.double().transpose(-1, -2) * SCALE + (sg.view(nb, 1, 1, L) <= 0).double() * AC.MASK
    P = torch.softmax(s, dim=-1)
    _check(what + "O", o[sel], o_ref, 1.5 * H8 * (P @ v.double().abs()) + _slack(o_ref))


def _same_as_rounding_and_quantising(r, ops):
    """the plane = RNE of the fp32 output, the MX-FP8 output = ops.quant_mxfp8 of it, byte for byte"""
    out = r["out"]
    assert torch.equal(r["plane"], out.to(torch.bfloat16).view(torch.int16).reshape(-1)), "plane != RNE(out)"
    ref = ops.quant_mxfp8(out.contiguous())
    n, E = out.shape
    assert torch.equal(r["q"], ref.q[:n * E]), "MX-FP8 bytes != quant_mxfp8(out)"
    assert torch.equal(r["s"], ref.s[:n * (E // 32)]), "MX-FP8 scales != quant_mxfp8(out)"


def _edge_case(i, batch, heads, L):
    """mask, planting position and span rotate with i (attn_cases.peaked_cases' pairs); the mask lies on the forward key block"""
    pos, mask, span, _ = AC.peaked_cases(i, L, 16)[(5 * i) % 16]
    block = _block(L)
    seg = AC.masks(batch, L, block)[mask]
    c = AC.exact_qkv(batch, heads, L, seed=500 + L, logit_span=span, scale=SCALE, plant=AC.plant_key(pos, L, block, seg))
    return c, seg, f"[{mask} {pos} span {span} block {block}] "


_EDGE = {}


def _edge_run(dev, i):
    """the i-th edge length's problem and its combined call, made once and shared by the edge test and the twin test"""
    if i not in _EDGE:
        batch, heads, L = SMALL + (EDGE_L[i],)
        c, seg, what = _edge_case(i, batch, heads, L)
        run = Infer(dev, c, seg)
        _EDGE[i] = (c, seg, what, run, run.run())
    return _EDGE[i]


# ------------------------------------------------------------------------------------------------ 1. edges
@pytest.mark.parametrize("i", range(len(EDGE_L)), ids=[f"L{L}" for L in EDGE_L])
def test_edges(dev, i):
    from lr2ppo_amd import ops
    c, seg, what, run, r = _edge_run(dev, i)
    print(f"\n({run.B}, {run.H}, {run.L}) {what}")
    c0 = ops.self_attn_fwd_bf16_blocked_launch_count()
    _gate_check(what, run.unheads(r["out"]), c, seg)
    _same_as_rounding_and_quantising(r, ops)
    for which in (("out",), ("mx",), ("plane",)):          # each output alone: the combined call's bytes
        one = run.run(which)
        for name, t in one.items():
            assert torch.equal(t, r[name]), (which, name)
    assert ops.self_attn_fwd_bf16_blocked_launch_count() == c0 + 3


# ------------------------------------------------------------------------------------------------ 2. the training twin's arithmetic
@pytest.mark.parametrize("i", [j for j, L in enumerate(EDGE_L) if L > 288 or L in (257, 288)],
                         ids=[f"L{L}" for L in EDGE_L if L > 288 or L in (257, 288)])
def test_plane_is_the_training_twins(dev, i):
    """Byte for byte: above 288 ops.self_attn_fwd_bf16_train(drop=None) is the merged blocked kernel at drop_p = 0; at 257 and 288 that
    kernel is reached through its entry point (ops sends these lengths to the one-block kernel)."""
    from lr2ppo_amd import _native, ops
    c, seg, what, run, r = _edge_run(dev, i)
    n, E, L = run.n, run.E, run.L
    twin = torch.full((n * E + E,), NAN16, dtype=torch.int16, device=dev)
    before = ops.self_attn_bf16_blocked_launch_counts()
    if L > 288:
        ops.self_attn_fwd_bf16_train(run.qkv, run.seg, twin[:n * E], drop=None, **run.kw)
    else:
        qp, kp, vp = ops._qkv_ptrs(run.qkv, E)
        _native.check(_native.lib().lr2_self_attn_fwd_bf16_train_blocked(qp, kp, vp, 3 * E, run.seg.data_ptr(), twin.data_ptr(), E, None,
                                                                         0.0, 0, 0, run.B, run.H, L, 64, SCALE, ops._stream()),
                      "lr2_self_attn_fwd_bf16_train_blocked")
    torch.cuda.synchronize()
    assert ops.self_attn_bf16_blocked_launch_counts() == (before[0] + 1, before[1])          # the blocked training forward ran
    assert bool((twin[n * E:] == NAN16).all())
    diff = int((twin[:n * E] != r["plane"]).sum())
    print(f"\n({run.B}, {run.H}, {L}) {what}: {diff} of {n * E} plane elements differ from the training twin's")
    assert diff == 0


# ------------------------------------------------------------------------------------------------ 3. peaked softmax
@pytest.mark.parametrize("mask", AC.MASKS)
@pytest.mark.parametrize("L", PEAKED_L)
def test_peaked_softmax_on_every_forward_block(dev, L, mask):
    """All four planting positions of one mask: prefix_block puts a first key block with no valid key, block2 / masked a row maximum
    behind the first block, masked the maximum on a masked key -- on every forward block size (160 / 192 / 224), two | three blocks."""
    batch, heads = SMALL
    i = PEAKED_L.index(L)
    pairs = [cse for cse in AC.peaked_cases(i, L, 16) if cse[1] == mask]
    assert [cse[0] for cse in pairs] == list(AC.POSITIONS)
    block = _block(L)
    seg = AC.masks(batch, L, block)[mask]
    for pos, _, span, _ in pairs:
        c = AC.exact_qkv(batch, heads, L, seed=600 + L, logit_span=span, scale=SCALE, plant=AC.plant_key(pos, L, block, seg))
        what = f"[{mask} {pos} span {span} block {block}] "
        print(f"\n({batch}, {heads}, {L}) {what}")
        run = Infer(dev, c, seg)
        _gate_check(what, run.unheads(run.run(("out",))["out"]), c, seg)


# ------------------------------------------------------------------------------------------------ 4. a sequence with no valid key
@pytest.mark.parametrize("L", [289, 449])
def test_all_padding_sequence(dev, L):
    """seg all 0 for the last sequence, V = 1: every context element is a convex combination of ones, P |V| = 1 in the gate"""
    batch, heads = SMALL
    seg = AC.masks(batch, L, _block(L))["none_valid"]
    assert not bool((seg[-1] > 0).any()) and bool((seg[0] > 0).all())
    c = AC.exact_qkv(batch, heads, L, seed=900 + L, logit_span=20, scale=SCALE)
    c = dict(c, v=torch.ones_like(c["v"]))
    out = Infer(dev, c, seg).run(("out",))["out"]
    assert bool(torch.isfinite(out).all())
    err = float((out.double() - 1.0).abs().max())
    print(f"\n({batch}, {heads}, {L}) none_valid, V = 1: max |O - 1| = {err:.3e} (gate {1.5 * H8:.3e})")
    assert err <= 1.5 * H8


# ------------------------------------------------------------------------------------------------ 5. more workgroups than CUs
def test_more_workgroups_than_cus(dev):
    from lr2ppo_amd import ops
    batch, heads, L = 256, 2, 289
    c, seg, what = _edge_case(3, batch, heads, L)
    print(f"\n({batch}, {heads}, {L}) {what}")
    run = Infer(dev, c, seg)
    r = run.run()
    _gate_check(what, run.unheads(r["out"]), c, seg, seqs=[0, 1, 254, 255])
    _same_as_rounding_and_quantising(r, ops)


# ------------------------------------------------------------------------------------------------ 6. strided operands and outputs
def test_strided_outputs(dev):
    """ld = 3E + 64, ld_o = E + 64 through the C ABI: the values of the contiguous call; the padding columns of the three outputs and
    of the scale matrix [rows, ld_o / 32] and the canaries behind them untouched (the operands' padding columns are NaN: never read)."""
    from lr2ppo_amd import _native, ops
    batch, heads, L = SMALL + (321,)
    c, seg, what = _edge_case(2, batch, heads, L)
    run = Infer(dev, c, seg)
    r = run.run()
    n, E = run.n, run.E
    ld, ld_o = 3 * E + 64, E + 64
    qkv = torch.full((n, ld), float("nan"), dtype=torch.bfloat16, device=dev)
    qkv[:, :3 * E] = run.qkv
    f = torch.full((n * ld_o + E,), float("nan"), device=dev)
    p = torch.full((n * ld_o + E,), NAN16, dtype=torch.int16, device=dev)
    q = torch.full((n * ld_o + E,), 0xFF, dtype=torch.uint8, device=dev)
    s = torch.full((n * (ld_o // 32) + E,), 0xFF, dtype=torch.uint8, device=dev)
    base = qkv.data_ptr()
    c0 = ops.self_attn_fwd_bf16_blocked_launch_count()
    _native.check(_native.lib().lr2_self_attn_fwd_bf16_blocked(base, base + 2 * E, base + 4 * E, ld, run.seg.data_ptr(), f.data_ptr(),
                                                               q.data_ptr(), s.data_ptr(), p.data_ptr(), ld_o, batch, heads, L, 64, SCALE,
                                                               ops._stream()), "lr2_self_attn_fwd_bf16_blocked")
    torch.cuda.synchronize()
    assert ops.self_attn_fwd_bf16_blocked_launch_count() == c0 + 1
    fm, pm, qm = f[:n * ld_o].view(n, ld_o), p[:n * ld_o].view(n, ld_o), q[:n * ld_o].view(n, ld_o)
    sm = s[:n * (ld_o // 32)].view(n, ld_o // 32)
    assert torch.equal(fm[:, :E], r["out"]) and torch.equal(pm[:, :E].reshape(-1), r["plane"])
    assert torch.equal(qm[:, :E].reshape(-1), r["q"]) and torch.equal(sm[:, :E // 32].reshape(-1), r["s"])
    assert bool(torch.isnan(fm[:, E:]).all()) and bool((pm[:, E:] == NAN16).all()) and bool((qm[:, E:] == 0xFF).all())
    assert bool((sm[:, E // 32:] == 0xFF).all())
    assert bool(torch.isnan(f[n * ld_o:]).all()) and bool((p[n * ld_o:] == NAN16).all()) and bool((q[n * ld_o:] == 0xFF).all())
    assert bool((s[n * (ld_o // 32):] == 0xFF).all())


# ------------------------------------------------------------------------------------------------ 7. determinism
def test_two_calls_give_the_same_bytes(dev):
    batch, heads, L = SMALL + (513,)
    c, seg, _ = _edge_case(8, batch, heads, L)
    run = Infer(dev, c, seg)
    a, b = run.run(), run.run()
    assert torch.equal(a["out"].view(torch.int32), b["out"].view(torch.int32)), "out"
    for name in ("plane", "q", "s"):
        assert torch.equal(a[name], b[name]), name


# ------------------------------------------------------------------------------------------------ 8. schedules
def _enc_args(**over):
    from lr2ppo_amd.tencentpretrain.opts import finetune_opts, tokenizer_opts
    p = argparse.ArgumentParser()
    finetune_opts(p)
    tokenizer_opts(p)
    d = vars(p.parse_args([]))
    d.update(dict(emb_size=128, feedforward_size=512, hidden_size=128, hidden_act="gelu", heads_num=2, layers_num=2, dropout=0.0,
                  max_seq_length=514, embedding=["word", "pos", "seg"], encoder="transformer", mask="fully_visible"))
    d.update(over)
    return argparse.Namespace(**d)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def _tower(dev, pre):
    """a 2-layer tower, E = 128, 2 heads (head width 64), built like test_bf16_mode_gpu's L = 304 case; inputs at L = 288 and 304"""
    from lr2ppo_amd.tencentpretrain.encoders import str2encoder
    torch.manual_seed(15)
    enc = str2encoder["transformer"](_enc_args(layernorm_positioning="pre" if pre else "post"))
    for n, p in enc.named_parameters():
        if "gamma" not in n and "beta" not in n:
            p.data.normal_(0, 0.02)
    enc = enc.to(dev).eval()
    data = {}
    for L in (288, 304):
        emb = torch.randn(2, L, 128, device=dev, generator=torch.Generator(device=dev).manual_seed(16 + L))
        data[L] = (emb, torch.ones(2, L, dtype=torch.int64, device=dev))
    return enc, data


@pytest.mark.parametrize("pre", [True, False], ids=["pre_ln", "post_ln"])
def test_forward_bf16_schedule(dev, pre):
    from lr2ppo_amd import ops
    enc, data = _tower(dev, pre)
    count = ops.self_attn_fwd_bf16_blocked_launch_count
    (e288, s288), (e304, s304) = data[288], data[304]
    c = count()
    off = enc.forward_bf16(e304, s304)
    assert count() == c                                                # switch off: the 3-pass attention
    out288 = enc.forward_bf16(e288, s288)                              # the existing one-block single-plane kernel
    r288 = _rel(out288, enc(e288, s288))
    enc.infer_attention_long = True
    assert count() == c
    on = enc.forward_bf16(e304, s304)
    assert count() == c + 2                                            # once per layer
    first = enc.forward_bf16(e304, s304, first_only=True)
    assert count() == c + 3                                            # the layers in front of the last
    short = enc.forward_bf16(e288, s288)
    assert count() == c + 3                                            # L <= 288: unaffected
    assert torch.equal(short, out288)
    r304 = _rel(on, enc(e304, s304))
    for t in (off, on, first, short):
        assert bool(torch.isfinite(t).all())
    assert first.shape == (2, 128) and not torch.equal(on, off)
    print(f"\nSCHED bf16 {'pre' if pre else 'post'}-LN: e288 {r288:.3e}  e304 {r304:.3e}  (ratio {r304 / r288:.2f}, gate 2; "
          f"switch off at 304: {_rel(off, enc(e304, s304)):.3e}; first_only vs row 0: {_rel(first, on[:, 0, :]):.3e})")
    assert r304 <= 2.0 * r288


@pytest.mark.parametrize("pre", [True, False], ids=["pre_ln", "post_ln"])
def test_forward_fp8_schedule(dev, pre, monkeypatch):
    from lr2ppo_amd import ops
    enc, data = _tower(dev, pre)
    count = ops.self_attn_fwd_bf16_blocked_launch_count
    (e288, s288), (e304, s304) = data[288], data[304]
    monkeypatch.setenv("LR2_FP8_ATTN", "1")
    c = count()
    off = enc.forward_fp8(e304, s304)
    fast288 = enc.forward_fp8(e288, s288)
    monkeypatch.setenv("LR2_FP8_ATTN", "0")
    slow288 = enc.forward_fp8(e288, s288)
    enc.infer_attention_long = True
    forced = enc.forward_fp8(e304, s304)                               # LR2_FP8_ATTN=0 still forces the 3-pass branch
    assert count() == c and torch.equal(forced, off)
    monkeypatch.setenv("LR2_FP8_ATTN", "1")
    on = enc.forward_fp8(e304, s304)
    assert count() == c + 2
    first = enc.forward_fp8(e304, s304, first_only=True)
    assert count() == c + 3
    short = enc.forward_fp8(e288, s288)
    assert count() == c + 3 and torch.equal(short, fast288)
    for t in (off, on, first, fast288, slow288):
        assert bool(torch.isfinite(t).all())
    d288, d304 = _rel(fast288, slow288), _rel(on, off)
    print(f"\nSCHED fp8 {'pre' if pre else 'post'}-LN: d288 {d288:.3e}  d304 {d304:.3e}  (ratio {d304 / d288:.2f}, gate 2; "
          f"vs split-bf16 at 304: on {_rel(on, enc(e304, s304)):.3e}, off {_rel(off, enc(e304, s304)):.3e})")
    assert first.shape == (2, 128) and not torch.equal(on, off)
    assert d304 <= 2.0 * d288


# ------------------------------------------------------------------------------------------------ 9. through the top
def test_feature_extractor(dev):
    from lr2ppo_amd import ops
    from lr2ppo_amd.finetune.features import TEXT_CONFIG, VIT_CONFIG, FeatureExtractor, encoder_args, synthetic_raw_batch
    torch.manual_seed(31)
    fx = FeatureExtractor(encoder_args(VIT_CONFIG, layers_num=1), encoder_args(TEXT_CONFIG, layers_num=1), seq_length=304,
                          precision="bf16", attention_long=True)
    for n, p in fx.named_parameters():
        if "gamma" not in n and "beta" not in n:
            p.data.normal_(0, 0.02)
    fx = fx.to(dev).eval()
    assert fx.image.encoder.infer_attention_long and fx.text.encoder.infer_attention_long
    frames, ids, seg, _ = synthetic_raw_batch(1, 2, n_img=2, seq_length=304, generator=torch.Generator().manual_seed(32))
    c = ops.self_attn_fwd_bf16_blocked_launch_count()
    text_emb, img_emb = fx.extract(frames.to(dev), ids.to(dev), seg.to(dev))
    assert ops.self_attn_fwd_bf16_blocked_launch_count() == c + 1          # the text tower's one layer at L = 304 (the image tower: L = 197)
    assert text_emb.shape == (1, 2, 304, 768) and bool(torch.isfinite(text_emb).all()) and bool(torch.isfinite(img_emb).all())
