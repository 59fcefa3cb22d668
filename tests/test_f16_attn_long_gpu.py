"""Key-blocked f16 attention above 288 tokens for the f16 inference mode: lr2_self_attn_fwd_f16_blocked
(csrc/selfattn_mx_blocked.hip) at the kernel level through ops.self_attn_fwd_f16_blocked, TransformerEncoder.f16_attention_long in
forward_f16 above it, and FeatureExtractor(precision="f16", f16_attention_long=True) at the top.

Structure, inputs and helpers are test_bf16_attn_infer_long_gpu.py's: attn_cases.exact_qkv at scale 1/8 -- small integers times a power
of two, every one exact in f16 (asserted: max |x| = 512), whose scores are exact in fp32 -- against attn_cases.reference in fp64, masks
laid on the forward key block read from ops.self_attn_bf16_blocked_plan(L)[0]; _check / _slack are test_bf16_attn_train_gpu.py's
(loaded as a module).  The gate on the fp32 context is derived, not measured:

    |O - ref| <= 1.5 * (2^-11 * (P |V|) + 2^-25 * sum_k |v_k|) + slack        slack = 2^-18 max(1, max|ref|), P from the fp64 reference

2^-11 is f16's unit roundoff on the un-normalised probability p~ in (0, 1]; below 2^-14 p~ is an f16 subnormal and its rounding error
is absolute, at most 2^-25, against a row sum l >= 1: the second term.  1.5 and the slack are the bf16 file's, for fp32 accumulation
and v_exp_f32.  The gate RELIES on the matrix core keeping f16 subnormal operands (a flush would cost up to 2^-14 per key, not 2^-25):
test_f16_mode_gpu.py::test_subnormal_operand_probe measured that it does (2^-20 x 2^10 -> 2^-10).  Every check prints the share of
the gate it reached (the largest measured is below).

The f16 plane is checked byte for byte against clamped round-to-nearest-even of the fp32 output.  Every output buffer starts as NaN
(fp32) or the pattern 0x7E00 (an f16 NaN) with a canary region behind it.

The random-data test is test_f16_mode_gpu.py::test_attention_plane_and_accuracy's assertion: the kernel's relative L2 from fp64 attention
of its own f16 operands is at most a QUARTER of ops.self_attn_fwd_bf16_blocked's from fp64 attention of its own bf16 operands (three
more significand bits: 8 expected, 4 asserted).

The schedule test has no derived bound; it measures against code this change does not touch, in the same run:
r288 = forward_f16 at L = 288 (the one-block f16 kernel) against the split-bf16 forward, r304 likewise at L = 304 with the switch on;
asserted r304 <= 2 r288 (both paths round at the same sites; the factor allows for length and draw) and r304 <= 1/4 of forward_bf16's
distance with infer_attention_long at L = 304 on the same inputs.

Measured on one MI355X (this file's own prints):

    forward_f16 vs the split-bf16 forward, rel. L2:   r288 (one-block kernel)   r304 (switch on)   r304 (switch off)   forward_bf16 at 304
        pre-LN                                        3.142e-5                  3.160e-5           3.157e-5            2.547e-4 (8.06 x)
        post-LN                                       3.158e-5                  3.158e-5           3.159e-5            2.533e-4 (8.02 x)

In the same run the fp32 context reached at most 0.524 of its derived gate (86 checks), the all-padding sequence |O - 1| = 1.2e-4
(gate 7.5e-4), the random-data distances were 1.75-1.83e-4 (f16) against 1.40-1.46e-3 (bf16), ratio 7.98-8.05, and the text features
of FeatureExtractor at L = 304 were 1.562e-4 (switch on) / 1.560e-4 (off) from the split-bf16 ones.
"""
import argparse
import importlib.util
import os

import pytest
import torch

import attn_cases as AC

pytestmark = pytest.mark.gpu


def _one_block_tests():
    """tests/test_bf16_attn_train_gpu.py as a module: _check and _slack"""
    spec = importlib.util.spec_from_file_location("_bf16_attn_train_gpu", os.path.join(os.path.dirname(__file__), "test_bf16_attn_train_gpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _one_block_tests()
_check, _slack = G._check, G._slack
H11, SUB = 2.0 ** -11, 2.0 ** -25      # f16's unit roundoff; half the smallest f16 subnormal: the absolute rounding error below 2^-14
NAN16 = 0x7E00                         # an f16 NaN: the clamping plane writer never produces it from a finite context
F16_MAX = 65504.0
SCALE, SMALL = 0.125, (2, 2)
LONG_L = (289, 320, 321, 384, 385, 448, 449, 512, 513, 514, 577, 768, 769, 1024, 1025)
SHORT_L = (1, 17, 160, 161, 257, 288)          # accepted by the entry point below its schedule's range
EDGE_L = LONG_L + SHORT_L
PEAKED_L = (289, 385, 449, 514)
_WORST = [0.0]                         # the largest share of the derived gate reached so far in this run


def _block(L):
    from lr2ppo_amd import ops
    return ops.self_attn_bf16_blocked_plan(L)[0]


def _rne_f16_bits(out):
    """the plane writer's rule on the host: clamp to +-65504, round to nearest even -> int16 bits"""
    return out.detach().float().cpu().clamp(-F16_MAX, F16_MAX).to(torch.float16).view(torch.int16).reshape(-1)


class Infer:
    """One problem on the device as ONE f16 plane [Q | K | V], and lr2_self_attn_fwd_f16_blocked on it.  Every output starts as a NaN
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
        assert torch.equal(x.to(torch.float16).float(), x), "every input is exact in f16"
        self.qkv = x.to(torch.float16).to(dev).contiguous()
        assert torch.equal(self.qkv.float().cpu(), x), "the plane holds the reference's numbers"
        self.kw = dict(batch=self.B, heads=self.H, L=self.L, head_dim=64, scale=SCALE)

    def run(self, which=("out", "plane")):
        """-> dict: "out" fp32 [n, E], "plane" int16 [n * E] for the outputs asked for"""
        n, E, dev = self.n, self.E, self.dev
        f = torch.full((n * E + E,), float("nan"), device=dev)
        p = torch.full((n * E + E,), NAN16, dtype=torch.int16, device=dev)
        self.ops.self_attn_fwd_f16_blocked(self.qkv, self.seg, out=f[:n * E].view(n, E) if "out" in which else None,
                                           out_plane=p[:n * E] if "plane" in which else None, **self.kw)
        torch.cuda.synchronize()
        assert bool(torch.isnan(f[n * E:]).all()) and bool((p[n * E:] == NAN16).all()), "written behind the last row"
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
    av = v.double().abs()
    bound = 1.5 * (H11 * (P @ av) + SUB * av.sum(dim=2, keepdim=True)) + _slack(o_ref)
    share = float(((o[sel].double() - o_ref.double()).abs() / bound).max())
    _WORST[0] = max(_WORST[0], share)
    print(f"    {what}share of the gate {share:.3f} (largest so far in this run: {_WORST[0]:.3f})")
    _check(what + "O", o[sel], o_ref, bound)


def _plane_is_rne_of_out(r):
    assert torch.equal(r["plane"].cpu(), _rne_f16_bits(r["out"])), "plane != RNE f16 (clamped) of out"


def _edge_case(i, batch, heads, L):
    """mask, planting position and span rotate with i (attn_cases.peaked_cases' pairs); the mask lies on the forward key block"""
    pos, mask, span, _ = AC.peaked_cases(i, L, 16)[(5 * i) % 16]
    block = _block(L)
    seg = AC.masks(batch, L, block)[mask]
    c = AC.exact_qkv(batch, heads, L, seed=500 + L, logit_span=span, scale=SCALE, plant=AC.plant_key(pos, L, block, seg))
    return c, seg, f"[{mask} {pos} span {span} block {block}] "


# ------------------------------------------------------------------------------------------------ 1. edges
@pytest.mark.parametrize("i", range(len(EDGE_L)), ids=[f"L{L}" for L in EDGE_L])
def test_edges(dev, i):
    """All 21 lengths against fp64 under the derived gate, which relies on the matrix core keeping f16 subnormal operands
    (test_f16_mode_gpu.py::test_subnormal_operand_probe measured that); the plane = RNE f16 (clamped) of the fp32 output; each output
    alone gives the combined call's bytes; the counter moves by one per call."""
    from lr2ppo_amd import ops
    batch, heads, L = SMALL + (EDGE_L[i],)
    c, seg, what = _edge_case(i, batch, heads, L)
    run = Infer(dev, c, seg)
    assert float(run.qkv.float().abs().max()) <= 512.0
    c0 = ops.self_attn_fwd_f16_blocked_launch_count()
    c1 = ops.self_attn_fwd_f16_launch_count()
    r = run.run()
    print(f"\n({run.B}, {run.H}, {run.L}) {what}")
    _gate_check(what, run.unheads(r["out"]), c, seg)
    _plane_is_rne_of_out(r)
    for which in (("out",), ("plane",)):          # each output alone: the combined call's bytes
        one = run.run(which)
        for name, t in one.items():
            bits = torch.int32 if name == "out" else torch.int16
            assert torch.equal(t.view(bits), r[name].view(bits)), (which, name)
    assert ops.self_attn_fwd_f16_blocked_launch_count() == c0 + 3
    assert ops.self_attn_fwd_f16_launch_count() == c1                  # the one-block entry point: not involved


# ------------------------------------------------------------------------------------------------ 2. peaked softmax
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


# ------------------------------------------------------------------------------------------------ 3. a sequence with no valid key
@pytest.mark.parametrize("L", [289, 449])
def test_all_padding_sequence(dev, L):
    """seg all 0 for the last sequence, V = 1: every context element is a convex combination of ones, P |V| = 1 and sum_k |v_k| = L"""
    batch, heads = SMALL
    seg = AC.masks(batch, L, _block(L))["none_valid"]
    assert not bool((seg[-1] > 0).any()) and bool((seg[0] > 0).all())
    c = AC.exact_qkv(batch, heads, L, seed=900 + L, logit_span=20, scale=SCALE)
    c = dict(c, v=torch.ones_like(c["v"]))
    out = Infer(dev, c, seg).run(("out",))["out"]
    assert bool(torch.isfinite(out).all())
    err = float((out.double() - 1.0).abs().max())
    gate = 1.5 * (H11 + L * SUB) + 2.0 ** -18
    print(f"\n({batch}, {heads}, {L}) none_valid, V = 1: max |O - 1| = {err:.3e} (gate {gate:.3e})")
    assert err <= gate


# ------------------------------------------------------------------------------------------------ 4. three more bits, on random data
def _attn_ref(qkv, seg, batch, L, heads):
    E = heads * 64
    q, k, v = (t.double().view(batch, L, heads, 64).transpose(1, 2) for t in qkv.split(E, dim=1))
    s = q @ k.transpose(-1, -2) * 0.125 + (seg <= 0).double()[:, None, None, :] * -10000.0
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(batch * L, E)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


@pytest.mark.parametrize("batch, heads", [(2, 4), (64, 4)])
@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("L", [289, 514])
def test_three_more_bits_than_the_bf16_kernel(dev, L, padded, batch, heads):
    """The kernel's distance (relative L2) from fp64 attention of its own f16 operands is at most a QUARTER of
    ops.self_attn_fwd_bf16_blocked's from fp64 attention of its own bf16 operands, on the same fp32 data: what remains is the 2-byte
    rounding of P, three bits finer (expected ratio 8; the factor 2 of margin covers fp32 accumulation and v_exp_f32)."""
    from lr2ppo_amd import ops
    E = heads * 64
    g = torch.Generator(device=dev).manual_seed(11)
    qkv32 = torch.randn(batch * L, 3 * E, device=dev, generator=g)
    seg = torch.ones(batch, L, dtype=torch.int64, device=dev)
    if padded:
        seg[:, (2 * L) // 3:] = 0
    kw = dict(batch=batch, heads=heads, L=L, head_dim=64, scale=0.125)
    qkv = qkv32.to(torch.float16)
    o32 = torch.full((batch * L, E), float("nan"), device=dev)
    ops.self_attn_fwd_f16_blocked(qkv, seg.view(-1), out=o32, **kw)
    assert bool(torch.isfinite(o32).all())
    d16 = _rel(o32, _attn_ref(qkv, seg, batch, L, heads))
    qkv_b = qkv32.to(torch.bfloat16)
    ob = torch.full((batch * L, E), float("nan"), device=dev)
    ops.self_attn_fwd_bf16_blocked(qkv_b, seg.view(-1), out=ob, **kw)
    dbf = _rel(ob, _attn_ref(qkv_b, seg, batch, L, heads))
    print(f"\nattention L={L} padded={padded} B={batch} H={heads}: f16 blocked {d16:.3e}, bf16 blocked {dbf:.3e}, "
          f"ratio {dbf / max(d16, 1e-30):.2f}")
    assert d16 <= dbf / 4


# ------------------------------------------------------------------------------------------------ 5. more workgroups than CUs
def test_more_workgroups_than_cus(dev):
    batch, heads, L = 256, 2, 289
    c, seg, what = _edge_case(3, batch, heads, L)
    print(f"\n({batch}, {heads}, {L}) {what}")
    run = Infer(dev, c, seg)
    r = run.run()
    _gate_check(what, run.unheads(r["out"]), c, seg, seqs=[0, 1, 254, 255])
    _plane_is_rne_of_out(r)


# ------------------------------------------------------------------------------------------------ 6. strided operands and outputs
def test_strides_through_the_c_abi(dev):
    """ld = 3E + 64, ld_o = E + 64 through the C ABI: the values of the contiguous call; the padding columns of the two outputs and the
    canaries behind them untouched (the operands' padding columns are NaN: never read)."""
    from lr2ppo_amd import _native, ops
    batch, heads, L = SMALL + (321,)
    c, seg, what = _edge_case(2, batch, heads, L)
    run = Infer(dev, c, seg)
    r = run.run()
    n, E = run.n, run.E
    ld, ld_o = 3 * E + 64, E + 64
    qkv = torch.full((n, ld), float("nan"), dtype=torch.float16, device=dev)
    qkv[:, :3 * E] = run.qkv
    f = torch.full((n * ld_o + E,), float("nan"), device=dev)
    p = torch.full((n * ld_o + E,), NAN16, dtype=torch.int16, device=dev)
    base = qkv.data_ptr()
    c0 = ops.self_attn_fwd_f16_blocked_launch_count()
    _native.check(_native.lib().lr2_self_attn_fwd_f16_blocked(base, base + 2 * E, base + 4 * E, ld, run.seg.data_ptr(), f.data_ptr(),
                                                              p.data_ptr(), ld_o, batch, heads, L, 64, SCALE, ops._stream()),
                  "lr2_self_attn_fwd_f16_blocked")
    torch.cuda.synchronize()
    assert ops.self_attn_fwd_f16_blocked_launch_count() == c0 + 1
    fm, pm = f[:n * ld_o].view(n, ld_o), p[:n * ld_o].view(n, ld_o)
    assert torch.equal(fm[:, :E], r["out"]) and torch.equal(pm[:, :E].reshape(-1), r["plane"])
    assert bool(torch.isnan(fm[:, E:]).all()) and bool((pm[:, E:] == NAN16).all())
    assert bool(torch.isnan(f[n * ld_o:]).all()) and bool((p[n * ld_o:] == NAN16).all())


# ------------------------------------------------------------------------------------------------ 7. determinism
def test_two_calls_give_the_same_bytes(dev):
    batch, heads, L = SMALL + (513,)
    c, seg, _ = _edge_case(8, batch, heads, L)
    run = Infer(dev, c, seg)
    a, b = run.run(), run.run()
    assert torch.equal(a["out"].view(torch.int32), b["out"].view(torch.int32)), "out"
    assert torch.equal(a["plane"], b["plane"]), "plane"


# ------------------------------------------------------------------------------------------------ 8. schedule
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


def _tower(dev, pre):
    """the bf16 file's tower: 2 layers, E = 128, 2 heads (head width 64); inputs at L = 288 and 304"""
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
def test_forward_f16_schedule(dev, pre):
    from lr2ppo_amd import ops
    enc, data = _tower(dev, pre)
    blocked, one_block = ops.self_attn_fwd_f16_blocked_launch_count, ops.self_attn_fwd_f16_launch_count
    (e288, s288), (e304, s304) = data[288], data[304]
    assert enc.f16_attention_long is False
    c, c1 = blocked(), one_block()
    off = enc.forward_f16(e304, s304).clone()
    assert blocked() == c and one_block() == c1                        # switch off: the 3-pass attention
    out288 = enc.forward_f16(e288, s288).clone()                       # the existing one-block f16 kernel
    assert blocked() == c and one_block() == c1 + 2
    ref288, ref304 = enc(e288, s288).clone(), enc(e304, s304).clone()  # the split-bf16 forward
    r288 = _rel(out288, ref288)
    enc.f16_attention_long = True
    on = enc.forward_f16(e304, s304).clone()
    assert blocked() == c + 2 and one_block() == c1 + 2                # L = 304: the new kernel, once per layer
    short = enc.forward_f16(e288, s288).clone()
    assert blocked() == c + 2 and one_block() == c1 + 4                # L = 288: the reverse
    assert torch.equal(short, out288)
    first = enc.forward_f16(e304, s304, first_only=True).clone()
    assert blocked() == c + 3                                          # the layers in front of the last
    r304, r304_off = _rel(on, ref304), _rel(off, ref304)
    enc.infer_attention_long = True
    rb304 = _rel(enc.forward_bf16(e304, s304), ref304)                 # the bf16 mode on its key-blocked kernel, same inputs
    for t in (off, on, first, short):
        assert bool(torch.isfinite(t).all())
    assert first.shape == (2, 128) and not torch.equal(on, off)
    print(f"\nSCHED f16 {'pre' if pre else 'post'}-LN: r288 {r288:.3e}  r304 {r304:.3e}  (ratio {r304 / r288:.2f}, gate 2)  "
          f"r304 switch off {r304_off:.3e}  bf16 mode at 304 {rb304:.3e} (ratio {rb304 / r304:.2f}, gate 4)  "
          f"first_only vs row 0: {_rel(first, on[:, 0, :]):.3e}")
    assert r304 <= 2.0 * r288
    assert r304 <= rb304 / 4


# ------------------------------------------------------------------------------------------------ 9. through the top
def test_feature_extractor(dev):
    from lr2ppo_amd import ops
    from lr2ppo_amd.finetune.features import TEXT_CONFIG, VIT_CONFIG, FeatureExtractor, encoder_args, synthetic_raw_batch

    def build(precision, **kw):
        torch.manual_seed(31)                                          # the same weights in every extractor
        fx = FeatureExtractor(encoder_args(VIT_CONFIG, layers_num=1), encoder_args(TEXT_CONFIG, layers_num=1), seq_length=304,
                              precision=precision, **kw)
        for n, p in fx.named_parameters():
            if "gamma" not in n and "beta" not in n:
                p.data.normal_(0, 0.02)
        return fx.to(dev).eval()

    frames, ids, seg, _ = synthetic_raw_batch(1, 2, n_img=2, seq_length=304, generator=torch.Generator().manual_seed(32))
    frames, ids, seg = frames.to(dev), ids.to(dev), seg.to(dev)
    ref = build("split_bf16").extract(frames, ids, seg)[0].clone()
    fx_off = build("f16")
    assert not fx_off.image.encoder.f16_attention_long and not fx_off.text.encoder.f16_attention_long
    c = ops.self_attn_fwd_f16_blocked_launch_count()
    off = fx_off.extract(frames, ids, seg)[0].clone()
    assert ops.self_attn_fwd_f16_blocked_launch_count() == c
    fx = build("f16", f16_attention_long=True)
    assert fx.image.encoder.f16_attention_long and fx.text.encoder.f16_attention_long
    text_emb, img_emb = fx.extract(frames, ids, seg)
    assert ops.self_attn_fwd_f16_blocked_launch_count() == c + 1       # the text tower's one layer at L = 304 (the image tower: L = 197)
    assert text_emb.shape == (1, 2, 304, 768) and bool(torch.isfinite(text_emb).all()) and bool(torch.isfinite(img_emb).all())
    d_on, d_off = _rel(text_emb, ref), _rel(off, ref)
    print(f"\nTOP f16 text features at L = 304 vs split-bf16: switch on {d_on:.3e}, off {d_off:.3e} (ratio {d_on / d_off:.2f}, gate 2)")
    assert d_on <= 2.0 * d_off
