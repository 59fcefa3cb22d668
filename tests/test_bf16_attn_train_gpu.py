"""Single-plane bf16 attention of the bf16_train mode: lr2_self_attn_fwd_bf16_train / lr2_self_attn_bwd_bf16 (csrc/selfattn_b1_train.hip)
at the kernel level, and TransformerEncoder.bf16_attention / FeatureExtractor(precision="bf16_train", bf16_attention=True) above them.

Kernel level.  Inputs are attn_cases.exact_qkv at scale 1/8: bf16 numbers with scores that are exact in fp32, so the only rounding left
is what these kernels add -- the bf16 A fragments P~ M (forward), dS (both backward kernels), Pd = P o M (dK / dV kernel) and the bf16
output planes.  The reference is attn_cases.reference in fp64 with oracle.lr2ppo_oracle.attention_keep_mask.  Gates are derived, not
measured: the half-ulp of bf16 is 2^-8 relative, so per element, with P, M = keep / (1 - p) and dS from the fp64 reference,

    |O  - ref| <= 1.5 * 2^-8 * (P o M)   |V|  + slack + 2^-8 |ref|
    |dQ - ref| <= 1.5 * 2^-8 * |dS|      |K|  + slack + 2^-8 |ref|
    |dK - ref| <= 1.5 * 2^-8 * |dS|^T    |Q|  + slack + 2^-8 |ref|
    |dV - ref| <= 1.5 * 2^-8 * (P o M)^T |dO| + slack + 2^-8 |ref|          slack = 2^-18 max(1, max|ref|)

(the last term: the output plane's own rounding).  A CPU emulation of the specified rounding over L in {1, 17, 65, 129, 225, 257, 288},
four masks, spans 2 / 20 / 100 and p in {0, 0.1, 0.5} reaches 0.89 (O), 1.03 (dQ), 0.94 (dK), 0.92 (dV) of the 2^-8 bound without the
factor 1.5, i.e. at most 0.69 of these gates; a wrong index, mask or operand is O(1).  lse: the existing 1e-5 + 1e-5 |ref|.

Measured gates (the rest is derived), one MI355X:

    gate                                                     measured                       margin   where
    all-padding sequence, dQ / dK / dV, rel. L2 vs fp64      2.73e-3 (18 gradients)         4 x      test_all_padding_sequence
    schedule vs torch emulation, worst rel. L2               1.37e-3 / 1.52e-3 (pre / post) 3 x      test_schedule_against_a_torch_emulation
    bf16_attention vs split-bf16, rel. L2 per tensor         MEASURED (pre, post)           1.5 x, floor 1e-3   test_gradients_against_split_bf16

Every derived gate measured at most 0.81 x in the same run (198 checks; the largest: dQ at (2, 2, 288), mask prefix_block, maximum planted on a masked key, span 2, p = 0).
"""
import argparse
import importlib.util
import os

import numpy as np
import pytest
import torch

import attn_cases as AC
from oracle import lr2ppo_oracle as O

pytestmark = pytest.mark.gpu

H8 = 2.0 ** -8
NAN16 = 0x7FC0
SCALE = 0.125
SMALL = (2, 2)
EDGE_L = (1, 15, 16, 17, 64, 65, 128, 129, 224, 225, 257, 288)          # both sides of every instantiation's edge (NT 4 / 8 / 14 / 18)
MANY = (256, 1, 33)                                                      # more pairs than CUs

# relative L2 against fp64 of (dQ, dK, dV) of the all-padding sequence: the maximum over the cases of test_all_padding_sequence
# (L = 33 / 200 / 257 at p = 0 and 0.1: 2.01e-3 .. 2.73e-3, the largest dK at L = 33, p = 0.1), measured on one MI355X; the gate is 4 x
_PAD_BWD_MEASURED = 2.73e-3


def _bf16_train_tests():
    """tests/test_bf16_train_gpu.py as a module: its small towers, its torch emulation's pieces and its measured table"""
    spec = importlib.util.spec_from_file_location("_bf16_train_gpu", os.path.join(os.path.dirname(__file__), "test_bf16_train_gpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _check(what, got, ref, bound):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert torch.isfinite(got).all(), f"{what}: not finite"
    err = (got - ref).abs()
    worst = float((err / bound.clamp(min=1e-300)).max()) if err.numel() else 0.0
    print(f"    {what}: max err {float(err.max()) if err.numel() else 0.0:.3e}, worst err / gate {worst:.3f}")
    assert bool((err <= bound).all()), f"{what}: max err {float(err.max()):.3e}, {worst:.2f} x the gate, {int((err > bound).sum())} bad"


def _slack(ref):
    return 2.0 ** -18 * max(1.0, float(ref.abs().max()))


class Run:
    """One problem on the device as single bf16 planes, and the two entry points on it.  Every output is filled with a NaN pattern and
    has one canary row group (E elements) behind it; every call checks that all of the output is finite and the canaries untouched."""

    def __init__(self, dev, c, seg, scale=SCALE):
        from lr2ppo_amd import ops
        self.ops, self.dev, self.scale = ops, dev, scale
        self.B, self.H, self.L, _ = c["q"].shape
        self.E = self.H * 64
        self.n = self.B * self.L
        self.seg_cpu = seg
        self.seg = seg.reshape(-1).to(dev)
        x, g = AC.pack(c["q"], c["k"], c["v"]), AC.pack(c["do"])
        self.qkv, self.do = x.to(torch.bfloat16).to(dev).contiguous(), g.to(torch.bfloat16).to(dev).contiguous()
        assert torch.equal(self.qkv.float().cpu(), x) and torch.equal(self.do.float().cpu(), g), "the planes hold the reference's numbers"
        self.q, self.k, self.v, self.g = c["q"], c["k"], c["v"], c["do"]
        self.kw = dict(batch=self.B, heads=self.H, L=self.L, head_dim=64, scale=scale)

    def _plane(self, rows, cols):
        buf = torch.full((rows * cols + self.E,), NAN16, dtype=torch.int16, device=self.dev)
        return buf[:rows * cols], buf[rows * cols:]

    def _f32(self, numel):
        buf = torch.full((numel + self.E,), float("nan"), device=self.dev)
        return buf[:numel], buf[numel:]

    @staticmethod
    def _intact(name, canary):
        if canary.dtype == torch.int16:
            assert bool((canary == NAN16).all()), f"{name}: written behind the last row"
        else:
            assert bool(torch.isnan(canary).all()), f"{name}: written behind the last row"

    def unheads(self, plane, cols):
        return AC.unpack(plane.view(torch.bfloat16).float().cpu().view(self.n, cols), self.B, self.H, self.L)

    def fwd(self, drop=None, with_lse=True):
        """(O [B, H, L, 64], lse [B, H, L] or None, the output plane's bytes)"""
        (o, oc), (lse, lc) = self._plane(self.n, self.E), self._f32(self.B * self.H * self.L)
        self.ops.self_attn_fwd_bf16_train(self.qkv, self.seg, o, lse=lse if with_lse else None, drop=drop, **self.kw)
        self._intact("o", oc), self._intact("lse", lc)
        (out,) = self.unheads(o, self.E)
        assert torch.isfinite(out).all(), "o: an element was not written"
        if with_lse:
            assert torch.isfinite(lse).all(), "lse: an element was not written"
        else:
            assert bool(torch.isnan(lse).all()), "lse: written without being asked for"
        return out, (lse.view(self.B, self.H, self.L).cpu() if with_lse else None), o

    def bwd(self, drop=None):
        """(dQ, dK, dV, lse workspace [B, H, L], the dQKV plane's bytes)"""
        d, dc = self._plane(self.n, 3 * self.E)
        (ws1, c1), (ws2, c2) = self._f32(self.B * self.H * self.L), self._f32(self.B * self.H * self.L)
        self.ops.self_attn_bwd_bf16(self.qkv, self.do, self.seg, d, ws1, ws2, drop=drop, **self.kw)
        self._intact("dqkv", dc), self._intact("lse_ws", c1), self._intact("dsum_ws", c2)
        dq, dk, dv = self.unheads(d, 3 * self.E)
        for name, t in (("dq", dq), ("dk", dk), ("dv", dv), ("lse_ws", ws1), ("dsum_ws", ws2)):
            assert torch.isfinite(t).all(), f"{name}: an element was not written"
        return dq, dk, dv, ws1.view(self.B, self.H, self.L).cpu(), d

    def keep(self, drop):
        return None if drop is None else O.attention_keep_mask(drop.seed, drop.site, self.B, self.H, self.L, drop.p)

    def check(self, drop=None, seqs=None, what=""):
        """forward, lse and the three gradients against fp64 under the derived gates (module docstring); seqs: of these sequences only"""
        p = drop.p if drop is not None else 0.0
        keep = self.keep(drop)
        o, lse, _ = self.fwd(drop)
        dq, dk, dv, lse_ws, _ = self.bwd(drop)
        sel = slice(None) if seqs is None else seqs
        q, k, v, g, seg = (t[sel] for t in (self.q, self.k, self.v, self.g, self.seg_cpu))
        keep_s = keep[sel] if keep is not None else None
        o_ref, lse_ref, dq_ref, dk_ref, dv_ref = AC.reference(q, k, v, seg, self.scale, keep=keep_s, p=p, do=g)
        # P, M and dS of the fp64 reference: what the gates are made of
        nb, L = q.shape[0], self.L
        s = q.double() @ k.double().transpose(-1, -2) * self.scale + (seg.view(nb, 1, 1, L) <= 0).double() * AC.MASK
        P = torch.softmax(s, dim=-1)
        M = torch.ones_like(P) if keep is None else torch.as_tensor(np.asarray(keep_s, dtype=np.float64)).view(nb, self.H, L, L) / (1.0 - p)
        dP = (g.double() @ v.double().transpose(-1, -2)) * M
        dS = P * (dP - (dP * P).sum(-1, keepdim=True)) * self.scale
        PM = P * M
        gate = lambda prod, ref: 1.5 * H8 * prod + _slack(ref) + H8 * ref.abs()          # noqa: E731
        _check(what + "O", o[sel], o_ref, gate(PM @ v.double().abs(), o_ref))
        _check(what + "lse", lse[sel], lse_ref, 1e-5 + 1e-5 * lse_ref.abs())
        _check(what + "lse_ws", lse_ws[sel], lse_ref, 1e-5 + 1e-5 * lse_ref.abs())
        _check(what + "dQ", dq[sel], dq_ref, gate(dS.abs() @ k.double().abs(), dq_ref))
        _check(what + "dK", dk[sel], dk_ref, gate(dS.abs().transpose(-1, -2) @ q.double().abs(), dk_ref))
        _check(what + "dV", dv[sel], dv_ref, gate(PM.transpose(-1, -2) @ g.double().abs(), dv_ref))
        return o, dq, dk, dv


def _drop(p, seed=20260, site=3):
    from lr2ppo_amd import ops
    return ops.Drop(p, seed, site) if p > 0 else None


def _edge_case(i, batch, heads, L):
    """The i-th edge shape's (inputs, seg): mask, planting position and span rotate with i (attn_cases.peaked_cases' pairs)."""
    pos, mask, span, _ = AC.peaked_cases(i, L, 16)[(5 * i) % 16]
    seg = AC.masks(batch, L, 288)[mask]
    c = AC.exact_qkv(batch, heads, L, seed=500 + L, logit_span=span, scale=SCALE, plant=AC.plant_key(pos, L, 288, seg))
    return c, seg, f"[{mask} {pos} span {span}] "


# ------------------------------------------------------------------------------------------------ 1. edges of every instantiation
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("i", range(len(EDGE_L) + 1), ids=[f"L{L}" for L in EDGE_L] + ["many_pairs"])
def test_edges_of_every_instantiation(dev, i, p):
    batch, heads, L = SMALL + (EDGE_L[i],) if i < len(EDGE_L) else MANY
    c, seg, what = _edge_case(i, batch, heads, L)
    print(f"\n({batch}, {heads}, {L}) p = {p} {what}")
    Run(dev, c, seg).check(_drop(p), what=what)


# ------------------------------------------------------------------------------------------------ 2. dropout replay
@pytest.mark.parametrize("p", [0.5, 0.9])
@pytest.mark.parametrize("L", [33, 200, 257])
def test_dropout_replay(dev, L, p):
    """Forward and backward given the same (seed, site) apply the mask oracle.attention_keep_mask describes; another site and another
    seed give other results."""
    batch, heads = SMALL
    seg = AC.masks(batch, L, 288)["suffix"]
    c = AC.exact_qkv(batch, heads, L, seed=700 + L, logit_span=2, scale=SCALE)
    r = Run(dev, c, seg)
    print(f"\n({batch}, {heads}, {L}) p = {p}")
    o, dq, dk, dv = r.check(_drop(p))
    for other in (_drop(p, site=4), _drop(p, seed=20261)):
        o2 = r.fwd(other)[0]
        dq2, dk2, dv2 = r.bwd(other)[:3]
        assert not torch.equal(o, o2) and not torch.equal(dq, dq2) and not torch.equal(dk, dk2) and not torch.equal(dv, dv2)


# ------------------------------------------------------------------------------------------------ 3. drop_p = 0: lr2_self_attn_fwd_bf16's bytes
@pytest.mark.parametrize("batch,heads,L", [(2, 2, 17), (2, 2, 129), (2, 2, 288), (256, 1, 33)])
def test_no_dropout_is_the_inference_kernels_bytes(dev, batch, heads, L):
    """The three bf16 modes share one attention arithmetic: without dropout the context plane is byte-equal to
    ops.self_attn_fwd_bf16(..., out_plane=) -- the one-pair kernel, and the persistent one at (256, 1, 33)."""
    from lr2ppo_amd import ops
    seg = AC.masks(batch, L, 288)["hole"]
    c = AC.exact_qkv(batch, heads, L, seed=800 + L, logit_span=20, scale=SCALE)
    r = Run(dev, c, seg)
    ref = torch.full((r.n * r.E,), NAN16, dtype=torch.int16, device=dev)
    ops.self_attn_fwd_bf16(r.qkv, r.seg, out_plane=ref, **r.kw)
    for with_lse in (True, False):
        got = r.fwd(None, with_lse=with_lse)[2]
        assert torch.equal(got, ref), f"{int((got != ref).sum())} of {ref.numel()} elements differ"


# ------------------------------------------------------------------------------------------------ 4. a sequence with no valid key
@pytest.mark.parametrize("L", [33, 200, 257])
def test_all_padding_sequence(dev, L):
    """Mask none_valid: every key of the last sequence carries -10000.  Everything stays finite; V = 1 gives O = 1 within 2^-8 + L 2^-23
    (the half-ulp of the rounded P~ against the unrounded row sum; the plane holds 1 exactly); the other sequence meets the gates of
    test_edges_of_every_instantiation; the padded sequence's gradients are held to relative L2 against fp64 (softmax(s - 10000) in
    fp32 rounds the scores at 10^4: a rounding pattern, hence a measured gate with a margin of 4)."""
    batch, heads = SMALL
    seg = AC.masks(batch, L, 288)["none_valid"]
    assert not bool((seg[-1] > 0).any()) and bool((seg[0] > 0).all())
    c = AC.exact_qkv(batch, heads, L, seed=900 + L, logit_span=20, scale=SCALE)
    print(f"\n({batch}, {heads}, {L}) none_valid")
    ones = dict(c, v=torch.ones_like(c["v"]))
    o1 = Run(dev, ones, seg).fwd(None)[0]
    err = float((o1.double() - 1.0).abs().max())
    print(f"    V = 1: max |O - 1| = {err:.3e} (gate {H8 + L * 2.0 ** -23:.3e})")
    assert err <= H8 + L * 2.0 ** -23
    r = Run(dev, c, seg)
    worst = 0.0
    for drop in (None, _drop(0.1)):
        o, dq, dk, dv = r.check(drop, seqs=slice(0, batch - 1), what="[valid sequences] ")
        _, _, dq_ref, dk_ref, dv_ref = AC.reference(r.q[-1:], r.k[-1:], r.v[-1:], seg[-1:], SCALE,
                                                    keep=r.keep(drop)[-1:] if drop is not None else None,
                                                    p=drop.p if drop is not None else 0.0, do=r.g[-1:])
        rels = {n: float((got[-1:].double() - ref).norm() / ref.norm())
                for n, got, ref in (("dQ", dq, dq_ref), ("dK", dk, dk_ref), ("dV", dv, dv_ref))}
        print(f"    PADBWD L {L} p {drop.p if drop is not None else 0.0}: " + ", ".join(f"{n} {v:.3e}" for n, v in rels.items()))
        worst = max(worst, max(rels.values()))
    assert _PAD_BWD_MEASURED is not None and worst <= 4 * _PAD_BWD_MEASURED, worst


# ------------------------------------------------------------------------------------------------ 5. every element written, nothing else
@pytest.mark.parametrize("L", [33, 200, 257])
def test_every_element_written_nothing_else_touched(dev, L):
    """o, the three column blocks of a [M, 3E] dQKV plane, lse, lse_ws and dsum_ws start as NaN patterns with one canary row group behind
    each (Run): after the calls every element in range is finite and every canary untouched, at lengths that are no multiple of 16."""
    batch, heads = SMALL
    seg = AC.masks(batch, L, 288)["alternate"]
    c = AC.exact_qkv(batch, heads, L, seed=1000 + L, logit_span=2, scale=SCALE)
    r = Run(dev, c, seg)
    for drop in (None, _drop(0.1)):
        o_plane = r.fwd(drop)[2]
        d_plane = r.bwd(drop)[4]
        assert not bool((o_plane == NAN16).any()) and not bool((d_plane == NAN16).any())
        for j in range(3):          # dQ | dK | dV: each block of the plane carries values (no block left at a constant)
            blk = d_plane.view(r.n, 3 * r.E)[:, j * r.E:(j + 1) * r.E]
            assert int(blk.unique().numel()) > 16, ("dq", "dk", "dv")[j]


# ------------------------------------------------------------------------------------------------ 6. random operands, 7. determinism
def test_random_normal_operands_and_determinism(dev):
    """The ViT-B/16 layer's shape at two sequences: normal operands rounded to bf16 (the reference takes the planes' numbers), scale
    1 / 8, p = 0.1, the same gates; two backward (and two forward) calls on the same inputs give the same bytes."""
    batch, heads, L = 2, 2, 197
    gen = torch.Generator().manual_seed(77)
    c = {n: torch.randn(batch, heads, L, 64, generator=gen).to(torch.bfloat16).float() for n in ("q", "k", "v", "do")}
    seg = AC.masks(batch, L, 288)["suffix"]
    r = Run(dev, c, seg)
    drop = _drop(0.1)
    print(f"\n({batch}, {heads}, {L}) random normal, p = 0.1")
    r.check(drop)
    assert torch.equal(r.bwd(drop)[4], r.bwd(drop)[4])
    assert torch.equal(r.fwd(drop)[2], r.fwd(drop)[2])


# ------------------------------------------------------------------------------------------------ 9. the schedule against a torch emulation
class _B1Attention(torch.autograd.Function):
    """The attention core as csrc/selfattn_b1_train.hip computes it, in fp64 with the kernels' rounding sites: Q | K | V as one bf16 plane;
    P~ M -> bf16 in front of P V (the row sum from the unrounded P~); in the backward dO -> bf16 (the `do` plane), dS -> bf16 and
    Pd = P o M -> bf16.  (o and dQ | dK | dV are rounded by the products that read them: _BLinear.)"""

    @staticmethod
    def forward(ctx, qkv, mask, m, scale):
        T = _bf16_train_tests()
        q, k, v = T._r(qkv)
        s = q @ k.transpose(-2, -1) * scale + mask
        pt = torch.exp(s - s.max(dim=-1, keepdim=True).values)
        l = pt.sum(-1, keepdim=True)
        ctx.save_for_backward(q, k, v, pt / l, m)
        ctx.scale = scale
        return (T._r(pt * m) @ v) / l

    @staticmethod
    def backward(ctx, do):
        T = _bf16_train_tests()
        q, k, v, P, m = ctx.saved_tensors
        g = T._r(do)
        dP = (g @ v.transpose(-2, -1)) * m
        dS = T._r(P * (dP - (dP * P).sum(-1, keepdim=True)) * ctx.scale)
        return torch.stack([dS @ k, dS.transpose(-2, -1) @ q, T._r(P * m).transpose(-2, -1) @ g]), None, None, None


def _emulated_layer(T, P, emb, seg, pre, heads, eps, drop):
    """test_bf16_train_gpu._emulated_layer with the attention core replaced by _B1Attention: one encoder layer (+ the pre-LN stack's
    final LayerNorm) in fp64, products and LayerNorm exact on bf16-rounded operands, the dropout masks of the HIP kernels."""
    B, L, E = emb.shape
    M, hd = B * L, E // heads
    mask = (1.0 - (seg > 0).double().view(B, 1, 1, L)) * -10000.0
    t = "transformer.0"
    ln = lambda x, k: O.layernorm_tp(x, P[f"{t}.{k}.gamma"], P[f"{t}.{k}.beta"], eps)          # noqa: E731
    lin = lambda x, k: T._BLinear.apply(x, P[f"{t}.{k}.weight"], P[f"{t}.{k}.bias"])            # noqa: E731
    p = float(drop["p"])
    keep = O.attention_keep_mask(int(drop["seed"]), int(drop["site_base"]), B, heads, L, p)
    m = torch.as_tensor(np.asarray(keep, dtype=np.float64)) / (1.0 - p)

    def attention(x):
        w = torch.cat([P[f"{t}.self_attn.linear_layers.{j}.weight"] for j in range(3)], 0)
        b = torch.cat([P[f"{t}.self_attn.linear_layers.{j}.bias"] for j in range(3)], 0)
        qkv = T._BLinear.apply(x, w, b).view(B, L, 3, heads, hd).permute(2, 0, 3, 1, 4)
        o = _B1Attention.apply(qkv, mask, m, 1.0 / hd ** 0.5).transpose(1, 2).reshape(M, E)
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
EMULATION_WORST = (1.37e-3, 1.52e-3)


@pytest.mark.parametrize("pre", [True, False], ids=["pre_ln", "post_ln"])
def test_schedule_against_a_torch_emulation(dev, pre):
    """Plumbing: shape and method of test_bf16_train_gpu.test_schedule_against_a_torch_emulation with bf16_attention on and the new
    rounding sites emulated too.  A transposed operand or a wrong dropout site is O(1)."""
    from lr2ppo_amd import ops, runtime
    T = _bf16_train_tests()
    B, L = 2, 197 if pre else 196
    enc = T._small_encoder(pre, dev, 11, layers=1)
    g = torch.Generator().manual_seed(12)
    emb = torch.randn(B, L, 256, generator=g)
    seg = torch.ones(B, L, dtype=torch.int64)
    if not pre:
        seg[1, 120:] = 0
    dout = torch.randn(B, L, 256, generator=g) * 0.1
    enc.bf16_train = enc.bf16_attention = True
    runtime.set_dropout_seed(4321)
    c0 = ops.self_attn_bf16_train_launch_counts()
    out, saved = enc._forward_train(emb.to(dev), seg.to(dev))
    p, seed = saved["drop"]
    demb, G = enc._backward_train(saved, dout.to(dev))
    assert ops.self_attn_bf16_train_launch_counts() == (c0[0] + 1, c0[1] + 1)
    P = {n: q.detach().double().cpu().requires_grad_() for n, q in enc.named_parameters()}
    e64 = emb.double().requires_grad_()
    ln_eps = enc.transformer[0].layer_norm_1.eps
    ref = _emulated_layer(T, P, e64, seg, pre, 4, ln_eps, {"p": p, "seed": seed, "site_base": 0})
    (ref * dout.double()).sum().backward()
    rel = lambda a, b: float((a.double().cpu() - b).norm() / b.norm())          # noqa: E731
    errs = {"output": rel(out, ref.detach()), "d_emb": rel(demb, e64.grad)}
    for n, q in enc.named_parameters():
        if n.endswith("linear_layers.1.bias"):      # true gradient 0: against the query bias's gradient
            errs[n] = float((G[q].double().cpu() - P[n].grad).norm() / P[n.replace(".1.bias", ".0.bias")].grad.norm())
        else:
            errs[n] = rel(G[q], P[n].grad)
    print(f"\n[bf16_attention vs torch emulation, {'pre' if pre else 'post'}-LN] EMUL {0 if pre else 1} worst {max(errs.values()):.3e}")
    for n, r in errs.items():
        print(f"  {n:50s} rel L2 {r:.4e}")
    gate = EMULATION_WORST[0 if pre else 1]
    assert gate is not None and max(errs.values()) <= 3 * gate, max(errs.values())


# ------------------------------------------------------------------------------------------------ 10. against the parity path
# relative L2 distance of bf16_train with bf16_attention from split_bf16, measured on one MI355X with test_bf16_train_gpu's two-layer
# towers and inputs (pre-LN, post-LN), the dispatch as shipped: the gates are 1.5 x these, floored at 1e-3.  The key bias's true gradient
# is 0: measured against the query bias's gradient.  (The same columns with the 3-pass attention: test_bf16_train_gpu.MEASURED.)
MEASURED = {
    "output": (0.0029, 0.0032),
    "d_emb": (0.0034, 0.0038),
    "transformer.0.self_attn.linear_layers.0.weight": (0.0067, 0.0071),
    "transformer.0.self_attn.linear_layers.0.bias": (0.0070, 0.0073),
    "transformer.0.self_attn.linear_layers.1.weight": (0.0067, 0.0072),
    "transformer.0.self_attn.linear_layers.1.bias": (0.0019, 0.0021),
    "transformer.0.self_attn.linear_layers.2.weight": (0.0056, 0.0061),
    "transformer.0.self_attn.linear_layers.2.bias": (0.0042, 0.0047),
    "transformer.0.self_attn.final_linear.weight": (0.0050, 0.0059),
    "transformer.0.self_attn.final_linear.bias": (0.0035, 0.0044),
    "transformer.0.feed_forward.linear_1.weight": (0.0044, 0.0047),
    "transformer.0.feed_forward.linear_1.bias": (0.0041, 0.0044),
    "transformer.0.feed_forward.linear_2.weight": (0.0041, 0.0044),
    "transformer.0.feed_forward.linear_2.bias": (0.0032, 0.0035),
    "transformer.0.layer_norm_1.gamma": (0.0064, 0.0038),
    "transformer.0.layer_norm_1.beta": (0.0042, 0.0041),
    "transformer.0.layer_norm_2.gamma": (0.0047, 0.0034),
    "transformer.0.layer_norm_2.beta": (0.0041, 0.0033),
    "transformer.1.self_attn.linear_layers.0.weight": (0.0072, 0.0076),
    "transformer.1.self_attn.linear_layers.0.bias": (0.0061, 0.0068),
    "transformer.1.self_attn.linear_layers.1.weight": (0.0071, 0.0076),
    "transformer.1.self_attn.linear_layers.1.bias": (0.0018, 0.0020),
    "transformer.1.self_attn.linear_layers.2.weight": (0.0043, 0.0046),
    "transformer.1.self_attn.linear_layers.2.bias": (0.0037, 0.0039),
    "transformer.1.self_attn.final_linear.weight": (0.0042, 0.0043),
    "transformer.1.self_attn.final_linear.bias": (0.0029, 0.0030),
    "transformer.1.feed_forward.linear_1.weight": (0.0046, 0.0046),
    "transformer.1.feed_forward.linear_1.bias": (0.0036, 0.0035),
    "transformer.1.feed_forward.linear_2.weight": (0.0041, 0.0042),
    "transformer.1.feed_forward.linear_2.bias": (0.0017, 0.0018),
    "transformer.1.layer_norm_1.gamma": (0.0042, 0.0033),
    "transformer.1.layer_norm_1.beta": (0.0038, 0.0027),
    "transformer.1.layer_norm_2.gamma": (0.0048, 0.0031),
    "transformer.1.layer_norm_2.beta": (0.0041, 0.0000),
    "layer_norm.gamma": (0.0029, None),
    "layer_norm.beta": (0.0000, None),
}


@pytest.mark.parametrize("pre", [True, False], ids=["pre_ln", "post_ln"])
def test_gradients_against_split_bf16(dev, pre):
    from lr2ppo_amd import ops
    T = _bf16_train_tests()
    B, L = (4, 197) if pre else (4, 196)
    col = 0 if pre else 1
    enc = T._small_encoder(pre, dev, 3)
    g = torch.Generator().manual_seed(4)
    emb = torch.randn(B, L, 256, generator=g).to(dev)
    seg = torch.ones(B, L, dtype=torch.int64)
    if not pre:
        seg[1, 150:] = 0
        seg[3, 40:] = 0
    seg = seg.to(dev)
    dout = torch.randn(B, L, 256, generator=g).to(dev) * 0.1
    ref_out, ref_demb, ref = T._grads(enc, False, emb, seg, dout)
    enc.bf16_attention = True
    c0 = ops.self_attn_bf16_train_launch_counts()
    out, demb, got = T._grads(enc, True, emb, seg, dout)
    assert ops.self_attn_bf16_train_launch_counts() == (c0[0] + 2, c0[1] + 2)
    rel = lambda a, b: float((a - b).norm() / b.norm().clamp_min(1e-30))            # noqa: E731
    res = {"output": rel(out, ref_out), "d_emb": rel(demb, ref_demb)}
    for n in ref:
        if n.endswith("linear_layers.1.bias"):
            res[n] = float((got[n] - ref[n]).norm() / ref[n.replace(".1.bias", ".0.bias")].norm())
        else:
            res[n] = rel(got[n], ref[n])
    print(f"\n[bf16_train + bf16_attention vs split_bf16, {'pre' if pre else 'post'}-LN]")
    for n, r in res.items():
        three_pass = T.MEASURED[n][col]
        ratio = f"{r / three_pass:.2f} x" if three_pass else "-"
        print(f"  B1ATT {col} {n} {r:.6f}   (3-pass attention: {three_pass}, ratio {ratio})")          # reported, not gated
    bad = [n for n, r in res.items() if n not in MEASURED or MEASURED[n][col] is None or not r <= T._gate(MEASURED[n][col])]
    assert not bad, bad
    for n in ref:
        if n.endswith("weight"):
            assert float(torch.nn.functional.cosine_similarity(got[n].flatten(), ref[n].flatten(), dim=0)) > 0.999, n


# ------------------------------------------------------------------------------------------------ 11. same bits where the mode promises them
def _tower_case(dev, pre, L=None):
    T = _bf16_train_tests()
    B = 4
    L = L or (197 if pre else 196)
    enc = T._small_encoder(pre, dev, 3)
    g = torch.Generator().manual_seed(5)
    emb = torch.randn(B, L, 256, generator=g).to(dev)
    seg = torch.ones(B, L, dtype=torch.int64)
    if not pre:
        seg[1, L // 2:] = 0
    dout = torch.randn(B, L, 256, generator=g).to(dev) * 0.1
    enc.bf16_train = True
    return T, enc, emb, seg.to(dev), dout


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(a[2][n], b[2][n]) for n in a[2])


@pytest.mark.parametrize("pre", [True, False], ids=["pre_ln", "post_ln"])
def test_same_bits_and_launch_counts(dev, pre):
    from lr2ppo_amd import ops, runtime
    T, enc, emb, seg, dout = _tower_case(dev, pre)
    layers = enc.layers_num
    counts = ops.self_attn_bf16_train_launch_counts
    # flag off: neither entry point is called
    c0 = counts()
    off = T._grads(enc, True, emb, seg, dout)
    assert counts() == c0
    # flag on: once per layer forward, once per layer backward
    enc.bf16_attention = True
    plain = T._grads(enc, True, emb, seg, dout)
    assert counts() == (c0[0] + layers, c0[1] + layers)
    assert not torch.equal(plain[0], off[0])
    # recompute=True: the same output and gradients (one more forward per layer)
    enc.recompute = True
    c1 = counts()
    rc = T._grads(enc, True, emb, seg, dout)
    assert counts() == (c1[0] + 2 * layers, c1[1] + layers)
    assert _same(plain, rc)
    enc.recompute = False
    # eval mode: a save=False forward (extract(), eval, the rollout) = the saving forward, through the same kernels
    enc.eval()
    runtime.set_dropout_seed(99)
    c2 = counts()
    kept = enc._forward_train_bf16(emb, seg, save=True)[0].clone()
    free, none = enc._forward_train_bf16(emb, seg, save=False)
    assert none is None and torch.equal(kept, free)
    with torch.no_grad():
        assert torch.equal(enc(emb, seg), kept)
    assert counts() == (c2[0] + 3 * layers, c2[1])


def test_long_sequences_keep_the_three_pass_branch(dev):
    """L = 300 > 288 with the flag on: the old branch -- no call of the new entry points, the bytes of the flag being off."""
    from lr2ppo_amd import ops
    T, enc, emb, seg, dout = _tower_case(dev, True, L=300)
    off = T._grads(enc, True, emb, seg, dout)
    enc.bf16_attention = True
    c0 = ops.self_attn_bf16_train_launch_counts()
    on = T._grads(enc, True, emb, seg, dout)
    assert ops.self_attn_bf16_train_launch_counts() == c0
    assert _same(off, on)


# ------------------------------------------------------------------------------------------------ 12. interface
def test_interface(dev):
    from lr2ppo_amd import ops
    from lr2ppo_amd.finetune import ppo
    from lr2ppo_amd.finetune.features import build_encoder_optimizer, finetune_pointwise_step
    T = _bf16_train_tests()
    for prec in ("split_bf16", "mxfp8_train"):
        with pytest.raises(ValueError):
            T._fx(dev, prec, bf16_attention=True)
    fx = T._fx(dev, "bf16_train", bf16_attention=True)
    assert fx.image.encoder.bf16_attention and fx.text.encoder.bf16_attention
    frames, ids, seg, tgts = T._batch(dev)
    args = argparse.Namespace(mode="reg", labels_num=3, seq_length=196, max_imgs=4, visual_feat_dim=768, is_master=True,
                              kl_div_loss_weight=0.001, entropy_weight=0.001, value_clip=0.5, optimizer="adamw", scheduler="linear",
                              learning_rate=1e-3, critic_learning_rate=1e-3, train_steps=41, warmup=0.1, device=dev)
    model = ppo.ActorCritic(args, None)
    ppo._init_normal(model.critic)
    model = model.to(dev)
    opt, copt, sch, csch = ppo.build_optimizer(args, model)
    eopt, esch = build_encoder_optimizer(args, fx)
    sch.step(), csch.step(), esch.step()
    before = {n: p.detach().clone() for n, p in fx.named_parameters()}
    c0 = ops.self_attn_bf16_train_launch_counts()
    loss = finetune_pointwise_step(args, fx, model.actor, opt, sch, eopt, esch, frames, ids, seg, tgts)
    c1 = ops.self_attn_bf16_train_launch_counts()
    assert torch.isfinite(loss)
    assert c1[0] >= c0[0] + 2 and c1[1] == c0[1] + 2                 # one layer per tower: two forwards (at least), two backwards
    moved = {n for n, p in fx.named_parameters() if not torch.equal(before[n], p.detach())}
    stuck = [n for n in before if ".encoder." in n and n not in moved]
    assert not stuck, stuck
