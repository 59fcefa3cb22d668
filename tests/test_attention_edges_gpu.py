"""Self-attention kernels (csrc/selfattn_fwd.hip, csrc/selfattn_bwd.hip, csrc/selfattn_mx.hip) on inputs whose scores are exact, at the edges of the softmax, of the
key mask and of the length dispatch.  Case builders and the fp64 reference: tests/attn_cases.py (checked by test_attention_edges_cpu.py).

Which form a call runs ("Self-attention: which length runs which kernel"; `persistent` = batch * heads >= the CU count):

    forward  (lr2_self_attn_fwd)       L <= 64 / <= 128 / <= 224   one key block in LDS, 4 / 8 / 14 key tiles   (F4 / F8 / F14)
                                       the same, persistent         self_attn_persist_kernel             (FP4 / FP8 / FP14)
                                       L > 224                      key blocks of 160 / 192 / 224 keys          (FB; 3 slots: L <= 384
                                                                                                                 or 224-key blocks, else 4)
    backward (lr2_self_attn_bwd)       L <= 64 / 128 / 224 / 256    recomputing, one block, 4 / 8 / 14 / 16 tiles (R4 / R8 / R14 / R16)
                                       L > 256                      recomputing, 128-row blocks                  (RB)
                                       o given, persistent, L<=224  streaming                              (S4 / S8 / S14)
    lr2_first_token_attn               any L <= 4096                                                             (FT)
    lr2_self_attn_fwd_bf16             L <= 64 / 128 / 224 / 288    one pair (B4 / B8 / B14 / B18), persistent   (BP)

Gates.  Taken from the existing tests of these kernels (test_kernels_gpu.py): O 2e-5 + 2e-5 |ref|; lse 1e-5 + 1e-5 |ref|; gradients
3e-5 max(1, max|ref|) + 5e-5 |ref|.  Derived: dropout multiplies them by 1 / (1 - p) (the kept terms are scaled by it); the bf16 kernel
rounds P to ONE bf16 plane, 2^-9 relative per probability, so its O gate is 2^-9 max|V| + the fp32 gate; "exact" comparisons are
torch.equal, relaxed only where a comment names the rounding operation.  Measured (everything not taken or derived above):

    gate                                                     measured vs fp64 (max)      margin   gate      measured
    all-padding sequence, recomputing backward, rel. L2      3.18e-4 (24 gradients)      4 x      1.27e-3   2026-10-18, MI355X
    all-padding sequence, streaming backward, rel. L2        4.51e-4 (6 gradients)       4 x      1.80e-3   2026-10-18, MI355X
    streaming backward, dQ, logit span 100 (peaked cases)    1.02 x the gradient gate    3 x      3.06 x    2026-10-18, MI355X
      (max err 9.59e-3 at max|ref| = 313: (256, 1, 129), maximum planted on a masked key, mask alternate; the recomputing dQ of the
       same case: 0.09 x.  The term that grows: the streaming kernels rebuild P = 2^(fma(s, scale log2 e, mask - lse log2 e)) from the
       forward's fp32 lse; lse and lse * log2 e each round at |lse| ~ 450 -- about 2^-24 |lse| (1 + 2 log2 e) ln 2 = 4e-5 relative on a
       whole row of P, hence of dS and dQ, where the gate allows 3e-5 of max|ref|.  Spans 2 and 20, dK and dV keep the plain gate.)

(all-padding: the maximum over dQ, dK, dV of every case of test_all_padding_sequence.  Every other check of this file measured at most
0.88 x its gate in the same runs, so no other gate needed a measured value.)

All-padding derivation: upstream evaluates softmax(s - 10000) in fp32, i.e. on scores rounded to the fp32 grid at 10^4 (2^-10): a score
moves by <= 2^-11 in either log domain, a probability by <= 2 * 2^-11 relative after normalisation, and a further factor 2 covers the
maximum and the sum both moving: |O - softmax(s) V| <= 2 * 2^-10 max|V| (the reference alone meets it: test_attention_edges_cpu.py).
The gradients of such a sequence inherit a rounding PATTERN that changes with the seed, hence a measured gate with a margin of 4."""
import math

import pytest
import torch

import attn_cases as AC
from oracle import lr2ppo_oracle as O

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
NAN16 = 0x7FC0
# relative L2 against fp64 of (dQ, dK, dV) of the all-padding sequence: the measured maximum over the cases of test_all_padding_sequence
# (table above); the gate is 4 x
_PAD_BWD_MEASURED = {"recomputing": 3.18e-4, "streaming": 4.51e-4}
_STREAM_DQ_SPAN100 = 3 * 1.02


fwd_block, bwd_block = AC.fwd_block, AC.bwd_block          # the dispatch, restated from the kernels' launch code (attn_cases.py)


def _o_gate(ref, k=1.0):
    return k * (2e-5 + 2e-5 * ref.abs())


def _lse_gate(ref):
    return 1e-5 + 1e-5 * ref.abs()


def _g_gate(ref, k=1.0):
    return k * (3e-5 * max(1.0, float(ref.abs().max())) + 5e-5 * ref.abs())


def _check(what, got, ref, bound):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert torch.isfinite(got).all(), f"{what}: not finite"
    err = (got - ref).abs()
    bound = bound if torch.is_tensor(bound) else torch.full_like(err, float(bound))
    worst = float((err / bound.clamp(min=1e-300)).max()) if err.numel() else 0.0
    print(f"    {what}: max err {float(err.max()) if err.numel() else 0.0:.3e}, worst err / gate {worst:.3f}")
    assert bool((err <= bound).all()), f"{what}: max err {float(err.max()):.3e}, {worst:.2f} x the gate, {int((err > bound).sum())} bad"


class Run:
    """One problem on the device: the planes, and every kernel entry point on them."""

    def __init__(self, dev, c, seg, scale):
        from lr2ppo_amd import ops
        self.ops, self.dev, self.scale = ops, dev, scale
        self.B, self.H, self.L, _ = c["q"].shape
        self.E = self.H * 64
        self.n = self.B * self.L
        self.seg_cpu = seg
        self.seg = seg.reshape(-1).to(dev)
        self.qkv = ops.split_planes(AC.pack(c["q"], c["k"], c["v"]).to(dev), ops.Planes.empty(self.n, 3 * self.E, dev))
        self.do = ops.split_planes(AC.pack(c["do"]).to(dev), ops.Planes.empty(self.n, self.E, dev))
        # the very numbers the planes hold
        self.q, self.k, self.v = (t.contiguous() for t in AC.unpack(self.qkv.to_float().cpu(), self.B, self.H, self.L))
        (self.g,) = (t.contiguous() for t in AC.unpack(self.do.to_float().cpu(), self.B, self.H, self.L))
        self.kw = dict(batch=self.B, heads=self.H, L=self.L, head_dim=64, scale=scale)
        self.extra = []                                                     # (name, canary view, expected bits)

    # -- allocation with one canary row group (E columns' worth) behind every output --
    def _f32(self, rows, cols, name):
        buf = torch.full((rows * cols + self.E,), float("nan"), device=self.dev)
        self.extra.append((name, buf[rows * cols:].view(torch.int32), None))
        return buf[:rows * cols].view(rows, cols) if cols > 1 else buf[:rows]

    def _planes(self, rows, cols, name):
        pad = self.E
        buf = torch.full((2 * (rows * cols + pad),), NAN16, dtype=torch.int16, device=self.dev)
        pl = self.ops.Planes(buf, rows, cols, lo_off=rows * cols + pad)
        self.extra.append((name + " hi", buf[rows * cols:rows * cols + pad], None))
        self.extra.append((name + " lo", buf[2 * rows * cols + pad:], None))
        return pl

    def check_canaries(self):
        for name, view, _ in self.extra:
            if view.dtype == torch.int16:
                assert bool((view == NAN16).all()), f"{name}: written behind the last row"
            else:
                assert bool((view == torch.full((1,), float("nan")).view(torch.int32).item()).all()), f"{name}: written behind the last row"

    def unheads(self, x):
        return AC.unpack(x.detach().float().cpu(), self.B, self.H, self.L)

    def fwd(self, drop=None):
        """(O [B, H, L, 64], lse [B, H, L], output planes) of lr2_self_attn_fwd: the fp32 output, and the planes output of a second call."""
        o, lse = self._f32(self.n, self.E, "o"), self._f32(self.B * self.H * self.L, 1, "lse")
        self.ops.self_attn_fwd(self.qkv, self.seg, o, lse=lse, drop=drop, **self.kw)
        op = self._planes(self.n, self.E, "o planes")
        self.ops.self_attn_fwd(self.qkv, self.seg, op, drop=drop, **self.kw)
        ref_pl = self.ops.split_planes(o.contiguous(), self.ops.Planes.empty(self.n, self.E, self.dev))
        m = self.n * self.E
        # KNOWN TO FAIL NOW AND THEN on the persistent forward (batch * heads >= the CU count): in one run of three on an MI355X two of ~130
        # such call pairs -- (256, 1, 100) and (256, 1, 224) -- gave different bits while every comparison with fp64 passed; the same
        # inputs gave equal bits in the other runs.  Two launches of self_attn_persist_kernel on the same inputs do not always agree: cause
        # not found.
        bad = int((op.buf[:m] != ref_pl.buf[:m]).sum()) + int((op.buf[op.lo_off:op.lo_off + m] != ref_pl.buf[m:]).sum())
        assert bad == 0, f"planes output != split(fp32 output): {bad} of {2 * m} plane elements differ between the two launches"
        self.o_planes, self.lse_dev = op, lse
        return self.unheads(o)[0], lse.view(self.B, self.H, self.L).cpu(), op

    def bwd(self, drop=None, streaming=False):
        """(dQ, dK, dV, lse workspace) of lr2_self_attn_bwd; streaming: given the forward's output planes and log-sum-exp (fwd() first)."""
        d = self._planes(self.n, 3 * self.E, "dqkv")
        ws1, ws2 = (self._f32(self.B * self.H * self.L, 1, n) for n in ("lse_ws", "dsum_ws"))
        if streaming:
            assert self.ops.self_attn_plan(self.B, self.H, self.L)[1]
            ws1.copy_(self.lse_dev)
            self.ops.self_attn_bwd(self.qkv, self.do, self.seg, d, ws1, ws2, drop=drop, o=self.o_planes, **self.kw)
            assert torch.equal(ws1, self.lse_dev)
        else:
            self.ops.self_attn_bwd(self.qkv, self.do, self.seg, d, ws1, ws2, drop=drop, **self.kw)
        got = d.to_float()
        assert torch.isfinite(got).all() and torch.isfinite(ws2).all()
        dq, dk, dv = self.unheads(got)
        return dq, dk, dv, ws1.view(self.B, self.H, self.L).cpu()

    def first_token(self):
        q0 = AC.pack(self.q[:, :, :1]).to(self.dev)                          # [B, E]: query row 0 of every sequence
        kv = self.ops.split_planes(AC.pack(self.k, self.v).to(self.dev), self.ops.Planes.empty(self.n, 2 * self.E, self.dev))
        buf = torch.full((self.B * self.E + self.E,), float("nan"), device=self.dev)
        self.extra.append(("first-token o", buf[self.B * self.E:].view(torch.int32), None))
        o = buf[:self.B * self.E].view(self.B, self.E)
        kw = dict(self.kw)
        self.ops.first_token_attn(q0, kv, self.seg, o, **kw)
        return o.cpu().view(self.B, self.H, 1, 64)

    def bf16(self):
        x = AC.pack(self.q, self.k, self.v).to(self.dev).to(torch.bfloat16).contiguous()
        assert torch.equal(x.float().cpu(), AC.pack(self.q, self.k, self.v)), "the bf16 kernel needs bf16-valued inputs"
        o = self._f32(self.n, self.E, "bf16 o")
        self.ops.self_attn_fwd_bf16(x, self.seg, out=o, **self.kw)
        return self.unheads(o)[0]

    def reference(self, keep=None, p=0.0, grads=True, seqs=None):
        """fp64 reference on the numbers the planes hold; seqs: of these sequences only (a large batch: the checks then compare them)."""
        q, k, v, g, seg = self.q, self.k, self.v, self.g, self.seg_cpu
        if seqs is not None:
            q, k, v, g, seg = (t[seqs] for t in (q, k, v, g, seg))
            keep = keep[seqs] if keep is not None else None
        return AC.reference(q, k, v, seg, self.scale, keep=keep, p=p, do=g if grads else None)


def _persistent(batch, heads, L):
    from lr2ppo_amd import ops
    return ops.self_attn_plan(batch, heads, L)


def _assert_form(batch, heads, L, persistent):
    f, b = _persistent(batch, heads, L)
    assert f == (persistent and L <= 224) and b == (persistent and L <= 224), (batch, heads, L, f, b)


SMALL = (2, 2)


# ------------------------------------------------------------------------------------------------ (a) one valid key: exact
# L -> forward form / backward form: 33 F4 / R4, 100 F8 / R8, 200 F14 / R14, 240 FB (160-key blocks) / R16,
# 257 FB (160, 3 slots) / RB, 449 FB (160, 4 slots) / RB, 514 FB (192, 4 slots) / RB
@pytest.mark.parametrize("L", [1, 33, 100, 200, 240, 257, 449, 514])
def test_one_valid_key_is_exact_one_pair_and_blocked_forms(dev, L):
    """Mask only_first: P is exactly one-hot (exp(-10000 + ...) = 0, exp(0) = 1, l = 1), so O[q] = V_hi[0] + V_lo[0] for a random fp32 V,
    lse[q] = s[q, 0], dQ = dK = 0, dV[k != 0] = 0 bit for bit and dV[0] = sum_q dO[q] to the fp32 summation order: every row / column /
    head index map of the forward, of first_token_attn and of the recomputing backward without a tolerance."""
    batch, heads = SMALL
    _assert_form(batch, heads, L, False)
    seg = AC.masks(batch, L, fwd_block(L))["only_first"]
    c = AC.exact_qkv(batch, heads, L, seed=100 + L, logit_span=20)
    _one_valid_key(dev, c, seg, streaming=False)


# FP / S with 4, 8 and 14 key tiles; one pair per CU and two heads per sequence
@pytest.mark.parametrize("batch,heads,L", [(256, 1, 50), (128, 2, 100), (256, 1, 200)])
def test_one_valid_key_is_exact_persistent_forms(dev, batch, heads, L):
    _assert_form(batch, heads, L, True)
    seg = AC.masks(batch, L, fwd_block(L))["only_first"]
    c = AC.exact_qkv(batch, heads, L, seed=200 + L, logit_span=2)
    _one_valid_key(dev, c, seg, streaming=True)


def _one_valid_key(dev, c, seg, streaming):
    batch, heads, L, _ = c["q"].shape
    s0 = (c["q"].double() @ c["k"].double().transpose(-1, -2))[..., 0] * 0.125       # exact in fp32 too
    one_block_fwd = L <= 224
    # forward on a random fp32 V: hi + lo of an fp32 number is exact in fp32
    cr = dict(c)
    cr["v"] = torch.randn(batch, heads, L, 64, generator=torch.Generator().manual_seed(L))
    r = Run(dev, cr, seg, 0.125)
    o, lse, _ = r.fwd()
    assert torch.equal(o, r.v[:, :, :1].expand_as(o)), "O != V[0]"
    ft = r.first_token()
    assert torch.equal(ft, r.v[:, :, :1]), "first_token_attn: O != V[0]"
    if one_block_fwd:
        # the one-block / persistent forward keeps the maximum in the log2 domain: lse = fl(fl(s * fl(scale * log2 e)) * ln 2) + log 1 rounds
        # twice (the fma and the multiplication by ln 2).  Two half-ulp roundings and the constants' errors can reach 1.14 x 2^-23 |s| in
        # general: 2^-23 |s| is NOT a general bound, it holds on these scores (multiples of 1/4 x scale: at most 0.73 x 2^-23 |s|, restated
        # in numpy by test_attention_edges_cpu.py::test_log2_domain_lse_of_one_valid_key_is_within_one_ulp_on_the_exact_scores)
        assert bool(((lse.double() - s0).abs() <= U * s0.abs()).all()), "lse != s[q, 0] (1 ulp)"
    else:
        assert torch.equal(lse.double(), s0), "lse != s[q, 0]"
    # backward on the exact V / dO: dP = dO V^T and D are exact, so dS = P (dP - D) vanishes bit for bit
    r = Run(dev, c, seg, 0.125)
    o, lse, _ = r.fwd()
    assert torch.equal(o, r.v[:, :, :1].expand_as(o))
    gsum, gabs = r.g.double().sum(dim=2), r.g.double().abs().sum(dim=2)
    for stream in ([False, True] if streaming else [False]):
        dq, dk, dv, lse_ws = r.bwd(streaming=stream)
        what = "streaming" if stream else "recomputing"
        assert not dq.any() and not dk.any(), f"{what}: dQ / dK != 0"
        assert not dv[:, :, 1:].any(), f"{what}: dV[k != 0] != 0"
        assert bool(((dv[:, :, 0].double() - gsum).abs() <= L * U * gabs).all()), f"{what}: dV[0] != sum_q dO[q]"
        if not stream:
            assert torch.equal(lse_ws.double(), s0), "recomputing backward: lse != s[q, 0]"     # natural-log domain: m + log 1


# B4 / B8 / B14 / B18 one pair, BP persistent (L = 288: two sub-tile rounds per wave)
@pytest.mark.parametrize("batch,heads,L", [(2, 2, 33), (2, 2, 100), (2, 2, 200), (2, 2, 287), (256, 1, 50), (128, 2, 287)])
def test_one_valid_key_is_exact_bf16_forward(dev, batch, heads, L):
    from lr2ppo_amd import ops
    assert ops.self_attn_bf16_plan(batch, heads, L) == (batch * heads >= 256)
    seg = AC.masks(batch, L, 288)["only_first"]
    c = AC.exact_qkv(batch, heads, L, seed=300 + L, logit_span=20)
    c["v"] = torch.randn(batch, heads, L, 64, generator=torch.Generator().manual_seed(L)).to(torch.bfloat16).float()
    r = Run(dev, c, seg, 0.125)
    o = r.bf16()
    assert torch.equal(o, c["v"][:, :, :1].expand_as(o)), "O != V[0]"


# ------------------------------------------------------------------------------------------------ (b) uniform softmax
@pytest.mark.parametrize("batch,heads,L,mask", [(2, 2, 33, "suffix"), (2, 2, 100, "alternate"), (2, 2, 200, "hole"), (2, 2, 240, "prefix_block"),
                                                (2, 2, 257, "alternate"), (2, 2, 449, "hole"), (2, 2, 514, "prefix_block"),
                                                (256, 1, 50, "alternate"), (128, 2, 200, "hole")])
def test_uniform_softmax_statistics(dev, batch, heads, L, mask):
    """Q = 0: P = 1 / n over the n valid keys: lse = log n to 1 ulp of logf (2 * 2^-23 log n), O = the mean of the valid V rows to
    L 2^-23 max|V|, dK = 0 bit for bit (dK = dS^T Q), dQ / dV against fp64 at the gates of the peaked cases."""
    persistent = batch * heads >= 256
    _assert_form(batch, heads, L, persistent)
    seg = AC.masks(batch, L, fwd_block(L))[mask]
    c = AC.exact_qkv(batch, heads, L, seed=400 + L, logit_span=0)
    r = Run(dev, c, seg, 0.125)
    o, lse, _ = r.fwd()
    n = (seg > 0).sum(dim=1).double().view(batch, 1, 1)
    assert bool(((lse.double() - n.log()).abs() <= 2 * U * n.log()).all()), "lse != log n"
    mean = ((seg > 0).double().view(batch, 1, L, 1) * r.v.double()).sum(dim=2, keepdim=True) / n.unsqueeze(-1)
    _check("O vs mean(V)", o, mean.expand_as(o), L * U * float(r.v.abs().max()))
    ft = r.first_token()
    _check("first_token O vs mean(V)", ft, mean, L * U * float(r.v.abs().max()))
    ref = r.reference()
    for stream in ([False, True] if persistent else [False]):
        dq, dk, dv, _ = r.bwd(streaming=stream)
        assert not dk.any(), "dK != 0"
        _check("dQ", dq, ref[2], _g_gate(ref[2]))
        _check("dV", dv, ref[4], _g_gate(ref[4]))


# ------------------------------------------------------------------------------------------------ (c) peaked softmax
# every dispatch edge; form reached (forward / recomputing backward):
#   1, 15, 16, 17, 64  F4 / R4       65, 128  F8 / R8       129, 224  F14 / R14       225, 256  FB 160-key blocks, 3 slots / R16
#   257  FB 160, 3 slots / RB        384  FB 192, 3 slots / RB        385  FB 224, 3 slots / RB        448  FB 224 (3 slots) / RB
#   449  FB 160, 4 slots / RB        512, 513  FB 192, 4 slots / RB   514  FB 192, 4 slots / RB
EDGE_L, SPANS, _peaked_cases = list(AC.EDGE_L), AC.SPANS, AC.peaked_cases


def _some_sequences(batch):
    """A large batch is compared with fp64 on its first, middle and last sequences (both parities: the mask patterns alternate)."""
    return sorted({0, 1, 2, 3, batch // 2 - 1, batch // 2, batch - 3, batch - 2, batch - 1}) if batch > 16 else None


def _peaked(dev, batch, heads, L, position, mask, span, block, scale=0.125, streaming=False, seed=0):
    seg = AC.masks(batch, L, block)[mask]
    key = AC.plant_key(position, L, block, seg)
    c = AC.exact_qkv(batch, heads, L, seed=500 + L + seed, logit_span=span, scale=scale, plant=key)
    print(f"  L {L} plant {position} (key {key}) mask {mask} span {span} block {block} scale {scale}")
    r = Run(dev, c, seg, scale)
    seqs = _some_sequences(batch)
    sl = (lambda t: t[seqs]) if seqs is not None else (lambda t: t)
    ref_o, ref_lse, ref_dq, ref_dk, ref_dv = r.reference(seqs=seqs)
    o, lse, op = r.fwd()
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    _check("O", sl(o), ref_o, _o_gate(ref_o))
    _check("lse", sl(lse), ref_lse, _lse_gate(ref_lse))
    ft = r.first_token()
    _check("first_token O", sl(ft), ref_o[:, :, :1], _o_gate(ref_o[:, :, :1]))
    for stream in ([False, True] if streaming else [False]):
        dq, dk, dv, lse_ws = r.bwd(streaming=stream)
        tag = "streaming " if stream else ""
        # streaming dQ at span 100: 3 x the measured 1.02 x (module docstring: the fp32 rounding of lse and lse * log2 e grows with |lse|)
        _check(tag + "dQ", sl(dq), ref_dq, _g_gate(ref_dq, _STREAM_DQ_SPAN100 if stream and span == 100 else 1.0))
        _check(tag + "dK", sl(dk), ref_dk, _g_gate(ref_dk))
        _check(tag + "dV", sl(dv), ref_dv, _g_gate(ref_dv))
        if not stream:
            _check("lse (backward)", sl(lse_ws), ref_lse, _lse_gate(ref_lse))
    return r, c, seg, o, lse, op


@pytest.mark.parametrize("i,L", list(enumerate(EDGE_L)))
def test_peaked_softmax_on_exact_scores_at_every_dispatch_edge(dev, i, L):
    """Exact scores with a planted row maximum (key 0, the last key of a ragged tile, the first key of the second block, a masked key that
    must still lose), logits spanning 2 / 20 / 100, every mask pattern: O, lse, dQ, dK, dV against fp64 at the existing gates -- what is
    left of the error (exp, the fp32 sums, the split of P, the P V and dS K products) does not grow with the logits."""
    batch, heads = SMALL
    _assert_form(batch, heads, L, False)
    for position, mask, span, block in _peaked_cases(i, L, 16):            # all 16 (position, mask) pairs at every length
        _peaked(dev, batch, heads, L, position, mask, span, block)


# persistent forms: 16, 33, 64 -> FP4 / S4; 65, 128 -> FP8 / S8; 129, 224 -> FP14 / S14 (and the recomputing backward at that batch).
# 8 pairs per length, the other 8 at the next one: each of the three tile counts sees all 16 (test_attention_edges_cpu.py checks it)
@pytest.mark.parametrize("i,L", list(enumerate(AC.PERSIST_L)))
def test_peaked_softmax_persistent_forms_equal_the_one_pair_kernels(dev, i, L):
    """The persistent forward and the streaming backward on the peaked cases, against fp64; and the first sequences alone (fewer pairs than
    CUs: the one-pair kernel) give the same O, lse and output planes BIT FOR BIT."""
    batch, heads = AC.PERSIST_SHAPES[i % 2]
    _assert_form(batch, heads, L, True)
    for position, mask, span, block in _peaked_cases(i, L, 8):
        r, c, seg, o, lse, op = _peaked(dev, batch, heads, L, position, mask, span, block, streaming=True, seed=7)
        nb = 4
        _assert_form(nb, heads, L, False)
        r2 = Run(dev, {n: t[:nb].contiguous() for n, t in c.items()}, seg[:nb].contiguous(), 0.125)
        o2, lse2, op2 = r2.fwd()
        assert torch.equal(o[:nb], o2) and torch.equal(lse[:nb], lse2), "persistent != one-pair forward"
        assert torch.equal(op.to_float()[:nb * L], op2.to_float()), "persistent != one-pair forward (planes)"


@pytest.mark.parametrize("i", range(len(AC.BF16_SHAPES)))
def test_peaked_softmax_bf16_forward(dev, i):
    """lr2_self_attn_fwd_bf16 on the same cases: P is rounded to one bf16 plane (2^-9 relative per probability; the row sum uses the
    unrounded values), so |O - ref| <= 2^-9 max|V| + the fp32 gate.  One pair: B4 / B8 / B14 / B18, all 16 pairs each; persistent (BP):
    8 pairs at each of its two shapes."""
    from lr2ppo_amd import ops
    batch, heads, L = AC.BF16_SHAPES[i]
    persistent = batch * heads >= 256
    assert ops.self_attn_bf16_plan(batch, heads, L) == persistent
    for position, mask, span, block in _peaked_cases(i, L, 8 if persistent else 16):
        block = block if block < L else 16 * 18                             # one block of up to 18 key tiles: the tile-wide patterns
        seg = AC.masks(batch, L, block)[mask]
        c = AC.exact_qkv(batch, heads, L, seed=600 + L, logit_span=span, plant=AC.plant_key(position, L, block, seg))
        r = Run(dev, c, seg, 0.125)
        seqs = _some_sequences(batch)
        ref_o, _ = r.reference(grads=False, seqs=seqs)
        o = r.bf16()
        assert torch.isfinite(o).all()
        _check(f"bf16 O (L {L}, {position}, {mask}, span {span})", o[seqs] if seqs is not None else o, ref_o,
               _o_gate(ref_o) + 2.0 ** -9 * float(r.v.abs().max()))


# ------------------------------------------------------------------------------------------------ (d) other scales
# one L per form: 33 F4 / R4, 100 F8 / R8, 200 F14 / R14, 240 FB / R16, 300 FB 160 / RB, 449 FB 4 slots / RB; persistent 100 (FP / S)
@pytest.mark.parametrize("scale", [1.0, 0.25, 2.0 ** -5])
def test_peaked_softmax_at_other_power_of_two_scales(dev, scale):
    for i, L in enumerate([33, 100, 200, 240, 300, 449]):
        position, mask, _, block = _peaked_cases(i, L, 16)[5 * i % 16]
        _peaked(dev, 2, 2, L, position, mask, 20, block, scale=scale)
    _peaked(dev, 256, 1, 100, "block2", "hole", 20, fwd_block(100), scale=scale, streaming=True)


@pytest.mark.parametrize("batch,heads,L", [(2, 2, 200), (2, 2, 300), (256, 1, 100)])
def test_random_inputs_at_scale_one_over_sqrt_32(dev, batch, heads, L):
    """Random Q, K, V, dO (non-zero lo planes everywhere) and a scale that is no power of two (the persistent kernels fold it into
    scale * log2 e): forward O and lse at the random-input gates plus the propagated score error 2.5 delta_q max|V|, delta_q = 2^-15
    scale max_k sum_d |q_d| |k_d| (2^-15 bounds the dropped lo x lo term, the two lo-plane roundings and 64 fp32 accumulations); dQ, dK,
    dV of the recomputing backward -- and at (256, 1, 100) of the streaming one, fma(a, scale * log2 e, mask - lse * log2 e) -- at the
    existing random-input gradient gate (test_self_attn_bwd_matches_autograd), unchanged."""
    scale = 1.0 / math.sqrt(32.0)
    g = torch.Generator().manual_seed(L)
    c = {n: torch.randn(batch, heads, L, 64, generator=g) * (0.7 if n in "qk" else 1.0) for n in ("q", "k", "v", "do")}
    seg = AC.masks(batch, L, fwd_block(L))["alternate"]
    r = Run(dev, c, seg, scale)
    ref_o, ref_lse = r.reference(grads=False)
    delta = 2.0 ** -15 * scale * (r.q.double().abs() @ r.k.double().abs().transpose(-1, -2)).max(dim=-1).values      # [B, H, L]
    o, lse, _ = r.fwd()
    _check("O", o, ref_o, _o_gate(ref_o) + 2.5 * delta.unsqueeze(-1) * float(r.v.abs().max()))
    _check("lse", lse, ref_lse, _lse_gate(ref_lse) + delta)
    _, _, ref_dq, ref_dk, ref_dv = r.reference()
    persistent = batch * heads >= 256
    _assert_form(batch, heads, L, persistent)
    for stream in ([False, True] if persistent else [False]):
        dq, dk, dv, lse_ws = r.bwd(streaming=stream)
        tag = "streaming " if stream else ""
        _check(tag + "dQ", dq, ref_dq, _g_gate(ref_dq))
        _check(tag + "dK", dk, ref_dk, _g_gate(ref_dk))
        _check(tag + "dV", dv, ref_dv, _g_gate(ref_dv))
        if not stream:
            _check("lse (backward)", lse_ws, ref_lse, _lse_gate(ref_lse) + delta)


# ------------------------------------------------------------------------------------------------ (e) dropout at the ends of its range
# 33 F4 / R4, 100 F8 / R8, 200 F14 / R14, 240 FB / R16, 257 FB 3 slots / RB, 449 FB 4 slots / RB; (256, 1, 50) FP / S
@pytest.mark.parametrize("p", [0.5, 0.9, 0.999])
@pytest.mark.parametrize("batch,heads,L", [(2, 2, 33), (2, 2, 100), (2, 2, 200), (2, 2, 240), (2, 2, 257), (2, 2, 449), (256, 1, 50)])
def test_probability_dropout_at_the_ends_of_its_range(dev, batch, heads, L, p):
    """Dropout on the probabilities at p = 0.5 / 0.9 / 0.999 against fp64 with the oracle's keep mask: the gates of the peaked cases times
    1 / (1 - p).  The streaming backward replays the forward's mask: (dropout forward, streaming backward) against the same reference."""
    from lr2ppo_amd import ops
    persistent = batch * heads >= 256
    _assert_form(batch, heads, L, persistent)
    seed, site = 77, 4
    seg = AC.masks(batch, L, fwd_block(L))["suffix"]
    c = AC.exact_qkv(batch, heads, L, seed=700 + L, logit_span=20, plant=L - 1)
    r = Run(dev, c, seg, 0.125)
    keep = O.attention_keep_mask(seed, site, batch, heads, L, p)
    ref_o, ref_lse, ref_dq, ref_dk, ref_dv = r.reference(keep=keep, p=p)
    drop, k = ops.Drop(p, seed, site), 1.0 / (1.0 - p)
    o, lse, _ = r.fwd(drop=drop)
    _check("O", o, ref_o, _o_gate(ref_o, k))
    _check("lse", lse, ref_lse, _lse_gate(ref_lse))
    for stream in ([False, True] if persistent else [False]):
        dq, dk, dv, _ = r.bwd(drop=drop, streaming=stream)
        tag = "streaming " if stream else ""
        _check(tag + "dQ", dq, ref_dq, _g_gate(ref_dq, k))
        _check(tag + "dK", dk, ref_dk, _g_gate(ref_dk, k))
        _check(tag + "dV", dv, ref_dv, _g_gate(ref_dv, k))


# ------------------------------------------------------------------------------------------------ (f) a sequence with no valid key
def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp(min=1e-300))


# 33 F4 / R4, 100 F8 / R8, 200 F14 / R14, 240 FB / R16, 257 FB / RB, 449 FB 4 slots / RB; (256, 1, 100), (128, 2, 200) FP / S
@pytest.mark.parametrize("batch,heads,L", [(2, 2, 33), (2, 2, 100), (2, 2, 200), (2, 2, 240), (2, 2, 257), (2, 2, 449), (256, 1, 100),
                                           (128, 2, 200)])
def test_all_padding_sequence(dev, batch, heads, L):
    """Mask none_valid (the last sequence has no valid key).  Contract (include/lr2ppo_hip.h): softmax over the -10000-shifted scores, as
    upstream; accurate to the fp32 grid at 10^4.  Every output finite; with V = 1 the probabilities sum to one (O = 1 to L 2^-23);
    |O - softmax(s) V| <= 2 * 2^-10 max|V| (module docstring); the gradients of that sequence against fp64 at 4 x the measured relative
    L2; the OTHER sequences of the batch meet the unchanged gates of the peaked cases (the persistent kernels prefetch the next pair's
    mask while they compute this one)."""
    persistent = batch * heads >= 256
    _assert_form(batch, heads, L, persistent)
    seg = AC.masks(batch, L, fwd_block(L))["none_valid"]
    c = AC.exact_qkv(batch, heads, L, seed=800 + L, logit_span=20, plant=L // 2)
    ones = dict(c)
    ones["v"] = torch.ones_like(c["v"])
    r1 = Run(dev, ones, seg, 0.125)
    o1, lse1, _ = r1.fwd()
    assert torch.isfinite(o1).all() and torch.isfinite(lse1).all()
    _check("V = 1: O", o1, torch.ones_like(o1), L * U)
    _check("V = 1: first_token O", r1.first_token(), torch.ones(batch, heads, 1, 64), L * U)
    r = Run(dev, c, seg, 0.125)
    ref_o, ref_lse, ref_dq, ref_dk, ref_dv = r.reference()
    free = torch.softmax(r.q[-1].double() @ r.k[-1].double().transpose(-1, -2) * 0.125, dim=-1) @ r.v[-1].double()
    grid = 2 * 2.0 ** -10 * float(r.v.abs().max())
    o, lse, _ = r.fwd()
    _check("padded sequence: O vs softmax(s) V", o[-1], free, grid)
    _check("other sequences: O", o[:-1], ref_o[:-1], _o_gate(ref_o[:-1]))
    _check("other sequences: lse", lse[:-1], ref_lse[:-1], _lse_gate(ref_lse[:-1]))
    # lse of the padded sequence = logsumexp(s) - 10000: the scores on the fp32 grid at 10^4 (2 * 2^-10 as for O) + one fp32 ulp at 10^4
    # (2^-10) for the stored value -- a mask constant in the wrong log domain is off by thousands
    _check("padded sequence: lse", lse[-1], ref_lse[-1], 3 * 2.0 ** -10)
    ft = r.first_token()
    _check("padded sequence: first_token O", ft[-1], free[:, :1], grid)
    _check("other sequences: first_token O", ft[:-1], ref_o[:-1, :, :1], _o_gate(ref_o[:-1, :, :1]))
    pad_rels = []
    for stream in ([False, True] if persistent else [False]):
        kind = "streaming" if stream else "recomputing"
        dq, dk, dv, lse_ws = r.bwd(streaming=stream)
        if not stream:
            _check("padded sequence: lse (backward)", lse_ws[-1], ref_lse[-1], 3 * 2.0 ** -10)
        rels = {}
        for name, got, ref in (("dQ", dq, ref_dq), ("dK", dk, ref_dk), ("dV", dv, ref_dv)):
            rels[name] = _rel_l2(got[-1], ref[-1])
            print(f"    padded sequence: {kind} {name} relative L2 vs fp64 {rels[name]:.3e}")
            _check(f"other sequences: {kind} {name}", got[:-1], ref[:-1], _g_gate(ref[:-1]))
        pad_rels.append((kind, rels))
    for kind, rels in pad_rels:
        for name, rel in rels.items():
            assert rel <= 4 * _PAD_BWD_MEASURED[kind], f"padded sequence: {kind} {name} relative L2 {rel:.3e}"


@pytest.mark.parametrize("batch,heads,L", [(2, 2, 33), (2, 2, 100), (2, 2, 200), (2, 2, 287), (256, 1, 100)])
def test_all_padding_sequence_bf16_forward(dev, batch, heads, L):
    seg = AC.masks(batch, L, 288)["none_valid"]
    c = AC.exact_qkv(batch, heads, L, seed=900 + L, logit_span=20, plant=L // 2)
    ones = dict(c)
    ones["v"] = torch.ones_like(c["v"])
    o1 = Run(dev, ones, seg, 0.125).bf16()
    # P is rounded to bf16 before P V while the row sum is not: sum_k bf16(p_k) / sum_k p_k = 1 to 2^-9
    _check("V = 1: O", o1, torch.ones_like(o1), 2.0 ** -9 + L * U)
    r = Run(dev, c, seg, 0.125)
    o = r.bf16()
    ref_o, _ = r.reference(grads=False)
    free = torch.softmax(r.q[-1].double() @ r.k[-1].double().transpose(-1, -2) * 0.125, dim=-1) @ r.v[-1].double()
    vmax = float(r.v.abs().max())
    _check("padded sequence: O vs softmax(s) V", o[-1], free, (2 * 2.0 ** -10 + 2.0 ** -9) * vmax)
    _check("other sequences: O", o[:-1], ref_o[:-1], _o_gate(ref_o[:-1]) + 2.0 ** -9 * vmax)


# ------------------------------------------------------------------------------------------------ (g) every element written, no more
# once per form, L no multiple of 16: 33 F4 / R4, 100 F8 / R8, 200 F14 / R14, 241 FB / R16, 257 FB 3 slots / RB, 449 FB 4 slots / RB,
# (256, 1, 33) and (128, 2, 200): FP / S; the bf16 kernel at its own lengths
@pytest.mark.parametrize("batch,heads,L", [(2, 2, 33), (2, 2, 100), (2, 2, 200), (2, 2, 241), (2, 2, 257), (2, 2, 449), (256, 1, 33),
                                           (128, 2, 200)])
def test_every_element_is_written_and_nothing_behind_the_last_row(dev, batch, heads, L):
    """O, the O planes, the dQKV planes, lse and the D workspace are allocated with one more row group (E columns' worth per plane) behind
    the last row, pre-filled with NaN patterns like the body: afterwards the body is finite and the canaries are untouched."""
    persistent = batch * heads >= 256
    _assert_form(batch, heads, L, persistent)
    seg = AC.masks(batch, L, fwd_block(L))["suffix"]
    c = AC.exact_qkv(batch, heads, L, seed=1000 + L, logit_span=20)
    r = Run(dev, c, seg, 0.125)
    o, lse, op = r.fwd()
    assert torch.isfinite(o).all() and torch.isfinite(lse).all() and torch.isfinite(op.to_float()).all()
    assert torch.isfinite(r.first_token()).all()
    for stream in ([False, True] if persistent else [False]):
        dq, dk, dv, ws = r.bwd(streaming=stream)                           # bwd() asserts that dQKV and D are finite
        assert torch.isfinite(ws).all()
    if L <= 288:
        assert torch.isfinite(r.bf16()).all()
    r.check_canaries()
