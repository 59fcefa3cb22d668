"""The case builders and the fp64 reference of the self-attention edge tests are themselves correct (tests/attn_cases.py): what the GPU
tests assert about the kernels rests on the properties checked here.  No GPU, nothing from lr2ppo_amd.ops."""
import math

import pytest
import torch

import attn_cases as AC

SHAPES = [(2, 2, 1), (1, 2, 17), (2, 1, 65), (1, 2, 257), (1, 1, 514)]


def _block(L):
    return 128 if L > 256 else 16 * 14


def _scores(c, scale, dtype, order=None):
    q, k = c["q"].to(dtype), c["k"].to(dtype)
    if order is None:
        return q @ k.transpose(-1, -2) * scale
    s = torch.zeros(q.shape[:-1] + (k.shape[-2],), dtype=dtype)
    for d in order:                                                        # one rounded addition per head column, in the given order
        s = s + q[..., :, None, d] * k[..., None, :, d]
    return s * scale


@pytest.mark.parametrize("batch,heads,L", SHAPES)
@pytest.mark.parametrize("span,scale", [(0, 0.125), (2, 0.125), (20, 0.125), (100, 0.125), (20, 1.0), (20, 2.0 ** -5)])
def test_exact_qkv_is_bf16_valued_with_exact_scores(batch, heads, L, span, scale):
    """Every entry is a bf16 number; the fp32 scores and the fp32 dP = dO V^T, summed forwards and backwards over the head columns, equal
    the fp64 ones -- with and without a planted key."""
    for plant in (None, L - 1):
        c = AC.exact_qkv(batch, heads, L, seed=3 * L + span, logit_span=span, scale=scale, plant=plant)
        for t in c.values():
            assert torch.equal(t.to(torch.bfloat16).float(), t)
        ref = _scores(c, scale, torch.float64)
        for order in (range(64), reversed(range(64))):
            assert torch.equal(_scores(c, scale, torch.float32, order).double(), ref)
        dp = c["do"].double() @ c["v"].double().transpose(-1, -2)
        assert torch.equal((c["do"] @ c["v"].transpose(-1, -2)).double(), dp)
        if span == 0:
            assert not c["q"].any()


@pytest.mark.parametrize("L", [1, 17, 65, 257])
@pytest.mark.parametrize("span,scale", [(2, 0.125), (20, 0.125), (100, 0.125), (20, 1.0), (20, 0.25), (20, 2.0 ** -5)])
def test_logit_span_is_met_within_a_factor_two(L, span, scale):
    """The spans and scales the GPU tests use (exact_qkv refuses a span its grid cannot reach within a factor 2)."""
    c = AC.exact_qkv(2, 2, L, seed=L + span, logit_span=span, scale=scale)
    top = float(_scores(c, scale, torch.float64).abs().max())
    assert span / 2 <= top <= span * 2, top


@pytest.mark.parametrize("batch,heads,L", SHAPES)
@pytest.mark.parametrize("mask", AC.MASKS)
@pytest.mark.parametrize("position", AC.POSITIONS)
def test_planted_key_is_the_row_maximum_unless_masked(batch, heads, L, mask, position):
    """The planted key holds the strict maximum of its query's raw scores, at least twice the runner-up and below 5000; it is the
    strict maximum after masking exactly when it is a valid key -- planted on a masked key it loses to a valid one."""
    seg = AC.masks(batch, L, _block(L))[mask]
    key = AC.plant_key(position, L, _block(L), seg)
    assert 0 <= key < L
    for span in (2, 100):
        c = AC.exact_qkv(batch, heads, L, seed=11 + L, logit_span=span, plant=key)
        s = _scores(c, 0.125, torch.float64)
        for b in range(batch):
            for h in range(heads):
                row = s[b, h, AC.plant_query(b, h, L)]
                rest = torch.cat([row[:key], row[key + 1:]])
                assert 2 * span <= row[key] < 5000
                if rest.numel():
                    assert row[key] >= 2 * rest.abs().max()
                masked = row + (seg[b] <= 0).double() * AC.MASK
                if seg[b, key] > 0:
                    assert int(masked.argmax()) == key and (rest.numel() == 0 or masked[key] > torch.cat([masked[:key], masked[key + 1:]]).max())
                else:
                    assert int(row.argmax()) == key and int(masked.argmax()) != key and seg[b, int(masked.argmax())] > 0


@pytest.mark.parametrize("L,block", [(1, 224), (15, 224), (64, 224), (225, 160), (257, 128), (449, 160), (514, 192)])
def test_mask_patterns(L, block):
    m = AC.masks(3, L, block)
    assert set(m) == set(AC.MASKS) | {"only_first", "none_valid"}
    for name, seg in m.items():
        assert seg.shape == (3, L) and seg.dtype == torch.long
        if name != "none_valid":
            assert ((seg > 0).sum(dim=1) >= 1).all(), name                   # every sequence keeps a valid key
    assert m["only_first"].sum() == 3 and (m["only_first"][:, 0] == 1).all()
    assert not m["none_valid"][-1].any() and torch.equal(m["none_valid"][:-1], m["suffix"][:-1])
    assert m["suffix"][:-1].all() and (L == 1 or not m["suffix"][-1, -1])
    assert m["prefix_block"][1].all() and m["hole"][1].all()                  # the sequences in between stay whole
    if L > 2 * block:
        assert not m["prefix_block"][-1, :block].any() and m["prefix_block"][-1, block:].all()
        assert not m["hole"][-1, block:2 * block].any() and m["hole"][-1, :block].all() and m["hole"][-1, 2 * block:].all()
    if L > 1:
        assert not m["prefix_block"][-1, 0] and m["prefix_block"][-1, -1]
        assert m["alternate"][-1, 0::2].all() and not m["alternate"][-1, 1::2].any()


def _loop_reference(q, k, v, seg, scale):
    batch, heads, L, _ = q.shape
    o = torch.zeros(batch, heads, L, 64, dtype=torch.float64)
    for b in range(batch):
        for h in range(heads):
            for i in range(L):
                s = [sum(float(q[b, h, i, d]) * float(k[b, h, j, d]) for d in range(64)) * scale + (0.0 if seg[b, j] > 0 else AC.MASK)
                     for j in range(L)]
                mx = max(s)
                e = [math.exp(x - mx) for x in s]
                z = sum(e)
                for j in range(L):
                    o[b, h, i] += e[j] / z * v[b, h, j].double()
    return o


@pytest.mark.parametrize("batch,heads,L,mask", [(2, 2, 17, "suffix"), (1, 2, 65, "alternate"), (2, 1, 257, "hole")])
def test_reference_agrees_with_an_independent_evaluation(batch, heads, L, mask):
    """reference() against torch's scaled_dot_product_attention in fp64 with an additive mask (a plain loop where torch has none), with
    the gradients of both by autograd: 1e-12."""
    import torch.nn.functional as F
    seg = AC.masks(batch, L, 128)[mask]
    c = AC.exact_qkv(batch, heads, L, seed=5, logit_span=20, plant=L - 1)
    o, lse, dq, dk, dv = AC.reference(c["q"], c["k"], c["v"], seg, 0.125, do=c["do"])
    if hasattr(F, "scaled_dot_product_attention"):
        q, k, v = (c[n].double().requires_grad_(True) for n in "qkv")
        add = ((seg <= 0).double() * AC.MASK).view(batch, 1, 1, L).expand(batch, heads, L, L)
        o2 = F.scaled_dot_product_attention(q, k, v, attn_mask=add, scale=0.125)
        o2.backward(c["do"].double())
        for got, ref in ((o, o2.detach()), (dq, q.grad), (dk, k.grad), (dv, v.grad)):
            assert (got - ref).abs().max() <= 1e-12 * max(1.0, float(ref.abs().max()))
    else:
        assert (o[:, :, :4] - _loop_reference(c["q"][:, :, :4], c["k"], c["v"], seg, 0.125)).abs().max() <= 1e-12 * float(o.abs().max())
    s = c["q"].double() @ c["k"].double().transpose(-1, -2) * 0.125 + ((seg <= 0).double() * AC.MASK).view(batch, 1, 1, L)
    assert (lse - s.exp().sum(-1).log()).abs().max() < 1e-12 * max(1.0, float(lse.abs().max())) or float(s.max()) > 700


def test_reference_applies_the_dropout_mask_after_the_softmax():
    batch, heads, L, p = 2, 2, 19, 0.5
    from oracle import lr2ppo_oracle as O
    keep = O.attention_keep_mask(7, 3, batch, heads, L, p)
    seg = AC.masks(batch, L, 224)["suffix"]
    c = AC.exact_qkv(batch, heads, L, seed=9, logit_span=2)
    o, lse = AC.reference(c["q"], c["k"], c["v"], seg, 0.125, keep=keep, p=p)
    s = c["q"].double() @ c["k"].double().transpose(-1, -2) * 0.125 + ((seg <= 0).double() * AC.MASK).view(batch, 1, 1, L)
    pr = torch.softmax(s, -1) * torch.from_numpy(keep).double() / (1 - p)
    assert (o - pr @ c["v"].double()).abs().max() < 1e-12 and (lse - torch.logsumexp(s, -1)).abs().max() < 1e-12
    assert 0.3 < keep.mean() < 0.7


@pytest.mark.parametrize("batch,heads,L", [(2, 2, 17), (1, 2, 257)])
def test_reference_closed_forms_for_one_valid_key_and_for_zero_queries(batch, heads, L):
    """only_first: O[q] = V[0], lse[q] = s[q, 0], dQ = dK = 0, dV[0] = sum_q dO[q], dV[k > 0] = 0 -- exactly, in fp64 too (the masked
    keys' exp(-10000 + ...) underflows to 0).  Q = 0: P = 1 / n, lse = log n, O = the mean of the valid V rows, dK = 0."""
    m = AC.masks(batch, L, 128)
    c = AC.exact_qkv(batch, heads, L, seed=2, logit_span=20)
    o, lse, dq, dk, dv = AC.reference(c["q"], c["k"], c["v"], m["only_first"], 0.125, do=c["do"])
    assert torch.equal(o, c["v"][:, :, :1].double().expand_as(o))
    assert torch.equal(lse, (c["q"].double() @ c["k"].double().transpose(-1, -2))[..., 0] * 0.125)
    assert not dq.any() and not dk.any() and not dv[:, :, 1:].any()
    assert torch.equal(dv[:, :, 0], c["do"].double().sum(dim=2))
    z = AC.exact_qkv(batch, heads, L, seed=2, logit_span=0)
    for name in ("suffix", "alternate", "hole"):
        seg = m[name]
        o, lse, dq, dk, dv = AC.reference(z["q"], z["k"], z["v"], seg, 0.125, do=z["do"])
        n = (seg > 0).sum(dim=1).double()
        assert (lse - n.log().view(batch, 1, 1)).abs().max() < 1e-14
        mean = ((seg > 0).double().view(batch, 1, L, 1) * z["v"].double()).sum(dim=2, keepdim=True) / n.view(batch, 1, 1, 1)
        assert (o - mean).abs().max() < 1e-14 and not dk.any()


@pytest.mark.parametrize("L,span", [(17, 2), (65, 20), (257, 100)])
def test_all_padding_sequence_fp32_grid_bound_holds_for_the_reference(L, span):
    """A sequence with no valid key: upstream's fp32 softmax(s - 10000) sees the scores on the fp32 grid at 10^4 (2^-10).  Rounding
    moves a score by <= 2^-11, a probability by <= 2 * 2^-11 relative (maximum and sum both move), so
    |softmax(fl32(s - 10000)) V - softmax(s) V| <= 2 * 2^-10 * max|V| with the factor 2 of margin the GPU test grants the kernels."""
    batch, heads = 2, 2
    seg = AC.masks(batch, L, 128)["none_valid"]
    c = AC.exact_qkv(batch, heads, L, seed=L, logit_span=span)
    s = c["q"].double() @ c["k"].double().transpose(-1, -2) * 0.125
    shifted = (s.float() - 10000.0).double()
    assert ((shifted + 10000.0) - s).abs().max() <= 2.0 ** -11
    v = c["v"].double()
    free = torch.softmax(s[-1], -1) @ v[-1]
    assert ((torch.softmax(shifted[-1], -1) @ v[-1]) - free).abs().max() <= 2 * 2.0 ** -10 * float(v.abs().max())
    o, _ = AC.reference(c["q"], c["k"], c["v"], seg, 0.125)                  # fp64: the shift is exact to 2^-39, far inside the bound
    assert (o[-1] - free).abs().max() <= 2 * 2.0 ** -10 * float(v.abs().max())
    assert (o[-1] - free).abs().max() < 1e-9 * float(v.abs().max())


def test_every_kernel_form_sees_every_position_mask_pair_and_every_span():
    """The peaked-softmax cases of the GPU tests (attn_cases.peaked_plan): each kernel form gets all 16 (planted position, mask) pairs
    and all three logit spans."""
    seen = {f: (set(), set()) for f in AC.FORMS}
    for forms, pos, mask, span in AC.peaked_plan():
        for f in forms:
            seen[f][0].add((pos, mask))
            seen[f][1].add(span)
    for f, (pairs, spans) in seen.items():
        assert len(pairs) == 16 and spans == set(AC.SPANS), (f, len(pairs), spans)
    assert AC.fwd_block(257) == 160 and AC.fwd_block(384) == 192 and AC.fwd_block(385) == 224 and AC.fwd_block(448) == 224
    assert AC.fwd_block(449) == 160 and AC.fwd_block(514) == 192 and AC.bwd_block(257) == 128 and AC.bwd_block(256) == 256


def test_log2_domain_lse_of_one_valid_key_is_within_one_ulp_on_the_exact_scores():
    """The one-block / persistent forward returns lse = fl(fl(s * fl(scale * log2 e)) * ln 2) + log 1 for a single valid key.  Two
    roundings of half an ulp each plus the constants' own errors (log2 e * ln 2 = 1 + 2^-25.9 in fp32) can reach 1.14 x 2^-23 |s| in
    general; on the scores exact_qkv produces (multiples of 1/4 times a power-of-two scale, |s| <= 250) the worst is 0.73, which is why
    the GPU test may ask for 2^-23 |s| there.  Restated here in numpy fp32."""
    import numpy as np
    f = np.float32
    log2e, ln2 = f(1.4426950408889634), f(0.6931471805599453)
    for scale in (0.125,):
        raw = np.arange(-8000, 8001, dtype=np.float64) * 0.25
        mx = (raw.astype(f) * f(f(scale) * log2e)).astype(f)
        lse = (mx * ln2).astype(f).astype(np.float64)
        true = raw * scale
        assert (np.abs(lse - true) <= 2.0 ** -23 * np.abs(true)).all()
