"""Case builders and the fp64 reference of the self-attention edge tests (test_attention_edges_cpu.py / test_attention_edges_gpu.py).

Nothing here touches the GPU or lr2ppo_amd.ops.  Tensors are [batch, heads, L, 64] on the CPU; pack() / unpack() convert to and from
the [batch * L, 3 * heads * 64] = [Q | K | V] matrix the kernels read.

Why "exact" inputs: every entry is (an integer of at most 7 bits) x (a power of two), i.e. a bf16 number, so the lo planes of the
split-bf16 operands are zero and each of the three passes of the split product adds integers (in units of 1/4) far below 2^24: with
`scale` a power of two every score sum_d q_d k_d * scale and every dP = dO V^T is the SAME fp32 number in any summation order.  What
is left to tolerate is the softmax arithmetic alone, so index maps, masks and the running-max rescale are tested sharply."""
import functools
import math

import numpy as np
import torch

HD = 64
MASK = -10000.0
POSITIONS = ("key0", "last", "block2", "masked")
MASKS = ("suffix", "prefix_block", "hole", "alternate")
_ROW_POW2 = torch.tensor([0.5, 1.0, 2.0])


# ---- the dispatch, restated from lr2ppo_amd/csrc/selfattn_fwd.hip (lr2_self_attn_fwd / fwd_blocked_dispatch), selfattn_bwd.hip (lr2_self_attn_bwd) and
# selfattn_mx.hip (lr2_self_attn_fwd_bf16); DESIGN.md 4.5 has the table.  `persistent` = batch * heads >= the CU count. ----
def fwd_block(L):
    """Key-block length of the forward at this L."""
    if L <= 224:
        return 64 if L <= 64 else 128 if L <= 128 else 224
    nb = (L + 223) // 224
    tiles = ((L + nb - 1) // nb + 15) // 16
    return 16 * (10 if tiles <= 10 else 12 if tiles <= 12 else 14)


def bwd_block(L):
    return 128 if L > 256 else 64 if L <= 64 else 128 if L <= 128 else 224 if L <= 224 else 256


def _tiles(L):
    return 4 if L <= 64 else 8 if L <= 128 else 14


def fwd_form(L, persistent):
    if L > 224:
        return "FB"
    return ("FP%d" if persistent else "F%d") % _tiles(L)


def bwd_forms(L, persistent):
    """The recomputing form, and the streaming one where a call given the forward's output takes it."""
    if L > 256:
        return ("RB",)
    if L > 224:
        return ("R16",)
    return ("R%d" % _tiles(L),) + (("S%d" % _tiles(L),) if persistent else ())


def bf16_form(L, persistent):
    return "BP" if persistent else "B%d" % (18 if L > 224 else _tiles(L))


# the lengths of the peaked-softmax cases: every dispatch edge on the one-pair / blocked forms, and the persistent forms
EDGE_L = (1, 15, 16, 17, 64, 65, 128, 129, 224, 225, 256, 257, 384, 385, 448, 449, 512, 513, 514)
PERSIST_L = (16, 33, 64, 65, 128, 129, 224)
PERSIST_SHAPES = ((256, 1), (128, 2))
BF16_SHAPES = ((2, 2, 17), (2, 2, 65), (2, 2, 129), (2, 2, 288), (256, 1, 33), (128, 2, 225))
SPANS = (2, 20, 100)
FORMS = ("F4", "F8", "F14", "FB", "FP4", "FP8", "FP14", "R4", "R8", "R14", "R16", "RB", "S4", "S8", "S14", "FT",
         "B4", "B8", "B14", "B18", "BP")


def peaked_cases(i, L, n=16):
    """n (position, mask, span, block) combinations for the i-th length of a list: pair number p = (n i + j) mod 16 is
    (POSITIONS[p % 4], MASKS[p // 4]), so n = 16 gives every pair at every length and n = 8 gives them to two neighbouring lengths;
    the span rotates with p + i and the mask's block is the forward's or the backward's by turns."""
    out = []
    for j in range(n):
        p = (n * i + j) % 16
        block = fwd_block(L) if (p + p // 4 + i) % 2 == 0 else bwd_block(L)
        out.append((POSITIONS[p % 4], MASKS[p // 4], SPANS[(p + i) % 3], block))
    return out


def peaked_plan():
    """(forms, position, mask, span) of every peaked-softmax case test_attention_edges_gpu.py runs: what its parametrisation is built
    from, and what test_attention_edges_cpu.py checks for coverage."""
    out = []
    for i, L in enumerate(EDGE_L):
        for pos, mask, span, _ in peaked_cases(i, L, 16):
            out.append(((fwd_form(L, False), "FT") + bwd_forms(L, False), pos, mask, span))
    for i, L in enumerate(PERSIST_L):
        for pos, mask, span, _ in peaked_cases(i, L, 8):
            out.append(((fwd_form(L, True), "FT") + bwd_forms(L, True), pos, mask, span))
    for i, (batch, heads, L) in enumerate(BF16_SHAPES):
        persistent = batch * heads >= 256
        for pos, mask, span, _ in peaked_cases(i, L, 8 if persistent else 16):
            out.append(((bf16_form(L, persistent),), pos, mask, span))
    return out


def _ints(gen, shape, a):
    """randint(-a, a + 1) times a power of two in {1/2, 1, 2} per row (last dimension)."""
    x = torch.randint(-a, a + 1, shape, generator=gen).float()
    r = _ROW_POW2[torch.randint(0, 3, shape[:-1], generator=gen)]
    return x * r.unsqueeze(-1)


def _unit(L, block):
    """Width of the masked prefix / hole: the kernel's key block where the sequence has more than one, else one 16-key tile, else
    half the sequence -- always < L for L > 1, so that a valid key remains."""
    if block < L:
        return block
    return 16 if L > 16 else max(1, L // 2)


def masks(batch, L, block):
    """name -> seg [batch, L] (int64; a key is valid where seg > 0).  `block` = the key-block length of the kernel under test at this L
    (read from its dispatch code by the caller).  The pattern is laid on the last sequence and every second one before it; the
    sequences between them stay fully valid, so that neighbouring (sequence, head) pairs carry different masks.  L = 1 has one key,
    which stays valid in every pattern but none_valid."""
    u = _unit(L, block)
    on = [b for b in range(batch) if (batch - 1 - b) % 2 == 0]
    out = {}
    seg = torch.ones(batch, L, dtype=torch.long)
    seg[-1, max(1, (2 * L) // 3):] = 0
    out["suffix"] = seg
    seg = torch.zeros(batch, L, dtype=torch.long)
    seg[:, 0] = 1
    out["only_first"] = seg
    seg = torch.ones(batch, L, dtype=torch.long)
    if L > 1:
        seg[on, :u] = 0
    out["prefix_block"] = seg
    seg = torch.ones(batch, L, dtype=torch.long)
    seg[on, u:min(2 * u, L - 1)] = 0
    out["hole"] = seg
    seg = torch.ones(batch, L, dtype=torch.long)
    seg[on, 1::2] = 0
    out["alternate"] = seg
    seg = out["suffix"].clone()
    seg[-1, :] = 0
    out["none_valid"] = seg
    return out


def plant_key(position, L, block, seg):
    """Key index of a named planting position.  block2 = the first key of the second key block (of the second 16-key tile where the
    kernel has one block); masked = the first key that is masked in every sequence that has a masked key (key 0 when there is none)."""
    if position == "key0":
        return 0
    if position == "last":
        return L - 1
    if position == "block2":
        return _unit(L, block) if L > 1 else 0
    if position == "masked":
        rows = seg[(seg <= 0).any(dim=1)]
        if rows.numel() == 0:
            return 0
        idx = torch.nonzero((rows <= 0).all(dim=0)).flatten()
        return int(idx[0]) if idx.numel() else 0
    raise ValueError(position)


def plant_query(b, h, L):
    """The query whose row maximum is planted in pair (b, h): a different row per pair."""
    return (7 * b + 3 * h + L // 3) % L


_CUTS = (0, 1, 2, 4, 8, 16, 32, 64)


@functools.lru_cache(maxsize=8)
def _base(batch, heads, L, seed, logit_span, scale):
    """(q, k, v, do) before planting; callers clone.  The scores are exact in fp32, so those of the first n columns are partial sums."""
    gen = torch.Generator().manual_seed(seed)
    k = _ints(gen, (batch, heads, L, HD), 4)
    v = _ints(gen, (batch, heads, L, HD), 4)
    do = _ints(gen, (batch, heads, L, HD), 4)
    q = torch.zeros(batch, heads, L, HD)
    if logit_span > 0:
        best, nb = None, min(batch, 4)                  # (a, n) is picked on the first sequences and verified on all of them
        for a in (1, 2, 4, 8, 16, 32, 64):
            qa = _ints(torch.Generator().manual_seed(seed + 1000 * a), (batch, heads, L, HD), a)
            part = torch.zeros(nb, heads, L, L)
            for lo, n in zip(_CUTS[:-1], _CUTS[1:]):
                part = part + qa[:nb, ..., lo:n] @ k[:nb, ..., lo:n].transpose(-1, -2)
                top = float(part.abs().max()) * scale
                miss = abs(math.log(max(top, 1e-30) / logit_span))
                if best is None or miss < best[0]:
                    best = (miss, a, n, qa)
        q = best[3].clone()
        q[..., best[2]:] = 0
        top = float((q @ k.transpose(-1, -2)).abs().max()) * scale
        if not logit_span / 2 <= top <= logit_span * 2:
            raise ValueError("logit_span out of reach of the grid at this scale")
    return q, k, v, do


def exact_qkv(batch, heads, L, seed, logit_span, scale=0.125, plant=None):
    """dict(q, k, v, do) of [batch, heads, L, 64] fp32 tensors with exact scores (module docstring).  K, V, dO: randint(-4, 5) x a row
    power of two.  Q: randint(-a, a + 1) on the first n of the 64 columns, (a, n) picked from a fixed grid so that the largest
    |q . k| * scale comes closest to `logit_span` (0: Q = 0).  plant = key index: in every pair (b, h) the K row of that key is
    overwritten with c x the Q row of query plant_query(b, h, L), c the power of two that puts this score at least 2 x above every other
    score of the row and of logit_span (and below 5000, so that a -10000 mask still decides)."""
    if scale <= 0 or math.frexp(scale)[0] != 0.5:
        raise ValueError("exact scores need a power-of-two scale")
    q, k, v, do = (t.clone() for t in _base(batch, heads, L, seed, logit_span, scale))
    if plant is not None and logit_span > 0:
        for b in range(batch):
            for h in range(heads):
                qi = plant_query(b, h, L)
                if not q[b, h, qi].any():
                    q[b, h, qi, 0] = 1.0
                row = q[b, h, qi]
                others = (k[b, h] @ row).abs()
                others[plant] = 0
                need = 2.0 * max(float(others.max()) * scale, float(logit_span))
                c = 2.0 ** math.ceil(math.log2(need / (float(row @ row) * scale)))
                k[b, h, plant] = c * row
                if float(row @ row) * c * scale >= 5000:
                    raise ValueError("planted score too large for the -10000 mask to decide")
    for name, t in (("q", q), ("k", k), ("v", v), ("do", do)):
        assert torch.equal(t.to(torch.bfloat16).float(), t), name
    return {"q": q, "k": k, "v": v, "do": do}


def pack(*ts):
    """[batch, heads, L, 64] tensors -> one [batch * L, len(ts) * heads * 64] matrix (head h in columns 64 h .. 64 h + 63 of its part)."""
    b, h, L, _ = ts[0].shape
    return torch.cat([t.transpose(1, 2).reshape(b * L, h * HD) for t in ts], dim=1).contiguous()


def unpack(x, batch, heads, L):
    """[batch * L, n * heads * 64] -> n tensors [batch, heads, L, 64]."""
    E = heads * HD
    return tuple(t.reshape(batch, L, heads, HD).transpose(1, 2) for t in x.split(E, dim=1))


def reference(q, k, v, seg, scale, keep=None, p=0.0, do=None):
    """fp64 softmax(Q K^T scale - 10000 (seg <= 0)) * keep / (1 - p) @ V on the numbers given (the expression of upstream's
    multi_headed_attn.py:61-74).  Returns (O, lse) -- lse of the masked scores, before dropout -- and with `do` also (dQ, dK, dV) by
    fp64 autograd.  keep: bool / 0-1 array [batch, heads, L, L] (oracle.lr2ppo_oracle.attention_keep_mask)."""
    batch, heads, L, _ = q.shape
    qd, kd, vd = (t.detach().double().clone().requires_grad_(do is not None) for t in (q, k, v))
    mask = (seg.view(batch, 1, 1, L) <= 0).double() * MASK
    s = qd @ kd.transpose(-1, -2) * scale + mask
    pr = torch.softmax(s, dim=-1)
    if keep is not None:
        pr = pr * (torch.as_tensor(np.asarray(keep, dtype=np.float64)).view(batch, heads, L, L) / (1.0 - p))
    o = pr @ vd
    lse = torch.logsumexp(s.detach(), dim=-1)
    if do is None:
        return o.detach(), lse
    o.backward(do.double())
    return o.detach(), lse, qd.grad, kd.grad, vd.grad
