"""Case builders and the fp64 reference of the head-width tests (test_selfattn_hd_cpu.py / test_selfattn_hd_gpu.py): tests/attn_cases.py's
pack / unpack / reference restated for a free head width (that module fixes 64).  Nothing here touches the GPU or lr2ppo_amd.ops.
Tensors are [batch, heads, L, head_dim] on the CPU; pack() / unpack() convert to and from the [batch * L, n * heads * head_dim] matrices
the kernels read."""
import numpy as np
import torch

MASK = -10000.0
BATCH, HEADS = 2, 3            # a middle head and a last head; sequence 1 carries the padded suffix


def pack(*ts):
    """[batch, heads, L, hd] tensors -> one [batch * L, len(ts) * heads * hd] matrix (head h in columns hd h .. hd h + hd - 1 of its part)."""
    b, h, L, hd = ts[0].shape
    return torch.cat([t.transpose(1, 2).reshape(b * L, h * hd) for t in ts], dim=1).contiguous()


def unpack(x, batch, heads, L, hd):
    """[batch * L, n * heads * hd] -> n tensors [batch, heads, L, hd]."""
    return tuple(t.reshape(batch, L, heads, hd).transpose(1, 2) for t in x.split(heads * hd, dim=1))


def suffix_seg(batch, L):
    """seg [batch, L] (a key is valid where seg > 0): the last sequence's last third is padding (at L = 1 nothing is)."""
    seg = torch.ones(batch, L, dtype=torch.long)
    seg[-1, max(1, (2 * L) // 3):] = 0
    return seg


def random_case(batch, heads, L, hd, seed):
    """dict(q, k, v, do) of standard normal fp32 tensors [batch, heads, L, hd] from one seeded generator."""
    gen = torch.Generator().manual_seed(seed)
    return {n: torch.randn(batch, heads, L, hd, generator=gen) for n in ("q", "k", "v", "do")}


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
