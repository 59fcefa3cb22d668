"""The head-width-general self-attention kernels (csrc/selfattn_hd.hip: lr2_self_attn_hd_fwd / lr2_self_attn_hd_bwd, head widths 32 .. 128
in steps of 16) against an fp64 reference computed from the very numbers the planes hold (tests/attn_hd_cases.py), with batch 2, 3 heads
(a middle head and a last head: a kernel that read a neighbouring head's columns as its padding would fail every check here) and a
padded suffix in sequence 1.

Every length runs one kernel form: 64-row blocks of the other operand, 4 waves x 16 rows per workgroup.  The lengths are one query block
(1, 15, 16, 17, 63, 64), the key-block seams (64 / 65, 129) and ViT-H/14's own 257.

Gates.  The project's own, from tests/test_attention_edges_gpu.py: O 2e-5 + 2e-5 |ref|; lse 1e-5 + 1e-5 |ref|; gradients
3e-5 max(1, max|ref|) + 5e-5 |ref|; dropout multiplies them by 1 / (1 - p).  Those were set at a 64-long contraction; no width up to
128 exceeds one, so none is replaced by a measured gate.  Measured over the cases of test_forward_backward_against_fp64 and test_dropout
(worst error / gate, the maximum over all widths and lengths; printed per case with -s):

    quantity   O       lse     dQ      dK      dV      all-padding O      measured
    err/gate   0.358   0.307   0.242   0.186   0.204   0.040              2026-10-21, MI355X

Two calls on the same inputs agree bit for bit (fixed summation order, no atomics): test_run_to_run_determinism.
All-padding sequence: |O - softmax(s) V| <= 2 * 2^-10 max|V|, derived in test_attention_edges_gpu.py's docstring."""
import ctypes as C

import pytest
import torch

import attn_hd_cases as HC
from oracle import lr2ppo_oracle as O

pytestmark = pytest.mark.gpu

B, H = HC.BATCH, HC.HEADS
WIDTHS = (32, 48, 80, 96, 112, 128)
LENGTHS = (1, 15, 16, 17, 63, 64, 65, 129, 257)
# every width at L in {17, 65, 257} and every L at width 80
CASES = sorted({(hd, L) for hd in WIDTHS for L in (17, 65, 257)} | {(80, L) for L in LENGTHS})
NAN32, NAN16 = 0x7FC00123, 0x7FC1            # canary patterns (quiet NaNs with a payload)


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
    worst = float((err / bound).max())
    print(f"    {what}: max err {float(err.max()):.3e}, worst err / gate {worst:.3f}")
    assert bool((err <= bound).all()), f"{what}: max err {float(err.max()):.3e}, {worst:.2f} x the gate, {int((err > bound).sum())} bad"


class Run:
    """One problem on the device: the planes, the numbers they hold, and both pairs of entry points on them."""

    def __init__(self, dev, hd, L, seed, seg=None, case=None):
        from lr2ppo_amd import _native, ops
        self.ops, self.lib, self.dev = ops, _native.lib(), dev
        self.hd, self.L, self.E, self.n = hd, L, H * hd, B * L
        self.scale = 1.0 / hd ** 0.5
        c = case if case is not None else HC.random_case(B, H, L, hd, seed)
        self.seg_cpu = HC.suffix_seg(B, L) if seg is None else seg
        self.seg = self.seg_cpu.reshape(-1).to(dev)
        self.qkv = ops.split_planes(HC.pack(c["q"], c["k"], c["v"]).to(dev), ops.Planes.empty(self.n, 3 * self.E, dev))
        self.do = ops.split_planes(HC.pack(c["do"]).to(dev), ops.Planes.empty(self.n, self.E, dev))
        self.q, self.k, self.v = (t.contiguous() for t in HC.unpack(self.qkv.to_float().cpu(), B, H, L, hd))
        (self.g,) = (t.contiguous() for t in HC.unpack(self.do.to_float().cpu(), B, H, L, hd))
        self.kw = dict(batch=B, heads=H, L=L, head_dim=hd, scale=self.scale)

    def unheads(self, x):
        return HC.unpack(x.detach().float().cpu(), B, H, self.L, self.hd)

    def reference(self, keep=None, p=0.0):
        return HC.reference(self.q, self.k, self.v, self.seg_cpu, self.scale, keep=keep, p=p, do=self.g)

    # -- through lr2ppo_amd.ops (the dispatch) --
    def fwd(self, drop=None):
        o = torch.empty(self.n, self.E, device=self.dev)
        lse = torch.empty(B * H * self.L, device=self.dev)
        self.ops.self_attn_fwd(self.qkv, self.seg, o, lse=lse, drop=drop, **self.kw)
        return o, lse

    def bwd(self, drop=None):
        d = self.ops.Planes.empty(self.n, 3 * self.E, self.dev)
        ws1, ws2 = (torch.empty(B * H * self.L, device=self.dev) for _ in range(2))
        self.ops.self_attn_bwd(self.qkv, self.do, self.seg, d, ws1, ws2, drop=drop, **self.kw)
        return d, ws1

    # -- the C entry points, by name, with free output strides --
    def c_fwd(self, name, o_ptr, o_hi_ptr, o_lo_off, ld_o, lse, drop=(0.0, 0, 0)):
        E, base = self.E, self.qkv.data_ptr()
        rc = getattr(self.lib, name)(base, base + 2 * E, base + 4 * E, self.qkv.lo_off, 3 * E, self.seg.data_ptr(), o_ptr, o_hi_ptr,
                                     o_lo_off, ld_o, lse.data_ptr() if lse is not None else None, drop[0], drop[1], drop[2], B, H,
                                     self.L, self.hd, self.scale, None)
        assert rc == 0, (name, rc)

    def c_bwd(self, name, d_ptr, d_lo_off, ld_d, ws1, ws2, drop=(0.0, 0, 0)):
        E, base = self.E, self.qkv.data_ptr()
        rc = getattr(self.lib, name)(base, base + 2 * E, base + 4 * E, self.qkv.lo_off, 3 * E, self.do.data_ptr(), self.do.lo_off, E,
                                     self.seg.data_ptr(), d_ptr, d_ptr + 2 * E, d_ptr + 4 * E, d_lo_off, ld_d, None, 0, 0,
                                     ws1.data_ptr(), ws2.data_ptr(), drop[0], drop[1], drop[2], B, H, self.L, self.hd, self.scale, None)
        assert rc == 0, (name, rc)

    def c_pair(self, fwd_name, bwd_name, drop=(0.0, 0, 0)):
        """(O, lse, dQKV as fp32) of one pair of entry points, compact strides."""
        o = torch.empty(self.n, self.E, device=self.dev)
        lse = torch.empty(B * H * self.L, device=self.dev)
        self.c_fwd(fwd_name, o.data_ptr(), None, 0, self.E, lse, drop)
        d = self.ops.Planes.empty(self.n, 3 * self.E, self.dev)
        ws1, ws2 = (torch.empty(B * H * self.L, device=self.dev) for _ in range(2))
        self.c_bwd(bwd_name, d.data_ptr(), d.lo_off, 3 * self.E, ws1, ws2, drop)
        torch.cuda.synchronize()
        return o, lse, d.to_float()


def _against_fp64(r, p=0.0, seed=0, site=0):
    keep, drop, k = None, None, 1.0
    if p > 0:
        keep = O.attention_keep_mask(seed, site, B, H, r.L, p)
        drop, k = r.ops.Drop(p, seed, site), 1.0 / (1.0 - p)
    ref_o, ref_lse, ref_dq, ref_dk, ref_dv = r.reference(keep=keep, p=p)
    before = r.ops.self_attn_hd_launch_counts()
    o, lse = r.fwd(drop=drop)
    d, lse_ws = r.bwd(drop=drop)
    assert r.ops.self_attn_hd_launch_counts() == (before[0] + 1, before[1] + 1)        # the new pair served both calls
    _check("O", r.unheads(o)[0], ref_o, _o_gate(ref_o, k))
    _check("lse", lse.view(B, H, r.L), ref_lse, _lse_gate(ref_lse))
    _check("lse (backward's)", lse_ws.view(B, H, r.L), ref_lse, _lse_gate(ref_lse))
    dq, dk, dv = r.unheads(d.to_float())
    _check("dQ", dq, ref_dq, _g_gate(ref_dq, k))
    _check("dK", dk, ref_dk, _g_gate(ref_dk, k))
    _check("dV", dv, ref_dv, _g_gate(ref_dv, k))


# ------------------------------------------------------------------------------------------------ 1. forward and backward against fp64
@pytest.mark.parametrize("hd,L", CASES)
def test_forward_backward_against_fp64(dev, hd, L):
    _against_fp64(Run(dev, hd, L, seed=1000 * hd + L))


# ------------------------------------------------------------------------------------------------ 2. dropout
@pytest.mark.parametrize("hd", [80, 128])
@pytest.mark.parametrize("L", [17, 65])
def test_dropout(dev, hd, L):
    """The forward and the backward of one call replay the mask oracle.attention_keep_mask describes: the gradients match the fp64
    autograd through that very mask."""
    _against_fp64(Run(dev, hd, L, seed=2000 * hd + L), p=0.1, seed=11 + L, site=5)


# ------------------------------------------------------------------------------------------------ 3. width 64: the new skeleton against the existing kernels
@pytest.mark.parametrize("L", [17, 65, 225])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_width_64_agrees_with_the_64_column_kernels(dev, L, p):
    """Both sit within one gate of fp64, hence within two of each other."""
    r = Run(dev, 64, L, seed=6400 + L)
    drop, k = (p, 21 + L, 3), 1.0 / (1.0 - p)
    keep = O.attention_keep_mask(drop[1], drop[2], B, H, L, p) if p > 0 else None
    ref_o, ref_lse, ref_dq, ref_dk, ref_dv = r.reference(keep=keep, p=p)
    before = r.ops.self_attn_hd_launch_counts()
    o_old, lse_old, d_old = r.c_pair("lr2_self_attn_fwd", "lr2_self_attn_bwd", drop)
    assert r.ops.self_attn_hd_launch_counts() == before
    o_new, lse_new, d_new = r.c_pair("lr2_self_attn_hd_fwd", "lr2_self_attn_hd_bwd", drop)
    assert r.ops.self_attn_hd_launch_counts() == (before[0] + 1, before[1] + 1)
    _check("O", r.unheads(o_new)[0], r.unheads(o_old)[0], 2 * _o_gate(ref_o, k))
    _check("lse", lse_new.view(B, H, L), lse_old.view(B, H, L).cpu(), 2 * _lse_gate(ref_lse))
    for name, new, old, ref in zip(("dQ", "dK", "dV"), r.unheads(d_new), r.unheads(d_old), (ref_dq, ref_dk, ref_dv)):
        _check(name, new, old, 2 * _g_gate(ref, k))


@pytest.mark.parametrize("L", [17, 65, 225])
def test_width_64_same_keep_mask_as_the_64_column_kernels(dev, L):
    """The zero pattern of O under dropout reads off the keep mask: with V = 1 a zero is a row whose keys were all dropped; with
    V[key, d] = (key % 64 == d), O[q, d] is zero exactly where every key = d (mod 64) of query q was dropped (at L = 17: keep itself)."""
    p, drop = 0.5, (0.5, 77 + L, 9)
    keep = torch.from_numpy(O.attention_keep_mask(drop[1], drop[2], B, H, L, p)).bool()
    c = HC.random_case(B, H, L, 64, seed=64000 + L)
    eye = (torch.arange(L).view(L, 1) % 64 == torch.arange(64).view(1, 64)).float()
    for one_hot in (False, True):
        c["v"] = eye.expand(B, H, L, 64).contiguous() if one_hot else torch.ones(B, H, L, 64)
        r = Run(dev, 64, L, seed=0, seg=torch.ones(B, L, dtype=torch.long), case=c)
        zeros = []
        for name in ("lr2_self_attn_fwd", "lr2_self_attn_hd_fwd"):
            o = torch.empty(r.n, r.E, device=dev)
            r.c_fwd(name, o.data_ptr(), None, 0, r.E, None, drop)
            zeros.append(r.unheads(o)[0] == 0)
        assert torch.equal(zeros[0], zeros[1])
        if one_hot:      # probabilities are positive (scores of standard normal inputs): a zero is a dropped key, nothing else
            expect = torch.stack([~keep[..., d::64].any(dim=-1) for d in range(64)], dim=-1)      # [B, H, L, 64]
            assert torch.equal(zeros[1], expect)


# ------------------------------------------------------------------------------------------------ 4. nothing outside the head is written
@pytest.mark.parametrize("hd", [48, 80, 128])
def test_gap_columns_and_guard_row_keep_their_canaries(dev, hd):
    """Output matrices with ld_o = E + 16 / ld = 3E + 16 and one guard row behind the last: the padded head columns [head_dim, HDP) of the
    LAST head would land in the gap (or, at the last row, in the guard row); every canary must keep its bits, and the columns inside
    must equal the compact call's."""
    L = 65
    r = Run(dev, hd, L, seed=4000 + hd)
    E, n = r.E, r.n
    o_c, lse_c, d_c = r.c_pair("lr2_self_attn_hd_fwd", "lr2_self_attn_hd_bwd")
    ld_o, ld_d = E + 16, 3 * E + 16
    # fp32 output
    o = torch.full(((n + 1) * ld_o,), NAN32, dtype=torch.int32, device=dev)
    r.c_fwd("lr2_self_attn_hd_fwd", o.data_ptr(), None, 0, ld_o, None)
    o2 = o.view(n + 1, ld_o)
    assert bool((o2[:, E:] == NAN32).all()) and bool((o2[n] == NAN32).all()), "fp32 O: a canary was overwritten"
    assert torch.equal(o2[:n, :E].contiguous().view(torch.float32), o_c)
    # planes output
    plane = (n + 1) * ld_o
    oh = torch.full((2 * plane,), NAN16, dtype=torch.int16, device=dev)
    r.c_fwd("lr2_self_attn_hd_fwd", None, oh.data_ptr(), plane, ld_o, None)
    for half, nm in ((oh[:plane], "hi"), (oh[plane:], "lo")):
        h2 = half.view(n + 1, ld_o)
        assert bool((h2[:, E:] == NAN16).all()) and bool((h2[n] == NAN16).all()), f"O planes ({nm}): a canary was overwritten"
        assert bool((h2[:n, :E] != NAN16).all()), f"O planes ({nm}): not every element was written"
    got = oh[:plane].view(n + 1, ld_o)[:n, :E].contiguous().view(torch.bfloat16).float() + \
        oh[plane:].view(n + 1, ld_o)[:n, :E].contiguous().view(torch.bfloat16).float()
    ref_pl = r.ops.split_planes(o_c.contiguous(), r.ops.Planes.empty(n, E, dev)).to_float()
    assert torch.equal(got, ref_pl)
    # dQKV planes
    plane = (n + 1) * ld_d
    d = torch.full((2 * plane,), NAN16, dtype=torch.int16, device=dev)
    ws1, ws2 = (torch.empty(B * H * L, device=dev) for _ in range(2))
    r.c_bwd("lr2_self_attn_hd_bwd", d.data_ptr(), plane, ld_d, ws1, ws2)
    for half, nm in ((d[:plane], "hi"), (d[plane:], "lo")):
        h2 = half.view(n + 1, ld_d)
        assert bool((h2[:, 3 * E:] == NAN16).all()) and bool((h2[n] == NAN16).all()), f"dQKV planes ({nm}): a canary was overwritten"
    got = d[:plane].view(n + 1, ld_d)[:n, :3 * E].contiguous().view(torch.bfloat16).float() + \
        d[plane:].view(n + 1, ld_d)[:n, :3 * E].contiguous().view(torch.bfloat16).float()
    assert torch.equal(got, d_c)


# ------------------------------------------------------------------------------------------------ 5. run-to-run determinism
def test_run_to_run_determinism(dev):
    r = Run(dev, 80, 257, seed=5)
    drop = r.ops.Drop(0.1, 1234, 2)
    o1, lse1 = r.fwd(drop=drop)
    d1, _ = r.bwd(drop=drop)
    o2, lse2 = r.fwd(drop=drop)
    d2, _ = r.bwd(drop=drop)
    assert torch.equal(o1, o2) and torch.equal(lse1, lse2)
    assert torch.equal(d1.buf, d2.buf)


# ------------------------------------------------------------------------------------------------ 6. all-padding sequence
def test_all_padding_sequence(dev):
    """seg = 0 on all of sequence 1: every key carries -10000, the softmax runs over the shifted scores as upstream's does."""
    hd, L = 80, 33
    seg = torch.ones(B, L, dtype=torch.long)
    seg[1] = 0
    r = Run(dev, hd, L, seed=6, seg=seg)
    o, lse = r.fwd()
    d, _ = r.bwd()
    o = r.unheads(o)[0]
    assert torch.isfinite(o).all() and torch.isfinite(lse).all() and torch.isfinite(d.to_float()).all()
    ref_o, _ = HC.reference(r.q, r.k, r.v, torch.ones(B, L, dtype=torch.long), r.scale)       # softmax(s) V: the shift cancels
    _check("O, valid sequence", o[0], ref_o[0], _o_gate(ref_o[0]))
    bound = 2 * 2.0 ** -10 * float(r.v[1].abs().max())
    _check("O, all-padding sequence", o[1], ref_o[1], torch.full_like(ref_o[1], bound))
