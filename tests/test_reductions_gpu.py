"""Edge tests of the kernels that reduce across lanes, waves and workgroups: LayerNorm forward / backward, the column sums and their
finishing kernel (csrc/norm.hip), the fused PPO loss, SmoothL1, the 768 -> 1 head and the period-row gradient (csrc/misc.hip).

Every reference is fp64 torch on the CPU (the oracle's formulas, autograd for the gradients), never another kernel of this project;
the one exception is a claim of the form "same bits as form X".  Gates for O(1) data are the ones tests/test_kernels_gpu.py uses for
the same quantity; wherever the inputs make the result exactly representable (small integers) the check is torch.equal, which does
not depend on the summation order.  The two derived gates (offset rows, small-variance rows) carry their derivation in the test's
docstring.  The case builders and references at the top need no GPU: tests/test_reductions_cpu.py imports them and checks the
properties the GPU tests rely on (guard bands of the committed seeds, the derived gates, the wrong-reference margin).
"""
import math

import numpy as np
import pytest
import torch

from oracle import lr2ppo_oracle as O

pytestmark = pytest.mark.gpu

NAN = float("nan")
LN_EPS = {0: 1e-5, 1: 1e-6}         # the eps each semantics runs with in the product (nn.LayerNorm / TencentPretrain LayerNorm)


# ======================================================================================================================
# CPU side: inputs, fp64 references, guard bands (imported by tests/test_reductions_cpu.py)
# ======================================================================================================================
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rand(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def _ints(g, lo, hi, *shape):
    """integer-valued fp32 in [lo, hi]"""
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _close(got, ref, atol, rtol, what=""):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    err = (got - ref).abs()
    bound = atol + rtol * ref.abs()
    bad = err > bound
    assert not bad.any(), f"{what}: max err {err.max().item():.3e} (ref scale {ref.abs().max().item():.3e}), {int(bad.sum())} bad"


def _within(got, ref, bound, what=""):
    err = (got.detach().double().cpu() - ref.double()).abs()
    bad = err > bound
    assert not bad.any(), f"{what}: max err / bound {(err / bound).max().item():.3f}, {int(bad.sum())} bad"


def ulp32(t):
    """spacing of fp32 at |t| (t: fp64 tensor)"""
    return torch.from_numpy(np.spacing(np.abs(t.numpy().astype(np.float32))).astype(np.float64))


def ln_ref(x, gam, bet, mode, eps=None):
    eps = LN_EPS[mode] if eps is None else eps
    return (O.layernorm_torch if mode == 0 else O.layernorm_tp)(x, gam, bet, eps)


def ln_stats(x64, mode, eps=None):
    """mean and rstd as the kernel defines them: 1 / sqrt(var_biased + eps) (mode 0), 1 / (std_unbiased + eps) (mode 1)"""
    eps = LN_EPS[mode] if eps is None else eps
    mean = x64.mean(-1)
    if mode == 0:
        return mean, 1.0 / torch.sqrt(((x64 - mean[:, None]) ** 2).mean(-1) + eps)
    return mean, 1.0 / (x64.std(-1) + eps)


def ln_bwd_ref(x, gam, bet, dy, mode, eps=None):
    """fp64 autograd through the oracle's forward -> (dx, dgamma, dbeta)"""
    xt, gt, bt = (t.double().requires_grad_(True) for t in (x, gam, bet))
    ln_ref(xt, gt, bt, mode, eps).backward(dy.double())
    return xt.grad, gt.grad, bt.grad


def ln_case(rows, D, seed, x_scale=1.0, x_shift=0.0):
    g = _gen(seed)
    return dict(x=_rand(g, rows, D) * x_scale + x_shift, gam=_rand(g, D), bet=_rand(g, D), dy=_rand(g, rows, D), rg=_rand(g, rows, D))


def offset_rows_case(D, mode):
    """x = 8 + 0.05 randn: rows whose mean is 160 standard deviations from zero.  Returns the inputs, the fp64 reference and the gate of
    test_layernorm_fwd_offset_rows (derivation there)."""
    g = _gen(8000 + D + mode)
    rows = 9
    x, gam, bet = 8.0 + 0.05 * _rand(g, rows, D), _rand(g, D), _rand(g, D)
    x64 = x.double()
    ref = ln_ref(x64, gam.double(), bet.double(), mode)
    mean, rstd = ln_stats(x64, mode)
    k = math.log2(D) + 2
    bound = 1e-5 + 1e-5 * ref.abs() + k * (ulp32(mean) * rstd)[:, None] * gam.double().abs()[None, :]
    return dict(x=x, gam=gam, bet=bet, ref=ref, bound=bound, mean=mean, rstd=rstd, rows=rows)


SMALL_VAR_EPS = 1e-6
SMALL_VAR_GATE = 1e-4              # of the row's max |dx_ref|


def tp_bwd_dx_analytic(x64, gam64, dy64, eps, with_factor=True):
    """dx of the TencentPretrain LayerNorm written out (csrc/norm.hip's formula) in fp64.  with_factor=False: the WRONG form that
    divides by (D - 1) alone, i.e. treats rstd as 1 / std."""
    D = x64.shape[-1]
    mean, std = x64.mean(-1, keepdim=True), x64.std(-1, keepdim=True)
    rstd = 1.0 / (std + eps)
    xh, g = (x64 - mean) * rstd, dy64 * gam64
    den = (D - 1) * (1.0 - eps * rstd) if with_factor else float(D - 1)
    return rstd * (g - g.mean(-1, keepdim=True) - xh * ((g * xh).sum(-1, keepdim=True) / den))


def small_variance_case(D):
    """x = 2e-5 randn with eps = 1e-6: eps * rstd is about 0.05, so the (1 - eps * rstd) factor of the mode-1 backward is 5 % off 1.
    dy = xhat + 0.5 randn: the factor multiplies sum(dy gamma xhat), which random dy would leave at O(1 / sqrt(D)) of the gradient --
    a dy correlated with xhat puts the whole factor into dx."""
    g = _gen(9000 + D)
    rows = 9
    x, gam, bet = 2e-5 * _rand(g, rows, D), 1.0 + 0.1 * _rand(g, D), _rand(g, D)
    x64 = x.double()
    xh = (x64 - x64.mean(-1, keepdim=True)) / (x64.std(-1, keepdim=True) + SMALL_VAR_EPS)
    dy = (xh + 0.5 * _rand(g, rows, D).double()).float()
    dx, dgam, dbet = ln_bwd_ref(x, gam, bet, dy, 1, SMALL_VAR_EPS)
    wrong = tp_bwd_dx_analytic(x64, gam.double(), dy.double(), SMALL_VAR_EPS, with_factor=False)
    return dict(x=x, gam=gam, bet=bet, dy=dy, dx=dx, dgam=dgam, dbet=dbet, wrong=wrong, rows=rows,
                eps_rstd=SMALL_VAR_EPS / (x64.std(-1) + SMALL_VAR_EPS))


# ---------------------------------------------------------------------------------------------------------------- PPO
def _clog(t):
    return torch.log(t.clamp(min=1e-20))


def ppo_ref(scores, value, old_scores, rewards, old_value, next_state, kl_w, ent_w, clip, rank_len=2, margin=0.01, adv_eps=-0.1):
    """finetune/ppo.py:539-584 in the dtype of its inputs, from O.rank_loss and O.clipped_value_loss, with the three constants the
    reference hard-codes as parameters: the target order is the last rank_len entries of next_state, reversed where adv < adv_eps.
    Returns (loss, value_loss, extras); extras also holds what the guard band and the branch-coverage assertions look at."""
    B = scores.shape[0]
    old_p, new_p = old_scores.softmax(dim=-1), scores.softmax(dim=-1)
    zero = torch.zeros(B, dtype=scores.dtype)
    kl = (old_p * (_clog(old_p) - _clog(new_p))).sum(dim=-1) if kl_w > 0 else zero
    ent = -(new_p * _clog(new_p)).sum(dim=-1) if ent_w > 0 else zero
    r = rewards - kl * kl_w
    adv = r - old_value
    tail = next_state[:, next_state.shape[1] - rank_len:]
    order = torch.where((adv >= adv_eps).unsqueeze(1), tail, tail.flip(dims=[-1]))
    rl = O.rank_loss(scores, order, margin)
    loss = (rl * adv.abs() - ent_w * ent).mean()
    vloss = O.clipped_value_loss(value, r.detach(), old_value, clip)
    s = torch.gather(scores.detach(), 1, order)
    iu = torch.triu_indices(rank_len, rank_len, offset=1)
    hgap = margin - (s[:, iu[0]] - s[:, iu[1]])                       # [B, pairs]: one entry per a < b of the target order
    extras = dict(kl=kl, entropy=ent, rewards=r, advantages=adv, rank_loss=rl, order=order, hgap=hgap,
                  count=(hgap > 0).sum().to(scores.dtype), dlt=(value - old_value).detach())
    return loss, vloss, extras


PPO_KW = dict(kl_w=0.001, ent_w=0.001, clip=0.5, margin=0.01, adv_eps=-0.1)
GUARD = 1e-4


def ppo_inputs(B, T, seed):
    """the input family of test_ppo_loss_and_gradients; next_state = [0, 1 | a permutation of the T tags]"""
    g = _gen(seed)
    scores = _rand(g, B, T, scale=0.3)
    old = scores + _rand(g, B, T, scale=0.05)
    rewards, old_value = _rand(g, B, scale=0.2), _rand(g, B, scale=0.2)
    value = old_value + _rand(g, B, scale=0.6)        # some |v - old| exceed the clip
    state = torch.stack([torch.randperm(T, generator=g) for _ in range(B)])
    nxt = torch.cat([torch.arange(2).unsqueeze(0).repeat(B, 1), state], dim=1)
    return dict(scores=scores, old=old, rewards=rewards, old_value=old_value, value=value, nxt=nxt, B=B, T=T)


def ppo_separated_inputs(B, T, seed, adv_eps=-0.1):
    """scores one apart along the target order (best first), so that no hinge margin - (s_a - s_b) is positive.  The order an item
    uses depends on its advantage, which moves with kl_w * KL (about 1e-6 here): the items are kept 0.02 away from adv_eps."""
    c = ppo_inputs(B, T, seed)
    raw = c["rewards"] - c["old_value"] - adv_eps
    c["rewards"] = c["rewards"] + torch.where(raw.abs() < 0.02, torch.where(raw >= 0, 0.04, -0.04), 0.0)
    keep = (c["rewards"] - c["old_value"]) >= adv_eps
    tail = c["nxt"][:, 2:]
    order = torch.where(keep.unsqueeze(1), tail, tail.flip(dims=[-1]))
    ranks = -torch.arange(T, dtype=torch.float32).repeat(B, 1)                          # 0, -1, -2, ... along the order
    c["scores"] = torch.zeros(B, T).scatter_(1, order, ranks) + c["scores"] * 0.1       # +- 0.1: the gaps stay >= 0.8
    c["old"] = c["scores"] + _rand(_gen(seed + 1), B, T, scale=0.05)
    return c


PROB_FLOOR = 1e-20                 # the reference's log(t.clamp(min=1e-20)), finetune/ppo.py:431-432


def ppo_peaked_inputs(B, T, seed):
    """scores of scale 40, old scores 2 away: softmax probabilities below the 1e-20 floor of the reference's clamped log in some items
    (the kernel's KL then follows the clamped form term by term) and above it in others (its cancellation-free form)"""
    c = ppo_inputs(B, T, seed)
    g = _gen(seed + 7)
    c["scores"] = _rand(g, B, T, scale=40.0)
    c["old"] = c["scores"] + _rand(g, B, T, scale=2.0)
    return c


def ppo_min_prob(c):
    """per item, the smallest softmax probability of the new and the old scores (fp64)"""
    return torch.minimum(c["scores"].double().softmax(-1).amin(-1), c["old"].double().softmax(-1).amin(-1))


def ppo_reference(c, rank_len=2, sl=None, **kw):
    """fp64 reference of a case (optionally of the items sl) -> dict with loss, vloss, dscores, dvalue and the extras"""
    kw = {**PPO_KW, **kw}
    pick = (lambda t: t) if sl is None else (lambda t: t[sl])
    st = pick(c["scores"]).double().clone().requires_grad_(True)
    vt = pick(c["value"]).double().clone().requires_grad_(True)
    loss, vloss, ex = ppo_ref(st, vt, pick(c["old"]).double(), pick(c["rewards"]).double(), pick(c["old_value"]).double(),
                              pick(c["nxt"]), kw["kl_w"], kw["ent_w"], kw["clip"], rank_len, kw["margin"], kw["adv_eps"])
    if loss.requires_grad:
        loss.backward()
    vloss.backward()
    ds = st.grad if st.grad is not None else torch.zeros_like(st)
    return dict(loss=loss.detach(), vloss=vloss.detach(), ds=ds, dv=vt.grad, clip=kw["clip"], adv_eps=kw["adv_eps"],
                **{k: v.detach() for k, v in ex.items()})


def ppo_guard_violations(ref):
    """items of the fp64 reference within GUARD of a threshold the kernel decides in fp32: adv >= adv_eps, hgap > 0, |dlt| <= clip
    (and adv's own sign, which the kernel's d|A| uses)"""
    return int(((ref["advantages"] - ref["adv_eps"]).abs() <= GUARD).sum() + (ref["advantages"].abs() <= GUARD).sum()
               + (ref["hgap"].abs() <= GUARD).sum() + ((ref["dlt"].abs() - ref["clip"]).abs() <= GUARD).sum())


def ppo_branch_coverage(ref, hinges=True):
    adv, dlt, hg = ref["advantages"], ref["dlt"].abs(), ref["hgap"]
    assert (adv >= ref["adv_eps"]).any() and (adv < ref["adv_eps"]).any(), "both target orders"
    assert (dlt <= ref["clip"]).any() and (dlt > ref["clip"]).any(), "inside and outside the value clip"
    if hinges:
        assert (hg > 0).any() and (hg <= 0).any(), "positive and non-positive hinge gaps"


# seeds with no item inside the guard band, found by scanning seeds 1, 2, ... on the CPU; tests/test_reductions_cpu.py re-checks each
_PPO_SEEDS = {(65, 2, 2): 2, (1000, 2, 2): 3, (1024, 2, 2): 2, (130, 1, 1): 2, (65, 2, 1): 2, (130, 3, 3): 2, (130, 5, 5): 2}   # else 1
_PPO_BTR = [(B, 2, 2) for B in (1, 63, 64, 65, 128, 129, 1000, 1024)]
_PPO_BTR += [(B, T, rl) for T in (1, 2, 3, 5, 8) for rl in sorted({1, min(2, T), T}) for B in (65, 130) if (B, T, rl) not in _PPO_BTR]
PPO_CASES = [(B, T, rl, _PPO_SEEDS.get((B, T, rl), 1)) for B, T, rl in _PPO_BTR]          # (B, T, rank_len, seed)
PPO_WEIGHT_CASES = [(0.0, 0.001), (0.001, 0.0), (0.0, 0.0)]           # (kl_w, ent_w) at B = 130, T = 3, rank_len = 3
PPO_WEIGHT_SEED = 2
PPO_NOHINGE_SEED = 1
PPO_TWO_PASS_SEED = 1
PPO_PEAKED_SEED = 3


# ----------------------------------------------------------------------------------------------------------- SmoothL1
SMOOTH_L1_SEEDS = {(64, 0.3): 2, (5000, 1.0): 2}         # (n, beta) -> seed with no |d| within GUARD of beta (else 1)


def smooth_l1_case(n, beta):
    g = _gen(SMOOTH_L1_SEEDS.get((n, beta), 1) * 1000 + n)
    pred, tgt = _rand(g, n), torch.randint(0, 3, (n,), generator=g).float()
    pt = pred.double().requires_grad_(True)
    ref = O.smooth_l1(pt, tgt.double(), beta)
    ref.backward()
    return dict(pred=pred, tgt=tgt, loss=ref.detach(), dp=pt.grad, d=(pred.double() - tgt.double()).abs())


# ======================================================================================================================
# GPU side
# ======================================================================================================================
@pytest.fixture(scope="module")
def ops(dev):
    from lr2ppo_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def lib(dev):
    from lr2ppo_amd import _native
    return _native.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    """2-byte storage (int16 planes buffer / bf16 tensor) as int16 on the CPU"""
    return t.view(torch.int16).cpu()


def _ln_fwd(ops, dev, x, gam, bet, mode, rows, D, eps=None, **kw):
    out = torch.full((rows, D), NAN, device=dev)
    mean, rstd = torch.full((rows,), NAN, device=dev), torch.full((rows,), NAN, device=dev)
    ops.layernorm_fwd(x.to(dev), gam.to(dev), bet.to(dev), out, mean, rstd, rows=rows, D=D, eps=LN_EPS[mode] if eps is None else eps,
                      mode=mode, **kw)
    return out, mean, rstd


# --------------------------------------------------------------------------------------------------- 1. LayerNorm fwd
@pytest.mark.parametrize("mode", [0, 1], ids=["mode0", "mode1"])
@pytest.mark.parametrize("D", [4, 8, 100, 252, 256, 260, 1020, 1024], ids=lambda d: f"D{d}")
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 9], ids=lambda r: f"rows{r}")
def test_layernorm_fwd_out_mean_rstd(ops, dev, rows, D, mode):
    """D off the 64-lane x float4 pitch (lanes with no column, a last float4 row per lane that only some lanes own), rows off the
    4-rows-per-workgroup pitch; rstd is asserted as well as mean (mode 1 divides by D - 1 and adds eps OUTSIDE the root)."""
    c = ln_case(rows, D, 100 * rows + D + mode, x_scale=2.0, x_shift=0.5)
    out, mean, rstd = _ln_fwd(ops, dev, c["x"], c["gam"], c["bet"], mode, rows, D)
    x64 = c["x"].double()
    _close(out, ln_ref(x64, c["gam"].double(), c["bet"].double(), mode), 1e-5, 1e-5, "out")
    ref_mean, ref_rstd = ln_stats(x64, mode)
    _close(mean, ref_mean, 1e-6, 1e-6, "mean")
    _close(rstd, ref_rstd, 1e-6, 1e-5, "rstd")


@pytest.mark.parametrize("mode", [0, 1], ids=["mode0", "mode1"])
@pytest.mark.parametrize("D", [4, 100, 1024], ids=lambda d: f"D{d}")
def test_layernorm_fwd_four_output_forms(ops, dev, D, mode):
    """fp32, planes, ONE bf16 plane, fp32 + planes: the same numbers in every form -- the hi plane and the single plane are
    out.bfloat16() bit for bit, and hi + lo is out to 2^-16 relative (bf16 twice: 2^-9 x 2^-9, with two bits to spare)."""
    rows = 5
    c = ln_case(rows, D, 300 + D + mode, x_scale=2.0, x_shift=0.5)
    xd, gd, bd = c["x"].to(dev), c["gam"].to(dev), c["bet"].to(dev)
    kw = dict(rows=rows, D=D, eps=LN_EPS[mode], mode=mode)
    out = torch.full((rows, D), NAN, device=dev)
    ops.layernorm_fwd(xd, gd, bd, out, **kw)
    _close(out, ln_ref(c["x"].double(), c["gam"].double(), c["bet"].double(), mode), 1e-5, 1e-5, "fp32 form")
    pl = ops.Planes.empty(rows, D, dev)
    ops.layernorm_fwd(xd, gd, bd, None, out_planes=pl, **kw)
    one = torch.full((rows, D), NAN, device=dev, dtype=torch.bfloat16)
    ops.layernorm_fwd(xd, gd, bd, None, out_plane=one, **kw)
    out2, pl2 = torch.full((rows, D), NAN, device=dev), ops.Planes.empty(rows, D, dev)
    ops.layernorm_fwd(xd, gd, bd, out2, out_planes=pl2, **kw)
    n = rows * D
    want_hi = _bits(out.bfloat16()).view(-1)
    assert torch.equal(_bits(pl.buf[:n]), want_hi), "hi plane != out.bfloat16()"
    assert torch.equal(_bits(one).view(-1), want_hi), "single plane != out.bfloat16()"
    err = (pl.to_float().double() - out.double()).abs()
    assert bool((err <= 2.0 ** -16 * out.double().abs()).all()), f"hi + lo vs out: {(err / out.double().abs()).max().item():.3e}"
    assert torch.equal(out2, out), "fp32 + planes: the fp32 half differs from the fp32-only call"
    assert torch.equal(_bits(pl2.buf), _bits(pl.buf)), "fp32 + planes: the planes differ from the planes-only call"


@pytest.mark.parametrize("mode", [0, 1], ids=["mode0", "mode1"])
@pytest.mark.parametrize("D", [8, 100], ids=lambda d: f"D{d}")
def test_layernorm_fwd_group_mapping_all_destinations(ops, dev, D, mode):
    """group = L, group_stride = (L + extra) D into the fp32, planes and one-plane destinations: the gaps keep a canary bit for bit,
    the mapped rows are the unmapped call's rows bit for bit."""
    n, L, extra = 3, 5, 2
    rows, W = n * L, (L + extra) * D
    c = ln_case(rows, D, 400 + D + mode)
    xd, gd, bd = c["x"].to(dev), c["gam"].to(dev), c["bet"].to(dev)
    kw = dict(rows=rows, D=D, eps=LN_EPS[mode], mode=mode)
    gkw = dict(group=L, group_stride=W, **kw)
    CAN_F, CAN_H = -77.25, 0x1234
    # unmapped
    out = torch.full((rows, D), NAN, device=dev)
    pl = ops.Planes.empty(rows, D, dev)
    ops.layernorm_fwd(xd, gd, bd, out, out_planes=pl, **kw)
    one = torch.zeros(rows, D, device=dev, dtype=torch.bfloat16)
    ops.layernorm_fwd(xd, gd, bd, None, out_plane=one, **kw)
    _close(out, ln_ref(c["x"].double(), c["gam"].double(), c["bet"].double(), mode), 1e-5, 1e-5, "unmapped out")
    # mapped
    flat = torch.full((n, W), CAN_F, device=dev)
    ops.layernorm_fwd(xd, gd, bd, flat, **gkw)
    assert torch.equal(flat[:, :L * D].reshape(rows, D), out), "fp32: mapped rows"
    assert bool((flat[:, L * D:] == CAN_F).all()), "fp32: the gap was written"
    fpl = ops.Planes(torch.full((2 * n * W,), CAN_H, dtype=torch.int16, device=dev), n, W)
    ops.layernorm_fwd(xd, gd, bd, None, out_planes=fpl, **gkw)
    fone = torch.full((n, W), CAN_H, dtype=torch.int16, device=dev)
    ops.layernorm_fwd(xd, gd, bd, None, out_plane=fone, **gkw)
    hi, lo = fpl.buf[:n * W].view(n, W), fpl.buf[fpl.lo_off:fpl.lo_off + n * W].view(n, W)
    for name, got, want in (("hi plane", hi, pl.buf[:rows * D]), ("lo plane", lo, pl.buf[pl.lo_off:pl.lo_off + rows * D]),
                            ("one plane", fone, one.view(torch.int16))):
        assert torch.equal(_bits(got[:, :L * D].reshape(rows, D)), _bits(want).view(rows, D)), f"{name}: mapped rows"
        assert bool((got[:, L * D:] == CAN_H).all()), f"{name}: the gap was written"


@pytest.mark.parametrize("mode", [0, 1], ids=["mode0", "mode1"])
@pytest.mark.parametrize("D", [4, 100, 1024], ids=lambda d: f"D{d}")
def test_layernorm_fwd_constant_rows(ops, dev, D, mode):
    """Rows of one repeated value (an all-zero row among them).  Every partial sum k * c is exact (c has 7 significant bits, k <= 1024),
    so mean == c exactly, x - mean == 0 and the output is beta exactly; rstd is 1 / sqrtf(eps) (mode 0) or 1 / eps (mode 1): finite.
    The mode-1 BACKWARD of a constant row is 0 / 0 in the reference's own autograd (d std / dx at std = 0): out of scope, not asserted."""
    consts = torch.tensor([0.0, 1.5, -3.0, 1000.0, 0.625])
    rows = consts.numel()
    g = _gen(500 + D)
    x, gam, bet = consts[:, None].repeat(1, D), _rand(g, D), _rand(g, D)
    out, mean, rstd = _ln_fwd(ops, dev, x, gam, bet, mode, rows, D)
    assert torch.equal(out.cpu(), bet[None, :].repeat(rows, 1)), "constant rows must give beta exactly"
    assert torch.equal(mean.cpu(), consts), "mean of a constant row"
    assert bool(torch.isfinite(rstd).all())
    eps32 = np.float32(LN_EPS[mode])
    want = np.float32(1.0) / np.sqrt(eps32) if mode == 0 else np.float32(1.0) / eps32
    assert np.all(np.abs(rstd.cpu().numpy().astype(np.float64) - np.float64(want)) <= np.spacing(want)), (rstd, want)


@pytest.mark.parametrize("mode", [0, 1], ids=["mode0", "mode1"])
@pytest.mark.parametrize("D", [768, 100], ids=lambda d: f"D{d}")
def test_layernorm_fwd_offset_rows(ops, dev, D, mode):
    """x = 8 + 0.05 randn.  The gate, derived: out = (x - mean) rstd gamma + beta, and x - mean is exact here (x and mean agree to
    1 %: Sterbenz), so an error d in the mean moves out by d rstd |gamma| and the variance only at second order.  The kernel's mean is
    ONE fp32 sum of D terms -- per lane a chain of 4 ceil(D / 256) additions, then 6 butterfly levels -- divided by D.  Each addition
    rounds by at most half an ulp of a partial sum <= the total, so d <= (4 ceil(D / 256) + 6 + 1) / 2 ulp: 9.5 ulp at D = 768,
    5.5 at D = 100, and a random walk of those roundings stays near 1 ulp.  The gate allows k ulp32(|mean|) rstd |gamma| on top of
    the base 1e-5 / 1e-5 with k = log2(D) + 2 (11.6 and 8.6): the depth of a pairwise sum of D terms plus the division and the mean's
    own representation.  With rstd about 20 and ulp32(8) = 2^-20 that is 2e-4 |gamma|, twenty times the base gate -- which is why the
    base gate alone would be wrong for such rows, and why a gate read off the kernel's output would be too.  A plain fp32 torch
    evaluation of the reference formula is held to the same gate first, on the CPU."""
    c = offset_rows_case(D, mode)
    cpu32 = ln_ref(c["x"], c["gam"], c["bet"], mode)
    _within(cpu32, c["ref"], c["bound"], "fp32 torch on the CPU")
    out, mean, rstd = _ln_fwd(ops, dev, c["x"], c["gam"], c["bet"], mode, c["rows"], D)
    _within(out, c["ref"], c["bound"], "kernel")
    _close(mean, c["mean"], 0.0, (math.log2(D) + 2) * 2.0 ** -23, "mean")       # k ulp, relative (ulp32(m) <= 2^-23 m)
    _close(rstd, c["rstd"], 1e-6, 1e-5, "rstd")


# --------------------------------------------------------------------------------------------------- 2. LayerNorm bwd
def _ln_bwd(ops, dev, c, mode, rows, D, *, eps=None, dx=True, planes=False, rg=False, drop=None, adjacent=False, dy_dev=None,
            group=0, group_stride=0, nblocks=None):
    """forward (for mean / rstd) + backward through ops.layernorm_bwd -> dict(dx, dxm, dgam, dbet)"""
    eps = LN_EPS[mode] if eps is None else eps
    xd, gd = c["x"].to(dev), c["gam"].to(dev)
    _, mean, rstd = _ln_fwd(ops, dev, c["x"], c["gam"], c["bet"], mode, rows, D, eps=eps)
    dxt = torch.full((rows, D), NAN, device=dev) if dx else None
    dxm = ops.Planes.empty(rows, D, dev) if planes else None
    if dxm is not None:
        dxm.buf.fill_(0x7FC0)                                     # bf16 NaN: every element must be written
    if adjacent:
        flat = torch.full((2 * D,), NAN, device=dev)
        dgam, dbet = flat[:D], flat[D:]
    else:
        dgam, dbet = torch.full((D,), NAN, device=dev), torch.full((D,), NAN, device=dev)
    nb = ops.LN_BWD_BLOCKS if nblocks is None else nblocks
    rgd = c["rg"].to(dev) if rg is True else (None if rg is False else rg)         # True: the case's; a tensor: that one
    partials = torch.full((nb * 2 * D,), NAN, device=dev)
    ops.layernorm_bwd(c["dy"].to(dev) if dy_dev is None else dy_dev, xd, gd, mean, rstd, dxt, partials, dgam, dbet, rows=rows, D=D,
                      group=group, group_stride=group_stride, resid_grad=rgd,
                      dx_planes=dxm, drop=drop, nblocks=nb, mode=mode, eps=eps)
    return dict(dx=dxt, dxm=dxm, dgam=dgam, dbet=dbet)


@pytest.mark.parametrize("mode", [0, 1], ids=["mode0", "mode1"])
@pytest.mark.parametrize("D", [4, 100, 256, 1024], ids=lambda d: f"D{d}")
@pytest.mark.parametrize("rows", [1, 3, 5, 50], ids=lambda r: f"rows{r}")
def test_layernorm_bwd_both_modes_and_gradient_layouts(ops, dev, rows, D, mode):
    """Both semantics against fp64 autograd, at rows / D off every pitch; and the two destination layouts of ops.layernorm_bwd --
    [dgamma | dbeta] adjacent in one buffer (one finishing launch over 2 D columns) and separate tensors (two launches with
    ld = 2 D) -- give the same bits."""
    c = ln_case(rows, D, 600 + 10 * rows + D + mode)
    dx, dgam, dbet = ln_bwd_ref(c["x"], c["gam"], c["bet"], c["dy"], mode)
    a = _ln_bwd(ops, dev, c, mode, rows, D, rg=True)
    _close(a["dx"], dx + c["rg"].double(), 2e-5, 2e-5, "dx")
    _close(a["dgam"], dgam, 1e-4, 1e-4, "dgamma")
    _close(a["dbet"], dbet, 1e-4, 1e-4, "dbeta")
    b = _ln_bwd(ops, dev, c, mode, rows, D, rg=True, adjacent=True)
    assert torch.equal(a["dgam"], b["dgam"]) and torch.equal(a["dbet"], b["dbet"]), "adjacent vs separate gradient buffers"
    assert torch.equal(a["dx"], b["dx"])


@pytest.mark.parametrize("D", [64, 768], ids=lambda d: f"D{d}")
def test_layernorm_bwd_mode1_small_variance_sees_the_eps_factor(ops, dev, D):
    """Mode 1 with x = 2e-5 randn and eps = 1e-6: rstd = 1 / (std + eps) is 5 % below 1 / std, and the backward's
    c2 = sum(g xhat) / ((D - 1)(1 - eps rstd)) carries that 5 % (at the product's std of about 1 the factor is 1 - 1e-6, invisible to
    every other test).  Gate: 1e-4 of the row's max |dx_ref|.  Derivation: nothing here cancels -- x - mean keeps the relative
    precision of x (2^-24, the values are small, not close), 1 - eps rstd is 0.95, g - c1 - xhat c2 is 5 % of its terms at worst (dy
    is xhat + 0.5 randn, so the xhat part cancels to eps rstd of itself: 2^-24 / 0.05 = 1.2e-6 relative) -- so the fp32 result is
    good to a few 1e-6 of the row's scale, and 1e-4 leaves the room the D-term sums need.  The same test proves on the CPU that the
    case can see the factor: the wrong reference that divides by (D - 1) alone is more than 100 gates away from the right one in
    every row."""
    c = small_variance_case(D)
    rows = c["rows"]
    assert bool(((c["eps_rstd"] > 0.03) & (c["eps_rstd"] < 0.07)).all())
    row_max = c["dx"].abs().amax(-1, keepdim=True)
    gate = SMALL_VAR_GATE * row_max
    right = tp_bwd_dx_analytic(c["x"].double(), c["gam"].double(), c["dy"].double(), SMALL_VAR_EPS)
    assert bool(((right - c["dx"]).abs() <= 1e-9 * row_max).all()), "the written-out formula is autograd's"
    assert bool(((c["wrong"] - c["dx"]).abs().amax(-1, keepdim=True) > 100 * gate).all()), "the case cannot see the factor"
    got = _ln_bwd(ops, dev, c, 1, rows, D, eps=SMALL_VAR_EPS)
    _within(got["dx"], c["dx"], gate.expand(rows, D), "dx")
    _close(got["dgam"], c["dgam"], 1e-4, 1e-4, "dgamma")
    _close(got["dbet"], c["dbet"], 1e-4, 1e-4, "dbeta")


@pytest.mark.parametrize("mode", [0, 1], ids=["mode0", "mode1"])
def test_layernorm_bwd_group_stride_on_dy(ops, dev, mode):
    """dy read through (group, group_stride) from a padded concat layout whose gaps hold NaN: the same bits as the contiguous-dy
    call (and so no gap element was read)."""
    n, L, extra, D = 3, 5, 2, 100
    rows, W = n * L, (L + extra) * D
    c = ln_case(rows, D, 700 + mode)
    base = _ln_bwd(ops, dev, c, mode, rows, D, rg=True)
    padded = torch.full((n, L + extra, D), NAN)
    padded[:, :L] = c["dy"].view(n, L, D)
    got = _ln_bwd(ops, dev, c, mode, rows, D, rg=True, dy_dev=padded.to(dev), group=L, group_stride=W)
    for k in ("dx", "dgam", "dbet"):
        assert torch.equal(got[k], base[k]), k
    dx, dgam, _ = ln_bwd_ref(c["x"], c["gam"], c["bet"], c["dy"], mode)
    _close(got["dx"], dx + c["rg"].double(), 2e-5, 2e-5, "dx")
    _close(got["dgam"], dgam, 1e-4, 1e-4, "dgamma")


@pytest.mark.parametrize("mode", [0, 1], ids=["mode0", "mode1"])
def test_layernorm_bwd_output_forms_and_optional_residual(ops, dev, mode):
    """dx only, dx_planes only (dx=None), both; resid_grad=None against a zero tensor; resid_grad with planes only."""
    rows, D = 9, 100
    c = ln_case(rows, D, 710 + mode)
    dx, _, _ = ln_bwd_ref(c["x"], c["gam"], c["bet"], c["dy"], mode)
    both = _ln_bwd(ops, dev, c, mode, rows, D, planes=True)
    only_dx = _ln_bwd(ops, dev, c, mode, rows, D)
    only_pl = _ln_bwd(ops, dev, c, mode, rows, D, dx=False, planes=True)
    _close(both["dx"], dx, 2e-5, 2e-5, "dx")
    _close(both["dxm"].to_float(), dx, 1e-4, 3e-5, "dx planes")
    assert torch.equal(only_dx["dx"], both["dx"])
    assert torch.equal(_bits(only_pl["dxm"].buf), _bits(both["dxm"].buf))
    for k in ("dgam", "dbet"):
        assert torch.equal(only_dx[k], both[k]) and torch.equal(only_pl[k], both[k]), k
    # no residual == a residual of zeros (x + 0 keeps every bit but the sign of a zero, which torch.equal does not see)
    zero = _ln_bwd(ops, dev, c, mode, rows, D, planes=True, rg=torch.zeros(rows, D, device=dev))
    assert torch.equal(zero["dx"], both["dx"])
    assert torch.equal(zero["dxm"].buf.view(torch.bfloat16), both["dxm"].buf.view(torch.bfloat16))
    # a residual with the planes output alone
    rg_pl = _ln_bwd(ops, dev, c, mode, rows, D, dx=False, planes=True, rg=True)
    rg_both = _ln_bwd(ops, dev, c, mode, rows, D, planes=True, rg=True)
    _close(rg_pl["dxm"].to_float(), dx + c["rg"].double(), 1e-4, 3e-5, "dx planes with residual")
    assert torch.equal(_bits(rg_pl["dxm"].buf), _bits(rg_both["dxm"].buf))
    _close(rg_both["dx"], dx + c["rg"].double(), 2e-5, 2e-5, "dx with residual")


@pytest.mark.parametrize("mode", [0, 1], ids=["mode0", "mode1"])
def test_layernorm_bwd_dropout_on_the_planes_output(ops, dev, mode):
    """The keep set is O.dropout_keep_mask; dropped elements are 0 in BOTH planes; kept values are split(dx / (1 - p)) -- bit for bit
    at p = 0.5 (the scale 2 is exact, so dx / (1 - p) has one fp32 value), and at the existing planes gate against fp64 at p = 0.1.
    A Drop carrying seed_dev = s with host seed t is the host-only Drop with seed s + t."""
    rows, D, seed, site = 9, 100, 1234, 6
    c = ln_case(rows, D, 720 + mode)
    dx, _, _ = ln_bwd_ref(c["x"], c["gam"], c["bet"], c["dy"], mode)
    ref = dx + c["rg"].double()
    n = rows * D
    for p in (0.5, 0.1):
        got = _ln_bwd(ops, dev, c, mode, rows, D, planes=True, rg=True, drop=ops.Drop(p, seed, site))
        keep = torch.from_numpy(O.dropout_keep_mask(seed, site, n, p)).view(rows, D)
        assert 0.6 * (1 - p) < keep.float().mean() < min(1.0, 1.4 * (1 - p))
        _close(got["dx"], ref, 2e-5, 2e-5, "dx (never dropped)")
        hi, lo = _bits(got["dxm"].buf[:n]).view(rows, D), _bits(got["dxm"].buf[got["dxm"].lo_off:got["dxm"].lo_off + n]).view(rows, D)
        assert bool((hi[~keep] == 0).all()) and bool((lo[~keep] == 0).all()), "dropped elements must be 0 in both planes"
        _close(got["dxm"].to_float(), ref * keep.double() / (1 - p), 1e-4, 3e-5, f"masked dx planes p={p}")
        if p == 0.5:
            m = got["dx"].cpu() * 2.0
            want_hi = m.bfloat16()
            want_lo = (m - want_hi.float()).bfloat16()
            assert torch.equal(hi[keep], want_hi.view(torch.int16)[keep]) and torch.equal(lo[keep], want_lo.view(torch.int16)[keep])
    s, t = 1000, 234
    sd = torch.tensor([s], dtype=torch.int64, device=dev)
    a = _ln_bwd(ops, dev, c, mode, rows, D, planes=True, rg=True, drop=ops.Drop(0.5, t, site, seed_dev=sd))
    b = _ln_bwd(ops, dev, c, mode, rows, D, planes=True, rg=True, drop=ops.Drop(0.5, s + t, site))
    assert torch.equal(_bits(a["dxm"].buf), _bits(b["dxm"].buf)), "seed_dev + seed"
    assert not torch.equal(_bits(a["dxm"].buf), _bits(_ln_bwd(ops, dev, c, mode, rows, D, planes=True, rg=True,
                                                               drop=ops.Drop(0.5, t, site))["dxm"].buf)), "seed_dev was ignored"


_LN_NB_REF = {}


def _ln_nblocks_case(rows):
    """integer dy in [-8, 8] (|column sums| <= 8 x 2049 < 2^24: dbeta is exact in any order), shared by the nblocks cases of a rows"""
    if rows not in _LN_NB_REF:
        D = 64
        g = _gen(800 + rows)
        c = dict(x=_rand(g, rows, D), gam=_rand(g, D), bet=_rand(g, D), dy=_ints(g, -8, 8, rows, D))
        _, c["dgam"], c["dbet"] = ln_bwd_ref(c["x"], c["gam"], c["bet"], c["dy"], 0)
        c["colsum"] = c["dy"].double().sum(0)
        _LN_NB_REF[rows] = c
    return _LN_NB_REF[rows]


@pytest.mark.parametrize("nblocks", [1, 3, 29, 32, 33, 64, 512], ids=lambda n: f"nblocks{n}")
@pytest.mark.parametrize("rows", [1, 50, 129, 2049], ids=lambda r: f"rows{r}")
def test_layernorm_bwd_nblocks(ops, lib, dev, rows, nblocks):
    """The workgroup count given as is (ops.layernorm_bwd clips it to ceil(rows / 4); the library does not): grid-stride over the rows
    (rows > 4 nblocks) and idle workgroups (4 nblocks > rows), which must still write their partial row -- the workspace starts as
    NaN.  dbeta of integer dy is the fp64 column sum bit for bit for every nblocks; dgamma at the existing gate; dx does not depend
    on nblocks."""
    D = 64
    c = _ln_nblocks_case(rows)
    xd, gd, dyd = c["x"].to(dev), c["gam"].to(dev), c["dy"].to(dev)
    _, mean, rstd = _ln_fwd(ops, dev, c["x"], c["gam"], c["bet"], 0, rows, D)
    dx = torch.full((rows, D), NAN, device=dev)
    partials = torch.full((nblocks * 2 * D,), NAN, device=dev)
    out = torch.full((2 * D,), NAN, device=dev)
    assert lib.lr2_layernorm_bwd(dyd.data_ptr(), 0, 0, xd.data_ptr(), gd.data_ptr(), mean.data_ptr(), rstd.data_ptr(), None,
                                 dx.data_ptr(), None, 0, 0.0, 0, 0, None, partials.data_ptr(), nblocks, rows, D, 0, LN_EPS[0],
                                 _stream()) == 0
    assert lib.lr2_colsum_partials_finish(partials.data_ptr(), nblocks, 2 * D, 2 * D, out.data_ptr(), 0, _stream()) == 0
    assert torch.equal(out[D:].cpu().double(), c["colsum"]), "dbeta of integer dy must be exact"
    _close(out[D:], c["dbet"], 0.0, 0.0, "dbeta vs autograd")
    _close(out[:D], c["dgam"], 1e-4, 1e-4, "dgamma")
    base = _ln_bwd(ops, dev, c, 0, rows, D)
    assert torch.equal(dx, base["dx"]), "dx depends on nblocks"
    assert torch.equal(out[D:], base["dbet"])


# ------------------------------------------------------------------------------ 3. column sums and the finishing kernel
@pytest.mark.parametrize("nblocks", [1, 2, 3, 4, 5, 27, 28, 29, 30, 31, 32, 33, 59, 60, 61, 64, 65, 128, 512],
                         ids=lambda n: f"nblocks{n}")
def test_colsum_partials_finish_unroll_edges(lib, dev, nblocks):
    """The 8-deep unrolled loop (b + 28 < nblocks; b += 32, four row slices) and its scalar tail around every edge, cols around the
    64-column workgroup, ld == cols and ld > cols (the pad columns hold NaN), accumulate 0 and 1.  Integer partials in [-64, 64]:
    |sums| <= 512 x 64 + 64, exact in fp32 in any order, so the result is the fp64 sum bit for bit.  out beyond cols and a canary
    after it stay untouched."""
    g = _gen(900 + nblocks)
    CAN = -1234.5
    for cols in (1, 63, 64, 65, 200):
        for ld in (cols, cols + 8):
            part = torch.full((nblocks, ld), NAN)
            part[:, :cols] = _ints(g, -64, 64, nblocks, cols)
            ref = part[:, :cols].double().sum(0)
            pd = part.to(dev)
            for accumulate in (0, 1):
                out = torch.full((cols + 72,), CAN)
                base = _ints(g, -64, 64, cols)
                if accumulate:
                    out[:cols] = base
                od = out.to(dev)
                assert lib.lr2_colsum_partials_finish(pd.data_ptr(), nblocks, cols, ld, od.data_ptr(), accumulate, _stream()) == 0
                got = od.cpu()
                want = ref + base.double() if accumulate else ref
                assert torch.equal(got[:cols].double(), want), (cols, ld, accumulate, (got[:cols].double() - want).abs().max())
                assert bool((got[cols:] == CAN).all()), f"cols={cols} ld={ld}: out beyond cols was written"


def _colsum_inputs(form, ints, ld):
    """[rows, ld] device storage of the values (ints / 256 for fp32 and planes, ints itself for the single plane), the pad columns
    NaN (never read) -> (host tensor, is_planes, lo_off)"""
    rows, cols = ints.shape
    if form == "fp32":
        x = torch.full((rows, ld), NAN)
        x[:, :cols] = ints / 256.0
        return x, 0, 0
    v = ints if form == "plane" else ints / 256.0
    hi = v.bfloat16()
    lo = (v - hi.float()).bfloat16()
    assert torch.equal(hi.float() + lo.float(), v), "the split of the test values must be exact"
    if form == "plane":
        assert torch.equal(hi.float(), v)
    planes = torch.full((2 if form == "planes" else 1, rows, ld), NAN, dtype=torch.bfloat16)
    planes[0, :, :cols] = hi
    if form == "planes":
        planes[1, :, :cols] = lo
    return planes, (1 if form == "planes" else 2), rows * ld


@pytest.mark.parametrize("rows", [1, 127, 128, 129, 300], ids=lambda r: f"rows{r}")
@pytest.mark.parametrize("form", ["fp32", "planes", "plane"])
def test_colsum_three_forms_exact(lib, dev, form, rows):
    """lr2_colsum on fp32, hi / lo planes and ONE bf16 plane (is_planes = 2, which ops.colsum cannot ask for: the library is called
    directly), cols around the 1024-column block, ld == cols and ld > cols, nblocks 1 / 128 / 256 (rows < nblocks included).
    fp32 / planes values are integers in [-2^10, 2^10] / 256 (hi + lo exact, sums < 2^24 / 256), the single plane holds integers in
    [-128, 128]: the result is the fp64 sum bit for bit."""
    g = _gen(1000 + rows)
    CAN = -4321.25
    all_ints = _ints(g, -128, 128, rows, 3072) if form == "plane" else _ints(g, -1024, 1024, rows, 3072)
    for cols in (4, 1020, 1024, 1028, 3072):
        ints = all_ints[:, :cols].contiguous()
        ref = ints.double().sum(0) / (1.0 if form == "plane" else 256.0)
        for ld in (cols, cols + 8):
            x, is_planes, lo_off = _colsum_inputs(form, ints, ld)
            xd = x.to(dev)
            for nblocks in (1, 128, 256):
                partials = torch.full((nblocks * cols,), NAN, device=dev)
                out = torch.full((cols + 16,), CAN, device=dev)
                assert lib.lr2_colsum(xd.data_ptr(), is_planes, lo_off, rows, cols, ld, partials.data_ptr(), nblocks, out.data_ptr(),
                                      _stream()) == 0
                got = out.cpu()
                assert torch.equal(got[:cols].double(), ref), (cols, ld, nblocks, (got[:cols].double() - ref).abs().max())
                assert bool((got[cols:] == CAN).all())


@pytest.mark.parametrize("form", ["fp32", "planes", "plane"])
def test_colsum_three_forms_random(lib, dev, form):
    """One random-data case per form at test_colsum's gate; the reference is the fp64 sum of the values the storage holds."""
    rows, cols, ld = 300, 1028, 1036
    g = _gen(1100)
    v = _rand(g, rows, cols)
    hi = v.bfloat16()
    lo = (v - hi.float()).bfloat16()
    if form == "fp32":
        x, is_planes, ref = torch.full((rows, ld), NAN), 0, v.double().sum(0)
        x[:, :cols] = v
    else:
        x = torch.full((2 if form == "planes" else 1, rows, ld), NAN, dtype=torch.bfloat16)
        x[0, :, :cols] = hi
        is_planes, ref = 2, hi.double().sum(0)
        if form == "planes":
            x[1, :, :cols] = lo
            is_planes, ref = 1, (hi.double() + lo.double()).sum(0)
    xd = x.to(dev)
    partials, out = torch.full((128 * cols,), NAN, device=dev), torch.full((cols,), NAN, device=dev)
    assert lib.lr2_colsum(xd.data_ptr(), is_planes, rows * ld, rows, cols, ld, partials.data_ptr(), 128, out.data_ptr(), _stream()) == 0
    _close(out, ref, 2e-4, 1e-5, form)


# ------------------------------------------------------------------------------------------- 4. PPO loss across waves
def _ppo_run(ops, dev, c, rank_len=2, sl=None, stats_out=None, global_stats=None, world=1, **kw):
    kw = {**PPO_KW, **kw}
    pick = (lambda t: t.to(dev)) if sl is None else (lambda t: t[sl].contiguous().to(dev))
    B = c["B"] if sl is None else sl.stop - sl.start
    T = c["T"]
    scal, per = torch.full((4,), NAN, device=dev), torch.full((4, B), NAN, device=dev)
    ds, dv = torch.full((B, T), NAN, device=dev), torch.full((B,), NAN, device=dev)
    ops.ppo_loss(pick(c["scores"]), pick(c["old"]), pick(c["rewards"]), pick(c["old_value"]), pick(c["value"]), pick(c["nxt"]),
                 scal, per, ds, dv, B=B, T=T, kl_w=kw["kl_w"], ent_w=kw["ent_w"], value_clip=kw["clip"], margin=kw["margin"],
                 adv_eps=kw["adv_eps"], rank_len=rank_len, stats_out=stats_out, global_stats=global_stats, world=world)
    return dict(scal=scal, per=per, ds=ds, dv=dv)


def _ppo_check(got, ref):
    """the gates of test_ppo_loss_and_gradients, plus the positive-hinge count (an integer); every quantity is looked at before the
    first failure is raised, so that a run shows all of them"""
    checks = [("policy loss", got["scal"][0], ref["loss"], 1e-7, 1e-5), ("value loss", got["scal"][1], ref["vloss"], 1e-7, 1e-5),
              ("rank loss", got["scal"][2], ref["rank_loss"], 1e-7, 1e-5), ("positive-hinge count", got["scal"][3], ref["count"], 0.0, 0.0),
              ("kl", got["per"][0], ref["kl"], 1e-7, 1e-4), ("entropy", got["per"][1], ref["entropy"], 1e-6, 1e-5),
              ("rewards", got["per"][2], ref["rewards"], 1e-7, 1e-5), ("advantages", got["per"][3], ref["advantages"], 1e-7, 1e-5),
              ("dscores", got["ds"], ref["ds"], 1e-8, 1e-4), ("dvalue", got["dv"], ref["dv"], 1e-8, 1e-4)]
    failed = []
    for what, g_, r_, atol, rtol in checks:
        try:
            _close(g_, r_, atol, rtol, what)
        except AssertionError as e:
            failed.append(str(e).splitlines()[0])
    assert not failed, "; ".join(failed)


@pytest.mark.parametrize("B,T,rank_len,seed", PPO_CASES, ids=[f"B{B}-T{T}-rank_len{rl}" for B, T, rl, _ in PPO_CASES])
def test_ppo_loss_across_waves(ops, dev, B, T, rank_len, seed):
    """B up to the 1024-thread workgroup (1, 2, 3, 16 waves; a last wave with one item; 1000: a partly filled last wave among 16):
    the cross-wave half of block_sum_1024 feeds R, the count, mean |A|, the entropy and the value loss, all checked against fp64.
    T up to the kernel's 8 with rank_len 1, 2 and T.  The kernel decides adv >= adv_eps, hgap > 0 and |dlt| <= clip in fp32: the
    committed seed leaves no item of the fp64 reference within 1e-4 of a threshold, asserted here over every item."""
    c = ppo_inputs(B, T, seed)
    ref = ppo_reference(c, rank_len)
    assert ppo_guard_violations(ref) == 0, "an item sits inside the guard band: pick another seed"
    if B >= 63:
        ppo_branch_coverage(ref, hinges=rank_len > 1)
    _ppo_check(_ppo_run(ops, dev, c, rank_len), ref)


@pytest.mark.parametrize("kl_w,ent_w", PPO_WEIGHT_CASES, ids=["kl_w0", "ent_w0", "kl_w0-ent_w0"])
def test_ppo_loss_zero_weights(ops, dev, kl_w, ent_w):
    """kl_w = 0 (no KL: r = rewards, d|A| / dscores gone), ent_w = 0, both: the branches the product's 0.001 / 0.001 never takes."""
    c = ppo_inputs(130, 3, PPO_WEIGHT_SEED)
    ref = ppo_reference(c, 3, kl_w=kl_w, ent_w=ent_w)
    assert ppo_guard_violations(ref) == 0
    ppo_branch_coverage(ref)
    got = _ppo_run(ops, dev, c, 3, kl_w=kl_w, ent_w=ent_w)
    _ppo_check(got, ref)
    if kl_w == 0:
        assert bool((got["per"][0] == 0).all())
    if ent_w == 0:
        assert bool((got["per"][1] == 0).all())


@pytest.mark.parametrize("which", ["separated-scores", "rank_len1"])
def test_ppo_loss_no_positive_hinge(ops, dev, which):
    """CNT == 0: R = 0 and invC = 0, never 0 / 0.  Scores one apart along the target order (T = rank_len = 3), and rank_len = 1 (no
    pair at all).  With ent_w = 0 the whole of dscores is the policy part, and that is exactly 0."""
    if which == "rank_len1":
        c, rank_len = ppo_inputs(65, 3, PPO_NOHINGE_SEED), 1
    else:
        c, rank_len = ppo_separated_inputs(65, 3, PPO_NOHINGE_SEED), 3
    ref = ppo_reference(c, rank_len)
    assert ppo_guard_violations(ref) == 0
    assert ref["count"] == 0 and ref["rank_loss"] == 0 and not (ref["hgap"] > 0).any()
    got = _ppo_run(ops, dev, c, rank_len)
    _ppo_check(got, ref)
    assert float(got["scal"][2]) == 0.0 and float(got["scal"][3]) == 0.0
    ref0 = ppo_reference(c, rank_len, ent_w=0.0)
    got0 = _ppo_run(ops, dev, c, rank_len, ent_w=0.0)
    _ppo_check(got0, ref0)
    assert bool((got0["ds"] == 0).all()), "the policy part of dscores must be exactly 0 without a positive hinge"
    assert float(got0["scal"][0]) == 0.0


def test_ppo_loss_kl_on_both_sides_of_the_probability_floor(ops, dev):
    """Items whose smallest probability is below the reference's 1e-20 floor (clamped log) and items above it in one launch: the
    kernel's two KL forms.  No item within a factor 2 of the floor (the kernel picks the form in fp32)."""
    c = ppo_peaked_inputs(65, 3, PPO_PEAKED_SEED)
    pm = ppo_min_prob(c)
    assert (pm < PROB_FLOOR).sum() >= 5 and (pm > PROB_FLOOR).sum() >= 5
    assert not ((pm > 0.5 * PROB_FLOOR) & (pm < 2 * PROB_FLOOR)).any()
    ref = ppo_reference(c, 3)
    assert ppo_guard_violations(ref) == 0
    _ppo_check(_ppo_run(ops, dev, c, 3), ref)


def test_ppo_loss_two_pass_form_in_one_process(ops, dev):
    """The data-parallel form without a second rank: 130 items as two halves of 65.  Pass 1 (stats_out) per half, the two stat
    triples added on the host, pass 2 with global_stats and world = 2: dscores / dvalue of a half are world x the matching slice of
    the single B = 130 launch (the rank AVERAGE of the gradients is the global-batch gradient -- the identity in the kernel's comment),
    R and the count are the single launch's.  Checked against the fp64 reference of the whole batch and against the single launch."""
    B, T, rank_len = 130, 2, 2
    c = ppo_inputs(B, T, PPO_TWO_PASS_SEED)
    ref = ppo_reference(c, rank_len)
    assert ppo_guard_violations(ref) == 0
    ppo_branch_coverage(ref)
    single = _ppo_run(ops, dev, c, rank_len)
    _ppo_check(single, ref)
    halves = [slice(0, 65), slice(65, 130)]
    stats = []
    for sl in halves:
        st = torch.full((3,), NAN, device=dev)
        _ppo_run(ops, dev, c, rank_len, sl=sl, stats_out=st)
        stats.append(st.cpu())
    _close(stats[0][0] + stats[1][0], (ref["hgap"].clamp(min=0)).sum(), 1e-7, 1e-5, "hinge sum")
    assert float(stats[0][1] + stats[1][1]) == float(ref["count"])
    _close(stats[0][2] + stats[1][2], ref["advantages"].abs().sum(), 1e-7, 1e-5, "sum |A|")
    glob = (stats[0] + stats[1]).to(dev)
    for sl in halves:
        got = _ppo_run(ops, dev, c, rank_len, sl=sl, global_stats=glob, world=2)
        _close(got["ds"], 2.0 * ref["ds"][sl], 1e-8, 1e-4, "dscores vs fp64")
        _close(got["dv"], 2.0 * ref["dv"][sl], 1e-8, 1e-4, "dvalue vs fp64")
        _close(got["ds"], 2.0 * single["ds"][sl].double(), 1e-8, 1e-4, "dscores vs the single launch")
        _close(got["dv"], 2.0 * single["dv"][sl].double(), 1e-8, 1e-4, "dvalue vs the single launch")
        _close(got["scal"][2], single["scal"][2].double(), 1e-7, 1e-5, "R")
        _close(got["scal"][2], ref["rank_loss"], 1e-7, 1e-5, "R vs fp64")
        assert float(got["scal"][3]) == float(single["scal"][3]) == float(ref["count"])
        _close(got["per"][0], ref["kl"][sl], 1e-7, 1e-4, "kl")
        _close(got["per"][1], ref["entropy"][sl], 1e-6, 1e-5, "entropy")
        _close(got["per"][2], ref["rewards"][sl], 1e-7, 1e-5, "rewards")
        _close(got["per"][3], ref["advantages"][sl], 1e-7, 1e-5, "advantages")


# ----------------------------------------------------------------------------- 5. the other block and row reductions
@pytest.mark.parametrize("with_dpred", [True, False], ids=["dpred", "dpredNone"])
@pytest.mark.parametrize("beta", [0.3, 1.0], ids=lambda b: f"beta{b}")
@pytest.mark.parametrize("n", [1, 64, 1023, 1024, 1025, 5000], ids=lambda n: f"n{n}")
def test_smooth_l1_block_stride(ops, dev, n, beta, with_dpred):
    """The 1024-thread block-stride loop at n below, at and beyond one pass, and its 16-wave reduction; |d| on both sides of beta,
    none within 1e-4 of it (the kernel compares in fp32)."""
    c = smooth_l1_case(n, beta)
    assert not ((c["d"] - beta).abs() <= GUARD).any(), "a |d| sits inside the guard band: pick another seed"
    if n >= 64:
        assert (c["d"] < beta).any() and (c["d"] > beta).any()
    loss = torch.full((1,), NAN, device=dev)
    dp = torch.full((n,), NAN, device=dev) if with_dpred else None
    ops.smooth_l1(c["pred"].to(dev), c["tgt"].to(dev), loss, dp, n=n, beta=beta)
    _close(loss, c["loss"].view(1), 1e-6, 1e-6, "loss")
    if with_dpred:
        _close(dp, c["dp"], 1e-8, 1e-5, "dpred")


def _head_ref(x, w, b, dy, rows, D, row_step, row_off, total_rows):
    sel = x.double()[row_off:row_off + rows * row_step:row_step]
    y = sel @ w.double().view(-1) + b.double()
    dx = torch.zeros(total_rows, D, dtype=torch.float64)
    dx[row_off:row_off + rows * row_step:row_step] = dy.double().view(-1, 1) * w.double().view(1, -1)
    return y, dx, (dy.double().view(-1, 1) * sel).sum(0, keepdim=True), dy.double().sum().view(1)


def _head_run(ops, dev, x, w, b, dy, rows, D, row_step, row_off, total_rows, want_dx=True, want_dw=True):
    xd, wd, dyd = x.to(dev), w.to(dev), dy.to(dev)
    y = torch.full((rows,), NAN, device=dev)
    ops.head_fwd(xd, wd, b.to(dev), y, rows=rows, D=D, row_step=row_step, row_off=row_off)
    dx = torch.full((total_rows, D), NAN, device=dev) if want_dx else None
    dw, db = (torch.full((1, D), NAN, device=dev), torch.full((1,), NAN, device=dev)) if want_dw else (None, None)
    ops.head_bwd(xd, wd, dyd, dx, dw, db, rows=rows, D=D, row_step=row_step, row_off=row_off, total_rows=total_rows)
    return y, dx, dw, db


@pytest.mark.parametrize("D", [4, 252, 256, 260, 1024], ids=lambda d: f"D{d}")
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 130], ids=lambda r: f"rows{r}")
def test_head_fwd_bwd_shapes(ops, dev, rows, D):
    """One wave per row with a 256-column stride (D below, at and beyond it; lanes without a column), rows off the 4-per-workgroup
    pitch, 130 rows in the sequential dw / db sums.  Random data at the existing gates, then integer data: y, dx, dw, db exact."""
    g = _gen(1200 + rows + D)
    x, w, b, dy = _rand(g, rows, D), _rand(g, 1, D), _rand(g, 1), _rand(g, rows)
    y, dx, dw, db = _head_run(ops, dev, x, w, b, dy, rows, D, 1, 0, rows)
    ry, rdx, rdw, rdb = _head_ref(x, w, b, dy, rows, D, 1, 0, rows)
    _close(y, ry, 1e-5, 1e-5, "y")
    _close(dx, rdx, 1e-6, 1e-6, "dx")
    _close(dw, rdw, 1e-5, 1e-5, "dw")
    _close(db, rdb, 1e-6, 1e-6, "db")
    x, w, b, dy = _ints(g, -4, 4, rows, D), _ints(g, -4, 4, 1, D), _ints(g, -4, 4, 1), _ints(g, -4, 4, rows)
    y, dx, dw, db = _head_run(ops, dev, x, w, b, dy, rows, D, 1, 0, rows)
    ry, rdx, rdw, rdb = _head_ref(x, w, b, dy, rows, D, 1, 0, rows)
    for name, got, want in (("y", y, ry), ("dx", dx, rdx), ("dw", dw, rdw), ("db", db, rdb)):
        assert torch.equal(got.cpu().double(), want), name


def test_head_row_select_with_trailing_rows_and_optional_outputs(ops, dev):
    """row_step = 3, row_off = 1 and total_rows = rows * row_step + 2: the last trailing row (16) has the selected offset but no item --
    dy holds `rows` entries, so it must come out 0 like every other unselected row, not dy[rows] * w.  Then dx=None (dw / db only)
    and dw=db=None (dx only), the two forms lr2_head_bwd accepts: each leaves the bits of the full call."""
    rows, D, row_step, row_off = 5, 260, 3, 1
    total = rows * row_step + 2
    g = _gen(1300)
    x, w, b, dy = _ints(g, -4, 4, total, D), _ints(g, -4, 4, 1, D), _ints(g, -4, 4, 1), _ints(g, 1, 4, rows)
    # dy sits in a buffer whose next element is non-zero, so an unguarded read of dy[rows] shows
    dy_buf = torch.cat([dy, torch.tensor([7.0])]).to(dev)
    dyd = dy_buf[:rows]
    xd, wd = x.to(dev), w.to(dev)
    y = torch.full((rows,), NAN, device=dev)
    ops.head_fwd(xd, wd, b.to(dev), y, rows=rows, D=D, row_step=row_step, row_off=row_off)
    ry, rdx, rdw, rdb = _head_ref(x, w, b, dy, rows, D, row_step, row_off, total)
    assert torch.equal(y.cpu().double(), ry)
    kw = dict(rows=rows, D=D, row_step=row_step, row_off=row_off, total_rows=total)
    dx, dw, db = torch.full((total, D), NAN, device=dev), torch.full((1, D), NAN, device=dev), torch.full((1,), NAN, device=dev)
    ops.head_bwd(xd, wd, dyd, dx, dw, db, **kw)
    sel = torch.zeros(total, dtype=torch.bool)
    sel[row_off:row_off + rows * row_step:row_step] = True
    assert bool((dx.cpu()[~sel] == 0).all()), "unselected rows of dx must be exactly 0"
    assert torch.equal(dx.cpu().double(), rdx) and torch.equal(dw.cpu().double(), rdw) and torch.equal(db.cpu().double(), rdb)
    dw2, db2 = torch.full((1, D), NAN, device=dev), torch.full((1,), NAN, device=dev)
    ops.head_bwd(xd, wd, dyd, None, dw2, db2, **kw)
    assert torch.equal(dw2, dw) and torch.equal(db2, db)
    dx2 = torch.full((total, D), NAN, device=dev)
    ops.head_bwd(xd, wd, dyd, dx2, None, None, **kw)
    assert torch.equal(dx2, dx)


@pytest.mark.parametrize("rows,period,D", [(11, 4, 8), (11, 4, 5), (3, 5, 8), (1, 1, 4)],
                         ids=["rows11-period4", "rows11-period4-D5", "period5-gt-rows3", "rows1-period1"])
def test_period_rows_grad_ragged(ops, dev, rows, period, D):
    """rows % period != 0 (the last period is short) and period > rows (table rows that no row reaches are 0): integers, exact."""
    g = _gen(1400 + rows + D)
    dy = _ints(g, -8, 8, rows, D)
    ref = torch.zeros(period, D, dtype=torch.float64)
    for r in range(rows):
        ref[r % period] += dy[r].double()
    dt = torch.full((period, D), NAN, device=dev)
    ops.period_rows_grad(dy.to(dev), dt, rows=rows, D=D, period=period)
    assert torch.equal(dt.cpu().double(), ref)
