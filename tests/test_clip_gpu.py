"""Kernel-level tests of global gradient-norm clipping (csrc/clip.hip and the fused GEMM epilogue's adam_gscale_dev): fixed-order fp64
sums against exact / fp64 references, the coefficient against torch.nn.utils.clip_grad_norm_'s formula, and the scaled AdamW update --
multi-tensor and fused into the weight-gradient GEMM -- against lr2_adamw_multi on gradients torch multiplied in fp32."""
import math

import pytest
import torch

from lr2ppo_amd import _native as native

pytestmark = pytest.mark.gpu

CH = 4096                       # chunk size of the tables built here (the optimizer's are 2^13 .. 2^18)
SIZES = [1, 3, 4, 255, 256, 257, CH - 1, CH + 1, 2 * CH + 5]
REL45, REL22 = 2.0 ** -45, 2.0 ** -22
HYP = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-6)


def _table(rows, dev):
    """rows: (p, g, m, v, weight_decay) tensors (None -> 0) -> (device table, n_chunks), chunks of at most CH elements."""
    chunks = []
    for p, g, m, v, wd in rows:
        n, off = g.numel(), 0
        while off < n:
            c = min(CH, n - off)
            chunks.append(tuple(0 if t is None else t.data_ptr() + 4 * off for t in (p, g, m, v)) + (c, wd))
            off += c
    arr = (native.AdamChunk * len(chunks))()
    for i, (p, g, m, v, c, wd) in enumerate(chunks):
        arr[i].p, arr[i].g, arr[i].m, arr[i].v, arr[i].count, arr[i].weight_decay = p, g, m, v, c, wd
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev), len(chunks)


def _view(values, start, dev, pad=float("nan")):
    """`values` placed `start` floats into a 16-byte aligned buffer filled with `pad` -> (buffer, view)."""
    n = values.numel()
    buf = torch.full((start + n + 9,), pad, dtype=torch.float32, device=dev)
    buf[start:start + n] = values.to(dev)
    return buf, buf[start:start + n]


def _sumsq(ops, views, dev):
    table, n = _table([(None, g, None, None, 0.0) for g in views], dev)
    buf = torch.full((n + 2,), -7.0, dtype=torch.float64, device=dev)
    ops.clip_sumsq(table, n, buf[1:1 + n])
    torch.cuda.synchronize()
    assert float(buf[0]) == -7.0 and float(buf[-1]) == -7.0            # canaries either side of the partials
    return buf[1:1 + n].clone()


@pytest.mark.parametrize("start", [0, 1, 2, 3])
def test_sumsq_sizes_alignments_exact_and_fp64(dev, start):
    from lr2ppo_amd import ops
    gen = torch.Generator().manual_seed(100 + start)
    ints = [torch.randint(-8, 9, (n,), generator=gen).float() for n in SIZES]
    rnd = [torch.randn(n, generator=gen) * 3.0 for n in SIZES]
    for vals, exact in ((ints, True), (rnd, False)):
        # a NaN either side of every view: a read past its ends poisons the sum
        views = [_view(v, start, dev) for v in vals]
        got = _sumsq(ops, [v for _, v in views], dev)
        again = _sumsq(ops, [v for _, v in views], dev)
        assert torch.equal(got, again)                                    # fixed order: equal bits from run to run
        i = 0
        for v in vals:
            n_chunks = -(-v.numel() // CH)
            total = math.fsum(float(x) for x in got[i:i + n_chunks].tolist())
            want = math.fsum(float(x) * float(x) for x in v.tolist())    # squares of fp32 values are exact in fp64
            if exact:
                assert total == want, (v.numel(), start)
                for c in range(n_chunks):                                 # and every partial is its own chunk's sum
                    assert float(got[i + c]) == float((v[c * CH:(c + 1) * CH].double() ** 2).sum())
            else:
                assert abs(total - want) <= REL45 * want, (v.numel(), start, total, want)
            i += n_chunks
        assert i == got.numel()


def test_sumsq_and_coef_follow_the_formula_through_nan_and_inf(dev):
    from lr2ppo_amd import ops
    out = torch.full((4,), 5.0, device=dev)
    for bad, want in ((float("nan"), (math.isnan, math.isnan)), (float("inf"), (lambda t: t == math.inf, lambda c: c == 0.0))):
        g = torch.ones(300)
        g[17] = bad
        part = _sumsq(ops, [g.to(dev)], dev)
        ops.clip_coef(part, 1, 1.0, out[1:3])
        total, coef = out[1:3].tolist()
        assert want[0](total) and want[1](coef), (bad, total, coef)
        assert out[0] == 5.0 and out[3] == 5.0


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 640])
def test_gram_dot_exact_and_fp64(dev, n):
    from lr2ppo_amd import ops
    gen = torch.Generator().manual_seed(n)
    slot = torch.full((3,), -7.0, dtype=torch.float64, device=dev)
    # integers: exact, contiguous and as the leading block of wider rows (ld > n, NaN behind every row)
    a, b = torch.randint(-9, 10, (n, n), generator=gen).float(), torch.randint(-9, 10, (n, n), generator=gen).float()
    want = float((a.double() * b.double()).sum())
    ops.clip_gram_dot(a.to(dev), b.to(dev), slot[1:2], n=n, factor=0.25)
    assert float(slot[1]) == 0.25 * want and float(slot[0]) == -7.0 and float(slot[2]) == -7.0
    for ld_a, ld_b, start in ((n + 4, n + 8, 0), (n + 3, n + 1, 1)):
        wa = torch.full((n * ld_a + start + 4,), float("nan"), device=dev)
        wb = torch.full((n * ld_b + start + 4,), float("nan"), device=dev)
        va, vb = wa[start:start + n * ld_a].view(n, ld_a), wb[start:start + n * ld_b].view(n, ld_b)
        va[:, :n], vb[:, :n] = a.to(dev), b.to(dev)
        ops.clip_gram_dot(wa[start:], wb[start:], slot[1:2], n=n, factor=1.0, ld_a=ld_a, ld_b=ld_b)
        assert float(slot[1]) == want, (n, ld_a, ld_b, start)
    # Gram matrices of random factors with a common component (as activations have): fp64 of the same fp32 matrices
    x, y = 1.0 + 0.1 * torch.randn(n, 32, generator=gen), 1.0 + 0.1 * torch.randn(n, 48, generator=gen)
    ga, gb = x @ x.t(), y @ y.t()
    want = float((ga.double() * gb.double()).sum())
    ops.clip_gram_dot(ga.to(dev), gb.to(dev), slot[1:2], n=n, factor=1.0)
    first = float(slot[1])
    assert abs(first - want) <= REL45 * want, (n, first, want)
    ops.clip_gram_dot(ga.to(dev), gb.to(dev), slot[1:2], n=n, factor=1.0)
    assert float(slot[1]) == first


def _coef_ref(total_sq, max_norm):
    total = math.sqrt(total_sq)
    return total, min(1.0, max_norm / (total + 1e-6))


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 700])
def test_coef_matches_clip_grad_norm_formula(dev, n):
    from lr2ppo_amd import ops
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float64).to(torch.float32))      # noqa: E731
    out = torch.full((4,), 5.0, device=dev)
    # integer slots with a perfect-square sum: exact
    slots = torch.zeros(n, dtype=torch.float64)
    slots[0], slots[-1] = slots[0] + 9.0, slots[-1] + 16.0                  # n == 1: 25
    if n > 2:
        slots[1:-1] = 4.0
    total_sq = float(slots.sum())
    k = math.isqrt(int(total_sq))
    slots[0] += (k + 1) ** 2 - total_sq                                     # round the sum up to the next square
    total_sq = float(slots.sum())
    buf = torch.full((n + 2,), float("nan"), dtype=torch.float64, device=dev)
    buf[1:1 + n] = slots.to(dev)
    for max_norm in (0.5, 3.0):
        ops.clip_coef(buf[1:], n, max_norm, out[1:3])
        total, coef = _coef_ref(total_sq, max_norm)
        assert total == k + 1 and out[1:3].tolist() == [f32(total), f32(coef)] and coef < 1.0
        assert out[0] == 5.0 and out[3] == 5.0
    ops.clip_coef(buf[1:], n, float(k + 2), out[1:3])                       # max_norm above the norm: exactly 1
    assert out[1:3].tolist() == [float(k + 1), 1.0]
    # generic values: the formula in Python fp64
    slots = torch.rand(n, dtype=torch.float64, generator=torch.Generator().manual_seed(n)) * 3.0
    buf[1:1 + n] = slots.to(dev)
    total, coef = _coef_ref(math.fsum(slots.tolist()), 0.37)
    ops.clip_coef(buf[1:], n, 0.37, out[1:3])
    got_total, got_coef = out[1:3].tolist()
    assert abs(got_total - total) <= REL22 * total and abs(got_coef - coef) <= REL22 * coef and got_coef < 1.0


def _adam_case(sizes, start, dev, seed):
    """Per size (p, g, m, v) values on the CPU, and per tensor a NaN-free canaried buffer + view `start` floats in."""
    gen = torch.Generator().manual_seed(seed)
    vals = [(torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 2.0, torch.randn(n, generator=gen) * 0.1,
             torch.rand(n, generator=gen) * 0.01) for n in sizes]
    return vals


def _run_adam(ops, vals, start, dev, *, scaled, g_mul=None, coef=None, lr_dev=None):
    bufs, rows = [], []
    for i, (p, g, m, v) in enumerate(vals):
        if g_mul is not None:
            g = (g.to(dev) * g_mul).cpu()                                    # torch's fp32 multiply, on the device like the kernel's
        quad = [_view(t, start, dev, pad=123.0) for t in (p, g, m, v)]
        bufs.append(quad)
        rows.append(tuple(vw for _, vw in quad) + (0.01 if i % 2 == 0 else 0.0,))
    table, n = _table(rows, dev)
    if scaled:
        ops.adamw_multi_scaled(table, n, HYP["lr"], HYP["beta1"], HYP["beta2"], HYP["eps"], coef, lr_dev=lr_dev)
    else:
        ops.adamw_multi(table, n, HYP["lr"], HYP["beta1"], HYP["beta2"], HYP["eps"], lr_dev=lr_dev)
    torch.cuda.synchronize()
    for quad, (p, g, m, v) in zip(bufs, vals):
        for buf, _ in quad:                                                  # canaries either side of every view
            assert bool((buf[:start] == 123.0).all()) and bool((buf[start + p.numel():] == 123.0).all())
    return [[vw.clone() for _, vw in quad] for quad in bufs]


@pytest.mark.parametrize("start", [0, 1, 2, 3])
def test_scaled_adamw_gives_the_bits_of_adamw_on_premultiplied_gradients(dev, start):
    from lr2ppo_amd import ops
    vals = _adam_case(SIZES, start, dev, 40 + start)
    one, c03 = torch.ones(1, device=dev), torch.full((1,), 0.3, device=dev)
    base = _run_adam(ops, vals, 0, dev, scaled=False)                                      # lr2_adamw_multi, aligned
    got1 = _run_adam(ops, vals, start, dev, scaled=True, coef=one)
    for a, b in zip(base, got1):
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
        assert torch.equal(a[1], b[1])                                                     # gradients in memory stay as they are
    pre = _run_adam(ops, vals, 0, dev, scaled=False, g_mul=c03)
    got = _run_adam(ops, vals, start, dev, scaled=True, coef=c03)
    for (p, g, m, v), a, b in zip(vals, pre, got):
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
        assert torch.equal(b[1].cpu(), g) and not torch.equal(a[0].cpu(), p)
    # the rate from device memory, as a captured step reads it
    lr_dev = torch.full((1,), HYP["lr"], device=dev)
    got_dev = _run_adam(ops, vals, start, dev, scaled=True, coef=c03, lr_dev=lr_dev)
    for a, b in zip(got, got_dev):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("planes", [False, True])
@pytest.mark.parametrize("K", [8, 64, 192])
@pytest.mark.parametrize("splits", [1, 2])
def test_fused_epilogue_scales_like_the_unfused_route(dev, planes, K, splits):
    """TN form, M = 128, N = 256: with adam_gscale_dev the fused weight-gradient + AdamW call bit-equals the unfused product, torch's
    fp32 multiply by the coefficient, then lr2_adamw_multi; with a null pointer it is today's fused call."""
    from lr2ppo_amd import ops
    M, N = 128, 256
    gen = torch.Generator().manual_seed(K + splits)
    a, b = torch.randn(K, M, generator=gen).to(dev), torch.randn(K, N, generator=gen).to(dev)
    if planes:
        a, b = ops.split_planes(a, ops.Planes.empty(K, M, dev)), ops.split_planes(b, ops.Planes.empty(K, N, dev))
    p0, m0, v0 = (torch.randn(M, N, generator=gen).to(dev), (torch.randn(M, N, generator=gen) * 0.1).to(dev),
                  (torch.rand(M, N, generator=gen) * 0.01).to(dev))
    ws = torch.empty(splits * M * N, device=dev) if splits > 1 else None
    kw = dict(trans_a=True, trans_b=True, lda=M, ldb=N, splitk_ws=ws, splits=splits, block_m=128, alpha=0.5)
    coef = torch.full((3,), 123.0, device=dev)
    coef[1] = 0.3

    def fused(gscale):
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        ops.gemm(a, b, None, M, N, K, adam=ops.AdamArgs(p, m, v, HYP["lr"], HYP["beta1"], HYP["beta2"], HYP["eps"], 0.01,
                                                       gscale_dev=gscale), **kw)
        return p, m, v

    def unfused(mul):
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        g = torch.empty(M, N, device=dev)
        ops.gemm(a, b, g, M, N, K, **kw)
        if mul is not None:
            g = g * mul
        table, n = _table([(p, g, m, v, 0.01)], dev)
        ops.adamw_multi(table, n, HYP["lr"], HYP["beta1"], HYP["beta2"], HYP["eps"])
        return p, m, v

    plain, today = unfused(None), fused(None)
    assert all(torch.equal(x, y) for x, y in zip(plain, today))
    want, got = unfused(coef[1:2]), fused(coef[1:2])
    assert all(torch.equal(x, y) for x, y in zip(want, got))
    assert not torch.equal(got[0], today[0]) and coef.tolist() == [123.0, pytest.approx(0.3), 123.0]
    ones = fused(torch.ones(1, device=dev))
    assert all(torch.equal(x, y) for x, y in zip(ones, today))
