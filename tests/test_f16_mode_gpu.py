"""The single-pass f16 inference mode on a real MI355X: the 256 x 256 f16 product (csrc/gemm256_f16.hip) against exact and fp64
references -- integers, 11-bit operands a bf16 instruction or plane would round, the fp32 accumulation bound --, the f16 plane writer
of the product / LayerNorm / lr2_round_f16 / attention byte for byte against round-to-nearest-even of the fp32 results (subnormal range
and saturation included), the attention (csrc/selfattn_mx.hip) against fp64 and against the bf16 kernel's distance from it,
TransformerEncoder.forward_f16 against an fp64 emulation that rounds to f16 where the schedule writes a plane, and
FeatureExtractor(precision="f16") against the split-bf16 path AND the bf16 mode of the same weights: at most a quarter of the bf16
mode's distance (three more significand bits: 8 x expected).

Measured on MI355X (this file's own prints), each against the reference its test names:
  plumbing, vs the f16 rounding emulation: pre-LN 8.988e-5, post-LN 5.618e-5 (the emulation is 2.706e-4 / 2.684e-4 from the
      unrounded encoder: the second condition of that test)                                       -> gate 3 x the worst = 2.70e-4
  first_only vs row 0 of the full call: 2.577e-4 / 2.664e-4                                        -> gate 1.5 x the worst (deterministic),
      far below the bf16 file's FIRST_ONLY_GATE (3.16e-3)
  attention vs fp64 of its own operands, f16 / bf16 (ratio): L = 16 1.2-1.4e-4 / 1.0-1.1e-3 (8.0-8.5), L = 197 and 288 1.7-1.8e-4 /
      1.4-1.5e-3 (7.98-8.06), one-pair and persistent form alike                                   -> asserted: ratio >= 4
  mode vs split-bf16, two layers, f16 / bf16 (ratio): E = 256 text 7.35e-5 / 5.75e-4 (7.8), image 4.03e-4 / 3.18e-3 (7.9); E = 768 text
      2.21e-4 / 1.77e-3 (8.0), image 5.26e-4 / 4.20e-3 (8.0), Actor logits (relative L2) 1.06e-3 / 4.16e-2 (39; max |d logit| 6.3e-5
      / 2.07e-3)                                                                                   -> asserted: ratio >= 4
  fallbacks vs split-bf16 (L = 304) / plain fp64 (head width 32): f16 3.15e-5 / 3.14e-5, bf16 2.53e-4 / 2.58e-4
  subnormal probe: the f16 MFMA KEEPS subnormal operands (2^-20 x 2^10 -> 2^-10)
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
F16_MAX = 65504.0
PLUMBING_GATE = 3 * 8.988e-5
FIRST_ONLY_GATE_F16 = 1.5 * 2.664e-4


def _shapes():
    from test_bf16_mode_gpu import SHAPES
    return SHAPES


SHAPES = [(256, 256, 64), (300, 256, 128), (257, 320, 192), (512, 264, 448), (1, 256, 64)]     # == tests/test_bf16_mode_gpu.py's


def test_shapes_are_the_bf16_files_and_cover_both_tile_forms():
    import ctypes

    from lr2ppo_amd import _native
    assert SHAPES == _shapes()
    rows = []
    for M, N, _ in SHAPES:
        r = ctypes.c_int(0)
        assert _native.lib().lr2_gemm256_tile_rows(M, N, ctypes.byref(r)) == 0
        rows.append(r.value)
    assert rows == [192, 256, 256, 192, 256], rows                  # the 192-row and the 256-row tile form


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def _h(x):
    """round to nearest even to f16 (through fp32, as the kernels hold fp32 values), back in fp64"""
    return x.float().to(torch.float16).double()


def _bits(t):
    return t.contiguous().view(-1).view(torch.int16)


def _f16_cpu(x32):
    """IEEE round-to-nearest-even f16 bits of an fp32 tensor, on the host"""
    return x32.detach().cpu().to(torch.float16).view(-1).view(torch.int16)


def _counted(ops, n=1):
    class _C:
        def __enter__(self):
            self.c0 = ops.gemm_f16_launch_count()

        def __exit__(self, *exc):
            if exc[0] is None:
                assert ops.gemm_f16_launch_count() - self.c0 == n
    return _C()


# ---- the product ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M, N, K", SHAPES)
def test_product_exact_on_integers(dev, M, N, K):
    """Integers in [-8, 8] against an asymmetric B (integers in [-3, 8]: a sign or operand mix-up cannot cancel): every partial sum is
    an integer below 2^24, the result equals the fp64 product exactly."""
    from lr2ppo_amd import ops
    g = torch.Generator(device=dev).manual_seed(1)
    a = torch.randint(-8, 9, (M, K), device=dev, generator=g).to(torch.float16)
    b = torch.randint(-3, 9, (N, K), device=dev, generator=g).to(torch.float16)
    out = torch.full((M, N), float("nan"), device=dev)
    with _counted(ops):
        ops.gemm_f16(a, b, out, M, N, K)
    assert torch.equal(out.double(), a.double() @ b.double().T)


@pytest.mark.parametrize("M, N", [(M, N) for M, N, _ in SHAPES])
def test_product_keeps_eleven_bits(dev, M, N):
    """K = 64.  At even k the A operand is 1 + j 2^-10 with j odd (exact in f16, NOT in bf16) and the B operand a small integer, at odd
    k the other way round: every product is a multiple of 2^-10 below 16 and every partial sum a multiple of 2^-10 below 2^10 -- exact
    in fp32, so the result must EQUAL the fp64 product.  A bf16 MFMA, or a bf16-rounded plane anywhere, fails this; so does a fragment
    map that pairs the wrong k."""
    from lr2ppo_amd import ops
    K = 64
    g = torch.Generator(device=dev).manual_seed(2)

    def fine(rows):
        return 1.0 + (2 * torch.randint(0, 512, (rows, K), device=dev, generator=g) + 1).double() * 2.0 ** -10

    def ints(rows, lo):
        return torch.randint(lo, 9, (rows, K), device=dev, generator=g).double()

    even = (torch.arange(K, device=dev) % 2 == 0)
    a64 = torch.where(even, fine(M), ints(M, -8))
    b64 = torch.where(even, ints(N, -3), fine(N))
    a, b = a64.to(torch.float16), b64.to(torch.float16)
    assert torch.equal(a.double(), a64) and torch.equal(b.double(), b64)                    # exact in f16 ...
    assert not torch.equal(a.to(torch.bfloat16).double(), a64)                               # ... and not in bf16
    out = torch.full((M, N), float("nan"), device=dev)
    ops.gemm_f16(a, b, out, M, N, K)
    assert torch.equal(out.double(), a64 @ b64.T)


def _normal_operands(M, N, K, dev, seed):
    """normal data rounded to f16; operands stay normal or zero (|x| >= 2^-14)"""
    g = torch.Generator(device=dev).manual_seed(seed)
    a = torch.randn(M, K, device=dev, generator=g).to(torch.float16)
    b = torch.randn(N, K, device=dev, generator=g).to(torch.float16)
    a[a.abs() < 2.0 ** -14] = 0
    b[b.abs() < 2.0 ** -14] = 0
    return a, b


@pytest.mark.parametrize("M, N, K", SHAPES)
def test_product_within_the_fp32_accumulation_bound(dev, M, N, K):
    """|err| <= K * 2^-24 * sum_k |a_k b_k| against the fp64 product of the f16 values (an f16 x f16 product is exact in fp32)."""
    from lr2ppo_amd import ops
    a, b = _normal_operands(M, N, K, dev, 3)
    out = torch.full((M, N), float("nan"), device=dev)
    ops.gemm_f16(a, b, out, M, N, K)
    ref = a.double() @ b.double().T
    bound = K * U * (a.double().abs() @ b.double().abs().T)
    err = (out.double() - ref).abs()
    print(f"\n{M}x{N}x{K} f16: max err / bound = {(err / bound.clamp_min(1e-300)).max().item():.3e}")
    assert (err <= bound).all()


def test_subnormal_operand_probe(dev):
    """Not asserted (the mode's contract does not depend on it; DESIGN.md 2 records the answer): one product 2^-20 x 2^10 -- the A
    operand an f16 subnormal -- is 2^-10 when the matrix core keeps subnormal operands and 0 when it flushes them."""
    from lr2ppo_amd import ops
    M = N = 256
    K = 64
    a = torch.zeros(M, K, device=dev, dtype=torch.float16)
    b = torch.zeros(N, K, device=dev, dtype=torch.float16)
    a[:, 5] = 2.0 ** -20
    b[:, 5] = 2.0 ** 10
    assert a[0, 5].item() == 2.0 ** -20
    out = torch.full((M, N), float("nan"), device=dev)
    ops.gemm_f16(a, b, out, M, N, K)
    v = out[3, 7].item()
    print(f"\nf16 subnormal operand 2^-20 x 2^10 -> {v!r} ({'kept' if v == 2.0 ** -10 else 'FLUSHED' if v == 0.0 else 'other'}); "
          f"uniform over the tile: {bool((out == v).all())}")
    assert torch.isfinite(out).all()


@pytest.mark.parametrize("M, N, K", SHAPES)
def test_product_with_bias_gelu_residual(dev, M, N, K):
    """tests/test_bf16_mode_gpu.py::test_product_with_bias_gelu_residual's tolerance expression, unchanged."""
    from lr2ppo_amd import ops
    a, b = _normal_operands(M, N, K, dev, 4)
    g = torch.Generator(device=dev).manual_seed(5)
    bias = torch.randn(N, device=dev, generator=g)
    resid = torch.randn(M, N, device=dev, generator=g)
    out = torch.full((M, N), float("nan"), device=dev)
    ops.gemm_f16(a, b, out, M, N, K, bias=bias, act=1, resid=resid)
    z = a.double() @ b.double().T + bias.double()
    gz = 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))
    ref = gz + resid.double()
    zb = K * U * (a.double().abs() @ b.double().abs().T) + 2 * U * z.abs()
    tol = 1.13 * zb + 3e-7 * z.abs() + 4 * U * (gz.abs() + z.abs()) + 2 * U * (resid.double().abs() + ref.abs())
    err = (out.double() - ref).abs()
    print(f"\n{M}x{N}x{K} f16 bias+GELU+resid: max err / tol = {(err / tol).max().item():.3e}")
    assert (err <= tol).all()
    # alpha, and a residual without the activation
    ops.gemm_f16(a, b, out, M, N, K, bias=bias, resid=resid, alpha=0.5)
    ref = 0.5 * (a.double() @ b.double().T) + bias.double() + resid.double()
    tol = 0.5 * K * U * (a.double().abs() @ b.double().abs().T) + 4 * U * (ref.abs() + resid.double().abs() + bias.double().abs())
    assert ((out.double() - ref).abs() <= tol).all()


@pytest.mark.parametrize("M, N, K", SHAPES)
def test_product_plane_is_rne_f16_of_the_fp32_result(dev, M, N, K):
    """The f16 plane of a both-outputs launch and of a plane-only launch == out.to(float16) byte for byte -- at the data's own scale,
    with GELU, and with alpha scaling the results into the f16 subnormal range (|v| in 1e-7 .. 6e-5); nothing is written behind it."""
    from lr2ppo_amd import ops
    a, b = _normal_operands(M, N, K, dev, 6)
    bias = torch.randn(N, device=dev, generator=torch.Generator(device=dev).manual_seed(7))
    for act, alpha, use_bias in ((0, 1.0, True), (1, 1.0, True), (0, 2e-6, False), (0, 3e-7, False)):
        out = torch.full((M, N), float("nan"), device=dev)
        both = torch.zeros(M * N + 8, dtype=torch.float16, device=dev)
        alone = torch.zeros(M * N + 8, dtype=torch.float16, device=dev)
        kw = dict(bias=bias if use_bias else None, act=act, alpha=alpha)
        ops.gemm_f16(a, b, out, M, N, K, out_plane=both, **kw)          # both outputs, one launch
        ops.gemm_f16(a, b, None, M, N, K, out_plane=alone, **kw)        # the plane alone
        want = _f16_cpu(out)
        if alpha < 1e-3:
            mag = out.abs()
            sub = ((mag > 1e-7) & (mag < 6e-5)).float().mean().item()
            assert sub > 0.5, sub                                       # the case is about subnormal results
            assert (want.view(torch.float16)[(mag.view(-1) > 1e-7).cpu()] != 0).all()        # ... stored as subnormals, not flushed
        assert torch.equal(_bits(both[:M * N]).cpu(), want), (act, alpha)
        assert torch.equal(_bits(alone[:M * N]).cpu(), want), (act, alpha)
        assert (both[M * N:] == 0).all() and (alone[M * N:] == 0).all()                      # nothing behind the plane
    # hi / lo bf16 planes out of the same kernel: the QKV product in front of the 3-pass attention kernels
    pl = ops.Planes.empty(M, N, dev)
    out = torch.empty(M, N, device=dev)
    ops.gemm_f16(a, b, out, M, N, K, bias=bias, out_planes=pl)
    hi = out.to(torch.bfloat16)
    assert torch.equal(pl.buf[:M * N], hi.view(-1).view(torch.int16))
    assert torch.equal(pl.buf[M * N:].view(torch.bfloat16), (out - hi.float()).to(torch.bfloat16).view(-1))


@pytest.mark.parametrize("M, N, K", SHAPES)
def test_product_plane_saturates(dev, M, N, K):
    """A bias of +-1e5: the plane holds +-65504 (0x7BFF / 0xFBFF), never inf; the fp32 output keeps the true value."""
    from lr2ppo_amd import ops
    a, b = _normal_operands(M, N, K, dev, 8)
    bias = torch.full((N,), 1e5, device=dev)
    bias[1::2] = -1e5
    out = torch.full((M, N), float("nan"), device=dev)
    both = torch.zeros(M * N, dtype=torch.float16, device=dev)
    alone = torch.zeros(M * N, dtype=torch.float16, device=dev)
    ops.gemm_f16(a, b, out, M, N, K, bias=bias, out_plane=both)
    ops.gemm_f16(a, b, None, M, N, K, bias=bias, out_plane=alone)
    ref = a.double() @ b.double().T + bias.double()
    assert ((out.double() - ref).abs() <= K * U * (a.double().abs() @ b.double().abs().T) + 2 * U * ref.abs()).all()
    assert (out.abs() > F16_MAX).all()
    want = torch.where(out > 0, torch.tensor(0x7BFF, device=dev), torch.tensor(0xFBFF - 0x10000, device=dev)).to(torch.int16).view(-1)
    assert torch.equal(_bits(both), want) and torch.equal(_bits(alone), want)


# ---- LayerNorm and round ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("D", [768, 100])
@pytest.mark.parametrize("rows", [1, 5, 300])
def test_layernorm_plane_is_rne_f16_of_its_fp32_output(dev, rows, D, mode):
    from lr2ppo_amd import ops
    g = torch.Generator(device=dev).manual_seed(9)
    x = torch.randn(rows, D, device=dev, generator=g) * 3 + 1
    gamma, beta = torch.randn(D, device=dev, generator=g), torch.randn(D, device=dev, generator=g)
    both = torch.zeros(rows * D + 8, dtype=torch.float16, device=dev)
    alone = torch.zeros(rows * D + 8, dtype=torch.float16, device=dev)
    f32 = torch.full((rows, D), float("nan"), device=dev)
    ops.layernorm_fwd_f16(x, gamma, beta, rows=rows, D=D, eps=1e-6, mode=mode, out=f32, out_plane=both)
    ops.layernorm_fwd_f16(x, gamma, beta, rows=rows, D=D, eps=1e-6, mode=mode, out_plane=alone)
    want = _f16_cpu(f32)
    assert torch.equal(_bits(both[:rows * D]).cpu(), want) and torch.equal(_bits(alone[:rows * D]).cpu(), want)
    assert (both[rows * D:] == 0).all() and (alone[rows * D:] == 0).all()
    # ... and the fp32 output is the existing kernel's (same statistics, same row)
    ref = torch.empty(rows, D, device=dev)
    ops.layernorm_fwd(x, gamma, beta, ref, rows=rows, D=D, eps=1e-6, mode=mode)
    assert torch.equal(f32, ref)


def test_round_f16(dev):
    from lr2ppo_amd import ops
    g = torch.Generator(device=dev).manual_seed(10)
    n = 4 * 70001
    x = torch.randn(n, device=dev, generator=g)
    x[::3] *= 1e-5                                                  # the f16 subnormal range
    x[1::7] *= 1e-8                                                 # below half the smallest subnormal: zero
    x[5::11] *= 300.0
    dst = torch.zeros(n + 8, dtype=torch.float16, device=dev)
    ops.round_f16(x, dst)
    assert torch.equal(_bits(dst[:n]).cpu(), _f16_cpu(x)) and (dst[n:] == 0).all()
    # saturation, ties at the top of the range, NaN
    y = torch.tensor([1e5, -1e5, 65504.0, -65504.0, 65519.9, 65520.0, -65520.0, 3.4e38, -3.4e38, float("inf"), float("-inf"), 0.0],
                     device=dev)
    d2 = torch.zeros(12, dtype=torch.float16, device=dev)
    ops.round_f16(y, d2)
    assert d2[:11].abs().tolist() == [F16_MAX] * 11 and torch.equal(d2[:11].sign(), y[:11].sign()) and d2[11].item() == 0.0
    z = torch.tensor([float("nan"), 1.0, -0.0, 2.0 ** -24], device=dev)
    d3 = torch.zeros(4, dtype=torch.float16, device=dev)
    ops.round_f16(z, d3)
    assert torch.isnan(d3[0]) and d3[1].item() == 1.0 and _bits(d3)[2].item() == -0x8000 and d3[3].item() == 2.0 ** -24


# ---- attention --------------------------------------------------------------------------------------------------------------------
def _attn_ref(qkv, seg, batch, L, heads):
    E = heads * 64
    q, k, v = (t.double().view(batch, L, heads, 64).transpose(1, 2) for t in qkv.split(E, dim=1))
    s = q @ k.transpose(-1, -2) * 0.125 + (seg <= 0).double()[:, None, None, :] * -10000.0
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(batch * L, E)


@pytest.mark.parametrize("batch, heads", [(2, 4), (64, 4)])
@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("L", [1, 16, 197, 288])
def test_attention_plane_and_accuracy(dev, L, padded, batch, heads):
    """The plane == RNE f16 of the fp32 context (both outputs at once, the plane alone), in the one-pair and in the persistent form; and
    the kernel's distance (relative L2) from fp64 attention of its own rounded operands is at most a QUARTER of
    ops.self_attn_fwd_bf16's on the same fp32 data: what remains is the 2-byte rounding of P, three bits finer (expected ratio 8; the
    factor 2 of margin covers fp32 accumulation and v_exp_f32)."""
    from lr2ppo_amd import _native, ops
    cus = _native.lib().lr2_device_info(None, 0)
    assert ops.self_attn_bf16_plan(batch, heads, L) == (batch * heads >= cus)   # (2, 4): one workgroup per pair; (64, 4): persistent
    E = heads * 64
    g = torch.Generator(device=dev).manual_seed(11)
    qkv32 = torch.randn(batch * L, 3 * E, device=dev, generator=g)
    qkv = qkv32.to(torch.float16)
    seg = torch.ones(batch, L, dtype=torch.int64, device=dev)
    if padded:
        seg[:, max(1, (2 * L) // 3):] = 0
    o32 = torch.full((batch * L, E), float("nan"), device=dev)
    both = torch.zeros(batch * L * E + 8, dtype=torch.float16, device=dev)
    alone = torch.zeros(batch * L * E + 8, dtype=torch.float16, device=dev)
    kw = dict(batch=batch, heads=heads, L=L, head_dim=64, scale=0.125)
    c0 = ops.self_attn_fwd_f16_launch_count()
    ops.self_attn_fwd_f16(qkv, seg.view(-1), out=o32, out_plane=both, **kw)
    ops.self_attn_fwd_f16(qkv, seg.view(-1), out_plane=alone, **kw)
    assert ops.self_attn_fwd_f16_launch_count() - c0 == 2
    assert torch.isfinite(o32).all()
    want = _f16_cpu(o32)
    n = batch * L * E
    assert torch.equal(_bits(both[:n]).cpu(), want) and torch.equal(_bits(alone[:n]).cpu(), want)
    assert (both[n:] == 0).all() and (alone[n:] == 0).all()
    d16 = _rel(o32, _attn_ref(qkv, seg, batch, L, heads))
    qkv_b = qkv32.to(torch.bfloat16)
    ob = torch.empty(batch * L, E, device=dev)
    ops.self_attn_fwd_bf16(qkv_b, seg.view(-1), out=ob, **kw)
    dbf = _rel(ob, _attn_ref(qkv_b, seg, batch, L, heads))
    print(f"\nattention L={L} padded={padded} B={batch} H={heads}: f16 {d16:.3e}, bf16 {dbf:.3e}, ratio {dbf / max(d16, 1e-30):.2f}")
    if L == 1 or (padded and max(1, (2 * L) // 3) == 1):
        assert d16 <= 4 * U                                         # one visible key: P = 1, the context is V's row (both kernels exact)
    else:
        assert d16 <= dbf / 4


@pytest.mark.parametrize("batch, heads", [(2, 4), (64, 4)])
def test_attention_exact_column_mean(dev, batch, heads):
    """Q = 0, V small integers, L = 16: every probability is 1 (exact in f16), the sum 16, the context the exact column mean."""
    from lr2ppo_amd import ops
    L, E = 16, heads * 64
    g = torch.Generator(device=dev).manual_seed(12)
    qkv = torch.randn(batch * L, 3 * E, device=dev, generator=g)
    qkv[:, :E] = 0
    qkv[:, 2 * E:] = torch.randint(-8, 9, (batch * L, E), device=dev, generator=g).float()
    qkv = qkv.to(torch.float16)
    seg = torch.ones(batch * L, dtype=torch.int64, device=dev)
    o32 = torch.full((batch * L, E), float("nan"), device=dev)
    ops.self_attn_fwd_f16(qkv, seg, out=o32, batch=batch, heads=heads, L=L, head_dim=64, scale=0.125)
    mean = qkv[:, 2 * E:].double().view(batch, L, E).mean(1, keepdim=True).expand(batch, L, E).reshape(batch * L, E)
    assert torch.equal(o32.double(), mean)


# ---- the schedule against an fp64 emulation that rounds to f16 where forward_f16 writes a plane ------------------------------------
def _ln(x, m):
    mean = x.mean(-1, keepdim=True)
    std = x.std(-1, unbiased=True, keepdim=True)
    return m.gamma.double() * (x - mean) / (std + m.eps) + m.beta.double()


def _emulate(enc, emb, seg, rnd):
    """tests/test_bf16_mode_gpu.py::_emulate with the rounding a parameter: forward_f16 in fp64, rounded by `rnd` (via fp32, as the
    kernels hold fp32 values) exactly where the schedule writes a plane -- the LayerNorm output / the post-LN hidden state in front of
    QKV, Q | K | V, the context, the LayerNorm output in front of FFN-1, GELU(z); the weights are rnd(W); inside the attention kernel
    the un-normalised probabilities are rounded, their sum is not.  rnd = identity: the encoder in plain fp64."""
    B, L, E = emb.shape
    H = enc.heads_num
    pre = enc.layernorm_positioning == "pre"
    h = emb.double().view(B * L, E)
    mask = (seg <= 0).double()[:, None, None, :] * -10000.0
    lin = lambda x, m: x @ rnd(m.weight.double()).T + m.bias.double()           # noqa: E731
    gelu = lambda z: 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))           # noqa: E731
    for layer in enc.transformer:
        att, ffn = layer.self_attn, layer.feed_forward
        x = rnd(_ln(h, layer.layer_norm_1)) if pre else rnd(h)
        q, k, v = (rnd(lin(x, m)).view(B, L, H, E // H).transpose(1, 2) for m in att.linear_layers)
        s = q @ k.transpose(-1, -2) / math.sqrt(E // H) + mask
        p = torch.exp(s - s.max(-1, keepdim=True).values)
        o = rnd(((rnd(p) @ v) / p.sum(-1, keepdim=True)).transpose(1, 2).reshape(B * L, E))
        h2 = lin(o, att.final_linear) + h
        if pre:
            t = rnd(_ln(h2, layer.layer_norm_2))
            h = lin(rnd(gelu(lin(t, ffn.linear_1))), ffn.linear_2) + h2
        else:
            xn = _ln(h2, layer.layer_norm_1)
            y = lin(rnd(gelu(lin(rnd(xn), ffn.linear_1))), ffn.linear_2) + xn
            h = _ln(y, layer.layer_norm_2)
    if enc.final_layernorm:
        h = _ln(h, enc.layer_norm)
    return h.view(B, L, E)


def _ident(x):
    return x


@pytest.mark.parametrize("placement, L, padded", [("pre", 197, False), ("post", 196, True)])
def test_forward_f16_matches_the_rounding_emulation(dev, placement, L, padded):
    """One layer, B = 2, E = 256, F = 1024, 4 heads (the bf16 file's case and weights).  Two conditions: 3 x the value measured on
    MI355X (PLUMBING_GATE), and -- whatever was measured -- below rel(emulate_f16, emulate_unrounded): the kernels may not deviate from
    their rounding model by more than the rounding itself (2.7e-4 with these weights).  first_only against row 0 of the full call:
    1.5 x measured, and below the bf16 file's FIRST_ONLY_GATE."""
    from test_bf16_mode_gpu import FIRST_ONLY_GATE, _enc_args

    from lr2ppo_amd.tencentpretrain.encoders import str2encoder
    torch.manual_seed(11)
    enc = str2encoder["transformer"](_enc_args(layernorm_positioning=placement))
    for n, p in enc.named_parameters():
        p.data.normal_(0, 0.05) if "gamma" not in n else p.data.normal_(1.0, 0.1)
    enc = enc.to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(12)
    emb = torch.randn(2, L, 256, device=dev, generator=g)
    seg = torch.ones(2, L, dtype=torch.int64, device=dev)
    if padded:
        seg[1, 150:] = 0
    from lr2ppo_amd import ops
    c0 = ops.self_attn_fwd_f16_launch_count()
    got = enc.forward_f16(emb, seg)
    assert ops.self_attn_fwd_f16_launch_count() - c0 == 1
    ref = _emulate(enc, emb, seg, _h)
    r = _rel(got, ref)
    model = _rel(ref, _emulate(enc, emb, seg, _ident))
    r3 = _rel(got, enc(emb, seg))
    print(f"\nforward_f16 {placement}-LN L={L}: vs emulation {r:.3e}; emulation vs unrounded {model:.3e}; vs the split-bf16 forward {r3:.3e}")
    assert torch.isfinite(got).all() and r < model
    assert r < PLUMBING_GATE
    first = enc.forward_f16(emb, seg, first_only=True)
    r0 = _rel(first, got[:, 0, :])
    print(f"first_only vs row 0 of the full call {r0:.3e}")
    assert first.shape == (2, 256) and torch.isfinite(first).all()
    assert r0 < FIRST_ONLY_GATE_F16 and r0 < FIRST_ONLY_GATE


# ---- the mode against the split-bf16 path and the bf16 mode ------------------------------------------------------------------------
def _three_precisions(fx, frames, ids, seg):
    out = {}
    for prec in ("split_bf16", "bf16", "f16"):
        fx.precision = prec
        out[prec] = fx.extract(frames, ids, seg)
    fx.precision = "split_bf16"
    t2, i2 = fx.extract(frames, ids, seg)
    assert torch.equal(out["split_bf16"][0], t2) and torch.equal(out["split_bf16"][1], i2)     # the shared weight planes are undisturbed
    return out


def _quarter(name, x16, xbf, x0):
    r16, rbf = _rel(x16, x0), _rel(xbf, x0)
    print(f"{name}: f16 {r16:.3e}, bf16 {rbf:.3e} vs split-bf16 (ratio {rbf / r16:.2f})")
    assert torch.isfinite(x16).all()
    assert r16 > 1e-6, name                                         # really another precision
    assert r16 <= rbf / 4, name                                     # three more bits: 8 x expected, 4 x asked


def test_f16_mode_is_four_times_closer_to_split_bf16_than_bf16(dev):
    """The decisive test, at E = 256: two-layer towers (the bf16 file's _small_extractor), split_bf16, bf16 and f16 from the same module;
    rel(f16, split) <= rel(bf16, split) / 4 for text_emb and img_emb (the denominator comes from code this mode does not touch; a single
    producer left in bf16 breaks it), rel(f16, split) > 1e-6, and a final split-bf16 extraction bit-equal to the first."""
    from test_bf16_mode_gpu import _small_extractor

    from lr2ppo_amd.finetune.features import synthetic_raw_batch
    fx = _small_extractor(dev)
    frames, ids, seg, _ = synthetic_raw_batch(2, 2, n_img=4, device=dev, generator=torch.Generator(device=dev).manual_seed(14))
    out = _three_precisions(fx, frames, ids, seg)
    print("\n2 layers, E = 256")
    _quarter("text_emb", out["f16"][0], out["bf16"][0], out["split_bf16"][0])
    _quarter("img_emb", out["f16"][1], out["bf16"][1], out["split_bf16"][1])
    fx.precision = "f16"
    with pytest.raises(NotImplementedError):
        fx.forward_train(frames, ids, seg)
    with pytest.raises(NotImplementedError):
        fx.train()(frames, ids, seg)


def test_f16_mode_is_four_times_closer_at_768_with_the_actors_logits(dev):
    """The same at E = 768, 12 heads, two layers each (ViT-B/16 + RoBERTa-base shapes), with the seeded Actor's logits vector."""
    import argparse as ap

    from test_bf16_mode_gpu import _small_extractor

    from lr2ppo_amd.finetune import ppo
    from lr2ppo_amd.finetune.features import synthetic_raw_batch
    from oracle import lr2ppo_oracle as O
    fx = _small_extractor(dev, hidden_size=768, emb_size=768, feedforward_size=3072, heads_num=12)
    args = ap.Namespace(mode="reg", labels_num=3, seq_length=196, max_imgs=16, visual_feat_dim=768, is_master=True, device=dev)
    actor = ppo.Actor(args, None)
    actor.load_state_dict(O.seeded_params(O.head_param_spec("actor"), seed=7), strict=True)
    actor = actor.to(dev).eval()
    frames, ids, seg, _ = synthetic_raw_batch(2, 2, device=dev, generator=torch.Generator(device=dev).manual_seed(19))
    out = _three_precisions(fx, frames, ids, seg)
    with torch.no_grad():
        lg = {k: actor(t, i, None) for k, (t, i) in out.items()}
    print(f"\n2 layers, E = 768; Actor max |d logit|: f16 {(lg['f16'] - lg['split_bf16']).abs().max().item():.3e}, "
          f"bf16 {(lg['bf16'] - lg['split_bf16']).abs().max().item():.3e}")
    _quarter("text_emb", out["f16"][0], out["bf16"][0], out["split_bf16"][0])
    _quarter("img_emb", out["f16"][1], out["bf16"][1], out["split_bf16"][1])
    _quarter("logits", lg["f16"], lg["bf16"], lg["split_bf16"])


def _fallback_encoder(dev, heads, seed):
    from test_bf16_mode_gpu import _enc_args

    from lr2ppo_amd.tencentpretrain.encoders import str2encoder
    torch.manual_seed(seed)
    enc = str2encoder["transformer"](_enc_args(layers_num=2, hidden_size=128, emb_size=128, feedforward_size=512, heads_num=heads))
    for n, p in enc.named_parameters():
        if "gamma" not in n and "beta" not in n:
            p.data.normal_(0, 0.02)
    return enc.to(dev).eval()


def test_long_sequences_take_the_three_pass_attention(dev):
    """L = 304 > 288 at head width 64: the QKV product writes bf16 hi / lo planes, the 3-pass attention kernels run (the f16 attention's
    launch counter does not move), the context goes through round_f16; finite, and no further from the split-bf16 forward than the
    bf16 mode's result on the same case."""
    from lr2ppo_amd import ops
    enc = _fallback_encoder(dev, 2, 15)
    emb = torch.randn(2, 304, 128, device=dev, generator=torch.Generator(device=dev).manual_seed(16))
    seg = torch.ones(2, 304, dtype=torch.int64, device=dev)
    c0 = ops.self_attn_fwd_f16_launch_count()
    got = enc.forward_f16(emb, seg)
    assert ops.self_attn_fwd_f16_launch_count() == c0
    ref = enc(emb, seg)
    r16, rbf = _rel(got, ref), _rel(enc.forward_bf16(emb, seg), ref)
    print(f"\nL = 304 fallback vs split-bf16: f16 {r16:.3e}, bf16 {rbf:.3e}")
    assert torch.isfinite(got).all() and 1e-7 < r16 <= rbf


def test_head_width_32_takes_the_three_pass_attention(dev):
    """E = 128, 4 heads (head width 32): forward_bf16's zero-padded heads on the 3-pass kernels.  The split-bf16 forward refuses this head
    width, so the reference is the same encoder in plain fp64, as in tests/test_bf16_mode_gpu.py (4e-6 from the split-bf16 path where
    both exist)."""
    from lr2ppo_amd import ops
    enc = _fallback_encoder(dev, 4, 17)
    emb = torch.randn(2, 64, 128, device=dev, generator=torch.Generator(device=dev).manual_seed(18))
    seg = torch.ones(2, 64, dtype=torch.int64, device=dev)
    seg[1, 50:] = 0
    c0 = ops.self_attn_fwd_f16_launch_count()
    got = enc.forward_f16(emb, seg)
    assert ops.self_attn_fwd_f16_launch_count() == c0
    ref = _emulate(enc, emb, seg, _ident)
    r16, rbf = _rel(got, ref), _rel(enc.forward_bf16(emb, seg), ref)
    print(f"\nhead width 32 vs fp64: f16 {r16:.3e}, bf16 {rbf:.3e}")
    assert torch.isfinite(got).all() and 1e-7 < r16 <= rbf


def test_weight_refresh(dev):
    """After an in-place weight update the next forward_f16 uses fresh f16 weights: the result changes and equals a new module's with
    those weights (same kernels, same bits)."""
    from test_bf16_mode_gpu import _enc_args

    from lr2ppo_amd.tencentpretrain.encoders import str2encoder
    torch.manual_seed(21)
    enc = str2encoder["transformer"](_enc_args())
    for n, p in enc.named_parameters():
        p.data.normal_(0, 0.05) if "gamma" not in n else p.data.normal_(1.0, 0.1)
    enc = enc.to(dev).eval()
    emb = torch.randn(2, 50, 256, device=dev, generator=torch.Generator(device=dev).manual_seed(22))
    seg = torch.ones(2, 50, dtype=torch.int64, device=dev)
    y0 = enc.forward_f16(emb, seg).clone()
    assert torch.equal(enc.forward_f16(emb, seg), y0)               # cached weights: the same bits
    with torch.no_grad():
        enc.transformer[0].feed_forward.linear_1.weight.mul_(1.25)
        enc.transformer[0].self_attn.linear_layers[1].weight.add_(0.01)
    y1 = enc.forward_f16(emb, seg).clone()
    assert _rel(y1, y0) > 1e-3
    torch.manual_seed(23)
    fresh = str2encoder["transformer"](_enc_args()).to(dev).eval()
    fresh.load_state_dict(enc.state_dict())
    assert torch.equal(fresh.forward_f16(emb, seg), y1)
    assert _rel(y1, enc(emb, seg)) < 2e-3                           # ... and they are the encoder's weights
