"""The 128- and 64-row f16 product tiles (csrc/gemm.hip's F16 instantiations), lr2_gemm_f16_tiled's dispatch and row split, and the
f16 schedule under ops.f16_block_m, on a real MI355X: the short tiles against exact and fp64 references (integers, 11-bit operands a
bf16 instruction would round, the fp32 accumulation bound), their f16 plane / hi-lo planes writers byte for byte, and -- the property
the default dispatch rests on -- THE SAME BITS as the 256 x 256 kernel (csrc/gemm256_f16.hip) for every shape, tile height and
epilogue form, for the row-split seam, and for TransformerEncoder.forward_f16 / FeatureExtractor(precision="f16") under the rule
against the same call inside ops.f16_force_256()."""
import math

import pytest
import torch

from test_f16_mode_gpu import F16_MAX, U, _bits, _f16_cpu, _normal_operands

pytestmark = pytest.mark.gpu

SHAPES = [(256, 256, 64), (300, 256, 128), (257, 320, 192), (512, 264, 448), (1, 256, 64)]     # == tests/test_f16_mode_gpu.py's
BMS = [128, 64]


def test_shapes_are_the_f16_files():
    """One K step and seven; ragged M for both tile heights (300 = 2 x 128 + 44 = 4 x 64 + 44, 257, 1); ragged N against 128-wide tiles
    (320 = 2 x 128 + 64, 264 = 2 x 128 + 8)."""
    import test_f16_mode_gpu
    assert SHAPES == test_f16_mode_gpu.SHAPES


class _Counted:
    """the kernel-launch counters move by `kernels`, the accepted-calls counter by `calls`"""

    def __init__(self, ops, kernels, calls=1):
        self.ops, self.kernels, self.calls = ops, kernels, calls

    def __enter__(self):
        self.k0, self.c0 = self.ops.gemm_f16_launch_counts(), self.ops.gemm_f16_launch_count()

    def __exit__(self, *exc):
        if exc[0] is None:
            k1 = self.ops.gemm_f16_launch_counts()
            assert (k1[0] - self.k0[0], k1[1] - self.k0[1]) == self.kernels
            assert self.ops.gemm_f16_launch_count() - self.c0 == self.calls


# ---- 1-3: the product on short tiles ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bm", BMS)
@pytest.mark.parametrize("M, N, K", SHAPES)
def test_product_exact_on_integers(dev, M, N, K, bm):
    """tests/test_f16_mode_gpu.py's construction: A in [-8, 8], B in [-3, 8]; every partial sum an integer below 2^24."""
    from lr2ppo_amd import ops
    g = torch.Generator(device=dev).manual_seed(1)
    a = torch.randint(-8, 9, (M, K), device=dev, generator=g).to(torch.float16)
    b = torch.randint(-3, 9, (N, K), device=dev, generator=g).to(torch.float16)
    out = torch.full((M, N), float("nan"), device=dev)
    with _Counted(ops, (0, 1)):
        ops.gemm_f16(a, b, out, M, N, K, block_m=bm)
    assert torch.equal(out.double(), a.double() @ b.double().T)


@pytest.mark.parametrize("bm", BMS)
@pytest.mark.parametrize("M, N", [(M, N) for M, N, _ in SHAPES])
def test_product_keeps_eleven_bits(dev, M, N, bm):
    """tests/test_f16_mode_gpu.py::test_product_keeps_eleven_bits' construction at K = 64: operands 1 + j 2^-10 with j odd (exact in
    f16, not in bf16) against small integers, alternating by k; the result must EQUAL the fp64 product.  A bf16 opcode left in place in
    the short-tile kernels fails here."""
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
    assert torch.equal(a.double(), a64) and torch.equal(b.double(), b64)
    assert not torch.equal(a.to(torch.bfloat16).double(), a64)
    out = torch.full((M, N), float("nan"), device=dev)
    ops.gemm_f16(a, b, out, M, N, K, block_m=bm)
    assert torch.equal(out.double(), a64 @ b64.T)


@pytest.mark.parametrize("bm", BMS)
@pytest.mark.parametrize("M, N, K", SHAPES)
def test_product_within_the_fp32_accumulation_bound(dev, M, N, K, bm):
    """|err| <= K * 2^-24 * sum_k |a_k b_k| on normal data; then bias + GELU + residual and alpha with the tolerance expressions of
    tests/test_f16_mode_gpu.py::test_product_with_bias_gelu_residual, unchanged."""
    from lr2ppo_amd import ops
    a, b = _normal_operands(M, N, K, dev, 3)
    out = torch.full((M, N), float("nan"), device=dev)
    ops.gemm_f16(a, b, out, M, N, K, block_m=bm)
    prod = a.double() @ b.double().T
    absprod = a.double().abs() @ b.double().abs().T
    err = (out.double() - prod).abs()
    print(f"\n{M}x{N}x{K} f16 bm={bm}: max err / bound = {(err / (K * U * absprod).clamp_min(1e-300)).max().item():.3e}")
    assert (err <= K * U * absprod).all()
    g = torch.Generator(device=dev).manual_seed(5)
    bias = torch.randn(N, device=dev, generator=g)
    resid = torch.randn(M, N, device=dev, generator=g)
    out.fill_(float("nan"))
    ops.gemm_f16(a, b, out, M, N, K, bias=bias, act=1, resid=resid, block_m=bm)
    z = prod + bias.double()
    gz = 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))
    ref = gz + resid.double()
    zb = K * U * absprod + 2 * U * z.abs()
    tol = 1.13 * zb + 3e-7 * z.abs() + 4 * U * (gz.abs() + z.abs()) + 2 * U * (resid.double().abs() + ref.abs())
    err = (out.double() - ref).abs()
    print(f"{M}x{N}x{K} f16 bm={bm} bias+GELU+resid: max err / tol = {(err / tol).max().item():.3e}")
    assert (err <= tol).all()
    out.fill_(float("nan"))
    ops.gemm_f16(a, b, out, M, N, K, bias=bias, resid=resid, alpha=0.5, block_m=bm)
    ref = 0.5 * prod + bias.double() + resid.double()
    tol = 0.5 * K * U * absprod + 4 * U * (ref.abs() + resid.double().abs() + bias.double().abs())
    assert ((out.double() - ref).abs() <= tol).all()


# ---- 4: the plane outputs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bm", BMS)
@pytest.mark.parametrize("M, N, K", SHAPES)
def test_plane_is_rne_f16_of_the_fp32_result_at_three_scales(dev, M, N, K, bm):
    """The f16 plane of a both-outputs launch and of a plane-only launch == out.to(float16) byte for byte at the data's own scale (with
    and without GELU), with alpha driving the results into the f16 subnormal range, and with alpha driving them past 65504: the plane
    saturates to +-65504 (0x7BFF / 0xFBFF), never Inf, and the fp32 output keeps the value.  Nothing is written behind the plane."""
    from lr2ppo_amd import ops
    a, b = _normal_operands(M, N, K, dev, 6)
    bias = torch.randn(N, device=dev, generator=torch.Generator(device=dev).manual_seed(7))
    for act, alpha, use_bias in ((0, 1.0, True), (1, 1.0, True), (0, 2e-6, False), (0, 3e-7, False), (0, 1e5, False)):
        out = torch.full((M, N), float("nan"), device=dev)
        both = torch.zeros(M * N + 8, dtype=torch.float16, device=dev)
        alone = torch.zeros(M * N + 8, dtype=torch.float16, device=dev)
        kw = dict(bias=bias if use_bias else None, act=act, alpha=alpha, block_m=bm)
        ops.gemm_f16(a, b, out, M, N, K, out_plane=both, **kw)
        ops.gemm_f16(a, b, None, M, N, K, out_plane=alone, **kw)
        assert torch.isfinite(out).all()
        mag = out.abs()
        if alpha < 1e-3:
            assert ((mag > 1e-7) & (mag < 6e-5)).float().mean().item() > 0.5          # the case is about subnormal results
        if alpha > 1e3:
            assert (mag > F16_MAX).float().mean().item() > 0.5                        # ... about saturation
            assert torch.isfinite(both).all() and torch.isfinite(alone).all()         # no Inf
            assert (both[:M * N].view(M, N)[mag > F16_MAX].abs() == F16_MAX).all()
        want = _f16_cpu(out.clamp(-F16_MAX, F16_MAX))              # (65504, 65520) rounds to 65504 anyway; beyond it the writer clamps
        assert torch.equal(_bits(both[:M * N]).cpu(), want), (act, alpha)
        assert torch.equal(_bits(alone[:M * N]).cpu(), want), (act, alpha)
        assert (both[M * N:] == 0).all() and (alone[M * N:] == 0).all()


@pytest.mark.parametrize("bm", BMS)
@pytest.mark.parametrize("M, K", [(300, 128), (1, 64), (129, 192)])
def test_hi_lo_planes_into_a_wider_matrix_at_head_width_32(dev, M, K, bm):
    """N = 32 with planes_col = 8 into a [M, 48] planes matrix (the head-width-32 fallback's product): hi + lo is the split of the fp32
    result; the columns outside [8, 40) and four canary rows behind M keep their bytes, in both planes."""
    from lr2ppo_amd import ops
    N, W, R = 32, 48, 4
    a, b = _normal_operands(M, N, K, dev, 9)
    bias = torch.randn(N, device=dev, generator=torch.Generator(device=dev).manual_seed(10))
    CAN = 0x5A5A
    buf = torch.full((2 * (M + R) * W,), CAN, dtype=torch.int16, device=dev)
    pl = ops.Planes(buf, M, W, lo_off=(M + R) * W)
    out = torch.full((M, N), float("nan"), device=dev)
    ops.gemm_f16(a, b, out, M, N, K, bias=bias, block_m=bm)
    ops.gemm_f16(a, b, None, M, N, K, bias=bias, out_planes=pl, planes_col=8, block_m=bm)
    hi = out.to(torch.bfloat16)
    lo = (out - hi.float()).to(torch.bfloat16)
    planes = buf.view(2, M + R, W)
    assert torch.equal(planes[0, :M, 8:40], hi.view(torch.int16))
    assert torch.equal(planes[1, :M, 8:40], lo.view(torch.int16))
    assert (planes[:, :M, :8] == CAN).all() and (planes[:, :M, 40:] == CAN).all() and (planes[:, M:, :] == CAN).all()


@pytest.mark.parametrize("bm", BMS)
@pytest.mark.parametrize("M, N, K", SHAPES)
def test_non_tight_leading_dimensions(dev, M, N, K, bm):
    """lda / ldb / ld_out from tests/gemm_cases.py::strides, two NaN rows behind A and behind B inside the extents the call may address
    (a ragged tile loads them: they may only reach accumulator rows that are never stored), NaN in the padding columns; canary columns
    and rows of the fp32 result untouched; integers: exact."""
    import gemm_cases as GC

    from lr2ppo_amd import ops
    st = GC.strides(M, N, K, "NT")
    g = torch.Generator(device=dev).manual_seed(11)
    a = torch.full((M + 2, st.lda), float("nan"), dtype=torch.float16, device=dev)
    b = torch.full((N + 2, st.ldb), float("nan"), dtype=torch.float16, device=dev)
    a[:M, :K] = torch.randint(-8, 9, (M, K), device=dev, generator=g).to(torch.float16)
    b[:N, :K] = torch.randint(-3, 9, (N, K), device=dev, generator=g).to(torch.float16)
    bias = torch.randint(-9, 10, (N,), device=dev, generator=g).float()
    out = torch.full((M + 2, st.ld_out), -77.0, device=dev)
    plane = torch.zeros(M * N + 8, dtype=torch.float16, device=dev)
    ops.gemm_f16(a.view(-1), b.view(-1), out, M, N, K, lda=st.lda, ldb=st.ldb, ld_out=st.ld_out, bias=bias, out_plane=plane, block_m=bm)
    ref = a[:M, :K].double() @ b[:N, :K].double().T + bias.double()
    assert torch.equal(out[:M, :N].double(), ref)
    assert (out[:M, N:] == -77.0).all() and (out[M:] == -77.0).all()
    assert torch.equal(_bits(plane[:M * N]).cpu(), _f16_cpu(out[:M, :N].contiguous())) and (plane[M * N:] == 0).all()


# ---- 5: the same bits as the 256 x 256 kernel ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bm", BMS)
@pytest.mark.parametrize("M, N, K", SHAPES)
def test_same_bits_as_the_256_kernel(dev, M, N, K, bm):
    """Both kernels run each accumulator through k in ascending 32-wide MFMA steps and share the epilogue code: with bias + GELU and
    with bias + residual, on normal data, the fp32 output and the plane bytes of block_m = 128 / 64 equal those of block_m = None
    (lr2_gemm_f16: the 256 x 256 kernel, 192-row form included).  What lets the schedule follow f16_block_m by default."""
    from lr2ppo_amd import ops
    a, b = _normal_operands(M, N, K, dev, 12)
    g = torch.Generator(device=dev).manual_seed(13)
    bias = torch.randn(N, device=dev, generator=g)
    resid = torch.randn(M, N, device=dev, generator=g)
    for kw in (dict(bias=bias, act=1), dict(bias=bias, resid=resid), dict(alpha=0.37)):
        got, want = [], []
        for dst, block_m in ((want, None), (got, bm)):
            out = torch.full((M, N), float("nan"), device=dev)
            plane = torch.zeros(M * N, dtype=torch.float16, device=dev)
            with _Counted(ops, (1, 0) if block_m is None else (0, 1)):
                ops.gemm_f16(a, b, out, M, N, K, out_plane=plane, block_m=block_m, **kw)
            dst += [out, plane]
        assert torch.isfinite(want[0]).all()
        assert torch.equal(got[0], want[0]), sorted(kw)
        assert torch.equal(_bits(got[1]), _bits(want[1])), sorted(kw)
    pw, pg = ops.Planes.empty(M, N, dev), ops.Planes.empty(M, N, dev)       # hi / lo planes: QKV in front of the 3-pass attention
    ops.gemm_f16(a, b, None, M, N, K, bias=bias, out_planes=pw)
    ops.gemm_f16(a, b, None, M, N, K, bias=bias, out_planes=pg, block_m=bm)
    assert torch.equal(pw.buf, pg.buf)


# ---- 6: the row split ----------------------------------------------------------------------------------------------------------------
def test_row_split_seam(dev):
    """ops.gemm_f16(block_m = 256) at gemm_cases.SEAM: 32 768 rows on the 256 x 256 kernel, 200 on 64-row tiles (one launch each, one
    accepted call).  Integer operands, bias and residual: exact across the seam; the f16 plane is RNE of the fp32 result on both sides
    of row 32 768; canary rows behind the result and elements behind the plane intact; and the split changes no bit against the
    unsplit 256 x 256 launch (block_m = None)."""
    import ctypes

    import gemm_cases as GC

    from lr2ppo_amd import _native, ops
    M, N, K = GC.SEAM
    M1, bm2 = GC.row_split_plan(M, N, K)
    r, t = ctypes.c_int(0), ctypes.c_int(0)
    assert _native.lib().lr2_gemm_row_split_plan(M, N, K, ctypes.byref(r), ctypes.byref(t)) == 0
    assert (M1, bm2) == (32768, 64) == (r.value, t.value)
    g = torch.Generator(device=dev).manual_seed(14)
    a = torch.randint(-8, 9, (M, K), device=dev, generator=g).to(torch.float16)
    b = torch.randint(-3, 9, (N, K), device=dev, generator=g).to(torch.float16)
    a[M1 - 1], a[M1] = 7.0, -8.0                                  # distinct rows on either side of the seam
    bias = torch.randint(-9, 10, (N,), device=dev, generator=g).float()
    resid = (torch.randint(-9, 10, (M, N), device=dev, generator=g) + (torch.arange(M, device=dev).view(-1, 1) % 5)).float()
    out = torch.full((M + 2, N), -77.0, device=dev)
    plane = torch.zeros(M * N + 8, dtype=torch.float16, device=dev)
    with _Counted(ops, (1, 1)):
        ops.gemm_f16(a, b, out, M, N, K, bias=bias, resid=resid, out_plane=plane, block_m=256)
    ref = a.double() @ b.double().T + bias.double() + resid.double()
    assert torch.equal(out[:M1].double(), ref[:M1]), "rows of the 256 x 256 launch"
    assert torch.equal(out[M1:M].double(), ref[M1:]), "rows of the short-tile launch"
    assert (out[M:] == -77.0).all()
    want = out[:M].to(torch.float16).view(-1)
    assert torch.equal(_bits(plane[:M1 * N]), _bits(want[:M1 * N])) and torch.equal(_bits(plane[M1 * N:M * N]), _bits(want[M1 * N:]))
    assert (plane[M * N:] == 0).all()
    out0 = torch.full((M, N), float("nan"), device=dev)
    with _Counted(ops, (1, 0)):
        ops.gemm_f16(a, b, out0, M, N, K, bias=bias, resid=resid)
    assert torch.equal(out0, out[:M])


# ---- 7: the schedule -----------------------------------------------------------------------------------------------------------------
def _encoder(dev, heads, placement, seed):
    from test_bf16_mode_gpu import _enc_args

    from lr2ppo_amd.tencentpretrain.encoders import str2encoder
    torch.manual_seed(seed)
    enc = str2encoder["transformer"](_enc_args(layers_num=2, hidden_size=128, emb_size=128, feedforward_size=512, heads_num=heads,
                                               layernorm_positioning=placement))
    for n, p in enc.named_parameters():
        if "gamma" not in n and "beta" not in n:
            p.data.normal_(0, 0.05)
    return enc.to(dev).eval()


@pytest.mark.parametrize("placement", ["pre", "post"])
@pytest.mark.parametrize("heads", [2, 4])
def test_schedule_under_the_rule_equals_the_forced_256_schedule(dev, heads, placement):
    """Two layers, E = 128, head width 64 (2 heads) and 32 (4 heads: the zero-padded per-head products), B = 2, L = 16: forward_f16
    under f16_block_m == forward_f16 inside f16_force_256() bit for bit, first_only included; the launch counters show the short tiles
    ran under the rule and only the 256 x 256 kernel inside the block; both make the same number of product calls."""
    from lr2ppo_amd import ops
    enc = _encoder(dev, heads, placement, 20 + heads)
    assert enc.layernorm_positioning == placement
    emb = torch.randn(2, 16, 128, device=dev, generator=torch.Generator(device=dev).manual_seed(21))
    seg = torch.ones(2, 16, dtype=torch.int64, device=dev)
    seg[1, 11:] = 0
    for first_only in (False, True):
        k0, c0 = ops.gemm_f16_launch_counts(), ops.gemm_f16_launch_count()
        got = enc.forward_f16(emb, seg, first_only=first_only).clone()
        k1, c1 = ops.gemm_f16_launch_counts(), ops.gemm_f16_launch_count()
        with ops.f16_force_256():
            want = enc.forward_f16(emb, seg, first_only=first_only).clone()
        k2, c2 = ops.gemm_f16_launch_counts(), ops.gemm_f16_launch_count()
        assert k1[1] - k0[1] > 0 and k1[0] == k0[0], "the rule sends these small products to the short tiles"
        assert k2[1] == k1[1] and k2[0] - k1[0] == c2 - c1 == c1 - c0, "inside the block: lr2_gemm_f16 only, call for call"
        assert torch.isfinite(want).all() and want.shape == ((2, 128) if first_only else (2, 16, 128))
        assert torch.equal(got, want), (heads, placement, first_only)
    assert ops.f16_schedule_block_m(32, 128, 128) == ops.f16_block_m(32, 128, 128)              # the block has ended


def test_feature_extractor_matches_its_forced_256_twin(dev):
    """FeatureExtractor(precision="f16").extract on the small config (two-layer towers, E = 256) under the rule == inside
    f16_force_256(), bit for bit, and the short tiles ran."""
    from test_bf16_mode_gpu import _small_extractor

    from lr2ppo_amd import ops
    from lr2ppo_amd.finetune.features import synthetic_raw_batch
    fx = _small_extractor(dev)
    fx.precision = "f16"
    frames, ids, seg, _ = synthetic_raw_batch(2, 2, n_img=4, device=dev, generator=torch.Generator(device=dev).manual_seed(14))
    k0 = ops.gemm_f16_launch_counts()
    t1, i1 = (x.clone() for x in fx.extract(frames, ids, seg))
    k1 = ops.gemm_f16_launch_counts()
    with ops.f16_force_256():
        t0, i0 = (x.clone() for x in fx.extract(frames, ids, seg))
    k2 = ops.gemm_f16_launch_counts()
    assert k1[1] > k0[1] and k2[1] == k1[1] and k2[0] > k1[0]
    assert torch.isfinite(t1).all() and torch.isfinite(i1).all()
    assert torch.equal(t1, t0) and torch.equal(i1, i0)
