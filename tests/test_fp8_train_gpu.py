"""MX-FP8 encoder training (FeatureExtractor(precision="mxfp8_train"), csrc/fp8_train.hip + the K-sliced product of csrc/fp8.hip):
the transposing quantiser against the OCP MX v1.0 rule restated with torch (bytes and scale bytes equal), the weight-gradient product
exact on exactly representable sums and within the MX product's bound on random data, the training schedule's gradients against the
split-bf16 schedule's (measured, printed, gated), and the public interface (routes, determinism, weight cache, fine-tune steps)."""
import argparse

import pytest
import torch

pytestmark = pytest.mark.gpu


def _ref_quant(x):
    R, K = x.shape
    xb = x.double().view(R, K // 32, 32)
    amax = xb.abs().amax(-1, keepdim=True)
    e = torch.floor(torch.log2(amax.clamp_min(1e-300))) - 8
    e = torch.where(amax < 1.17549435e-38, torch.full_like(e, -127.0), e).clamp(-127, 127)
    q = (xb * torch.exp2(-e)).clamp(-448, 448).float().to(torch.float8_e4m3fn)
    return q.view(R, K).view(torch.uint8), (e + 127).to(torch.uint8).view(R, K // 32)


def _same_bytes(got, want):
    return (got == want) | ((got & 0x7F) == 0) & ((want & 0x7F) == 0)          # +0 / -0


def _padded_t(x):
    R, C = x.shape
    Rp = -(-R // 128) * 128
    xp = torch.zeros(Rp, C, dtype=x.dtype)
    xp[:R] = x
    return xp.t().contiguous()


@pytest.mark.parametrize("R,C", [(394, 768), (4096, 256), (12544, 128)])
def test_transposing_quantiser_matches_the_mx_rule(dev, R, C):
    from lr2ppo_amd import ops
    g = torch.Generator().manual_seed(R + C)
    x = (torch.randn(R, C, generator=g) + 0.25) * torch.exp(torch.randn(1, C, generator=g) * 2)
    x[:32, 3] = 0.0                                          # an all-zero block (of x^T)
    x[40, 5] = 1e30                                          # a huge outlier
    xd = x.to(dev)
    colsum = torch.full((C,), float("nan"), device=dev)
    mt, mr, _ = ops.quant_mxfp8_t(xd, row_blocked=True, colsum=colsum)
    Rp = mt.cols
    assert Rp % 128 == 0 and Rp - R < 128 and mt.rows == C
    q_ref, s_ref = _ref_quant(_padded_t(x))
    assert torch.equal(mt.s.view(C, Rp // 32).cpu(), s_ref)
    same = _same_bytes(mt.q.view(C, Rp).cpu(), q_ref)
    assert bool(same.all()), f"{int((~same).sum())} of {C * Rp} bytes differ"
    assert bool((mt.q.view(C, Rp)[:, R:] == 0).all())                      # padding: zero bytes
    row = ops.quant_mxfp8(xd)
    assert torch.equal(mr.q[:R * C], row.q[:R * C]) and torch.equal(mr.s[:R * C // 32], row.s[:R * C // 32])
    want = x.double().sum(0)
    err = (colsum.double().cpu() - want).abs() / x.double().abs().sum(0)
    assert float(err.max()) < 1e-6, float(err.max())
    again = torch.empty_like(colsum)
    ops.quant_mxfp8_t(xd, colsum=again)
    assert torch.equal(colsum, again)
    ops.quant_mxfp8_t(xd, colsum=again, accumulate=True)
    assert torch.equal(again, colsum + colsum)
    # the planes form (what the attention backward writes) = the fp32 form of hi + lo
    pl = ops.Planes.empty(R, C, dev)
    ops.split_planes(torch.randn(R, C, generator=g).to(dev), pl)
    a, ar, _ = ops.quant_mxfp8_t(pl, row_blocked=True)
    b, br, _ = ops.quant_mxfp8_t(pl.to_float().contiguous(), row_blocked=True)
    assert torch.equal(a.q, b.q) and torch.equal(a.s, b.s) and torch.equal(ar.q, br.q) and torch.equal(ar.s, br.s)


def test_quantiser_prologues_match_torch_then_the_quantiser(dev):
    from lr2ppo_amd import ops
    g = torch.Generator().manual_seed(5)
    R, C = 394, 512
    z, dh = torch.randn(R, C, generator=g) * 2, torch.randn(R, C, generator=g)
    zd = z.to(dev)
    z64 = z.double()
    cdf = 0.5 * (1 + torch.erf(z64 / 2 ** 0.5))
    for act, val in ((1, z64 * cdf), (2, dh.double() * (cdf + z64 * torch.exp(-0.5 * z64 ** 2) / (2 * torch.pi) ** 0.5))):
        got, gr, _ = ops.quant_mxfp8_t(dh.to(dev) if act == 2 else zd, act=act, z=zd if act == 2 else None, row_blocked=True)
        ref = ops.quant_mxfp8_t(val.float().to(dev))[0]
        # the kernels' erf is a few ulp from torch's: an element may round to the neighbouring e4m3 value, nothing more
        diff = (got.to_float() - ref.to_float()).abs()
        assert float((diff > 0).float().mean()) < 2e-3
        rv = ref.to_float()
        blk = rv.abs().view(C, -1, 32).amax(-1, keepdim=True).expand(-1, -1, 32).reshape(rv.shape)
        assert bool((diff <= 0.0625 * rv.abs() + 2.0 ** -9 * blk).all())      # one e4m3 step (a subnormal one near 0)


def _int_mx(M, K, g, dev):
    from lr2ppo_amd import ops
    return ops.quant_mxfp8(torch.randint(-4, 5, (M, K), generator=g).float().to(dev))


@pytest.mark.parametrize("splits", [1, 3, 8])
def test_wgrad_product_is_exact_on_representable_sums(dev, splits):
    from lr2ppo_amd import ops
    g = torch.Generator().manual_seed(splits)
    M, N, K = 256, 384, 4096
    a, b = _int_mx(M, K, g, dev), _int_mx(N, K, g, dev)
    ws = torch.empty(splits * M * N, device=dev)
    out = torch.full((M, N), float("nan"), device=dev)
    ops.gemm_mxfp8_wgrad(a, b, out, splits=splits, workspace=ws)
    want = a.to_float().double() @ b.to_float().double().t()
    assert torch.equal(out.double(), want)
    # accumulate into a pre-filled destination whose row stride is not N; two runs, same bits
    big = torch.randn(M, N + 128, device=dev)
    dst, pre = big[:, :N], big[:, :N].clone()
    ops.gemm_mxfp8_wgrad(a, b, dst, splits=splits, workspace=ws, accumulate=True)
    assert torch.equal(dst, (pre.double() + want).float())
    out2 = torch.empty_like(out)
    ops.gemm_mxfp8_wgrad(a, b, out2, splits=splits, workspace=ws)
    assert torch.equal(out, out2)


def test_wgrad_product_on_random_data(dev):
    from lr2ppo_amd import ops
    g = torch.Generator().manual_seed(9)
    T, M, N = 12544, 768, 256
    dy, x = torch.randn(T, M, generator=g), torch.randn(T, N, generator=g) * 0.1
    at = ops.quant_mxfp8_t(dy.to(dev))[0]
    bt = ops.quant_mxfp8_t(x.to(dev))[0]
    sp = ops.mxfp8_wgrad_splits(M, N, at.cols)
    assert sp * (M // 128) * (N // 128) >= 256
    out = torch.empty(M, N, device=dev)
    ops.gemm_mxfp8_wgrad(at, bt, out, splits=sp, workspace=torch.empty(sp * M * N, device=dev))
    da, db = at.to_float().double(), bt.to_float().double()
    err = (out.double() - da @ db.t()).abs()
    bound = 2e-3 * (da.abs() @ db.abs().t()) + 1e-5
    assert bool((err <= bound).all()), f"worst excess {(err - bound).max().item():.3e}"
    out2 = torch.empty_like(out)
    ops.gemm_mxfp8_wgrad(at, bt, out2, splits=sp, workspace=torch.empty(sp * M * N, device=dev))
    assert torch.equal(out, out2)


def _fixed_blocks(x):
    """Four fixed 32-element MX blocks written into x [R, C], each once down a column (rows [0, 32) of columns 1, 3, 5, 7: a block of
    x^T, cut short by a smaller R) and once along a row (row 7 j mod R, a 32-column block behind the first one, where R and C leave
    room): amax exactly 2^3; amax = 1.9999 x 2^-5, which the shared scale takes to 511.97 > 448 (it must saturate at 448, not wrap);
    every element below FLT_MIN (scale byte 0, the values still resolved); amax = 2^127."""
    R, C = x.shape
    g = torch.Generator().manual_seed(R * 1000 + C)
    u = lambda: torch.rand(32, generator=g) * 2 - 1          # noqa: E731
    blocks = []
    for lead, rest in ((8.0, 8.0), (1.9999 * 2.0 ** -5, 2.0 ** -6), (1.1e-38, 1e-39), (2.0 ** 127, 2.0 ** 120)):
        v = u() * rest
        v[0] = lead                     # first, so that a block cut short by R < 32 still holds its amax
        blocks.append(v)
    n = min(32, R)
    used = set()
    for j, v in enumerate(blocks):
        x[:n, 2 * j + 1] = v[:n]
        spot = ((7 * j) % R, 1 + j % (C // 32 - 1))
        if spot not in used:
            used.add(spot)
            x[spot[0], 32 * spot[1]:32 * spot[1] + 32] = v
    return x


def _inside_nan(x, left, right, dev):
    """x as a column slice of a wider NaN-filled matrix on the device: row stride > cols, a 16-byte-aligned offset"""
    big = torch.full((x.shape[0], left + x.shape[1] + right), float("nan"))
    big[:, left:left + x.shape[1]] = x
    view = big.to(dev)[:, left:left + x.shape[1]]
    assert view.stride(0) > x.shape[1] and view.data_ptr() % 16 == 0
    return view


@pytest.mark.parametrize("C", [64, 192])
@pytest.mark.parametrize("R", [1, 31, 32, 33, 127, 128, 129, 394])
def test_quantiser_argument_forms_and_fixed_blocks(dev, R, C):
    """The forms of lr2_quant_mxfp8_t beside the dense fp32 one, at row counts around the 32-row block and the 128-row tile: a strided
    source, a strided z, no transposed output, planes through a prologue, accumulated column sums through an oversized workspace.
    Bytes and scale bytes equal the MX rule (or, behind a GELU prologue whose erf is the kernels' own, the dense form's)."""
    from lr2ppo_amd import ops
    g = torch.Generator().manual_seed(R * 7 + C)
    x = _fixed_blocks((torch.randn(R, C, generator=g) + 0.25) * torch.exp(torch.randn(1, C, generator=g) * 2))
    xs = _inside_nan(x, 64, 64, dev)
    Rp = -(-R // 128) * 128
    # strided source -> x^T and the row-blocked form, against the rule; padding bytes and padding scale bytes zero
    mt, mr, _ = ops.quant_mxfp8_t(xs, row_blocked=True)
    assert (mt.rows, mt.cols, mr.rows, mr.cols) == (C, Rp, R, C)
    q_ref, s_ref = _ref_quant(_padded_t(x))
    qt, st = mt.q.view(C, Rp).cpu(), mt.s.view(C, Rp // 32).cpu()
    assert torch.equal(st, s_ref)
    same = _same_bytes(qt, q_ref)
    assert bool(same.all()), f"x^T: {int((~same).sum())} of {C * Rp} bytes differ"
    assert bool((qt[:, R:] == 0).all()) and bool((st[:, -(-R // 32):] == 0).all())
    qr_ref, sr_ref = _ref_quant(x)
    assert torch.equal(mr.s.view(R, C // 32).cpu(), sr_ref)
    same = _same_bytes(mr.q.view(R, C).cpu(), qr_ref)
    assert bool(same.all()), f"rows: {int((~same).sum())} of {R * C} bytes differ"
    row = ops.quant_mxfp8(x.to(dev))
    assert torch.equal(mr.q, row.q) and torch.equal(mr.s, row.s)
    # the fixed blocks did what they are there for
    assert int(st[1, 0]) == 127 + 3 - 8 and int(st[5, 0]) == 0 and int(st[7, 0]) == 127 + 127 - 8
    assert int(qt[3, 0]) == 0x7E and int(st[3, 0]) == 127 - 5 - 8              # 1.9999 x 2^-5 -> +448, saturated
    # no transposed output: rows_out alone
    r2 = ops.Mx8.empty(R, C, dev)
    none, got, _ = ops.quant_mxfp8_t(xs, rows_out=r2, transposed=False)
    assert none is None and got is r2 and torch.equal(r2.q, mr.q) and torch.equal(r2.s, mr.s)
    # prologues, on plain data (a product with GELU'(z) beside 2^127 would overflow): x * GELU'(z) with x and z both strided = the
    # dense form; planes through GELU = the fp32 form of hi + lo
    y, z = torch.randn(R, C, generator=g), torch.randn(R, C, generator=g) * 2
    yd, ys = y.to(dev), _inside_nan(y, 64, 0, dev)
    a, ar, _ = ops.quant_mxfp8_t(yd, act=2, z=z.to(dev), row_blocked=True)
    b, br, _ = ops.quant_mxfp8_t(ys, act=2, z=_inside_nan(z, 32, 96, dev), row_blocked=True)
    assert torch.equal(a.q, b.q) and torch.equal(a.s, b.s) and torch.equal(ar.q, br.q) and torch.equal(ar.s, br.s)
    plain = ops.quant_mxfp8_t(yd)[0]
    assert not torch.equal(a.q, plain.q)
    pl = ops.Planes.empty(R, C, dev)
    ops.split_planes(yd, pl)
    a, ar, _ = ops.quant_mxfp8_t(pl, act=1, row_blocked=True)
    b, br, _ = ops.quant_mxfp8_t(pl.to_float().contiguous(), act=1, row_blocked=True)
    assert torch.equal(a.q, b.q) and torch.equal(a.s, b.s) and torch.equal(ar.q, br.q) and torch.equal(ar.s, br.s)
    assert not torch.equal(a.q, ops.quant_mxfp8_t(pl)[0].q)
    # column sums: written, then added to a prefilled vector through a workspace larger than rows_pad / 128 * cols
    written = torch.full((C,), float("nan"), device=dev)
    ops.quant_mxfp8_t(ys, colsum=written)
    err = (written.double().cpu() - y.double().sum(0)).abs()
    assert bool((err <= (R + 2) * 2.0 ** -24 * y.double().abs().sum(0)).all())      # an fp32 sum of R terms in any order
    pre = torch.randn(C, generator=g).to(dev)
    acc = pre.clone()
    used = (Rp // 128) * C
    partials = torch.full((used + 1000,), float("nan"), device=dev)
    ops.quant_mxfp8_t(ys, colsum=acc, accumulate=True, partials=partials)
    assert torch.equal(acc, pre + written)
    assert bool(torch.isfinite(partials[:used]).all()) and bool(torch.isnan(partials[used:]).all())


@pytest.mark.parametrize("splits", [1, 2, 4, 8, 64])
@pytest.mark.parametrize("M,N,K", [(128, 128, 128), (128, 256, 640), (384, 128, 1152)])
def test_wgrad_slice_counts_and_strided_destination(dev, M, N, K, splits):
    """Slice counts beyond K / 128 (capped) and ones the step count does not divide (K = 640, 4 slices asked: 3 of 2, 2 and 1 steps), the
    workspace sized for the count asked for; exact on integer operands.  The destination is the left N columns of a wider NaN-filled
    matrix: the columns beside it keep their bits, written or accumulated."""
    from lr2ppo_amd import ops
    g = torch.Generator().manual_seed(M + N + K + splits)
    a, b = _int_mx(M, K, g, dev), _int_mx(N, K, g, dev)
    want = a.to_float().double() @ b.to_float().double().t()
    assert torch.equal(want.float().double(), want)                      # integers below 2^24: fp32 holds the product exactly
    ws = torch.full((splits * M * N,), float("nan"), device=dev)
    for accumulate in (False, True):
        big = torch.full((M, N + 128), float("nan"), device=dev)
        pre = torch.randn(M, N, generator=g).to(dev)
        if accumulate:
            big[:, :N] = pre
        before = big.clone()
        ops.gemm_mxfp8_wgrad(a, b, big[:, :N], splits=splits, workspace=ws, accumulate=accumulate)
        expect = (pre.double() + want).float() if accumulate else want.float()
        assert torch.equal(big[:, :N], expect), f"accumulate={accumulate}"
        assert torch.equal(big.view(torch.int32)[:, N:], before.view(torch.int32)[:, N:]), f"accumulate={accumulate}: columns beside the destination"


def _small_encoder(pre, dev, seed, layers=2):
    from lr2ppo_amd.finetune.features import TEXT_CONFIG, VIT_CONFIG, encoder_args
    from lr2ppo_amd.tencentpretrain.encoders import str2encoder
    a = encoder_args(VIT_CONFIG if pre else TEXT_CONFIG, layers_num=layers, hidden_size=256, emb_size=256, feedforward_size=1024, heads_num=4,
                     dropout=0.1)
    g = torch.Generator().manual_seed(seed)
    enc = str2encoder["transformer"](a)
    for n, p in enc.named_parameters():
        if "gamma" in n:
            p.data.uniform_(0.8, 1.2, generator=g)
        else:
            p.data.normal_(0, 0.05, generator=g)
    return enc.to(dev).train()


def _grads(enc, fp8, emb, seg, dout):
    from lr2ppo_amd import runtime
    enc.fp8_train = fp8
    runtime.set_dropout_seed(1234)
    out, saved = enc._forward_train(emb, seg)
    demb, G = enc._backward_train(saved, dout)
    return out, demb.clone(), {n: G[p].clone() for n, p in enc.named_parameters()}


# relative L2 distance of mxfp8_train from split_bf16, measured on one MI355X with the inputs below (pre-LN, post-LN): the gates are
# 1.5 x these, capped at 0.15 (and floored at 1e-3, the print resolution of a 0.0000).  The key bias's true gradient is 0 (it shifts
# every score of a query row alike): both paths give rounding noise there, measured against the query bias's gradient.
MEASURED = {
    "output": (0.0545, 0.0596),
    "d_emb": (0.0635, 0.0702),
    "transformer.0.self_attn.linear_layers.0.weight": (0.1106, 0.1179),
    "transformer.0.self_attn.linear_layers.0.bias": (0.1120, 0.1098),
    "transformer.0.self_attn.linear_layers.1.weight": (0.1092, 0.1159),
    "transformer.0.self_attn.linear_layers.1.bias": (0.0000, 0.0000),
    "transformer.0.self_attn.linear_layers.2.weight": (0.0939, 0.1017),
    "transformer.0.self_attn.linear_layers.2.bias": (0.0814, 0.0843),
    "transformer.0.self_attn.final_linear.weight": (0.0858, 0.0971),
    "transformer.0.self_attn.final_linear.bias": (0.0642, 0.0723),
    "transformer.0.feed_forward.linear_1.weight": (0.0809, 0.0863),
    "transformer.0.feed_forward.linear_1.bias": (0.0725, 0.0715),
    "transformer.0.feed_forward.linear_2.weight": (0.0770, 0.0809),
    "transformer.0.feed_forward.linear_2.bias": (0.0537, 0.0586),
    "transformer.0.layer_norm_1.gamma": (0.0988, 0.0672),
    "transformer.0.layer_norm_1.beta": (0.0824, 0.0723),
    "transformer.0.layer_norm_2.gamma": (0.0838, 0.0614),
    "transformer.0.layer_norm_2.beta": (0.0873, 0.0586),
    "transformer.1.self_attn.linear_layers.0.weight": (0.1181, 0.1287),
    "transformer.1.self_attn.linear_layers.0.bias": (0.1018, 0.1092),
    "transformer.1.self_attn.linear_layers.1.weight": (0.1178, 0.1274),
    "transformer.1.self_attn.linear_layers.1.bias": (0.0000, 0.0000),
    "transformer.1.self_attn.linear_layers.2.weight": (0.0742, 0.0796),
    "transformer.1.self_attn.linear_layers.2.bias": (0.0612, 0.0614),
    "transformer.1.self_attn.final_linear.weight": (0.0779, 0.0834),
    "transformer.1.self_attn.final_linear.bias": (0.0461, 0.0478),
    "transformer.1.feed_forward.linear_1.weight": (0.0853, 0.0859),
    "transformer.1.feed_forward.linear_1.bias": (0.0591, 0.0590),
    "transformer.1.feed_forward.linear_2.weight": (0.0760, 0.0782),
    "transformer.1.feed_forward.linear_2.bias": (0.0116, 0.0101),
    "transformer.1.layer_norm_1.gamma": (0.0771, 0.0610),
    "transformer.1.layer_norm_1.beta": (0.0667, 0.0475),
    "transformer.1.layer_norm_2.gamma": (0.0922, 0.0580),
    "transformer.1.layer_norm_2.beta": (0.0830, 0.0000),
    "layer_norm.gamma": (0.0534, None),
    "layer_norm.beta": (0.0000, None),
}


def _gate(measured):
    return min(0.15, max(1.5 * measured, 1e-3))


@pytest.mark.parametrize("pre", [True, False])
def test_gradients_against_split_bf16(dev, pre):
    B, L = (4, 197) if pre else (4, 196)
    col = 0 if pre else 1
    enc = _small_encoder(pre, dev, 3)
    g = torch.Generator().manual_seed(4)
    emb = torch.randn(B, L, 256, generator=g).to(dev)
    seg = torch.ones(B, L, dtype=torch.int64)
    if not pre:
        seg[1, 150:] = 0
        seg[3, 40:] = 0
    seg = seg.to(dev)
    dout = torch.randn(B, L, 256, generator=g).to(dev) * 0.1
    ref_out, ref_demb, ref = _grads(enc, False, emb, seg, dout)
    out, demb, got = _grads(enc, True, emb, seg, dout)
    rel = lambda a, b: float((a - b).norm() / b.norm().clamp_min(1e-30))            # noqa: E731
    print(f"\n[mxfp8_train vs split_bf16, {'pre' if pre else 'post'}-LN] output {rel(out, ref_out):.4f}, d emb {rel(demb, ref_demb):.4f}")
    bad = [k for k, r in (("output", rel(out, ref_out)), ("d_emb", rel(demb, ref_demb))) if r > _gate(MEASURED[k][col])]
    for n in ref:
        if n.endswith("linear_layers.1.bias"):
            r = float((got[n] - ref[n]).norm() / ref[n.replace(".1.bias", ".0.bias")].norm())
            cos = 1.0
        else:
            r = rel(got[n], ref[n])
            cos = float(torch.nn.functional.cosine_similarity(got[n].flatten(), ref[n].flatten(), dim=0))
        print(f"  {n:50s} rel L2 {r:.4f}  cos {cos:.5f}  (gate {_gate(MEASURED[n][col]):.4f})")
        if r > _gate(MEASURED[n][col]) or (n.endswith("weight") and cos < 0.98):
            bad.append(n)
    assert not bad, bad
    # a second identical backward: identical bits
    _, demb2, got2 = _grads(enc, True, emb, seg, dout)
    assert torch.equal(demb, demb2) and all(torch.equal(got[n], got2[n]) for n in got)


def _qdq(x, dim):
    """x quantised to MX-FP8 with the blocks running along `dim` (the reduction axis of the product that reads it; zero padding to a
    whole block), dequantised, fp64"""
    xt = x.movedim(dim, -1)
    shp, K = xt.shape, xt.shape[-1]
    Kp = -(-K // 32) * 32
    flat = xt.reshape(-1, K)
    if Kp != K:
        flat = torch.cat([flat, flat.new_zeros(flat.shape[0], Kp - K)], 1)
    q, s = _ref_quant(flat.contiguous())
    deq = q.view(torch.float8_e4m3fn).double().view(-1, Kp // 32, 32) * torch.exp2(s.double() - 127.0).unsqueeze(-1)
    return deq.reshape(-1, Kp)[:, :K].reshape(shp).movedim(-1, dim)


class _QLinear(torch.autograd.Function):
    """y = x W^T + b as the MX-FP8 schedule computes it: forward on x and W blocked along `in`; input gradient on dY blocked along
    `out` and W blocked along `out`; weight gradient on dY and x blocked along the tokens; bias gradient unquantised."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return _qdq(x, 1) @ _qdq(w, 1).t() + b

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        return _qdq(dy, 1) @ _qdq(w, 0), _qdq(dy, 0).t() @ _qdq(x, 0), dy.sum(0)


def _emulated_layer(P, emb, seg, pre, heads, eps, drop):
    """one encoder layer (+ the pre-LN stack's final LayerNorm) in fp64: the MX-FP8 schedule's quantisation points, attention and
    LayerNorm exact, the dropout masks of the HIP kernels (oracle.lr2ppo_oracle)"""
    from oracle import lr2ppo_oracle as O
    B, L, E = emb.shape
    M, hd = B * L, E // heads
    mask = (1.0 - (seg > 0).double().view(B, 1, 1, L)) * -10000.0
    t = "transformer.0"
    ln = lambda x, k: O.layernorm_tp(x, P[f"{t}.{k}.gamma"], P[f"{t}.{k}.beta"], eps)          # noqa: E731
    lin = lambda x, k: _QLinear.apply(x, P[f"{t}.{k}.weight"], P[f"{t}.{k}.bias"])            # noqa: E731

    def attention(x):
        w = torch.cat([P[f"{t}.self_attn.linear_layers.{j}.weight"] for j in range(3)], 0)
        b = torch.cat([P[f"{t}.self_attn.linear_layers.{j}.bias"] for j in range(3)], 0)
        q, k, v = _QLinear.apply(x, w, b).view(B, L, 3, heads, hd).permute(2, 0, 3, 1, 4)
        p = torch.softmax(q @ k.transpose(-2, -1) / hd ** 0.5 + mask, dim=-1)
        o = (O._apply_dropout(p, drop, 0, pitch4=True) @ v).transpose(1, 2).reshape(M, E)
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


@pytest.mark.parametrize("pre", [True, False])
def test_schedule_against_a_torch_emulation(dev, pre):
    """Plumbing: the MX-FP8 schedule against the same quantise -> dequantise points emulated in torch (fp64 attention / LayerNorm,
    the same dropout masks).  A transposed, mis-blocked or mis-scaled operand, a wrong dropout site or a bias gradient from the wrong
    tensor is O(1).  What separates the two otherwise: the block-scaled instruction's adder tree (up to 2e-3 of the sum of |terms| per
    product, tests/test_fp8_gpu.py) and the e4m3 roundings it flips downstream.  Over 394 tokens the QKV weight gradients are sums of
    ~20x more |terms| than their result, so that alone puts them (and the pre-LN LayerNorm-1 gain fed by the same gradient) at
    1.6-2.2e-2 measured; every other tensor is at <= 9.6e-3.  Gate: 3e-2."""
    from lr2ppo_amd import runtime
    B, L = 2, 197 if pre else 196
    enc = _small_encoder(pre, dev, 11, layers=1)
    g = torch.Generator().manual_seed(12)
    emb = torch.randn(B, L, 256, generator=g)
    seg = torch.ones(B, L, dtype=torch.int64)
    if not pre:
        seg[1, 120:] = 0
    dout = torch.randn(B, L, 256, generator=g) * 0.1
    enc.fp8_train = True
    runtime.set_dropout_seed(4321)
    out, saved = enc._forward_train(emb.to(dev), seg.to(dev))
    p, seed = saved["drop"]
    demb, G = enc._backward_train(saved, dout.to(dev))
    P = {n: q.detach().double().cpu().requires_grad_() for n, q in enc.named_parameters()}
    e64 = emb.double().requires_grad_()
    ln_eps = enc.transformer[0].layer_norm_1.eps
    ref = _emulated_layer(P, e64, seg, pre, 4, ln_eps, {"p": p, "seed": seed, "site_base": 0})
    (ref * dout.double()).sum().backward()
    rel = lambda a, b: float((a.double().cpu() - b).norm() / b.norm())          # noqa: E731
    errs = {"output": rel(out, ref.detach()), "d_emb": rel(demb, e64.grad)}
    for n, q in enc.named_parameters():
        if n.endswith("linear_layers.1.bias"):      # true gradient 0: against the query bias's gradient
            errs[n] = float((G[q].double().cpu() - P[n].grad).norm() / P[n.replace(".1.bias", ".0.bias")].grad.norm())
        else:
            errs[n] = rel(G[q], P[n].grad)
    print(f"\n[mxfp8_train vs torch emulation, {'pre' if pre else 'post'}-LN] worst {max(errs.values()):.2e}")
    for n, r in errs.items():
        print(f"  {n:50s} rel L2 {r:.4e}")
    bad = [n for n, r in errs.items() if not r <= 3e-2]
    assert not bad, bad


def _fx(dev, precision):
    from lr2ppo_amd.finetune.features import TEXT_CONFIG, VIT_CONFIG, FeatureExtractor, encoder_args
    fx = FeatureExtractor(encoder_args(VIT_CONFIG, layers_num=1), encoder_args(TEXT_CONFIG, layers_num=1), precision=precision)
    fx.init_normal(generator=torch.Generator().manual_seed(8))
    return fx.to(dev)


def test_interface_routes_and_steps(dev):
    from lr2ppo_amd import runtime
    from lr2ppo_amd.finetune import ppo
    from lr2ppo_amd.finetune.features import (build_encoder_optimizer, finetune_pointwise_step, finetune_ppo_step,
                                              synthetic_raw_batch)
    fx = _fx(dev, "mxfp8_train")
    assert fx.image.encoder.fp8_train and fx.text.encoder.fp8_train
    frames, ids, seg, tgts = synthetic_raw_batch(1, 2, n_img=4, generator=torch.Generator().manual_seed(3))
    frames, ids, seg, tgts = frames.to(dev), ids.to(dev), seg.to(dev), tgts.to(dev)
    # extract() = forward_train's features with dropout off, bit for bit
    t0, i0 = fx.extract(frames, ids, seg)
    fx.eval()
    t1, i1, _ = fx.forward_train(frames, ids, seg)
    assert torch.equal(t0, t1) and torch.equal(i0, i1)
    # autograd route = explicit route, bit for bit (train mode: dropout on, same seeds)
    fx.train()
    gt = torch.randn(t0.shape, generator=torch.Generator().manual_seed(1)).to(dev) * 0.01
    gi = torch.randn(i0.shape, generator=torch.Generator().manual_seed(2)).to(dev) * 0.01
    runtime.set_dropout_seed(77)
    te, ie = fx(frames, ids, seg)
    fx.zero_grad(set_to_none=True)
    ((te * gt).sum() + (ie * gi).sum()).backward()
    auto = {n: p.grad.clone() for n, p in fx.named_parameters() if p.grad is not None}
    runtime.set_dropout_seed(77)
    te2, ie2, ctx = fx.forward_train(frames, ids, seg)
    assert torch.equal(te, te2) and torch.equal(ie, ie2)
    fx.zero_grad(set_to_none=True)
    fx.bind_grads()
    fx.backward_train(ctx, gt, gi)
    expl = {n: p.grad.clone() for n, p in fx.named_parameters()}
    enc_names = [n for n in expl if ".encoder." in n]
    assert enc_names and all(torch.equal(auto[n], expl[n]) for n in enc_names)
    # grad_flats() sizes do not depend on the precision
    ref = _fx(dev, "split_bf16")
    assert [t.numel() for t in fx.grad_flats()] == [t.numel() for t in ref.grad_flats()]
    del ref
    # the weight cache: re-quantised after an optimizer step, not otherwise
    args = argparse.Namespace(mode="reg", labels_num=3, seq_length=196, max_imgs=4, visual_feat_dim=768, is_master=True,
                              kl_div_loss_weight=0.001, entropy_weight=0.001, value_clip=0.5, optimizer="adamw", scheduler="linear",
                              learning_rate=1e-3, critic_learning_rate=1e-3, train_steps=41, warmup=0.1, device=dev)
    enc = fx.text.encoder
    n0 = enc.fp8_weight_quantisations
    fx.forward_train(frames, ids, seg)
    fx.extract(frames, ids, seg)
    assert enc.fp8_weight_quantisations == n0
    model = ppo.ActorCritic(args, None)
    ppo._init_normal(model.critic)
    model = model.to(dev)
    reward = ppo.Reward(args, None)
    ppo._init_normal(reward)
    reward = reward.to(dev).eval()
    opt, copt, sch, csch = ppo.build_optimizer(args, model)
    eopt, esch = build_encoder_optimizer(args, fx)
    sch.step(), csch.step(), esch.step()
    before = {n: p.detach().clone() for n, p in fx.named_parameters()}
    for k in range(3):
        loss = finetune_pointwise_step(args, fx, model.actor, opt, sch, eopt, esch, frames, ids, seg, tgts)
        assert torch.isfinite(loss)
    n3 = enc.fp8_weight_quantisations
    assert n0 + 2 <= n3 <= n0 + 3                                  # the forwards after the first two steps' writes (+ the last's, if any)
    fx.text.encoder._fp8_train_weights()
    assert enc.fp8_weight_quantisations in (n3, n3 + 1)
    n3 = enc.fp8_weight_quantisations
    fx.text.encoder._fp8_train_weights()
    assert enc.fp8_weight_quantisations == n3
    metrics = finetune_ppo_step(args, fx, model, reward, opt, copt, eopt, frames, ids, seg, tgts)
    assert bool(torch.isfinite(torch.as_tensor(metrics)).all())
    moved = {n for n, p in fx.named_parameters() if not torch.equal(before[n], p.detach())}
    stuck = [n for n in before if ".encoder." in n and n not in moved]
    assert not stuck, stuck
