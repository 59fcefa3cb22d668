"""Edge suite of the MX-FP8 family on a real MI355X: the scale-and-round rule of every producer (the stand-alone quantiser, the
row- / column-blocked training quantiser, LayerNorm, the epilogues of the 128 x 128 and of the 256 x 256 ring product, the one-pair,
the persistent and the key-blocked attention) on the edge blocks of tests/mx_cases.py, byte for byte against the rule restated on the
CPU (mx_cases.ref_quant: no float8 cast), and the small product kernels (lr2_gemm_mxfp8 below the ring, lr2_gemm_mxfp8_wgrad) on
exact integers, strides, canaries, extreme operand scales and refusals.

The reference is always the rule applied to the fp32 values that reached the quantiser.  Where a launch also emits fp32, that output
is first asserted equal to the planted values (==, NaN positions matching) and its census (mx_cases.census) is asserted, so a producer
that did not receive the edges cannot pass quietly; then every byte and every scale byte is compared (the sign of a zero byte and the
byte of a NaN element are not the rule's: for those, every producer must give what every other gives --
test_producers_agree_where_the_rule_does_not_decide)."""
import functools
import math

import pytest
import torch

import mx_cases as MC

pytestmark = pytest.mark.gpu

NAN = float("nan")
OUTCOMES = {}             # producer -> {one of KEYS: set of bytes}
CASES = {}                # producer -> launches compared
PRODUCERS = ["quant_mxfp8", "quant_mxfp8_t rows", "quant_mxfp8_t columns", "layernorm_fwd_mxfp8", "gemm_mxfp8 128", "gemm_mxfp8 ring",
             "self_attn_fwd_bf16 one pair", "self_attn_fwd_bf16 persistent", "self_attn_fwd_bf16_blocked"]


@pytest.fixture(scope="module")
def ops(dev):
    from lr2ppo_amd import ops as _ops
    return _ops


@functools.lru_cache(maxsize=None)
def edge(rows, width, start=0, full=None, bf16=False, exact_planes=False):
    """(E [rows, 32 * width], block index [rows, width], blocks, reference, census counts): computed once per layout, never changed."""
    blocks = MC.BLOCKS_BF16 if bf16 else MC.BLOCKS
    if exact_planes:
        blocks = [b for b in blocks if MC.splits_exactly(b.vals)]
    x, idx = MC.lay(blocks, rows, width, start, full)
    return x, idx, blocks, MC.ref_quant(x), MC.census_counts(MC.census(x))


def has_edges(cen):
    """Census counts of a matrix that carries the whole list: every tie at three scales in both signs, a maximum at every position,
    saturating values in every slot (three amax >= 449 that planes hold exactly x 4 elements x 3 scales)."""
    return cen[0] >= 3 * 2 * 126 and min(cen[5]) >= 1 and cen[2] >= 36


def eq_nan(a, b):
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def mx_dest(ops, M, N, dev, extra=MC.XROWS):
    """Mx8 [M, N] at the head of sentinel allocations of M + 3 rows."""
    q = torch.full(((M + extra) * N,), MC.SENT8, dtype=torch.uint8, device=dev)
    s = torch.full(((M + extra) * (N // 32),), MC.SENT8, dtype=torch.uint8, device=dev)
    return ops.Mx8(q, s, M, N)


def mx_tail_ok(mx):
    return bool((mx.q[mx.rows * mx.cols:] == MC.SENT8).all()) and bool((mx.s[mx.rows * (mx.cols // 32):] == MC.SENT8).all())


def mx_cpu(mx):
    return mx.q[:mx.rows * mx.cols].view(mx.rows, mx.cols).cpu(), mx.s[:mx.rows * (mx.cols // 32)].view(mx.rows, mx.cols // 32).cpu()


KEYS = ("nan", "+0", "-0", "+inf", "-inf", "+round0", "-round0")


def record(producer, x, q, ref, signs):
    """What the producer made of the inputs the rule leaves open: NaN, +0, -0, and non-zero values that round to a zero byte (its sign);
    +-Inf beside them (the rule says +-448).  signs=False: x is what was planted, behind an addition (0 + bias, + residual) that the
    launch did not emit as fp32 -- a planted -0 reached the quantiser as +0, so the zeros of x are not recorded."""
    bits = x.contiguous().view(torch.int32)
    o = OUTCOMES.setdefault(producer, {})
    r0 = ((ref.q & 0x7F) == 0) & ~ref.free
    for key, mask in (("nan", torch.isnan(x)), ("+0", bits == 0), ("-0", bits == -2 ** 31), ("+inf", x == math.inf), ("-inf", x == -math.inf),
                      ("+round0", r0 & (x > 0)), ("-round0", r0 & (x < 0))):
        if signs or key not in ("+0", "-0"):
            o.setdefault(key, set()).update(q[mask].unique().tolist())
        else:
            o.setdefault(key, set())
    CASES[producer] = CASES.get(producer, 0) + 1


def check(producer, mx, x, idx=None, blocks=None, ref=None, signs=True):
    """Every scale byte and every byte of mx (an Mx8, or a (q, s) pair of CPU tensors) against the rule applied to x (CPU fp32)."""
    q, s = mx_cpu(mx) if hasattr(mx, "rows") else mx
    ref = ref or MC.ref_quant(x)

    def where(r, b):
        return f"block ({r}, {b})" + (f" [{blocks[int(idx[r, b])].name}]" if idx is not None and r < idx.shape[0] and b < idx.shape[1] else "")

    bad = (s != ref.s).nonzero()
    if len(bad):
        r, b = bad[0].tolist()
        raise AssertionError(f"{producer}: {len(bad)} of {s.numel()} scale bytes differ; first at {where(r, b)}: got {int(s[r, b])}, "
                             f"rule {int(ref.s[r, b])}")
    bad = (~MC.same_bytes(q, ref)).nonzero()
    if len(bad):
        r, k = bad[0].tolist()
        raise AssertionError(f"{producer}: {len(bad)} of {q.numel()} bytes differ; first at {where(r, k // 32)} element {k % 32}: "
                             f"x {float(x[r, k])!r} got 0x{int(q[r, k]):02X}, rule 0x{int(ref.q[r, k]):02X}")
    record(producer, x, q, ref, signs)


# ---- 1. lr2_quant_mxfp8 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 3, 17])
@pytest.mark.parametrize("strided", [False, True], ids=["tight", "strided"])
def test_quantiser_on_the_edge_blocks(ops, dev, R, strided):
    W = MC.rows_for(MC.BLOCKS, R)
    x, idx, blocks, ref, cen = edge(R, W)
    K = 32 * W
    assert has_edges(cen) and cen[3] >= 3 and cen[4] >= 3
    if strided:
        buf = torch.full((R + 1, MC.leading_dims(K, K)["ldx"]), NAN)
        buf[:R, :K] = x
        xd = buf.to(dev)[:R, :K]
        assert xd.stride(0) == K + 8
    else:
        xd = x.to(dev)
    dst = mx_dest(ops, R, K, dev)
    ops.quant_mxfp8(xd, dst)
    check("quant_mxfp8", dst, x, idx, blocks, ref)
    assert mx_tail_ok(dst)
    assert eq_nan(xd.cpu(), x)                                # the input is not written


# ---- 2. lr2_quant_mxfp8_t -----------------------------------------------------------------------------------------------------------
def planes_input(ops, x, dev):
    """(Planes whose hi + lo is x, hi + lo as the kernel forms it: x itself but for -0, whose lo plane is +0 and whose sum is +0)."""
    hi, lo = MC.planes_of(x)
    eff = hi.float() + lo.float()
    assert torch.equal(eff, x)
    buf = torch.cat([hi.view(torch.int16).flatten(), lo.view(torch.int16).flatten()]).to(dev)
    return ops.Planes(buf, x.shape[0], x.shape[1]), eff


@pytest.mark.parametrize("rows", [40, 128, 200])
@pytest.mark.parametrize("kind", ["fp32", "planes"])
def test_training_quantiser_row_blocked(ops, dev, rows, kind):
    pl = kind == "planes"
    nb = len(edge(1, 1, exact_planes=pl)[2])
    W = 2 * -(-nb // (2 * rows))                             # cols % 64 == 0
    x, idx, blocks, ref, cen = edge(rows, W, exact_planes=pl)
    assert rows * W >= nb and has_edges(cen)
    ro = mx_dest(ops, rows, 32 * W, dev)
    xin, x = planes_input(ops, x, dev) if pl else (x.to(dev), x)
    ops.quant_mxfp8_t(xin, rows_out=ro, transposed=False)
    check("quant_mxfp8_t rows", ro, x, idx, blocks, ref)
    assert mx_tail_ok(ro)


@pytest.mark.parametrize("rows", [40, 128, 200])
@pytest.mark.parametrize("kind", ["fp32", "planes"])
def test_training_quantiser_column_blocked(ops, dev, rows, kind):
    """x = E^T: the blocks run down the columns of x.  rows is no multiple of 128 (40, 200: not of 32 either), so the last block of a
    column is partly or wholly padding: zero bytes, scale byte 0 where all of it is."""
    pl = kind == "planes"
    nb = len(edge(1, 1, exact_planes=pl)[2])
    full, Wt = rows // 32, -(-rows // 32)
    cols = 64 * -(-nb // (64 * full))
    et, idx, blocks, _, _ = edge(cols, Wt, full=full, exact_planes=pl)
    x = et[:, :rows].t().contiguous()                        # [rows, cols]
    xin, x = planes_input(ops, x, dev) if pl else (None, x)
    rows_pad = -(-rows // 128) * 128
    want = torch.zeros(cols, rows_pad)
    want[:, :rows] = x.t()
    cen = MC.census_counts(MC.census(want))
    assert has_edges(cen) and cen[3] >= cols * (rows_pad - 32 * Wt) // 32
    dst = mx_dest(ops, cols, rows_pad, dev)
    if pl:
        ops.quant_mxfp8_t(xin, dst=dst)
    else:
        buf = torch.full((rows + 1, cols + 8), NAN)          # strided rows, NaN in the pad columns and behind the last row
        buf[:rows, :cols] = x
        ops.quant_mxfp8_t(buf.to(dev)[:rows, :cols], dst=dst)
    check("quant_mxfp8_t columns", dst, want, idx, blocks)
    q, s = mx_cpu(dst)
    assert bool((s[:, Wt:] == 0).all()) and bool((q[:, rows:] == 0).all())
    assert mx_tail_ok(dst)


# ---- 3. lr2_layernorm_fwd_mxfp8 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 768, 1024])
@pytest.mark.parametrize("mode", [0, 1])
def test_layernorm_output_on_the_edge_blocks(ops, dev, D, mode):
    """gamma = 0: the row that reaches the quantiser is beta, a row of edge blocks (one launch per row of E; 5 token rows each -- two
    workgroups, the second with one row)."""
    W = D // 32
    R = MC.rows_for(MC.BLOCKS, W)
    x, idx, blocks, ref, cen = edge(R, W)
    assert has_edges(cen)
    rows = 5
    g = torch.Generator().manual_seed(D + mode)
    xin = (torch.randn(rows, D, generator=g) * 3).to(dev)
    gamma, beta = torch.zeros(D, device=dev), x.to(dev)
    got = [(mx_dest(ops, rows, D, dev), torch.full((rows, D), NAN, device=dev)) for _ in range(R)]
    for r in range(R):
        ops.layernorm_fwd_mxfp8(xin, gamma, beta[r], got[r][0], got[r][1], rows=rows, D=D, eps=1e-6, mode=mode)
    out32 = torch.stack([o for _, o in got]).cpu()                                   # [R, rows, D]
    assert eq_nan(out32, x.view(R, 1, D).expand(R, rows, D)), "the fp32 output is not beta"
    qs = [mx_cpu(m) for m, _ in got]
    assert MC.census_counts(MC.census(out32[:, 0].contiguous())) == cen
    for t in range(rows):
        check("layernorm_fwd_mxfp8", (torch.stack([q[t] for q, _ in qs]), torch.stack([s[t] for _, s in qs])), out32[:, t].contiguous(), idx,
              blocks, ref)
    assert all(mx_tail_ok(m) for m, _ in got)


# ---- 4. the 128 x 128 product's epilogue --------------------------------------------------------------------------------------------
def zero_a(ops, M, K, dev):
    return ops.Mx8(torch.zeros(M * K, dtype=torch.uint8, device=dev), torch.full((M * (K // 32),), 127, dtype=torch.uint8, device=dev), M, K)


def some_b(ops, N, K, dev):
    g = torch.Generator().manual_seed(N + K)
    return ops.quant_mxfp8((torch.randn(N, K, generator=g) * 3).to(dev))


def planes_dest(ops, M, N, dev):
    n = (M + MC.XROWS) * N
    buf = torch.full((2 * n + 8,), MC.PAT16, dtype=torch.int16, device=dev)
    return ops.Planes(buf, M, N, lo_off=n + 8), n


def check_planes(pl, n, x):
    """hi / lo planes of the emitted row: the RNE split on every finite element; nothing outside [0:M, 0:N] of either plane."""
    M, N = x.shape
    buf = pl.buf.cpu()
    hi, lo = MC.planes_of(x)
    fin = torch.isfinite(x) & torch.isfinite(hi.float())
    got_hi, got_lo = buf[:M * N].view(M, N).view(torch.bfloat16).float(), buf[n + 8:n + 8 + M * N].view(M, N).view(torch.bfloat16).float()
    assert torch.equal(got_hi[fin], hi.float()[fin]) and torch.equal(got_lo[fin], lo.float()[fin]), "planes != the RNE split of the row"
    assert bool((buf[M * N:n + 8] == MC.PAT16).all()) and bool((buf[n + 8 + M * N:] == MC.PAT16).all())


@pytest.mark.parametrize("M", [1, 65, 130])
@pytest.mark.parametrize("dests", ["out", "mx", "planes", "out+mx", "out+mx+planes"])
def test_product_epilogue_quantises_the_residual_row(ops, dev, M, dests):
    """A = 0 (zero bytes, scale 2^0), act 0, no bias: what the epilogue stores and quantises is the residual, E; strided out and resid,
    NaN in resid's pad columns."""
    N, K = 256, 128
    assert not MC.takes_ring(M, N, K)
    x, idx, blocks, ref, cen = edge(M, N // 32)
    if M >= 65:
        assert has_edges(cen)
    ld = MC.leading_dims(K, N)
    rbuf = torch.full((M + 1, ld["ld_resid"]), NAN)
    rbuf[:M, :N] = x
    resid = rbuf.to(dev)[:M, :N]
    obuf = torch.full((M + MC.XROWS, ld["ld_out"]), MC.PAT32, dtype=torch.int32, device=dev).view(torch.float32)
    out = obuf[:M, :N] if "out" in dests else None
    mx = mx_dest(ops, M, N, dev) if "mx" in dests else None
    pl, n = planes_dest(ops, M, N, dev) if "planes" in dests else (None, 0)
    ops.gemm_mxfp8(zero_a(ops, M, K, dev), some_b(ops, N, K, dev), out, resid=resid, act=0, out_mx=mx, out_planes=pl)
    emitted = x
    if out is not None:
        emitted = out.cpu().contiguous()
        assert eq_nan(emitted, x), "the fp32 output is not the residual"
        assert MC.census_counts(MC.census(emitted)) == cen
        v = obuf.view(torch.int32).clone()
        v[:M, :N] = MC.PAT32
        assert bool((v == MC.PAT32).all()), "out written outside [0:M, 0:N]"
    if mx is not None:
        check("gemm_mxfp8 128", mx, emitted, idx, blocks, signs=out is not None)
        assert mx_tail_ok(mx), "out_mx written past row M"
    if pl is not None:
        check_planes(pl, n, x)


def test_product_epilogue_quantises_the_bias_row(ops, dev):
    """The same with bias = a row of edge blocks and no residual (one launch per 8 blocks): every row of the result is the bias."""
    M, N, K = 65, 256, 128
    R = MC.rows_for(MC.BLOCKS, N // 32)
    x, idx, blocks, ref, cen = edge(R, N // 32)
    a, b, bias = zero_a(ops, M, K, dev), some_b(ops, N, K, dev), x.to(dev)
    got = [(mx_dest(ops, M, N, dev), torch.full((M, N), NAN, device=dev)) for _ in range(R)]
    for r in range(R):
        ops.gemm_mxfp8(a, b, got[r][1], bias=bias[r], act=0, out_mx=got[r][0])
    out = torch.stack([o for _, o in got]).cpu()
    assert eq_nan(out, x.view(R, 1, N).expand(R, M, N)), "the fp32 output is not the bias"
    qs = [mx_cpu(m) for m, _ in got]
    for t in (0, 31, 63, 64):
        emitted = out[:, t].contiguous()
        assert MC.census_counts(MC.census(emitted)) == cen
        check("gemm_mxfp8 128", (torch.stack([q[t] for q, _ in qs]), torch.stack([s[t] for _, s in qs])), emitted, idx, blocks)
    for q, s in qs:
        assert bool((q == q[0]).all()) and bool((s == s[0]).all())
    assert all(mx_tail_ok(m) for m, _ in got)


# ---- 5. the ring kernel's epilogue --------------------------------------------------------------------------------------------------
RM, RN, RK = MC.RING_SHAPES[0]


def rows_all_equal(mx):
    q, s = mx.q[:mx.rows * mx.cols].view(mx.rows, mx.cols), mx.s[:mx.rows * (mx.cols // 32)].view(mx.rows, mx.cols // 32)
    return bool((q == q[0]).all()) and bool((s == s[0]).all())


def test_ring_epilogue_quantises_the_bias_row_in_its_straight_line_form(ops, dev):
    """out_mx only, act 0: the straight-line MX form.  Every row is the bias, 64 edge blocks per launch."""
    assert MC.takes_ring(RM, RN, RK)
    a, b = zero_a(ops, RM, RK, dev), some_b(ops, RN, RK, dev)
    seen = torch.zeros(6 + 32, dtype=torch.long)
    for start in (0, 64, 128):
        x, idx, blocks, ref, cen = edge(1, RN // 32, start)
        mx = mx_dest(ops, RM, RN, dev)
        ops.gemm_mxfp8(a, b, None, bias=x[0].to(dev), act=0, out_mx=mx)
        assert rows_all_equal(mx) and mx_tail_ok(mx)
        q, s = mx.q[:RN].view(1, RN).cpu(), mx.s[:RN // 32].view(1, RN // 32).cpu()
        check("gemm_mxfp8 ring", (q, s), x, idx, blocks, ref, signs=False)
        seen += torch.tensor(list(cen[:5]) + [0] + list(cen[5]))
    assert has_edges((int(seen[0]), 0, int(seen[2]), 0, 0, tuple(seen[6:].tolist())))


def test_ring_epilogue_gelu_form_equals_the_general_body(ops, dev):
    """act 1 on a bias of ordinary values: out + out_mx (the general body) emits the fp32 row, GELU(bias); the rule on that row is the
    reference of both, and out_mx alone (the straight-line GELU form) must give the same bytes."""
    a, b = zero_a(ops, RM, RK, dev), some_b(ops, RN, RK, dev)
    g = torch.Generator().manual_seed(5)
    bias = torch.randn(RN, generator=g) * 2
    out, mx = torch.full((RM, RN), NAN, device=dev), mx_dest(ops, RM, RN, dev)
    ops.gemm_mxfp8(a, b, out, bias=bias.to(dev), act=1, out_mx=mx)
    assert bool((out == out[0]).all())
    emitted = out[:1].cpu()
    want = bias.double() * 0.5 * (1 + torch.erf(bias.double() / math.sqrt(2)))
    assert float((emitted[0].double() - want).abs().max()) < 1e-5          # |GELU| < 10: a dozen fp32 ulps; the row is GELU(bias) at all
    only = mx_dest(ops, RM, RN, dev)
    ops.gemm_mxfp8(a, b, None, bias=bias.to(dev), act=1, out_mx=only)
    for m in (mx, only):
        assert rows_all_equal(m) and mx_tail_ok(m)
        check("gemm_mxfp8 ring", (m.q[:RN].view(1, RN).cpu(), m.s[:RN // 32].view(1, RN // 32).cpu()), emitted)


@pytest.mark.parametrize("M", [m for m, _, _ in MC.RING_SHAPES])
def test_ring_epilogue_quantises_the_residual_rows(ops, dev, M):
    """resid = three rows of E tiled down the matrix, out + out_mx: the general body; M = 8100: a ragged last tile row, and there out
    and resid are strided."""
    N, K = RN, RK
    assert MC.takes_ring(M, N, K)
    x, idx, blocks, ref, cen = edge(3, N // 32)
    assert has_edges(cen)
    reps = -(-M // 3)
    ld = MC.leading_dims(K, N) if M % 256 else dict(ld_out=N, ld_resid=N)
    rbuf = torch.full((M, ld["ld_resid"]), NAN, device=dev)
    rbuf[:, :N] = x.to(dev).repeat(reps, 1)[:M]
    obuf = torch.full((M + MC.XROWS, ld["ld_out"]), MC.PAT32, dtype=torch.int32, device=dev).view(torch.float32)
    mx = mx_dest(ops, M, N, dev)
    ops.gemm_mxfp8(zero_a(ops, M, K, dev), some_b(ops, N, K, dev), obuf[:M, :N], resid=rbuf[:, :N], act=0, out_mx=mx)
    assert eq_nan(obuf[:M, :N], rbuf[:, :N]), "the fp32 output is not the residual"
    v = obuf.view(torch.int32).clone()
    v[:M, :N] = MC.PAT32
    assert bool((v == MC.PAT32).all()) and mx_tail_ok(mx)
    emitted = obuf[:3, :N].cpu().contiguous()
    assert MC.census_counts(MC.census(emitted)) == cen
    check("gemm_mxfp8 ring", (mx.q[:3 * N].view(3, N).cpu(), mx.s[:3 * N // 32].view(3, N // 32).cpu()), emitted, idx, blocks)
    q, s = mx.q[:M * N].view(M, N), mx.s[:M * N // 32].view(M, N // 32)
    assert bool((q == q[:3].repeat(reps, 1)[:M]).all()) and bool((s == s[:3].repeat(reps, 1)[:M]).all()), "rows differ down the matrix"


# ---- 6 / 7. the attention kernels' MX-FP8 context -----------------------------------------------------------------------------------
def attention_case(ops, dev, producer, fn, batch, heads, L, start):
    """Exactly one unmasked key per sequence, its V row = 8 edge blocks of bf16 numbers (every other V row small and finite): every
    context row of the sequence is that row.  Returns the emitted rows [batch, E] (one per sequence)."""
    E = heads * 64
    x, idx, blocks, _, _ = edge(batch, E // 32, start, bf16=True)
    g = torch.Generator().manual_seed(batch + L)
    qkv = torch.randn(batch, L, 3 * E, generator=g) * 0.5
    seg = torch.zeros(batch, L, dtype=torch.long)
    key = (37 * torch.arange(batch) + 3) % L                 # L = 304: in the first and in the second key block
    for b in range(batch):
        seg[b, key[b]] = 1
        qkv[b, key[b], 2 * E:] = x[b]
    qkv = qkv.view(batch * L, 3 * E).to(torch.bfloat16)
    assert eq_nan(qkv.view(batch, L, 3 * E)[torch.arange(batch), key, 2 * E:].float(), x)
    out = torch.full((batch * L, E), 12345.0, device=dev)
    mx = mx_dest(ops, batch * L, E, dev)
    fn(qkv.to(dev), seg.view(-1).to(dev), batch=batch, heads=heads, L=L, head_dim=64, scale=0.125, out=out, out_mx=mx)
    emitted = out.cpu()
    rows = emitted.view(batch, L, E)
    assert eq_nan(rows, rows[:, :1].expand(batch, L, E)), "context rows of one sequence differ"
    exact = eq_nan(rows[:, 0], x)
    full_idx = idx.repeat_interleave(L, 0)
    check(producer, mx, emitted, full_idx, blocks)
    assert mx_tail_ok(mx)
    return rows[:, 0].contiguous(), exact


def attention_census(rows, exact, want_blocks):
    c = MC.census(torch.cat(rows))
    print(f"  fp32 context bit-equal to the planted rows: {exact}; census {MC.census_counts(c)[:5]}")
    assert c.ties >= 1 and c.above448 >= 1 and bool((c.pos >= 1).all()), MC.census_counts(c)
    if all(exact):
        assert MC.census_counts(c) == MC.census_counts(MC.census(MC.lay(MC.BLOCKS_BF16, want_blocks // 8, 8)[0]))


def test_one_pair_attention_context_on_the_edge_blocks(ops, dev):
    batch, heads, L = 2, 4, 17
    assert not ops.self_attn_bf16_plan(batch, heads, L)
    n = -(-len(MC.BLOCKS_BF16) // 16)
    res = [attention_case(ops, dev, "self_attn_fwd_bf16 one pair", ops.self_attn_fwd_bf16, batch, heads, L, 16 * i) for i in range(n)]
    attention_census([r for r, _ in res], [e for _, e in res], 16 * n)


def test_persistent_attention_context_on_the_edge_blocks(ops, dev):
    batch, heads, L = 80, 4, 40
    assert ops.self_attn_bf16_plan(batch, heads, L)
    r, e = attention_case(ops, dev, "self_attn_fwd_bf16 persistent", ops.self_attn_fwd_bf16, batch, heads, L, 0)
    attention_census([r], [e], 8 * batch)


def test_blocked_attention_context_on_the_edge_blocks(ops, dev):
    batch, heads, L = -(-len(MC.BLOCKS_BF16) // 8), 4, 304
    c0 = ops.self_attn_fwd_bf16_blocked_launch_count()
    r, e = attention_case(ops, dev, "self_attn_fwd_bf16_blocked", ops.self_attn_fwd_bf16_blocked, batch, heads, L, 0)
    assert ops.self_attn_fwd_bf16_blocked_launch_count() == c0 + 1
    attention_census([r], [e], 8 * batch)


# ---- cross-producer -----------------------------------------------------------------------------------------------------------------
def test_producers_agree_where_the_rule_does_not_decide():
    """The byte of a NaN element and the sign of a zero byte (and, decided by the rule, the byte of +-Inf): one outcome per input in every
    producer, the same in all of them (asserted when the whole file ran; the outcomes are DESIGN.md's MX-FP8 table)."""
    for p in PRODUCERS:
        if p in OUTCOMES:
            print(f"  {p}: {CASES[p]} launches compared; " + ", ".join(f"{k} -> {sorted(hex(b) for b in v)}" for k, v in OUTCOMES[p].items()))
    if any(p not in OUTCOMES for p in PRODUCERS):
        return
    for key in KEYS:
        seen = {p: OUTCOMES[p][key] for p in PRODUCERS if OUTCOMES[p][key]}
        # an addition in front of the quantiser (0 + bias, + residual; the attention's accumulation) turns -0 into +0: three
        # producers take their input as it is
        assert len(seen) >= (3 if key == "-0" else len(PRODUCERS)), (key, list(seen))
        assert all(len(v) == 1 for v in seen.values()), (key, seen)
        assert len({next(iter(v)) for v in seen.values()}) == 1, (key, seen)
    assert all(OUTCOMES[p]["+inf"] == {0x7E} and OUTCOMES[p]["-inf"] == {0xFE} for p in PRODUCERS)


# ---- small-kernel product edges -----------------------------------------------------------------------------------------------------
def quant_exact(ops, t, dev):
    m = ops.quant_mxfp8(t.float().to(dev))
    assert torch.equal(m.to_float().cpu().double(), t), "the operand does not dequantise to the integers"
    return m


@pytest.mark.parametrize("M,N,K", MC.PRODUCT_SHAPES)
def test_small_product_is_exact_on_small_integers(ops, dev, M, N, K):
    assert not MC.takes_ring(M, N, K)
    a, b = MC.int_operands(M, N, K)
    am, bm = quant_exact(ops, a, dev), quant_exact(ops, b, dev)
    out = torch.full((M, N), NAN, device=dev)
    ops.gemm_mxfp8(am, bm, out)
    assert torch.equal(out.cpu().double(), a @ b.t())


@pytest.mark.parametrize("M,N,K", [(129, 384, 256), (1, 128, 128)])
def test_small_product_strides_and_canaries(ops, dev, M, N, K):
    """ld_out = N + 12, ld_resid = N + 20, bias, all three destinations at once: the exact result everywhere inside, the canary everywhere
    outside (pad columns, rows >= M, the tail of each allocation)."""
    a, b = MC.int_operands(M, N, K, seed=1)
    g = torch.Generator().manual_seed(M + N)
    bias = torch.randint(-9, 10, (N,), generator=g).double()
    resid = torch.randint(-9, 10, (M, N), generator=g).double() + (torch.arange(M) % 5).view(-1, 1)
    want = (a @ b.t() + bias + resid).float()
    ld = MC.leading_dims(K, N)
    rbuf = torch.full((M + 1, ld["ld_resid"]), NAN)
    rbuf[:M, :N] = resid.float()
    obuf = torch.full((M + MC.XROWS, ld["ld_out"]), MC.PAT32, dtype=torch.int32, device=dev).view(torch.float32)
    mx = mx_dest(ops, M, N, dev)
    pl, n = planes_dest(ops, M, N, dev)
    ops.gemm_mxfp8(quant_exact(ops, a, dev), quant_exact(ops, b, dev), obuf[:M, :N], bias=bias.float().to(dev), resid=rbuf.to(dev)[:M, :N],
                   out_mx=mx, out_planes=pl)
    assert torch.equal(obuf[:M, :N].cpu(), want)
    v = obuf.view(torch.int32).clone()
    v[:M, :N] = MC.PAT32
    assert bool((v == MC.PAT32).all()), "out written outside [0:M, 0:N]"
    check("gemm_mxfp8 128 (integers)", mx, want)
    assert mx_tail_ok(mx)
    check_planes(pl, n, want)


def test_small_product_with_extreme_operand_scales(ops, dev):
    """Hand-built operands: A blocks at scale byte 0 (2^-127) against B blocks at 254 (2^127) in the even K blocks, the reverse in the
    odd ones; elements +-1, +-2, +-3 or 0 (bytes 0x38, 0x40, 0x44): every product is a small integer times 2^0, the sum exact."""
    M, N, K = 64, 128, 256
    byte_of = torch.tensor([0x00, 0x38, 0x40, 0x44], dtype=torch.uint8)
    g = torch.Generator().manual_seed(11)
    a_blk = torch.where(torch.arange(K // 32) % 2 == 0, 0, 254).to(torch.uint8)

    def operand(rows, scale_blk):
        v = torch.randint(-3, 4, (rows, K), generator=g)
        q = byte_of[v.abs()] | ((v < 0).to(torch.uint8) << 7)
        return v.double(), ops.Mx8(q.flatten().to(dev), scale_blk.repeat(rows).to(dev), rows, K)

    (av, am), (bv, bm) = operand(M, a_blk), operand(N, 254 - a_blk)
    assert set(am.s.unique().tolist()) == {0, 254} and bool((am.s[:K // 32].long() + bm.s[:K // 32].long() == 254).all())
    out = torch.full((M, N), NAN, device=dev)
    ops.gemm_mxfp8(am, bm, out)
    assert torch.equal(out.cpu().double(), av @ bv.t())


@pytest.mark.parametrize("splits", [1, 2, 5])
@pytest.mark.parametrize("accumulate", [False, True])
def test_wgrad_is_exact_on_small_integers(ops, dev, splits, accumulate):
    M, N, K = MC.WGRAD_SHAPE
    a, b = MC.int_operands(M, N, K, seed=2)
    g = torch.Generator().manual_seed(splits)
    target = torch.randint(-9, 10, (M, N), generator=g).double() - (torch.arange(N) % 3)
    ld = N + 12
    obuf = torch.full((M + MC.XROWS, ld), MC.PAT32, dtype=torch.int32, device=dev).view(torch.float32)
    obuf[:M, :N] = target.float().to(dev)
    ws = torch.full((splits * M * N + MC.XROWS * N,), MC.PAT32, dtype=torch.int32, device=dev).view(torch.float32)
    ops.gemm_mxfp8_wgrad(quant_exact(ops, a, dev), quant_exact(ops, b, dev), obuf[:M, :N], splits=splits, accumulate=accumulate, workspace=ws)
    want = a @ b.t() + (target if accumulate else 0)
    assert torch.equal(obuf[:M, :N].cpu().double(), want)
    v = obuf.view(torch.int32).clone()
    v[:M, :N] = MC.PAT32
    assert bool((v == MC.PAT32).all()), "out written outside [0:M, 0:N]"
    assert bool((ws.view(torch.int32)[splits * M * N:] == MC.PAT32).all()), "workspace written past its slabs"


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
ERR_ARG, ERR_SHAPE = -1, -2


def test_refusals_leave_every_destination_untouched(ops, dev):
    from lr2ppo_amd import _native
    lib = _native.lib()
    M, N, K = 128, 128, 256               # two K steps: two slices exist, so "splits = 2 without a workspace" is a refusal
    x = torch.ones(M, K + 8, device=dev)
    f32 = torch.full((M + 1, N + 16), MC.PAT32, dtype=torch.int32, device=dev)
    q = torch.full((2 * M * N,), MC.SENT8, dtype=torch.uint8, device=dev)
    s = torch.full((2 * M * N // 32,), MC.SENT8, dtype=torch.uint8, device=dev)
    pl = torch.full((2 * M * N,), MC.PAT16, dtype=torch.int16, device=dev)
    am, bm = ops.quant_mxfp8(torch.ones(M, K, device=dev)), ops.quant_mxfp8(torch.ones(N, K, device=dev))
    P = lambda t: t.data_ptr()

    def quant(K_, ldx):
        return lib.lr2_quant_mxfp8(P(x), ldx, P(q), P(s), M, K_, None)

    def gemm(N_=N, K_=K, act=0, out=True, oq=None, os_=None, ld_out=N + 16, resid=None, ld_resid=0):
        return lib.lr2_gemm_mxfp8(P(am.q), P(am.s), P(bm.q), P(bm.s), P(f32) if out else None, ld_out, None, resid, ld_resid, act, oq, os_,
                                  P(pl), M * N, N_, M, N_, K_, None)

    def wgrad(M_=M, splits=1, ws=None):
        return lib.lr2_gemm_mxfp8_wgrad(P(am.q), P(am.s), P(bm.q), P(bm.s), P(f32), N + 16, 0, ws, splits, M_, N, K, None)

    cases = [("quant K % 32", lambda: quant(K - 16, K + 8), ERR_SHAPE), ("quant ldx < K", lambda: quant(K, K - 4), ERR_SHAPE),
             ("quant ldx % 4", lambda: quant(K, K + 2), ERR_SHAPE),
             ("gemm N % 128", lambda: gemm(N_=N - 64), ERR_SHAPE), ("gemm K % 128", lambda: gemm(K_=K - 64), ERR_SHAPE),
             ("gemm act 2", lambda: gemm(act=2), ERR_ARG), ("gemm out_q without out_scales", lambda: gemm(oq=P(q)), ERR_ARG),
             ("gemm out_scales without out_q", lambda: gemm(os_=P(s)), ERR_ARG),
             ("gemm ld_out < N", lambda: gemm(ld_out=N - 4), ERR_SHAPE),
             ("gemm ld_resid % 4", lambda: gemm(resid=P(x), ld_resid=N + 2), ERR_SHAPE),
             ("wgrad M % 128", lambda: wgrad(M_=M - 64), ERR_SHAPE), ("wgrad splits > 1 without a workspace", lambda: wgrad(splits=2), ERR_ARG)]
    assert quant(K, K + 8) == 0 and gemm(oq=P(q), os_=P(s)) == 0 and wgrad() == 0         # the same calls, valid: accepted
    torch.cuda.synchronize()
    for t, pat in ((f32, MC.PAT32), (q, MC.SENT8), (s, MC.SENT8), (pl, MC.PAT16)):
        t.fill_(pat)
    for name, call, want in cases:
        assert call() == want, name
    torch.cuda.synchronize()
    assert bool((f32 == MC.PAT32).all()) and bool((q == MC.SENT8).all()) and bool((s == MC.SENT8).all()) and bool((pl == MC.PAT16).all())
    assert bool((x == 1).all())
