"""Edge suite of the kernels that feed and drain the encoders, on a real MI355X: the row gathers and the concat copy, the text and ViT
embedding front-ends (forward and backward), the XiT cross-attention pair and the NDCG kernel, each against a plain CPU reference of
the same operation (tests/frontend_cases.py has the tables, the input builders and the references; test_frontend_edges_cpu.py proves
the exact input classes exact and holds the argument contracts).

Conventions of every case.  A destination is allocated with canary rows behind it (fp32: the NaN pattern 0x7FC0BEEF; bf16 planes:
0x7FC1, the gap between the hi and the lo plane included, lo_off = plane size + gap) and the region to be written is pre-filled with
the same pattern: after the call nothing outside the region has changed and nothing inside is still the pattern.  Inputs carry NaN
wherever the kernel must not read into a kept result.  Data movement (gathers, copies, patchify, planes) is compared with torch.equal;
a planes output must equal ops.split_planes of the fp32 output of the same call, bit for bit.

Large-score class of the XiT attention (test_xattn_large_scores): unit-variance inputs, no pre-scale, so |S| reaches 42 at head_dim 96.
The bound is not invented: the kernels' formulas evaluated in fp32 torch on the CPU are off the fp64 reference by at most
    O 8.0e-07, dQ 4.6e-06, dK 4.5e-06, dV 8.7e-07      (max |fp32 - fp64|, measured; the largest of the table's three shapes, 256 x 16:
                                                        3.2e-06, 1.9e-05, 1.8e-05 and 3.5e-06 allowed)
and the kernel is allowed 4 times the figure of its own shape (it multiplies by log2 e and uses the hardware exp2: two more roundings
of an argument of this size); the test computes both numbers again on every run and prints them."""
import pytest
import torch

import frontend_cases as FC

pytestmark = pytest.mark.gpu

PAT32 = 0x7FC0BEEF        # canary / pre-fill of fp32 destinations (a NaN)
PAT16 = 0x7FC1            # canary / pre-fill of bf16 planes and of the gap between them (a NaN)
GAP = 8                   # bf16 elements between the hi and the lo plane
XROWS = 3                 # canary rows behind every destination


@pytest.fixture(scope="module")
def ops(dev):
    from lr2ppo_amd import ops as _ops
    return _ops


def P(table):
    return dict(argnames="case", argvalues=table, ids=FC.ids_of(table))


# ---- destinations -------------------------------------------------------------------------------------------------------------------
def dest32(n, dev, extra):
    """fp32 destination of n elements with `extra` canary elements behind it, all of it the NaN pattern."""
    return torch.full((n + extra,), PAT32, dtype=torch.int32, device=dev).view(torch.float32)


def check32(buf, ref, what):
    """buf[:n] equals ref (finite, so nothing in it is still the pattern) and the canaries behind it are intact."""
    n = ref.numel()
    got = buf[:n].cpu()
    assert bool(torch.isfinite(ref).all())
    assert not bool(torch.isnan(got).any()), f"{what}: NaN inside the written region (an element not written, or a NaN input read)"
    assert torch.equal(got, ref.reshape(-1).float()), f"{what}: max |diff| {float((got.double() - ref.reshape(-1).double()).abs().max()):.3e}"
    assert bool((buf[n:].view(torch.int32) == PAT32).all()), f"{what}: written past the destination"


class PlanesDest:
    """hi | gap | lo planes of [rows + xrows, cols], everything the pattern; the result goes to the first rows * cols of each."""

    def __init__(self, ops, rows, cols, dev, xrows=XROWS, gap=GAP):
        self.n, self.span, self.gap = rows * cols, (rows + xrows) * cols, gap
        self.buf = torch.full((2 * self.span + gap,), PAT16, dtype=torch.int16, device=dev)
        self.planes = ops.Planes(self.buf, rows, cols, lo_off=self.span + gap)

    def check(self, ops, dense, what):
        """Both planes bit-equal to split_planes of the dense fp32 result, canaries and gap intact."""
        want = ops.split_planes(dense.contiguous().view(-1), ops.Planes.empty(1, self.n, dense.device))
        exp = torch.full_like(self.buf, PAT16)
        exp[:self.n] = want.buf[:self.n]
        lo = self.planes.lo_off
        exp[lo:lo + self.n] = want.buf[self.n:2 * self.n]
        assert not bool((want.buf == PAT16).any())
        bad = (self.buf != exp).nonzero().view(-1)
        assert bad.numel() == 0, f"{what}: planes differ from split_planes(fp32 result) / canaries at elements {bad[:8].tolist()} of {bad.numel()}"


# ---- gather_rows / gather_rows_bwd --------------------------------------------------------------------------------------------------
_GATHER = {}


def gather_setup(case):
    """Computed once per case and shared by the three gather tests (never modified)."""
    if case["id"] not in _GATHER:
        B, t_in, t_out, re = case["B"], case["t_in"], case["t_out"], case["row_elems"]
        gen = torch.Generator().manual_seed(re + B)
        index = FC.gather_index(case)
        clamped = FC.gather_clamped(case, index)
        x = FC.small_ints(gen, B, t_in, re, lo=-8, hi=8)
        y = FC.small_ints(gen, B, t_out, re, lo=-8, hi=8)
        _GATHER[case["id"]] = (index, clamped, x, y)
    return _GATHER[case["id"]]


def run_gather(ops, dev, case, x, index):
    B, t_in, t_out, re = case["B"], case["t_in"], case["t_out"], case["row_elems"]
    src, off, bstride, tstride = FC.gather_source(case, x)
    src = src.to(dev)
    dst = dest32(B * t_out * re, dev, XROWS * 4)
    ops.gather_rows(src[off:], None if index is None else index.to(dev), dst, B=B, t_in=t_in, t_out=t_out, row_elems=re,
                    src_bstride=bstride, src_tstride=tstride)
    return dst


def run_gather_bwd(ops, dev, case, y, index):
    B, t_in, t_out, re = case["B"], case["t_in"], case["t_out"], case["row_elems"]
    dsrc = dest32(B * t_in * re, dev, XROWS * 4)
    ops.gather_rows_bwd(y.to(dev), None if index is None else index.to(dev), dsrc, B=B, t_in=t_in, t_out=t_out, row_elems=re)
    return dsrc


@pytest.mark.parametrize(**P(FC.GATHER))
def test_gather_rows(ops, dev, case):
    """dst[b, j] = src[b, clamp(index[b, j])] bit for bit in all three stride forms, through the wrapped grid-stride loop too; source rows
    that no index selects are NaN (as are the skipped columns of the offset view), so a wrong row shows at once."""
    index, clamped, x, _ = gather_setup(case)
    xs = x.clone()
    for b in range(case["B"]):
        unused = torch.ones(case["t_in"], dtype=torch.bool)
        unused[clamped[b]] = False
        xs[b, unused] = FC.NAN
    dst = run_gather(ops, dev, case, xs, index)
    check32(dst, FC.gather_fwd_ref(x, clamped), "gather_rows")


@pytest.mark.parametrize(**P(FC.GATHER))
def test_gather_rows_bwd(ops, dev, case):
    """dsrc[b, t] = sum of ddst[b, j] over the j whose clamped index is t, on integer-valued gradients (exact in any order): every row
    is written, a row never selected as zeros; an index below 0 or >= t_in counts for the row the forward read."""
    index, clamped, _, y = gather_setup(case)
    dsrc = run_gather_bwd(ops, dev, case, y, index)
    check32(dsrc, FC.gather_bwd_ref(y, clamped, case["t_in"]), "gather_rows_bwd")


@pytest.mark.parametrize(**P(FC.GATHER))
def test_gather_pair_is_adjoint(ops, dev, case):
    """<gather(x), y> == <x, gather_bwd(y)> for every index tensor the forward accepts; integer-valued x and y make both sides exact."""
    index, _, x, y = gather_setup(case)
    n_out, n_in = y.numel(), x.numel()
    g = run_gather(ops, dev, case, x, index)[:n_out].cpu().double()
    gb = run_gather_bwd(ops, dev, case, y, index)[:n_in].cpu().double()
    lhs, rhs = float((g * y.view(-1).double()).sum()), float((x.view(-1).double() * gb).sum())
    assert lhs == rhs, (lhs, rhs)


# ---- copy_rows ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(**P(FC.COPY))
def test_copy_rows(ops, dev, case):
    """Every element of the strided destination, gaps and tail included, bit for bit: the rows where the formula puts them, the pattern
    everywhere else (fp32), or split_planes of the rows in both planes (planes)."""
    rows, D = case["rows"], case["D"]
    src = torch.randn(rows, D, generator=torch.Generator().manual_seed(rows))
    idx, span = FC.copy_dst_index(case)
    idx = idx.to(dev)
    kw = dict(rows=rows, D=D, group=case["group"], dst_gstride=case["gstride"], dst_off=case["off"])
    if not case["planes"]:
        dst = dest32(span, dev, XROWS * D)
        ops.copy_rows(src.to(dev), dst, **kw)
        exp = torch.full_like(dst.view(torch.int32), PAT32)
        exp[idx.view(-1)] = src.view(-1).to(dev).view(torch.int32)
        assert torch.equal(dst.view(torch.int32), exp)
        return
    total = span + XROWS * D
    buf = torch.full((2 * total + GAP,), PAT16, dtype=torch.int16, device=dev)
    lo_off = total + GAP
    ops.copy_rows(src.to(dev), ops.Planes(buf, 1, total, lo_off=lo_off), **kw)
    want = ops.split_planes(src.to(dev).view(-1), ops.Planes.empty(1, rows * D, dev))
    exp = torch.full_like(buf, PAT16)
    exp[idx.view(-1)] = want.buf[:rows * D]
    exp[idx.view(-1) + lo_off] = want.buf[rows * D:]
    assert torch.equal(buf, exp)


# ---- text_embed ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(**P(FC.TEXT_EMBED))
def test_text_embed(ops, dev, case):
    """Bit-equal to fp32 (word[ids] + pos[r % L]) + seg_table[seg]; an out-of-range id reads row 0 and sets its bit of the error word
    (token: bit 0, segment: bit 1) and nothing else; with err = None the output is the same."""
    rows, L, D = case["rows"], case["L"], case["D"]
    ids, seg, word, pos, seg_table, ids_ok, seg_ok = FC.text_embed_inputs(case)
    ref = FC.text_embed_ref(ids_ok, seg_ok, word, pos, seg_table, L)
    args = [t.to(dev) for t in (ids, seg, word, pos, seg_table)]
    errbuf = torch.tensor([0x5A5A5A5A, 0, 0x5A5A5A5A], dtype=torch.int32, device=dev)
    out = dest32(rows * D, dev, XROWS * D)
    ops.text_embed(*args, out, rows=rows, L=L, D=D, err=errbuf[1:2])
    check32(out, ref, "text_embed")
    assert errbuf.tolist() == [0x5A5A5A5A, FC.text_embed_err(case), 0x5A5A5A5A]
    out2 = dest32(rows * D, dev, XROWS * D)
    ops.text_embed(*args, out2, rows=rows, L=L, D=D, err=None)
    assert torch.equal(out2.view(torch.int32), out.view(torch.int32))


# ---- text_embed_bwd -----------------------------------------------------------------------------------------------------------------
def run_embed_bwd(ops, dev, dx, ids, seg, vocab, n_seg):
    D = dx.shape[1]
    dword = dest32(vocab * D, dev, XROWS * D)
    dseg = dest32(n_seg * D, dev, XROWS * D)
    ops.text_embed_bwd(dx.to(dev), ids.to(dev), seg.to(dev), dword[:vocab * D].view(vocab, D), dseg[:n_seg * D].view(n_seg, D),
                       rows=dx.shape[0], D=D)
    return dword, dseg


def check_word_table(dword, ref, present, what):
    """Rows of present tokens equal the reference; every other row (absent ids, the canary rows) keeps its pre-fill bit for bit."""
    vocab, D = ref.shape
    got = dword.cpu()
    exp = torch.full_like(got.view(torch.int32), PAT32)
    exp[:vocab * D].view(vocab, D)[present] = ref[present].float().view(torch.int32)
    bad = (got.view(torch.int32) != exp).nonzero().view(-1)
    assert bad.numel() == 0, f"{what}: {bad.numel()} elements differ, first at table row {int(bad[0]) // D} (rows present: {present.nonzero().view(-1).tolist()})"


@pytest.mark.parametrize(**P(FC.EMBED_BWD_WORD))
def test_text_embed_bwd_word_pieces(ops, dev, case):
    """The piece logic at the sorted positions where it can be off by one, on integer-valued dx (any summation order is exact) against an
    fp64 index_add_: every present row exact, every absent row and every row of an out-of-range id untouched."""
    ids, vocab = FC.embed_bwd_word_ids(case)
    rows, D = ids.numel(), case["D"]
    gen = torch.Generator().manual_seed(rows)
    dx = FC.small_ints(gen, rows, D)
    seg = torch.arange(rows) % 2
    dword, dseg = run_embed_bwd(ops, dev, dx, ids, seg, vocab, 2)
    ref, present = FC.index_add_ref(dx, ids, vocab)
    check_word_table(dword, ref, present, "dword")
    check32(dseg, FC.index_add_ref(dx, seg, 2)[0], "dseg")


@pytest.mark.parametrize(**P(FC.EMBED_BWD_SEG))
def test_text_embed_bwd_segment_table(ops, dev, case):
    """Segment sums at the 64-row workgroup edges for every n_seg; ids >= n_seg and negative ones are dropped; all n_seg rows are written."""
    rows, n_seg, D = case["rows"], case["n_seg"], 8
    dx = FC.small_ints(torch.Generator().manual_seed(rows + n_seg), rows, D)
    seg = FC.embed_bwd_seg_ids(rows, n_seg)
    ids = torch.arange(rows) % 5
    dword, dseg = run_embed_bwd(ops, dev, dx, ids, seg, 6, n_seg)
    check32(dseg, FC.index_add_ref(dx, seg, n_seg)[0], "dseg")
    check_word_table(dword, *FC.index_add_ref(dx, ids, 6), "dword")


@pytest.mark.parametrize(**P(FC.EMBED_BWD_RANDOM))
def test_text_embed_bwd_random_values(ops, dev, case):
    """N(0, 1) gradients, one run of 700 among 1500 shuffled rows: three calls give identical bits, and every element is within the
    bound of a sequential fp32 sum, n 2^-24 sum |dx_i| over the n rows summed into it."""
    rows, run, D = case["rows"], case["run"], case["D"]
    gen = torch.Generator().manual_seed(rows)
    vocab = 40
    ids = torch.cat([torch.full((run,), 9, dtype=torch.int64), torch.randint(0, vocab, (rows - run,), generator=gen)])
    ids = ids[torch.randperm(rows, generator=gen)]
    seg = torch.randint(0, 3, (rows,), generator=gen)
    dx = torch.randn(rows, D, generator=gen)
    outs = [run_embed_bwd(ops, dev, dx, ids, seg, vocab, 3) for _ in range(3)]
    for dword, dseg in outs[1:]:
        assert torch.equal(dword.view(torch.int32), outs[0][0].view(torch.int32)) and torch.equal(dseg.view(torch.int32), outs[0][1].view(torch.int32))
    for name, got, idv, n in (("dword", outs[0][0], ids, vocab), ("dseg", outs[0][1], seg, 3)):
        ref, present = FC.index_add_ref(dx, idv, n)
        assert bool(present.all())
        err = (got[:n * D].cpu().double().view(n, D) - ref).abs()
        bound = FC.seq_sum_bound(dx, idv, n)
        print(f"  [{name}] max |err| {float(err.max()):.3e}, smallest bound / err ratio {float((bound / err.clamp_min(1e-300)).min()):.1f}")
        assert bool((err <= bound).all()), name
        assert bool((got[n * D:].view(torch.int32) == PAT32).all())


# ---- patchify -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(**P(FC.PATCHIFY_PLANES))
def test_patchify_planes(ops, dev, case):
    """Both planes bit-equal to split_planes of the torch view / permute / reshape of the (normalised) image, pad columns zeros, canaries
    intact -- in the strip kernel (1, 2 and 3 trips of its loop), the generic kernel at VEC 4 and at VEC 2.
    case["kernel"] is the kernel the case reaches, derived from lr2_patchify_planes' dispatch (FC.patchify_kernel restates it)."""
    assert FC.patchify_kernel(case) == case["kernel"]
    B, C, H, W, ps = case["B"], case["C"], case["H"], case["W"], case["ps"]
    ld = FC.patchify_ld(case)
    img, x = FC.patchify_image(case)
    rows = B * (H // ps) * (W // ps)
    dst = PlanesDest(ops, rows, ld, dev, gap=GAP + 2 if case["lo2"] else GAP)
    assert dst.planes.lo_off % 4 == (2 if case["lo2"] else 0)
    kw = dict(mean=FC.CLIP_MEAN, std=FC.CLIP_STD) if case["src"] == "u8n" else {}
    ops.patchify_planes(img.to(dev), dst.planes, B=B, Cc=C, H=H, W=W, ps=ps, **kw)
    dst.check(ops, FC.patch_rows(x, ps, ld).to(dev), "patchify_planes")


@pytest.mark.parametrize(**P(FC.PATCHIFY))
def test_patchify(ops, dev, case):
    B, C, H, W, ps = case["B"], case["C"], case["H"], case["W"], case["ps"]
    img = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(H))
    out = dest32(B * C * H * W, dev, XROWS * C * ps * ps)
    ops.patchify(img.to(dev), out, B=B, Cc=C, H=H, W=W, ps=ps)
    check32(out, FC.patch_rows(img, ps), "patchify")


# ---- vit_assemble -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(**P(FC.VIT_ASSEMBLE))
def test_vit_assemble(ops, dev, case):
    """Bit-equal to fp32 cat([cls, proj]) + pos; the position table has two more rows than P + 1, NaN."""
    B, Pn, D = case["B"], case["P"], case["D"]
    gen = torch.Generator().manual_seed(B * Pn + D)
    proj, cls, pos = torch.randn(B * Pn, D, generator=gen), torch.randn(D, generator=gen), torch.randn(Pn + 3, D, generator=gen)
    pos[Pn + 1:] = FC.NAN
    ref = torch.cat([cls.view(1, 1, D).expand(B, 1, D), proj.view(B, Pn, D)], dim=1) + pos[:Pn + 1]
    out = dest32(B * (Pn + 1) * D, dev, XROWS * D)
    ops.vit_assemble(proj.to(dev), cls.to(dev), pos.to(dev), out, B=B, P=Pn, D=D)
    check32(out, ref, "vit_assemble")


# ---- XiT cross-attention ------------------------------------------------------------------------------------------------------------
def run_xattn(ops, dev, case, q, k, v, do, planes=False):
    """-> (O, dQ, dK, dV) destinations: canaried fp32 buffers, or PlanesDest objects."""
    batch, heads, Lq, Lk, hd = (case[n] for n in ("batch", "heads", "Lq", "Lk", "hd"))
    E = heads * hd
    kw = dict(batch=batch, heads=heads, Lq=Lq, Lk=Lk, head_dim=hd, post_scale=FC.xattn_post_scale(case))
    qd, kd, vd, dod = (t.to(dev).view(-1, E) for t in (q, k, v, do))
    if planes:            # K-sized outputs get one canary row more, so that q_lo_off != kv_lo_off even when Lq == Lk
        o, dq = PlanesDest(ops, batch * Lq, E, dev), PlanesDest(ops, batch * Lq, E, dev)
        dk, dv = PlanesDest(ops, batch * Lk, E, dev, xrows=XROWS + 1), PlanesDest(ops, batch * Lk, E, dev, xrows=XROWS + 1)
        assert dq.planes.lo_off != dk.planes.lo_off
        ops.xattn_fwd(qd, kd, vd, o.planes, **kw)
        ops.xattn_bwd(qd, kd, vd, dod, dq.planes, dk.planes, dv.planes, **kw)
        return o, dq, dk, dv
    o, dq = dest32(batch * Lq * E, dev, XROWS * E), dest32(batch * Lq * E, dev, XROWS * E)
    dk, dv = dest32(batch * Lk * E, dev, XROWS * E), dest32(batch * Lk * E, dev, XROWS * E)
    ops.xattn_fwd(qd, kd, vd, o[:batch * Lq * E].view(-1, E), **kw)
    ops.xattn_bwd(qd, kd, vd, dod, dq[:batch * Lq * E].view(-1, E), dk[:batch * Lk * E].view(-1, E), dv[:batch * Lk * E].view(-1, E), **kw)
    return o, dq, dk, dv


def check_close(buf, ref, atol, rtol, what):
    n = ref.numel()
    got = buf[:n].cpu().double()
    err = (got - ref.reshape(-1)).abs()
    bad = ~(err <= atol + rtol * ref.reshape(-1).abs())
    print(f"  [{what}] max |err| {float(err.max()):.3e} (atol {atol:.2e}, rtol {rtol:.0e}, ref scale {float(ref.abs().max()):.3e})")
    assert not bool(bad.any()), f"{what}: max err {float(err.max()):.3e}, {int(bad.sum())} bad"
    assert bool((buf[n:].view(torch.int32) == PAT32).all()), f"{what}: written past the destination"


@pytest.mark.parametrize(**P(FC.XATTN_ONEHOT))
def test_xattn_one_hot_is_exact(ops, dev, case):
    """Each query's best key leads by >= 200, so the softmax is exactly one-hot: O = c V[winner], dQ = 0, dK = 0, dV[j] = c sum of dO
    over the queries that chose j, all with torch.equal.  The winner depends on the query, the head and the sequence, and V / dO differ
    per head and sequence: a wrong head or sequence offset cannot pass as rounding."""
    q, k, v, do = FC.xattn_inputs(case)
    got = run_xattn(ops, dev, case, q, k, v, do)
    for name, g, r in zip(("O", "dQ", "dK", "dV"), got, FC.xattn_onehot_expected(case, v, do, FC.xattn_post_scale(case))):
        check32(g, r, f"one-hot {name}")


@pytest.mark.parametrize(**P(FC.XATTN_UNIFORM))
def test_xattn_uniform_is_exact(ops, dev, case):
    """Q = 0 and Lk a power of two: p = 1 / Lk exactly, so O = c / Lk sum V, dV = c / Lk sum dO, dK = 0 (every dS is multiplied by Q = 0)
    and dQ = sum_j dS_j K_j are small integers times a power of two -- the fp64 formula, compared with torch.equal."""
    q, k, v, do = FC.xattn_inputs(case)
    got = run_xattn(ops, dev, case, q, k, v, do)
    ref = FC.xattn_formula(q, k, v, do, case["heads"], FC.xattn_post_scale(case), torch.float64)
    assert not bool(ref[2].any()) and (case["Lk"] == 1 or bool(ref[1].any()))
    for name, g, r in zip(("O", "dQ", "dK", "dV"), got, ref):
        check32(g, r, f"uniform {name}")


@pytest.mark.parametrize(**P(FC.XATTN_RANDOM))
def test_xattn_random(ops, dev, case):
    """Input scales and tolerances of test_kernels_gpu.py::test_xattn_fwd_bwd, against fp64 autograd, at the edge shapes."""
    q, k, v, do = FC.xattn_inputs(case)
    o, dq, dk, dv = run_xattn(ops, dev, case, q, k, v, do)
    ro, rq, rk, rv = FC.xattn_autograd(q, k, v, do, case["heads"], FC.xattn_post_scale(case))
    check_close(o, ro, 1e-6, 1e-5, "xattn fwd")
    check_close(dq, rq, 1e-6, 1e-4, "dq")
    check_close(dk, rk, 1e-5, 1e-4, "dk")
    check_close(dv, rv, 1e-5, 1e-4, "dv")


@pytest.mark.parametrize(**P(FC.XATTN_LARGE))
def test_xattn_large_scores(ops, dev, case):
    """Unit inputs without a pre-scale: the bound is 4 x the error of the same formulas in fp32 torch on the CPU (see the header)."""
    q, k, v, do = FC.xattn_inputs(case)
    post = FC.xattn_post_scale(case)
    ref = FC.xattn_formula(q, k, v, do, case["heads"], post, torch.float64)
    f32 = FC.xattn_formula(q, k, v, do, case["heads"], post, torch.float32)
    got = run_xattn(ops, dev, case, q, k, v, do)
    fails = []
    for name, g, r, f in zip(("O", "dQ", "dK", "dV"), got, ref, f32):
        n = r.numel()
        e32 = float((f.double() - r).abs().max())
        err = float((g[:n].cpu().double() - r.reshape(-1)).abs().max())
        print(f"  [large {name}] fp32 torch formula max |err| {e32:.3e}; kernel max |err| {err:.3e}; allowed {4 * e32:.3e}")
        assert bool((g[n:].view(torch.int32) == PAT32).all())
        if not err <= 4 * e32:
            fails.append((name, err, 4 * e32))
    assert not fails, fails


@pytest.mark.parametrize(**P(FC.XATTN_PLANES))
def test_xattn_planes_outputs(ops, dev, case):
    """Planes outputs of the forward and the backward equal split_planes of the fp32 outputs of the same calls, bit for bit, with
    canaries behind the Q-sized and the K-sized outputs and q_lo_off != kv_lo_off."""
    q, k, v, do = FC.xattn_inputs(case)
    dense = run_xattn(ops, dev, case, q, k, v, do)
    planes = run_xattn(ops, dev, case, q, k, v, do, planes=True)
    for name, d, p in zip(("O", "dQ", "dK", "dV"), dense, planes):
        assert bool((d[p.n:].view(torch.int32) == PAT32).all()) and not bool(torch.isnan(d[:p.n]).any())
        p.check(ops, d[:p.n], f"planes {name}")


# ---- NDCG ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(**P(FC.NDCG))
def test_ndcg(ops, dev, case):
    """Every item against the kernel's documented rule in sequential fp32 (FC.ndcg_ref) and, where the host meter applies, against
    AverageNDCGMeter, both at the existing tests' atol 1e-6: empty items are rows of ones, items of 65 elements and labels 63 / -1 rows
    of NaN with their neighbours intact, label 62 finite, ties resolved earlier index first."""
    from lr2ppo_amd.ndcg import AverageNDCGMeter
    items = FC.ndcg_items(case)
    offs = [0]
    for s, _, _ in items:
        offs.append(offs[-1] + s.numel())
    out = ops.ndcg(torch.cat([s for s, _, _ in items]).to(dev), torch.cat([g for _, g, _ in items]).to(dev),
                   torch.tensor(offs, dtype=torch.int64, device=dev), ks=FC.NDCG_KS).cpu()
    assert out.shape == (len(items), len(FC.NDCG_KS))
    meter = AverageNDCGMeter(FC.NDCG_KS)
    for i, (s, g, kind) in enumerate(items):
        want = FC.ndcg_ref(s, g, FC.NDCG_KS)
        if kind in ("t65", "label63", "label-1"):
            assert bool(torch.isnan(want).all()) and bool(torch.isnan(out[i]).all()), (i, kind, out[i])
            continue
        assert bool(torch.isfinite(out[i]).all()), (i, kind, out[i])
        assert float((out[i] - want).abs().max()) <= 1e-6, (i, kind, out[i], want)
        if kind == "t0":
            assert torch.equal(out[i], torch.ones(len(FC.NDCG_KS)))
        if FC.ndcg_meter_applies(kind, s.numel()):
            assert float((out[i] - meter.return_ndcg_at_k_from_scores(s, g)).abs().max()) <= 1e-6, (i, kind)
