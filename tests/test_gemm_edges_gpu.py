"""Edge suite of the GEMM family on a real MI355X: lr2_gemm, lr2_gemm_bf16 and lr2_gemm_bf16_train at the smallest shapes where each
kernel can go wrong, against a plain fp64 product of the same operands (tests/gemm_cases.py has the tables and the operand classes;
test_gemm_edges_cpu.py proves the classes exact).

Layout is the point.  Every case runs with distinct, non-tight leading dimensions on everything the wrapper lets the caller set, NaN
in every byte of an input the product must not read into a kept result (pad columns, rows past M / N inside the buffer, a gap between
the hi and the lo plane), and a fixed bit pattern in every byte of a destination it must not write ([M + 3, ld] allocations, checked
bit for bit outside [0:M, 0:N]).  Exact classes are compared with torch.equal; what passes through GELU / GELU' by the tolerance
rules already written down (test_kernels_gpu.py's header: 6e-5 sqrt(K) + 5e-5 |ref| at three passes; test_gemm_nt_forward's 1e-4 sqrt(K)
+ 1e-4 |ref| against bf16-rounded operands at one pass; half an ulp for mul_gelu_grad_exact).  Each case asserts through the launch
counters which kernel family it reached, the 256 x 256 NT cases also the tile height of the launcher's rule."""
import ctypes
import math

import pytest
import torch

import gemm_cases as GC
from oracle import lr2ppo_oracle as O

pytestmark = pytest.mark.gpu

NAN = float("nan")
PAT32 = 0x7FC0BEEF        # canary of fp32 destinations (a NaN)
PAT16 = 0x7FC1            # canary of bf16 destinations and of the gap between input planes (a NaN)
GAP = 8                   # bf16 elements between the hi and the lo plane
XROWS = 3                 # canary rows behind every destination, NaN rows behind A and B


def ws_dest(splits, M, N, dev):
    """Split-K workspace with canary rows behind the last slab."""
    return torch.full((splits * M * N + XROWS * N,), PAT32, dtype=torch.int32, device=dev).view(torch.float32)

REACH = {}                # family -> cases that reached it (test_every_family_was_reached)
N_CASES = len(GC.GENERAL) + len(GC.NT256) + 1 + len(GC.TN256) + len(GC.B1) + len(GC.B1T_NT) + len(GC.B1T_TN)


@pytest.fixture(scope="module")
def ops(dev):
    from lr2ppo_amd import ops as _ops
    return _ops


# ---- layout helpers -----------------------------------------------------------------------------------------------------------------
def padded(x, rows, ld, dev, dtype=torch.float32):
    """x [R, C] inside a NaN [rows, ld] buffer."""
    buf = torch.full((rows, ld), NAN, dtype=dtype)
    buf[:x.shape[0], :x.shape[1]] = x.to(dtype)
    return buf.to(dev)


def in_planes(ops, x_pad):
    """Planes of a padded fp32 matrix, the lo plane GAP NaN elements behind the hi plane."""
    R, ld = x_pad.shape
    buf = torch.full((2 * R * ld + GAP,), PAT16, dtype=torch.int16, device=x_pad.device)
    pl = ops.split_planes(x_pad, ops.Planes(buf, R, ld, lo_off=R * ld + GAP))
    assert bool((buf[R * ld:R * ld + GAP] == PAT16).all())
    return pl


def operand(ops, kind, x, rows, ld, dev):
    """kind f: padded fp32 matrix; p: planes of it; b: ONE bf16 plane."""
    if kind == "b":
        return padded(x, rows, ld, dev, torch.bfloat16)
    xp = padded(x, rows, ld, dev)
    return in_planes(ops, xp) if kind == "p" else xp


def dest32(M, N, ld, dev, init=None):
    buf = torch.full((M + XROWS, ld), PAT32, dtype=torch.int32, device=dev).view(torch.float32)
    if init is not None:
        buf[:M, :N] = init.float().to(dev)
    return buf


def canary32_ok(buf, M, N, col0=0):
    v = buf.view(torch.int32).clone()
    v[:M, col0:col0 + N] = PAT32
    return bool((v == PAT32).all())


class PlanesDest:
    """hi / lo planes [M + 3, ld] with a gap between them, everything prefilled with the canary; the result goes to columns
    [col0, col0 + N)."""

    def __init__(self, ops, M, N, ld, dev, col0=0):
        self.M, self.N, self.ld, self.col0, self.rows = M, N, ld, col0, M + XROWS
        n = self.rows * ld
        self.buf = torch.full((2 * n + GAP,), PAT16, dtype=torch.int16, device=dev)
        self.planes = ops.Planes(self.buf, M, ld, lo_off=n + GAP)

    def parts(self):
        n = self.rows * self.ld
        return self.buf[:n].view(self.rows, self.ld), self.buf[n:n + GAP], self.buf[n + GAP:].view(self.rows, self.ld)

    def check(self, ops, out_dense):
        """Canaries intact and the interior bit-equal to split_planes of the fp32 result (None: the canaries alone)."""
        hi, gap, lo = self.parts()
        M, N, c = self.M, self.N, self.col0
        if out_dense is not None:
            want = ops.split_planes(out_dense.contiguous(), ops.Planes.empty(M, N, out_dense.device))
            assert torch.equal(hi[:M, c:c + N], want.buf[:M * N].view(M, N)), "hi plane != split_planes(out)"
            assert torch.equal(lo[:M, c:c + N], want.buf[M * N:2 * M * N].view(M, N)), "lo plane != split_planes(out)"
        for name, p in (("hi", hi), ("lo", lo)):
            v = p.clone()
            v[:M, c:c + N] = PAT16
            assert bool((v == PAT16).all()), f"{name} plane written outside [0:M, {c}:{c}+N]"
        assert bool((gap == PAT16).all()), "gap between the planes written"


def plane_dest(M, N, dev):
    """ONE bf16 plane (tight [M, N]: the wrappers fix its stride) with canary rows behind it."""
    return torch.full(((M + XROWS) * N,), PAT16, dtype=torch.int16, device=dev)


def check_plane(one, out_dense, M, N):
    assert torch.equal(one[:M * N].view(torch.bfloat16).view(M, N), out_dense.bfloat16()), "single plane != out.bfloat16()"
    assert bool((one[M * N:] == PAT16).all()), "single plane written past M rows"


def close(got, ref, atol, rtol, what):
    got, ref = got.detach().double().cpu(), ref.double()
    err = (got - ref).abs()
    bad = ~(err <= atol + rtol * ref.abs())
    print(f"  [{what}] max |err| {float(err.max()):.3e} (atol {atol:.2e}, rtol {rtol:.0e}, ref scale {float(ref.abs().max()):.3e})")
    assert not bad.any(), f"{what}: max err {float(err.max()):.3e}, {int(bad.sum())} bad"


def tol(passes, K):
    """The project's written rules: test_kernels_gpu.py's header at three passes, test_gemm_nt_forward's single-pass rule."""
    return (6e-5 * math.sqrt(K), 5e-5) if passes == 3 else (1e-4 * math.sqrt(K), 1e-4)


def half_ulp_ok(got, ref64, what):
    """|got - ref| <= half the fp32 spacing at the correctly rounded ref (mul_gelu_grad_exact's claim; 2^-20 of slack for the fp64
    evaluation of GELU' on either side, 2^-29 relative to an ulp's 2^-23)."""
    got = got.detach().double().cpu()
    r32 = ref64.float()
    _, e = torch.frexp(r32.abs().clamp_min(2.0 ** -126))
    ulp = torch.ldexp(torch.ones_like(r32), e - 24).double()
    worst = float(((got - ref64).abs() / ulp).max())
    print(f"  [{what}] worst |err| {worst:.4f} ulp")
    assert worst <= 0.5 * (1.0 + 2.0 ** -20), f"{what}: {worst} ulp"


def counts(ops, entry):
    if entry == "gemm":
        from lr2ppo_amd import _native
        c = (ctypes.c_uint64 * 3)()
        assert _native.lib().lr2_gemm_launch_counts(c) == 0
        return tuple(int(x) for x in c)
    return ops.gemm_bf16_launch_counts() if entry == "bf16" else ops.gemm_bf16_train_launch_counts()


def tile_rows(M, N):
    from lr2ppo_amd import _native
    r = ctypes.c_int(0)
    assert _native.lib().lr2_gemm256_tile_rows(M, N, ctypes.byref(r)) == 0
    assert r.value == GC.tile_rows_256(M, N)
    return r.value


def reached(family, case):
    REACH.setdefault(family, []).append(case)


def rounded(x, passes):
    return x.float().bfloat16().double() if passes == 1 else x


def keep_mask(M, N):
    p, seed, site = GC.DROP
    return torch.from_numpy(O.dropout_keep_mask(seed, site, M * N, p)).view(M, N)


# ---- the runner of one lr2_gemm case ----------------------------------------------------------------------------------------------
def run_gemm(ops, dev, form, kinds, bm, passes, M, N, K, splits, cls, epi, expect, colsum=False, seed=0):
    e = GC.EPI[epi]
    colsum = colsum or bool(e.get("colsum"))
    s = GC.strides(M, N, K, form)
    a, b = GC.operands(cls, M, N, K, seed)
    ins = GC.epilogue_inputs(epi, M, N, seed)
    keep = keep_mask(M, N) if e.get("drop") else None
    prod = rounded(a, passes) @ rounded(b, passes).t()
    ref, z_ref = GC.reference(epi, prod, ins, keep)
    # storage: A [M, K] (NT, NN) or [K, M] (TN); B [N, K] (NT) or [K, N] (NN, TN); NaN rows behind the row-major operands
    a_st = operand(ops, kinds[0], a.t() if form == "TN" else a, (K if form == "TN" else M + XROWS), s.lda, dev)
    b_st = operand(ops, kinds[1], b if form == "NT" else b.t(), (N + XROWS if form == "NT" else K), s.ldb, dev)
    out = None if e.get("no_out") else dest32(M, N, s.ld_out, dev, ins.get("acc"))
    kw = dict(trans_a=form == "TN", trans_b=form != "NT", lda=s.lda, ldb=s.ldb, ld_out=s.ld_out, block_m=bm, passes=passes,
              splits=splits, alpha=e.get("alpha", 1.0), act=e.get("act", 0), accumulate=bool(e.get("acc")))
    if "bias" in ins:
        kw["bias"] = ins["bias"].float().to(dev)
    if "resid" in ins:
        kw["resid"] = padded(ins["resid"], M + XROWS, s.ld_resid, dev)
    if "aux" in ins:
        kw["aux_z"] = padded(ins["aux"], M + XROWS, s.ld_aux, dev)
    z = pl = ws = cs = None
    if e.get("keep_z"):
        z = kw["out_z"] = dest32(M, N, s.ld_z, dev)
    if e.get("planes"):
        pl = PlanesDest(ops, M, N, s.ld_planes, dev)
        kw["out_planes"] = pl.planes
    if e.get("drop"):
        kw["drop"] = ops.Drop(*GC.DROP)
    if splits > 1:
        ws = kw["splitk_ws"] = ws_dest(splits, M, N, dev)
    if colsum:
        cs = torch.full((M + XROWS,), PAT32, dtype=torch.int32, device=dev).view(torch.float32)
        kw["colsum"] = cs[:M]
        kw["colsum_ws"] = torch.full((max(128, splits * ((N + 255) // 256)) * M,), NAN, device=dev)
    c0 = counts(ops, "gemm")
    ops.gemm(a_st, b_st, out, M, N, K, **kw)
    torch.cuda.synchronize()
    delta = tuple(x - y for x, y in zip(counts(ops, "gemm"), c0))
    assert delta == expect, (delta, expect)
    what = f"{form} {kinds} bm{bm} x{passes} {M}x{N}x{K} s{splits} {cls} {epi}"
    if out is None:           # planes alone: the value they hold (hi + lo carries 16 bits: 2^-17 |ref|, inside the rule's 5e-5 |ref|)
        hi, _, lo = pl.parts()
        got = hi[:M, :N].view(torch.bfloat16).float() + lo[:M, :N].view(torch.bfloat16).float()
    else:
        got = out[:M, :N]
    assert not torch.isnan(got).any(), "poison reached the result (or an element was not written)"
    if cls == "rand" or e.get("tol"):
        close(got, ref, *tol(passes, K), what)
    else:
        want = ref.float() if out is not None else sum(GC.rne_split(ref)).float()
        assert torch.equal(got.cpu(), want), f"{what}: max err {float((got.cpu().double() - ref).abs().max())}"
    if z is not None:
        if cls == "rand":
            close(z[:M, :N], z_ref, *tol(passes, K), what + " z")
        else:
            assert torch.equal(z[:M, :N].cpu(), z_ref.float()), what + ": kept pre-activation"
        assert canary32_ok(z, M, N), "out_z written outside [0:M, 0:N]"
    if out is not None:
        assert canary32_ok(out, M, N), "out written outside [0:M, 0:N]"
    if pl is not None:      # bit-equal to the split of the fp32 result (of the exact reference when there is no fp32 result)
        if out is not None or not (cls == "rand" or e.get("tol")):
            pl.check(ops, got if out is not None else ref.float().to(dev))
        else:
            pl.check(ops, None)
    if ws is not None:
        assert bool((ws.view(torch.int32)[splits * M * N:] == PAT32).all()), "split-K workspace written past splits * M * N"
    if cs is not None:
        assert bool((cs.view(torch.int32)[M:] == PAT32).all()), "colsum written past M"
        assert torch.equal(cs[:M].cpu(), a.sum(1).float()), what + ": column sums"        # colsum[m] = sum_k A[k, m]
    return delta


@pytest.mark.parametrize("case", GC.GENERAL, ids=lambda c: "-".join(str(v) for v in c))
def test_general_family(ops, dev, case):
    form, kinds, bm, passes, M, N, K, splits, cls, epi = case
    run_gemm(ops, dev, form, kinds, bm, passes, M, N, K, splits, cls, epi, (0, 0, 1))
    reached("lr2_gemm general", case)


@pytest.mark.parametrize("case", GC.NT256, ids=lambda c: "-".join(str(v) for v in c))
def test_gemm256_nt(ops, dev, case):
    M, N, K, cls, epi = case
    rows = tile_rows(M, N)
    run_gemm(ops, dev, "NT", "pp", 256, 3, M, N, K, 1, cls, epi, (1, 0, 0))
    reached(f"lr2_gemm 256 NT, {rows}-row tiles", case)


def test_gemm256_nt_two_requests_fall_back(ops, dev):
    """resid + accumulate are two per-element requests: block_m = 256 runs on the general family, and is still exact."""
    M, N, K, cls, epi = GC.NT256_TWO_REQUESTS
    run_gemm(ops, dev, "NT", "pp", 256, 3, M, N, K, 1, cls, epi, (0, 0, 1))
    reached("lr2_gemm general", GC.NT256_TWO_REQUESTS)


@pytest.mark.parametrize("case", GC.TN256, ids=lambda c: "-".join(str(v) for v in c))
def test_gemm256_tn(ops, dev, case):
    M, N, K, splits, cls, epi, colsum = case
    run_gemm(ops, dev, "TN", "pp", 256, 3, M, N, K, splits, cls, epi, (0, 1, 0), colsum=colsum)
    reached("lr2_gemm 256 TN", case)


def test_fused_adamw_at_a_ragged_shape(ops, dev):
    """The optimizer step in the epilogue of a ragged TN product against lr2_adamw_multi on the exact gradient: same bits in p, m, v."""
    from lr2ppo_amd import _native as nat
    M, N, K = 100, 132, 33
    s = GC.strides(M, N, K, "TN")
    a, b = GC.operands("exactA", M, N, K, 3)
    grad = (0.5 * (a @ b.t())).float()
    assert GC.is_fp32(0.5 * (a @ b.t()))
    g = torch.Generator().manual_seed(9)
    p0, m0, v0 = torch.randn(M, N, generator=g), torch.randn(M, N, generator=g) * 0.1, torch.rand(M, N, generator=g) * 0.01
    hp = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-6, weight_decay=0.01)

    def state(t):            # [M, N] at the head of an [M + 3, N] buffer (the wrapper wants p, m, v tight), canary rows behind it
        buf = dest32(M, N, N, dev, t)
        return buf, buf[:M]

    (pbuf, pa), (mbuf, ma), (vbuf, va) = state(p0), state(m0), state(v0)
    a_st, b_st = operand(ops, "p", a.t(), K, s.lda, dev), operand(ops, "p", b.t(), K, s.ldb, dev)
    c0 = counts(ops, "gemm")
    ops.gemm(a_st, b_st, None, M, N, K, trans_a=True, trans_b=True, lda=s.lda, ldb=s.ldb, alpha=0.5, block_m=128, splits=1,
             adam=ops.AdamArgs(pa, ma, va, **hp))
    assert tuple(x - y for x, y in zip(counts(ops, "gemm"), c0)) == (0, 0, 1)
    pb, mb, vb, gd = (t.clone().to(dev) for t in (p0, m0, v0, grad))
    arr = (nat.AdamChunk * 1)()
    arr[0].p, arr[0].g, arr[0].m, arr[0].v, arr[0].count, arr[0].weight_decay = pb.data_ptr(), gd.data_ptr(), mb.data_ptr(), \
        vb.data_ptr(), M * N, hp["weight_decay"]
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    ops.adamw_multi(table, 1, hp["lr"], hp["beta1"], hp["beta2"], hp["eps"])
    torch.cuda.synchronize()
    assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb)
    assert canary32_ok(pbuf, M, N) and canary32_ok(mbuf, M, N) and canary32_ok(vbuf, M, N)
    assert not torch.equal(pa.cpu(), p0)


# ---- single-plane entry points ------------------------------------------------------------------------------------------------------
def run_b1(ops, dev, entry, M, N, K, bm, epi, dst, seed=0):
    """One NT case of gemm_bf16 (entry "bf16") or gemm_bf16_train (entry "bf16_train"); returns the counter delta."""
    e = GC.EPI[epi]
    s = GC.strides(M, N, K, "NT")
    a, b = GC.operands("int", M, N, K, seed)
    ins = GC.epilogue_inputs(epi, M, N, seed)
    keep = keep_mask(M, N) if e.get("drop") else None
    prod = a @ b.t()
    ref, z_ref = GC.reference(epi, prod, ins, keep)
    a_st, b_st = operand(ops, "b", a, M + XROWS, s.lda, dev), operand(ops, "b", b, N + XROWS, s.ldb, dev)
    kw = dict(lda=s.lda, ldb=s.ldb, block_m=bm, alpha=e.get("alpha", 1.0), act=e.get("act", 0))
    out = None
    if dst not in ("plane", "planes_only"):
        out = dest32(M, N, s.ld_out, dev, ins.get("acc"))
        kw["ld_out"] = s.ld_out
    if "bias" in ins:
        kw["bias"] = ins["bias"].float().to(dev)
    if "resid" in ins:
        kw["resid"] = padded(ins["resid"], M + XROWS, s.ld_resid, dev)
    z = pl = one = None
    if entry == "bf16_train":
        kw["accumulate"] = bool(e.get("acc"))
        if "aux" in ins:
            kw["aux_z"] = padded(ins["aux"], M + XROWS, s.ld_aux, dev)
        if e.get("keep_z"):
            z = kw["out_z"] = dest32(M, N, s.ld_z, dev)
        if e.get("drop"):
            kw["drop"] = ops.Drop(*GC.DROP)
    col0 = 0
    if dst in ("planes_col", "planes_only"):          # gemm_bf16: columns [8, 8 + N) of a wider planes matrix
        col0 = 8
        pl = PlanesDest(ops, M, N, col0 + N + 12, dev, col0)
        kw["out_planes"], kw["planes_col"] = pl.planes, col0
    elif dst == "out+planes":        # gemm_bf16_train: [M, N] by the wrapper's rule; canary rows and a gap behind each plane
        pl = PlanesDest(ops, M, N, N, dev)
        kw["out_planes"] = pl.planes
    elif dst in ("out+plane", "plane"):
        one = kw["out_plane"] = plane_dest(M, N, dev)
    fn = ops.gemm_bf16 if entry == "bf16" else ops.gemm_bf16_train
    c0 = counts(ops, entry)
    fn(a_st, b_st, out, M, N, K, **kw)
    torch.cuda.synchronize()
    delta = tuple(x - y for x, y in zip(counts(ops, entry), c0))
    what = f"{entry} bm{bm} {M}x{N}x{K} {epi} {dst}"
    if out is not None:
        got = out[:M, :N]
        assert not torch.isnan(got).any(), "poison reached the result (or an element was not written)"
        if e.get("act") == 2 and entry == "bf16_train":
            half_ulp_ok(got, ref, what)                  # the EXACT kernels: one rounding of product x GELU'(z)
        elif e.get("tol"):
            close(got, ref, *tol(1, K), what)
        else:
            assert torch.equal(got.cpu(), ref.float()), f"{what}: max err {float((got.cpu().double() - ref).abs().max())}"
        assert canary32_ok(out, M, N), "out written outside [0:M, 0:N]"
        if pl is not None:
            pl.check(ops, got)
        if one is not None:
            check_plane(one, got, M, N)
    else:
        assert not e.get("tol")
        if one is not None:
            check_plane(one, ref.float().to(dev), M, N)
        else:
            pl.check(ops, ref.float().to(dev))
    if z is not None:
        assert torch.equal(z[:M, :N].cpu(), z_ref.float()), what + ": kept pre-activation"
        assert canary32_ok(z, M, N), "out_z written outside [0:M, 0:N]"
    return delta


@pytest.mark.parametrize("case", GC.B1, ids=lambda c: "-".join(str(v) for v in c))
def test_gemm_bf16(ops, dev, case):
    M, N, K, bm, epi, dst = case
    delta = run_b1(ops, dev, "bf16", M, N, K, bm, epi, dst)
    assert delta == ((1, 0) if bm == 256 else (0, 1))
    reached(f"gemm_bf16 256 NT, {tile_rows(M, N)}-row tiles" if bm == 256 else "gemm_bf16 general", case)


@pytest.mark.parametrize("case", GC.B1T_NT, ids=lambda c: "-".join(str(v) for v in c))
def test_gemm_bf16_train_nt(ops, dev, case):
    M, N, K, bm, epi, dst = case
    delta = run_b1(ops, dev, "bf16_train", M, N, K, bm, epi, dst)
    on256 = bm == 256 and epi != "resid_acc"             # two requests: the general family
    assert delta == ((1, 0, 0) if on256 else (0, 0, 1))
    fam = f"256 NT, {tile_rows(M, N)}-row tiles" if on256 else "general"
    reached(f"gemm_bf16_train {fam}" + (", exact GELU'" if epi == "act2" else ""), case)


@pytest.mark.parametrize("case", GC.B1T_TN, ids=lambda c: "-".join(str(v) for v in c))
def test_gemm_bf16_train_tn(ops, dev, case):
    M, N, K, bm, splits, alpha, colsum = case
    s = GC.strides(M, N, K, "TN")
    a, b = GC.operands("int", M, N, K)
    ref = (alpha * (a @ b.t())).float()
    a_st, b_st = operand(ops, "b", a.t(), K, s.lda, dev), operand(ops, "b", b.t(), K, s.ldb, dev)
    out = dest32(M, N, s.ld_out, dev)
    kw = dict(trans=True, lda=s.lda, ldb=s.ldb, ld_out=s.ld_out, alpha=alpha, block_m=bm, splits=splits)
    ws = cs = None
    if splits > 1:
        ws = kw["splitk_ws"] = ws_dest(splits, M, N, dev)
    if colsum:
        cs = torch.full((M + XROWS,), PAT32, dtype=torch.int32, device=dev).view(torch.float32)
        kw["colsum"], kw["colsum_ws"] = cs[:M], torch.full((max(128, splits * ((N + 255) // 256)) * M,), NAN, device=dev)
    c0 = counts(ops, "bf16_train")
    ops.gemm_bf16_train(a_st, b_st, out, M, N, K, **kw)
    torch.cuda.synchronize()
    delta = tuple(x - y for x, y in zip(counts(ops, "bf16_train"), c0))
    assert delta == ((0, 1, 0) if bm == 256 else (0, 0, 1))
    assert torch.equal(out[:M, :N].cpu(), ref), f"max err {float((out[:M, :N].cpu().double() - ref.double()).abs().max())}"
    assert canary32_ok(out, M, N), "out written outside [0:M, 0:N]"
    if ws is not None:
        assert bool((ws.view(torch.int32)[splits * M * N:] == PAT32).all()), "split-K workspace written past splits * M * N"
    if cs is not None:
        assert torch.equal(cs[:M].cpu(), a.sum(1).float()), "column sums"
        assert bool((cs.view(torch.int32)[M:] == PAT32).all()), "colsum written past M"
    reached("gemm_bf16_train 256 TN" if bm == 256 else "gemm_bf16_train general", case)


# ---- ragged K and the extents ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["gemm_fp32", "gemm_planes", "gemm_planes_256", "bf16_train", "bf16_train_256"])
def test_ragged_k_operands_inside_taller_buffers(ops, dev, how):
    """TN form, K = 100: the operands are the first K rows of buffers that hold K + 40 rows, the extra rows NaN.  The kernels never
    compare a row with K -- rows past it read as zero only because the extents passed down end there -- so the wrappers must pass the
    extent of K rows, not of the allocation.  Before ops.gemm did, rows K .. the end of the last K tile were added into the product."""
    M, N, K, extra = 132, 128, 100, 40
    s = GC.strides(M, N, K, "TN")
    single = how.startswith("bf16")
    a, b = GC.operands("int" if single else "exactA", M, N, K)
    ref = (a @ b.t()).float()
    kind = "b" if single else ("f" if how == "gemm_fp32" else "p")
    a_st, b_st = operand(ops, kind, a.t(), K + extra, s.lda, dev), operand(ops, kind, b.t(), K + extra, s.ldb, dev)
    out = dest32(M, N, s.ld_out, dev)
    bm = 256 if how.endswith("256") else 128
    if single:
        ops.gemm_bf16_train(a_st, b_st, out, M, N, K, trans=True, lda=s.lda, ldb=s.ldb, ld_out=s.ld_out, block_m=bm, splits=1)
    else:
        ops.gemm(a_st, b_st, out, M, N, K, trans_a=True, trans_b=True, lda=s.lda, ldb=s.ldb, ld_out=s.ld_out, block_m=bm, splits=1)
    torch.cuda.synchronize()
    got = out[:M, :N].cpu()
    assert not torch.isnan(got).any(), "rows past K were added into the product"
    assert torch.equal(got, ref)
    assert canary32_ok(out, M, N)


# ---- the row-split seam -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seam(dev):
    """Operands and fp64 references of the seam shape, computed once."""
    M, N, K = GC.SEAM
    out = {}
    for cls in ("exactA", "int"):
        a, b = GC.operands(cls, M, N, K)
        bias = GC.epilogue_inputs("gelu_z_planes", M, N)["bias"]
        resid = GC.epilogue_inputs("resid", M, N)["resid"]
        prod = a @ b.t()
        out[cls] = dict(a=a, b=b, bias=bias, resid=resid, z=(prod + bias).float(), gelu=GC.gelu64(prod + bias), sum=(prod + resid).float())
    return out


@pytest.mark.parametrize("entry", ["gemm", "bf16", "bf16_train"])
def test_row_split_seam(ops, dev, seam, entry):
    """M = 32 768 + 200: one whole round of 256 x 256 tiles and a tail of 64-row tiles (test_gemm_edges_cpu.py asserts the plan).  Every
    epilogue pointer of the second launch is advanced by 32 768 rows of ITS OWN leading dimension."""
    M, N, K = GC.SEAM
    assert GC.row_split_plan(M, N, K) == (32768, 64)
    s = GC.strides(M, N, K, "NT")
    d = seam["exactA" if entry == "gemm" else "int"]
    kind = "p" if entry == "gemm" else "b"
    a_st, b_st = operand(ops, kind, d["a"], M + XROWS, s.lda, dev), operand(ops, kind, d["b"], N + XROWS, s.ldb, dev)
    bias = d["bias"].float().to(dev)
    resid = padded(d["resid"], M + XROWS, s.ld_resid, dev)
    fn = {"gemm": ops.gemm, "bf16": ops.gemm_bf16, "bf16_train": ops.gemm_bf16_train}[entry]
    passes = 3 if entry == "gemm" else 1
    common = dict(lda=s.lda, ldb=s.ldb, ld_out=s.ld_out, block_m=256)
    if entry == "gemm":
        common.update(splits=1, passes=3)
    # 1. bias + GELU (+ the kept pre-activation where the entry point has one) + planes
    out = dest32(M, N, s.ld_out, dev)
    z = dest32(M, N, s.ld_z, dev) if entry != "bf16" else None
    kw = dict(common, bias=bias, act=1)
    if z is not None:
        kw["out_z"] = z
    if entry == "gemm":
        pl = PlanesDest(ops, M, N, s.ld_planes, dev)
    elif entry == "bf16":
        pl = PlanesDest(ops, M, N, 8 + N + 12, dev, 8)
        kw["planes_col"] = 8
    else:
        pl = PlanesDest(ops, M, N, N, dev)
    kw["out_planes"] = pl.planes
    c0 = counts(ops, entry)
    fn(a_st, b_st, out, M, N, K, **kw)
    torch.cuda.synchronize()
    delta = tuple(x - y for x, y in zip(counts(ops, entry), c0))
    assert delta == {"gemm": (1, 0, 1), "bf16": (1, 1), "bf16_train": (1, 0, 1)}[entry]      # two launches
    got = out[:M, :N]
    if z is not None:
        assert torch.equal(z[:M, :N], d["z"].to(dev)), "kept pre-activation across the seam"
        assert canary32_ok(z, M, N)
    atol, rtol = tol(passes, K)
    ref = d["gelu"].to(dev)
    err = (got.double() - ref).abs()
    print(f"  [seam {entry} gelu] max |err| {float(err.max()):.3e}")
    assert bool((err <= atol + rtol * ref.abs()).all())
    assert canary32_ok(out, M, N)
    pl.check(ops, got)
    # 2. residual: the whole result is exact
    out2 = dest32(M, N, s.ld_out, dev)
    c0 = counts(ops, entry)
    fn(a_st, b_st, out2, M, N, K, **dict(common, resid=resid))
    torch.cuda.synchronize()
    assert tuple(x - y for x, y in zip(counts(ops, entry), c0)) == {"gemm": (1, 0, 1), "bf16": (1, 1), "bf16_train": (1, 0, 1)}[entry]
    assert torch.equal(out2[:M, :N], d["sum"].to(dev)), "product + residual across the seam"
    assert canary32_ok(out2, M, N)
    reached({"gemm": "lr2_gemm", "bf16": "gemm_bf16", "bf16_train": "gemm_bf16_train"}[entry] + " row split (256 NT + general)", GC.SEAM)


def test_every_family_was_reached():
    """Across the file the launch counters showed every kernel family (asserted only when the whole file ran)."""
    for fam in sorted(REACH):
        print(f"  {fam}: {len(REACH[fam])} cases")
    if sum(len(v) for v in REACH.values()) < N_CASES + 3:
        return
    want = ["lr2_gemm general", "lr2_gemm 256 NT, 192-row tiles", "lr2_gemm 256 NT, 256-row tiles", "lr2_gemm 256 TN",
            "gemm_bf16 general", "gemm_bf16 256 NT, 192-row tiles", "gemm_bf16 256 NT, 256-row tiles",
            "gemm_bf16_train general", "gemm_bf16_train general, exact GELU'", "gemm_bf16_train 256 TN",
            "gemm_bf16_train 256 NT, 192-row tiles", "gemm_bf16_train 256 NT, 256-row tiles",
            "gemm_bf16_train 256 NT, 192-row tiles, exact GELU'", "gemm_bf16_train 256 NT, 256-row tiles, exact GELU'",
            "lr2_gemm row split (256 NT + general)", "gemm_bf16 row split (256 NT + general)",
            "gemm_bf16_train row split (256 NT + general)"]
    assert not [f for f in want if f not in REACH], [f for f in want if f not in REACH]
