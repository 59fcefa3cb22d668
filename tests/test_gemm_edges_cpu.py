"""The CPU half of the GEMM edge suite (tests/gemm_cases.py, test_gemm_edges_gpu.py): the exact operand classes are what they claim to
be for every (shape, class) of the tables, the restated tile-height and row-split rules agree with the library, and lr2_gemm /
lr2_gemm_bf16 refuse bad arguments before launching anything (lr2_gemm_bf16_train's matrix is in test_bf16_train_cpu.py; the
leading-dimension refusals of all three entry points are here)."""
import ctypes

import pytest
import torch

import gemm_cases as GC


# ---- the operand classes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls, M, N, K", GC.all_exact_cases(), ids=lambda v: str(v))
def test_exact_classes_are_exact(cls, M, N, K):
    a, b = GC.operands(cls, M, N, K)
    assert GC.is_fp32(a) and GC.is_fp32(b)
    assert GC.exact_condition(a, b) < 2.0 ** 24, (cls, M, N, K)
    a_hi, a_lo = GC.rne_split(a)
    b_hi, b_lo = GC.rne_split(b)
    assert torch.equal(a_hi + a_lo, a) and torch.equal(b_hi + b_lo, b)           # two planes hold the value
    if cls == "exactA":
        split, whole = (a, a_hi, a_lo), (b, b_hi, b_lo)
    elif cls == "exactB":
        split, whole = (b, b_hi, b_lo), (a, a_hi, a_lo)
    else:
        assert not a_lo.any() and not b_lo.any()                                 # bf16 numbers: one plane holds them
        return
    x, hi, lo = split
    assert torch.equal(hi, torch.round(x)) and bool((hi.abs() >= 5).all()) and bool((hi.abs() <= 7).all())   # hi = h
    assert torch.equal(lo * 512.0, torch.round(lo * 512.0)) and bool((lo.abs() * 512.0 <= 7).all())         # lo = j / 512
    if x.numel() >= 64:
        assert float((lo != 0).double().mean()) > 0.8                            # a lo-plane addressing error is visible
    assert not whole[2].any() and torch.equal(whole[0], torch.round(whole[0]))   # the other side: integers, zero lo plane
    # asymmetry: neither operand repeats along rows or columns
    if min(whole[0].shape) >= 8:
        w = whole[0]
        assert not torch.equal(w[0], w[1]) and not torch.equal(w[:, 0], w[:, 1])
    # the fp64 product is an fp32 number, and so is every epilogue of the exact kind applied to it
    prod = a @ b.t()
    assert GC.is_fp32(prod)
    for epi in ("alpha_half", "bias", "acc_alpha2", "drop_resid", "resid_acc"):
        ins = GC.epilogue_inputs(epi, M, N)
        keep = torch.ones(M, N)
        out, _ = GC.reference(epi, prod, ins, keep)
        assert GC.is_fp32(out), epi


def test_reference_epilogue_order():
    """alpha and bias before GELU, dropout before the residual, accumulate last (include/lr2ppo_hip.h)."""
    prod = torch.tensor([[2.0, -4.0]], dtype=torch.float64)
    ins = {"bias": torch.tensor([1.0, 1.0], dtype=torch.float64), "resid": torch.tensor([[10.0, 10.0]], dtype=torch.float64)}
    keep = torch.tensor([[1.0, 0.0]])
    out, z = GC.reference("drop_resid", prod, ins, keep)
    assert z is None and out.tolist() == [[(2.0 + 1.0) * 2.0 + 10.0, 10.0]]
    out, z = GC.reference("gelu_z_planes", prod, {"bias": ins["bias"]})
    assert z.tolist() == [[3.0, -3.0]] and torch.allclose(out, GC.gelu64(z))
    zz = torch.linspace(-4, 4, 33, dtype=torch.float64).requires_grad_(True)
    GC.gelu64(zz).sum().backward()
    assert torch.allclose(GC.gelu_grad64(zz.detach()), zz.grad, rtol=1e-13, atol=1e-15)


def test_strides_are_distinct_and_legal():
    for form in ("NT", "NN", "TN"):
        for M, N, K in ((1, 4, 1), (129, 132, 100), (257, 260, 96)):
            s = GC.strides(M, N, K, form)
            assert s.lda % 8 == 0 and s.ldb % 8 == 0 and all(v % 4 == 0 for v in s[2:])
            assert s.lda > (M if form == "TN" else K) and s.ldb > (K if form == "NT" else N) and min(s[2:]) > N
            assert len(set(s[2:])) == 5 and s.ld_planes % 4 == 0


# ---- the dispatch rules, restated ---------------------------------------------------------------------------------------------------
def _lib():
    from lr2ppo_amd import _native as native
    return native, native.lib()


def test_tile_height_rule():
    _, lib = _lib()
    r = ctypes.c_int(0)
    shapes = [(M, N) for M, N, *_ in GC.NT256] + [(M, N) for M, N, *_ in GC.B1 + GC.B1T_NT] + \
        [(512, 512), (256, 256), (600, 512), (12544, 768), (12544, 3072), (100864, 768), GC.SEAM[:2], (32768, 512)]
    for M, N in shapes:
        assert lib.lr2_gemm256_tile_rows(M, N, ctypes.byref(r)) == 0 and r.value == GC.tile_rows_256(M, N), (M, N)
    # the shapes of the older "gemm256" exactness tests run 192-row tiles
    assert GC.tile_rows_256(512, 512) == 192 and GC.tile_rows_256(256, 256) == 192
    # a single tile row holds M <= 192 either way: the launcher keeps the 256-row form
    assert [GC.tile_rows_256(M, 256) for M in (1, 191, 192, 193, 256, 257, 320, 384, 512)] == [256, 256, 256, 192, 192, 256, 256, 256, 192]
    # both heights are reached by the tables of every entry point
    for table in (GC.NT256, [c for c in GC.B1 if c[3] == 256], [c for c in GC.B1T_NT if c[3] == 256]):
        assert {GC.tile_rows_256(c[0], c[1]) for c in table} == {192, 256}
    assert lib.lr2_gemm256_tile_rows(0, 4, ctypes.byref(r)) == -1 and lib.lr2_gemm256_tile_rows(4, 4, None) == -1


def test_row_split_plan_of_the_seam_case():
    _, lib = _lib()
    M, N, K = GC.SEAM
    r, t = ctypes.c_int(-1), ctypes.c_int(-1)
    assert lib.lr2_gemm_row_split_plan(M, N, K, ctypes.byref(r), ctypes.byref(t)) == 0
    assert (r.value, t.value) == (32768, 64) == GC.row_split_plan(M, N, K)
    assert GC.tile_rows_256(32768, N) == 256                     # the leading launch: one whole round of 256-row tiles
    for shape in ((12544, 3072, 768), (600, 512, 256), (32768, 512, 64), (M, N, 96), (25088, 768, 3072)):
        assert lib.lr2_gemm_row_split_plan(*shape, ctypes.byref(r), ctypes.byref(t)) == 0
        assert (r.value, t.value) == GC.row_split_plan(*shape), shape


# ---- refusals: nothing is launched by a rejected call -------------------------------------------------------------------------------
A = 16          # a stand-in device address (nothing is dereferenced: every call fails)
ARG, SHAPE = -1, -2


def _epi(native, **kw):
    e = native.Epilogue()
    e.out, e.ld_out, e.alpha = A, 256, 1.0
    for k, v in kw.items():
        setattr(e, k, v)
    return e


def test_gemm_validates_before_launching():
    native, lib = _lib()

    def epi(**kw):
        return ctypes.byref(_epi(native, **kw))

    def call(e, *, a=A, b=A, M=256, N=256, K=64, lda=None, ldb=None, ta=0, tb=0, a_bytes=None, b_bytes=None, ap=0, bp=0, a_lo=None,
             b_lo=None, ws=None, splits=1, bm=128, passes=3):
        lda = (M if ta else K) if lda is None else lda
        ldb = (N if tb else K) if ldb is None else ldb
        el_a, el_b = (2 if ap else 4), (2 if bp else 4)
        a_bytes = M * K * el_a if a_bytes is None else a_bytes
        b_bytes = N * K * el_b if b_bytes is None else b_bytes
        a_lo = (a_bytes if ap else 0) if a_lo is None else a_lo
        b_lo = (b_bytes if bp else 0) if b_lo is None else b_lo
        return lib.lr2_gemm(a, b, M, N, K, lda, ldb, ta, tb, a_bytes, b_bytes, ap, a_lo, bp, b_lo, e, ws, splits, bm, passes, None)

    before = (ctypes.c_uint64 * 3)()
    assert lib.lr2_gemm_launch_counts(before) == 0
    forms = ((0, 0), (0, 1), (1, 1))
    for ta, tb in forms:
        f = dict(ta=ta, tb=tb)
        assert call(epi(), a=None, **f) == ARG and call(epi(), b=None, **f) == ARG            # null operands
        assert call(None, **f) == ARG                                                        # no epilogue
        assert call(epi(out=None), **f) == ARG                                               # no destination
        assert call(epi(), M=0, **f) == ARG and call(epi(), N=0, **f) == ARG and call(epi(), K=0, **f) == ARG
        for passes in (0, 2, 4):
            assert call(epi(), passes=passes, **f) == ARG
        assert call(epi(), bp=1, **f) == ARG                                                 # (fp32 A, planes B)
        assert call(epi(out=None, out_hi=A, ld_planes=256, accumulate=1), **f) == ARG        # accumulate without `out`
        # the fused optimizer step excludes `out`, planes and dropout; needs m and v
        adam = dict(out=None, adam_p=A, adam_m=A, adam_v=A)
        assert call(epi(**{**adam, "out": A}), **f) == ARG
        assert call(epi(**adam, out_hi=A, ld_planes=256), **f) == ARG
        assert call(epi(**adam, drop_p=0.1), **f) == ARG
        assert call(epi(**{**adam, "adam_m": None}), **f) == ARG and call(epi(**{**adam, "adam_v": None}), **f) == ARG
        assert call(epi(**adam, ld_out=258), **f) == ARG
        assert call(epi(drop_p=0.1, drop_seed_dev=A, drop_site=65536), **f) == ARG            # the site travels in 16 bits
        # GELU' needs its input; act is 0, 1 or 2 (new with this suite: a NULL aux_z was dereferenced by the kernel)
        for bm in (64, 128, 256):
            assert call(epi(act=2), bm=bm, ap=1, bp=1, **f) == ARG
            assert call(epi(act=2), bm=bm, **f) == ARG
        assert call(epi(act=3), **f) == ARG and call(epi(act=-1), **f) == ARG and call(epi(act=18, aux_z=A, ld_aux=256), **f) == ARG
        # split-K without a workspace
        assert call(epi(), K=256, splits=2, **f) == ARG
        assert call(epi(), K=256, splits=2, ap=1, bp=1, bm=256 if ta else 128, **f) == ARG
        # N % 4, alignment of every stride
        assert call(epi(), N=254, ldb=256, **f) == SHAPE
        assert call(epi(), lda=258, **f) == SHAPE and call(epi(), ldb=258, **f) == SHAPE      # fp32 rows: multiples of 4
        assert call(epi(), lda=260, ap=1, **f) == SHAPE                                       # planes rows: multiples of 8
        assert call(epi(), lda=264, ldb=260, ap=1, bp=1, **f) == SHAPE
        assert call(epi(ld_out=258), **f) == SHAPE
        assert call(epi(act=1, out_z=A, ld_z=258), **f) == SHAPE
        assert call(epi(resid=A, ld_resid=258), **f) == SHAPE
        assert call(epi(act=2, aux_z=A, ld_aux=258), **f) == SHAPE
        assert call(epi(out_hi=A, ld_planes=258), **f) == SHAPE
        # the 4 GiB limits
        assert call(epi(), a_bytes=1 << 32, **f) == SHAPE and call(epi(), b_bytes=1 << 32, **f) == SHAPE
        assert call(epi(), ap=1, a_lo=1 << 32, **f) == SHAPE and call(epi(), ap=1, bp=1, b_lo=1 << 32, **f) == SHAPE
        # leading dimensions smaller than the row they address (new with this suite; ld = 0 is a zeroed epilogue struct)
        assert call(epi(), lda=(256 if ta else 64) - 8, **f) == SHAPE
        assert call(epi(), ldb=(256 if tb else 64) - 8, **f) == SHAPE
        assert call(epi(), lda=0, **f) == SHAPE and call(epi(), ldb=0, **f) == SHAPE
        for ld in (0, 252):
            assert call(epi(ld_out=ld), **f) == SHAPE
            assert call(epi(act=1, out_z=A, ld_z=ld), **f) == SHAPE
            assert call(epi(resid=A, ld_resid=ld), **f) == SHAPE
            assert call(epi(act=2, aux_z=A, ld_aux=ld), **f) == SHAPE
            assert call(epi(out_hi=A, ld_planes=ld), **f) == SHAPE
            assert call(epi(**adam, ld_out=ld), **f) == SHAPE
    # column sums: the TN form only, with a workspace, M % 4
    assert call(epi(colsum=A, colsum_ws=A)) == ARG and call(epi(colsum=A, colsum_ws=A), tb=1) == ARG
    assert call(epi(colsum=A), ta=1, tb=1) == ARG
    assert call(epi(colsum=A, colsum_ws=A), M=258, lda=264, ta=1, tb=1) == ARG
    assert call(epi(), ta=1, tb=0) == ARG                                                     # (1,0) is no form of the entry
    # K % BK per form and kernel: 64 with an fp32 operand or K-contiguous planes, 32 for planes with a strided B (NN) and on the
    # 256 x 256 NT kernel; the TN form takes any K
    assert call(epi(), K=96) == SHAPE and call(epi(), K=32, tb=1) == SHAPE
    assert call(epi(), K=96, ap=1, bp=1) == SHAPE and call(epi(), K=96, ap=1) == SHAPE and call(epi(), K=96, ap=1, tb=1) == SHAPE
    assert call(epi(), K=48, lda=48, ldb=256, ap=1, bp=1, tb=1) == SHAPE
    assert call(epi(), K=48, lda=48, ldb=48, ap=1, bp=1, bm=256) == SHAPE
    assert call(epi(), K=96, ap=1, bp=1, bm=256, ws=A, splits=2) == SHAPE                     # split-K: not the 256 x 256 NT kernel
    counts = (ctypes.c_uint64 * 3)()
    assert lib.lr2_gemm_launch_counts(counts) == 0 and list(counts) == list(before)           # nothing was launched
    assert lib.lr2_gemm_launch_counts(None) == ARG


def test_gemm_bf16_validates_before_launching():
    native, lib = _lib()

    def epi(**kw):
        return ctypes.byref(_epi(native, **kw))

    def call(e, *, a=A, b=A, M=256, N=256, K=64, lda=None, ldb=None, a_bytes=None, b_bytes=None, bm=256):
        return lib.lr2_gemm_bf16(a, b, M, N, K, K if lda is None else lda, K if ldb is None else ldb,
                                 M * K * 2 if a_bytes is None else a_bytes, N * K * 2 if b_bytes is None else b_bytes, e, bm, None)

    before = (ctypes.c_uint64 * 2)()
    assert lib.lr2_gemm_bf16_launch_counts(before) == 0
    for bm in (256, 128, 64):
        f = dict(bm=bm)
        assert call(epi(), a=None, **f) == ARG and call(epi(), b=None, **f) == ARG and call(None, **f) == ARG
        assert call(epi(out=None), **f) == ARG
        assert call(epi(), M=0, **f) == ARG and call(epi(), N=0, **f) == ARG and call(epi(), K=0, **f) == ARG
        # inference only
        assert call(epi(drop_p=0.5), **f) == ARG
        assert call(epi(act=2, aux_z=A, ld_aux=256), **f) == ARG and call(epi(act=3), **f) == ARG and call(epi(act=-1), **f) == ARG
        assert call(epi(accumulate=1), **f) == ARG
        assert call(epi(act=1, out_z=A, ld_z=256), **f) == ARG
        assert call(epi(out=None, adam_p=A, adam_m=A, adam_v=A), **f) == ARG
        assert call(epi(colsum=A, colsum_ws=A), **f) == ARG
        # whole 64-deep K steps, N % 4, alignment, the 4 GiB limits
        assert call(epi(), K=96, **f) == SHAPE and call(epi(), K=32, **f) == SHAPE
        assert call(epi(), N=254, **f) == SHAPE
        assert call(epi(), lda=68, **f) == SHAPE and call(epi(), ldb=68, **f) == SHAPE
        assert call(epi(ld_out=258), **f) == SHAPE
        assert call(epi(resid=A, ld_resid=258), **f) == SHAPE
        assert call(epi(out_hi=A, ld_planes=258), **f) == SHAPE
        assert call(epi(), a_bytes=1 << 32, **f) == SHAPE and call(epi(), b_bytes=1 << 32, **f) == SHAPE
        # leading dimensions smaller than the row they address (new with this suite)
        assert call(epi(), lda=56, **f) == SHAPE and call(epi(), ldb=56, **f) == SHAPE
        assert call(epi(), lda=0, **f) == SHAPE and call(epi(), ldb=0, **f) == SHAPE
        for ld in (0, 252):
            assert call(epi(ld_out=ld), **f) == SHAPE
            assert call(epi(resid=A, ld_resid=ld), **f) == SHAPE
            assert call(epi(out_hi=A, ld_planes=ld), **f) == SHAPE
            assert call(epi(out=None, out_hi=A, ld_planes=ld), **f) == SHAPE
    counts = (ctypes.c_uint64 * 2)()
    assert lib.lr2_gemm_bf16_launch_counts(counts) == 0 and list(counts) == list(before)
    assert lib.lr2_gemm_bf16_launch_counts(None) == ARG


def test_gemm_bf16_train_refuses_short_leading_dimensions():
    """The leading-dimension refusals of lr2_gemm_bf16_train (the rest of its matrix: test_bf16_train_cpu.py)."""
    native, lib = _lib()

    def epi(**kw):
        return ctypes.byref(_epi(native, **kw))

    def call(e, *, t=0, M=256, N=256, K=64, lda=None, ldb=None, bm=256):
        lda = (M if t else K) if lda is None else lda
        ldb = (N if t else K) if ldb is None else ldb
        return lib.lr2_gemm_bf16_train(A, A, M, N, K, lda, ldb, t, t, M * K * 2, N * K * 2, e, None, 1, bm, None)

    before = (ctypes.c_uint64 * 3)()
    assert lib.lr2_gemm_bf16_train_launch_counts(before) == 0
    for bm in (256, 128, 64):
        for t in (0, 1):
            assert call(epi(), t=t, lda=(256 if t else 64) - 8, bm=bm) == SHAPE
            assert call(epi(), t=t, ldb=(256 if t else 64) - 8, bm=bm) == SHAPE
            assert call(epi(), t=t, lda=0, bm=bm) == SHAPE and call(epi(), t=t, ldb=0, bm=bm) == SHAPE
            for ld in (0, 252):
                assert call(epi(ld_out=ld), t=t, bm=bm) == SHAPE
        for ld in (0, 252):
            assert call(epi(act=1, out_z=A, ld_z=ld), bm=bm) == SHAPE
            assert call(epi(resid=A, ld_resid=ld), bm=bm) == SHAPE
            assert call(epi(act=2, aux_z=A, ld_aux=ld), bm=bm) == SHAPE
            assert call(epi(out_hi=A, ld_planes=ld), bm=bm) == SHAPE
    counts = (ctypes.c_uint64 * 3)()
    assert lib.lr2_gemm_bf16_train_launch_counts(counts) == 0 and list(counts) == list(before)


def test_tables_cover_the_axes():
    """Every edge value of every axis appears with every form (general family) / in every table."""
    for form, ks in (("NT", {64, 128}), ("NN", {32, 96}), ("TN", {1, 31, 32, 33, 63, 65, 100})):
        rows = [c for c in GC.GENERAL if c[0] == form]
        assert {c[4] for c in rows} >= {1, 63, 64, 65, 127, 128, 129}, form
        assert {c[5] for c in rows} >= {4, 124, 128, 132}, form
        assert {c[6] for c in rows} >= ks, form
        assert {c[1] for c in rows} == {"ff", "pp", "pf"} and {c[2] for c in rows} == {64, 128} and {c[3] for c in rows} == {1, 3}
    assert {c[0] for c in GC.NT256} >= {1, 191, 192, 193, 256, 257, 320, 384} and {c[1] for c in GC.NT256} >= {4, 252, 256, 260}
    assert {c[2] for c in GC.NT256} == {32, 64, 96}
    assert {c[0] for c in GC.TN256} == {c[1] for c in GC.TN256} == {4, 252, 256, 260}
    assert {c[2] for c in GC.TN256} == {1, 31, 32, 33, 64, 97}
    assert {c[2] for c in GC.B1} == {c[2] for c in GC.B1T_NT} == {64, 128, 192}
    assert {c[2] for c in GC.B1T_TN if c[3] == 256} == {1, 31, 32, 33, 63, 64, 65, 127, 129}
