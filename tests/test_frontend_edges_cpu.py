"""The CPU half of the front-end edge suite (tests/frontend_cases.py, test_frontend_edges_gpu.py): the argument contracts of the entry
points through the C ABI, the proof that the "exact" input classes are exact, and the check that every case table is consumed by a
GPU test.

Contracts: every call below is rejected before anything is launched, so nothing is dereferenced (each entry point was read: the
refusals asserted here all return above its first LR2_LAUNCH).  -1 = LR2_ERR_ARG (NULL, a count that is not positive), -2 =
LR2_ERR_SHAPE (a size off the vector width or outside the kernel's range, a pointer off the alignment the kernel's vector accesses
need: 16 bytes for what is read or written as float4 / uint4, 8 bytes and lo_off % 4 == 0 for a planes destination, 4 bytes for the
two-element stores of the generic patchify kernel)."""
import ctypes
import importlib

import pytest
import torch

import frontend_cases as FC


@pytest.fixture(scope="module")
def lib():
    from lr2ppo_amd import _native as native
    return native.lib()


A = 64          # a stand-in device address with every alignment the kernels need (nothing is dereferenced: every call fails)
OFF16 = (4, 8, 12)      # byte offsets that break 16-byte alignment
OFF8 = (2, 4, 6)        # ... 8-byte alignment


# ---- argument contracts -------------------------------------------------------------------------------------------------------------
def test_gather_rows_contract(lib):
    g = lib.lr2_gather_rows          # (src, index, dst, B, t_in, t_out, row_elems, src_bstride, src_tstride, stream)
    assert g(None, A, A, 1, 1, 1, 4, 4, 4, None) == -1
    assert g(A, A, None, 1, 1, 1, 4, 4, 4, None) == -1
    for B, ti, to in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1)):
        assert g(A, A, A, B, ti, to, 4, 4, 4, None) == -1
    assert g(A, None, A, 1, 1, 1, 0, 0, 0, None) == -1                    # row_elems == 0: an empty copy, not a launch
    assert g(A, A, A, 1, 1, 1, 6, 8, 8, None) == -2                       # row_elems % 4
    assert g(A, A, A, 1, 1, 1, 4, 6, 4, None) == -2                       # strides % 4
    assert g(A, A, A, 1, 1, 1, 4, 4, 2, None) == -2
    for off in OFF16:
        assert g(A + off, A, A, 1, 1, 1, 4, 4, 4, None) == -2
        assert g(A, A, A + off, 1, 1, 1, 4, 4, 4, None) == -2

    b = lib.lr2_gather_rows_bwd      # (ddst, index, dsrc, B, t_in, t_out, row_elems, stream)
    assert b(None, A, A, 1, 1, 1, 4, None) == -1
    assert b(A, A, None, 1, 1, 1, 4, None) == -1
    for B, ti, to in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        assert b(A, A, A, B, ti, to, 4, None) == -1
    assert b(A, None, A, 1, 1, 1, 0, None) == -1
    assert b(A, A, A, 1, 1, 1, 6, None) == -2
    for off in OFF16:
        assert b(A + off, A, A, 1, 1, 1, 4, None) == -2
        assert b(A, A, A + off, 1, 1, 1, 4, None) == -2


def test_copy_rows_contract(lib):
    c = lib.lr2_copy_rows            # (src, dst, dst_planes, dst_lo_off, rows, D, group, dst_gstride, dst_off, stream)
    assert c(None, A, 0, 0, 1, 4, 1, 4, 0, None) == -1
    assert c(A, None, 0, 0, 1, 4, 1, 4, 0, None) == -1
    for rows, D, group in ((0, 4, 1), (1, 0, 1), (1, 4, 0), (1, -4, 1)):
        assert c(A, A, 0, 0, rows, D, group, 4, 0, None) == -1
    assert c(A, A, 0, 0, 1, 6, 1, 8, 0, None) == -2                       # D % 4
    assert c(A, A, 0, 0, 1, 4, 1, 6, 0, None) == -2                       # dst_gstride % 4
    assert c(A, A, 0, 0, 1, 4, 1, 8, 2, None) == -2                       # dst_off % 4
    for off in OFF16:
        assert c(A + off, A, 0, 0, 1, 4, 1, 4, 0, None) == -2             # float4 loads of src, whatever the destination
        assert c(A + off, A, 1, 8, 1, 4, 1, 4, 0, None) == -2
        assert c(A, A + off, 0, 0, 1, 4, 1, 4, 0, None) == -2             # float4 stores of an fp32 destination
    for off in OFF8:
        assert c(A, A + off, 1, 8, 1, 4, 1, 4, 0, None) == -2             # 4 x bf16 stores: hi plane off 8 bytes
    for lo in (2, 6, 9):
        assert c(A, A, 1, lo, 1, 4, 1, 4, 0, None) == -2                  # ... lo plane off 8 bytes


def test_text_embed_contract(lib):
    t = lib.lr2_text_embed           # (src, seg, word, pos, seg_table, out, rows, L, D, vocab, n_seg, err_flag, stream)
    ok = [A, A, A, A, A, A]
    for i in range(6):
        p = list(ok)
        p[i] = None
        assert t(*p, 1, 1, 4, 10, 2, None, None) == -1
    for rows, L, D, vocab, n_seg in ((0, 1, 4, 10, 2), (1, 0, 4, 10, 2), (1, 1, 0, 10, 2), (1, 1, -4, 10, 2), (1, 1, 4, 0, 2), (1, 1, 4, 10, 0)):
        assert t(*ok, rows, L, D, vocab, n_seg, None, None) == -1
    assert t(*ok, 1, 1, 6, 10, 2, None, None) == -2                       # D % 4
    for i in (2, 3, 4, 5):                                                # word, pos, seg_table, out: float4
        for off in OFF16:
            p = list(ok)
            p[i] = A + off
            assert t(*p, 1, 1, 4, 10, 2, None, None) == -2


def test_text_embed_bwd_contract(lib):
    t = lib.lr2_text_embed_bwd       # (dx, sorted_ids, order, seg, dword, dseg, seg_partials, word_partials, rows, D, vocab, n_seg, stream)
    ok = [A] * 8
    for i in range(8):
        p = list(ok)
        p[i] = None
        assert t(*p, 1, 4, 10, 2, None) == -1
    for rows, D, vocab in ((0, 4, 10), (1, 0, 10), (1, 4, 0), (1, 4, -1)):
        assert t(*ok, rows, D, vocab, 2, None) == -1
    assert t(*ok, 1, 6, 10, 2, None) == -2                                # D % 4
    assert t(*ok, 1, 4, 10, 0, None) == -2                                # n_seg outside [1, 4]
    assert t(*ok, 1, 4, 10, 5, None) == -2
    for i in (0, 4, 7):                                                   # dx, dword, word_partials: the word kernels' float4
        for off in OFF16:
            p = list(ok)
            p[i] = A + off
            assert t(*p, 1, 4, 10, 2, None) == -2


def test_patchify_contract(lib):
    pp = lib.lr2_patchify_planes     # (img, is_u8, out_hi, lo_off, ld, B, C, H, W, ps, mean3, std3, stream)
    assert pp(None, 1, A, 768, 768, 1, 3, 16, 16, 16, None, None, None) == -1
    assert pp(A, 1, None, 768, 768, 1, 3, 16, 16, 16, None, None, None) == -1
    for B, C, H, W, ps in ((0, 3, 16, 16, 16), (1, 0, 16, 16, 16), (1, 3, 0, 16, 16), (1, 3, 16, 0, 16), (1, 3, -16, 16, 16), (1, 3, 16, -16, 16),
                           (1, 3, 16, 16, 0)):
        assert pp(A, 1, A, 768, 768, B, C, H, W, ps, None, None, None) == -1
    assert pp(A, 1, A, 768, 768, 1, 3, 24, 16, 16, None, None, None) == -2    # H % ps
    assert pp(A, 1, A, 768, 768, 1, 3, 16, 24, 16, None, None, None) == -2    # W % ps
    assert pp(A, 1, A, 1024, 1024, 1, 4, 16, 16, 16, None, None, None) == -2  # C > 3
    assert pp(A, 1, A, 148, 148, 1, 3, 7, 7, 7, None, None, None) == -2       # ps odd
    assert pp(A, 1, A, 764, 764, 1, 3, 16, 16, 16, None, None, None) == -2    # ld < Kd
    assert pp(A, 1, A, 770, 770, 1, 3, 16, 16, 16, None, None, None) == -2    # ld % 4
    assert pp(A, 1, A, 769, 768, 1, 3, 16, 16, 16, None, None, None) == -2    # lo_off odd
    for u8 in (0, 1):
        for off in OFF16 + (1, 2):                                            # the strip kernel: uint4 / float4 loads of the image
            assert pp(A + off, u8, A, 768, 768, 1, 3, 16, 16, 16, None, None, None) == -2
        for off in OFF8:                                                      # strip and generic VEC 4: 4 x bf16 stores per plane
            assert pp(A, u8, A + off, 768, 768, 1, 3, 16, 16, 16, None, None, None) == -2
            assert pp(A, u8, A + off, 832, 832, 1, 3, 16, 16, 16, None, None, None) == -2
            assert pp(A, u8, A + off, 192, 192, 1, 3, 8, 8, 8, None, None, None) == -2
        for ps, ld, lo in ((16, 768, 770), (6, 128, 128), (14, 640, 640)):    # generic VEC 2: 2 x bf16 stores, 4 bytes
            assert pp(A, u8, A + 2, lo, ld, 1, 3, ps, ps, ps, None, None, None) == -2
            assert pp(A, u8, A + 6, lo, ld, 1, 3, ps, ps, ps, None, None, None) == -2

    p = lib.lr2_patchify             # (img, out, B, C, H, W, ps, stream)
    assert p(None, A, 1, 3, 16, 16, 16, None) == -1
    assert p(A, None, 1, 3, 16, 16, 16, None) == -1
    for B, C, H, W, ps in ((0, 3, 16, 16, 16), (1, 0, 16, 16, 16), (1, 3, 0, 16, 16), (1, 3, 16, 0, 16), (1, 3, -16, 16, 16), (1, 3, 16, -16, 16),
                           (1, 3, 16, 16, 0)):
        assert p(A, A, B, C, H, W, ps, None) == -1
    assert p(A, A, 1, 3, 24, 16, 16, None) == -2
    assert p(A, A, 1, 3, 16, 24, 16, None) == -2


def test_vit_assemble_contract(lib):
    v = lib.lr2_vit_assemble         # (patch_proj, cls, pos, out, B, P, D, stream)
    ok = [A, A, A, A]
    for i in range(4):
        p = list(ok)
        p[i] = None
        assert v(*p, 1, 1, 4, None) == -1
    for B, Pn, D in ((0, 1, 4), (1, 0, 4), (1, 1, 0), (1, 1, -4)):
        assert v(*ok, B, Pn, D, None) == -1
    assert v(*ok, 1, 1, 6, None) == -2
    for i in range(4):
        for off in OFF16:
            p = list(ok)
            p[i] = A + off
            assert v(*p, 1, 1, 4, None) == -2


def test_xattn_contract(lib):
    f = lib.lr2_xattn_fwd            # (Q, K, V, O, o_planes, o_lo_off, batch, heads, Lq, Lk, head_dim, post_scale, stream)
    ok = [A, A, A, A]
    for i in range(4):
        p = list(ok)
        p[i] = None
        assert f(*p, 0, 0, 1, 1, 1, 1, 4, 1.0, None) == -1
    assert f(*ok, 0, 0, 0, 1, 1, 1, 4, 1.0, None) == -1
    assert f(*ok, 0, 0, 1, 0, 1, 1, 4, 1.0, None) == -1
    shapes = ((0, 1, 4), (257, 1, 4), (1, 0, 4), (1, 17, 4), (1, 1, 0), (1, 1, -4), (1, 1, 100), (1, 1, 6))      # (Lq, Lk, head_dim)
    for Lq, Lk, hd in shapes:
        assert f(*ok, 0, 0, 1, 1, Lq, Lk, hd, 1.0, None) == -2, (Lq, Lk, hd)
    for off in OFF16:
        assert f(A + off, A, A, A, 0, 0, 1, 1, 1, 1, 4, 1.0, None) == -2      # float4 loads of Q
        assert f(A + off, A, A, A, 1, 8, 1, 1, 1, 1, 4, 1.0, None) == -2
        assert f(A, A, A, A + off, 0, 0, 1, 1, 1, 1, 4, 1.0, None) == -2      # float4 stores of an fp32 O
    for off in OFF8:
        assert f(A, A, A, A + off, 1, 8, 1, 1, 1, 1, 4, 1.0, None) == -2      # planes O: hi plane off 8 bytes
    for lo in (2, 6, 9):
        assert f(A, A, A, A, 1, lo, 1, 1, 1, 1, 4, 1.0, None) == -2           # ... lo plane off 8 bytes

    b = lib.lr2_xattn_bwd            # (Q, K, V, dO, dQ, dK, dV, planes, q_lo_off, kv_lo_off, batch, heads, Lq, Lk, head_dim, post_scale, stream)
    ok = [A] * 7
    for i in range(7):
        p = list(ok)
        p[i] = None
        assert b(*p, 0, 0, 0, 1, 1, 1, 1, 4, 1.0, None) == -1
    assert b(*ok, 0, 0, 0, 0, 1, 1, 1, 4, 1.0, None) == -1
    assert b(*ok, 0, 0, 0, 1, 0, 1, 1, 4, 1.0, None) == -1
    for Lq, Lk, hd in shapes:
        assert b(*ok, 0, 0, 0, 1, 1, Lq, Lk, hd, 1.0, None) == -2, (Lq, Lk, hd)
    for i in (0, 3, 4, 5, 6):                                                 # Q, dO: float4 loads; fp32 dQ, dK, dV: float4 stores
        for off in OFF16:
            p = list(ok)
            p[i] = A + off
            assert b(*p, 0, 0, 0, 1, 1, 1, 1, 4, 1.0, None) == -2
    for i in (4, 5, 6):                                                       # planes dQ, dK, dV: 4 x bf16 stores
        for off in OFF8:
            p = list(ok)
            p[i] = A + off
            assert b(*p, 1, 8, 8, 1, 1, 1, 1, 4, 1.0, None) == -2
    for qlo, kvlo in ((6, 8), (8, 6), (9, 8), (8, 2)):
        assert b(*ok, 1, qlo, kvlo, 1, 1, 1, 1, 4, 1.0, None) == -2


def test_ndcg_contract(lib):
    n = lib.lr2_ndcg                 # (scores, gold, offsets, disc, ks, n_k, out, n_items, stream)
    ok = [A, A, A, A, A]
    for i in range(5):
        p = list(ok)
        p[i] = None
        assert n(*p, 1, A, 1, None) == -1
    assert n(*ok, 1, None, 1, None) == -1
    assert n(*ok, 0, A, 1, None) == -1
    assert n(*ok, 1, A, 0, None) == -1


# ---- the exact classes are exact ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FC.XATTN_ONEHOT, ids=FC.ids_of(FC.XATTN_ONEHOT))
def test_one_hot_class_is_exact(case):
    """The kernels' formulas in fp32 torch equal, bit for bit, the closed form O = c V[winner], dQ = dK = 0, dV[j] = c sum of dO over the
    queries that chose j (evaluated in fp64, where it is exact); each winner leads by >= 200 and the winners differ from query to
    query.  The fp64 formula keeps the losers' exp(-200) = 1e-87, so it agrees with the closed form to 1e-80 and no further."""
    q, k, v, do = FC.xattn_inputs(case)
    heads, post = case["heads"], FC.xattn_post_scale(case)
    s = FC._heads(q.double(), heads) @ FC._heads(k.double(), heads).transpose(-1, -2)
    top = s.topk(min(2, case["Lk"]), dim=-1)
    assert torch.equal(top.indices[..., 0], FC.xattn_onehot_winner(case))
    if case["Lk"] > 1:
        assert float((top.values[..., 0] - top.values[..., 1]).min()) >= FC.ONEHOT_LEAD
        if case["Lq"] > 1:
            assert bool((top.indices[..., 0, 0] != top.indices[..., 1, 0]).all())
    assert float(s.abs().max()) < 2 ** 24 and post == 2.0 ** -4
    f32 = FC.xattn_formula(q, k, v, do, heads, post, torch.float32)
    f64 = FC.xattn_formula(q, k, v, do, heads, post, torch.float64)
    closed = FC.xattn_onehot_expected(case, v, do, post)
    for a, b, c in zip(f32, f64, closed):
        assert torch.equal(a.double(), c) and float((b - c).abs().max()) < 1e-80


@pytest.mark.parametrize("case", FC.XATTN_UNIFORM, ids=FC.ids_of(FC.XATTN_UNIFORM))
def test_uniform_class_is_exact(case):
    """Q = 0, Lk a power of two: fp32 equals fp64; O = c / Lk sum V, dV = c / Lk sum dO, dK = 0 and dQ = sum_j dS_j K_j."""
    q, k, v, do = FC.xattn_inputs(case)
    heads, post, Lk = case["heads"], FC.xattn_post_scale(case), case["Lk"]
    f32 = FC.xattn_formula(q, k, v, do, heads, post, torch.float32)
    f64 = FC.xattn_formula(q, k, v, do, heads, post, torch.float64)
    for a, b in zip(f32, f64):
        assert torch.equal(a.double(), b)
    vh, gh = FC._heads(v.double(), heads), FC._heads(do.double(), heads)
    assert torch.equal(FC._heads(f64[0], heads), (post / Lk) * vh.sum(2, keepdim=True).expand(-1, -1, case["Lq"], -1))
    assert torch.equal(FC._heads(f64[3], heads), (post / Lk) * gh.sum(2, keepdim=True).expand(-1, -1, Lk, -1))
    assert not bool(f64[2].any())


@pytest.mark.parametrize("case", FC.XATTN_RANDOM[:4], ids=FC.ids_of(FC.XATTN_RANDOM[:4]))
def test_formula_is_the_autograd_of_the_forward(case):
    """FC.xattn_formula (the kernels' backward formulas) in fp64 agrees with fp64 autograd: the exact classes check the right thing."""
    q, k, v, do = FC.xattn_inputs(case)
    for a, b in zip(FC.xattn_formula(q, k, v, do, case["heads"], FC.xattn_post_scale(case), torch.float64),
                    FC.xattn_autograd(q, k, v, do, case["heads"], FC.xattn_post_scale(case))):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


def test_integer_sums_are_exact():
    """The integer-valued gradients of the gather and embedding-backward cases: an fp32 sum in ANY order equals the fp64 sum (every
    partial sum is an integer below 2^24)."""
    gen = torch.Generator().manual_seed(0)
    for lo, hi, n in ((-3, 3, 885), (-8, 8, 64)):
        x = FC.small_ints(gen, n, 8, lo=lo, hi=hi)
        assert float(x.abs().sum(0).max()) < 2 ** 24
        ref = x.double().sum(0)
        for perm in (torch.arange(n), torch.arange(n).flip(0), torch.randperm(n, generator=gen)):
            acc = torch.zeros(8)
            for r in perm.tolist():
                acc = acc + x[r]
            assert torch.equal(acc.double(), ref)


def test_references_on_small_examples():
    """The references themselves on examples small enough to check by hand."""
    case = dict(B=1, t_in=3, t_out=4, row_elems=4)
    idx = torch.tensor([[-5, 1, 7, 1]])
    cl = FC.gather_clamped(case, idx)
    assert cl.tolist() == [[0, 1, 2, 1]]
    y = torch.arange(16.).view(1, 4, 4)
    assert torch.equal(FC.gather_bwd_ref(y, cl, 3)[0], torch.stack([y[0, 0], y[0, 1] + y[0, 3], y[0, 2]]).double())
    assert FC.gather_clamped(dict(B=1, t_in=1, t_out=3), None).tolist() == [[0, 0, 0]]
    # copy_rows: rows 0, 1 in group 0 and row 2 in group 1
    idx, span = FC.copy_dst_index(dict(rows=3, D=4, group=2, gstride=16, off=4))
    assert idx[:, 0].tolist() == [4, 8, 20] and span == 32
    # NDCG: ties resolved earlier index first, the empty item, the refusals
    s, g = torch.tensor([1.0, 1.0, 2.0]), torch.tensor([0, 1, 0])
    want = (1.0 / torch.log2(torch.tensor(4.0))) / (1.0 / torch.log2(torch.tensor(2.0)))
    assert abs(float(FC.ndcg_ref(s, g, (10,))[0]) - float(want)) < 1e-7           # label 1 ends up third
    assert FC.ndcg_ref(torch.zeros(0), torch.zeros(0, dtype=torch.int64), (1, 5)).tolist() == [1.0, 1.0]
    assert bool(torch.isnan(FC.ndcg_ref(torch.zeros(65), torch.zeros(65, dtype=torch.int64), (1,))).all())
    assert bool(torch.isnan(FC.ndcg_ref(torch.zeros(2), torch.tensor([0, 63]), (1,))).all())
    assert bool(torch.isfinite(FC.ndcg_ref(torch.zeros(2), torch.tensor([0, 62]), (1,))).all())


def test_ndcg_reference_agrees_with_the_host_meter():
    from lr2ppo_amd.ndcg import AverageNDCGMeter
    meter = AverageNDCGMeter(FC.NDCG_KS)
    n = 0
    for case in FC.NDCG:
        for s, g, kind in FC.ndcg_items(case):
            if FC.ndcg_meter_applies(kind, s.numel()):
                assert float((FC.ndcg_ref(s, g, FC.NDCG_KS) - meter.return_ndcg_at_k_from_scores(s, g)).abs().max()) <= 1e-6
                n += 1
    assert n > 200


def test_case_tables_hold_what_the_suite_promises():
    """The sizes at which each kernel takes another path are in the tables."""
    assert {c["row_elems"] for c in FC.GATHER} == {4, 1024, 65536, 65540} and {c["B"] for c in FC.GATHER} == {1, 3}
    assert {c["form"] for c in FC.GATHER} == {"tight", "shared", "offset"} and {c["index"] for c in FC.GATHER} == {"repeat", "same", "none", "oob"}
    assert {c["group"] for c in FC.COPY} == {1, 2, 3}
    assert all((c["group"] == 1 or c["rows"] % c["group"]) and c["gstride"] > c["group"] * c["D"] + c["off"] > c["group"] * c["D"] for c in FC.COPY)
    assert any(c["rows"] * c["D"] // 4 > FC.GRID_CAP for c in FC.COPY)
    assert {c["rows"] * c["D"] // 4 for c in FC.TEXT_EMBED} >= {1, 255, 256, 257} and any(c["rows"] * c["D"] // 4 > FC.GRID_CAP for c in FC.TEXT_EMBED)
    assert all(256 % c["L"] for c in FC.TEXT_EMBED if c["L"] > 1) and {c["D"] for c in FC.TEXT_EMBED} == {4, 36, 768}
    assert {FC.text_embed_err(c) for c in FC.TEXT_EMBED} == {0, 1, 2, 3}
    assert {c["bounds"][-1] for c in FC.EMBED_BWD_WORD} >= {1, 255, 256, 257, 512, 513}
    assert {c["rows"] for c in FC.EMBED_BWD_SEG} == {1, 63, 64, 65, 129} and {c["n_seg"] for c in FC.EMBED_BWD_SEG} == {1, 2, 3, 4}
    strip = [c for c in FC.PATCHIFY_PLANES if c["kernel"] == "strip" and c["C"] == 3]
    assert {c["W"] // 16 * 3 * 16 for c in strip} >= {48, 240, 288, 672}
    assert all(FC.patchify_kernel(c) == c["kernel"] for c in FC.PATCHIFY_PLANES) and {c["kernel"] for c in FC.PATCHIFY_PLANES} == {"strip", "vec4", "vec2"}
    assert {c["ps"] for c in FC.PATCHIFY_PLANES} == {4, 6, 8, 14, 16} and {c["C"] for c in FC.PATCHIFY_PLANES if c["src"] == "u8n"} == {1, 2, 3}
    assert any(c["B"] * (c["H"] // c["ps"]) * (c["W"] // c["ps"]) * FC.patchify_ld(c) // 4 > FC.GRID_CAP for c in FC.PATCHIFY_PLANES if c["kernel"] == "vec4")
    for c in FC.PATCHIFY_PLANES:
        if c["all256"]:
            img, _ = FC.patchify_image(c)
            assert all(img[0, ch].unique().numel() == 256 for ch in range(c["C"]))
    assert any(c["B"] * (c["P"] + 1) * c["D"] // 4 > FC.GRID_CAP for c in FC.VIT_ASSEMBLE)
    sh = FC.XATTN_SHAPES
    assert {c["Lk"] for c in sh} >= {1, 2, 15, 16} and {c["Lq"] for c in sh} == {1, 2, 3, 255, 256} and {c["hd"] for c in sh} == {4, 64, 92, 96}
    assert {c["heads"] for c in sh} == {1, 3} and {c["batch"] for c in sh} == {1, 2}
    assert {(c["Lq"], c["Lk"]) for c in sh} >= {(1, 1), (1, 16), (256, 1), (256, 16), (3, 15)}
    assert {c["Lk"] for c in FC.XATTN_UNIFORM} == {1, 2, 4, 8, 16} and FC.XATTN_LARGE and len(FC.XATTN_PLANES) >= 4
    assert {c["n_items"] for c in FC.NDCG} == {1, 63, 64, 65, 129}
    kinds = {k for c in FC.NDCG for k in c["special"].values()}
    assert kinds == {"t0", "t65", "label62", "label63", "label-1", "equal", "ties"}
    sizes = {s.numel() for c in FC.NDCG for s, _, _ in FC.ndcg_items(c)}
    assert sizes >= {0, 1, 63, 64, 65}
    for name, table in FC.TABLES.items():
        ids = FC.ids_of(table)
        assert len(set(ids)) == len(ids), name


def test_every_case_table_is_consumed_by_a_gpu_test():
    """Each table of frontend_cases.TABLES is, as a whole, the argument list of a parametrised test of test_frontend_edges_gpu.py, so every
    entry is run."""
    mod = importlib.import_module("test_frontend_edges_gpu")
    used = set()
    for name in dir(mod):
        fn = getattr(mod, name)
        if name.startswith("test_") and callable(fn):
            for m in getattr(fn, "pytestmark", []):
                if m.name == "parametrize":
                    vals = m.kwargs.get("argvalues", m.args[1] if len(m.args) > 1 else None)
                    used |= {n for n, t in FC.TABLES.items() if vals is t}
    assert used == set(FC.TABLES), sorted(set(FC.TABLES) - used)
    listed = {id(t) for t in FC.TABLES.values()}
    stray = [n for n in dir(FC) if n.isupper() and isinstance(getattr(FC, n), list) and getattr(FC, n) and isinstance(getattr(FC, n)[0], dict)
             and id(getattr(FC, n)) not in listed and n != "XATTN_SHAPES"]
    assert not stray, stray
