"""The CPU half of the wide XiT cross-attention suite (tests/xattn_wide_cases.py, test_xattn_wide_gpu.py): the argument contract of
lr2_xattn_fwd_wide / lr2_xattn_bwd_wide through the C ABI (every refusal returns before anything is launched, so nothing is
dereferenced and the launch counters stay), the proof that the exact input classes of tests/frontend_cases.py stay exact at 17 to 64
keys, the shape coverage of the table, and the limit in words of ops and of the head modules."""
import argparse
import ctypes

import pytest
import torch

import frontend_cases as FC
import xattn_wide_cases as WC

A = 64          # a stand-in device address with every alignment the kernels need (nothing is dereferenced: every call fails)
OFF16 = (4, 8, 12)      # byte offsets that break 16-byte alignment
OFF8 = (2, 4, 6)        # ... 8-byte alignment


@pytest.fixture(scope="module")
def lib():
    from lr2ppo_amd import _native as native
    return native.lib()


def _counts(lib):
    c = (ctypes.c_uint64 * 2)()
    assert lib.lr2_xattn_wide_launch_counts(c) == 0
    return int(c[0]), int(c[1])


# ---- argument contract --------------------------------------------------------------------------------------------------------------
SHAPES_REFUSED = ((0, 1, 4), (257, 1, 4), (1, 0, 4), (1, 65, 4), (1, 1, 0), (1, 1, 100), (1, 1, 6))      # (Lq, Lk, head_dim)


def test_xattn_wide_contract(lib):
    assert lib.lr2_xattn_wide_launch_counts(None) == -1
    before = _counts(lib)
    f = lib.lr2_xattn_fwd_wide       # (Q, K, V, O, o_planes, o_lo_off, batch, heads, Lq, Lk, head_dim, post_scale, stream)
    ok = [A, A, A, A]
    for i in range(4):
        p = list(ok)
        p[i] = None
        assert f(*p, 0, 0, 1, 1, 1, 1, 4, 1.0, None) == -1
    assert f(*ok, 0, 0, 0, 1, 1, 1, 4, 1.0, None) == -1
    assert f(*ok, 0, 0, 1, 0, 1, 1, 4, 1.0, None) == -1
    assert f(*ok, 0, 0, -1, 1, 1, 1, 4, 1.0, None) == -1
    for Lq, Lk, hd in SHAPES_REFUSED + ((1, 1, -4),):
        assert f(*ok, 0, 0, 1, 1, Lq, Lk, hd, 1.0, None) == -2, (Lq, Lk, hd)
    for off in OFF16:
        assert f(A + off, A, A, A, 0, 0, 1, 1, 1, 17, 4, 1.0, None) == -2     # float4 loads of Q
        assert f(A + off, A, A, A, 1, 8, 1, 1, 1, 17, 4, 1.0, None) == -2
        assert f(A, A, A, A + off, 0, 0, 1, 1, 1, 17, 4, 1.0, None) == -2     # float4 stores of an fp32 O
    for off in OFF8:
        assert f(A, A, A, A + off, 1, 8, 1, 1, 1, 17, 4, 1.0, None) == -2     # planes O: hi plane off 8 bytes
    for lo in (2, 6, 9):
        assert f(A, A, A, A, 1, lo, 1, 1, 1, 17, 4, 1.0, None) == -2          # ... lo plane off 8 bytes (9: odd)

    b = lib.lr2_xattn_bwd_wide       # (Q, K, V, dO, dQ, dK, dV, planes, q_lo_off, kv_lo_off, batch, heads, Lq, Lk, head_dim, post_scale, stream)
    ok = [A] * 7
    for i in range(7):
        p = list(ok)
        p[i] = None
        assert b(*p, 0, 0, 0, 1, 1, 1, 1, 4, 1.0, None) == -1
    assert b(*ok, 0, 0, 0, 0, 1, 1, 1, 4, 1.0, None) == -1
    assert b(*ok, 0, 0, 0, 1, 0, 1, 1, 4, 1.0, None) == -1
    assert b(*ok, 0, 0, 0, 1, -2, 1, 1, 4, 1.0, None) == -1
    for Lq, Lk, hd in SHAPES_REFUSED + ((1, 1, -4),):
        assert b(*ok, 0, 0, 0, 1, 1, Lq, Lk, hd, 1.0, None) == -2, (Lq, Lk, hd)
    for i in (0, 3, 4, 5, 6):                                                 # Q, dO: float4 loads; fp32 dQ, dK, dV: float4 stores
        for off in OFF16:
            p = list(ok)
            p[i] = A + off
            assert b(*p, 0, 0, 0, 1, 1, 1, 17, 4, 1.0, None) == -2
    for i in (4, 5, 6):                                                       # planes dQ, dK, dV: 4 x bf16 stores
        for off in OFF8:
            p = list(ok)
            p[i] = A + off
            assert b(*p, 1, 8, 8, 1, 1, 1, 17, 4, 1.0, None) == -2
    for qlo, kvlo in ((6, 8), (8, 6), (9, 8), (8, 2), (8, 9)):
        assert b(*ok, 1, qlo, kvlo, 1, 1, 1, 17, 4, 1.0, None) == -2
    assert _counts(lib) == before, "a refused call moved a launch counter"


def test_narrow_pair_still_refuses_17_keys(lib):
    """The 16-key entry points keep their range: the wide pair is an addition, not a widening."""
    assert lib.lr2_xattn_fwd(A, A, A, A, 0, 0, 1, 1, 1, 17, 4, 1.0, None) == -2
    assert lib.lr2_xattn_bwd(A, A, A, A, A, A, A, 0, 0, 0, 1, 1, 1, 17, 4, 1.0, None) == -2


def test_ops_names_the_limit_before_any_native_call(lib):
    """Lk = 65 is a ValueError that names 64, raised before the tensors are even looked at; the head modules say so at construction."""
    from lr2ppo_amd import ops
    from lr2ppo_amd.finetune import ppo
    before = _counts(lib)
    kw = dict(batch=1, heads=1, Lq=1, Lk=65, head_dim=4, post_scale=1.0)
    t = torch.zeros(65, 4)
    for wide in (False, True):
        with pytest.raises(ValueError, match="64"):
            ops.xattn_fwd(t, t, t, t, wide=wide, **kw)
        with pytest.raises(ValueError, match="64"):
            ops.xattn_bwd(t, t, t, t, t, t, t, wide=wide, **kw)
    assert _counts(lib) == before
    args = dict(mode="reg", labels_num=3, seq_length=196, visual_feat_dim=768)
    for cls in (ppo.Actor, ppo.Critic, ppo.Reward):
        with pytest.raises(ValueError, match="64"):
            cls(argparse.Namespace(max_imgs=65, **args), None)
        with pytest.raises(ValueError, match="64"):
            cls(argparse.Namespace(max_imgs=0, **args), None)


# ---- the table covers the kernel's seams --------------------------------------------------------------------------------------------
def test_table_covers_the_key_block_seams():
    lks = {c["Lk"] for c in WC.WIDE_SHAPES}
    assert {17, 31, 32, 33, 48, 64} <= lks and (63 in lks or 64 in lks)
    kb = WC.KEY_BLOCK
    for seam in range(kb, WC.MAX_LK + 1, kb):                                  # 16, 32, 48, 64: on, one short of and one past each
        for lk in (seam - 1, seam, seam + 1):
            if 1 <= lk <= WC.MAX_LK:
                assert lk in {c["Lk"] for c in WC.ALL_SHAPES}, lk
    assert {c["Lk"] for c in WC.NARROW_SHAPES} == {1, 15, 16}
    assert all(WC.is_wide_only(c) for c in WC.WIDE_SHAPES) and not any(WC.is_wide_only(c) for c in WC.NARROW_SHAPES)
    assert {c["Lq"] for c in WC.WIDE_SHAPES} >= {1, 2, 3, 196, 255, 256} and {c["hd"] for c in WC.WIDE_SHAPES} == {4, 64, 92, 96}
    for c in WC.ALL_SHAPES:
        assert 1 <= c["Lq"] <= 256 and 1 <= c["Lk"] <= WC.MAX_LK and c["hd"] % 4 == 0 and 4 <= c["hd"] <= 96
    assert {c["Lk"] for c in WC.XATTN_UNIFORM} >= {32, 64} and {c["hd"] for c in WC.XATTN_LARGE} == {92, 96}
    assert any(WC.is_wide_only(c) for c in WC.XATTN_PLANES) and all(WC.is_wide_only(c) for c in WC.XATTN_DETERMINISM)


def test_every_table_is_consumed_by_a_gpu_test():
    src = open(__file__.replace("test_xattn_wide_cpu.py", "test_xattn_wide_gpu.py")).read()
    for name in WC.TABLES:
        assert f"WC.{name}" in src, name


# ---- the exact classes are exact ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", WC.XATTN_ONEHOT, ids=FC.ids_of(WC.XATTN_ONEHOT))
def test_one_hot_class_is_exact(case):
    """As test_frontend_edges_cpu.py::test_one_hot_class_is_exact, at up to 64 keys: the winner leads by >= 200, the scores (up to 7.9e5)
    are integers below 2^24, and the kernels' formulas in fp32 torch equal the closed form bit for bit."""
    q, k, v, do = WC.inputs(case)
    heads, post = case["heads"], FC.xattn_post_scale(case)
    s = FC._heads(q.double(), heads) @ FC._heads(k.double(), heads).transpose(-1, -2)
    top = s.topk(min(2, case["Lk"]), dim=-1)
    assert torch.equal(top.indices[..., 0], FC.xattn_onehot_winner(case))
    if case["Lk"] > 1:
        assert float((top.values[..., 0] - top.values[..., 1]).min()) >= FC.ONEHOT_LEAD
        if case["Lq"] > 1:
            assert bool((top.indices[..., 0, 0] != top.indices[..., 1, 0]).all())
    assert float(s.abs().max()) < 2 ** 24 and post == 2.0 ** -4
    assert torch.equal(s, s.round())
    f32 = FC.xattn_formula(q, k, v, do, heads, post, torch.float32)
    f64 = FC.xattn_formula(q, k, v, do, heads, post, torch.float64)
    closed = FC.xattn_onehot_expected(case, v, do, post)
    for a, b, c in zip(f32, f64, closed):
        assert torch.equal(a.double(), c) and float((b - c).abs().max()) < 1e-80


@pytest.mark.parametrize("case", WC.XATTN_UNIFORM, ids=FC.ids_of(WC.XATTN_UNIFORM))
def test_uniform_class_is_exact(case):
    """Q = 0, Lk a power of two (32 and 64 among them): fp32 equals fp64; O = c / Lk sum V, dV = c / Lk sum dO, dK = 0."""
    q, k, v, do = WC.inputs(case)
    heads, post, Lk = case["heads"], FC.xattn_post_scale(case), case["Lk"]
    f32 = FC.xattn_formula(q, k, v, do, heads, post, torch.float32)
    f64 = FC.xattn_formula(q, k, v, do, heads, post, torch.float64)
    for a, b in zip(f32, f64):
        assert torch.equal(a.double(), b)
    vh, gh = FC._heads(v.double(), heads), FC._heads(do.double(), heads)
    assert torch.equal(FC._heads(f64[0], heads), (post / Lk) * vh.sum(2, keepdim=True).expand(-1, -1, case["Lq"], -1))
    assert torch.equal(FC._heads(f64[3], heads), (post / Lk) * gh.sum(2, keepdim=True).expand(-1, -1, Lk, -1))
    assert not bool(f64[2].any())


@pytest.mark.parametrize("case", WC.XATTN_RANDOM[:4], ids=FC.ids_of(WC.XATTN_RANDOM[:4]))
def test_formula_is_the_autograd_of_the_forward(case):
    q, k, v, do = WC.inputs(case)
    for a, b in zip(FC.xattn_formula(q, k, v, do, case["heads"], FC.xattn_post_scale(case), torch.float64),
                    FC.xattn_autograd(q, k, v, do, case["heads"], FC.xattn_post_scale(case))):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


def test_fp32_formula_uses_a_fraction_of_the_random_tolerances():
    """The tolerances of the random class (those of test_xattn_random) against an independent fp32 evaluation: the fp32 torch formula
    uses well under half of each on every shape of the table, so a correct fp32 kernel has room and a wrong one has none."""
    worst = 0.0
    for case in WC.XATTN_RANDOM:
        q, k, v, do = WC.inputs(case)
        ref = FC.xattn_autograd(q, k, v, do, case["heads"], FC.xattn_post_scale(case))
        f32 = FC.xattn_formula(q, k, v, do, case["heads"], FC.xattn_post_scale(case), torch.float32)
        for (atol, rtol), a, r in zip(((1e-6, 1e-5), (1e-6, 1e-4), (1e-5, 1e-4), (1e-5, 1e-4)), f32, ref):
            worst = max(worst, float(((a.double() - r).abs() / (atol + rtol * r.abs())).max()))
    print(f"  fp32 torch formula uses at most {worst:.2f} of the random-class tolerances")
    assert worst < 0.5
