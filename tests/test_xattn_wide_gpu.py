"""The wide XiT cross-attention pair (csrc/attn_wide.hip, 17 to 64 image tokens) on a real MI355X, with the conventions, input classes,
references and tolerances of test_frontend_edges_gpu.py (canaried destinations, exact one-hot and uniform classes, fp64 autograd for
the random class at the tolerances of test_xattn_random, 4 x the fp32 torch formula's own error for the large-score class, planes
outputs bit-equal to split_planes of the fp32 outputs) at the shapes of tests/xattn_wide_cases.py, which test_xattn_wide_cpu.py proves
exact.  The table's three shapes with Lk <= 16 run the wide form through wide=True and meet the same bounds (bit equality with the
16-key kernels is not asked: the backward adds in another order).  Every case with Lk >= 17 fails without the wide kernels: the
16-key entry points answer LR2_ERR_SHAPE."""
import pytest
import torch

import frontend_cases as FC
import xattn_wide_cases as WC
from test_frontend_edges_gpu import PAT32, XROWS, PlanesDest, check32, check_close, dest32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(dev):
    from lr2ppo_amd import ops as _ops
    return _ops


def P(table):
    return dict(argnames="case", argvalues=table, ids=FC.ids_of(table))


def run_wide(ops, dev, case, q, k, v, do, planes=False):
    """-> (O, dQ, dK, dV) destinations: canaried fp32 buffers, or PlanesDest objects.  Lk >= 17 goes through the plain dispatch of
    ops.xattn_fwd / xattn_bwd, Lk <= 16 is forced onto the wide pair; either way the wide launch counters must move by one each."""
    batch, heads, Lq, Lk, hd = (case[n] for n in ("batch", "heads", "Lq", "Lk", "hd"))
    E = heads * hd
    kw = dict(batch=batch, heads=heads, Lq=Lq, Lk=Lk, head_dim=hd, post_scale=FC.xattn_post_scale(case))
    if not WC.is_wide_only(case):
        kw["wide"] = True
    qd, kd, vd, dod = (t.to(dev).view(-1, E) for t in (q, k, v, do))
    before = ops.xattn_wide_launch_counts()
    if planes:            # K-sized outputs get one canary row more, so that q_lo_off != kv_lo_off even when Lq == Lk
        o, dq = PlanesDest(ops, batch * Lq, E, dev), PlanesDest(ops, batch * Lq, E, dev)
        dk, dv = PlanesDest(ops, batch * Lk, E, dev, xrows=XROWS + 1), PlanesDest(ops, batch * Lk, E, dev, xrows=XROWS + 1)
        assert dq.planes.lo_off != dk.planes.lo_off
        ops.xattn_fwd(qd, kd, vd, o.planes, **kw)
        ops.xattn_bwd(qd, kd, vd, dod, dq.planes, dk.planes, dv.planes, **kw)
    else:
        o, dq = dest32(batch * Lq * E, dev, XROWS * E), dest32(batch * Lq * E, dev, XROWS * E)
        dk, dv = dest32(batch * Lk * E, dev, XROWS * E), dest32(batch * Lk * E, dev, XROWS * E)
        ops.xattn_fwd(qd, kd, vd, o[:batch * Lq * E].view(-1, E), **kw)
        ops.xattn_bwd(qd, kd, vd, dod, dq[:batch * Lq * E].view(-1, E), dk[:batch * Lk * E].view(-1, E), dv[:batch * Lk * E].view(-1, E), **kw)
    after = ops.xattn_wide_launch_counts()
    assert after == (before[0] + 1, before[1] + 1), "the wide kernels did not run"
    return o, dq, dk, dv


@pytest.mark.parametrize(**P(WC.XATTN_ONEHOT))
def test_wide_one_hot_is_exact(ops, dev, case):
    """Each query's best key leads by >= 200 (scores up to 7.9e5, exact integers): O = c V[winner], dQ = 0, dK = 0, dV[j] = c sum of dO
    over the queries that chose j, with torch.equal; winners in every key block, nothing written past the destinations."""
    q, k, v, do = WC.inputs(case)
    got = run_wide(ops, dev, case, q, k, v, do)
    for name, g, r in zip(("O", "dQ", "dK", "dV"), got, FC.xattn_onehot_expected(case, v, do, FC.xattn_post_scale(case))):
        check32(g, r, f"one-hot {name}")


@pytest.mark.parametrize(**P(WC.XATTN_UNIFORM))
def test_wide_uniform_is_exact(ops, dev, case):
    """Q = 0 and Lk a power of two (32 and 64): p = 1 / Lk exactly; the fp64 formula, compared with torch.equal."""
    q, k, v, do = WC.inputs(case)
    got = run_wide(ops, dev, case, q, k, v, do)
    ref = FC.xattn_formula(q, k, v, do, case["heads"], FC.xattn_post_scale(case), torch.float64)
    assert not bool(ref[2].any()) and (case["Lk"] == 1 or bool(ref[1].any()))
    for name, g, r in zip(("O", "dQ", "dK", "dV"), got, ref):
        check32(g, r, f"uniform {name}")


@pytest.mark.parametrize(**P(WC.XATTN_RANDOM))
def test_wide_random(ops, dev, case):
    """Against fp64 autograd at the tolerances of test_xattn_random (the fp32 torch formula uses under half of them on these shapes:
    test_xattn_wide_cpu.py)."""
    q, k, v, do = WC.inputs(case)
    o, dq, dk, dv = run_wide(ops, dev, case, q, k, v, do)
    ro, rq, rk, rv = FC.xattn_autograd(q, k, v, do, case["heads"], FC.xattn_post_scale(case))
    check_close(o, ro, 1e-6, 1e-5, "xattn fwd")
    check_close(dq, rq, 1e-6, 1e-4, "dq")
    check_close(dk, rk, 1e-5, 1e-4, "dk")
    check_close(dv, rv, 1e-5, 1e-4, "dv")


@pytest.mark.parametrize(**P(WC.XATTN_LARGE))
def test_wide_large_scores(ops, dev, case):
    """Unit inputs without a pre-scale at head_dim 92 / 96: the bound is 4 x the error of the same formulas in fp32 torch on the CPU,
    computed and printed here -- the rule of test_xattn_large_scores and its reason (the kernel multiplies by log2 e and uses the
    hardware exp2: two more roundings of an argument of this size)."""
    q, k, v, do = WC.inputs(case)
    post = FC.xattn_post_scale(case)
    ref = FC.xattn_formula(q, k, v, do, case["heads"], post, torch.float64)
    f32 = FC.xattn_formula(q, k, v, do, case["heads"], post, torch.float32)
    got = run_wide(ops, dev, case, q, k, v, do)
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


@pytest.mark.parametrize(**P(WC.XATTN_PLANES))
def test_wide_planes_outputs(ops, dev, case):
    """Planes outputs of the forward and the backward equal split_planes of the fp32 outputs of the same calls, bit for bit, with
    canaries behind the Q-sized and the K-sized outputs and in the gap between the planes, and q_lo_off != kv_lo_off."""
    q, k, v, do = WC.inputs(case)
    dense = run_wide(ops, dev, case, q, k, v, do)
    planes = run_wide(ops, dev, case, q, k, v, do, planes=True)
    for name, d, p in zip(("O", "dQ", "dK", "dV"), dense, planes):
        assert bool((d[p.n:].view(torch.int32) == PAT32).all()) and not bool(torch.isnan(d[:p.n]).any())
        p.check(ops, d[:p.n], f"planes {name}")


@pytest.mark.parametrize(**P(WC.XATTN_DETERMINISM))
def test_wide_is_deterministic(ops, dev, case):
    """No atomics, every sum in a fixed order: the forward and the backward called twice give the same bits."""
    q, k, v, do = WC.inputs(case)
    a = run_wide(ops, dev, case, q, k, v, do)
    b = run_wide(ops, dev, case, q, k, v, do)
    for name, x, y in zip(("O", "dQ", "dK", "dV"), a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), name


def test_dispatch_by_key_count(ops, dev):
    """ops.xattn_fwd / xattn_bwd at Lk = 16 run the 16-key kernels (the wide counters stay), at Lk = 17 the wide ones; Lk = 65 is a
    ValueError that names the limit, and launches nothing."""
    heads, Lq, hd = 2, 5, 8
    E = heads * hd
    gen = torch.Generator().manual_seed(3)
    for Lk, moves in ((16, 0), (17, 1)):
        q, do = torch.randn(Lq, E, generator=gen).to(dev), torch.randn(Lq, E, generator=gen).to(dev)
        k, v = torch.randn(Lk, E, generator=gen).to(dev), torch.randn(Lk, E, generator=gen).to(dev)
        o, dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(k), torch.empty_like(k)
        kw = dict(batch=1, heads=heads, Lq=Lq, Lk=Lk, head_dim=hd, post_scale=0.25)
        before = ops.xattn_wide_launch_counts()
        ops.xattn_fwd(q, k, v, o, **kw)
        ops.xattn_bwd(q, k, v, do, dq, dk, dv, **kw)
        assert ops.xattn_wide_launch_counts() == (before[0] + moves, before[1] + moves), Lk
        ref = FC.xattn_autograd(q.cpu()[None], k.cpu()[None], v.cpu()[None], do.cpu()[None], heads, 0.25)
        for got, r in zip((o, dq, dk, dv), ref):
            assert float((got.cpu().double() - r[0]).abs().max()) <= 1e-5 * max(1.0, float(r.abs().max()))
    before = ops.xattn_wide_launch_counts()
    t = torch.zeros(65, E, device=dev)
    kw = dict(batch=1, heads=heads, Lq=Lq, Lk=65, head_dim=hd, post_scale=0.25)
    with pytest.raises(ValueError, match="64"):
        ops.xattn_fwd(t, t, t, t, **kw)
    with pytest.raises(ValueError, match="64"):
        ops.xattn_bwd(t, t, t, t, t, t, t, **kw)
    assert ops.xattn_wide_launch_counts() == before
