"""The parts of the reduction-kernel tests that need no GPU.

1. Argument contracts of the reduction entry points of csrc/norm.hip and csrc/misc.hip that tests/test_host_cpu.py and
   tests/test_pointwise_cpu.py do not already assert: every call below is rejected before anything is launched (a launch on a box
   without a GPU would come back as LR2_ERR_LAUNCH, not as the code asserted), so nothing is dereferenced.  -1 = LR2_ERR_ARG (NULL, a
   count or mode out of range), -2 = LR2_ERR_SHAPE (a size the kernel's vector width / register budget / workgroup cannot take).
2. The properties tests/test_reductions_gpu.py relies on, checked where they are decided -- on the CPU, in fp64: the local PPO
   reference is O.ppo_update_math at the reference's constants, every committed seed keeps every item out of the guard band and
   takes every branch, the two derived LayerNorm gates hold for a plain fp32 evaluation, and the small-variance case can tell the
   mode-1 backward with its (1 - eps rstd) factor from the one without.
"""
import pytest
import torch

from oracle import lr2ppo_oracle as O

import test_reductions_gpu as G


@pytest.fixture(scope="module")
def lib():
    from lr2ppo_amd import _native as native
    return native.lib()


A = 64          # a stand-in device address with every alignment the kernels need (nothing is dereferenced: every call fails)
ARG, SHAPE = -1, -2


# ------------------------------------------------------------------------------------------------- argument contracts
def test_layernorm_fwd_contract(lib):
    def call(x=A, gamma=A, beta=A, out=A, out_hi=None, rows=4, D=64, mode=0):
        return lib.lr2_layernorm_fwd(x, gamma, beta, out, out_hi, 0, A, A, rows, D, 1e-5, mode, 0, 0, None)
    for D in (6, 66, 1022):                     # D % 4
        assert call(D=D) == SHAPE
    for D in (0, 2, -4):                        # D < 4
        assert call(D=D) == SHAPE
    for D in (1028, 2048):                      # D > 1024: four float4 per lane
        assert call(D=D) == SHAPE
    for rows in (0, -1):
        assert call(rows=rows) == ARG
    assert call(out=None, out_hi=None) == ARG   # neither output
    for k in ("x", "gamma", "beta"):
        assert call(**{k: None}) == ARG


def test_layernorm_bwd_contract(lib):
    def call(dy=A, x=A, gamma=A, mean=A, rstd=A, dx=A, dxm=None, partials=A, nblocks=8, rows=4, D=64, mode=0):
        return lib.lr2_layernorm_bwd(dy, 0, 0, x, gamma, mean, rstd, None, dx, dxm, 0, 0.0, 0, 0, None, partials, nblocks, rows, D,
                                     mode, 1e-5, None)
    for D in (6, 66, 1022, 0, 2, -4, 1028, 2048):
        assert call(D=D) == SHAPE
    for rows in (0, -1):
        assert call(rows=rows) == ARG
    for nblocks in (0, -1):
        assert call(nblocks=nblocks) == ARG
    for mode in (2, -1):
        assert call(mode=mode) == ARG
    assert call(dx=None, dxm=None) == ARG       # neither output
    for k in ("dy", "x", "gamma", "mean", "rstd", "partials"):
        assert call(**{k: None}) == ARG


def test_colsum_contract(lib):
    def call(x=A, is_planes=0, rows=8, cols=64, ld=64, partials=A, nblocks=4, out=A):
        return lib.lr2_colsum(x, is_planes, 1024, rows, cols, ld, partials, nblocks, out, None)
    for is_planes in (0, 1, 2):
        assert call(is_planes=is_planes, cols=6, ld=8) == SHAPE         # cols % 4
        assert call(is_planes=is_planes, cols=62, ld=64) == SHAPE
        assert call(is_planes=is_planes, cols=64, ld=66) == SHAPE       # ld % 4
        assert call(is_planes=is_planes, cols=64, ld=60) == SHAPE       # a row pitch below the row length
        assert call(is_planes=is_planes, cols=64, ld=0) == SHAPE
        assert call(is_planes=is_planes, cols=64, ld=-64) == SHAPE
        for k in ("rows", "cols", "nblocks"):
            for v in (0, -4):
                assert call(is_planes=is_planes, **{k: v}) == ARG
    for k in ("x", "partials", "out"):
        assert call(**{k: None}) == ARG


def test_colsum_partials_finish_contract(lib):
    def call(partials=A, nblocks=4, cols=64, ld=64, out=A, accumulate=0):
        return lib.lr2_colsum_partials_finish(partials, nblocks, cols, ld, out, accumulate, None)
    for accumulate in (0, 1):
        for v in (0, -1):
            assert call(nblocks=v, accumulate=accumulate) == ARG
            assert call(cols=v, accumulate=accumulate) == ARG
        for ld in (63, 0, -64):                 # a row pitch below the row length; a negative one would read in front of the buffer
            assert call(ld=ld, accumulate=accumulate) == SHAPE
    assert call(partials=None) == ARG
    assert call(out=None) == ARG


def test_ppo_loss_contract(lib):
    def call(B=8, T=2, rank_len=2, ns_len=4, scalars=A, per_item=A, dscores=A, dvalue=A, stats_out=None, global_stats=None, world=1,
             **ins):
        p = {k: ins.get(k, A) for k in ("scores", "old_scores", "rewards", "old_value", "value", "next_state")}
        return lib.lr2_ppo_loss(p["scores"], p["old_scores"], p["rewards"], p["old_value"], p["value"], p["next_state"], ns_len,
                                rank_len, B, T, 0.001, 0.001, 0.5, 0.01, -0.1, scalars, per_item, dscores, dvalue, stats_out,
                                global_stats, world, None)
    for B in (0, 1025, -1):
        assert call(B=B) == SHAPE
    for T in (0, 9):
        assert call(T=T, rank_len=1) == SHAPE
    for T in (1, 2, 8):
        assert call(T=T, rank_len=0, ns_len=10) == SHAPE
        assert call(T=T, rank_len=T + 1, ns_len=10) == SHAPE
    assert call(T=4, rank_len=3, ns_len=2) == SHAPE                     # ns_len < rank_len
    assert call(T=2, rank_len=2, ns_len=1) == SHAPE
    for world in (0, -2):
        assert call(global_stats=A, world=world) == ARG
    for k in ("scalars", "per_item", "dscores", "dvalue"):              # pass 2 / single-rank form: every output is needed
        assert call(**{k: None}) == ARG
        assert call(global_stats=A, world=2, **{k: None}) == ARG
    for k in ("scores", "old_scores", "rewards", "old_value", "value", "next_state"):
        assert call(**{k: None}) == ARG
        assert call(stats_out=A, scalars=None, per_item=None, dscores=None, dvalue=None, **{k: None}) == ARG
    # pass 1 needs no other output -- but still a legal shape
    assert call(stats_out=A, scalars=None, per_item=None, dscores=None, dvalue=None, B=1025) == SHAPE


def test_smooth_l1_contract(lib):
    for beta in (0.0, -0.3):
        assert lib.lr2_smooth_l1(A, A, 8, beta, A, A, None) == ARG
        assert lib.lr2_smooth_l1(A, A, 8, beta, A, None, None) == ARG
    for n in (0, -1):
        assert lib.lr2_smooth_l1(A, A, n, 0.3, A, A, None) == ARG
    assert lib.lr2_smooth_l1(None, A, 8, 0.3, A, A, None) == ARG
    assert lib.lr2_smooth_l1(A, None, 8, 0.3, A, A, None) == ARG
    assert lib.lr2_smooth_l1(A, A, 8, 0.3, None, A, None) == ARG


# ------------------------------------------------------------------------- what the GPU tests rely on, decided on the CPU
@pytest.mark.parametrize("B,T,seed", [(65, 2, 2), (1024, 2, 2), (130, 8, 1), (7, 4, 3)])
def test_local_ppo_reference_is_the_oracle_at_the_reference_constants(B, T, seed):
    """rank_len = 2, margin = 0.01, adv_eps = -0.1 are what finetune/ppo.py hard-codes and O.ppo_update_math mirrors"""
    c = G.ppo_inputs(B, T, seed)
    a = [c[k].double() for k in ("scores", "value", "old", "rewards", "old_value")]
    for kl_w, ent_w in ((0.001, 0.001), (0.0, 0.001), (0.001, 0.0)):
        loss, vloss, ex = G.ppo_ref(*a, c["nxt"], kl_w, ent_w, 0.5, rank_len=2, margin=0.01, adv_eps=-0.1)
        oloss, ovloss, oex = O.ppo_update_math(a[0], a[1], a[2], a[3], a[4], c["nxt"], kl_w, ent_w, 0.5)
        assert torch.equal(loss, oloss) and torch.equal(vloss, ovloss)
        assert torch.equal(ex["order"], oex["order"]) and torch.equal(ex["rank_loss"], oex["rank_loss"])
        for k in ("kl", "entropy", "rewards", "advantages"):
            assert torch.equal(ex[k], oex[k].double()), k
        # the extras the guard band looks at are the quantities the losses were built from
        assert ex["count"] == torch.sign(torch.relu(ex["hgap"])).sum()
        if ex["count"] > 0:
            assert torch.allclose(ex["rank_loss"], torch.relu(ex["hgap"]).sum() / ex["count"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("B,T,rank_len,seed", G.PPO_CASES, ids=[f"B{B}-T{T}-rank_len{rl}" for B, T, rl, _ in G.PPO_CASES])
def test_ppo_seeds_keep_every_item_out_of_the_guard_band(B, T, rank_len, seed):
    ref = G.ppo_reference(G.ppo_inputs(B, T, seed), rank_len)
    assert G.ppo_guard_violations(ref) == 0
    if B >= 63:
        G.ppo_branch_coverage(ref, hinges=rank_len > 1)
    assert torch.isfinite(ref["ds"]).all() and torch.isfinite(ref["dv"]).all()


def test_ppo_special_case_seeds():
    c = G.ppo_inputs(130, 3, G.PPO_WEIGHT_SEED)
    for kl_w, ent_w in G.PPO_WEIGHT_CASES:
        ref = G.ppo_reference(c, 3, kl_w=kl_w, ent_w=ent_w)
        assert G.ppo_guard_violations(ref) == 0
        G.ppo_branch_coverage(ref)
    for c, rank_len in ((G.ppo_inputs(65, 3, G.PPO_NOHINGE_SEED), 1), (G.ppo_separated_inputs(65, 3, G.PPO_NOHINGE_SEED), 3)):
        for ent_w in (0.001, 0.0):
            ref = G.ppo_reference(c, rank_len, ent_w=ent_w)
            assert G.ppo_guard_violations(ref) == 0
            assert ref["count"] == 0 and ref["rank_loss"] == 0
            if ent_w == 0.0:
                assert not ref["ds"].any(), "without a positive hinge and without the entropy term the score gradient is 0"
        if rank_len == 3:                                   # both target orders occur, each one apart
            assert (ref["advantages"] >= -0.1).any() and (ref["advantages"] < -0.1).any()
            assert (ref["hgap"] < -0.7).all()
    ref = G.ppo_reference(G.ppo_inputs(130, 2, G.PPO_TWO_PASS_SEED), 2)
    assert G.ppo_guard_violations(ref) == 0
    G.ppo_branch_coverage(ref)
    c = G.ppo_peaked_inputs(65, 3, G.PPO_PEAKED_SEED)
    pm = G.ppo_min_prob(c)
    assert (pm < G.PROB_FLOOR).sum() >= 5 and (pm > G.PROB_FLOOR).sum() >= 5
    assert not ((pm > 0.5 * G.PROB_FLOOR) & (pm < 2 * G.PROB_FLOOR)).any()
    assert G.ppo_guard_violations(G.ppo_reference(c, 3)) == 0


def test_two_pass_identity_holds_for_the_reference():
    """world x the slice of the global-batch gradient == the gradient of (global R, global mean |A|) x this half's terms: the
    identity the GPU test asserts of the kernel, first for the fp64 reference itself"""
    c = G.ppo_inputs(130, 2, G.PPO_TWO_PASS_SEED)
    ref = G.ppo_reference(c, 2)
    for sl in (slice(0, 65), slice(65, 130)):
        half = G.ppo_reference(c, 2, sl=sl)
        assert torch.allclose(2.0 * ref["dv"][sl], half["dv"], rtol=1e-12, atol=0)       # the value loss is a plain mean
        assert torch.equal(ref["kl"][sl], half["kl"]) and torch.equal(ref["advantages"][sl], half["advantages"])


@pytest.mark.parametrize("beta", [0.3, 1.0])
@pytest.mark.parametrize("n", [1, 64, 1023, 1024, 1025, 5000])
def test_smooth_l1_seeds_keep_every_element_off_beta(n, beta):
    c = G.smooth_l1_case(n, beta)
    assert not ((c["d"] - beta).abs() <= G.GUARD).any()
    if n >= 64:
        assert (c["d"] < beta).any() and (c["d"] > beta).any()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("D", [768, 100])
def test_offset_rows_gate_holds_for_fp32_torch(D, mode):
    c = G.offset_rows_case(D, mode)
    G._within(G.ln_ref(c["x"], c["gam"], c["bet"], mode), c["ref"], c["bound"], "fp32 torch")
    # the derived part is k <= 12 ulp of the mean (ulp32 of a value in [4, 16) is at most 2^-20) times rstd |gamma|, nothing more
    extra = c["bound"] - (1e-5 + 1e-5 * c["ref"].abs())
    assert (c["mean"] > 4).all() and (c["mean"] < 16).all()
    assert (extra <= 12 * 2.0 ** -20 * c["rstd"].max() * c["gam"].double().abs()[None, :] + 1e-18).all()


@pytest.mark.parametrize("D", [64, 768])
def test_small_variance_case_sees_the_eps_factor(D):
    c = G.small_variance_case(D)
    assert ((c["eps_rstd"] > 0.03) & (c["eps_rstd"] < 0.07)).all()
    row_max = c["dx"].abs().amax(-1, keepdim=True)
    right = G.tp_bwd_dx_analytic(c["x"].double(), c["gam"].double(), c["dy"].double(), G.SMALL_VAR_EPS)
    assert ((right - c["dx"]).abs() <= 1e-9 * row_max).all()
    assert ((c["wrong"] - c["dx"]).abs().amax(-1, keepdim=True) > 100 * G.SMALL_VAR_GATE * row_max).all()
    # and at the product's scale (std about 1) the two agree to 1e-6 of the row: no other test can tell them apart
    g = G._gen(1)
    x, gam, dy = G._rand(g, 9, D).double(), G._rand(g, D).double(), G._rand(g, 9, D).double()
    a, b = G.tp_bwd_dx_analytic(x, gam, dy, 1e-6), G.tp_bwd_dx_analytic(x, gam, dy, 1e-6, with_factor=False)
    assert ((a - b).abs() <= 2e-6 * a.abs().amax(-1, keepdim=True)).all()
