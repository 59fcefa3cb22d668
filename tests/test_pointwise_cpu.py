"""Argument contracts of the pointwise entry points of csrc/misc.hip (the planes splits, the dropout family, the mode='cls' chain), the
parts that need no GPU: every call below is rejected before anything is launched, so nothing is dereferenced.  -1 = LR2_ERR_ARG (NULL,
a count or probability out of range), -2 = LR2_ERR_SHAPE (a size off the vector width, C outside [1, 8], a pointer off the alignment
the kernel's vector accesses need: 16 bytes for fp32 sources / destinations, 8 for a planes destination and its lo plane)."""
import pytest


@pytest.fixture(scope="module")
def lib():
    from lr2ppo_amd import _native as native
    return native.lib()


A = 64          # a stand-in device address with every alignment the kernels need (nothing is dereferenced: every call fails)


def test_split_planes_contract(lib):
    assert lib.lr2_split_planes(None, A, 4, 4, None) == -1
    assert lib.lr2_split_planes(A, None, 4, 4, None) == -1
    assert lib.lr2_split_planes(A, A, 4, 0, None) == -1
    assert lib.lr2_split_planes(A, A, 8, 6, None) == -2                   # n % 4
    assert lib.lr2_split_planes(A, A, 6, 4, None) == -2                   # lo plane off 8 bytes
    for off in (4, 8, 12):
        assert lib.lr2_split_planes(A + off, A, 4, 4, None) == -2         # fp32 source off 16 bytes
    for off in (2, 4, 6):
        assert lib.lr2_split_planes(A, A + off, 4, 4, None) == -2         # hi plane off 8 bytes


def test_split_planes_t_contract(lib):
    # the transposing kernel reads fp32 and writes bf16 one element at a time (through its LDS tile): NULL / empty shapes are the
    # whole contract, there is no vector access to misalign
    assert lib.lr2_split_planes_t(None, A, 16, 4, 4, None) == -1
    assert lib.lr2_split_planes_t(A, None, 16, 4, 4, None) == -1
    assert lib.lr2_split_planes_t(A, A, 16, 0, 4, None) == -1
    assert lib.lr2_split_planes_t(A, A, 16, 4, 0, None) == -1
    assert lib.lr2_split_planes_t(A, A, 16, -1, 4, None) == -1


def test_dropout_planes_contract(lib):
    assert lib.lr2_dropout_planes(None, A, 4, 4, 0.1, 0, 0, None) == -1
    assert lib.lr2_dropout_planes(A, None, 4, 4, 0.1, 0, 0, None) == -1
    assert lib.lr2_dropout_planes(A, A, 4, 0, 0.1, 0, 0, None) == -1
    assert lib.lr2_dropout_planes(A, A, 4, 4, -0.1, 0, 0, None) == -1
    assert lib.lr2_dropout_planes(A, A, 4, 4, 1.0, 0, 0, None) == -1
    assert lib.lr2_dropout_planes(A, A, 8, 6, 0.1, 0, 0, None) == -2
    assert lib.lr2_dropout_planes(A, A, 6, 4, 0.1, 0, 0, None) == -2
    for p in (0.0, 0.1):                                                  # p = 0 is lr2_split_planes: the same rule
        assert lib.lr2_dropout_planes(A + 4, A, 4, 4, p, 0, 0, None) == -2
        assert lib.lr2_dropout_planes(A + 8, A, 4, 4, p, 0, 0, None) == -2
        assert lib.lr2_dropout_planes(A, A + 2, 4, 4, p, 0, 0, None) == -2
        assert lib.lr2_dropout_planes(A, A + 4, 4, 4, p, 0, 0, None) == -2


def test_dropout_apply_contract(lib):
    assert lib.lr2_dropout_apply(None, A, 4, 0.1, 0, 0, None) == -1
    assert lib.lr2_dropout_apply(A, None, 4, 0.1, 0, 0, None) == -1
    assert lib.lr2_dropout_apply(A, A, 0, 0.1, 0, 0, None) == -1
    assert lib.lr2_dropout_apply(A, A, 4, 0.0, 0, 0, None) == -1
    assert lib.lr2_dropout_apply(A, A, 4, 1.0, 0, 0, None) == -1
    assert lib.lr2_dropout_apply(A, A, 6, 0.1, 0, 0, None) == -2
    for off in (4, 8, 12):
        assert lib.lr2_dropout_apply(A + off, A, 4, 0.1, 0, 0, None) == -2
        assert lib.lr2_dropout_apply(A, A + off, 4, 0.1, 0, 0, None) == -2
        assert lib.lr2_dropout_apply(A + off, A + off, 4, 0.1, 0, 0, None) == -2      # in place


def test_split_planes_multi_contract(lib):
    # the chunk table is device memory: only the table pointer and the chunk count can be judged on the host
    assert lib.lr2_split_planes_multi(None, 1, None) == -1
    assert lib.lr2_split_planes_multi(A, 0, None) == -1
    assert lib.lr2_split_planes_multi(A, -3, None) == -1


def test_cls_head_contract(lib):
    assert lib.lr2_cls_head_fwd(None, A, A, A, 1, 4, 3, None) == -1
    assert lib.lr2_cls_head_fwd(A, None, A, A, 1, 4, 3, None) == -1
    assert lib.lr2_cls_head_fwd(A, A, None, A, 1, 4, 3, None) == -1
    assert lib.lr2_cls_head_fwd(A, A, A, None, 1, 4, 3, None) == -1
    assert lib.lr2_cls_head_fwd(A, A, A, A, 0, 4, 3, None) == -1
    assert lib.lr2_cls_head_fwd(A, A, A, A, 1, 6, 3, None) == -2          # D % 4
    assert lib.lr2_cls_head_fwd(A, A, A, A, 1, 4, 0, None) == -2
    assert lib.lr2_cls_head_fwd(A, A, A, A, 1, 4, 9, None) == -2
    for off in (4, 8, 12):
        assert lib.lr2_cls_head_fwd(A + off, A, A, A, 1, 4, 3, None) == -2
        assert lib.lr2_cls_head_fwd(A, A + off, A, A, 1, 4, 3, None) == -2

    assert lib.lr2_cls_head_bwd(None, A, A, A, A, A, 1, 4, 3, None) == -1
    assert lib.lr2_cls_head_bwd(A, None, A, A, A, A, 1, 4, 3, None) == -1
    assert lib.lr2_cls_head_bwd(A, A, None, A, A, A, 1, 4, 3, None) == -1
    assert lib.lr2_cls_head_bwd(A, A, A, A, A, A, 0, 4, 3, None) == -1
    assert lib.lr2_cls_head_bwd(A, A, A, A, A, A, 1, 6, 3, None) == -2
    assert lib.lr2_cls_head_bwd(A, A, A, A, A, A, 1, 4, 0, None) == -2
    assert lib.lr2_cls_head_bwd(A, A, A, A, A, A, 1, 4, 9, None) == -2
    for off in (4, 8, 12):                                                # the input-gradient kernel's float4 accesses: w and dx
        assert lib.lr2_cls_head_bwd(A, A + off, A, A, A, A, 1, 4, 3, None) == -2
        assert lib.lr2_cls_head_bwd(A, A, A, A + off, A, A, 1, 4, 3, None) == -2
        assert lib.lr2_cls_head_bwd(A, A, A, A + off, None, None, 1, 4, 3, None) == -2


def test_cls_scores_and_nll_contract(lib):
    assert lib.lr2_cls_scores(None, A, A, 1, 3, 1, None) == -1
    assert lib.lr2_cls_scores(A, A, None, 1, 3, 1, None) == -1
    assert lib.lr2_cls_scores(A, None, A, 0, 3, 1, None) == -1
    assert lib.lr2_cls_scores(A, None, A, 1, 0, 1, None) == -2
    assert lib.lr2_cls_scores(A, None, A, 1, 9, 1, None) == -2

    assert lib.lr2_cls_scores_bwd(None, A, A, A, 1, 3, None) == -1
    assert lib.lr2_cls_scores_bwd(A, None, A, A, 1, 3, None) == -1
    assert lib.lr2_cls_scores_bwd(A, A, None, A, 1, 3, None) == -1
    assert lib.lr2_cls_scores_bwd(A, A, A, None, 1, 3, None) == -1
    assert lib.lr2_cls_scores_bwd(A, A, A, A, 0, 3, None) == -1
    assert lib.lr2_cls_scores_bwd(A, A, A, A, 1, 0, None) == -2
    assert lib.lr2_cls_scores_bwd(A, A, A, A, 1, 9, None) == -2

    assert lib.lr2_nll_loss(None, A, 1, 3, A, None, None) == -1
    assert lib.lr2_nll_loss(A, None, 1, 3, A, None, None) == -1
    assert lib.lr2_nll_loss(A, A, 1, 3, None, None, None) == -1
    assert lib.lr2_nll_loss(A, A, 0, 3, A, None, None) == -1
    assert lib.lr2_nll_loss(A, A, 1, 0, A, A, None) == -2
    assert lib.lr2_nll_loss(A, A, 1, 9, A, A, None) == -2
