"""The f16 short tiles, the parts that need no GPU: the additive ABI (lr2_gemm_f16_tiled / lr2_gemm_f16_launch_counts inside ABI 27),
lr2_gemm_f16_tiled's argument checks (lr2_gemm_f16's list at every block_m; nothing launched or counted by a refused call), the dispatch
rule ops.f16_block_m against the measured table in its own docstring, and tools/gemm_bench.py's parser."""
import ctypes
import os
import re
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_number_stays_27_and_the_new_names_are_declared():
    from lr2ppo_amd import _native as native
    hdr = open(os.path.join(REPO, "include", "lr2ppo_hip.h")).read()
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert native.ABI_VERSION == 27 == int(re.search(r"#define LR2_ABI_VERSION (\d+)", hdr).group(1))
    assert int(re.search(r"lr2_abi_version\(\) == (\d+)", doc).group(1)) == 27 and native.lib().lr2_abi_version() == 27
    for name in ("lr2_gemm_f16_tiled", "lr2_gemm_f16_launch_counts"):
        assert name in native.SIGNATURES
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in doc
        assert hasattr(native.lib(), name)
    assert native.SIGNATURES["lr2_gemm_f16_tiled"] == native.SIGNATURES["lr2_gemm_bf16"]
    # ... and the header gives it lr2_gemm_bf16's parameter list, block_m before stream
    params = lambda n: re.sub(r"\s+", " ", re.search(r"\bint %s\(([^;]*)\);" % n, hdr).group(1))       # noqa: E731
    assert params("lr2_gemm_f16_tiled") == params("lr2_gemm_bf16")
    assert params("lr2_gemm_f16_tiled").endswith("int block_m, void* stream")
    # lr2_gemm_f16 keeps its signature
    assert native.SIGNATURES["lr2_gemm_f16"] == native.SIGNATURES["lr2_gemm_bf16"][:-2] + native.SIGNATURES["lr2_gemm_bf16"][-1:]


@pytest.mark.parametrize("block_m", [256, 128, 64])
def test_gemm_f16_tiled_validates_before_launching(block_m):
    """tests/test_f16_mode_cpu.py::test_gemm_f16_validates_before_launching's list, through lr2_gemm_f16_tiled."""
    from lr2ppo_amd import _native as native
    lib = native.lib()
    A = 16          # a stand-in device address (nothing is dereferenced: every call fails)

    def epi(**kw):
        e = native.Epilogue()
        e.out, e.ld_out, e.alpha = A, 256, 1.0
        for k, v in kw.items():
            setattr(e, k, v)
        return ctypes.byref(e)

    def call(a, b, M, N, K, e, a_bytes=None, b_bytes=None):
        return lib.lr2_gemm_f16_tiled(a, b, M, N, K, K, K, M * K * 2 if a_bytes is None else a_bytes,
                                      N * K * 2 if b_bytes is None else b_bytes, e, block_m, None)

    def counters():
        c, k = ctypes.c_uint64(0), (ctypes.c_uint64 * 2)()
        assert lib.lr2_gemm_f16_launch_count(ctypes.byref(c)) == 0 and lib.lr2_gemm_f16_launch_counts(k) == 0
        return c.value, k[0], k[1]

    before = counters()
    assert call(None, None, 256, 256, 64, epi()) == -1                       # null operands
    assert call(A, None, 256, 256, 64, epi()) == -1
    assert call(None, A, 256, 256, 64, epi()) == -1
    assert call(A, A, 256, 256, 64, None) == -1                              # no epilogue
    assert call(A, A, 256, 256, 64, epi(out=None)) == -1                     # no destination
    assert call(A, A, 256, 256, 96, epi()) == -2                             # K must be whole 64-deep steps
    assert call(A, A, 256, 256, 32, epi()) == -2
    assert call(A, A, 256, 254, 64, epi()) == -2                             # N % 4
    assert call(A, A, 256, 256, 64, epi(ld_out=128)) == -2                   # a leading dimension smaller than the row
    # inference only: every training epilogue request
    assert call(A, A, 256, 256, 64, epi(drop_p=0.1)) == -1                   # dropout
    assert call(A, A, 256, 256, 64, epi(out=None, adam_p=A, adam_m=A, adam_v=A)) == -1   # the fused optimizer
    assert call(A, A, 256, 256, 64, epi(adam_p=A, adam_m=A, adam_v=A)) == -1
    assert call(A, A, 256, 256, 64, epi(act=2, aux_z=A, ld_aux=256)) == -1   # GELU'
    assert call(A, A, 256, 256, 64, epi(accumulate=1)) == -1
    assert call(A, A, 256, 256, 64, epi(out_z=A, ld_z=256, act=1)) == -1     # the kept pre-activation
    assert call(A, A, 256, 256, 64, epi(colsum=A, colsum_ws=A)) == -1
    # operand extents: 4 GiB and more at every tile height (32-bit buffer extents) ...
    assert call(A, A, 256, 256, 64, epi(), a_bytes=1 << 32) == -2
    assert call(A, A, 256, 256, 64, epi(), b_bytes=(1 << 32) + 512) == -2
    # ... and the ring's 4 GiB - 768 B limit for the call that asks for the 256 x 256 kernel
    if block_m == 256:
        assert call(A, A, 256, 256, 64, epi(), a_bytes=0xFFFFFD01) == -2
        assert call(A, A, 256, 256, 64, epi(), b_bytes=0xFFFFFFFF) == -2
    assert counters() == before                                              # nothing was launched, nothing counted
    assert lib.lr2_gemm_f16_launch_counts(None) == -1


SPREAD = 0.03           # the largest spread between two runs of one variant in the measurement (f16_block_m's docstring)


def _docstring_table():
    from lr2ppo_amd import ops
    rows = re.findall(r"M=(\d+) N=(\d+) K=(\d+):\s*([\d.]+) / ([\d.]+) / ([\d.]+) / ([\d.]+)\s*->\s*(\d+)", ops.f16_block_m.__doc__)
    return [(int(m), int(n), int(k), tuple(float(x) for x in us), int(bm)) for m, n, k, *us, bm in rows]


def test_f16_block_m_agrees_with_its_measured_table():
    """Every shape the rule was to be fitted on is in the docstring (us: lr2_gemm_f16 as before / block_m 256 / 128 / 64 -> the rule's
    answer); the rule answers what the table says; no listed shape is slower than lr2_gemm_f16 was (beyond the measured spread); and
    a shape leaves the 256 x 256 kernel for a short tile only where that tile is ahead by more than the spread."""
    from lr2ppo_amd import ops
    table = _docstring_table()
    listed = {(m, n, k) for m, n, k, _, _ in table}
    want = {(M, N, K) for M in (100864, 12544) for N, K in ((3072, 768), (768, 3072), (2304, 768))}
    want |= {(12544, 768, 768)} | {(6304, N, K) for N, K in ((2304, 768), (768, 768), (3072, 768), (768, 3072))}
    assert want <= listed and len(table) == len(listed), sorted(want - listed)
    for M, N, K, us, bm in table:
        assert ops.f16_block_m(M, N, K) == bm, (M, N, K)
        before, t = us[0], dict(zip((256, 128, 64), us[1:]))
        assert t[bm] <= before * (1 + SPREAD), (M, N, K)
        if bm != 256:
            assert t[bm] < min(before, t[256]) / (1 + SPREAD), (M, N, K)
            assert t[bm] == min(t.values()), (M, N, K)


def test_f16_block_m_is_a_tile_height_everywhere():
    from lr2ppo_amd import ops
    for M in (1, 32, 197, 788, 6304, 12544, 25088, 100864, 125440):
        for N in (32, 64, 128, 256, 768, 1536, 2304, 3072):
            for K in (64, 128, 768, 3072):
                assert ops.f16_block_m(M, N, K) in (256, 128, 64), (M, N, K)
    # K % 64 != 0 (never true in the schedule; either kernel refuses it): a short tile, never the 256 x 256 ring
    for M, N in ((100864, 3072), (12544, 768), (32, 32)):
        for K in (32, 100, 800):
            assert ops.f16_block_m(M, N, K) in (128, 64), (M, N, K)


def test_force_256_bypasses_the_rule():
    from lr2ppo_amd import ops
    assert ops.f16_schedule_block_m(32, 384, 128) == ops.f16_block_m(32, 384, 128)
    with ops.f16_force_256():
        assert ops.f16_schedule_block_m(32, 384, 128) is None
        with ops.f16_force_256():
            assert ops.f16_schedule_block_m(12544, 3072, 768) is None
        assert ops.f16_schedule_block_m(32, 384, 128) is None
    assert ops.f16_schedule_block_m(32, 384, 128) == ops.f16_block_m(32, 384, 128)


def test_gemm_bench_takes_the_f16_tile_heights():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import gemm_bench
    a = gemm_bench.parse_args(["--f16", "--bm", "64"])
    assert a.f16 and a.bm == 64
    assert gemm_bench.parse_args(["--f16"]).bm is None                        # -> ops.f16_block_m
    with pytest.raises(SystemExit):
        gemm_bench.parse_args(["--f16", "--bm", "192"])
    with pytest.raises(SystemExit):
        gemm_bench.parse_args(["--f16", "--bf16"])
    shapes = {(M, N, K) for form, M, N, K in gemm_bench.SHAPES if form == "NT"}
    assert {(6304, 2304, 768), (6304, 768, 768), (6304, 3072, 768), (6304, 768, 3072)} <= shapes


def test_the_two_f16_kernels_of_the_family_use_no_scratch():
    """The F16 instantiations of gemm_kernel (the last template argument true): no spilled register, no private memory."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import kernel_resources
    ks = [k for k in kernel_resources.kernels() if k["name"].startswith("gemm_kernel<") and k["name"].endswith(", false, true>")]
    assert sorted(k["name"].split(",")[0] for k in ks) == ["gemm_kernel<128", "gemm_kernel<64"], [k["name"] for k in ks]
    for k in ks:
        assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
