"""CPU half of the MX-FP8 edge suite: tests/mx_cases.py's reference quantiser against torch's own e4m3fn cast where that cast is
defined, the scale-byte anchors of the rule, the census of the assembled edge matrix (what test_mx_edges_gpu.py asserts before it
compares a byte), the half-step property of the dequantised reference, and the restated kernel-choice rule on the shapes the GPU
file uses."""
import math

import pytest
import torch

import mx_cases as MC


def _torch_bytes(v):
    return v.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)


def test_table_is_the_e4m3fn_magnitudes():
    back = torch.arange(127, dtype=torch.uint8).view(torch.float8_e4m3fn).double()
    assert torch.equal(back, MC.TABLE)
    assert float(MC.TABLE[-1]) == 448.0 and float(MC.TABLE[1]) == 2.0 ** -9 and float(MC.TABLE[8]) == 2.0 ** -6
    assert len(MC.MID) == 126 and bool((MC.MID.float().double() == MC.MID).all())
    assert MC.is_bf16(MC.MID.float())                     # every tie is a bf16 number: an attention V row can carry it


def test_reference_equals_torchs_cast_on_ties_neighbours_magnitudes_and_the_clamp_band():
    """1022 points at scale 2^0 (an anchor of 256 in every block): all 126 midpoints, their fp32 neighbours on both sides, all 127
    magnitudes, 448 / 456 / 463.99 / 464 / 480 / 1e4, both signs of everything."""
    mid = MC.MID.float()
    up = torch.nextafter(mid, torch.full_like(mid, math.inf))
    down = torch.nextafter(mid, torch.full_like(mid, -math.inf))
    pts = torch.cat([mid, up, down, MC.TABLE.float(), torch.tensor([448.0, 456.0, 463.99, 464.0, 480.0, 1e4])])
    pts = torch.cat([pts, -pts])
    assert pts.numel() == 1022
    n = -(-pts.numel() // 31)
    x = torch.zeros(n, 32)
    x[:, 0] = 256.0
    body = torch.zeros(n * 31)
    body[:pts.numel()] = pts
    x[:, 1:] = body.view(n, 31)
    x[:, 0] = torch.where(x[:, 1:].abs().amax(1) >= 512, x[:, 1:].abs().amax(1), x[:, 0])      # (1e4 sets its own block's scale)
    ref = MC.ref_quant(x)
    e = (ref.s.double() - 127.0)
    want = _torch_bytes((x.view(n, 1, 32).double() * torch.exp2(-e).unsqueeze(-1)).float().view(n, 32))
    assert not ref.free.any()
    assert torch.equal(ref.q, want), f"{int((ref.q != want).sum())} of {x.numel()} differ"


@pytest.mark.parametrize("amax,byte", [(2.0 ** -149, 0), (2.0 ** -127, 0), (MC.FLT_MIN, 0), (1.5 * 2.0 ** -126, 0), (2.0 ** -119, 0),
                                       (1.99 * 2.0 ** -118, 1), (1.0, 119), (255.99, 126), (256.0, 127), (448.0, 127),
                                       (MC.FLT_MAX, 246), (math.inf, 247)])
def test_scale_byte_anchors(amax, byte):
    assert MC.scale_byte(amax) == byte
    x = torch.full((1, 32), 0.0)
    x[0, 13] = -amax
    assert int(MC.ref_quant(x).s[0, 0]) == byte


def test_a_nan_takes_no_part_in_the_maximum_and_is_left_undecided():
    x = torch.full((1, 32), 1.0)
    x[0, 7] = math.nan
    ref = MC.ref_quant(x)
    assert int(ref.s[0, 0]) == 119 and bool(ref.free[0, 7]) and int(ref.free.sum()) == 1
    assert bool((ref.q[0][~ref.free[0]] == 0x78).all())            # 1.0 * 2^8 = 256 = byte 0x78


def _edge_matrix(blocks, width=8):
    return MC.lay(blocks, MC.rows_for(blocks, width), width)[0]


@pytest.mark.parametrize("which", ["fp32", "bf16"])
def test_census_of_the_edge_matrix(which):
    """Every tie at each of the three scales in both signs, every position of the maximum, and each other class present."""
    blocks = MC.BLOCKS if which == "fp32" else MC.BLOCKS_BF16
    c = MC.census(_edge_matrix(blocks))
    for s in MC.SHIFTS:
        assert 127 + s in c.tie_map and bool(c.tie_map[127 + s].all()), f"ties missing at 2^{s}"
    assert c.ties >= 3 * 2 * 126
    assert bool((c.pos >= 1).all()), c.pos.tolist()
    assert c.subnormal >= 3 * 2 * 5 and c.above448 >= 3 * 4 * 4 + 2 and c.scale0 >= 3 and c.scale_hi >= 3
    if which == "bf16":
        assert all(MC.is_bf16(b.vals) for b in blocks)
    classes = {b.cls for b in blocks}
    assert classes == {"ties", "subnormal", "saturate", "pow2", "tiny", "huge", "nan", "position", "outlier"}
    print(f"{which}: {len(blocks)} blocks, census {MC.census_counts(c)[:5]}")


def test_saturating_values_sit_in_every_slot_of_a_packed_conversion():
    """A copy that dropped the clamp on one of its conversions (4 per lane in the epilogues, 8 in the stand-alone quantiser) meets a
    value >= 464 * scale in that slot."""
    slots = set()
    for b in MC.BLOCKS:
        if b.cls == "saturate":
            y, _ = MC._scaled(b.vals.view(1, 32))
            slots |= {p % 8 for p in (y[0, 0] >= 464.0).nonzero().flatten().tolist()}
    assert slots == set(range(8))


def test_position_blocks_stand_between_neighbours_of_another_scale():
    pos = [b for b in MC.BLOCKS if b.cls == "position"]
    assert len(pos) == 32
    sb = [MC.scale_byte(float(b.vals.abs().max())) for b in pos]
    for i, b in enumerate(pos):
        assert int(b.vals.abs().argmax()) == i
        assert MC.scale_byte(float(b.vals.abs().sort().values[-2])) <= sb[i] - 7          # without its large element: another byte
        assert abs(sb[i] - sb[(i + 1) % 32]) >= 20 or i == 31


def test_dequantised_reference_is_within_half_a_step():
    x = _edge_matrix(MC.BLOCKS)
    ref = MC.ref_quant(x)
    ok = ~ref.free & torch.isfinite(x)
    err = (MC.dequant(ref.q, ref.s) - x.double()).abs()
    h = MC.half_step(x)
    assert bool((err[ok] <= h[ok]).all()), float((err[ok] - h[ok]).max())
    sat = torch.isinf(h) & ok
    assert int(sat.sum()) >= 3 * 4 * 5 and bool(((ref.q[sat] & 0x7F) == 0x7E).all())       # what saturates is +-448


def test_planes_split_is_exact_on_most_blocks():
    exact = [b for b in MC.BLOCKS if MC.splits_exactly(b.vals)]
    assert {b.cls for b in exact} >= {"ties", "subnormal", "saturate", "pow2", "position"}
    assert sum(b.cls == "ties" for b in exact) == sum(b.cls == "ties" for b in MC.BLOCKS)


def test_takes_ring_on_the_shapes_the_gpu_file_uses():
    for M, N, K in MC.RING_SHAPES:
        assert MC.takes_ring(M, N, K)
    assert not MC.takes_ring(8192 - 256, 2048, 128)                 # 248 tiles: the smallest ring shape is the one used
    for M, N, K in MC.PRODUCT_SHAPES + [(1, 256, 128), (65, 256, 128), (130, 256, 128)]:
        assert not MC.takes_ring(M, N, K)


def test_the_flt_min_line_of_the_rule_follows_from_the_clamp():
    """Every kernel copy has `if (amax < FLT_MIN) e = -127` in front of `if (e < -127) e = -127`.  Below FLT_MIN the exponent field
    is 0, so the field alone gives -127 - 8 = -135 and the clamp gives -127: the two lines cannot be told apart by any input (a mutant
    that drops the first from one copy passes every test, by arithmetic and not for want of a case)."""
    a = torch.tensor([0.0, 2.0 ** -149, 2.0 ** -127, 1.5 * 2.0 ** -127, float(torch.nextafter(torch.tensor(MC.FLT_MIN, dtype=torch.float32),
                                                                                            torch.tensor(0.0)))])
    field = ((a.view(torch.int32) >> 23) & 0xFF) - 127 - 8
    assert bool((field == -135).all()) and bool((field.clamp(-127, 127) == MC.shared_exponent(a)).all())


def test_wgrad_slices_carry_different_scales():
    """The K slices of the weight-gradient cases (splits 2 and 5 of K = 640) start at scale bytes unlike those at K = 0."""
    M, N, K = MC.WGRAD_SHAPE
    a, b = MC.int_operands(M, N, K, seed=2)
    for t in (a, b):
        s = MC.ref_quant(t.float()).s
        for splits in (2, 5):
            per = 4 * -(-(K // 128) // splits)                       # scale bytes per slice
            for i in range(1, -(-(K // 32) // per)):
                n = min(per, K // 32 - i * per)
                assert not torch.equal(s[:, i * per:i * per + n], s[:, :n]), (splits, i)


def test_integer_operands_are_exact():
    for M, N, K in MC.PRODUCT_SHAPES + [MC.WGRAD_SHAPE]:
        a, b = MC.int_operands(M, N, K)
        for t in (a, b):
            ref = MC.ref_quant(t.float())
            assert torch.equal(MC.dequant(ref.q, ref.s), t)
        assert float((a.abs() @ b.abs().t()).max()) < 2.0 ** 24
        assert not torch.equal(a[:min(M, N)] @ b.t()[:, :min(M, N)], (a[:min(M, N)] @ b.t()[:, :min(M, N)]).t()) or M == 1
        scales = MC.ref_quant(a.float()).s
        assert M == 1 or len(scales.unique()) >= 3
