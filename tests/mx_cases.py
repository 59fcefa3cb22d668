"""Reference quantiser, edge blocks, census and layout helpers of the MX-FP8 edge tests (test_mx_edges_cpu.py / test_mx_edges_gpu.py).

Nothing here touches the GPU or lr2ppo_amd.ops: everything returns CPU tensors, the GPU file lays them out and runs them.

The rule (OCP MX v1.0 section 6.3 as csrc/fp8.hip states it): per 32 consecutive elements, amax = max |x| (a NaN does not take
part); shared exponent e = floor(log2 amax) - 8 read from the fp32 exponent field, -127 when amax < FLT_MIN, clamped to [-127, 127];
scale byte e + 127; element = e4m3fn of clamp(x * 2^-e, -448, 448), round to nearest, ties to the even mantissa.

ref_quant() restates it WITHOUT a float8 cast: the 127 finite non-negative e4m3fn magnitudes as a table, the scaled value in fp64 (a
power-of-two factor: exact), the nearest entry, the even byte on a tie, the sign bit on top.  What it does not decide: the byte of a
NaN element (`free` in its result) and the sign of a zero byte (compare with same_bytes()).

Edge blocks (32 fp32 values each; `s` runs over SHIFTS wherever a class is built "at 2^s"):
  ties       anchor 256 * 2^s (scale exactly 2^s) + every midpoint of adjacent magnitudes * 2^s, both signs, with its fp32 successor
             and predecessor
  subnormal  k * 2^-10 * 2^s for k = 1, 2, 3, 5, 7 with neighbours (the 0 / 1 tie at 2^-10, the 1 / 2 tie at 3 * 2^-10), 2^-6 * 2^s and
             the number below it
  saturate   amax in {448, 449, 463.99, 464, 480, 511.99} * 2^s in both signs on four neighbouring elements (every slot of a packed
             conversion), ordinary companions: all +-448; from 464 up an unclamped conversion would not give 448
  pow2       amax = 2^k and the number below it, k in {-126, -118, 0, 8, 9, 127}
  tiny       +0 / -0 mixed; all fp32-denormal; amax = FLT_MIN
  huge       amax = FLT_MAX; +Inf, -Inf among ordinary values
  nan        one NaN among ordinary values
  position   32 blocks, the one large element of block i at position i; consecutive blocks at 2^0, 2^+20, 2^-20, so a maximum taken
             over the wrong lanes, or across a block boundary, changes a scale byte
  outlier    one 1e30 among values near 1
build_blocks(bf16=True) is the same list restricted to numbers one bf16 plane holds (midpoints without their fp32 neighbours,
saturating values on the bf16 grid): what an attention V row can carry."""
import math
from collections import namedtuple

import torch

FLT_MIN = 2.0 ** -126
FLT_MAX = float.fromhex("0x1.fffffep127")
SHIFTS = (0, -20, 30)
SENT8 = 0xA5              # canary byte of e4m3 / scale destinations
PAT32 = 0x7FC0BEEF        # canary of fp32 destinations (a NaN)
PAT16 = 0x7FC1            # canary of bf16 destinations (a NaN)
XROWS = 3                 # canary rows behind every destination


def _table():
    t = []
    for byte in range(127):
        ex, m = byte >> 3, byte & 7
        t.append(m / 8.0 * 2.0 ** -6 if ex == 0 else (1.0 + m / 8.0) * 2.0 ** (ex - 7))
    return torch.tensor(t, dtype=torch.float64)


TABLE = _table()                          # TABLE[b] = |value| of e4m3fn byte b, b = 0 .. 0x7E (0x7F is NaN)
MID = (TABLE[1:] + TABLE[:-1]) / 2        # the 126 rounding ties


# ---- the rule ----
def block_amax(xb):
    """max |x| over the last axis, NaN left out (fmaxf)."""
    a = xb.float().abs()
    return torch.where(torch.isnan(a), torch.zeros_like(a), a).amax(-1)


def shared_exponent(amax):
    """floor(log2 amax) - 8 from the fp32 bit pattern; -127 below FLT_MIN; clamped to [-127, 127]."""
    a = amax.float().contiguous()
    e = ((a.view(torch.int32) >> 23) & 0xFF) - 127 - 8
    e = torch.where(a < FLT_MIN, torch.full_like(e, -127), e)
    return e.clamp(-127, 127)


def scale_byte(amax):
    return int(shared_exponent(torch.tensor([amax], dtype=torch.float32))[0]) + 127


def _scaled(x):
    """(|x| * 2^-e in fp64 [R, K / 32, 32], e [R, K / 32])."""
    R, K = x.shape
    assert K % 32 == 0 and x.dtype == torch.float32
    xb = x.view(R, K // 32, 32)
    e = shared_exponent(block_amax(xb))
    return xb.double().abs() * torch.exp2(-e.double()).unsqueeze(-1), e


RefQuant = namedtuple("RefQuant", "q s free")


def ref_quant(x):
    """x fp32 [R, K] -> (bytes uint8 [R, K], scale bytes uint8 [R, K / 32], free bool [R, K]: True where the rule does not decide)."""
    R, K = x.shape
    y, e = _scaled(x)
    free = torch.isnan(y)
    y = torch.where(free, torch.zeros_like(y), y).clamp(max=448.0)
    hi = torch.searchsorted(TABLE, y.contiguous()).clamp(max=126)      # first entry >= y
    lo = (hi - 1).clamp(min=0)
    dlo, dhi = y - TABLE[lo], TABLE[hi] - y
    even = torch.where(lo % 2 == 0, lo, hi)
    pick = torch.where(dlo < dhi, lo, torch.where(dhi < dlo, hi, even))
    sign = torch.signbit(x.view(R, K // 32, 32)).to(torch.int64) << 7
    return RefQuant((pick | sign).to(torch.uint8).view(R, K), (e + 127).to(torch.uint8), free.view(R, K))


def dequant(q, s):
    """bytes [R, K], scale bytes [R, K / 32] -> fp64 [R, K] (every byte finite)."""
    R, K = q.shape
    mag = TABLE[(q & 0x7F).long().clamp(max=126)]
    v = torch.where((q & 0x80) != 0, -mag, mag).view(R, K // 32, 32)
    return (v * torch.exp2(s.double() - 127.0).unsqueeze(-1)).view(R, K)


def same_bytes(got, ref):
    """Bool [R, K]: equal, or a zero on both sides (its sign is not the rule's), or not decided by the rule."""
    return (got == ref.q) | (((got & 0x7F) == 0) & ((ref.q & 0x7F) == 0)) | ref.free


def half_step(x):
    """fp64 [R, K]: half the e4m3 spacing at the scaled value, in units of x; inf where the element saturates or is not finite."""
    R, K = x.shape
    y, e = _scaled(x)
    step = torch.where(y < 2.0 ** -6, torch.full_like(y, 2.0 ** -9), torch.exp2(torch.floor(torch.log2(y.clamp_min(2.0 ** -6))) - 3))
    h = 0.5 * step * torch.exp2(e.double()).unsqueeze(-1)
    return torch.where((y <= 448.0), h, torch.full_like(h, math.inf)).view(R, K)


# ---- census ----
Census = namedtuple("Census", "ties subnormal above448 scale0 scale_hi pos tie_map")


def census(x):
    """What an fp32 matrix [R, K] puts in front of a quantiser.  Elements whose scaled value is an exact rounding tie / inside the e4m3
    subnormal range (0, 2^-6) / above 448; blocks with scale byte 0 / >= 246 / their maximum at each of the 32 positions (pos, first
    occurrence, blocks with amax > 0); tie_map: scale byte -> bool [2 signs, 126 midpoints] of the ties seen at that scale."""
    R, K = x.shape
    y, e = _scaled(x)
    fin = torch.isfinite(y)
    idx = torch.searchsorted(MID, torch.where(fin, y, torch.zeros_like(y)).contiguous()).clamp(max=125)
    tie = fin & (MID[idx] == y)
    xb = x.view(R, K // 32, 32)
    a = torch.where(torch.isnan(xb), torch.zeros_like(xb), xb.abs())
    pos = torch.bincount(a.argmax(-1)[a.amax(-1) > 0].flatten(), minlength=32)
    tie_map = {}
    neg = torch.signbit(xb)
    for r, b, k in tie.nonzero().tolist():
        m = tie_map.setdefault(int(e[r, b]) + 127, torch.zeros(2, 126, dtype=torch.bool))
        m[int(neg[r, b, k]), int(idx[r, b, k])] = True
    return Census(int(tie.sum()), int((fin & (y > 0) & (y < 2.0 ** -6)).sum()), int((y > 448.0).sum()), int((e == -127).sum()),
                  int((e + 127 >= 246).sum()), pos, tie_map)


def census_counts(c):
    return (c.ties, c.subnormal, c.above448, c.scale0, c.scale_hi, tuple(c.pos.tolist()))


# ---- edge blocks ----
Block = namedtuple("Block", "cls name vals")


def _f32(v):
    return torch.tensor(v, dtype=torch.float64).float()


def _up(v):
    return torch.nextafter(v, torch.full_like(v, math.inf))


def _down(v):
    """Towards zero for the non-negative values this is used on."""
    return torch.nextafter(v, torch.full_like(v, -math.inf))


def _companions(scale):
    """31 ordinary values in +-[0.75, 1.69] * scale, alternating sign, each a 6-bit number times the scale."""
    j = torch.arange(31, dtype=torch.float64)
    return (((24 + j) / 32.0) * (1 - 2 * (j % 2)) * scale).float()


def _block(cls, name, special, at, scale):
    """`special` (a list of values) at positions at, at + 1, ... (mod 32); ordinary companions * scale elsewhere."""
    v = torch.zeros(32)
    comp = _companions(scale)
    taken = {(at + i) % 32 for i in range(len(special))}
    free = [p for p in range(32) if p not in taken]
    for p, c in zip(free, comp.tolist()):
        v[p] = c
    for i, sv in enumerate(special):
        v[(at + i) % 32] = sv
    return Block(cls, name, v)


def build_blocks(bf16=False):
    out = []
    n = [0]

    def at():                   # a new position for the special elements of each block: 7 k mod 32 visits every residue mod 8
        n[0] += 1
        return (7 * n[0]) % 32

    def chunks(cls, name, vals, anchor, scale):
        for i in range(0, len(vals), 31):
            part = vals[i:i + 31]
            out.append(_block(cls, f"{name}[{i // 31}]", [anchor] + part, at(), scale))

    for s in SHIFTS:
        f = 2.0 ** s
        mids = (MID * f).float()
        assert bool((mids.double() == MID * f).all())
        vals = []
        for m in mids:
            m = m.reshape(1)
            group = [m] if bf16 else [m, _up(m), _down(m)]
            for g in group:
                vals += [float(g), -float(g)]
        chunks("ties", f"ties 2^{s}", vals, 256.0 * f, f)
        vals = []
        for k in (1, 2, 3, 5, 7):
            m = _f32([k * 2.0 ** -10 * f])
            for g in ([m] if bf16 else [m, _up(m), _down(m)]):
                vals += [float(g), -float(g)]
        top = _f32([2.0 ** -6 * f])
        below = top * (1 - 2.0 ** -8) if bf16 else _down(top)
        vals += [float(top), -float(top), float(below), -float(below)]
        chunks("subnormal", f"subnormal 2^{s}", vals, 256.0 * f, f)
        for a in ((448.0, 464.0, 480.0, 496.0, 508.0) if bf16 else (448.0, 449.0, 463.99, 464.0, 480.0, 511.99)):
            a32 = float(_f32([a])) * f
            out.append(_block("saturate", f"saturate {a} 2^{s}", [a32, -a32, a32, -a32], at(), f))
    for k in (-126, -118, 0, 8, 9, 127):
        p = _f32([2.0 ** k])
        below = p * (1 - 2.0 ** -6) if bf16 else _down(p)        # 63 / 64: a bf16 number even as a denormal
        for name, v in ((f"pow2 2^{k}", p), (f"pow2 below 2^{k}", below)):
            sign = -1.0 if len(out) % 2 else 1.0
            out.append(_block("pow2", name, [sign * float(v)], at(), 2.0 ** max(k - 2, -128)))
    j = torch.arange(32)
    out.append(Block("tiny", "tiny zeros", torch.where(j % 3 == 0, -torch.zeros(32), torch.zeros(32))))
    lo_exp = -133 if bf16 else -149
    den = torch.exp2((lo_exp + (j * (-127 - lo_exp)) // 31).double()).float() * (1 - 2 * (j % 2)).float()
    out.append(Block("tiny", "tiny denormals", den))
    out.append(_block("tiny", "tiny FLT_MIN", [FLT_MIN], at(), 2.0 ** -128))
    big = FLT_MAX
    if bf16:
        big = float(torch.tensor([0x7F7F], dtype=torch.int16).view(torch.bfloat16).float())      # the largest finite bf16
    hv = _block("huge", "huge FLT_MAX", [-big], at(), 2.0 ** 120).vals
    hv[(torch.arange(32) % 5 == 0) & (hv.abs() < 2.0 ** 121)] = 1.25       # ordinary values next to it: they scale to zero
    out.append(Block("huge", "huge FLT_MAX", hv))
    out.append(_block("huge", "huge +Inf", [math.inf], at(), 1.0))
    out.append(_block("huge", "huge -Inf", [-math.inf], at(), 1.0))
    out.append(_block("nan", "nan", [math.nan, 300.0], at(), 1.0))
    for i in range(32):
        f = 2.0 ** (20 * ((i + 1) % 3 - 1))                    # 2^0, 2^+20, 2^-20, ...
        out.append(_block("position", f"position {i}", [300.0 * f * (-1.0 if i % 2 else 1.0)], i, f))
    huge = float(torch.tensor([1e30]).bfloat16().float()) if bf16 else float(_f32([1e30]))
    out.append(_block("outlier", "outlier", [huge], at(), 1.0))
    return out


BLOCKS = build_blocks()
BLOCKS_BF16 = build_blocks(bf16=True)


def is_bf16(v):
    r = v.bfloat16().float()
    return bool(((r == v) | (torch.isnan(r) & torch.isnan(v))).all())


def planes_of(x):
    """(hi, lo) bf16 of the RNE split of an fp32 tensor."""
    hi = x.bfloat16()
    return hi, (x - hi.float()).bfloat16()


def splits_exactly(v):
    """hi + lo == v, every value finite: what a Planes operand can hand a quantiser unchanged."""
    hi, lo = planes_of(v)
    return bool(torch.isfinite(v).all()) and bool(torch.equal(hi.float() + lo.float(), v)) and bool(torch.isfinite(lo.float()).all())


# ---- layouts ----
def lay(blocks, rows, width, start=0, full=None):
    """fp32 [rows, 32 * width]: slot (r, b) holds block (start + r * full + b) mod len(blocks); full (default width) < width leaves the
    last slot of a row to a block that will be cut (a transposed operand whose row count is no multiple of 32).  Consecutive rows
    continue the list, so every row carries another sequence.  Returns (matrix, index [rows, width])."""
    full = width if full is None else full
    nb = len(blocks)
    idx = torch.empty(rows, width, dtype=torch.long)
    for r in range(rows):
        for b in range(width):
            idx[r, b] = (start + r * full + b) % nb if b < full else (start + rows * full + r) % nb
    m = torch.stack([blocks[i].vals for i in idx.flatten().tolist()]).view(rows, width * 32)
    return m.clone(), idx


def rows_for(blocks, width):
    return -(-len(blocks) // width)


def leading_dims(K, N):
    """Distinct, non-tight leading dimensions (multiples of 4) for x [., K], out [., N], resid [., N]."""
    return dict(ldx=K + 8, ld_out=N + 12, ld_resid=N + 20)


def takes_ring(M, N, K):
    """lr2_gemm_mxfp8's choice of the 256 x 256 ring kernel, restated from csrc/fp8.hip."""
    t256 = -(-M // 256) * -(-N // 256)
    rounds = -(-t256 // 256)
    lim = 0xFFFFFD00
    return t256 >= 256 and t256 * 100 >= 80 * rounds * 256 and M * K <= lim and N * K <= lim


# ---- exact products ----
def int_operands(M, N, K, seed=0):
    """A [M, K], B [N, K] (fp64): small integers j * 2^k, |j| <= 3, k in 0 .. 4 drawn per (row mod 3, K block) for A and per (row mod 2,
    K block) for B: every 32-element K block of a row on its own power-of-two scale, in no periodic order along K (a K slice that took
    another slice's scales would not pass), B unlike A.  |a|, |b| <= 48, so every partial sum is an integer below 640 * 48 * 48 < 2^24
    up to K = 640, and an element is an e4m3 number under its block's scale."""
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K + seed)
    ka = torch.randint(0, 5, (3, K // 32), generator=g)[torch.arange(M) % 3]
    kb = torch.randint(0, 5, (2, K // 32), generator=g)[torch.arange(N) % 2]
    a = torch.randint(-3, 4, (M, K), generator=g).double() * torch.exp2(ka.double()).repeat_interleave(32, 1)
    b = torch.randint(-3, 4, (N, K), generator=g).double() * torch.exp2(kb.double()).repeat_interleave(32, 1)
    return a, b


PRODUCT_SHAPES = [(1, 128, 128), (63, 128, 256), (64, 256, 128), (129, 384, 640), (257, 128, 256)]
WGRAD_SHAPE = (128, 256, 640)
RING_SHAPES = [(8192, 2048, 128), (8100, 2048, 128)]
