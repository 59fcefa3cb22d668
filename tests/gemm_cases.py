"""Case tables, operand builders and fp64 references of the GEMM edge tests (test_gemm_edges_cpu.py / test_gemm_edges_gpu.py).

Nothing here touches the GPU or lr2ppo_amd.ops: the builders return CPU tensors, the GPU file lays them out and runs them.

Operand classes (logical A [M, K], B [N, K]; the product is always A . B^T):
  "exactA": A = h + j / 512 with |h| in {5, 6, 7} and |j| <= 7, so that A lies inside the binade [4, 8) (bf16 spacing 1/32): the RNE split
            gives hi = h and lo = j / 512 exactly, the lo plane non-zero almost everywhere; B = small integers whose range depends on the
            row (and A's sign / magnitude on row and column): a transposed output, a swapped half or plane changes the result.
  "exactB": the mirror.
  "int":    small integers on both sides (bf16 numbers: what the single-plane entry points can hold exactly).
  "rand":   randn, for the tolerance checks.
With sum_k |a||b| * 2^9 < 2^24 for every output element (exact_condition) every product and every partial sum, in any order, is a
multiple of 2^-9 below 2^24 of them: exact in fp32.  One operand has a zero lo plane, so the lo x lo term the three passes drop is
zero and the result must EQUAL the fp64 product.  Epilogue values that keep this: alpha 0.5 / 2, integer bias / residual / accumulate
target, dropout at p = 0.5 (scale exactly 2).

Layout (strides()): every leading dimension the entry point lets the caller set is distinct and not tight."""
import math
import zlib
from collections import namedtuple

import torch

BMAX = 9          # |B| (|A| in exactB) of the exact classes: 7.02 * 9 * K * 2^9 < 2^24 up to K = 518


# ---- tile-height rule of the 256 x 256 NT launchers, restated from csrc/gemm256.hip::gemm256_nt_tile_rows (launch_gemm256_nt, and
# launch_gemm256_b1 / launch_gemm256_b1_exact of gemm256_b1.hip, call it with the launch's M and N) ----
def tile_rows_256(M, N):
    tn = (N + 255) // 256
    t256, t192 = ((M + 255) // 256) * tn, ((M + 191) // 192) * tn
    return 192 if (t256 < 256 and t192 <= 256 and t192 > t256) else 256


# ---- lr2_gemm_row_split_plan, restated from csrc/gemm.hip ----
def row_split_plan(M, N, K):
    tn256 = (N + 255) // 256
    tiles = ((M + 255) // 256) * tn256
    full, rem = tiles // 256, tiles % 256
    M1 = ((full * 256) // tn256) * 256
    if full < 1 or full > 4 or rem <= 0 or 2 * rem >= 256 or K % 64 or M1 <= 0 or M1 >= M:
        return 0, 128
    t128 = ((M - M1 + 127) // 128) * ((N + 127) // 128)
    last = t128 % 512
    return M1, (64 if (t128 < 512 or 0 < last <= 128) else 128)


SEAM = (32768 + 200, 512, 64)      # 258 tiles of 256 x 256: one whole round + 2 -> 32 768 rows on the 256 x 256 kernel, 200 on 64-row tiles


def rup(x, m):
    return (x + m - 1) // m * m


Strides = namedtuple("Strides", "lda ldb ld_out ld_z ld_resid ld_aux ld_planes")


def strides(M, N, K, form):
    """Distinct, non-tight leading dimensions: multiples of 8 on the operands (planes rows of 16 bytes), of 4 on the epilogue's."""
    a_cols = M if form == "TN" else K
    b_cols = K if form == "NT" else N
    return Strides(rup(a_cols, 8) + 8, rup(b_cols, 8) + 24, N + 12, N + 20, N + 28, N + 36, N + 8)


# ---- operands ----
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _ints(g, rows, cols, bmax=BMAX):
    """Integers in [-bmax, bmax], the range shifted by the row's residue mod 7 (distinct rows) and the column's mod 3."""
    r = torch.arange(rows).view(-1, 1)
    c = torch.arange(cols).view(1, -1)
    x = torch.randint(-3, 4, (rows, cols), generator=g) + (r % 7) * 2 - 6 + (c % 3) - 1
    return x.clamp_(-bmax, bmax).double()


def _split_exact(g, rows, cols):
    """(value, h, j): value = h + j / 512, |h| in {5, 6, 7} by row and column, j in [-7, 7]."""
    r = torch.arange(rows).view(-1, 1)
    c = torch.arange(cols).view(1, -1)
    mag = 5 + (torch.randint(0, 3, (rows, cols), generator=g) + r + 2 * c) % 3
    sign = 1 - 2 * ((torch.randint(0, 2, (rows, cols), generator=g) + r) % 2)
    h = (mag * sign).double()
    j = torch.randint(-7, 8, (rows, cols), generator=g).double()
    return h + j / 512.0, h, j


def operands(cls, M, N, K, seed=0):
    """Logical A [M, K], B [N, K] as fp64 (every value an fp32 number)."""
    g = _gen(cls, M, N, K, seed)
    if cls == "exactA":
        return _split_exact(g, M, K)[0], _ints(g, N, K)
    if cls == "exactB":
        return _ints(g, M, K), _split_exact(g, N, K)[0]
    if cls == "int":
        return _ints(g, M, K, 7), _ints(g, N, K, 7)
    if cls == "rand":
        return torch.randn(M, K, generator=g).float().double(), torch.randn(N, K, generator=g).float().double()
    raise ValueError(cls)


def exact_condition(a, b):
    """max over the output elements of sum_k |a||b| * 2^9; must stay below 2^24."""
    return float((a.abs() @ b.abs().t()).max()) * 512.0


def rne_split(x):
    """(hi, lo) of the split-bf16 format, as fp64."""
    x32 = x.float()
    hi = x32.bfloat16().float()
    lo = (x32 - hi).bfloat16().float()
    return hi.double(), lo.double()


# ---- epilogues ----
# name -> what the call asks for.  "tol": the result passes through GELU / GELU' and is compared by the project's written tolerance
# rule, everything else of an exact class by torch.equal.
EPI = {
    "plain": {},
    "alpha_half": dict(alpha=0.5),
    "bias": dict(bias=True, alpha=2.0),
    "planes": dict(planes=True),
    "alpha_planes": dict(alpha=0.5, planes=True),
    "resid": dict(resid=True),
    "acc": dict(acc=True),
    "acc_alpha2": dict(acc=True, alpha=2.0),
    "resid_acc": dict(resid=True, acc=True),                  # two per-element requests
    "drop_resid": dict(bias=True, drop=True, resid=True, planes=True),
    "bias_resid": dict(bias=True, resid=True, planes=True),
    "act2": dict(act=2, tol=True),
    "gelu_z_planes": dict(bias=True, act=1, keep_z=True, planes=True, tol=True),
    "full": dict(bias=True, act=1, keep_z=True, drop=True, resid=True, planes=True, tol=True),
    # the forms the straight-line fast paths of the epilogue take (gemm_common.h::epilogue_fast_dispatch) on wave tiles inside the matrix
    "bias_only": dict(bias=True),
    "planes_only": dict(bias=True, planes=True, no_out=True),
    "gelu_z_noout": dict(bias=True, act=1, keep_z=True, planes=True, no_out=True, tol=True),
    "drop_resid_out": dict(bias=True, drop=True, resid=True),
    "drop_planes_only": dict(drop=True, planes=True, no_out=True),
    "resid_planes": dict(resid=True, planes=True),
}
DROP = (0.5, 4242, 5)       # p, seed, site


def gelu64(x):
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad64(z):
    return 0.5 * torch.erfc(-z / math.sqrt(2.0)) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def epilogue_inputs(epi, M, N, seed=0):
    """Integer bias [N], residual and accumulate target [M, N]; random aux_z (the GELU' input); all fp64."""
    g = _gen("epi", M, N, seed)
    e = EPI[epi]
    out = {}
    if e.get("bias"):
        out["bias"] = torch.randint(-9, 10, (N,), generator=g).double()
    if e.get("resid"):
        out["resid"] = (torch.randint(-9, 10, (M, N), generator=g) + (torch.arange(M).view(-1, 1) % 5)).double()
    if e.get("acc"):
        out["acc"] = (torch.randint(-9, 10, (M, N), generator=g) - (torch.arange(N).view(1, -1) % 3)).double()
    if e.get("act") == 2:
        out["aux"] = (torch.randn(M, N, generator=g) * 1.5).float().double()
    return out


def reference(epi, prod, ins, keep=None):
    """The epilogue of include/lr2ppo_hip.h in fp64, in its order: alpha, bias, GELU (z kept), dropout, GELU', resid, accumulate.
    Returns (out, z or None)."""
    e = EPI[epi]
    v = prod * e.get("alpha", 1.0)
    if "bias" in ins:
        v = v + ins["bias"].view(1, -1)
    z = None
    if e.get("act") == 1:
        z = v
        v = gelu64(v)
    if e.get("drop"):
        v = torch.where(keep.bool(), v / (1.0 - DROP[0]), torch.zeros_like(v))       # a dropped element is +0, whatever its sign was
    if e.get("act") == 2:
        v = v * gelu_grad64(ins["aux"])
    if "resid" in ins:
        v = v + ins["resid"]
    if "acc" in ins:
        v = v + ins["acc"]
    return v, z


def is_fp32(x):
    return bool((x.float().double() == x).all())


# ---- case tables ----
# lr2_gemm, general family: (form, kinds, block_m, passes, M, N, K, splits, class, epilogue).  kinds: f = fp32 matrix, p = planes.
# Every M in {1, 63, 64, 65, 127, 128, 129} and N in {4, 124, 128, 132} appears with every form; K: NT {64, 128}; NN of planes (32-deep
# tiles) {32, 96}; TN {1, 31, 32, 33, 63, 65, 100}.  128-row planes x planes NT / NN at three passes are the 8-wave kernels.
GENERAL = [
    ("NT", "ff", 64, 3, 1, 4, 64, 1, "exactA", "plain"),
    ("NT", "pp", 128, 3, 129, 132, 128, 1, "exactA", "gelu_z_planes"),
    ("NT", "pp", 64, 3, 63, 124, 64, 1, "exactB", "drop_resid"),
    ("NT", "pf", 128, 3, 127, 128, 128, 1, "exactA", "acc_alpha2"),
    ("NT", "pp", 128, 1, 128, 132, 64, 1, "exactA", "alpha_planes"),
    ("NT", "ff", 128, 3, 65, 128, 128, 1, "exactB", "act2"),
    ("NT", "pf", 64, 1, 64, 124, 64, 1, "exactB", "planes"),
    ("NT", "pp", 128, 3, 64, 4, 64, 1, "rand", "gelu_z_planes"),
    ("NT", "pp", 128, 3, 129, 132, 64, 1, "exactB", "resid_acc"),
    ("NT", "pp", 128, 3, 129, 132, 128, 1, "exactA", "gelu_z_noout"),
    ("NT", "pp", 128, 3, 128, 132, 64, 1, "exactA", "planes_only"),
    ("NN", "pp", 128, 3, 129, 132, 96, 1, "exactB", "drop_resid_out"),
    ("NT", "pp", 64, 3, 65, 132, 64, 1, "exactB", "resid_planes"),
    ("NN", "pp", 128, 3, 129, 132, 96, 1, "exactA", "drop_resid"),
    ("NN", "pp", 64, 3, 1, 4, 32, 1, "exactB", "plain"),
    ("NN", "ff", 128, 3, 63, 124, 64, 1, "exactA", "bias"),
    ("NN", "pf", 64, 3, 65, 128, 128, 1, "exactA", "planes"),
    ("NN", "pp", 128, 1, 127, 128, 32, 1, "exactB", "acc_alpha2"),
    ("NN", "pp", 64, 3, 64, 132, 96, 1, "rand", "gelu_z_planes"),
    ("NN", "ff", 64, 1, 128, 124, 64, 1, "exactB", "alpha_half"),
    ("TN", "pp", 128, 3, 129, 132, 100, 1, "exactA", "plain"),
    ("TN", "ff", 64, 3, 1, 4, 1, 1, "exactB", "alpha_half"),
    ("TN", "pp", 64, 3, 63, 124, 31, 1, "exactB", "acc_alpha2"),
    ("TN", "pf", 128, 3, 64, 128, 32, 1, "exactA", "bias"),
    ("TN", "ff", 128, 3, 65, 132, 33, 1, "exactA", "planes"),
    ("TN", "pp", 128, 1, 127, 128, 63, 1, "exactA", "plain"),
    ("TN", "pp", 64, 3, 128, 4, 65, 1, "exactB", "drop_resid"),
    ("TN", "pp", 128, 3, 128, 124, 100, 1, "exactA", "colsum"),
    # split-K: the whole epilogue runs in the reducer.  K tiles: 4 / 2 splits; 3 / 2 (uneven); 4 / 3 (TN, 32-deep, uneven); 2 / 5 (clamped)
    ("NT", "pp", 128, 3, 129, 132, 256, 2, "exactA", "full"),
    ("NT", "ff", 64, 3, 65, 124, 192, 2, "exactB", "full"),
    ("TN", "pp", 128, 3, 127, 132, 100, 3, "exactA", "full"),
    ("NN", "pp", 64, 3, 63, 128, 64, 5, "exactB", "full"),
    ("NT", "pf", 128, 3, 64, 4, 128, 2, "exactA", "drop_resid"),
]
EPI["colsum"] = dict(colsum=True)

# lr2_gemm(block_m = 256), NT, planes x planes, three passes: (M, N, K, class, epilogue).  By the tile-height rule M in {193, 256, 512}
# runs 192-row tiles and M in {1, 191, 192, 257, 320, 384} 256-row tiles (one tile row of 256 holds M <= 192 as well as one of 192).
NT256 = [
    (1, 4, 32, "exactA", "plain"),
    (191, 252, 64, "exactB", "gelu_z_planes"),
    (192, 256, 96, "exactA", "act2"),
    (193, 260, 32, "exactA", "resid"),
    (256, 256, 64, "exactB", "acc_alpha2"),
    (257, 260, 96, "exactA", "gelu_z_planes"),
    (320, 252, 32, "exactB", "drop_resid"),
    (384, 4, 64, "exactA", "planes"),
    (512, 260, 64, "exactA", "alpha_planes"),
    (257, 256, 96, "rand", "gelu_z_planes"),
    (193, 252, 96, "exactB", "acc"),
    (257, 260, 96, "exactA", "gelu_z_noout"),
    (320, 260, 64, "exactB", "drop_resid_out"),
    (193, 260, 32, "exactA", "planes_only"),
    (384, 256, 64, "exactA", "drop_planes_only"),
    (512, 252, 96, "exactB", "resid_planes"),
]
NT256_TWO_REQUESTS = (193, 256, 64, "exactA", "resid_acc")       # falls back to the general family

# lr2_gemm(block_m = 256), TN: (M, N, K, splits, class, epilogue, colsum).  32-deep K steps; splits beyond them are clamped.
TN256 = [
    (4, 260, 1, 1, "exactA", "plain", False),
    (252, 4, 31, 2, "exactB", "plain", True),
    (256, 256, 32, 1, "exactA", "acc_alpha2", False),
    (260, 252, 33, 2, "exactB", "acc_alpha2", True),
    (252, 256, 64, 3, "exactA", "plain", True),
    (260, 260, 97, 2, "exactA", "alpha_half", False),
    (256, 252, 97, 3, "exactB", "plain", True),
    (4, 4, 64, 9, "exactA", "acc_alpha2", True),
]

# gemm_bf16 (inference epilogue): (M, N, K, block_m, epilogue, destination).  destination: "out+plane", "plane", "planes_col" (hi / lo
# planes into columns [8, 8 + N) of a wider matrix, fp32 out beside it).
B1 = [
    (1, 4, 64, 256, "plain", "out+plane"),
    (193, 260, 128, 256, "bias_resid", "planes_col"),
    (257, 252, 192, 256, "alpha_half", "plane"),
    (320, 256, 64, 256, "gelu", "planes_col"),
    (192, 4, 128, 256, "resid", "out+plane"),
    (129, 132, 128, 128, "bias_resid", "planes_col"),
    (65, 124, 64, 64, "plain", "out+plane"),
    (127, 128, 192, 64, "gelu", "out+plane"),
    (63, 132, 64, 128, "alpha_half", "plane"),
    (320, 260, 128, 256, "resid", "out"),
    (256, 260, 64, 256, "bias_only", "planes_only"),
    (193, 256, 192, 256, "bias_only", "plane"),
]
EPI["gelu"] = dict(bias=True, act=1, tol=True)

# gemm_bf16_train, NT: (M, N, K, block_m, epilogue, destination).  act2 at block_m 256 / 128 / 64 = launch_gemm256_b1_exact,
# launch_exact<128>, launch_exact<64>.  destination: "out", "out+planes" ([M, N], the wrapper's rule), "out+plane".
B1T_NT = [
    (193, 260, 128, 256, "act2", "out+planes"),
    (257, 256, 64, 256, "act2", "out+plane"),
    (129, 132, 128, 128, "act2", "out+planes"),
    (63, 124, 64, 64, "act2", "out"),
    (192, 252, 192, 256, "gelu_z", "out+planes"),
    (384, 4, 64, 256, "drop_resid_b1", "out+plane"),
    (256, 260, 128, 256, "acc_alpha2", "out"),
    (1, 256, 64, 256, "alpha_half", "out+plane"),
    (65, 128, 64, 64, "drop_resid_b1", "out+planes"),
    (127, 132, 192, 128, "gelu_z", "out+plane"),
    (193, 256, 64, 256, "resid_acc", "out"),               # two requests: the general family
]
EPI["gelu_z"] = dict(bias=True, act=1, keep_z=True, tol=True)
EPI["drop_resid_b1"] = dict(bias=True, drop=True, resid=True)

# gemm_bf16_train(trans=True): (M, N, K, block_m, splits, alpha, colsum).  block_m 256 = gemm256_tn_b1 (64-deep K steps of two
# 32-row halves: K <= 32 leaves the whole second half out of range).
B1T_TN = [
    (4, 260, 1, 256, 1, 1.0, False),
    (252, 4, 31, 256, 1, 1.0, True),
    (256, 256, 32, 256, 2, 1.0, False),
    (260, 252, 33, 256, 1, 0.5, False),
    (252, 256, 63, 256, 1, 1.0, True),
    (256, 260, 64, 256, 1, 2.0, False),
    (260, 4, 65, 256, 2, 1.0, True),
    (4, 252, 127, 256, 2, 0.5, False),
    (256, 256, 129, 256, 3, 1.0, True),
    (260, 260, 129, 256, 9, 1.0, False),
    (128, 132, 100, 128, 1, 1.0, True),
    (65, 124, 33, 64, 2, 2.0, False),
]


def all_exact_cases():
    """(class, M, N, K) of every table entry that is compared by torch.equal somewhere."""
    out = set()
    for form, kinds, bm, passes, M, N, K, sp, cls, epi in GENERAL:
        out.add((cls, M, N, K))
    for M, N, K, cls, epi in NT256 + [NT256_TWO_REQUESTS]:
        out.add((cls, M, N, K))
    for M, N, K, sp, cls, epi, cs in TN256:
        out.add((cls, M, N, K))
    for M, N, K, bm, epi, dst in B1 + B1T_NT:
        out.add(("int", M, N, K))
    for M, N, K, bm, sp, alpha, cs in B1T_TN:
        out.add(("int", M, N, K))
    out.add(("exactA", 264, 512, 64))         # the seam case's value ranges at a size the CPU file can afford (K is what matters)
    out.add(("exactA", 132, 128, 100))        # the ragged-K cases
    return sorted(c for c in out if c[0] != "rand")
