"""Case table of the wide XiT cross-attention pair (csrc/attn_wide.hip: 1 <= Lk <= 64, key blocks of 16), shared by
test_xattn_wide_cpu.py (which proves the exact classes exact on these shapes and holds the argument contract) and test_xattn_wide_gpu.py.
The input builders, the references and the class rules are those of tests/frontend_cases.py; only the shapes are new."""
import frontend_cases as FC

KEY_BLOCK = 16           # keys per block of the wide kernels
MAX_LK = 64


def _xs(batch, heads, Lq, Lk, hd):
    return FC._xs(batch, heads, Lq, Lk, hd)


# (batch, heads, Lq, Lk, head_dim): every Lk of {17, 31, 32, 33, 47, 48, 49, 63, 64} -- one key past, one short of and exactly on every
# block seam above 16 --, Lq of {1, 2, 3, 5, 7, 196, 255, 256}, head_dim of {4, 64, 92, 96}, heads of {1, 3, 8}, batch of {1, 2}, the
# corners (1, 17) and (256, 64), and the PPO shape's (196, 32, 8 heads of 96).
WIDE_SHAPES = [_xs(1, 1, 1, 17, 4), _xs(2, 3, 3, 31, 96), _xs(2, 3, 256, 32, 96), _xs(1, 3, 255, 33, 64), _xs(2, 1, 256, 48, 92),
               _xs(2, 3, 256, 64, 96), _xs(1, 3, 2, 64, 64), _xs(1, 8, 196, 32, 96), _xs(2, 1, 5, 47, 4), _xs(1, 3, 7, 49, 64),
               _xs(1, 1, 3, 63, 92)]
# the wide form forced at sizes the 16-key pair serves: one key, one short of a block, a whole block
NARROW_SHAPES = [_xs(1, 1, 1, 1, 4), _xs(2, 3, 3, 15, 96), _xs(2, 3, 256, 16, 96)]
ALL_SHAPES = WIDE_SHAPES + NARROW_SHAPES

XATTN_ONEHOT = [dict(c, cls="onehot") for c in ALL_SHAPES]
XATTN_UNIFORM = [dict(c, cls="uniform") for c in ALL_SHAPES if c["Lk"] in (1, 16, 32, 64)]      # Lk a power of two: p = 1 / Lk exact
XATTN_RANDOM = [dict(c, cls="random") for c in ALL_SHAPES]
XATTN_LARGE = [dict(c, cls="large") for c in ALL_SHAPES if c["hd"] in (92, 96) and c["Lk"] > 1]
XATTN_PLANES = [dict(c, cls="random") for c in ALL_SHAPES if (c["Lq"], c["Lk"]) in ((1, 17), (3, 31), (196, 32), (256, 64), (3, 15))]
XATTN_DETERMINISM = [dict(c, cls="random") for c in ALL_SHAPES if (c["Lq"], c["Lk"]) in ((255, 33), (256, 64))]

TABLES = dict(XATTN_ONEHOT=XATTN_ONEHOT, XATTN_UNIFORM=XATTN_UNIFORM, XATTN_RANDOM=XATTN_RANDOM, XATTN_LARGE=XATTN_LARGE,
              XATTN_PLANES=XATTN_PLANES, XATTN_DETERMINISM=XATTN_DETERMINISM)


def is_wide_only(case):
    """True for the cases the 16-key pair refuses: they fail without the wide kernels."""
    return case["Lk"] > KEY_BLOCK


_INPUTS = {}


def inputs(case):
    """FC.xattn_inputs(case), built once per (class, shape) and shared by the tests that need it (never modified)."""
    key = (case["cls"], case["id"])
    if key not in _INPUTS:
        _INPUTS[key] = FC.xattn_inputs(case)
    return _INPUTS[key]
