"""Case tables, input builders and plain references of the front-end edge suite (test_frontend_edges_cpu.py / test_frontend_edges_gpu.py):
the row gathers and the concat copy, the text and ViT embedding front-ends, the XiT cross-attention pair and the NDCG kernel of
csrc/misc.hip and csrc/attn.hip.  Torch on the CPU only, fp64 wherever arithmetic is involved; nothing here touches a GPU.

Every table is a list of dicts with a unique "id"; TABLES names them all, and test_frontend_edges_cpu.py checks that each one is the
argument list of a parametrised GPU test."""
import math

import numpy as np
import torch

NAN = float("nan")
I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1
GRID_CAP = 4096 * 256        # float4 items one launch of the capped grid-stride kernels covers before its loop wraps


def ids_of(table):
    return [c["id"] for c in table]


def small_ints(gen, *shape, lo=-3, hi=3):
    """Integer-valued fp32 in [lo, hi]: sums and products of a few thousand of them are exact in fp32 in any order."""
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


# ---- row gathers --------------------------------------------------------------------------------------------------------------------
# row_elems: 4 = one float4; 1024 = exactly one workgroup (256 float4); 65536 = exactly the grid cap (64 workgroups x 256 float4);
# 65540 = one trip past it (the grid-stride loop wraps).  form: "tight"; "shared" = src_tstride 0, src_bstride row_elems (one row per
# b, what the shared image features pass: t_in = 1, index None, every j clamps to row 0); "offset" = the view the embedding / engine
# backward pass: base `off` floats into a row of off + t_in * row_elems floats, NaN in the skipped columns.
# index: "repeat" (one t never selected), "same" (one t selected by every j), "none" (index NULL), "oob" (below 0 and >= t_in too).
GATHER = [
    dict(id="one-float4-repeat", B=1, t_in=3, t_out=5, row_elems=4, index="repeat", form="tight"),
    dict(id="one-workgroup-same", B=3, t_in=4, t_out=2, row_elems=1024, index="same", form="tight"),
    dict(id="grid-cap-repeat", B=1, t_in=2, t_out=3, row_elems=65536, index="repeat", form="tight"),
    dict(id="past-cap-identity", B=3, t_in=3, t_out=2, row_elems=65540, index="none", form="tight"),
    dict(id="past-cap-oob", B=1, t_in=2, t_out=4, row_elems=65540, index="oob", form="tight"),
    dict(id="one-workgroup-oob", B=3, t_in=5, t_out=6, row_elems=1024, index="oob", form="tight"),
    dict(id="shared-past-cap", B=3, t_in=1, t_out=4, row_elems=65540, index="none", form="shared"),
    dict(id="shared-one-float4-oob", B=3, t_in=1, t_out=3, row_elems=4, index="oob", form="shared"),
    dict(id="offset-past-cap", B=3, t_in=1, t_out=1, row_elems=65540, index="none", form="offset", off=12),
    dict(id="offset-one-float4", B=1, t_in=1, t_out=1, row_elems=4, index="none", form="offset", off=4),
    dict(id="offset-grid-cap-repeat", B=3, t_in=3, t_out=4, row_elems=65536, index="repeat", form="offset", off=8),
]


def gather_index(case):
    """int64 [B, t_out] or None."""
    B, t_in, t_out = case["B"], case["t_in"], case["t_out"]
    kind = case["index"]
    if kind == "none":
        return None
    if kind == "same":
        return torch.full((B, t_out), t_in - 2 if t_in > 1 else 0, dtype=torch.int64)
    gen = torch.Generator().manual_seed(1000 + B * 100 + t_in * 10 + t_out)
    if kind == "repeat":                                  # t = t_in - 2 (or 0 when t_in < 3 ... then t_in - 1) is never selected
        skip = t_in - 2 if t_in >= 3 else t_in - 1
        allowed = torch.tensor([t for t in range(t_in) if t != skip], dtype=torch.int64)
        idx = allowed[torch.randint(0, allowed.numel(), (B, t_out), generator=gen)]
        idx[:, 0] = idx[:, -1] = allowed[0]               # at least one repeat in every b
        return idx
    assert kind == "oob"
    idx = torch.randint(-3, t_in + 3, (B, t_out), generator=gen)
    idx[0, 0], idx[0, 1], idx[-1, -1] = -1, t_in, I64_MAX
    if t_out > 2:
        idx[0, 2] = I64_MIN
    return idx


def gather_clamped(case, index):
    """The row each (b, j) reads: the kernels' documented clamp of the index into [0, t_in - 1]; index None = j."""
    B, t_in, t_out = case["B"], case["t_in"], case["t_out"]
    if index is None:
        index = torch.arange(t_out, dtype=torch.int64).expand(B, t_out)
    return index.clamp(0, t_in - 1)


def gather_source(case, x):
    """x: logical fp32 [B, t_in, row_elems] -> (buffer, element offset of the base, src_bstride, src_tstride) in the case's stride form."""
    B, t_in, re = case["B"], case["t_in"], case["row_elems"]
    form = case["form"]
    if form == "tight":
        return x.contiguous().view(-1), 0, t_in * re, re
    if form == "shared":
        assert t_in == 1
        return x.contiguous().view(-1), 0, re, 0
    off = case["off"]
    width = off + t_in * re + 4                           # 4 NaN columns behind the rows as well
    buf = torch.full((B, width), NAN)
    buf[:, off:off + t_in * re] = x.reshape(B, t_in * re)
    return buf.view(-1), off, width, re


def gather_fwd_ref(x, clamped):
    B, t_out = clamped.shape
    return torch.stack([x[b, clamped[b]] for b in range(B)])


def gather_bwd_ref(y, clamped, t_in):
    """fp64 index_add of y [B, t_out, row_elems] over the clamped index -> [B, t_in, row_elems]."""
    B, t_out, re = y.shape
    out = torch.zeros(B, t_in, re, dtype=torch.float64)
    for b in range(B):
        out[b].index_add_(0, clamped[b], y[b].double())
    return out


# ---- copy_rows ----------------------------------------------------------------------------------------------------------------------
# dst[(r / group) * gstride + (r % group) * D + off + c] = src[r * D + c]; rows is no multiple of group (the last group is partial),
# gstride > group * D + off (canaries in the gaps).  "big": rows * D / 4 = 1 049 856, just above the 4096-workgroup cap.
COPY = [
    dict(id="group1-f32", rows=5, D=8, group=1, gstride=20, off=4, planes=False),
    dict(id="group1-planes", rows=5, D=8, group=1, gstride=20, off=4, planes=True),
    dict(id="group2-f32", rows=7, D=12, group=2, gstride=36, off=4, planes=False),
    dict(id="group2-planes", rows=7, D=12, group=2, gstride=36, off=4, planes=True),
    dict(id="group3-f32", rows=10, D=4, group=3, gstride=24, off=8, planes=False),
    dict(id="group3-planes", rows=10, D=4, group=3, gstride=24, off=8, planes=True),
    dict(id="past-cap-f32", rows=1367, D=3072, group=2, gstride=2 * 3072 + 12, off=4, planes=False),
    dict(id="past-cap-planes", rows=1367, D=3072, group=2, gstride=2 * 3072 + 12, off=4, planes=True),
]


def copy_dst_index(case):
    """[rows, D] destination element offsets, and the number of elements the destination spans."""
    rows, D, group, gs, off = case["rows"], case["D"], case["group"], case["gstride"], case["off"]
    r = torch.arange(rows)
    base = (r // group) * gs + (r % group) * D + off
    return base[:, None] + torch.arange(D)[None, :], ((rows + group - 1) // group) * gs


# ---- text_embed ---------------------------------------------------------------------------------------------------------------------
# rows * D / 4 = 1, 255, 256, 257: the workgroup edges; 5462 x 768 = 1 048 704 float4, just above the cap.  L never divides 256.
# bad: {row: (token id or None, segment id or None)} out-of-range ids.  With D = 4 a row is one float4, so rows 3 and 280 have their
# column-0 element in workgroups 0 and 1; with D = 36 (9 float4 per row) rows 2, 40 and 60 have it in workgroups 0, 1 and 2.
TEXT_EMBED = [
    dict(id="1-float4", rows=1, L=1, D=4, bad={}),
    dict(id="255-float4", rows=255, L=7, D=4, bad={}),
    dict(id="256-float4", rows=256, L=7, D=4, bad={}),
    dict(id="257-float4", rows=257, L=7, D=4, bad={}),
    dict(id="d36", rows=5, L=3, D=36, bad={}),
    dict(id="past-cap-d768", rows=5462, L=197, D=768, bad={}),
    dict(id="bad-token", rows=300, L=7, D=4, bad={280: (-1, None)}),
    dict(id="bad-segment", rows=300, L=7, D=4, bad={3: (None, 3)}),
    dict(id="bad-both-two-workgroups", rows=300, L=7, D=4, bad={3: (50, None), 280: (None, -1)}),
    dict(id="bad-both-one-row", rows=64, L=5, D=36, bad={40: (2 ** 40, 2 ** 33)}),
    dict(id="bad-three-workgroups", rows=64, L=5, D=36, bad={2: (-7, None), 40: (I64_MIN, 7), 60: (I64_MAX, None)}),
]
TE_VOCAB, TE_NSEG = 50, 3


def text_embed_inputs(case):
    """ids, seg (as the kernel gets them), the tables, and (ids, seg) with every out-of-range id replaced by 0 (the documented row-0
    substitution).  Table rows that no (substituted) id selects are NaN, and so are the position rows past L."""
    rows, L, D = case["rows"], case["L"], case["D"]
    gen = torch.Generator().manual_seed(rows * 31 + D)
    ids = torch.randint(1, TE_VOCAB, (rows,), generator=gen)
    ids[ids % 5 == 3] = 7                                   # a repeated token; ids = 3 mod 5 are absent
    seg = torch.randint(0, 2, (rows,), generator=gen)      # segment 2 is absent
    ids_ok, seg_ok = ids.clone(), seg.clone()
    for r, (t, s) in case["bad"].items():
        if t is not None:
            ids[r], ids_ok[r] = t, 0
        if s is not None:
            seg[r], seg_ok[r] = s, 0
    word = torch.randn(TE_VOCAB, D, generator=gen)
    pos = torch.randn(L + 2, D, generator=gen)
    seg_table = torch.randn(TE_NSEG, D, generator=gen)
    absent = torch.ones(TE_VOCAB, dtype=torch.bool)
    absent[ids_ok] = False
    word[absent] = NAN
    pos[L:] = NAN
    absent = torch.ones(TE_NSEG, dtype=torch.bool)
    absent[seg_ok] = False
    seg_table[absent] = NAN
    return ids, seg, word, pos, seg_table, ids_ok, seg_ok


def text_embed_ref(ids_ok, seg_ok, word, pos, seg_table, L):
    """The fp32 expression the kernel documents: (word + pos) + seg."""
    r = torch.arange(ids_ok.numel())
    return (word[ids_ok] + pos[r % L]) + seg_table[seg_ok]


def text_embed_err(case):
    return (1 if any(t is not None for t, _ in case["bad"].values()) else 0) | \
           (2 if any(s is not None for _, s in case["bad"].values()) else 0)


# ---- text_embed_bwd -----------------------------------------------------------------------------------------------------------------
# Word table.  The ids are built in sorted-position terms: "bounds" are the sorted positions where a new token starts, the last one is
# `rows`; run i carries token 2 i + 1, so every even table row is absent and must keep its pre-fill.  "toks" overrides the tokens
# (out-of-range ones included; they must stay sorted).  Pieces are cut at multiples of 256 sorted positions; chunk c's partial slots
# are 2c (a piece that starts the chunk inside a run) and 2c + 1 (the piece holding a run's start).  shuffle: the rows are permuted, so
# `order` is no identity.
def _wb(id, bounds, toks=None, D=8, shuffle=False):
    return dict(id=id, bounds=bounds, toks=toks, D=D, shuffle=shuffle)


EMBED_BWD_WORD = [
    _wb("rows1", [0, 1]),
    _wb("rows255", [0, 100, 255]),
    _wb("rows256-one-run", [0, 256]),                     # one piece, ends at the last position, rows % 256 == 0: written directly
    _wb("rows257-one-run", [0, 257]),                     # slot 1 + slot 2
    _wb("rows512", [0, 3, 512], shuffle=True),            # run 3..512: slot 1, slot 2; ends at the last position, rows % 256 == 0
    _wb("rows513-one-run", [0, 513]),                     # slots 1, 2, 4
    _wb("run256-then-other", [0, 256, 300]),              # a run of exactly 256 from 0 (direct), then another token starting chunk 1
    _wb("from255-to256", [0, 255, 256, 261]),             # a run of one row at 255
    _wb("from255-to257", [0, 255, 257, 262]),             # slot 1, slot 2
    _wb("from255-to511", [0, 255, 511, 516]),
    _wb("from255-to512", [0, 255, 512, 517]),             # the continuation piece fills chunk 1 exactly
    _wb("from255-to513", [0, 255, 513, 518]),             # slots 1, 2, 4
    _wb("from255-to769", [0, 255, 769, 774], shuffle=True),   # slots 1, 2, 4, 6
    _wb("from255-to-end512", [0, 255, 512]),              # ... ending at the last position, rows % 256 == 0
    _wb("from300-to-end768", [0, 300, 768]),              # starts inside chunk 1 (slot 3), slot 4; ends at the last position
    _wb("from256-across512", [0, 256, 600, 610]),         # a run starting exactly at 256: its first piece is a run start, slot 3, then 4
    _wb("two-crossings", [0, 200, 300, 500, 600, 700], D=1028, shuffle=True),   # slots 1 + 2 and 3 + 4 live at once; the column loop
    _wb("whole-input-3-chunks", [0, 700]),                # slots 1, 2, 4
    # out-of-range runs (dropped; no table row written) with valid runs next to them: the negative ones sort first, those >= vocab last
    _wb("oob-runs", [0, 10, 310, 560, 590, 880, 885], toks=[-3, -2, 1, 5, "vocab", "vocab+1"], shuffle=True),
]
# Segment table: 64 rows per workgroup; ids >= n_seg and negative ones are dropped.
EMBED_BWD_SEG = [dict(id=f"rows{r}-nseg{n}", rows=r, n_seg=n) for r, n in ((1, 1), (63, 2), (64, 3), (65, 4), (129, 3), (129, 1))]
EMBED_BWD_RANDOM = [dict(id="n01-rows1500-run700", rows=1500, run=700, D=16)]


def embed_bwd_word_ids(case):
    """-> (ids int64 [rows] in ROW order, vocab)."""
    bounds = case["bounds"]
    n_runs = len(bounds) - 1
    vocab = 2 * n_runs + 2
    toks = case["toks"] or [2 * i + 1 for i in range(n_runs)]
    toks = [vocab if t == "vocab" else vocab + 1 if t == "vocab+1" else t for t in toks]
    assert toks == sorted(toks) and len(set(toks)) == n_runs
    ids = torch.cat([torch.full((bounds[i + 1] - bounds[i],), toks[i], dtype=torch.int64) for i in range(n_runs)])
    if case["shuffle"]:
        ids = ids[torch.randperm(ids.numel(), generator=torch.Generator().manual_seed(ids.numel()))]
    return ids, vocab


def embed_bwd_seg_ids(rows, n_seg):
    seg = (torch.arange(rows) * 7 + 1) % n_seg
    if rows >= 63:
        seg[5], seg[17], seg[rows - 1], seg[rows // 2] = n_seg, -1, 7, 4
    return seg


def index_add_ref(dx, ids, n_rows):
    """fp64 sum of the rows of dx per id; ids outside [0, n_rows) are dropped.  -> (sums fp64 [n_rows, D], present bool [n_rows])."""
    ok = (ids >= 0) & (ids < n_rows)
    out = torch.zeros(n_rows, dx.shape[1], dtype=torch.float64)
    out.index_add_(0, ids[ok], dx[ok].double())
    present = torch.zeros(n_rows, dtype=torch.bool)
    present[ids[ok]] = True
    return out, present


def seq_sum_bound(dx, ids, n_rows):
    """n * 2^-24 * sum |dx_i| per element over the rows summed into it: the standard bound of a sequential fp32 sum of n terms (each of
    the n - 1 additions is off by at most 2^-24 of a partial sum that never exceeds sum |dx_i|); any fixed summation order obeys it."""
    ok = (ids >= 0) & (ids < n_rows)
    sabs = torch.zeros(n_rows, dx.shape[1], dtype=torch.float64)
    sabs.index_add_(0, ids[ok], dx[ok].double().abs())
    n = torch.bincount(ids[ok], minlength=n_rows).double()
    return n[:, None] * 2.0 ** -24 * sabs


# ---- patchify -----------------------------------------------------------------------------------------------------------------------
# kernel: what lr2_patchify_planes dispatches to -- "strip" (ps == 16, ld == Kd, lo_off % 4 == 0), else "vec4" (ps % 4 == 0 and
# lo_off % 4 == 0), else "vec2".  pad: ld = Kd rounded up to a multiple of 64, or Kd + pad.  lo2: the lo plane starts 2 (mod 4)
# elements behind the hi plane.  src: "u8n" uint8 + CLIP normalisation, "u8" uint8 / 255 only, "f32".  all256: every byte value in
# every channel.  per_strip = (W / 16) * C * 16 triples per strip of the strip kernel: 48, 240, 288, 672 at C = 3.
def _pp(id, kernel, ps, C, H, W, B=2, src="u8n", pad=0, lo2=False, all256=False):
    return dict(id=id, kernel=kernel, ps=ps, C=C, H=H, W=W, B=B, src=src, pad=pad, lo2=lo2, all256=all256)


PATCHIFY_PLANES = [
    _pp("strip-w16", "strip", 16, 3, 32, 16),             # per_strip 48: one partial trip
    _pp("strip-w80", "strip", 16, 3, 32, 80),             # 240: just below one full trip
    _pp("strip-w96", "strip", 16, 3, 32, 96),             # 288: two trips
    _pp("strip-w224", "strip", 16, 3, 32, 224),           # 672: three trips (production width)
    _pp("strip-c1", "strip", 16, 1, 32, 80),
    _pp("strip-c2", "strip", 16, 2, 32, 96),
    _pp("strip-u8-raw", "strip", 16, 3, 32, 96, src="u8"),
    _pp("strip-f32", "strip", 16, 3, 32, 96, src="f32"),
    _pp("strip-all256", "strip", 16, 3, 32, 16, B=1, all256=True),
    _pp("ps16-padded", "vec4", 16, 3, 32, 48, pad=64),    # ld = Kd + 64
    _pp("ps16-lo2", "vec2", 16, 3, 32, 48, lo2=True),     # lo_off = 2 (mod 4)
    _pp("ps4", "vec4", 4, 3, 8, 12),
    _pp("ps8", "vec4", 8, 3, 16, 24),
    _pp("ps8-c1", "vec4", 8, 1, 16, 24),
    _pp("ps8-c2-f32", "vec4", 8, 2, 16, 24, src="f32"),
    _pp("ps8-all256", "vec4", 8, 3, 16, 32, B=1, all256=True),
    _pp("ps6-padded", "vec2", 6, 3, 12, 18, pad="64"),    # Kd 108 -> ld 128
    _pp("ps14-padded", "vec2", 14, 3, 28, 42, pad="64"),  # Kd 588 -> ld 640
    _pp("ps14-u8-raw-c2", "vec2", 14, 2, 28, 14, src="u8", pad="64"),
    _pp("ps8-past-cap", "vec4", 8, 3, 848, 848, B=2),     # B * P * ld / 4 = 22472 * 48 = 1 078 656 > 1 048 576
]
PATCHIFY = [
    dict(id="ps2", B=1, C=1, H=4, W=6, ps=2),
    dict(id="ps7", B=2, C=3, H=14, W=28, ps=7),
    dict(id="ps16", B=2, C=2, H=32, W=16, ps=16),
]
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def patchify_ld(case):
    Kd = case["C"] * case["ps"] ** 2
    return (Kd + 63) // 64 * 64 if case["pad"] == "64" else Kd + case["pad"]


def patchify_kernel(case):
    """The dispatch of lr2_patchify_planes, restated."""
    Kd = case["C"] * case["ps"] ** 2
    lo_ok = not case["lo2"]
    if case["ps"] == 16 and patchify_ld(case) == Kd and lo_ok:
        return "strip"
    return "vec4" if case["ps"] % 4 == 0 and lo_ok else "vec2"


def patchify_image(case):
    """-> (img as the kernel gets it (uint8 or fp32 [B, C, H, W]), the fp32 pixels the patch rows must hold)."""
    B, C, H, W = case["B"], case["C"], case["H"], case["W"]
    gen = torch.Generator().manual_seed(H * W + C)
    if case["src"] == "f32":
        img = torch.randn(B, C, H, W, generator=gen)
        return img, img
    if case["all256"]:
        assert H * W >= 256
        img = ((torch.arange(H * W).view(1, 1, H, W) + 37 * torch.arange(C).view(1, C, 1, 1)) % 256).to(torch.uint8).expand(B, C, H, W).contiguous()
    else:
        img = torch.randint(0, 256, (B, C, H, W), generator=gen).to(torch.uint8)
    x = img.float().div(255)
    if case["src"] == "u8n":                               # the loader's expression (x.float().div(255), then Normalize)
        x = x.sub(torch.tensor(CLIP_MEAN[:C]).view(1, C, 1, 1)).div(torch.tensor(CLIP_STD[:C]).view(1, C, 1, 1))
    return img, x


def patch_rows(x, ps, ld=None):
    """[B, C, H, W] -> [B * P, ld] patch rows (columns past C ps ps are zeros)."""
    B, C, H, W = x.shape
    Kd = C * ps * ps
    rows = x.view(B, C, H // ps, ps, W // ps, ps).permute(0, 2, 4, 1, 3, 5).reshape(-1, Kd)
    if ld is None or ld == Kd:
        return rows.contiguous()
    out = torch.zeros(rows.shape[0], ld)
    out[:, :Kd] = rows
    return out


# ---- vit_assemble -------------------------------------------------------------------------------------------------------------------
VIT_ASSEMBLE = [
    dict(id="b1-p1-d4", B=1, P=1, D=4),
    dict(id="b3-p196-d4", B=3, P=196, D=4),
    dict(id="b1-p1-d768", B=1, P=1, D=768),
    dict(id="b3-p196-d768", B=3, P=196, D=768),
    dict(id="past-cap", B=28, P=196, D=768),               # 28 * 197 * 192 = 1 059 072 float4 > 1 048 576
]


# ---- XiT cross-attention ------------------------------------------------------------------------------------------------------------
# Every Lk of {1, 2, 15, 16}, Lq of {1, 2, 3, 255, 256}, hd of {4, 64, 92, 96}, heads of {1, 3}, batch of {1, 2}, the corners
# (Lq, Lk) = (1, 1), (1, 16), (256, 1), (256, 16), (3, 15), and Lk = 4, 8 for the uniform class.
def _xs(batch, heads, Lq, Lk, hd):
    return dict(id=f"b{batch}-h{heads}-q{Lq}-k{Lk}-d{hd}", batch=batch, heads=heads, Lq=Lq, Lk=Lk, hd=hd)


XATTN_SHAPES = [_xs(1, 1, 1, 1, 4), _xs(2, 3, 1, 16, 96), _xs(1, 3, 256, 1, 64), _xs(2, 1, 256, 16, 92), _xs(2, 3, 3, 15, 96),
                _xs(1, 3, 2, 2, 64), _xs(2, 3, 255, 16, 4), _xs(2, 3, 256, 16, 96), _xs(1, 3, 3, 4, 92), _xs(2, 1, 255, 8, 64)]
XATTN_ONEHOT = [dict(c, cls="onehot") for c in XATTN_SHAPES]
XATTN_UNIFORM = [dict(c, cls="uniform") for c in XATTN_SHAPES if c["Lk"] in (1, 2, 4, 8, 16)]
XATTN_RANDOM = [dict(c, cls="random") for c in XATTN_SHAPES]
XATTN_LARGE = [dict(c, cls="large") for c in XATTN_SHAPES if c["hd"] == 96 and c["Lk"] > 1]
XATTN_PLANES = [dict(c, cls="random") for c in XATTN_SHAPES if (c["Lq"], c["Lk"]) in ((1, 1), (3, 15), (256, 16), (256, 1))]
ONEHOT_LEAD = 200            # the best key's score leads by at least this much: exp(-200) = 2^-288 is 0 in fp32, through exp2 as well


def xattn_post_scale(case):
    """1 / sqrt(E) for the random classes (the product's value); a power of two for the exact classes."""
    return 2.0 ** -4 if case["cls"] in ("onehot", "uniform") else 1.0 / math.sqrt(case["heads"] * case["hd"])


def xattn_inputs(case):
    """q, do [batch, Lq, E]; k, v [batch, Lk, E] fp32; data differs per head and per sequence in every class."""
    batch, heads, Lq, Lk, hd = (case[n] for n in ("batch", "heads", "Lq", "Lk", "hd"))
    E = heads * hd
    gen = torch.Generator().manual_seed(7 + batch * 1000 + heads * 100 + Lq * 10 + Lk + hd)
    cls = case["cls"]
    if cls == "random":                                     # the scales of test_kernels_gpu.py::test_xattn_fwd_bwd
        return (torch.randn(batch, Lq, E, generator=gen) * 0.5, torch.randn(batch, Lk, E, generator=gen) * 0.5,
                torch.randn(batch, Lk, E, generator=gen), torch.randn(batch, Lq, E, generator=gen))
    if cls == "large":                                      # unit inputs, no pre-scale: |S| reaches several sqrt(hd)
        return tuple(torch.randn(batch, n, E, generator=gen) for n in (Lq, Lk, Lk, Lq))
    v, do = small_ints(gen, batch, Lk, E, lo=-2, hi=2), small_ints(gen, batch, Lq, E, lo=-2, hi=2)
    if cls == "uniform":                                    # Q = 0: every score 0, p = 1 / Lk
        return torch.zeros(batch, Lq, E), small_ints(gen, batch, Lk, E, lo=-2, hi=2), v, do
    # one-hot: per (b, h) the query t prefers key w = (t + b + 2 h) % Lk.  K_j = (2 j M, -j^2 M, c_2, c_3, ...) with constants c_d per
    # (b, h), Q_t = (w, 1, small integers): S_tj = M (w^2 - (j - w)^2) + const_t, the winner leads by M = ONEHOT_LEAD at least.
    assert cls == "onehot"
    q = small_ints(gen, batch, Lq, heads, hd)
    k = small_ints(gen, batch, 1, heads, hd).expand(batch, Lk, heads, hd).clone()
    j = torch.arange(Lk).float()
    k[:, :, :, 0] = (2 * ONEHOT_LEAD * j).view(1, Lk, 1)
    k[:, :, :, 1] = (-ONEHOT_LEAD * j * j).view(1, Lk, 1)
    q[:, :, :, 0] = xattn_onehot_winner(case).permute(0, 2, 1).float()
    q[:, :, :, 1] = 1.0
    return q.reshape(batch, Lq, E), k.reshape(batch, Lk, E), v, do


def xattn_onehot_winner(case):
    """int64 [batch, heads, Lq]."""
    batch, heads, Lq, Lk = (case[n] for n in ("batch", "heads", "Lq", "Lk"))
    t, b, h = torch.arange(Lq).view(1, 1, Lq), torch.arange(batch).view(batch, 1, 1), torch.arange(heads).view(1, heads, 1)
    return (t + b + 2 * h) % Lk


def _heads(x, heads):
    b, n, e = x.shape
    return x.view(b, n, heads, e // heads).permute(0, 2, 1, 3)


def _unheads(x):
    b, h, n, d = x.shape
    return x.permute(0, 2, 1, 3).reshape(b, n, h * d)


def xattn_formula(q, k, v, do, heads, post_scale, dtype):
    """The kernels' formulas (csrc/attn.hip) evaluated in `dtype`: S = Q K^T, p = softmax(S), O = (c p) V; dPs = c (dO . V),
    dS = p (dPs - sum p dPs), dQ = dS K, dK = dS^T Q, dV = (c p)^T dO.  -> O, dQ, dK, dV as [batch, L, E]."""
    qh, kh, vh, gh = (_heads(t.to(dtype), heads) for t in (q, k, v, do))
    s = qh @ kh.transpose(-1, -2)
    e = torch.exp(s - s.max(dim=-1, keepdim=True).values)
    p = e / e.sum(dim=-1, keepdim=True)
    c = torch.tensor(post_scale, dtype=dtype)
    o = (p * c) @ vh
    dp = (gh @ vh.transpose(-1, -2)) * c
    ds = p * (dp - (p * dp).sum(dim=-1, keepdim=True))
    return _unheads(o), _unheads(ds @ kh), _unheads(ds.transpose(-1, -2) @ qh), _unheads((p * c).transpose(-1, -2) @ gh)


def xattn_autograd(q, k, v, do, heads, post_scale):
    """fp64 autograd of softmax(Q K^T) * post_scale @ V: the reference of the random classes."""
    qt, kt, vt = (t.double().requires_grad_(True) for t in (q, k, v))
    att = torch.softmax(_heads(qt, heads) @ _heads(kt, heads).transpose(-1, -2), dim=-1) * post_scale
    o = _unheads(att @ _heads(vt, heads))
    o.backward(do.double())
    return o.detach(), qt.grad, kt.grad, vt.grad


def xattn_onehot_expected(case, v, do, post_scale):
    """O = c V[winner], dQ = 0, dK = 0, dV[j] = c sum of dO over the queries that chose j (fp64; exact in fp32 for these inputs)."""
    batch, heads, Lq, Lk, hd = (case[n] for n in ("batch", "heads", "Lq", "Lk", "hd"))
    w = xattn_onehot_winner(case)                                                   # [b, h, Lq]
    vh, gh = _heads(v.double(), heads), _heads(do.double(), heads)                  # [b, h, L, d]
    o = post_scale * torch.gather(vh, 2, w[..., None].expand(batch, heads, Lq, hd))
    dv = torch.zeros_like(vh)
    dv.scatter_add_(2, w[..., None].expand(batch, heads, Lq, hd), post_scale * gh)
    E = heads * hd
    return _unheads(o), torch.zeros(batch, Lq, E, dtype=torch.float64), torch.zeros(batch, Lk, E, dtype=torch.float64), _unheads(dv)


# ---- NDCG ---------------------------------------------------------------------------------------------------------------------------
NDCG_KS = (1, 5, 20, 63, 64, 100, 10 ** 8)                # 1; equal to T for the items of 1, 5, 20, 63, 64; above every T; 10^8
# items: n_items ragged items whose sizes cycle through `sizes`; special: {item: kind} -- "t0" (an empty item), "t65" (too long: NaN),
# "label62" (finite), "label63" / "label-1" (NaN), "equal" (all scores equal, one label), "ties" (tied scores, different labels).
NDCG = [
    dict(id="one-item-of-1", n_items=1, sizes=(1,), special={}),
    dict(id="63-items", n_items=63, sizes=(1, 63, 64, 5, 20), special={3: "t0", 10: "label62", 62: "equal"}),
    dict(id="64-items", n_items=64, sizes=(64, 1, 20, 63), special={0: "t65", 63: "label63", 30: "ties"}),
    dict(id="65-items", n_items=65, sizes=(5, 64, 63, 1), special={63: "t0", 64: "label-1", 1: "label62"}),
    dict(id="129-items", n_items=129, sizes=(20, 1, 64, 63, 7), special={64: "t65", 65: "t0", 128: "ties", 127: "equal", 0: "label62"}),
]


def ndcg_items(case):
    """-> list of (scores fp32 [T], gold int64 [T], kind)."""
    gen = torch.Generator().manual_seed(case["n_items"])
    items = []
    for i in range(case["n_items"]):
        kind = case["special"].get(i, "")
        T = {"t0": 0, "t65": 65}.get(kind, case["sizes"][i % len(case["sizes"])])
        if kind in ("ties", "equal") and T < 5:
            T = 5
        s = torch.randn(T, generator=gen)                  # distinct with probability 1 (asserted below)
        g = torch.randint(0, 5, (T,), generator=gen)
        if kind == "label62":
            g[T // 2] = 62
        elif kind == "label63":
            g[T - 1] = 63
        elif kind == "label-1":
            g[0] = -1
        elif kind == "equal":
            s, g = torch.full((T,), 0.25), torch.full((T,), 2, dtype=torch.int64)
        elif kind == "ties":                               # groups of tied scores whose labels differ
            s = torch.tensor([1.0, 1.0, 0.5, 1.0, 0.5] + [0.5] * (T - 5))
            g = torch.tensor([0, 3, 1, 4, 2] + [i % 5 for i in range(T - 5)])
        else:
            assert s.unique().numel() == T
        items.append((s, g, kind))
    return items


def ndcg_ref(scores, gold, ks):
    """The kernel's documented rule in sequential fp32: stable sort by score descending (earlier index first on ties), ideal = labels
    sorted descending, gain 2^rel - 1, discount log2(i + 2) from the same fp32 table, NDCG = 1 when the ideal DCG <= 1e-6.  An item of
    more than 64 elements or with a label outside [0, 62] is a row of NaN."""
    T = scores.numel()
    if T > 64 or bool(((gold < 0) | (gold > 62)).any()):
        return torch.full((len(ks),), NAN)
    disc = torch.log2(torch.arange(64, dtype=torch.int64) + 2).numpy()
    order = sorted(range(T), key=lambda i: (-float(scores[i]), i))
    by_score = [int(gold[i]) for i in order]
    ideal = sorted((int(x) for x in gold), reverse=True)
    out = []
    for k in ks:
        pred, tru = np.float32(0), np.float32(0)
        for i in range(min(k, T)):
            pred = np.float32(pred + np.float32(np.float32(2 ** by_score[i] - 1) / disc[i]))
            tru = np.float32(tru + np.float32(np.float32(2 ** ideal[i] - 1) / disc[i]))
        out.append(1.0 if tru <= np.float32(1e-6) else float(np.float32(pred / tru)))
    return torch.tensor(out, dtype=torch.float32)


def ndcg_meter_applies(kind, T):
    """The host meter needs one element at least, labels it can shift by, and -- its torch.sort is not stable -- no tie between
    elements of different labels."""
    return T >= 1 and kind in ("", "label62", "equal")


TABLES = dict(GATHER=GATHER, COPY=COPY, TEXT_EMBED=TEXT_EMBED, EMBED_BWD_WORD=EMBED_BWD_WORD, EMBED_BWD_SEG=EMBED_BWD_SEG,
              EMBED_BWD_RANDOM=EMBED_BWD_RANDOM, PATCHIFY_PLANES=PATCHIFY_PLANES, PATCHIFY=PATCHIFY, VIT_ASSEMBLE=VIT_ASSEMBLE,
              XATTN_ONEHOT=XATTN_ONEHOT, XATTN_UNIFORM=XATTN_UNIFORM, XATTN_RANDOM=XATTN_RANDOM, XATTN_LARGE=XATTN_LARGE,
              XATTN_PLANES=XATTN_PLANES, NDCG=NDCG)
