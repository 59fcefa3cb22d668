"""Direct references for the pointwise kernels every training step runs but no test called on their own (csrc/misc.hip and
lr2_dropout_residual of csrc/fp8_train.hip): the dropout family bit for bit against the mask of oracle.dropout_keep_mask and fp32
arithmetic restated with numpy (the kernels pin contraction off), lr2_split_planes_multi against lr2_split_planes with canaries around
every chunk, and the mode='cls' chain (head forward / backward, expected-label scores, NLL) against fp64 at the edges of their loops.
Every output element is compared; nothing is skipped or masked out."""
import itertools

import numpy as np
import pytest
import torch

from oracle import lr2ppo_oracle as O

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # unit roundoff of fp32


@pytest.fixture(scope="module")
def ops(dev):
    from lr2ppo_amd import ops as _ops
    return _ops


# ------------------------------------------------------------------------------------------- dropout family
# zeros, fp32 subnormals, +-65504, the smallest normal, values whose bf16 lo plane is subnormal (x = 2^-120 (1 + 2^-10): hi = 2^-120,
# lo = 2^-130 < 2^-126), a value that rounds up into the next bf16 binade, and magnitudes up to 1e30: times the largest scale here
# (1 / (1 - 0.99999) ~ 1e5) still far below the largest finite bf16 (3.3895e38), beyond which hi would round to infinity
_SPECIAL = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 5.8e-39, -1.1e-38, 65504.0, -65504.0, 1.17549435e-38, -1.17549435e-38,
                     2.0 ** -120 * (1 + 2.0 ** -10), -(2.0 ** -120) * (1 + 2.0 ** -10), 2.0 ** -125 * (1 + 2.0 ** -9), 2.0 ** -126 * 1.5,
                     1.99999988, -1.99999988, 1.00390625, 1.0078125, 1e30, -1e30, 3.0e-5, -7.0, 1.0, -1.0, 0.333333343, 255.998],
                    dtype=np.float32)
_NS = [4, 1020, 1024, 4 * 1024 * 1024 + 4]          # the last: one float4 past the 4096-block x 256-thread grid cap (a second trip)
_PS = [1e-5, 0.1, 0.5, 0.99999]                     # thresholds 0 (all kept, still scaled), 6553, 32768, 65535 (capped)
_SEEDS = [0, 1234, 2 ** 64 - 1]
_SITES = [0, 7, 65535, 2 ** 24 - 1]


def _keys(n, p):
    """(seed, site) pairs of one (n, p) case: the whole product at the small sizes; at the 4M-element size one pair per p, which
    over the four p still visits every seed and every site"""
    if n < 1 << 20:
        return list(itertools.product(_SEEDS, _SITES))
    return [list(zip(_SEEDS + [1234], _SITES))[_PS.index(p)]]


def _data(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g) * torch.exp(torch.randn(n, generator=g) * 3)
    k = min(n, len(_SPECIAL))
    x[:k] = torch.from_numpy(_SPECIAL[:k])
    if n > 2 * len(_SPECIAL):
        x[-len(_SPECIAL):] = torch.from_numpy(_SPECIAL)          # ... and in the last elements (the second grid-stride trip)
    assert bool(torch.isfinite(x).all()) and float(x.abs().max()) < 1.01e30
    return x


def _bf16_rne_bits(v):
    """fp32 array -> bf16 bits, round to nearest even (finite inputs), on the integer representation"""
    b = v.view(np.uint32).astype(np.uint64)
    return (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def _ref_planes(v):
    hi = _bf16_rne_bits(v)
    hi_f = (hi.astype(np.uint32) << 16).view(np.float32)
    return hi, _bf16_rne_bits(v - hi_f)


def _ref_dropout(x, seed, site, p, resid=None):
    """(keep, fp32 result): keep ? fl32(x * scale) : +0, scale = 1 / (1 - p) in fp32; the residual form adds resid with one more
    fp32 rounding"""
    xn = x.numpy()
    keep = O.dropout_keep_mask(seed, site, xn.size, p)
    scale = np.float32(1) / (np.float32(1) - np.float32(p))
    v = np.where(keep, xn * scale, np.float32(0))
    if resid is not None:
        v = v + resid.numpy()
    assert v.dtype == np.float32
    return keep, v


def _same_bits(got, want, dropped_negative, what):
    """Every element bit-identical.  The one licence: where the mask DROPPED a negative input the result is a zero whose sign the
    contract does not fix (`keep ? x * scale : 0` gives +0, a multiply by a 0 / 1 mask would give -0), so there -- and only there --
    +0 and -0 count as equal.  got / want: integer views of the same width."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    magnitude = got.dtype.type((1 << (8 * got.dtype.itemsize - 1)) - 1)          # every bit but the sign
    ok = (got == want) | (dropped_negative & ((got & magnitude) == 0) & ((want & magnitude) == 0))
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} of {ok.size} elements differ, first at {int(np.argmax(~ok))}"


def _planes_with_canaries(n, gap, tail, dev, ops):
    """planes storage [hi (n) | gap | lo (n) | tail] filled with a canary; lo_off = n + gap"""
    buf = torch.full((2 * n + gap + tail,), 0x5A5A, dtype=torch.int16, device=dev)
    return buf, ops.Planes(buf, 1, n, lo_off=n + gap)


def _check_planes(buf, n, gap, hi, lo, loose, what):
    got = buf.cpu().numpy().view(np.uint16)
    _same_bits(got[:n], hi, loose, what + " hi plane")
    _same_bits(got[n + gap:2 * n + gap], lo, loose, what + " lo plane")
    assert bool((got[n:n + gap] == 0x5A5A).all()) and bool((got[2 * n + gap:] == 0x5A5A).all()), what + ": canary overwritten"


@pytest.mark.parametrize("p", _PS)
@pytest.mark.parametrize("n", _NS)
def test_dropout_family_bit_for_bit(ops, dev, n, p):
    x = _data(n, n + 1)
    resid = _data(n, n + 2).flip(0).contiguous()
    xd, rd = x.to(dev), resid.to(dev)
    neg = np.signbit(x.numpy())
    if p == _PS[0]:
        assert bool(O.dropout_keep_mask(5, 1, n, p).all())              # threshold 0: nothing dropped
    for seed, site in _keys(n, p):
        drop = ops.Drop(p, seed=seed, site=site)
        keep, want = _ref_dropout(x, seed, site, p)
        loose = ~keep & neg
        wbits = want.view(np.uint32)
        # dropout_apply, out of place into a buffer with NaN behind it, then in place
        buf = torch.full((n + 64,), float("nan"), device=dev)
        ops.dropout_apply(xd, buf[:n], drop)
        got = buf.cpu().numpy()
        _same_bits(got[:n].view(np.uint32), wbits, loose, f"dropout_apply seed {seed} site {site}")
        assert bool(np.isnan(got[n:]).all())
        inpl = xd.clone()
        ops.dropout_apply(inpl, inpl, drop)
        _same_bits(inpl.cpu().numpy().view(np.uint32), wbits, loose, f"dropout_apply in place seed {seed} site {site}")
        # dropout_planes, the lo plane further behind than n, canaries between and behind the planes
        gap, tail = 8, 12
        pbuf, pl = _planes_with_canaries(n, gap, tail, dev, ops)
        ops.dropout_planes(xd, pl, drop)
        hi, lo = _ref_planes(want)
        _check_planes(pbuf, n, gap, hi, lo, loose, f"dropout_planes seed {seed} site {site}")
        # dropout_residual
        _, wres = _ref_dropout(x, seed, site, p, resid)
        buf.fill_(float("nan"))
        ops.dropout_residual(xd, rd, buf[:n], drop)
        got = buf.cpu().numpy()
        _same_bits(got[:n].view(np.uint32), wres.view(np.uint32), loose, f"dropout_residual seed {seed} site {site}")
        assert bool(np.isnan(got[n:]).all())


@pytest.mark.parametrize("n", _NS)
def test_dropout_planes_without_dropout_is_split_planes(ops, dev, n):
    x = _data(n, n + 3)
    xd = x.to(dev)
    hi, lo = _ref_planes(x.numpy())
    never = np.zeros(n, dtype=bool)
    ref_buf, ref_pl = _planes_with_canaries(n, 0, 4, dev, ops)
    ops.split_planes(xd, ref_pl)
    _check_planes(ref_buf, n, 0, hi, lo, never, "split_planes")
    for drop in (None, ops.Drop(0.0, seed=1234, site=7)):
        for gap in (0, 8):
            buf, pl = _planes_with_canaries(n, gap, 4, dev, ops)
            ops.dropout_planes(xd, pl, drop)
            _check_planes(buf, n, gap, hi, lo, never, "dropout_planes(p = 0)")
            assert torch.equal(buf[:n], ref_buf[:n]) and torch.equal(buf[n + gap:2 * n + gap], ref_buf[n:2 * n])


def test_every_kernel_keeps_the_same_elements(ops, dev):
    """One (seed, site, p) -> one kept set, in the three pointwise kernels and in the fused GEMM epilogue at ld_out == N: what the
    backward relies on when dropout_planes replays a forward epilogue's mask.  Inputs have no exact zero, so kept = (out != 0)."""
    M, N, K = 96, 128, 64
    g = torch.Generator().manual_seed(31)
    a, w = torch.randn(M, K, generator=g).to(dev), torch.randn(N, K, generator=g).to(dev)
    plain = torch.empty(M, N, device=dev)
    ops.gemm(a, w, plain, M, N, K)
    assert bool((plain != 0).all())
    x = plain.flatten().contiguous()
    for seed, site, p in ((1234, 7, 0.1), (2 ** 64 - 1, 2 ** 24 - 1, 0.5), (0, 65535, 0.99999), (77, 0, 1e-5)):
        drop = ops.Drop(p, seed=seed, site=site)
        keep = torch.from_numpy(O.dropout_keep_mask(seed, site, M * N, p))
        out = torch.empty(M, N, device=dev)
        ops.gemm(a, w, out, M, N, K, drop=drop)
        assert torch.equal((out != 0).flatten().cpu(), keep), "GEMM epilogue"
        assert torch.equal((ops.dropout_apply(x, torch.empty_like(x), drop) != 0).cpu(), keep), "dropout_apply"
        pl = ops.dropout_planes(x, ops.Planes.empty(1, M * N, dev), drop)
        assert torch.equal((pl.buf[:M * N] != 0).cpu(), keep), "dropout_planes"
        assert torch.equal((pl.to_float().flatten() != 0).cpu(), keep)
        resid = torch.full_like(x, 3.0)
        assert torch.equal((ops.dropout_residual(x, resid, torch.empty_like(x), drop) != resid).cpu(), keep), "dropout_residual"


# ------------------------------------------------------------------------------------------- split_planes_multi
def test_split_planes_multi_chunks_and_canaries(ops, dev):
    """Six chunks in one launch: counts at the edges of the 256-thread x 4-element loop, each with its own lo_off, two of them writing
    consecutive row blocks of ONE planes buffer (as the fused QKV weight's three sources do).  Each chunk = split_planes of its
    source, byte for byte; every other byte of the destinations keeps its canary."""
    from lr2ppo_amd import _native
    counts = [4, 252, 1024, 1028, 300000, 1028]
    srcs = [_data(c, 50 + i).to(dev) for i, c in enumerate(counts)]
    CAN = 0x3C3C
    # chunks 0-3: one buffer each, [lead | hi | gap | lo | 8] with a different lead and gap; chunks 4 and 5: rows [0, 75000) and
    # [75000, 75257) of one [75257, 4] planes buffer, whose lo plane lies shared_n elements behind its hi plane for both
    shared_n = counts[4] + counts[5]
    shared = torch.full((2 * shared_n + 16,), CAN, dtype=torch.int16, device=dev)
    bufs, rows, owned = [], [], []
    for i in range(4):
        c, gap, lead = counts[i], 4 * (i + 1), 8 * (i + 1)
        b = torch.full((lead + 2 * c + gap + 8,), CAN, dtype=torch.int16, device=dev)
        bufs.append(b)
        rows.append((srcs[i].data_ptr(), b.data_ptr() + 2 * lead, c + gap, c))
        owned.append((b, lead, c + gap, c))
    rows.append((srcs[4].data_ptr(), shared.data_ptr(), shared_n, counts[4]))
    rows.append((srcs[5].data_ptr(), shared.data_ptr() + 2 * counts[4], shared_n, counts[5]))
    arr = (_native.SplitChunk * len(rows))()
    for i, (s, d, lo, cnt) in enumerate(rows):
        assert s % 16 == 0 and d % 8 == 0 and lo % 4 == 0 and cnt % 4 == 0
        arr[i].src, arr[i].dst_hi, arr[i].lo_off, arr[i].count = s, d, lo, cnt
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    ops.split_planes_multi(table, len(rows))
    torch.cuda.synchronize()

    def single(src):
        pl = ops.Planes.empty(1, src.numel(), dev)
        ops.split_planes(src, pl)
        n = src.numel()
        return pl.buf[:n].cpu(), pl.buf[n:2 * n].cpu()

    for i, (b, lead, lo_off, c) in enumerate(owned):
        hi, lo = single(srcs[i])
        got = b.cpu()
        assert torch.equal(got[lead:lead + c], hi) and torch.equal(got[lead + lo_off:lead + lo_off + c], lo), f"chunk {i}"
        mine = torch.zeros(got.numel(), dtype=torch.bool)
        mine[lead:lead + c] = True
        mine[lead + lo_off:lead + lo_off + c] = True
        assert bool((got[~mine] == CAN).all()), f"chunk {i}: canary overwritten"
        whi, wlo = _ref_planes(srcs[i].cpu().numpy())                    # ... and split_planes itself = the CPU rule
        assert np.array_equal(hi.numpy().view(np.uint16), whi) and np.array_equal(lo.numpy().view(np.uint16), wlo)
    got = shared.cpu()
    h4, l4 = single(srcs[4])
    h5, l5 = single(srcs[5])
    assert torch.equal(got[:shared_n], torch.cat([h4, h5])) and torch.equal(got[shared_n:2 * shared_n], torch.cat([l4, l5]))
    assert bool((got[2 * shared_n:] == CAN).all())


# ------------------------------------------------------------------------------------------- 'cls' head
_ROWS, _DS, _CS = [1, 3, 4, 5, 257, 1200], [4, 252, 256, 260, 768, 1028], [1, 2, 3, 8]


def _cls_head_cases():
    """a seeded subset of rows x D x C: 12 triples, every value of every axis at least once (each axis: its values, padded with
    seeded picks to 12 and shuffled)"""
    rng = np.random.RandomState(20)
    cols = []
    for axis in (_ROWS, _DS, _CS):
        v = list(axis) + [axis[i] for i in rng.randint(0, len(axis), 12 - len(axis))]
        cols.append([v[i] for i in rng.permutation(12)])
    cases = sorted(set(zip(*cols)))
    for axis, col in zip((_ROWS, _DS, _CS), zip(*cases)):
        assert set(axis) == set(col)
    return cases


def _with_canary(shape, dev):
    n = int(np.prod(shape))
    buf = torch.full((n + 64,), float("nan"), device=dev)
    return buf, buf[:n].view(*shape)


def _within(got, ref, bound, what):
    err = (got.double().cpu() - ref).abs()
    ok = err <= bound
    assert bool(ok.all()), f"{what}: worst |err| / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}, {int((~ok).sum())} elements"


@pytest.mark.parametrize("rows,D,C", _cls_head_cases())
def test_cls_head_forward_and_backward_against_fp64(ops, dev, rows, D, C):
    """Allowance: the a-priori bound of an fp32 sum of n products in ANY order, |err| <= (n + 2) 2^-24 sum |terms| (each term passes
    at most n + 1 roundings, the + 2 covers the second-order part for n < 4096): n = D (+ the bias) forward, C for dx, rows for
    dw / db.  sum |terms| is formed in fp64 from the same inputs."""
    g = torch.Generator().manual_seed(rows * 10000 + D * 10 + C)
    x, w, b = torch.randn(rows, D, generator=g), torch.randn(C, D, generator=g) * 0.2, torch.randn(C, generator=g)
    dy = torch.randn(rows, C, generator=g)
    xd, wd, bd, dyd = x.to(dev), w.to(dev), b.to(dev), dy.to(dev)
    x64, w64, b64, dy64 = x.double(), w.double(), b.double(), dy.double()
    ybuf, y = _with_canary((rows, C), dev)
    ops.cls_head_fwd(xd, wd, bd, y, rows=rows, D=D, C=C)
    _within(y, x64 @ w64.t() + b64, (D + 2) * U * (x64.abs() @ w64.abs().t() + b64.abs()), "y")
    assert bool(torch.isnan(ybuf[rows * C:]).all())
    refs = {"dx": (dy64 @ w64, (C + 2) * U * (dy64.abs() @ w64.abs())),
            "dw": (dy64.t() @ x64, (rows + 2) * U * (dy64.abs().t() @ x64.abs())),
            "db": (dy64.sum(0), (rows + 2) * U * dy64.abs().sum(0))}
    shapes = {"dx": (rows, D), "dw": (C, D), "db": (C,)}
    full = {}
    for given in (("dx", "dw", "db"), ("dw", "db"), ("dx",)):
        outs = {k: _with_canary(shapes[k], dev) for k in given}
        ops.cls_head_bwd(xd, wd, dyd, *[outs[k][1] if k in outs else None for k in ("dx", "dw", "db")], rows=rows, D=D, C=C)
        for k, (buf, t) in outs.items():
            _within(t, refs[k][0], refs[k][1], f"{k} (outputs {given})")
            assert bool(torch.isnan(buf[t.numel():]).all()), k
            assert torch.equal(full.setdefault(k, t.clone()), t), f"{k} depends on which other outputs are asked for"


# ------------------------------------------------------------------------------------------- 'cls' scores and NLL
def _logits(rows, C, shift, seed):
    """rows cycle through four kinds, starting at kind `shift`: N(0, 1) logits; every entry +80 or -80 at random (ties, and exp(-160)
    beside exp(0)); all +80; all -80.  Without the max shift exp(80) overflows fp32 and exp(-80) sums to a denormal."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(rows, C, generator=g)
    kind = (torch.arange(rows) + shift) % 4
    pm = torch.randint(0, 2, (rows, C), generator=g).float() * 160 - 80
    z = torch.where((kind == 1).view(-1, 1), pm, z)
    z = torch.where((kind == 2).view(-1, 1), torch.full_like(z, 80.0), z)
    z = torch.where((kind == 3).view(-1, 1), torch.full_like(z, -80.0), z)
    return z, g


def _scores_chain(z, ds):
    """probs = softmax(z), scores = sum_k k p_k, dlogits = autograd of (scores * ds).sum(), in the dtype of z"""
    z = z.clone().requires_grad_()
    p = torch.softmax(z, -1)
    s = (p * torch.arange(z.shape[1], dtype=z.dtype)).sum(-1)
    (s * ds.to(z.dtype)).sum().backward()
    return {"probs": p.detach(), "scores": s.detach(), "dlogits": z.grad}


def _nll_chain(z, t):
    z = z.clone().requires_grad_()
    loss = torch.nn.functional.nll_loss(torch.log_softmax(z, -1), t)
    loss.backward()
    return {"loss": loss.detach().view(1), "dlogits": z.grad}


def _rel(got, ref):
    """max |got - ref| / max |ref|; a reference that is identically zero (C = 1: scores, loss and both gradients) asks for exact
    zeros: any error is then infinite"""
    err, scale = float((got.double() - ref).abs().max()), float(ref.abs().max())
    return 0.0 if err == 0.0 else (err / scale if scale > 0 else float("inf"))


_SCORE_CASES = [(r, c, s) for r in (1, 255, 256, 257, 5000) for c in (1, 2, 8) for s in (0, 1)]
_NLL_CASES = [(r, c, s) for r in (1, 1023, 1024, 1025, 3000) for c in (1, 3, 8) for s in (0, 1)]
FLOOR = 8 * U

# max |fp32 - fp64| / max |fp64| of TORCH'S OWN fp32 CPU evaluation of the formulas above (_scores_chain / _nll_chain on the float32
# inputs against the same function on their float64 copies), on the inputs of each case -- measured on the CPU, never on the kernels
# (`PYTHONPATH=. python tests/test_pointwise_gpu.py` prints the tables again).  The kernels are gated at 4 x these per output tensor,
# floored at 8 x 2^-24: the factor covers expf / logf being a few ulp apart between libraries and the other summation order of the
# 1024-way block reduction.  The two 1.00 entries: a single row of +80 / -80 logits, whose true gradient (~1e-68) is below the
# smallest fp32 number -- fp32 gives 0, the whole of the reference is the error; anything but a vanishing result still fails there.
# (rows, C, shift): (probs, scores, dlogits)
MEASURED_SCORES = {
    (1, 1, 0): (0.00e+00, 0.00e+00, 0.00e+00),
    (1, 1, 1): (0.00e+00, 0.00e+00, 0.00e+00),
    (1, 2, 0): (9.53e-09, 7.02e-08, 1.36e-07),
    (1, 2, 1): (3.26e-70, 0.00e+00, 1.00e+00),
    (1, 8, 0): (6.00e-08, 1.08e-07, 1.13e-07),
    (1, 8, 1): (3.26e-70, 0.00e+00, 1.00e+00),
    (255, 1, 0): (0.00e+00, 0.00e+00, 0.00e+00),
    (255, 1, 1): (0.00e+00, 0.00e+00, 0.00e+00),
    (255, 2, 0): (6.64e-08, 5.99e-08, 1.88e-07),
    (255, 2, 1): (8.08e-08, 8.08e-08, 1.54e-07),
    (255, 8, 0): (7.32e-08, 9.65e-08, 2.40e-07),
    (255, 8, 1): (7.77e-08, 1.17e-07, 1.78e-07),
    (256, 1, 0): (0.00e+00, 0.00e+00, 0.00e+00),
    (256, 1, 1): (0.00e+00, 0.00e+00, 0.00e+00),
    (256, 2, 0): (6.11e-08, 6.05e-08, 1.47e-07),
    (256, 2, 1): (6.29e-08, 6.29e-08, 8.01e-08),
    (256, 8, 0): (1.11e-07, 9.91e-08, 3.23e-07),
    (256, 8, 1): (9.29e-08, 1.11e-07, 1.32e-07),
    (257, 1, 0): (0.00e+00, 0.00e+00, 0.00e+00),
    (257, 1, 1): (0.00e+00, 0.00e+00, 0.00e+00),
    (257, 2, 0): (6.36e-08, 6.36e-08, 1.10e-07),
    (257, 2, 1): (8.23e-08, 5.45e-08, 1.26e-07),
    (257, 8, 0): (8.63e-08, 8.56e-08, 2.92e-07),
    (257, 8, 1): (5.67e-08, 9.40e-08, 1.08e-07),
    (5000, 1, 0): (0.00e+00, 0.00e+00, 0.00e+00),
    (5000, 1, 1): (0.00e+00, 0.00e+00, 0.00e+00),
    (5000, 2, 0): (7.77e-08, 7.77e-08, 1.44e-07),
    (5000, 2, 1): (8.13e-08, 8.13e-08, 1.15e-07),
    (5000, 8, 0): (9.87e-08, 1.20e-07, 1.77e-07),
    (5000, 8, 1): (8.48e-08, 1.13e-07, 2.06e-07),
}
# (rows, C, shift): (loss, dlogits)
MEASURED_NLL = {
    (1, 1, 0): (0.00e+00, 0.00e+00),
    (1, 1, 1): (0.00e+00, 0.00e+00),
    (1, 3, 0): (4.66e-08, 6.65e-08),
    (1, 3, 1): (2.75e-09, 3.26e-70),
    (1, 8, 0): (2.24e-08, 3.18e-08),
    (1, 8, 1): (2.75e-09, 1.09e-70),
    (1023, 1, 0): (0.00e+00, 0.00e+00),
    (1023, 1, 1): (0.00e+00, 0.00e+00),
    (1023, 3, 0): (7.33e-08, 7.33e-08),
    (1023, 3, 1): (2.33e-08, 8.74e-08),
    (1023, 8, 0): (1.36e-07, 9.58e-08),
    (1023, 8, 1): (5.48e-08, 7.35e-08),
    (1024, 1, 0): (0.00e+00, 0.00e+00),
    (1024, 1, 1): (0.00e+00, 0.00e+00),
    (1024, 3, 0): (1.01e-07, 9.69e-08),
    (1024, 3, 1): (5.38e-08, 1.16e-07),
    (1024, 8, 0): (1.93e-08, 1.02e-07),
    (1024, 8, 1): (8.56e-08, 1.23e-07),
    (1025, 1, 0): (0.00e+00, 0.00e+00),
    (1025, 1, 1): (0.00e+00, 0.00e+00),
    (1025, 3, 0): (1.56e-07, 9.18e-08),
    (1025, 3, 1): (7.67e-08, 1.02e-07),
    (1025, 8, 0): (4.70e-08, 9.50e-08),
    (1025, 8, 1): (3.33e-08, 1.13e-07),
    (3000, 1, 0): (0.00e+00, 0.00e+00),
    (3000, 1, 1): (0.00e+00, 0.00e+00),
    (3000, 3, 0): (6.97e-08, 1.19e-07),
    (3000, 3, 1): (6.98e-08, 1.28e-07),
    (3000, 8, 0): (6.56e-08, 8.99e-08),
    (3000, 8, 1): (2.12e-07, 9.34e-08),
}


def _gate(measured):
    return max(4.0 * measured, FLOOR)


def _score_inputs(rows, C, shift):
    z, g = _logits(rows, C, shift, 7000 + rows * 10 + C)
    return z, torch.randn(rows, generator=g)


def _nll_inputs(rows, C, shift):
    z, g = _logits(rows, C, shift, 9000 + rows * 10 + C)
    t = torch.randint(0, C, (rows,), generator=g)
    t[:min(rows, C)] = torch.arange(min(rows, C))
    assert rows < C or set(t.tolist()) == set(range(C))                                # every class is a target
    return z, t


@pytest.mark.parametrize("rows,C,shift", _SCORE_CASES)
def test_cls_scores_and_backward_against_fp64(ops, dev, rows, C, shift):
    z, ds = _score_inputs(rows, C, shift)
    ref = _scores_chain(z.double(), ds)
    zd = z.to(dev)
    pbuf, probs = _with_canary((rows, C), dev)
    sbuf, scores = _with_canary((rows,), dev)
    gbuf, dlogits = _with_canary((rows, C), dev)
    ops.cls_scores(zd, probs, scores, rows=rows, C=C, softmax=True)
    ops.cls_scores_bwd(probs, scores, ds.to(dev), dlogits, rows=rows, C=C)
    got = {"probs": probs.cpu(), "scores": scores.cpu(), "dlogits": dlogits.cpu()}
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    bad = []
    for i, k in enumerate(("probs", "scores", "dlogits")):
        r, gate = _rel(got[k], ref[k]), _gate(MEASURED_SCORES[(rows, C, shift)][i])
        print(f"  cls_scores rows {rows} C {C} shift {shift}: {k:8s} {r:.3e} (gate {gate:.3e})")
        if not r <= gate:
            bad.append((k, r, gate))
    assert not bad, bad
    for buf, t in ((pbuf, probs), (sbuf, scores), (gbuf, dlogits)):
        assert bool(torch.isnan(buf[t.numel():]).all())
    # probs is optional: the scores do not depend on it
    s2 = torch.empty(rows, device=dev)
    ops.cls_scores(zd, None, s2, rows=rows, C=C, softmax=True)
    assert torch.equal(s2, scores)


@pytest.mark.parametrize("rows,C,shift", _NLL_CASES)
def test_nll_loss_against_fp64(ops, dev, rows, C, shift):
    z, t = _nll_inputs(rows, C, shift)
    ref = _nll_chain(z.double(), t)
    zd, td = z.to(dev), t.to(dev)
    lbuf, loss = _with_canary((1,), dev)
    gbuf, dlogits = _with_canary((rows, C), dev)
    ops.nll_loss(zd, td, loss, dlogits, rows=rows, C=C)
    got = {"loss": loss.cpu(), "dlogits": dlogits.cpu()}
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    bad = []
    for i, k in enumerate(("loss", "dlogits")):
        r, gate = _rel(got[k], ref[k]), _gate(MEASURED_NLL[(rows, C, shift)][i])
        print(f"  nll_loss rows {rows} C {C} shift {shift}: {k:8s} {r:.3e} (gate {gate:.3e})")
        if not r <= gate:
            bad.append((k, r, gate))
    assert not bad, bad
    assert bool(torch.isnan(lbuf[1:]).all()) and bool(torch.isnan(gbuf[rows * C:]).all())
    # the gradient is optional: the loss does not depend on it
    l2 = torch.full((1,), float("nan"), device=dev)
    ops.nll_loss(zd, td, l2, None, rows=rows, C=C)
    assert torch.equal(l2, loss)


if __name__ == "__main__":          # the CPU measurement behind MEASURED_SCORES / MEASURED_NLL (no GPU, no kernel)
    print("MEASURED_SCORES = {")
    for case in _SCORE_CASES:
        z, ds = _score_inputs(*case)
        lo, hi = _scores_chain(z, ds), _scores_chain(z.double(), ds)
        print(f"    {case}: (" + ", ".join(f"{_rel(lo[k], hi[k]):.2e}" for k in ("probs", "scores", "dlogits")) + "),")
    print("}\nMEASURED_NLL = {")
    for case in _NLL_CASES:
        z, t = _nll_inputs(*case)
        lo, hi = _nll_chain(z, t), _nll_chain(z.double(), t)
        print(f"    {case}: (" + ", ".join(f"{_rel(lo[k], hi[k]):.2e}" for k in ("loss", "dlogits")) + "),")
    print("}")
