"""A/B of two whole builds of liblr2ppo_hip.so (same ABI) on the self-attention entry points, alternating inside one process:

    python tools/dbg/attn_lib_ab.py A.so B.so           us per call of lr2_self_attn_fwd (plain; dropout 0.1 + lse) and lr2_self_attn_bwd
                                                        (given o + lse, dropout 0.1) at the training shape 512 x 12 x 197
    python tools/dbg/attn_lib_ab.py --bits A.so B.so    both libraries on the same inputs at the smallest shapes that reach every kernel
                                                        form and edge: per entry point and shape, is every output byte equal?  Where
                                                        it is not, A is also run against itself (open finding).

Only lr2_self_attn_fwd / _bwd / _fwd_bf16 are bound; inputs are made with torch, so the in-tree library is not loaded."""
import ctypes as C
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from lr2ppo_amd import _native  # noqa: E402

SYMBOLS = ("lr2_self_attn_fwd", "lr2_self_attn_bwd", "lr2_self_attn_fwd_bf16")
dev = torch.device("cuda:0")


def load(path):
    lib = C.CDLL(os.path.abspath(path))
    for name in SYMBOLS:
        getattr(lib, name).argtypes, getattr(lib, name).restype = _native.SIGNATURES[name], C.c_int
    return lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def planes(x):
    """fp32 [rows, cols] -> int16 [2 * rows * cols] = [hi | lo] bf16 planes, x ~ hi + lo"""
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()
    return torch.cat([hi.view(torch.int16).reshape(-1), lo.view(torch.int16).reshape(-1)])


class Case:
    """Inputs of one (batch, heads, L) and fresh, pattern-filled outputs per call."""

    def __init__(self, batch, heads, L, seed=0):
        self.batch, self.heads, self.L, self.E, self.rows = batch, heads, L, heads * 64, batch * L
        g = torch.Generator(device=dev).manual_seed(seed)
        x = torch.randn(self.rows, 3 * self.E, device=dev, generator=g) * 0.5
        self.qkv, self.qkv1 = planes(x), x.bfloat16().view(torch.int16).reshape(-1)      # two planes / one plane
        self.do = planes(torch.randn(self.rows, self.E, device=dev, generator=g))
        seg = torch.ones(batch, L, dtype=torch.int64, device=dev)
        if L > 2:
            seg[1::2, L - (L // 3):] = 0                                                  # odd sequences: the last third is padding
        self.seg = seg.reshape(-1)

    def out(self, n, dtype):
        return torch.full((n * torch.empty(0, dtype=dtype).element_size(),), 0x5a, dtype=torch.uint8, device=dev).view(dtype)

    def qkv_ptrs(self, t):
        return t.data_ptr(), t.data_ptr() + 2 * self.E, t.data_ptr() + 4 * self.E

    def fwd(self, lib, drop, outs=None):
        """outs: the dict an earlier call returned, written again (timings: no allocation between the calls)"""
        o, lse = (outs["o"], outs["lse"]) if outs else (self.out(2 * self.rows * self.E, torch.int16),
                                                        self.out(self.batch * self.heads * self.L, torch.float32))
        rc = lib.lr2_self_attn_fwd(*self.qkv_ptrs(self.qkv), self.rows * 3 * self.E, 3 * self.E, self.seg.data_ptr(), None, o.data_ptr(),
                                   self.rows * self.E, self.E, lse.data_ptr(), drop, 7, 1, self.batch, self.heads, self.L, 64, 0.125, stream())
        assert rc == 0, rc
        return {"o": o, "lse": lse}

    def bwd(self, lib, drop, given=None, outs=None):
        """given = the forward's {"o", "lse"}: the streaming backward where the shape allows it; None: the recomputing one"""
        n = self.batch * self.heads * self.L
        if outs:
            d, lse, dsum = outs["dqkv"], outs["lse"], outs["dsum"]
        else:
            d, dsum = self.out(2 * self.rows * 3 * self.E, torch.int16), self.out(n, torch.float32)
            lse = given["lse"].clone() if given else self.out(n, torch.float32)
        rc = lib.lr2_self_attn_bwd(*self.qkv_ptrs(self.qkv), self.rows * 3 * self.E, 3 * self.E, self.do.data_ptr(), self.rows * self.E, self.E,
                                   self.seg.data_ptr(), *self.qkv_ptrs(d), self.rows * 3 * self.E, 3 * self.E,
                                   given["o"].data_ptr() if given else None, self.rows * self.E if given else 0, self.E if given else 0,
                                   lse.data_ptr(), dsum.data_ptr(), drop, 7, 1, self.batch, self.heads, self.L, 64, 0.125, stream())
        assert rc == 0, rc
        return {"dqkv": d, "lse": lse, "dsum": dsum}

    def fwd_bf16(self, lib):
        of, ob = self.out(self.rows * self.E, torch.float32), self.out(self.rows * self.E, torch.int16)
        oq, os_ = self.out(self.rows * self.E, torch.uint8), self.out(self.rows * self.E // 32, torch.uint8)
        rc = lib.lr2_self_attn_fwd_bf16(*self.qkv_ptrs(self.qkv1), 3 * self.E, self.seg.data_ptr(), of.data_ptr(), oq.data_ptr(), os_.data_ptr(),
                                        ob.data_ptr(), self.E, self.batch, self.heads, self.L, 64, 0.125, stream())
        assert rc == 0, rc
        return {"o_f32": of, "o_q": oq, "o_scales": os_, "o_bf16": ob}


def differing(x, y):
    """names of the outputs that are not byte-equal, with the number of differing bytes"""
    torch.cuda.synchronize()
    bad = []
    for k in x:
        n = int((x[k].view(torch.uint8) != y[k].view(torch.uint8)).sum())
        if n:
            bad.append(f"{k}: {n} of {x[k].numel() * x[k].element_size()} bytes")
    return bad


def bits(lib_a, lib_b):
    checks = []      # (label, function of a library -> outputs)
    for L in (1, 17, 64, 65, 128, 129, 224, 225, 256, 257, 385, 514):
        c = Case(2, 2, L)
        for drop in (0.0, 0.1):
            checks.append((f"fwd                    (2, 2, {L}) dropout {drop}", lambda lib, c=c, drop=drop: c.fwd(lib, drop)))
            checks.append((f"bwd, recomputing       (2, 2, {L}) dropout {drop}", lambda lib, c=c, drop=drop: c.bwd(lib, drop)))
    for L in (64, 224):
        c = Case(256, 1, L)
        given = c.fwd(lib_a, 0.1)
        checks.append((f"bwd given o, streaming (256, 1, {L}) dropout 0.1", lambda lib, c=c, given=given: c.bwd(lib, 0.1, given)))
    for shape in ((2, 2, 288), (256, 1, 224)):
        c = Case(*shape)
        checks.append((f"fwd_bf16               {shape}", lambda lib, c=c: c.fwd_bf16(lib)))
    for L in (100, 224):
        c = Case(256, 1, L)
        for drop in (0.0, 0.1):
            checks.append((f"fwd, persistent        (256, 1, {L}) dropout {drop}", lambda lib, c=c, drop=drop: c.fwd(lib, drop)))
    n_bad = 0
    for label, run in checks:
        a = run(lib_a)
        bad = differing(a, run(lib_b))
        if not bad:
            print(f"equal   {label}", flush=True)
            continue
        n_bad += 1
        again = differing(a, run(lib_a))
        print(f"DIFFER  {label}: {'; '.join(bad)} -- A against itself: {'; '.join(again) if again else 'equal'}", flush=True)
    print(f"{len(checks) - n_bad} of {len(checks)} checks byte-equal")
    return n_bad


def timings(libs):
    batch, heads, L = 512, 12, 197
    c = Case(batch, heads, L)
    first = next(iter(libs.values()))
    given = c.fwd(first, 0.1)
    fo, bo = c.fwd(first, 0.0), c.bwd(first, 0.1, given)
    res = {}
    for rep in range(3):
        for n, lib in libs.items():
            calls = {"bwd": lambda: c.bwd(lib, 0.1, given, bo), "fwd": lambda: c.fwd(lib, 0.0, fo),
                     "fwd, dropout 0.1 + lse": lambda: c.fwd(lib, 0.1, fo)}
            for what, call in calls.items():
                for _ in range(2):
                    call()
                torch.cuda.synchronize()
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(8):
                    call()
                e.record()
                torch.cuda.synchronize()
                res.setdefault((n, what), []).append(s.elapsed_time(e) / 8 * 1e3)
    for (n, what), ts in sorted(res.items()):
        print(f"{n:>2} {what}: {min(ts):8.1f} us", flush=True)


if __name__ == "__main__":
    paths = [a for a in sys.argv[1:] if not a.startswith("-")]
    if len(paths) != 2:
        sys.exit(__doc__)
    lib_a, lib_b = load(paths[0]), load(paths[1])
    if "--bits" in sys.argv:
        sys.exit(1 if bits(lib_a, lib_b) else 0)
    timings({"A": lib_a, "B": lib_b})
