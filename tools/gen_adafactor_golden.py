"""Generate tests/golden/adafactor.npz and tests/golden/sched_all.json from the REFERENCE's Adafactor and schedule functions.

Run once on a CPU:  python -B tools/gen_adafactor_golden.py --reference /path/to/reference

The reference's tencentpretrain/utils/optimizers.py is loaded by file path at generation time only; no test runs this script or
reads the reference.  The fixtures hold data only.

adafactor.npz: two param groups (weight decay 0.01 / 0) over [5,7] [1,7] [7,1] [4,768] | [3] [768]; three steps with a learning
rate that changes every step; parameter 1 has no gradient on step 2.  Stored: p0_i, g{s}_i, p{s}_i, step{s}_i, the state after
step 2 (row2_i / col2_i / v2_i: what the interchange test loads), lrs, and -- for the tolerance rule of
tests/test_adafactor_gpu.py -- dist_<quantity> = [relative L2, max-abs / max|.|]: the largest one-step distance between the
reference's fp32 result and an fp64 restatement of the same step started from the reference's fp32 state, over steps and tensors.
Inputs keep 8 mantissa bits so that the compressed file stays under 100 KB.
"""
import argparse
import importlib.util
import json
import math
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
SHAPES = [[(5, 7), (1, 7), (7, 1), (4, 768)], [(3,), (768,)]]
WDS = [0.01, 0.0]
LRS = [[1e-3, 7e-4, 1.3e-3], [5e-4, 9e-4, 2e-4]]       # per group, per step
SKIP = (2, 1)                                          # (step, flat parameter index) without a gradient
EPS0, CLIP, DECAY_RATE = 1e-30, 1.0, -0.8


def restate(p, g, st, t, lr, wd, eps0=EPS0, clip=CLIP, decay_rate=DECAY_RATE):
    """One Adafactor step (relative_step=False, scale_parameter=False, beta1=None) in fp64 -> (p_new, new state)."""
    p, g = p.double(), g.double()
    b = 1.0 - math.pow(t, decay_rate)
    u = g * g + eps0
    if p.dim() == 2:
        row = b * st["row"].double() + (1 - b) * u.mean(1)
        col = b * st["col"].double() + (1 - b) * u.mean(0)
        U = g * (row / row.mean()).rsqrt()[:, None] * col.rsqrt()[None, :]
        new = {"row": row, "col": col}
    else:
        v = b * st["v"].double() + (1 - b) * u
        U = g * v.rsqrt()
        new = {"v": v}
    U = U / max(1.0, float(U.norm() / math.sqrt(U.numel())) / clip) * lr
    return p + (-wd * lr) * p - U, new


def coarse(t):
    """keep 8 mantissa bits (the upper 16 bits of the fp32 pattern): exact in fp32, and it compresses"""
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


def dist(a32, b64):
    d = (a32.double() - b64).abs()
    return float(d.norm() / b64.norm()), float(d.max() / b64.abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference tree (holds tencentpretrain/utils/optimizers.py)")
    a = ap.parse_args()
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("ref_optimizers", os.path.join(a.reference, "tencentpretrain", "utils", "optimizers.py"))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)

    gen = torch.Generator().manual_seed(20261021)
    flat = [s for grp in SHAPES for s in grp]
    ps = [torch.nn.Parameter(coarse(0.02 * torch.randn(*s, generator=gen))) for s in flat]
    n0 = len(SHAPES[0])
    opt = R.Adafactor([{"params": ps[:n0], "weight_decay": WDS[0]}, {"params": ps[n0:], "weight_decay": WDS[1]}], lr=LRS[0][0],
                      scale_parameter=False, relative_step=False)
    arrays = {f"p0_{i}": p.detach().clone() for i, p in enumerate(ps)}
    arrays["lrs"] = torch.tensor(LRS, dtype=torch.float64)
    worst = {k: [0.0, 0.0] for k in ("row", "col", "v", "delta")}

    def note(k, a32, b64):
        d = dist(a32, b64)
        worst[k] = [max(worst[k][0], d[0]), max(worst[k][1], d[1])]

    for s in range(1, 4):
        before, before_state = [], []
        for i, p in enumerate(ps):
            g = coarse(0.1 * torch.randn(*flat[i], generator=gen))
            p.grad = None if (s, i) == SKIP else g
            if p.grad is not None:
                arrays[f"g{s}_{i}"] = g
            before.append(p.detach().clone())
            st = opt.state[p]
            if len(st) == 0:
                before_state.append({"row": torch.zeros(flat[i][0]), "col": torch.zeros(flat[i][-1])} if len(flat[i]) == 2
                                    else {"v": torch.zeros(flat[i])})
            else:
                before_state.append({"row": st["exp_avg_sq_row"].clone(), "col": st["exp_avg_sq_col"].clone()} if len(flat[i]) == 2
                                    else {"v": st["exp_avg_sq"].clone()})
        for gi, grp in enumerate(opt.param_groups):
            grp["lr"] = LRS[gi][s - 1]
        opt.step()
        for i, p in enumerate(ps):
            arrays[f"p{s}_{i}"] = p.detach().clone()
            st = opt.state[p]
            arrays[f"step{s}_{i}"] = torch.tensor(st.get("step", 0))
            if p.grad is None:
                assert torch.equal(p.detach(), before[i])
            gi = 0 if i < n0 else 1
            if len(st):
                names = {"row": "exp_avg_sq_row", "col": "exp_avg_sq_col"} if len(flat[i]) == 2 else {"v": "exp_avg_sq"}
                for k, name in names.items():
                    if s == 2:
                        arrays[f"{k}{s}_{i}"] = st[name].clone()
            if p.grad is not None:
                p64, new = restate(before[i], p.grad, before_state[i], st["step"], LRS[gi][s - 1], WDS[gi])
                for k, v64 in new.items():
                    note(k, st[names[k]], v64)
                # the parameter delta (the parameter itself would hide errors); fp32 - fp32 in fp64 is exact
                note("delta", before[i].double() - p.detach().double(), before[i].double() - p64)
    for k, v in worst.items():
        arrays["dist_" + k] = torch.tensor(v, dtype=torch.float64)
    os.makedirs(GOLD, exist_ok=True)
    path = os.path.join(GOLD, "adafactor.npz")
    np.savez_compressed(path, **{k: v.detach().numpy() for k, v in arrays.items()})
    print("wrote", path, os.path.getsize(path), "bytes;", {k: ["%.2e" % x for x in v] for k, v in worst.items()})

    # the multiplier tables of all eight schedules, stepped like sched.json; tri_stage as trainer.py:585-586 calls it
    base_lr, train_steps, warmup, decay = 1e-3, 57, 0.1, 0.3
    out = {"base_lr": base_lr, "train_steps": train_steps, "warmup": warmup, "decay": decay, "lrs": {}}
    ref = {"linear": R.get_linear_schedule_with_warmup, "cosine": R.get_cosine_schedule_with_warmup,
           "cosine_with_restarts": R.get_cosine_with_hard_restarts_schedule_with_warmup,
           "polynomial": R.get_polynomial_decay_schedule_with_warmup, "constant": R.get_constant_schedule,
           "constant_with_warmup": R.get_constant_schedule_with_warmup,
           "inverse_sqrt": R.get_inverse_square_root_schedule_with_warmup, "tri_stage": R.get_tri_stage_schedule}
    for name, fn in ref.items():
        o = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=base_lr)
        if name == "constant":
            sch = fn(o)
        elif name == "constant_with_warmup":
            sch = fn(o, train_steps * warmup)
        elif name == "tri_stage":
            sch = fn(o, train_steps * warmup, train_steps * decay, train_steps)
        else:
            sch = fn(o, train_steps * warmup, train_steps)
        lrs = [o.param_groups[0]["lr"]]
        for _ in range(train_steps + 3):
            o.step()
            sch.step()
            lrs.append(o.param_groups[0]["lr"])
        out["lrs"][name] = lrs
    with open(os.path.join(GOLD, "sched_all.json"), "w") as f:
        json.dump(out, f)
    print("wrote sched_all.json")


if __name__ == "__main__":
    main()
