"""AdamW, Adafactor + LR schedules with the TencentPretrain call signatures, stepping on table-driven HIP kernels.

Drop-in for the symbols finetune/ppo.py uses from tencentpretrain/utils/optimizers.py of the reference:
`AdamW(params, lr, betas, eps, weight_decay, correct_bias)` (:305-402), `get_linear_schedule_with_warmup`
(:62-86), `get_constant_schedule(_with_warmup)` and the `str2optimizer` / `str2scheduler` registries.
The update is the reference's exactly (eps 1e-6 outside the sqrt, optional bias correction folded into the
step size, decoupled decay applied AFTER the Adam update with the same lr) but runs as ONE launch per
parameter group over a device-resident chunk table instead of ~5 small kernels per tensor.
`Adafactor` (:405-603) steps on lr2_adafactor_multi (four launches per group) for the arguments every launcher passes
(relative_step=False, scale_parameter=False, beta1=None); the eight schedules of `str2scheduler` are the reference's (:29-302).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Callable, Iterable, Tuple

import torch
from torch.optim import Optimizer
from torch.optim.lr_scheduler import LambdaLR

from ... import _native, ops

CHUNK_ELEMS = 1 << 18   # 1 MiB of fp32 per workgroup: 4000 workgroups for the 1.05 B parameters of actor+critic


class AdamW(Optimizer):
    def __init__(self, params: Iterable, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-6,
                 weight_decay: float = 0.0, correct_bias: bool = True):
        if lr < 0.0:
            raise ValueError("Invalid learning rate: {} - should be >= 0.0".format(lr))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter: {} - should be in [0.0, 1.0[".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter: {} - should be in [0.0, 1.0[".format(betas[1]))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {} - should be >= 0.0".format(eps))
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, correct_bias=correct_bias))
        self._tables = {}
        self._external = set()
        self._external_seen = set()     # ids of parameters ever updated through external_update
        self._lr_dev = None      # per group: float32[1] device tensor the kernels read the learning rate from (use_device_lr)
        self._max_norm = None    # set_grad_clip
        self._clip_out = None    # float32[2] on the device: total_norm, coefficient
        self._clip_slots = None  # float64: [CLIP_EXT slots of externally updated parameters | one partial per chunk]
        self._clip_ready = False
        self._ext_slot = {}      # id(p) -> slot of a parameter taken out of the next step() while clipping is on

    CLIP_EXT = 4                 # externally updated parameters per step that can owe a squared norm

    def set_grad_clip(self, max_norm):
        """Clip the global L2 norm of the gradients to `max_norm` in every later step(); None (or 0) switches it off again.
        The rule is torch.nn.utils.clip_grad_norm_'s (norm_type 2, error_if_nonfinite False) over exactly the parameters the next
        step() updates -- those with a gradient -- plus the parameters handed to external_update since the last step: one norm per
        optimizer, total_norm = sqrt(sum g^2), coef = min(1, max_norm / (total_norm + 1e-6)).  Norm, coefficient and the scaled
        update are device kernels (lr2_clip_sumsq / lr2_clip_coef / lr2_adamw_multi_scaled): nothing synchronises, a captured graph
        holds them as they are.  `.total_norm` and `.clip_coef` are float32[1] device tensors, valid after the step.
        The gradients IN MEMORY STAY UNSCALED: the kernels multiply on the fly, p.grad is what backward wrote.
        With external_update in play the caller stores the squared norm of that gradient in AdamArgs.norm_slot, calls
        clip_prepare(), runs the fused kernel (it reads AdamArgs.gscale_dev) and only then step()."""
        if max_norm is not None:
            max_norm = float(max_norm)
            if max_norm != max_norm or max_norm < 0.0 or max_norm == float("inf"):
                raise ValueError(f"set_grad_clip: max_norm must be a finite number >= 0 or None, got {max_norm}")
            if max_norm == 0.0:
                max_norm = None
        if self._external:
            raise RuntimeError("set_grad_clip: a fused update is pending (external_update without step())")
        self._max_norm = max_norm
        self._clip_ready = False

    @property
    def max_grad_norm(self):
        return self._max_norm

    def _clip_state(self):
        """(slots, out) on the parameters' device.  Sized once for every chunk table this optimizer can build (chunks hold at least
        2^13 elements), so the slot a fused update was promised never moves."""
        ps = [p for g in self.param_groups for p in g["params"]]
        dev = ps[0].device
        need = self.CLIP_EXT + sum(-(-p.numel() // (1 << 13)) for p in ps)
        if self._clip_slots is None or self._clip_slots.device != dev or self._clip_slots.numel() < need:
            if self._ext_slot:
                raise RuntimeError("AdamW: parameters changed while a fused update is pending")
            self._clip_slots = torch.zeros(need, dtype=torch.float64, device=dev)
            self._clip_out = torch.zeros(2, dtype=torch.float32, device=dev)
        return self._clip_slots, self._clip_out

    @property
    def total_norm(self):
        """float32[1] device tensor: the gradient norm the last step() measured (None while clipping is off)."""
        return None if self._max_norm is None else self._clip_state()[1][0:1]

    @property
    def clip_coef(self):
        """float32[1] device tensor: the coefficient the last step() multiplied its gradients by (None while clipping is off)."""
        return None if self._max_norm is None else self._clip_state()[1][1:2]

    @torch.no_grad()
    def clip_prepare(self):
        """Measure the norm and form the coefficient for the next step() (step() calls this itself unless a fused update is
        pending: its caller must, after filling AdamArgs.norm_slot and before launching the fused kernel)."""
        if self._max_norm is None:
            return None
        slots, out = self._clip_state()
        off = self.CLIP_EXT
        for gi, group in enumerate(self.param_groups):
            table, n, _, n_params = self._table(gi, group)
            if table is None:
                continue
            ops.clip_sumsq(table, n, slots[off:off + n], n_params=n_params)
            off += n
        first = self.CLIP_EXT - len(self._ext_slot)
        if off > first:
            ops.clip_coef(slots[first:off], off - first, self._max_norm, out)
        self._clip_ready = True
        return out[1:2]

    def _ensure_state(self, p):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = 0
            st["exp_avg"] = torch.zeros_like(p.data)
            st["exp_avg_sq"] = torch.zeros_like(p.data)
        return st

    def use_device_lr(self, tensors):
        """tensors: one float32[1] device tensor per param group (ops.StepScalars.lr_tensor), or None to go back to by-value
        learning rates.  While set, step() / external_update() launch kernels that read the rate from there -- a HIP graph
        captured around them follows the scheduler; the CALLER stores group["lr"] there before every step."""
        if tensors is not None and len(tensors) != len(self.param_groups):
            raise ValueError("use_device_lr: one tensor per param group")
        self._lr_dev = list(tensors) if tensors is not None else None

    def count_replayed_step(self):
        """Book-keeping of one step() that ran inside a replayed graph: per-parameter step counters and write marks."""
        ps = [p for g in self.param_groups for p in g["params"] if p.grad is not None or id(p) in self._external_seen]
        for p in ps:
            self._ensure_state(p)["step"] += 1
        ops.mark_params_written(ps)

    def external_update(self, p) -> "ops.AdamArgs":
        """Take parameter `p` out of the next step(): its update is done by a kernel that produces the gradient and
        applies this optimizer's rule in one pass (ops.gemm(adam=...), used for the 2 GB out_layer.fc1.weight).
        Returns the state tensors and the hyper-parameters the next step() would have used; p.grad is not read."""
        for gi, group in enumerate(self.param_groups):
            if any(q is p for q in group["params"]):
                break
        else:
            raise ValueError("external_update: parameter is not managed by this optimizer")
        if group["correct_bias"]:
            raise NotImplementedError("external_update needs correct_bias=False (what LR2PPO uses)")
        if p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous():
            raise RuntimeError("lr2ppo_amd AdamW needs contiguous float32 HIP parameters")
        gscale = slot = None
        if self._max_norm is not None:
            # clipping: the producer of this gradient owes its squared norm (AdamArgs.norm_slot) and scales by the coefficient
            if id(p) not in self._ext_slot and len(self._ext_slot) >= self.CLIP_EXT:
                raise RuntimeError(f"AdamW: at most {self.CLIP_EXT} fused updates per step while clipping is on")
            slots, out = self._clip_state()
            k = self._ext_slot.setdefault(id(p), len(self._ext_slot))
            slot, gscale = slots[self.CLIP_EXT - 1 - k:self.CLIP_EXT - k], out[1:2]
            self._clip_ready = False
        st = self._ensure_state(p)
        st["step"] += 1
        self._external.add(id(p))
        self._external_seen.add(id(p))
        return ops.AdamArgs(p.data, st["exp_avg"], st["exp_avg_sq"], group["lr"], group["betas"][0], group["betas"][1],
                            group["eps"], group["weight_decay"], lr_dev=self._lr_dev[gi] if self._lr_dev else None,
                            gscale_dev=gscale, norm_slot=slot)

    def _table(self, gi: int, group):
        ps = [p for p in group["params"] if p.grad is not None and id(p) not in self._external]
        if not ps:
            return None, 0, ps, 0
        # the table holds raw pointers: parameters, gradients AND both moment tensors (load_state_dict replaces the latter)
        sig = tuple((p.data_ptr(), p.grad.data_ptr(), p.numel(), self._ensure_state(p)["exp_avg"].data_ptr(),
                     self.state[p]["exp_avg_sq"].data_ptr()) for p in ps)
        gi = (gi, len(ps))        # separate cached tables with / without externally updated parameters
        cached = self._tables.get(gi)
        if cached is not None and cached[0] == sig:
            return cached[1], cached[2], ps, cached[3]
        rows = []
        # one workgroup per chunk: keep >= ~2000 workgroups in flight even when the group is small (the 20 M parameters
        # left after out_layer.fc1.weight is updated inside its GEMM would otherwise run on 90 workgroups)
        total = sum(p.numel() for p in ps)
        chunk_elems = min(CHUNK_ELEMS, max(1 << 13, (-(-total // 2048) + 1023) // 1024 * 1024))
        for p in ps:
            if p.grad.is_sparse:
                raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
            if p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous() or not p.grad.is_contiguous():
                raise RuntimeError("lr2ppo_amd AdamW needs contiguous float32 HIP parameters and gradients")
            st = self._ensure_state(p)
            n, off = p.numel(), 0
            while off < n:
                c = min(chunk_elems, n - off)
                rows.append((p.data_ptr() + 4 * off, p.grad.data_ptr() + 4 * off, st["exp_avg"].data_ptr() + 4 * off,
                             st["exp_avg_sq"].data_ptr() + 4 * off, c, group["weight_decay"]))
                off += c
        arr = (_native.AdamChunk * len(rows))()
        for i, (a, b, c_, d, cnt, wd) in enumerate(rows):
            arr[i].p, arr[i].g, arr[i].m, arr[i].v, arr[i].count, arr[i].weight_decay = a, b, c_, d, cnt, wd
        dev = ps[0].device
        table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
        self._tables[gi] = (sig, table, len(rows), sum(p.numel() for p in ps))
        return table, len(rows), ps, self._tables[gi][3]

    @torch.no_grad()
    def step(self, closure: Callable = None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        clip = self._max_norm is not None
        if clip and not self._clip_ready:
            if self._ext_slot:
                raise RuntimeError("AdamW.step: clipping is on and a fused update is pending -- call clip_prepare() after its "
                                   "squared norm is in AdamArgs.norm_slot and before the fused kernel")
            self.clip_prepare()
        for gi, group in enumerate(self.param_groups):
            table, n, ps, n_params = self._table(gi, group)
            if table is None:
                continue
            beta1, beta2 = group["betas"]
            step_size = group["lr"]
            for p in ps:
                self.state[p]["step"] += 1
            if group["correct_bias"]:
                t = self.state[ps[0]]["step"]
                step_size = step_size * math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
                if group["weight_decay"] > 0.0 and step_size != group["lr"]:
                    # decay must use the raw lr (optimizers.py:399-400): run the decay-free update, then decay
                    raise NotImplementedError("correct_bias=True with weight decay is not used by LR2PPO")
            lr_dev = self._lr_dev[gi] if self._lr_dev else None
            if lr_dev is not None and group["correct_bias"]:
                raise NotImplementedError("device learning rates need correct_bias=False (what LR2PPO uses)")
            if clip:
                ops.adamw_multi_scaled(table, n, step_size, beta1, beta2, group["eps"], self._clip_out[1:2], n_params=n_params,
                                       lr_dev=lr_dev)
            else:
                ops.adamw_multi(table, n, step_size, beta1, beta2, group["eps"], n_params=n_params, lr_dev=lr_dev)
            ops.mark_params_written(ps)
        if self._external:          # parameters a fused kernel updated since the last step (external_update)
            ops.mark_params_written([p for g_ in self.param_groups for p in g_["params"] if id(p) in self._external])
        self._external.clear()
        self._ext_slot.clear()
        self._clip_ready = False
        return loss


def adafactor_plan(shapes):
    """The tables of one lr2_adafactor_multi call for tensors of these shapes (1-D or 2-D), as plain Python:
    -> (per-tensor dicts, tiles [(tensor, index)], fin [(tensor, kind, start)], workspace bytes).
    A 2-D tensor is cut into TILE_ROWS x TILE_COLS tiles in row-major tile order, a 1-D one into CHUNK_1D chunks.  The workspace
    holds, per tensor, one fp64 sum-of-U^2 partial per tile (all of these first: 8-byte aligned), and per 2-D tensor the fp32 row
    partials [col tiles][rows], the fp32 column partials [row tiles][cols] and mean(row).  Offsets are in bytes."""
    TR, TC, CH, FC = (_native.ADAFACTOR_TILE_ROWS, _native.ADAFACTOR_TILE_COLS, _native.ADAFACTOR_CHUNK_1D,
                      _native.ADAFACTOR_FIN_COLS)
    tensors, tiles, fin = [], [], []
    off = 0
    for ti, shape in enumerate(shapes):
        if len(shape) == 2:
            rows, cols = shape
            n_rt, n_ct = -(-rows // TR), -(-cols // TC)
            n = n_rt * n_ct
        elif len(shape) == 1:
            rows, cols, n_rt, n_ct = 0, shape[0], 0, 0
            n = -(-cols // CH)
        else:
            raise NotImplementedError(f"Adafactor steps 1-D and 2-D parameters, got shape {tuple(shape)}")
        if cols < 1 or (len(shape) == 2 and rows < 1):
            raise ValueError(f"Adafactor: empty parameter of shape {tuple(shape)}")
        tensors.append(dict(rows=rows, cols=cols, n_tiles=n, n_row_tiles=n_rt, n_col_tiles=n_ct, ws_sq=off, ws_row=0, ws_col=0,
                            ws_mean=0))
        off += 8 * n
        tiles += [(ti, i) for i in range(n)]
        if rows:
            fin.append((ti, 0, 0))
            fin += [(ti, 1, s) for s in range(0, cols, FC)]
    for t in tensors:
        if t["rows"]:
            t["ws_row"] = off
            off += 4 * t["n_col_tiles"] * t["rows"]
            t["ws_col"] = off
            off += 4 * t["n_row_tiles"] * t["cols"]
            t["ws_mean"] = off
            off += 4
    return tensors, tiles, fin, off


class Adafactor(Optimizer):
    """The reference's Adafactor (tencentpretrain/utils/optimizers.py:405-603; constructor signature, defaults and state keys are
    its own) stepping on lr2_adafactor_multi: four launches per param group whatever the number of tensors, no host
    synchronisation.  The device path serves what every launcher passes -- an external learning rate without a first moment:
    relative_step=False, scale_parameter=False, beta1=None -- and 1-D / 2-D parameters; anything else raises at construction.
    State per parameter: `step`, `exp_avg_sq_row` [R] / `exp_avg_sq_col` [C] (2-D) or `exp_avg_sq` (1-D), and `RMS`.  `RMS` is
    kept for the layout of a reference-written state only and holds 0: the reference reads it under scale_parameter=True alone.
    There is no external_update: the heads' step functions then take the unfused out_layer.fc1 route on their own."""

    def __init__(self, params, lr=None, eps=(1e-30, 1e-3), clip_threshold=1.0, decay_rate=-0.8, beta1=None, weight_decay=0.0,
                 scale_parameter=True, relative_step=True, warmup_init=False):
        if lr is not None and relative_step:
            raise ValueError("Cannot combine manual lr and relative_step options")
        if warmup_init and not relative_step:
            raise ValueError("warmup_init requires relative_step=True")
        if relative_step or scale_parameter or beta1 is not None:
            raise NotImplementedError("lr2ppo_amd Adafactor serves relative_step=False, scale_parameter=False, beta1=None with an "
                                      "external lr (what every LR2PPO launcher passes); got "
                                      f"relative_step={relative_step}, scale_parameter={scale_parameter}, beta1={beta1}")
        if lr is None:
            raise NotImplementedError("lr2ppo_amd Adafactor needs an external lr (relative_step=False)")
        super().__init__(params, dict(lr=lr, eps=eps, clip_threshold=clip_threshold, decay_rate=decay_rate, beta1=beta1,
                                      weight_decay=weight_decay, scale_parameter=scale_parameter, relative_step=relative_step,
                                      warmup_init=warmup_init))
        for group in self.param_groups:
            for p in group["params"]:
                if p.dim() not in (1, 2):
                    raise NotImplementedError(f"lr2ppo_amd Adafactor steps 1-D and 2-D parameters, got shape {tuple(p.shape)} "
                                              "(the reference's _approx_sq_grad is a torch.mm and cannot step it either)")
        self._tables = {}

    def _ensure_state(self, p):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = 0
            if p.dim() == 2:
                st["exp_avg_sq_row"] = torch.zeros(p.shape[0], dtype=torch.float32, device=p.device)
                st["exp_avg_sq_col"] = torch.zeros(p.shape[1], dtype=torch.float32, device=p.device)
            else:
                st["exp_avg_sq"] = torch.zeros_like(p.data)
            st["RMS"] = 0
        return st

    def _moments(self, p):
        st = self._ensure_state(p)
        ms = (st["exp_avg_sq_row"], st["exp_avg_sq_col"]) if p.dim() == 2 else (st["exp_avg_sq"],)
        want = ((p.shape[0],), (p.shape[1],)) if p.dim() == 2 else (tuple(p.shape),)
        for m, w in zip(ms, want):
            if m.dtype != torch.float32 or m.device != p.device or not m.is_contiguous() or tuple(m.shape) != w:
                raise RuntimeError("lr2ppo_amd Adafactor needs contiguous float32 HIP state tensors of the parameter's row / column shape")
        return ms

    MAX_TABLES = 8      # cached (tables, workspace) entries; the oldest goes first

    def _table(self, gi: int, group, ps):
        """Device tables and workspace of one call over `ps`, cached per (group, set of parameters) with the raw pointers as the
        entry's signature.  As with AdamW._tables, a pointer that changes -- zero_grad(set_to_none=True) followed by a freshly
        allocated gradient, load_state_dict -- rebuilds the entry, and the rebuild is a blocking host-to-device copy of pageable
        memory inside step(): keep gradients in place (bind_grads does) to stay asynchronous.  Every entry owns a workspace (5.9 MB
        for a head), so at most MAX_TABLES are kept: a group whose skip pattern varies (pointwise_2data_trad: two patterns) stays
        within that."""
        # the tables hold raw pointers: parameters, gradients AND the state vectors (load_state_dict replaces the latter)
        sig = tuple((p.data_ptr(), p.grad.data_ptr(), tuple(p.shape), group["weight_decay"]) + tuple(m.data_ptr() for m in self._moments(p))
                    for p in ps)
        key = (gi,) + tuple(id(p) for p in ps)
        cached = self._tables.get(key)
        if cached is not None and cached[0] == sig:
            return cached[1]
        tensors, tiles, fin, ws_bytes = adafactor_plan([tuple(p.shape) for p in ps])
        dev = ps[0].device
        tarr = (_native.AdafactorTensor * len(ps))()
        n_bytes = 0.0
        for i, (p, t) in enumerate(zip(ps, tensors)):
            ms = self._moments(p)
            a = tarr[i]
            a.p, a.g, a.row, a.col = p.data_ptr(), p.grad.data_ptr(), ms[0].data_ptr(), ms[1].data_ptr() if len(ms) == 2 else None
            a.rows, a.cols, a.n_tiles, a.n_col_tiles, a.n_row_tiles = t["rows"], t["cols"], t["n_tiles"], t["n_col_tiles"], t["n_row_tiles"]
            a.ws_row, a.ws_col, a.ws_mean, a.ws_sq = t["ws_row"], t["ws_col"], t["ws_mean"], t["ws_sq"]
            a.weight_decay = group["weight_decay"]
            n_bytes += (20.0 if t["rows"] else 28.0) * p.numel()
        larr = (_native.AdafactorTile * len(tiles))()
        for i, (ti, idx) in enumerate(tiles):
            larr[i].tensor, larr[i].index = ti, idx
        farr = (_native.AdafactorFin * max(1, len(fin)))()
        for i, (ti, kind, start) in enumerate(fin):
            farr[i].tensor, farr[i].kind, farr[i].start = ti, kind, start
        up = lambda arr: torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)      # noqa: E731
        entry = dict(tensors=up(tarr), tiles=up(larr), n_tiles=len(tiles), fin=up(farr) if fin else None, n_fin=len(fin),
                     ws=torch.empty((ws_bytes + 7) // 8, dtype=torch.float64, device=dev), n_params=sum(p.numel() for p in ps),
                     n_bytes=n_bytes)
        self._tables.pop(key, None)
        while len(self._tables) >= self.MAX_TABLES:
            self._tables.pop(next(iter(self._tables)))
        self._tables[key] = (sig, entry)
        return entry

    @torch.no_grad()
    def step(self, closure: Callable = None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # everything is checked before any launch and before any step count moves: a refusal leaves the optimizer as it was
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("Adafactor does not support sparse gradients.")
                if p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous() or not p.grad.is_contiguous() \
                        or p.grad.dtype != torch.float32:
                    raise RuntimeError("lr2ppo_amd AdamW needs contiguous float32 HIP parameters and gradients")
                self._moments(p)
        for gi, group in enumerate(self.param_groups):
            ps = [p for p in group["params"] if p.grad is not None]      # a parameter without a gradient is skipped: no step, no decay
            # beta2t = 1 - step^decay_rate travels by value, one per call: parameters that skipped steps (pointwise_2data_trad's
            # unused projection) go in a call of their own, so a group costs ADAFACTOR_LAUNCHES launches per distinct step count
            by_step = {}
            for p in ps:
                st = self._ensure_state(p)
                st["step"] += 1
                by_step.setdefault(st["step"], []).append(p)
            for t, sub in by_step.items():
                e = self._table(gi, group, sub)
                beta2t = 1.0 - math.pow(t, group["decay_rate"])
                ops.adafactor_multi(e["tensors"], e["tiles"], e["n_tiles"], e["fin"], e["n_fin"], e["ws"], group["lr"], beta2t,
                                    group["eps"][0], group["clip_threshold"], n_params=e["n_params"], n_bytes=e["n_bytes"])
            ops.mark_params_written(ps)
        return loss


def get_constant_schedule(optimizer, last_epoch=-1):
    return LambdaLR(optimizer, lambda _: 1, last_epoch=last_epoch)


def get_constant_schedule_with_warmup(optimizer, num_warmup_steps, last_epoch=-1):
    def lr_lambda(current_step):
        if current_step < num_warmup_steps:
            return float(current_step) / float(max(1.0, num_warmup_steps))
        return 1.0
    return LambdaLR(optimizer, lr_lambda, last_epoch=last_epoch)


def get_linear_schedule_with_warmup(optimizer, num_warmup_steps, num_training_steps, last_epoch=-1):
    """lambda(s) = s/warm for s < warm, then linear decay to 0 at num_training_steps.  lambda(0) = 0, so an
    optimizer used before the first scheduler.step() runs at lr 0 -- finetune/ppo.py steps its schedulers once
    per train_model call, hence the whole first PPO cycle trains at lr 0."""
    def lr_lambda(current_step: int):
        if current_step < num_warmup_steps:
            return float(current_step) / float(max(1, num_warmup_steps))
        return max(0.0, float(num_training_steps - current_step) / float(max(1, num_training_steps - num_warmup_steps)))
    return LambdaLR(optimizer, lr_lambda, last_epoch)


# The five schedules below give the reference's multipliers (tests/golden/sched_all.json to 1e-12: the same floating-point
# operations in the same order) behind its signatures and defaults (optimizers.py:89-302); the text is this project's.
def _ramp(step, warm):
    """Share of a linear warm-up from 0 that `step` has covered."""
    return float(step) / float(max(1, warm))


def _after_warmup(step, warm, total):
    """Share of the steps between the warm-up's end and `total` that `step` has covered."""
    return float(step - warm) / float(max(1, total - warm))


def get_tri_stage_schedule(optimizer, num_warmup_steps, num_decay_steps, num_training_steps, init_lr_scale=0.01, final_lr_scale=0.05,
                           last_epoch=-1):
    """Three stages (arXiv 1904.08779): a linear rise from init_lr_scale to 1 over the warm-up, 1 until num_decay_steps before the
    end, then an exponential fall that reaches final_lr_scale at num_training_steps and stays there."""
    peak = optimizer.defaults["lr"]
    first, last = peak * init_lr_scale, peak * final_lr_scale
    fall_from = num_training_steps - num_decay_steps

    def multiplier(step):
        if step < num_warmup_steps:
            per_step = (peak - first) / num_warmup_steps
            return (first + step * per_step) / peak
        if step < fall_from:
            return 1
        if step > num_training_steps:
            return last / peak
        rate = -math.log(final_lr_scale) / max(num_decay_steps, 1)
        return math.exp(-rate * (step - num_training_steps + num_decay_steps))
    return LambdaLR(optimizer, multiplier, last_epoch)


def get_cosine_schedule_with_warmup(optimizer, num_warmup_steps, num_training_steps, num_cycles=0.5, last_epoch=-1):
    """Linear warm-up from 0, then num_cycles periods of a cosine between 1 and 0 (the default half period ends at 0)."""
    def multiplier(step):
        if step < num_warmup_steps:
            return _ramp(step, num_warmup_steps)
        angle = math.pi * float(num_cycles) * 2.0 * _after_warmup(step, num_warmup_steps, num_training_steps)
        return max(0.0, 0.5 * (1.0 + math.cos(angle)))
    return LambdaLR(optimizer, multiplier, last_epoch)


def get_cosine_with_hard_restarts_schedule_with_warmup(optimizer, num_warmup_steps, num_training_steps, num_cycles=1, last_epoch=-1):
    """Linear warm-up from 0, then num_cycles half cosines from 1 to 0, each starting again at 1; 0 from num_training_steps on."""
    def multiplier(step):
        if step < num_warmup_steps:
            return _ramp(step, num_warmup_steps)
        done = _after_warmup(step, num_warmup_steps, num_training_steps)
        if done >= 1.0:
            return 0.0
        within_cycle = (float(num_cycles) * done) % 1.0
        return max(0.0, 0.5 * (1.0 + math.cos(math.pi * within_cycle)))
    return LambdaLR(optimizer, multiplier, last_epoch)


def get_polynomial_decay_schedule_with_warmup(optimizer, num_warmup_steps, num_training_steps, lr_end=1e-7, power=1.0, last_epoch=-1):
    """Linear warm-up from 0, then (share of the decay steps left) ** power between the optimizer's lr and lr_end; lr_end past
    num_training_steps.  The multiplier is the target rate over the optimizer's lr."""
    top = optimizer.defaults["lr"]
    if not top > lr_end:
        raise AssertionError(f"polynomial schedule: lr_end {lr_end} is not below the optimizer's lr {top}")

    def multiplier(step):
        if step < num_warmup_steps:
            return _ramp(step, num_warmup_steps)
        if step > num_training_steps:
            return lr_end / top
        left = 1 - (step - num_warmup_steps) / (num_training_steps - num_warmup_steps)
        return ((top - lr_end) * left ** power + lr_end) / top
    return LambdaLR(optimizer, multiplier, last_epoch)


def get_inverse_square_root_schedule_with_warmup(optimizer, num_warmup_steps, num_training_steps, warmup_init_lr=0.0, last_epoch=-1):
    """Linear warm-up from warmup_init_lr to the optimizer's lr, then lr * sqrt(num_warmup_steps / step); a rate of 1e-7 past
    num_training_steps."""
    top = optimizer.defaults["lr"]
    if not top > warmup_init_lr:
        raise AssertionError(f"inverse-sqrt schedule: warmup_init_lr {warmup_init_lr} is not below the optimizer's lr {top}")

    def multiplier(step):
        if step < num_warmup_steps:
            per_step = (top - warmup_init_lr) / num_warmup_steps
            return (warmup_init_lr + step * per_step) / top
        if step > num_training_steps:
            return 1e-7 / top
        return (top * num_warmup_steps ** 0.5 * step ** -0.5) / top
    return LambdaLR(optimizer, multiplier, last_epoch)


def apply_grad_clip(args, *optimizers):
    """--max_grad_norm X of the training launchers (a flag of this build; 0 = off, the default): every optimizer clips the global L2
    norm of its own parameter list to X (AdamW.set_grad_clip), as one torch.nn.utils.clip_grad_norm_ call per optimizer would.
    Adafactor gets no clip and the combination is refused: its update is invariant to the gradient's scale down to eps[0], and it
    clips its own update (clip_threshold)."""
    max_norm = float(getattr(args, "max_grad_norm", 0.0) or 0.0)
    if max_norm != max_norm or max_norm < 0.0:
        raise ValueError(f"--max_grad_norm must be >= 0 (0 = off), got {max_norm}")
    if max_norm == 0.0:
        return
    for o in optimizers:
        if not isinstance(o, AdamW):
            raise ValueError("--max_grad_norm needs --optimizer adamw: Adafactor's update is invariant to the gradient's scale (down "
                             "to eps[0]) and it clips its own update (clip_threshold), so it gets no gradient-norm clip")
    for o in optimizers:
        o.set_grad_clip(max_norm)


str2optimizer = {"adamw": AdamW, "adafactor": Adafactor}
str2scheduler = {"linear": get_linear_schedule_with_warmup, "cosine": get_cosine_schedule_with_warmup,
                 "cosine_with_restarts": get_cosine_with_hard_restarts_schedule_with_warmup,
                 "polynomial": get_polynomial_decay_schedule_with_warmup, "constant": get_constant_schedule,
                 "constant_with_warmup": get_constant_schedule_with_warmup,
                 "inverse_sqrt": get_inverse_square_root_schedule_with_warmup, "tri_stage": get_tri_stage_schedule}
