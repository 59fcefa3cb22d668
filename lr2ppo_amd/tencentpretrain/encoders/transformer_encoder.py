"""TransformerEncoder.forward(emb, seg) -> hidden on the gfx950 kernels (inference schedule).

Mirrors the reference's encoders/transformer_encoder.py:7-138 + layers/transformer.py:50-73 for
mask="fully_visible": additive key mask -10000 * (seg <= 0) applied AFTER the 1/sqrt(64) scale, post-LN
(RoBERTa-base) or pre-LN + final LayerNorm (ViT-B/16), exact-erf GELU, TencentPretrain LayerNorm semantics.

Per layer: ONE fused QKV GEMM (N = 3*hidden, weights concatenated once), the MFMA self-attention kernel, the output
projection (+residual), FFN1 (+GELU), FFN2 (+residual) and 2 wavefront LayerNorms.  Everything a GEMM consumes travels as
bf16 hi/lo planes written by the producing kernel (LayerNorm, attention, GEMM epilogue) and is streamed by LDS-DMA; the
residual stream stays fp32.  Weight planes are split once and re-split only when a parameter changes.
With autograd enabled (train mode or parameters that require grad) the same kernels run a saving schedule and a
hand-written backward (`_EncoderFn`): MFMA attention backward with recomputed probabilities, TencentPretrain-LayerNorm
backward, dgrad / wgrad GEMMs with fused GELU' and residual epilogues, dropout at the reference's three sites per layer
(attention probabilities, dropout_1, dropout_2) from the counter-based mask stream of lr2ppo_amd.runtime."""
import math
import os

import torch
import torch.nn as nn

from ... import engine, ops, runtime
from ..layers.layer_norm import LayerNorm
from ..layers.transformer import TransformerLayer


class _LayerPlanes(dict):
    """One layer's GEMM operands; `wqkv_f32`, `wqkv_t`, `w1_t` are produced on first access after a refresh."""

    def __missing__(self, key):
        if key == "wqkv_f32":
            v = torch.cat([lin.weight.data for lin in self._qkv], dim=0, out=self._f32)
        elif key == "wqkv_t":
            v = ops.split_planes_t(self["wqkv_f32"], self._t_qkv)
        elif key == "w1_t":
            v = ops.split_planes_t(self._w1.data.contiguous(), self._t_w1)
        else:
            raise KeyError(key)
        self[key] = v
        return v


class _StackPlanes:
    """bf16 hi / lo planes of every GEMM weight of an encoder stack in one buffer + the device table that re-splits them from the
    fp32 parameters in one launch (lr2_split_planes_multi).  Wq, Wk, Wv are split straight into the row blocks of one [3E, E] planes
    matrix (hi plane of all three, then lo plane): no fp32 concatenation on the forward path."""
    CHUNK = 1 << 16
    LAZY = ("wqkv_f32", "wqkv_t", "w1_t")

    def __init__(self, enc, dev):
        layers = list(enc.transformer)
        E = layers[0].self_attn.final_linear.out_features
        F = layers[0].feed_forward.linear_1.out_features
        per = 3 * E * E + E * E + 2 * E * F
        self.dev = dev
        self.buf = torch.empty(2 * per * len(layers), dtype=torch.int16, device=dev)
        self.ptrs = tuple(p.data_ptr() for p in enc.parameters())
        self.layers, rows, cur = [], [], 0
        base = self.buf.data_ptr()

        def add(sources, nrows, ncols):
            nonlocal cur
            n = nrows * ncols
            pl = ops.Planes(self.buf[cur:cur + 2 * n], nrows, ncols)
            r0 = 0
            for w in sources:
                if w.dim() != 2 or w.shape[1] != ncols or not w.is_contiguous() or w.numel() % 4:
                    raise ValueError("encoder GEMM weights must be contiguous 2-D fp32 tensors")
                k, o = w.numel(), 0
                while o < k:
                    c = min(self.CHUNK, k - o)
                    rows.append((w.data_ptr() + 4 * o, base + 2 * (cur + r0 * ncols + o), n, c))
                    o += c
                r0 += w.shape[0]
            cur += 2 * n
            return pl

        for layer in layers:
            att, ffn = layer.self_attn, layer.feed_forward
            ent = _LayerPlanes()
            ent["wqkv"] = add([att.linear_layers[i].weight.data for i in range(3)], 3 * E, E)
            ent["wo"] = add([att.final_linear.weight.data], E, E)
            ent["w1"] = add([ffn.linear_1.weight.data], F, E)
            ent["w2"] = add([ffn.linear_2.weight.data], E, F)
            ent["bqkv"] = torch.empty(3 * E, device=dev)
            ent._qkv, ent._w1 = [att.linear_layers[i] for i in range(3)], ffn.linear_1.weight
            ent._f32 = torch.empty(3 * E, E, device=dev)
            ent._t_qkv, ent._t_w1 = ops.Planes.empty(E, 3 * E, dev), ops.Planes.empty(E, F, dev)
            self.layers.append(ent)
        import ctypes as C  # noqa: F401
        from ... import _native
        arr = (_native.SplitChunk * len(rows))()
        for i, (src, dst, lo, cnt) in enumerate(rows):
            arr[i].src, arr[i].dst_hi, arr[i].lo_off, arr[i].count = src, dst, lo, cnt
        self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
        self.n_chunks = len(rows)
        self.sig = None

    @staticmethod
    def signature(enc):
        return tuple((p._version, ops.param_write_count(p)) for p in enc.parameters())

    def matches(self, enc, dev) -> bool:
        return self.dev == dev and self.ptrs == tuple(p.data_ptr() for p in enc.parameters())

    def refresh(self, enc):
        ops.split_planes_multi(self.table, self.n_chunks)
        for ent in self.layers:
            for k in self.LAZY:
                ent.pop(k, None)
            torch.cat([lin.bias.data for lin in ent._qkv], dim=0, out=ent["bqkv"])
        self.sig = self.signature(enc)


class _Kept:
    """Where a training layer's tensors go when the backward reads them from the forward: carved from one Arena (split-bf16; the
    names are unused, the order of the calls is the layout), or a fresh tensor each (no arena: MX-FP8)."""

    def __init__(self, dev, arena=None):
        self.dev, self.arena = dev, arena

    def mat(self, name, rows, cols):
        return self.arena.mat(rows, cols) if self.arena is not None else torch.empty(rows, cols, device=self.dev)

    def vec(self, name, numel):
        return self.arena.vec(numel) if self.arena is not None else torch.empty(numel, device=self.dev)

    def planes(self, name, rows, cols):
        return self.arena.planes(rows, cols) if self.arena is not None else ops.Planes.empty(rows, cols, self.dev)

    def plane(self, name, rows, cols):                                   # ONE bf16 plane (the bf16_train mode)
        return self.arena.plane(rows, cols) if self.arena is not None else torch.empty(rows * cols, dtype=torch.int16, device=self.dev)

    def mx_t(self, name, rows, cols):
        return None                                                      # quant_mxfp8_t allocates the column-blocked copy


class _Reused:
    """The same tensors as named workspace buffers, reused by every layer and every step: a forward nothing reads afterwards, or a
    layer recomputed right in front of its backward.  out: the _Kept that holds the layer output (`hn*`) instead -- the recomputing
    forward keeps it as the next layer's input."""

    def __init__(self, enc, dev, prefix, out=None):
        self.enc, self.dev, self.prefix, self.out = enc, dev, prefix, out

    def mat(self, name, rows, cols):
        if self.out is not None and name.startswith("hn"):
            return self.out.mat(name, rows, cols)
        return self.enc._ws.mat(self.prefix + name, rows, cols)

    def vec(self, name, numel):
        return self.enc._ws.vec(self.prefix + name, numel)

    def planes(self, name, rows, cols):
        return self.enc._ws.planes(self.prefix + name, rows, cols)

    def plane(self, name, rows, cols):
        return self.enc._ws.plane(self.prefix + name, rows, cols)

    def mx_t(self, name, rows, cols):
        return self.enc._mx(self.prefix + name, rows, cols, self.dev)


class TransformerEncoder(nn.Module):
    # True: the training schedule (and, for bit-identical features, every forward) runs the four projections of every layer as MX-FP8
    # products, forward and backward (_forward_train_fp8 / _backward_train_fp8; FeatureExtractor(precision="mxfp8_train"))
    fp8_train = False
    # True: the training forward keeps each layer's INPUT only; the backward re-runs layer i's forward (same dropout seed and sites, same
    # weight operands: the same bits) into reused workspace buffers right before layer i's backward
    recompute = False
    # True: the training schedule (and every forward) runs the four projections of every layer as ONE bf16 pass, forward, input gradient
    # and weight gradient (_forward_train_bf16 / _backward_train_bf16; FeatureExtractor(precision="bf16_train"))
    bf16_train = False
    # True (with bf16_train): a layer with head_dim 64 and L <= 288 runs its attention core on ONE bf16 plane per operand, forward and
    # backward (ops.self_attn_fwd_bf16_train / ops.self_attn_bwd_bf16; FeatureExtractor(..., bf16_attention=True)); every
    # other layer shape keeps the 3-pass kernels
    bf16_attention = False
    # True (with bf16_attention): a layer with head_dim 64 and L > 288 takes the single-plane attention too, on the key- / query-blocked
    # kernels of csrc/selfattn_b1_blocked.hip (the same ops calls; FeatureExtractor(..., bf16_attention_long=True))
    bf16_attention_long = False
    # True: the two inference-only schedules (forward_bf16, forward_fp8) run a layer with head_dim 64 and L > 288 on ONE bf16 plane per
    # operand too, on the key-blocked kernel of csrc/selfattn_mx_blocked.hip (ops.self_attn_fwd_bf16_blocked;
    # FeatureExtractor(precision="bf16" | "mxfp8", attention_long=True)); off: the 3-pass attention kernels above 288
    infer_attention_long = False
    # True: the f16 inference schedule (forward_f16) runs a layer with head_dim 64 and L > 288 on ONE f16 plane per operand too, on the
    # key-blocked kernel of csrc/selfattn_mx_blocked.hip (ops.self_attn_fwd_f16_blocked; FeatureExtractor(precision="f16",
    # f16_attention_long=True)); off: the 3-pass attention kernels above 288
    f16_attention_long = False

    def __init__(self, args):
        super().__init__()
        self.mask = args.mask
        self.layers_num = args.layers_num
        self.layernorm_positioning = args.layernorm_positioning
        self.heads_num, self.hidden_size = args.heads_num, args.hidden_size
        unsupported = [k for k in ("parameter_sharing", "factorized_embedding_parameterization", "relative_position_embedding",
                                   "has_residual_attention") if getattr(args, k, False)]
        if unsupported or self.mask != "fully_visible":
            raise NotImplementedError(f"HIP TransformerEncoder: unsupported options {unsupported or self.mask}")
        self.transformer = nn.ModuleList([TransformerLayer(args) for _ in range(self.layers_num)])
        self.final_layernorm = self.layernorm_positioning == "pre"       # transformer_encoder.py:36-37,134-135 upstream
        if self.final_layernorm:
            self.layer_norm = LayerNorm(args.hidden_size)
        self._ws = None
        self._wplanes = None

    def _weight_planes(self, dev, cache=True):
        """Per layer a dict: Wqkv planes [3E, E] (rows Q | K | V), bqkv [3E], Wo, W1, W2 planes -- and, computed on first use after
        a refresh, the fp32 concatenation `wqkv_f32` (large-M input gradients transpose it) and the transposed planes `wqkv_t` /
        `w1_t` (the NN form of the forward on small batches).  All planes of the stack live in ONE buffer and are re-split from the
        fp32 parameters by ONE multi-tensor launch (round 3; rounds 1-2: 2 concatenations + 6 allocations + 6 split launches per layer
        and forward); re-split when any parameter was written (torch's version counters + the per-parameter write counters the HIP
        optimizer bumps: its kernels write through raw pointers).  cache=False (training): always re-split."""
        sp = self._wplanes
        if sp is None or not sp.matches(self, dev):
            sp = self._wplanes = _StackPlanes(self, dev)
            fresh = False
        else:
            fresh = cache and sp.sig == sp.signature(self)
        if not fresh:
            sp.refresh(self)
        return sp.layers

    def forward(self, emb, seg):
        if emb.dtype != torch.float32 or not emb.is_cuda:
            raise TypeError("lr2ppo_amd: emb must be a float32 tensor on the HIP device (no CPU path)")
        needs_grad = torch.is_grad_enabled() and (emb.requires_grad or any(p.requires_grad for p in self.parameters()))
        if needs_grad:
            return _EncoderFn.apply(self, emb, seg, *list(self.parameters()))
        if self.fp8_train:
            return self._forward_train_fp8(emb, seg, save=False)[0]      # no backward follows: nothing kept, no x^T written
        if self.bf16_train:
            return self._forward_train_bf16(emb, seg, save=False)[0]
        if self.training and any(l.dropout_1.p > 0 for l in self.transformer):
            out, _ = self._forward_train(emb, seg)       # dropout without a graph (torch.no_grad() in train mode)
            return out
        return self._forward_infer(emb, seg)

    def forward_first_token(self, emb, seg):
        """hidden[:, 0, :] of forward(emb, seg), [batch, hidden] -- for callers that pool with 'first' (utils/misc.py:23-35
        upstream; the image encoder in front of the heads, finetune/ppo.py:120-127).  In inference the LAST layer then needs
        its keys and values for every row but its query, output projection and feed-forward for row 0 only: 5/6 of that
        layer's matrix work is never consumed and is not computed.  With gradients enabled: the full forward, sliced."""
        needs_grad = torch.is_grad_enabled() and (emb.requires_grad or any(p.requires_grad for p in self.parameters()))
        if needs_grad or self.fp8_train or self.bf16_train or (self.training and any(l.dropout_1.p > 0 for l in self.transformer)):
            return self.forward(emb, seg)[:, 0, :]
        if emb.dtype != torch.float32 or not emb.is_cuda:
            raise TypeError("lr2ppo_amd: emb must be a float32 tensor on the HIP device (no CPU path)")
        return self._forward_infer(emb, seg, first_only=True)

    @torch.no_grad()
    def _forward_infer(self, emb, seg, first_only=False):
        B, L, E = emb.shape
        H, hd = self.heads_num, E // self.heads_num
        if first_only and hd != 64:                                   # lr2_first_token_attn is built for head width 64: the full
            return self._forward_infer(emb, seg)[:, 0, :].contiguous()  # last layer, sliced (as forward_bf16 does)
        M = B * L
        if self._ws is None or self._ws.device != emb.device:
            self._ws = engine.Workspace(emb.device)
        ws = self._ws
        seg = seg.to(device=emb.device, dtype=torch.int64).contiguous().view(-1)
        W = self._weight_planes(emb.device)
        h, h2 = ws.mat("h", M, E), ws.mat("h2", M, E)
        h.copy_(emb.contiguous().view(M, E))
        pre = self.layernorm_positioning == "pre"
        F = self.transformer[0].feed_forward.linear_1.out_features
        x_p, t_p = ws.planes("x_p", M, E), ws.planes("t_p", M, E)        # GEMM inputs: LN outputs / hidden
        qkv_p, o_p, ff_p = ws.planes("qkv_p", M, 3 * E), ws.planes("o_p", M, E), ws.planes("ff_p", M, F)
        scale = 1.0 / math.sqrt(float(hd))
        # wide outputs: NT on the weight's own layout when the 256 x 256 kernel takes the product, else NN on W^T
        big_qkv, big_ff = ops.use_gemm256(M, 3 * E, E), ops.use_gemm256(M, F, E)
        if not pre:
            ops.split_planes(h, x_p)
        for li, (layer, w) in enumerate(zip(self.transformer, W)):
            att, ffn = layer.self_attn, layer.feed_forward
            ln1, ln2 = layer.layer_norm_1, layer.layer_norm_2
            if pre:                                                   # layers/transformer.py:63-73
                ops.layernorm_fwd(h, ln1.gamma.data, ln1.beta.data, None, rows=M, D=E, eps=ln1.eps, mode=1, out_planes=x_p)
            if first_only and li == self.layers_num - 1:
                return self._last_layer_first_token(ws, layer, w, h, x_p, seg, B, L, E, F)
            engine.linear_fwd(ws, x_p, w["wqkv" if big_qkv else "wqkv_t"], w["bqkv"], None, M, 3 * E, E, out_planes=qkv_p)
            ops.self_attn_fwd(qkv_p, seg, o_p, batch=B, heads=H, L=L, head_dim=hd, scale=scale)
            engine.linear_fwd(ws, o_p, w["wo"], att.final_linear.bias.data, h2, M, E, E, resid=h)
            if pre:
                ops.layernorm_fwd(h2, ln2.gamma.data, ln2.beta.data, None, rows=M, D=E, eps=ln2.eps, mode=1, out_planes=t_p)
                engine.linear_fwd(ws, t_p, w["w1" if big_ff else "w1_t"], ffn.linear_1.bias.data, None, M, F, E, act=1, out_planes=ff_p)
                engine.linear_fwd(ws, ff_p, w["w2"], ffn.linear_2.bias.data, h, M, E, F, resid=h2)
            else:                                                     # layers/transformer.py:54-61
                ops.layernorm_fwd(h2, ln1.gamma.data, ln1.beta.data, h, rows=M, D=E, eps=ln1.eps, mode=1, out_planes=t_p)
                engine.linear_fwd(ws, t_p, w["w1" if big_ff else "w1_t"], ffn.linear_1.bias.data, None, M, F, E, act=1, out_planes=ff_p)
                engine.linear_fwd(ws, ff_p, w["w2"], ffn.linear_2.bias.data, h2, M, E, F, resid=h)
                ops.layernorm_fwd(h2, ln2.gamma.data, ln2.beta.data, h, rows=M, D=E, eps=ln2.eps, mode=1, out_planes=x_p)
        out = torch.empty(B, L, E, device=emb.device)
        if self.final_layernorm:
            ops.layernorm_fwd(h, self.layer_norm.gamma.data, self.layer_norm.beta.data, out.view(M, E), rows=M, D=E,
                              eps=self.layer_norm.eps, mode=1)
        else:
            out.view(M, E).copy_(h)
        return out

    # ---- MX-FP8 inference (BASELINE.json configs[4] "fp8 MFMA"): NOT the parity path, an explicit fast mode ------------------
    def _fp8_weights(self):
        """Per layer: the four projection weights quantised to MX-FP8 once (ops.quant_mxfp8), re-done when a parameter is rewritten."""
        sig = tuple((p.data_ptr(), p._version, ops.param_write_count(p)) for p in self.parameters())
        if getattr(self, "_fp8_sig", None) != sig:
            out = []
            for layer in self.transformer:
                att, ffn = layer.self_attn, layer.feed_forward
                wqkv = ops.quant_mxfp8(torch.cat([l.weight.data for l in att.linear_layers], 0))
                E = wqkv.cols                                          # rows [E, 3E) = [Wk; Wv]: the pruned last layer's product
                wkv = ops.Mx8(wqkv.q[E * E:], wqkv.s[E * (E // 32):], 2 * E, E)
                out.append({"wqkv": wqkv, "wkv": wkv, "bqkv": torch.cat([l.bias.data for l in att.linear_layers], 0),
                            "wo": ops.quant_mxfp8(att.final_linear.weight.data), "w1": ops.quant_mxfp8(ffn.linear_1.weight.data),
                            "w2": ops.quant_mxfp8(ffn.linear_2.weight.data)})
            self._fp8_w, self._fp8_sig = out, sig
        return self._fp8_w

    @torch.no_grad()
    def forward_fp8(self, emb, seg, first_only: bool = False):
        """forward(emb, seg) with the four projections of every layer as MX-FP8 products (csrc/fp8.hip); LayerNorm, attention and the
        residual stream stay fp32 / split-bf16 (head width 64, L <= 288: single-plane bf16 attention, the context straight to MX-FP8;
        L > 288: the 3-pass kernels and a quantise pass, or with infer_attention_long ops.self_attn_fwd_bf16_blocked writing MX-FP8;
        LR2_FP8_ATTN=0 forces the 3-pass kernels at every L).  An element keeps 3 mantissa bits: expect the output a few per cent away from
        forward()'s -- the throughput mode of BASELINE.json configs[4] (FeatureExtractor(precision="mxfp8")), never the parity path.
        first_only: -> hidden[:, 0, :] ([batch, hidden]); the last layer then computes keys / values for every row (MX-FP8) and
        everything behind the scores for row 0 only (forward_first_token's schedule, B rows: split-bf16)."""
        if emb.dtype != torch.float32 or not emb.is_cuda:
            raise TypeError("lr2ppo_amd: emb must be a float32 tensor on the HIP device (no CPU path)")
        B, L, E = emb.shape
        H, hd, M = self.heads_num, E // self.heads_num, B * L
        F = self.transformer[0].feed_forward.linear_1.out_features
        if E % 128 or F % 128:
            raise ValueError("forward_fp8: hidden and feed-forward widths must be multiples of 128")
        if self._ws is None or self._ws.device != emb.device:
            self._ws = engine.Workspace(emb.device)
        ws, dev = self._ws, emb.device
        seg = seg.to(device=dev, dtype=torch.int64).contiguous().view(-1)
        W = self._fp8_weights()
        pre = self.layernorm_positioning == "pre"
        h, h2, xn = ws.mat("h", M, E), ws.mat("h2", M, E), ws.mat("fp8_xn", M, E)
        o32 = ws.mat("fp8_o", M, E)
        qkv_p = ws.planes("qkv_p", M, 3 * E)
        # (longer sequences: the 3-pass kernels, or with infer_attention_long the key-blocked single-plane kernel)
        fast_attn = hd == 64 and (L <= 288 or self.infer_attention_long) and os.environ.get("LR2_FP8_ATTN", "1") != "0"
        attn_b1 = ops.self_attn_fwd_bf16 if L <= 288 else ops.self_attn_fwd_bf16_blocked
        qkv_b = qkv_p.buf[:M * 3 * E]
        if getattr(self, "_fp8_act", None) is None or self._fp8_act[0].rows != M:
            self._fp8_act = (ops.Mx8.empty(M, E, dev), ops.Mx8.empty(M, F, dev))
        x_q, ff_q = self._fp8_act
        h.copy_(emb.contiguous().view(M, E))
        scale = 1.0 / math.sqrt(float(hd))
        for li, (layer, w) in enumerate(zip(self.transformer, W)):
            att, ffn, ln1, ln2 = layer.self_attn, layer.feed_forward, layer.layer_norm_1, layer.layer_norm_2
            if pre:
                ops.layernorm_fwd_mxfp8(h, ln1.gamma.data, ln1.beta.data, x_q, rows=M, D=E, eps=ln1.eps, mode=1)
            else:
                ops.quant_mxfp8(h, x_q)
            if first_only and li == self.layers_num - 1:
                kv_p = ws.planes("kv_p", M, 2 * E)
                ops.gemm_mxfp8(x_q, w["wkv"], None, bias=w["bqkv"][E:], out_planes=kv_p)
                return self._last_layer_first_token(ws, layer, self._weight_planes(dev)[li], h, None, seg, B, L, E, F, kv_p=kv_p)
            if fast_attn:
                # Q | K | V as ONE bf16 plane, single-pass attention, context straight to MX-FP8 (csrc/selfattn_mx.hip)
                ops.gemm_mxfp8(x_q, w["wqkv"], None, bias=w["bqkv"], out_bf16=qkv_b)
                attn_b1(qkv_b, seg, batch=B, heads=H, L=L, head_dim=hd, scale=scale, out_mx=x_q)
            else:
                ops.gemm_mxfp8(x_q, w["wqkv"], None, bias=w["bqkv"], out_planes=qkv_p)     # the 3-pass attention kernels take bf16 hi / lo planes
                ops.self_attn_fwd(qkv_p, seg, o32, batch=B, heads=H, L=L, head_dim=hd, scale=scale)
                ops.quant_mxfp8(o32, x_q)
            ops.gemm_mxfp8(x_q, w["wo"], h2, bias=att.final_linear.bias.data, resid=h)
            if pre:                                                   # layers/transformer.py:63-73
                ops.layernorm_fwd_mxfp8(h2, ln2.gamma.data, ln2.beta.data, x_q, rows=M, D=E, eps=ln2.eps, mode=1)
                ops.gemm_mxfp8(x_q, w["w1"], None, bias=ffn.linear_1.bias.data, act=1, out_mx=ff_q)
                ops.gemm_mxfp8(ff_q, w["w2"], h, bias=ffn.linear_2.bias.data, resid=h2)
            else:                                                     # layers/transformer.py:54-61
                ops.layernorm_fwd_mxfp8(h2, ln1.gamma.data, ln1.beta.data, x_q, xn, rows=M, D=E, eps=ln1.eps, mode=1)
                ops.gemm_mxfp8(x_q, w["w1"], None, bias=ffn.linear_1.bias.data, act=1, out_mx=ff_q)
                ops.gemm_mxfp8(ff_q, w["w2"], h2, bias=ffn.linear_2.bias.data, resid=xn)
                ops.layernorm_fwd(h2, ln2.gamma.data, ln2.beta.data, h, rows=M, D=E, eps=ln2.eps, mode=1)
        out = torch.empty(B, L, E, device=dev)
        if self.final_layernorm:
            ops.layernorm_fwd(h, self.layer_norm.gamma.data, self.layer_norm.beta.data, out.view(M, E), rows=M, D=E,
                              eps=self.layer_norm.eps, mode=1)
        else:
            out.view(M, E).copy_(h)
        return out

    # ---- single-pass bf16 inference (BASELINE.json configs[2] "bf16"): NOT the parity path, the mode between it and MX-FP8 ------
    # replaces, in that mode, the nn.Linear calls of tencentpretrain/layers/multi_headed_attn.py:55-76 and position_ffn.py:12-15 and the
    # scores / softmax / context of multi_headed_attn.py:60-74 -- the same sites as forward_fp8.
    @torch.no_grad()
    def forward_bf16(self, emb, seg, first_only: bool = False):
        """forward(emb, seg) with every GEMM operand ONE bf16 plane and every projection ONE bf16 pass (ops.gemm_bf16,
        csrc/gemm256_b1.hip): the LayerNorm output, Q | K | V as one [M, 3E] plane, the attention context (ops.self_attn_fwd_bf16) and
        GELU(z) are written as a single plane each by the kernel that produces them; the residual stream stays fp32.  The weights are
        the hi planes of _weight_planes (hi == bf16(W)): no copy, no cache of their own.  A third of the parity path's matrix work
        and half its activation traffic; features 4-7e-3 (relative) from forward()'s -- FeatureExtractor(precision="bf16").
        L > 288: the 3-pass attention kernels (the QKV product then writes hi / lo planes, the context goes through split_planes);
        with infer_attention_long the key-blocked single-plane kernel (ops.self_attn_fwd_bf16_blocked) on the same single planes.
        Head width below 64 (a multiple of 4): the same kernels, which are built for head width 64, on heads ZERO-PADDED to 64 columns
        -- one small bf16 product per head and per Q / K / V block writes its columns into a zeroed [M, 3 * heads * 64] planes matrix
        (zero columns add nothing to Q K^T and give zero context columns); a correct route for small test models, not a fast one.
        first_only: -> hidden[:, 0, :] ([batch, hidden]): the last layer computes K | V for every row (a bf16 product) and everything
        behind the scores for row 0 only (forward_first_token's schedule, B rows: split-bf16)."""
        if emb.dtype != torch.float32 or not emb.is_cuda:
            raise TypeError("lr2ppo_amd: emb must be a float32 tensor on the HIP device (no CPU path)")
        B, L, E = emb.shape
        H, hd, M = self.heads_num, E // self.heads_num, B * L
        F = self.transformer[0].feed_forward.linear_1.out_features
        if E % 64 or F % 64:
            raise ValueError("forward_bf16: hidden and feed-forward widths must be multiples of 64")
        if hd != 64 and (hd > 64 or hd % 4):
            raise ValueError("forward_bf16: head width must be 64, or a multiple of 4 below it (zero-padded heads)")
        if first_only and hd != 64:                                   # lr2_first_token_attn is built for head width 64
            return self.forward_bf16(emb, seg)[:, 0, :].contiguous()
        if self._ws is None or self._ws.device != emb.device:
            self._ws = engine.Workspace(emb.device)
        ws, dev = self._ws, emb.device
        seg = seg.to(device=dev, dtype=torch.int64).contiguous().view(-1)
        W = self._weight_planes(dev)
        pre = self.layernorm_positioning == "pre"
        h, h2 = ws.mat("h", M, E), ws.mat("h2", M, E)
        # the planes buffers of _forward_infer, their first half used as the single plane
        x_p, qkv_p, o_p = ws.planes("x_p", M, E), ws.planes("qkv_p", M, 3 * E), ws.planes("o_p", M, E)
        x_b, qkv_b, o_b = x_p.buf[:M * E], qkv_p.buf[:M * 3 * E], o_p.buf[:M * E]
        t_b, ff_b = ws.planes("t_p", M, E).buf[:M * E], ws.planes("ff_p", M, F).buf[:M * F]
        fast_attn = hd == 64 and (L <= 288 or self.infer_attention_long)
        attn_b1 = ops.self_attn_fwd_bf16 if L <= 288 else ops.self_attn_fwd_bf16_blocked
        h.copy_(emb.contiguous().view(M, E))
        scale = 1.0 / math.sqrt(float(hd))
        if not pre:
            ops.split_planes(h, x_p)                                  # hi plane = bf16(h): the first layer's operand
        for li, (layer, w) in enumerate(zip(self.transformer, W)):
            att, ffn, ln1, ln2 = layer.self_attn, layer.feed_forward, layer.layer_norm_1, layer.layer_norm_2
            if pre:
                ops.layernorm_fwd(h, ln1.gamma.data, ln1.beta.data, None, rows=M, D=E, eps=ln1.eps, mode=1, out_plane=x_b)
            if first_only and li == self.layers_num - 1:
                kv_p = ws.planes("kv_p", M, 2 * E)
                ops.gemm_bf16(x_b, w["wqkv"].buf[E * E:3 * E * E], None, M, 2 * E, E, bias=w["bqkv"][E:], out_planes=kv_p)
                return self._last_layer_first_token(ws, layer, w, h, None, seg, B, L, E, F, kv_p=kv_p)
            if fast_attn:
                ops.gemm_bf16(x_b, w["wqkv"], None, M, 3 * E, E, bias=w["bqkv"], out_plane=qkv_b)
                attn_b1(qkv_b, seg, batch=B, heads=H, L=L, head_dim=hd, scale=scale, out_plane=o_b)
            elif hd != 64:
                Ep, o32 = H * 64, ws.mat("bf16_o", M, E)
                pad_p, pad_o = ws.planes("bf16_qkv_pad", M, 3 * Ep), ws.mat("bf16_o_pad", M, Ep)
                if li == 0:
                    pad_p.buf[:2 * M * 3 * Ep].zero_()                 # the padding columns: written by nothing below
                w_hi = w["wqkv"].buf
                for blk in range(3):
                    for hh in range(H):
                        r0 = blk * E + hh * hd                        # rows of [Wq; Wk; Wv] = this head's output columns
                        ops.gemm_bf16(x_b, w_hi[r0 * E:(r0 + hd) * E], None, M, hd, E, bias=w["bqkv"][r0:r0 + hd],
                                      out_planes=pad_p, planes_col=blk * Ep + hh * 64)
                ops.self_attn_fwd(pad_p, seg, pad_o, batch=B, heads=H, L=L, head_dim=64, scale=scale)
                o32.copy_(pad_o.view(M, H, 64)[:, :, :hd].reshape(M, E))
                ops.split_planes(o32, o_p)                            # hi plane = bf16(context)
            else:
                o32 = ws.mat("bf16_o", M, E)
                ops.gemm_bf16(x_b, w["wqkv"], None, M, 3 * E, E, bias=w["bqkv"], out_planes=qkv_p)    # the 3-pass kernels take hi / lo planes
                ops.self_attn_fwd(qkv_p, seg, o32, batch=B, heads=H, L=L, head_dim=hd, scale=scale)
                ops.split_planes(o32, o_p)                            # hi plane = bf16(context)
            ops.gemm_bf16(o_b, w["wo"], h2, M, E, E, bias=att.final_linear.bias.data, resid=h)
            if pre:                                                   # layers/transformer.py:63-73
                ops.layernorm_fwd(h2, ln2.gamma.data, ln2.beta.data, None, rows=M, D=E, eps=ln2.eps, mode=1, out_plane=t_b)
                ops.gemm_bf16(t_b, w["w1"], None, M, F, E, bias=ffn.linear_1.bias.data, act=1, out_plane=ff_b)
                ops.gemm_bf16(ff_b, w["w2"], h, M, E, F, bias=ffn.linear_2.bias.data, resid=h2)
            else:                                                     # layers/transformer.py:54-61
                xn = ws.mat("bf16_xn", M, E)
                ops.layernorm_fwd(h2, ln1.gamma.data, ln1.beta.data, xn, rows=M, D=E, eps=ln1.eps, mode=1, out_plane=t_b)
                ops.gemm_bf16(t_b, w["w1"], None, M, F, E, bias=ffn.linear_1.bias.data, act=1, out_plane=ff_b)
                ops.gemm_bf16(ff_b, w["w2"], h2, M, E, F, bias=ffn.linear_2.bias.data, resid=xn)
                ops.layernorm_fwd(h2, ln2.gamma.data, ln2.beta.data, h, rows=M, D=E, eps=ln2.eps, mode=1, out_plane=x_b)
        out = torch.empty(B, L, E, device=dev)
        if self.final_layernorm:
            ops.layernorm_fwd(h, self.layer_norm.gamma.data, self.layer_norm.beta.data, out.view(M, E), rows=M, D=E,
                              eps=self.layer_norm.eps, mode=1)
        else:
            out.view(M, E).copy_(h)
        return out

    # ---- single-pass f16 inference: forward_bf16's schedule with every single plane in IEEE binary16 (11 significand bits per operand
    # instead of 8: DESIGN 2).  NOT the parity path.  Same sites replaced as forward_bf16.
    def _f16_weights(self):
        """Per layer: the four projection weights as ONE f16 plane each (ops.round_f16 of the fp32 parameters -- not the bf16 hi planes
        of _weight_planes), rounded once and again when a parameter is rewritten (_fp8_weights' signature)."""
        sig = tuple((p.data_ptr(), p._version, ops.param_write_count(p)) for p in self.parameters())
        if getattr(self, "_f16_sig", None) != sig:
            def plane(t):
                return ops.round_f16(t.contiguous(), torch.empty(t.numel(), dtype=torch.float16, device=t.device))
            out = []
            for layer in self.transformer:
                att, ffn = layer.self_attn, layer.feed_forward
                out.append({"wqkv": plane(torch.cat([l.weight.data for l in att.linear_layers], 0)),      # rows Q | K | V
                            "bqkv": torch.cat([l.bias.data for l in att.linear_layers], 0),
                            "wo": plane(att.final_linear.weight.data), "w1": plane(ffn.linear_1.weight.data),
                            "w2": plane(ffn.linear_2.weight.data)})
            self._f16_w, self._f16_sig = out, sig
        return self._f16_w

    @torch.no_grad()
    def forward_f16(self, emb, seg, first_only: bool = False):
        """forward(emb, seg) with every GEMM operand ONE f16 plane and every projection ONE f16 pass (ops.gemm_f16:
        csrc/gemm256_f16.hip or the f16 short tiles of csrc/gemm.hip by ops.f16_block_m, the same bits either way): forward_bf16's schedule -- the LayerNorm output (ops.layernorm_fwd_f16), Q | K | V as one [M, 3E] plane, the
        attention context (ops.self_attn_fwd_f16) and GELU(z) are written as a single f16 plane each by the kernel that produces them; the
        residual stream stays fp32.  The weights are f16 planes of the fp32 parameters (_f16_weights).  The bf16 mode's cost with eight
        times less operand rounding -- FeatureExtractor(precision="f16").
        L > 288: the 3-pass attention kernels (the QKV product then writes bf16 hi / lo planes, the context goes through ops.round_f16),
        or with f16_attention_long the key-blocked single-plane kernel (ops.self_attn_fwd_f16_blocked) on the same single f16 planes: QKV
        as one plane, no rounding pass over the context.  Head width below 64 (a multiple of 4): forward_bf16's zero-padded heads on the same kernels.
        first_only: -> hidden[:, 0, :] ([batch, hidden]): the last layer computes K | V for every row (an f16 product into hi / lo planes)
        and everything behind the scores for row 0 only (forward_first_token's schedule, B rows: split-bf16)."""
        if emb.dtype != torch.float32 or not emb.is_cuda:
            raise TypeError("lr2ppo_amd: emb must be a float32 tensor on the HIP device (no CPU path)")
        B, L, E = emb.shape
        H, hd, M = self.heads_num, E // self.heads_num, B * L
        F = self.transformer[0].feed_forward.linear_1.out_features
        if E % 64 or F % 64:
            raise ValueError("forward_f16: hidden and feed-forward widths must be multiples of 64")
        if hd != 64 and (hd > 64 or hd % 4):
            raise ValueError("forward_f16: head width must be 64, or a multiple of 4 below it (zero-padded heads)")
        if first_only and hd != 64:                                   # lr2_first_token_attn is built for head width 64
            return self.forward_f16(emb, seg)[:, 0, :].contiguous()
        if self._ws is None or self._ws.device != emb.device:
            self._ws = engine.Workspace(emb.device)
        ws, dev = self._ws, emb.device
        seg = seg.to(device=dev, dtype=torch.int64).contiguous().view(-1)
        W = self._f16_weights()
        pre = self.layernorm_positioning == "pre"
        h, h2 = ws.mat("h", M, E), ws.mat("h2", M, E)
        # the planes buffers of _forward_infer, their first half used as the single f16 plane
        qkv_p = ws.planes("qkv_p", M, 3 * E)
        x_b, qkv_b, o_b = ws.planes("x_p", M, E).buf[:M * E], qkv_p.buf[:M * 3 * E], ws.planes("o_p", M, E).buf[:M * E]
        t_b, ff_b = ws.planes("t_p", M, E).buf[:M * E], ws.planes("ff_p", M, F).buf[:M * F]
        fast_attn = hd == 64 and (L <= 288 or self.f16_attention_long)
        attn_f16 = ops.self_attn_fwd_f16 if L <= 288 else ops.self_attn_fwd_f16_blocked
        h.copy_(emb.contiguous().view(M, E))
        scale = 1.0 / math.sqrt(float(hd))
        bm = lambda N, K: ops.f16_schedule_block_m(M, N, K)            # noqa: E731  (tile height by the measured rule; None in f16_force_256)
        if not pre:
            ops.round_f16(h, x_b)                                     # the first layer's operand
        for li, (layer, w) in enumerate(zip(self.transformer, W)):
            att, ffn, ln1, ln2 = layer.self_attn, layer.feed_forward, layer.layer_norm_1, layer.layer_norm_2
            if pre:
                ops.layernorm_fwd_f16(h, ln1.gamma.data, ln1.beta.data, rows=M, D=E, eps=ln1.eps, mode=1, out_plane=x_b)
            if first_only and li == self.layers_num - 1:
                kv_p = ws.planes("kv_p", M, 2 * E)
                ops.gemm_f16(x_b, w["wqkv"][E * E:], None, M, 2 * E, E, bias=w["bqkv"][E:], out_planes=kv_p, block_m=bm(2 * E, E))
                return self._last_layer_first_token(ws, layer, self._weight_planes(dev)[li], h, None, seg, B, L, E, F, kv_p=kv_p)
            if fast_attn:
                ops.gemm_f16(x_b, w["wqkv"], None, M, 3 * E, E, bias=w["bqkv"], out_plane=qkv_b, block_m=bm(3 * E, E))
                attn_f16(qkv_b, seg, batch=B, heads=H, L=L, head_dim=hd, scale=scale, out_plane=o_b)
            elif hd != 64:
                Ep, o32 = H * 64, ws.mat("bf16_o", M, E)
                pad_p, pad_o = ws.planes("bf16_qkv_pad", M, 3 * Ep), ws.mat("bf16_o_pad", M, Ep)
                if li == 0:
                    pad_p.buf[:2 * M * 3 * Ep].zero_()                 # the padding columns: written by nothing below
                for blk in range(3):
                    for hh in range(H):
                        r0 = blk * E + hh * hd                        # rows of [Wq; Wk; Wv] = this head's output columns
                        ops.gemm_f16(x_b, w["wqkv"][r0 * E:(r0 + hd) * E], None, M, hd, E, bias=w["bqkv"][r0:r0 + hd],
                                     out_planes=pad_p, planes_col=blk * Ep + hh * 64, block_m=bm(hd, E))
                ops.self_attn_fwd(pad_p, seg, pad_o, batch=B, heads=H, L=L, head_dim=64, scale=scale)
                o32.copy_(pad_o.view(M, H, 64)[:, :, :hd].reshape(M, E))
                ops.round_f16(o32, o_b)
            else:
                o32 = ws.mat("bf16_o", M, E)
                ops.gemm_f16(x_b, w["wqkv"], None, M, 3 * E, E, bias=w["bqkv"], out_planes=qkv_p,     # the 3-pass kernels take hi / lo planes
                             block_m=bm(3 * E, E))
                ops.self_attn_fwd(qkv_p, seg, o32, batch=B, heads=H, L=L, head_dim=hd, scale=scale)
                ops.round_f16(o32, o_b)
            ops.gemm_f16(o_b, w["wo"], h2, M, E, E, bias=att.final_linear.bias.data, resid=h, block_m=bm(E, E))
            if pre:                                                   # layers/transformer.py:63-73
                ops.layernorm_fwd_f16(h2, ln2.gamma.data, ln2.beta.data, rows=M, D=E, eps=ln2.eps, mode=1, out_plane=t_b)
                ops.gemm_f16(t_b, w["w1"], None, M, F, E, bias=ffn.linear_1.bias.data, act=1, out_plane=ff_b, block_m=bm(F, E))
                ops.gemm_f16(ff_b, w["w2"], h, M, E, F, bias=ffn.linear_2.bias.data, resid=h2, block_m=bm(E, F))
            else:                                                     # layers/transformer.py:54-61
                xn = ws.mat("bf16_xn", M, E)
                ops.layernorm_fwd_f16(h2, ln1.gamma.data, ln1.beta.data, rows=M, D=E, eps=ln1.eps, mode=1, out=xn, out_plane=t_b)
                ops.gemm_f16(t_b, w["w1"], None, M, F, E, bias=ffn.linear_1.bias.data, act=1, out_plane=ff_b, block_m=bm(F, E))
                ops.gemm_f16(ff_b, w["w2"], h2, M, E, F, bias=ffn.linear_2.bias.data, resid=xn, block_m=bm(E, F))
                ops.layernorm_fwd_f16(h2, ln2.gamma.data, ln2.beta.data, rows=M, D=E, eps=ln2.eps, mode=1, out=h, out_plane=x_b)
        out = torch.empty(B, L, E, device=dev)
        if self.final_layernorm:
            ops.layernorm_fwd(h, self.layer_norm.gamma.data, self.layer_norm.beta.data, out.view(M, E), rows=M, D=E,
                              eps=self.layer_norm.eps, mode=1)
        else:
            out.view(M, E).copy_(h)
        return out

    def _last_layer_first_token(self, ws, layer, w, h, x_p, seg, B, L, E, F, kv_p=None):
        """Last layer of the inference schedule for row 0 of every sequence.  h: the layer's input [B*L, E] (fp32); x_p: the
        planes its QKV projection reads (LayerNorm_1(h) for 'pre', h itself for 'post').  K, V: all rows; everything after the
        scores: B rows.  Same kernels and epilogues as the full schedule (the row-0 GEMMs run at M = B).
        kv_p: the [K | V] planes already computed by the caller (forward_fp8); x_p is then unused."""
        att, ffn, ln1, ln2 = layer.self_attn, layer.feed_forward, layer.layer_norm_1, layer.layer_norm_2
        H, hd, M = self.heads_num, E // self.heads_num, B * L
        pre = self.layernorm_positioning == "pre"
        wqkv, dev = w["wqkv"], h.device
        w_q = ops.Planes(wqkv.buf, E, E, lo_off=wqkv.lo_off)                       # rows [0, E) of [Wq; Wk; Wv]
        w_kv = ops.Planes(wqkv.buf[E * E:], 2 * E, E, lo_off=wqkv.lo_off)          # rows [E, 3E)
        if kv_p is None:
            kv_p = ws.planes("kv_p", M, 2 * E)
            engine.linear_fwd(ws, x_p, w_kv, w["bqkv"][E:], None, M, 2 * E, E, out_planes=kv_p)
        h0 = h.view(B, L, E)[:, 0, :].contiguous()                                  # the layer's input at row 0
        x0_p, q0, o0, o0_p = ws.planes("x0_p", B, E), ws.mat("q0", B, E), ws.mat("o0", B, E), ws.planes("o0_p", B, E)
        if pre:
            ops.layernorm_fwd(h0, ln1.gamma.data, ln1.beta.data, None, rows=B, D=E, eps=ln1.eps, mode=1, out_planes=x0_p)
        else:
            ops.split_planes(h0, x0_p)
        engine.linear_fwd(ws, x0_p, w_q, w["bqkv"][:E], q0, B, E, E)
        ops.first_token_attn(q0, kv_p, seg, o0, batch=B, heads=H, L=L, head_dim=hd, scale=1.0 / math.sqrt(float(hd)))
        ops.split_planes(o0, o0_p)
        a0, t0_p, ff0_p, y0 = ws.mat("a0", B, E), ws.planes("t0_p", B, E), ws.planes("ff0_p", B, F), ws.mat("y0", B, E)
        out = torch.empty(B, E, device=dev)
        engine.linear_fwd(ws, o0_p, w["wo"], att.final_linear.bias.data, a0, B, E, E, resid=h0)
        if pre:                                                       # layers/transformer.py:63-73
            ops.layernorm_fwd(a0, ln2.gamma.data, ln2.beta.data, None, rows=B, D=E, eps=ln2.eps, mode=1, out_planes=t0_p)
            engine.linear_fwd(ws, t0_p, w["w1"], ffn.linear_1.bias.data, None, B, F, E, act=1, out_planes=ff0_p)
            engine.linear_fwd(ws, ff0_p, w["w2"], ffn.linear_2.bias.data, y0, B, E, F, resid=a0)
            if self.final_layernorm:
                ops.layernorm_fwd(y0, self.layer_norm.gamma.data, self.layer_norm.beta.data, out, rows=B, D=E,
                                  eps=self.layer_norm.eps, mode=1)
            else:
                out.copy_(y0)
        else:                                                         # layers/transformer.py:54-61
            i0 = ws.mat("i0", B, E)
            ops.layernorm_fwd(a0, ln1.gamma.data, ln1.beta.data, i0, rows=B, D=E, eps=ln1.eps, mode=1, out_planes=t0_p)
            engine.linear_fwd(ws, t0_p, w["w1"], ffn.linear_1.bias.data, None, B, F, E, act=1, out_planes=ff0_p)
            engine.linear_fwd(ws, ff0_p, w["w2"], ffn.linear_2.bias.data, y0, B, E, F, resid=i0)
            ops.layernorm_fwd(y0, ln2.gamma.data, ln2.beta.data, out, rows=B, D=E, eps=ln2.eps, mode=1)
        return out

    # ---- training schedule: same kernels, activations kept for the backward -------------------------------------
    def _dims(self, emb):
        B, L, E = emb.shape
        return B, L, E, self.heads_num, E // self.heads_num, B * L, self.transformer[0].feed_forward.linear_1.out_features

    def _saved_bytes(self, B, L, recompute):
        """(bytes per layer, bytes behind the last layer) a training forward keeps until its backward.  split-bf16: the sizes the
        activation arena is allocated with.  MX-FP8 keeps separate tensors: their sum."""
        E, H, F = self.hidden_size, self.heads_num, self.transformer[0].feed_forward.linear_1.out_features
        M = B * L
        pre = self.layernorm_positioning == "pre"
        if recompute:                                                   # each layer's output = the next one's input (256: alignment)
            return 4 * M * E + 256, (8 * M + 8 * 256 if self.final_layernorm else 0)
        if self.bf16_train:
            # the split-bf16 list below with the LayerNorm outputs (x_p, x2_p / inter_p: 2 x M x E each) and GELU(z) (2 x M x F) kept as
            # ONE bf16 plane instead of hi / lo planes: 4 M E + 2 M F bytes less per layer, either placement
            per_layer = (28 if pre else 36) * M * E + 6 * M * F + 16 * M + 4 * B * H * L + 20 * 256
            if self._b1_attention(E // H, L):
                # Q | K | V (6 M E) and the context (2 M E) as ONE plane each, and no log-sum-exp (the backward recomputes it)
                per_layer -= 8 * M * E + 4 * B * H * L
            return per_layer, 4 * M * E + 8 * M + 8 * 256
        if self.fp8_train:
            Mp = -(-M // 128) * 128                                     # x^T, o^T, x2^T [E, Mp] and GELU(z)^T [F, Mp]: bytes + scale bytes
            return ((24 if pre else 32) * M * E + 4 * M * F + 16 * M + 4 * B * H * L + (3 * E + F) * (Mp + Mp // 32),
                    8 * M if self.final_layernorm else 0)
        # per layer 32 (pre-LN) / 40 (post-LN) x M x E bytes of hidden-width tensors, 8 x M x F of feed-forward ones, 4 row
        # statistics; + the final LayerNorm's statistics
        return (32 if pre else 40) * M * E + 8 * M * F + 16 * M + 4 * B * H * L + 20 * 256, 4 * M * E + 8 * M + 8 * 256

    def saved_activation_bytes(self, batch: int, seq_len: int, recompute=None) -> int:
        """Bytes of activations one training forward over [batch, seq_len] keeps between forward and backward (the arena of
        _forward_train; recompute=None: this encoder's own setting).  Arithmetic only: callable on a CPU module."""
        per_layer, tail = self._saved_bytes(batch, seq_len, self.recompute if recompute is None else bool(recompute))
        return self.layers_num * per_layer + tail

    def _layer_fwd_train(self, i, w, h, h_p, A, seg, dims, drop):
        """Layer i of the split-bf16 training schedule.  h: the layer's input [M, E] (fp32); h_p: its planes (post-LN; None for pre-LN);
        A: the allocator of everything the layer writes (_Kept: the forward's arena; _Reused: workspace buffers).
        -> (S: what the layer's backward reads, the layer's output, its planes (post-LN) or None)."""
        B, L, E, H, hd, M, F = dims
        ws = self._ws                                                   # split-K / reduction scratch only
        layer = self.transformer[i]
        att, ffn = layer.self_attn, layer.feed_forward
        ln1, ln2 = layer.layer_norm_1, layer.layer_norm_2
        pre = self.layernorm_positioning == "pre"
        scale = 1.0 / math.sqrt(float(hd))
        big_qkv, big_ff = ops.use_gemm256(M, 3 * E, E), ops.use_gemm256(M, F, E)
        mat, vec, pl = A.mat, A.vec, A.planes
        s0 = 4 * i
        S = {}
        if pre:
            x_p, S["m1"], S["r1"], S["h_in"] = pl("x_p", M, E), vec("m1", M), vec("r1", M), h
            ops.layernorm_fwd(h, ln1.gamma.data, ln1.beta.data, None, S["m1"], S["r1"], rows=M, D=E, eps=ln1.eps, mode=1,
                              out_planes=x_p)
        else:
            x_p = h_p
        qkv_p, o_p, t1 = pl("qkv_p", M, 3 * E), pl("o_p", M, E), mat("t1", M, E)
        engine.linear_fwd(ws, x_p, w["wqkv" if big_qkv else "wqkv_t"], w["bqkv"], None, M, 3 * E, E, out_planes=qkv_p)
        S["lse"] = vec("lse", B * H * L)                                # the attention's log-sum-exp: an input of its backward
        ops.self_attn_fwd(qkv_p, seg, o_p, batch=B, heads=H, L=L, head_dim=hd, scale=scale, lse=S["lse"], drop=drop(s0))
        engine.linear_fwd(ws, o_p, w["wo"], att.final_linear.bias.data, t1, M, E, E, resid=h, drop=drop(s0 + 1))
        z, ff_p = mat("z", M, F), pl("ff_p", M, F)
        S.update(x_p=x_p, qkv_p=qkv_p, o_p=o_p, t1=t1, z=z, ff_p=ff_p)
        if pre:
            x2_p, S["m2"], S["r2"] = pl("x2_p", M, E), vec("m2", M), vec("r2", M)
            ops.layernorm_fwd(t1, ln2.gamma.data, ln2.beta.data, None, S["m2"], S["r2"], rows=M, D=E, eps=ln2.eps, mode=1,
                              out_planes=x2_p)
            engine.linear_fwd(ws, x2_p, w["w1" if big_ff else "w1_t"], ffn.linear_1.bias.data, None, M, F, E, act=1, out_z=z, out_planes=ff_p)
            hn = mat("hn", M, E)
            engine.linear_fwd(ws, ff_p, w["w2"], ffn.linear_2.bias.data, hn, M, E, F, resid=t1, drop=drop(s0 + 2))
            S["x2_p"] = x2_p
            return S, hn, None
        inter, inter_p, S["m1"], S["r1"] = mat("inter", M, E), pl("inter_p", M, E), vec("m1", M), vec("r1", M)
        ops.layernorm_fwd(t1, ln1.gamma.data, ln1.beta.data, inter, S["m1"], S["r1"], rows=M, D=E, eps=ln1.eps, mode=1,
                          out_planes=inter_p)
        engine.linear_fwd(ws, inter_p, w["w1" if big_ff else "w1_t"], ffn.linear_1.bias.data, None, M, F, E, act=1, out_z=z, out_planes=ff_p)
        t2 = mat("t2", M, E)
        engine.linear_fwd(ws, ff_p, w["w2"], ffn.linear_2.bias.data, t2, M, E, F, resid=inter, drop=drop(s0 + 2))
        # a recomputed layer writes its output planes while its input planes (x_p: its QKV weight gradient reads them afterwards)
        # must stay: two buffers, by layer parity (names matter to _Reused only)
        hn, hn_p, S["m2"], S["r2"] = mat("hn", M, E), pl("h_p%d" % ((i + 1) & 1), M, E), vec("m2", M), vec("r2", M)
        ops.layernorm_fwd(t2, ln2.gamma.data, ln2.beta.data, hn, S["m2"], S["r2"], rows=M, D=E, eps=ln2.eps, mode=1,
                          out_planes=hn_p)
        S.update(inter_p=inter_p, t2=t2)
        return S, hn, hn_p

    @torch.no_grad()
    def _forward_train(self, emb, seg):
        if self.fp8_train:
            return self._forward_train_fp8(emb, seg)
        if self.bf16_train:
            return self._forward_train_bf16(emb, seg)
        dims = B, L, E, H, hd, M, F = self._dims(emb)
        dev = emb.device
        if self._ws is None or self._ws.device != dev:
            self._ws = engine.Workspace(dev)
        seg = seg.to(device=dev, dtype=torch.int64).contiguous().view(-1)
        W = self._weight_planes(dev, cache=False)
        p = float(self.transformer[0].dropout_1.p) if self.training else 0.0
        seed = runtime.next_drop(p, 0).seed if p > 0 else 0
        drop = (lambda site: ops.Drop(p, seed, site)) if p > 0 else (lambda site: None)
        pre = self.layernorm_positioning == "pre"
        rc = bool(self.recompute)
        # everything the backward needs lives in one allocation per forward
        per_layer, tail = self._saved_bytes(B, L, rc)
        kept = _Kept(dev, engine.Arena(dev, self.layers_num * per_layer + tail))
        # recompute: only the layer outputs are kept (each the next layer's input); the rest lands in buffers every layer overwrites
        A = _Reused(self, dev, "rc:", out=kept) if rc else kept
        h = emb.detach().contiguous().view(M, E)
        h_p = None
        if not pre:
            h_p = ops.split_planes(h, A.planes("h_p0", M, E))
        saved = {"layers": [], "seg": seg, "dims": dims, "drop": (p, seed), "W": W, "recompute": rc}
        for i, w in enumerate(W):
            S, hn, hn_p = self._layer_fwd_train(i, w, h, h_p, A, seg, dims, drop)
            saved["layers"].append({"h_in": h} if rc else S)
            h, h_p = hn, hn_p
        if self.final_layernorm:
            out = torch.empty(B, L, E, device=dev)
            saved["h_final"], saved["mf"], saved["rf"] = h, kept.vec("mf", M), kept.vec("rf", M)
            ops.layernorm_fwd(h, self.layer_norm.gamma.data, self.layer_norm.beta.data, out.view(M, E), saved["mf"], saved["rf"],
                              rows=M, D=E, eps=self.layer_norm.eps, mode=1)
        else:
            out = h.view(B, L, E)
        return out, saved

    def _grad_layout(self, flat):
        """Views of `flat` (numel = all parameters) as {parameter: gradient} plus, per layer, the [3E, E] / [3E] blocks that hold the
        Q, K, V weight / bias gradients CONTIGUOUSLY: the fused QKV weight gradient (one TN GEMM + its column sums) is written
        straight into them -- no per-layer copies into three separate tensors."""
        views, qkv, off = {}, [], 0
        for layer in self.transformer:
            lin = layer.self_attn.linear_layers
            E = lin[0].weight.shape[0]
            wblk = flat[off:off + 3 * E * E].view(3 * E, E)
            off += 3 * E * E
            bblk = flat[off:off + 3 * E]
            off += 3 * E
            for j in range(3):
                views[lin[j].weight] = wblk[j * E:(j + 1) * E]
                views[lin[j].bias] = bblk[j * E:(j + 1) * E]
            qkv.append((wblk, bblk))
        for q in self.parameters():
            if q not in views:
                views[q] = flat[off:off + q.numel()].view_as(q)
                off += q.numel()
        return views, qkv

    def grad_buffers(self):
        """{parameter: gradient} views of ONE persistent flat fp32 buffer (the explicit training path of
        lr2ppo_amd.finetune.features: no per-step allocation, fixed addresses for the optimizer's chunk table and one
        contiguous all-reduce under data parallelism)."""
        params = list(self.parameters())
        dev = params[0].device
        if getattr(self, "_gflat", None) is None or self._gflat.device != dev:
            self._gflat = torch.zeros(sum(q.numel() for q in params), device=dev)
            self._gviews, self._gqkv = self._grad_layout(self._gflat)
        return self._gviews

    @torch.no_grad()
    def _backward_train(self, saved, dout, G=None):
        """-> (d emb [B, L, E], {parameter: gradient}) for the forward that produced `saved`.  G: write the parameter gradients
        into these tensors (grad_buffers()) instead of a fresh allocation."""
        if saved.get("fp8"):
            return self._backward_train_fp8(saved, dout, G)
        if saved.get("bf16"):
            return self._backward_train_bf16(saved, dout, G)
        B, L, E, H, hd, M, F = saved["dims"]
        dev, seg, W = dout.device, saved["seg"], saved["W"]
        ws = self._ws
        p, seed = saved["drop"]
        drop = (lambda site: ops.Drop(p, seed, site)) if p > 0 else (lambda site: None)
        # transient gradients: named workspace buffers, reused by every layer and every call (one stream, sequential); the
        # running hidden-state gradient alternates between two of them
        mat = lambda name, r, c: ws.mat("bwd:" + name, r, c)            # noqa: E731
        pl = lambda name, r, c: ws.planes("bwd:" + name, r, c)          # noqa: E731
        if G is None:
            G, qkv_blocks = self._grad_layout(torch.empty(sum(q.numel() for q in self.parameters()), device=dev))
        else:
            if G is not getattr(self, "_gviews", None):
                raise ValueError("_backward_train(G=...): pass grad_buffers()")
            qkv_blocks = self._gqkv
        partials = ws.vec("ln_partials", ops.LN_BWD_BLOCKS * 2 * E)
        dsum_ws = ws.vec("attn_dsum", B * H * L)
        pre = self.layernorm_positioning == "pre"
        scale = 1.0 / math.sqrt(float(hd))
        big_dqkv = ops.use_gemm256(M, E, 3 * E)     # the QKV input gradient goes through a transposed fp32 concatenation only then
        dh = dout.contiguous().view(M, E)
        if self.final_layernorm:
            ln = self.layer_norm
            dnew = mat("dh0", M, E)
            # pre-LN: the top layer's first consumer of this gradient is dropout_2's mask + the planes split (FFN-2's dY): the LayerNorm
            # backward writes them on the way out instead of a separate pass over [M, E]
            top = self.layers_num - 1
            ops.layernorm_bwd(dh, saved["h_final"], ln.gamma.data, saved["mf"], saved["rf"], dnew, partials, G[ln.gamma],
                              G[ln.beta], rows=M, D=E, mode=1, eps=ln.eps, dx_planes=pl("dff_p", M, E) if pre else None,
                              drop=drop(4 * top + 2) if pre else None)
            dh = dnew
        dff_ready = pre and self.final_layernorm
        flip = 1
        rc = _Reused(self, dev, "rc:") if saved.get("recompute") else None
        for i in reversed(range(self.layers_num)):
            layer, w, S = self.transformer[i], W[i], saved["layers"][i]
            if rc is not None:
                # the layer's forward again, from its saved input: the forward's seed (no draw: the counter stays where the plain
                # path leaves it), sites and weight operands -> the same bits; its output is dropped.  Post-LN: the input planes
                # are the split of the input, as the LayerNorm below wrote them (same rounding of the same fp32 values)
                h_in = S["h_in"]
                h_p = None if pre else ops.split_planes(h_in, rc.planes("h_p%d" % (i & 1), M, E))
                S = self._layer_fwd_train(i, w, h_in, h_p, rc, seg, saved["dims"], drop)[0]
            att, ffn = layer.self_attn, layer.feed_forward
            ln1, ln2 = layer.layer_norm_1, layer.layer_norm_2
            s0 = 4 * i
            dff_p, dz_p = pl("dff_p", M, E), pl("dz_p", M, F)
            if pre:
                if not dff_ready:
                    ops.dropout_planes(dh, dff_p, drop(s0 + 2))
                ffn_in_p = S["x2_p"]
            else:
                d_t2 = mat("d_t2", M, E)
                ops.layernorm_bwd(dh, S["t2"], ln2.gamma.data, S["m2"], S["r2"], d_t2, partials, G[ln2.gamma], G[ln2.beta],
                                  rows=M, D=E, dx_planes=dff_p, drop=drop(s0 + 2), mode=1, eps=ln2.eps)
                ffn_in_p = S["inter_p"]
            engine.linear_wgrad(ws, dff_p, S["ff_p"], G[ffn.linear_2.weight], G[ffn.linear_2.bias], M, F, E)
            engine.linear_dgrad(ws, dff_p, w["w2"], None, M, F, E, act=2, aux_z=S["z"], out_planes=dz_p, w_f32=ffn.linear_2.weight.data)
            engine.linear_wgrad(ws, dz_p, ffn_in_p, G[ffn.linear_1.weight], G[ffn.linear_1.bias], M, E, F)
            d_t1, dao_p = mat("d_t1", M, E), pl("dao_p", M, E)
            if pre:
                d_x2 = mat("d_x2", M, E)
                engine.linear_dgrad(ws, dz_p, w["w1"], d_x2, M, E, F, w_f32=ffn.linear_1.weight.data)
                ops.layernorm_bwd(d_x2, S["t1"], ln2.gamma.data, S["m2"], S["r2"], d_t1, partials, G[ln2.gamma], G[ln2.beta],
                                  rows=M, D=E, resid_grad=dh, dx_planes=dao_p, drop=drop(s0 + 1), mode=1, eps=ln2.eps)
            else:
                d_inter = mat("d_x2", M, E)
                engine.linear_dgrad(ws, dz_p, w["w1"], d_inter, M, E, F, resid=d_t2, w_f32=ffn.linear_1.weight.data)
                ops.layernorm_bwd(d_inter, S["t1"], ln1.gamma.data, S["m1"], S["r1"], d_t1, partials, G[ln1.gamma], G[ln1.beta],
                                  rows=M, D=E, dx_planes=dao_p, drop=drop(s0 + 1), mode=1, eps=ln1.eps)
            engine.linear_wgrad(ws, dao_p, S["o_p"], G[att.final_linear.weight], G[att.final_linear.bias], M, E, E)
            do_p, dqkv_p = pl("do_p", M, E), pl("dqkv_p", M, 3 * E)
            engine.linear_dgrad(ws, dao_p, w["wo"], None, M, E, E, out_planes=do_p, w_f32=att.final_linear.weight.data)
            ops.self_attn_bwd(S["qkv_p"], do_p, seg, dqkv_p, S["lse"], dsum_ws, batch=B, heads=H, L=L, head_dim=hd, scale=scale,
                              drop=drop(s0), o=S["o_p"])
            engine.linear_wgrad(ws, dqkv_p, S["x_p"], qkv_blocks[i][0], qkv_blocks[i][1], M, E, 3 * E)     # = the three gradients
            # the gradient handed back to autograd (layer 0) gets its own storage: it outlives this call
            dprev = torch.empty(M, E, device=dev) if i == 0 else mat("dh%d" % flip, M, E)
            flip ^= 1
            if pre:
                d_x1 = mat("d_x1", M, E)
                engine.linear_dgrad(ws, dqkv_p, w["wqkv"], d_x1, M, E, 3 * E, w_f32=w["wqkv_f32"] if big_dqkv else None)
                # ... and the layer below gets its dropout_2-masked planes from this LayerNorm backward (dff_p is free again: its
                # readers of this layer ran earlier on the stream)
                nxt = i > 0
                ops.layernorm_bwd(d_x1, S["h_in"], ln1.gamma.data, S["m1"], S["r1"], dprev, partials, G[ln1.gamma], G[ln1.beta],
                                  rows=M, D=E, resid_grad=d_t1, mode=1, eps=ln1.eps, dx_planes=dff_p if nxt else None,
                                  drop=drop(s0 - 4 + 2) if nxt else None)
                dff_ready = nxt
            else:
                engine.linear_dgrad(ws, dqkv_p, w["wqkv"], dprev, M, E, 3 * E, resid=d_t1, w_f32=w["wqkv_f32"] if big_dqkv else None)
            dh = dprev
            saved["layers"][i] = None                                   # release this layer's activations
        return dh.view(B, L, E), G


    # ---- MX-FP8 training schedule (FeatureExtractor(precision="mxfp8_train")) ------------------------------------------------------
    # _forward_train / _backward_train in the same order, with the same dropout sites, `saved` / G contract and gradient layout, but
    # every projection -- forward, input gradient, weight gradient -- an MX-FP8 product (csrc/fp8.hip, csrc/fp8_train.hip).  The
    # attention (3-pass planes kernels), every LayerNorm, the residual stream and the embeddings stay as they are.
    def _fp8_train_weights(self):
        """Per layer: the four projection weights quantised once per parameter write -- row-blocked (forward: B = W [out, in]) and
        column-blocked (input gradient: B = W^T [in, out], MX blocks along `out`)."""
        sig = tuple((p.data_ptr(), p._version, ops.param_write_count(p)) for p in self.parameters())
        if getattr(self, "_fp8t_sig", None) != sig:
            out = []
            for layer in self.transformer:
                att, ffn = layer.self_attn, layer.feed_forward
                ent = {"bqkv": torch.cat([l.bias.data for l in att.linear_layers], 0)}
                for k, w in (("wqkv", torch.cat([l.weight.data for l in att.linear_layers], 0)), ("wo", att.final_linear.weight.data),
                             ("w1", ffn.linear_1.weight.data), ("w2", ffn.linear_2.weight.data)):
                    ent[k + "_t"], ent[k], _ = ops.quant_mxfp8_t(w.contiguous(), row_blocked=True)
                out.append(ent)
            self._fp8t_w, self._fp8t_sig = out, sig
            self.fp8_weight_quantisations = getattr(self, "fp8_weight_quantisations", 0) + 1
        return self._fp8t_w

    def _mx(self, name, rows, cols, dev):
        """A named reusable Mx8 scratch matrix (operands consumed inside one forward or backward call)."""
        bufs = self.__dict__.setdefault("_mx_bufs", {})
        m = bufs.get(name)
        if m is None or m.rows != rows or m.cols != cols or m.q.device != dev:
            m = bufs[name] = ops.Mx8.empty(rows, cols, dev)
        return m

    def _layer_fwd_train_fp8(self, i, w, h, A, seg, dims, drop, transposed):
        """Layer i of the MX-FP8 training schedule.  h: the layer's input [M, E]; A: the allocator of what the layer writes (_Kept:
        fresh tensors; _Reused: workspace buffers); transposed: also write the column-blocked copies the weight gradients read.
        -> (S: what the layer's backward reads, the layer's output)."""
        B, L, E, H, hd, M, F = dims
        ws, dev = self._ws, h.device
        layer = self.transformer[i]
        att, ffn = layer.self_attn, layer.feed_forward
        ln1, ln2 = layer.layer_norm_1, layer.layer_norm_2
        pre = self.layernorm_positioning == "pre"
        scale = 1.0 / math.sqrt(float(hd))
        Mp = -(-M // 128) * 128
        xs, ys = ws.mat("fp8t_x", M, E), ws.mat("fp8t_y", M, E)        # transient fp32: LayerNorm output, projection before dropout
        x_q, f_q = self._mx("fx", M, E, dev), self._mx("ff", M, F, dev)  # transient row-blocked A operands
        mat, vec, pl = A.mat, A.vec, A.planes

        def quant(name, x, a_q, act=0):
            """row-blocked a_q of x (GELU(x) with act 1), and, when asked, the column-blocked copy of x^T the weight gradient reads"""
            return ops.quant_mxfp8_t(x, rows_out=a_q, act=act, transposed=transposed,
                                     dst=A.mx_t(name, a_q.cols, Mp) if transposed else None)[0]

        def proj_out(a_q, wq, bias, resid, out, site):
            """out = resid + dropout(a . W^T + bias): the split-bf16 epilogue's order"""
            if site is None:
                ops.gemm_mxfp8(a_q, wq, out, bias=bias, resid=resid)
            else:
                ops.gemm_mxfp8(a_q, wq, ys, bias=bias)
                ops.dropout_residual(ys, resid, out, site)

        s0 = 4 * i
        S = {}
        if pre:
            S["m1"], S["r1"], S["h_in"] = vec("m1", M), vec("r1", M), h
            ops.layernorm_fwd(h, ln1.gamma.data, ln1.beta.data, xs, S["m1"], S["r1"], rows=M, D=E, eps=ln1.eps, mode=1)
            S["xT"] = quant("xT", xs, x_q)
        else:
            S["xT"] = quant("xT", h, x_q)
        qkv_p, o_p = pl("qkv", M, 3 * E), pl("o", M, E)
        ops.gemm_mxfp8(x_q, w["wqkv"], None, bias=w["bqkv"], out_planes=qkv_p)
        S["lse"] = vec("lse", B * H * L)
        ops.self_attn_fwd(qkv_p, seg, o_p, batch=B, heads=H, L=L, head_dim=hd, scale=scale, lse=S["lse"], drop=drop(s0))
        S["oT"] = quant("oT", o_p, x_q)
        t1 = mat("t1", M, E)
        proj_out(x_q, w["wo"], att.final_linear.bias.data, h, t1, drop(s0 + 1))
        z = mat("z", M, F)
        S.update(qkv_p=qkv_p, o_p=o_p, t1=t1, z=z)
        hn = mat("hn%d" % (i & 1), M, E)                                # reused buffers: the layer output alternates between two
        if pre:
            S["m2"], S["r2"] = vec("m2", M), vec("r2", M)
            ops.layernorm_fwd(t1, ln2.gamma.data, ln2.beta.data, xs, S["m2"], S["r2"], rows=M, D=E, eps=ln2.eps, mode=1)
            S["x2T"] = quant("x2T", xs, x_q)
            ops.gemm_mxfp8(x_q, w["w1"], z, bias=ffn.linear_1.bias.data)
            S["ffT"] = quant("ffT", z, f_q, act=1)
            proj_out(f_q, w["w2"], ffn.linear_2.bias.data, t1, hn, drop(s0 + 2))
        else:
            inter, S["m1"], S["r1"] = mat("inter", M, E), vec("m1", M), vec("r1", M)
            ops.layernorm_fwd(t1, ln1.gamma.data, ln1.beta.data, inter, S["m1"], S["r1"], rows=M, D=E, eps=ln1.eps, mode=1)
            S["x2T"] = quant("x2T", inter, x_q)
            ops.gemm_mxfp8(x_q, w["w1"], z, bias=ffn.linear_1.bias.data)
            S["ffT"] = quant("ffT", z, f_q, act=1)
            t2 = mat("t2", M, E)
            proj_out(f_q, w["w2"], ffn.linear_2.bias.data, inter, t2, drop(s0 + 2))
            S["m2"], S["r2"] = vec("m2", M), vec("r2", M)
            ops.layernorm_fwd(t2, ln2.gamma.data, ln2.beta.data, hn, S["m2"], S["r2"], rows=M, D=E, eps=ln2.eps, mode=1)
            S["t2"] = t2
        return S, hn

    @torch.no_grad()
    def _forward_train_fp8(self, emb, seg, save: bool = True):
        """save=False (a forward no backward follows: extract(), eval and rollout forwards): the same arithmetic and the same output
        bits, but the activations live in reused workspace buffers and the column-blocked copies are not written.  With `recompute` a
        saving forward runs that way too and keeps only each layer's input (the previous layer's output, a tensor of its own)."""
        dims = B, L, E, H, hd, M, F = self._dims(emb)
        if E % 128 or F % 128:
            raise ValueError("mxfp8_train: hidden and feed-forward widths must be multiples of 128")
        dev = emb.device
        if self._ws is None or self._ws.device != dev:
            self._ws = engine.Workspace(dev)
        seg = seg.to(device=dev, dtype=torch.int64).contiguous().view(-1)
        W = self._fp8_train_weights()
        p = float(self.transformer[0].dropout_1.p) if self.training else 0.0
        seed = runtime.next_drop(p, 0).seed if p > 0 else 0
        drop = (lambda site: ops.Drop(p, seed, site)) if p > 0 else (lambda site: None)
        rc = save and bool(self.recompute)
        # what the backward reads: fresh tensors when saving, else named workspace buffers
        kept = _Kept(dev)
        A = kept if save and not rc else _Reused(self, dev, "fp8e:", out=kept if rc else None)
        h = emb.detach().contiguous().view(M, E)
        saved = {"fp8": True, "layers": [], "seg": seg, "dims": dims, "drop": (p, seed), "W": W, "recompute": rc}
        for i, w in enumerate(W):
            S, hn = self._layer_fwd_train_fp8(i, w, h, A, seg, dims, drop, transposed=save and not rc)
            if save:
                saved["layers"].append({"h_in": h} if rc else S)
            h = hn
        if self.final_layernorm:
            out = torch.empty(B, L, E, device=dev)
            fin = kept if save else A
            mf, rf = fin.vec("mf", M), fin.vec("rf", M)
            ops.layernorm_fwd(h, self.layer_norm.gamma.data, self.layer_norm.beta.data, out.view(M, E), mf, rf,
                              rows=M, D=E, eps=self.layer_norm.eps, mode=1)
            saved["h_final"], saved["mf"], saved["rf"] = h, mf, rf
        else:
            out = h.view(B, L, E) if save else h.clone().view(B, L, E)      # not a view of a reused workspace buffer
        return out, (saved if save else None)

    @torch.no_grad()
    def _backward_train_fp8(self, saved, dout, G=None):
        """_backward_train for a forward of _forward_train_fp8: every product's operands quantised once along the axis it reduces
        over (quant_mxfp8_t: one read of a gradient gives the input-gradient product's A, the weight-gradient product's A^T and the
        bias gradient), weight gradients written straight into G's views by the K-sliced product."""
        B, L, E, H, hd, M, F = saved["dims"]
        dev, seg, W = dout.device, saved["seg"], saved["W"]
        ws = self._ws
        p, seed = saved["drop"]
        drop = (lambda site: ops.Drop(p, seed, site)) if p > 0 else (lambda site: None)
        mat = lambda name, r, c: ws.mat("bwd:" + name, r, c)            # noqa: E731
        pl = lambda name, r, c: ws.planes("bwd:" + name, r, c)          # noqa: E731
        if G is None:
            G, qkv_blocks = self._grad_layout(torch.empty(sum(q.numel() for q in self.parameters()), device=dev))
        else:
            if G is not getattr(self, "_gviews", None):
                raise ValueError("_backward_train(G=...): pass grad_buffers()")
            qkv_blocks = self._gqkv
        partials = ws.vec("ln_partials", ops.LN_BWD_BLOCKS * 2 * E)
        dsum_ws = ws.vec("attn_dsum", B * H * L)
        Mp = -(-M // 128) * 128
        cs_ws = ws.vec("fp8t_colsum", (Mp // 128) * 3 * E if 3 * E > F else (Mp // 128) * F)
        pre = self.layernorm_positioning == "pre"
        scale = 1.0 / math.sqrt(float(hd))
        d_q, dT = self._mx("bd", M, max(3 * E, F), dev), self._mx("bdT", max(3 * E, F), Mp, dev)

        def quant_grad(x, cols, bias_grad, act=0, z=None):
            """row-blocked [M, cols] + column-blocked [cols, Mp] of a gradient, and its column sums into bias_grad"""
            a = ops.Mx8(d_q.q, d_q.s, M, cols)
            at = ops.Mx8(dT.q, dT.s, cols, Mp)
            ops.quant_mxfp8_t(x, rows_out=a, dst=at, colsum=bias_grad, partials=cs_ws, act=act, z=z)
            return a, at

        def wgrad(at, bt, out):
            M_, N_ = at.rows, bt.rows
            sp = ops.mxfp8_wgrad_splits(M_, N_, Mp)
            ops.gemm_mxfp8_wgrad(at, bt, out, splits=sp, workspace=ws.vec("fp8t_wgrad", sp * M_ * N_) if sp > 1 else None)

        dh = dout.contiguous().view(M, E)
        if self.final_layernorm:
            ln = self.layer_norm
            dnew = mat("dh0", M, E)
            top = self.layers_num - 1
            ops.layernorm_bwd(dh, saved["h_final"], ln.gamma.data, saved["mf"], saved["rf"], dnew, partials, G[ln.gamma],
                              G[ln.beta], rows=M, D=E, mode=1, eps=ln.eps, dx_planes=pl("dff_p", M, E) if pre else None,
                              drop=drop(4 * top + 2) if pre else None)
            dh = dnew
        dff_ready = pre and self.final_layernorm
        flip = 1
        rc = _Reused(self, dev, "fp8e:") if saved.get("recompute") else None
        for i in reversed(range(self.layers_num)):
            layer, w, S = self.transformer[i], W[i], saved["layers"][i]
            if rc is not None:          # the saving forward of this layer alone (see _backward_train); W: the forward's quantised weights
                S = self._layer_fwd_train_fp8(i, w, S["h_in"], rc, seg, saved["dims"], drop, transposed=True)[0]
            att, ffn = layer.self_attn, layer.feed_forward
            ln1, ln2 = layer.layer_norm_1, layer.layer_norm_2
            s0 = 4 * i
            dff_p = pl("dff_p", M, E)
            if pre:
                if not dff_ready:
                    ops.dropout_planes(dh, dff_p, drop(s0 + 2))
            else:
                d_t2 = mat("d_t2", M, E)
                ops.layernorm_bwd(dh, S["t2"], ln2.gamma.data, S["m2"], S["r2"], d_t2, partials, G[ln2.gamma], G[ln2.beta],
                                  rows=M, D=E, dx_planes=dff_p, drop=drop(s0 + 2), mode=1, eps=ln2.eps)
            # FFN-2: dW2 = dff^T . GELU(z), dh_ff = dff . W2; FFN-1: dz = dh_ff * GELU'(z), dW1 = dz^T . x2, d x2 = dz . W1
            a, at = quant_grad(dff_p, E, G[ffn.linear_2.bias])
            wgrad(at, S["ffT"], G[ffn.linear_2.weight])
            dff32 = mat("dff32", M, F)
            ops.gemm_mxfp8(a, w["w2_t"], dff32)
            a, at = quant_grad(dff32, F, G[ffn.linear_1.bias], act=2, z=S["z"])
            wgrad(at, S["x2T"], G[ffn.linear_1.weight])
            d_t1, dao_p, d_x2 = mat("d_t1", M, E), pl("dao_p", M, E), mat("d_x2", M, E)
            if pre:
                ops.gemm_mxfp8(a, w["w1_t"], d_x2)
                ops.layernorm_bwd(d_x2, S["t1"], ln2.gamma.data, S["m2"], S["r2"], d_t1, partials, G[ln2.gamma], G[ln2.beta],
                                  rows=M, D=E, resid_grad=dh, dx_planes=dao_p, drop=drop(s0 + 1), mode=1, eps=ln2.eps)
            else:
                ops.gemm_mxfp8(a, w["w1_t"], d_x2, resid=d_t2)
                ops.layernorm_bwd(d_x2, S["t1"], ln1.gamma.data, S["m1"], S["r1"], d_t1, partials, G[ln1.gamma], G[ln1.beta],
                                  rows=M, D=E, dx_planes=dao_p, drop=drop(s0 + 1), mode=1, eps=ln1.eps)
            # output projection, attention, QKV
            a, at = quant_grad(dao_p, E, G[att.final_linear.bias])
            wgrad(at, S["oT"], G[att.final_linear.weight])
            do_p, dqkv_p = pl("do_p", M, E), pl("dqkv_p", M, 3 * E)
            ops.gemm_mxfp8(a, w["wo_t"], None, out_planes=do_p)
            ops.self_attn_bwd(S["qkv_p"], do_p, seg, dqkv_p, S["lse"], dsum_ws, batch=B, heads=H, L=L, head_dim=hd, scale=scale,
                              drop=drop(s0), o=S["o_p"])
            a, at = quant_grad(dqkv_p, 3 * E, qkv_blocks[i][1])
            wgrad(at, S["xT"], qkv_blocks[i][0])
            dprev = torch.empty(M, E, device=dev) if i == 0 else mat("dh%d" % flip, M, E)
            flip ^= 1
            if pre:
                d_x1 = mat("d_x1", M, E)
                ops.gemm_mxfp8(a, w["wqkv_t"], d_x1)
                nxt = i > 0
                ops.layernorm_bwd(d_x1, S["h_in"], ln1.gamma.data, S["m1"], S["r1"], dprev, partials, G[ln1.gamma], G[ln1.beta],
                                  rows=M, D=E, resid_grad=d_t1, mode=1, eps=ln1.eps, dx_planes=dff_p if nxt else None,
                                  drop=drop(s0 - 4 + 2) if nxt else None)
                dff_ready = nxt
            else:
                ops.gemm_mxfp8(a, w["wqkv_t"], dprev, resid=d_t1)
            dh = dprev
            saved["layers"][i] = None
        return dh.view(B, L, E), G

    # ---- single-pass bf16 training schedule (FeatureExtractor(precision="bf16_train")) -----------------------------------
    # _forward_train / _backward_train in the same order, with the same dropout sites, `saved` / G contract and gradient layout, but every
    # projection -- forward, input gradient, weight gradient -- ONE bf16 pass with fp32 accumulation (ops.gemm_bf16_train:
    # csrc/gemm256_b1.hip, csrc/gemm256_tn_b1.hip, the 128- / 64-row family at passes = 1).  The attention (3-pass planes kernels on hi / lo
    # qkv_p, o_p, do_p, dqkv_p; with bf16_attention and head_dim 64, L <= 288 -- any L with bf16_attention_long: the single-plane kernels
    # of csrc/selfattn_b1_train.hip / selfattn_b1_blocked.hip
    # on ONE plane qkv_b, o_b, do_b, dqkv_b each), every LayerNorm, the fp32 residual stream and the fp32 master weights stay as they
    # are.  An activation that only feeds products (LayerNorm outputs, GELU(z)) is kept as ONE plane; a product reads the hi plane
    # (= bf16(x)) of a tensor that exists as hi / lo planes for another reader.
    def _bf16_train_weights(self, dev):
        """Per layer: the hi planes of _weight_planes (forward: B = bf16(W) [out, in]) and of their split_planes_t transposes (input
        gradient: B = bf16(W^T) [in, out]); re-split when a parameter was written."""
        W = self._weight_planes(dev)
        sig = (dev,) + tuple((p.data_ptr(), p._version, ops.param_write_count(p)) for p in self.parameters())
        if getattr(self, "_bf16t_sig", None) != sig:
            out = []
            for layer, w in zip(self.transformer, W):
                att, ffn = layer.self_attn, layer.feed_forward
                E, F = att.final_linear.out_features, ffn.linear_1.out_features
                ent = {"bqkv": w["bqkv"]}
                for k in ("wqkv", "wo", "w1", "w2"):
                    ent[k] = w[k].buf[:w[k].rows * w[k].cols]
                ent["wqkv_t"], ent["w1_t"] = w["wqkv_t"], w["w1_t"]
                ent["wo_t"] = ops.split_planes_t(att.final_linear.weight.data.contiguous(), ops.Planes.empty(E, E, dev))
                ent["w2_t"] = ops.split_planes_t(ffn.linear_2.weight.data.contiguous(), ops.Planes.empty(F, E, dev))
                out.append(ent)
            self._bf16t_w, self._bf16t_sig = out, sig
            self.bf16_weight_splits = getattr(self, "bf16_weight_splits", 0) + 1
        return self._bf16t_w

    def _b1_attention(self, hd, L):
        """Does a bf16_train layer of this shape take the single-plane attention (csrc/selfattn_b1_train.hip; L > 288 with
        bf16_attention_long: csrc/selfattn_b1_blocked.hip)?"""
        return bool(self.bf16_train and self.bf16_attention and hd == 64 and (L <= 288 or self.bf16_attention_long))

    def _layer_fwd_train_bf16(self, i, w, h, h_b, A, seg, dims, drop):
        """Layer i of the bf16 training schedule.  h: the layer's input [M, E] (fp32); h_b: its bf16 plane (post-LN; None for pre-LN);
        A: the allocator of everything the layer writes.  -> (S: what the backward reads, the layer's output, its plane (post-LN) or None)."""
        B, L, E, H, hd, M, F = dims
        layer = self.transformer[i]
        att, ffn = layer.self_attn, layer.feed_forward
        ln1, ln2 = layer.layer_norm_1, layer.layer_norm_2
        pre = self.layernorm_positioning == "pre"
        scale = 1.0 / math.sqrt(float(hd))
        mat, vec, pl, p1 = A.mat, A.vec, A.planes, A.plane
        fwd = engine.linear_fwd_bf16
        s0 = 4 * i
        S = {}
        if pre:
            x_b, S["m1"], S["r1"], S["h_in"] = p1("x_b", M, E), vec("m1", M), vec("r1", M), h
            ops.layernorm_fwd(h, ln1.gamma.data, ln1.beta.data, None, S["m1"], S["r1"], rows=M, D=E, eps=ln1.eps, mode=1, out_plane=x_b)
        else:
            x_b = h_b
        if self._b1_attention(hd, L):
            # ONE plane each for Q | K | V and the context; no log-sum-exp is kept (ops.self_attn_bwd_bf16 recomputes it)
            qkv_b, o_b, t1 = p1("qkv_b", M, 3 * E), p1("o_b", M, E), mat("t1", M, E)
            fwd(x_b, w["wqkv"], w["bqkv"], None, M, 3 * E, E, out_plane=qkv_b)
            ops.self_attn_fwd_bf16_train(qkv_b, seg, o_b, batch=B, heads=H, L=L, head_dim=hd, scale=scale, drop=drop(s0))
            fwd(o_b, w["wo"], att.final_linear.bias.data, t1, M, E, E, resid=h, drop=drop(s0 + 1))
            S.update(qkv_b=qkv_b, o_b=o_b)
        else:
            qkv_p, o_p, t1 = pl("qkv_p", M, 3 * E), pl("o_p", M, E), mat("t1", M, E)
            fwd(x_b, w["wqkv"], w["bqkv"], None, M, 3 * E, E, out_planes=qkv_p)          # hi / lo: the 3-pass attention reads both
            S["lse"] = vec("lse", B * H * L)
            ops.self_attn_fwd(qkv_p, seg, o_p, batch=B, heads=H, L=L, head_dim=hd, scale=scale, lse=S["lse"], drop=drop(s0))
            fwd(o_p, w["wo"], att.final_linear.bias.data, t1, M, E, E, resid=h, drop=drop(s0 + 1))
            S.update(qkv_p=qkv_p, o_p=o_p)
        z, ff_b = mat("z", M, F), p1("ff_b", M, F)
        S.update(x_b=x_b, t1=t1, z=z, ff_b=ff_b)
        if pre:
            x2_b, S["m2"], S["r2"] = p1("x2_b", M, E), vec("m2", M), vec("r2", M)
            ops.layernorm_fwd(t1, ln2.gamma.data, ln2.beta.data, None, S["m2"], S["r2"], rows=M, D=E, eps=ln2.eps, mode=1, out_plane=x2_b)
            fwd(x2_b, w["w1"], ffn.linear_1.bias.data, None, M, F, E, act=1, out_z=z, out_plane=ff_b)
            hn = mat("hn%d" % (i & 1), M, E)                            # reused buffers: the layer output alternates between two
            fwd(ff_b, w["w2"], ffn.linear_2.bias.data, hn, M, E, F, resid=t1, drop=drop(s0 + 2))
            S["x2_b"] = x2_b
            return S, hn, None
        inter, inter_b, S["m1"], S["r1"] = mat("inter", M, E), p1("inter_b", M, E), vec("m1", M), vec("r1", M)
        ops.layernorm_fwd(t1, ln1.gamma.data, ln1.beta.data, inter, S["m1"], S["r1"], rows=M, D=E, eps=ln1.eps, mode=1, out_plane=inter_b)
        fwd(inter_b, w["w1"], ffn.linear_1.bias.data, None, M, F, E, act=1, out_z=z, out_plane=ff_b)
        t2 = mat("t2", M, E)
        fwd(ff_b, w["w2"], ffn.linear_2.bias.data, t2, M, E, F, resid=inter, drop=drop(s0 + 2))
        # (two output-plane buffers by layer parity: see _layer_fwd_train)
        hn, hn_b, S["m2"], S["r2"] = mat("hn%d" % (i & 1), M, E), p1("h_b%d" % ((i + 1) & 1), M, E), vec("m2", M), vec("r2", M)
        ops.layernorm_fwd(t2, ln2.gamma.data, ln2.beta.data, hn, S["m2"], S["r2"], rows=M, D=E, eps=ln2.eps, mode=1, out_plane=hn_b)
        S.update(inter_b=inter_b, t2=t2)
        return S, hn, hn_b

    def _input_plane(self, h, A, name, M, E):
        """bf16(h) as ONE plane: the hi plane of a planes split (post-LN: the first layer's, or a recomputed layer's, operand)."""
        return ops.split_planes(h, A.planes(name, M, E)).buf[:M * E]

    @torch.no_grad()
    def _forward_train_bf16(self, emb, seg, save: bool = True):
        """save=False (a forward no backward follows: extract(), eval and rollout forwards): the same arithmetic and the same output
        bits, with the activations in reused workspace buffers."""
        dims = B, L, E, H, hd, M, F = self._dims(emb)
        if E % 64 or F % 64:
            raise ValueError("bf16_train: hidden and feed-forward widths must be multiples of 64")
        dev = emb.device
        if self._ws is None or self._ws.device != dev:
            self._ws = engine.Workspace(dev)
        seg = seg.to(device=dev, dtype=torch.int64).contiguous().view(-1)
        W = self._bf16_train_weights(dev)
        p = float(self.transformer[0].dropout_1.p) if self.training else 0.0
        seed = runtime.next_drop(p, 0).seed if p > 0 else 0
        drop = (lambda site: ops.Drop(p, seed, site)) if p > 0 else (lambda site: None)
        pre = self.layernorm_positioning == "pre"
        rc = save and bool(self.recompute)
        per_layer, tail = self._saved_bytes(B, L, rc)
        kept = _Kept(dev, engine.Arena(dev, self.layers_num * per_layer + tail)) if save else None
        A = kept if save and not rc else _Reused(self, dev, "b16:", out=kept if rc else None)
        h = emb.detach().contiguous().view(M, E)
        h_b = None if pre else self._input_plane(h, A, "h_p0", M, E)
        saved = {"bf16": True, "layers": [], "seg": seg, "dims": dims, "drop": (p, seed), "W": W, "recompute": rc}
        for i, w in enumerate(W):
            S, hn, hn_b = self._layer_fwd_train_bf16(i, w, h, h_b, A, seg, dims, drop)
            if save:
                saved["layers"].append({"h_in": h} if rc else S)
            h, h_b = hn, hn_b
        if self.final_layernorm:
            out = torch.empty(B, L, E, device=dev)
            fin = kept if save else A
            mf, rf = fin.vec("mf", M), fin.vec("rf", M)
            ops.layernorm_fwd(h, self.layer_norm.gamma.data, self.layer_norm.beta.data, out.view(M, E), mf, rf,
                              rows=M, D=E, eps=self.layer_norm.eps, mode=1)
            saved["h_final"], saved["mf"], saved["rf"] = h, mf, rf
        else:
            out = h.view(B, L, E) if save else h.clone().view(B, L, E)      # not a view of a reused workspace buffer
        return out, (saved if save else None)

    @torch.no_grad()
    def _backward_train_bf16(self, saved, dout, G=None):
        """_backward_train for a forward of _forward_train_bf16.  A gradient that a LayerNorm backward or the attention backward wrote
        as hi / lo planes enters its two products (input gradient: A; weight gradient: A^T, with the bias gradient) as its hi plane."""
        B, L, E, H, hd, M, F = saved["dims"]
        dev, seg, W = dout.device, saved["seg"], saved["W"]
        ws = self._ws
        p, seed = saved["drop"]
        drop = (lambda site: ops.Drop(p, seed, site)) if p > 0 else (lambda site: None)
        mat = lambda name, r, c: ws.mat("bwd:" + name, r, c)            # noqa: E731
        pl = lambda name, r, c: ws.planes("bwd:" + name, r, c)          # noqa: E731
        dgrad, wgrad = engine.linear_dgrad_bf16, engine.linear_wgrad_bf16
        if G is None:
            G, qkv_blocks = self._grad_layout(torch.empty(sum(q.numel() for q in self.parameters()), device=dev))
        else:
            if G is not getattr(self, "_gviews", None):
                raise ValueError("_backward_train(G=...): pass grad_buffers()")
            qkv_blocks = self._gqkv
        partials = ws.vec("ln_partials", ops.LN_BWD_BLOCKS * 2 * E)
        dsum_ws = ws.vec("attn_dsum", B * H * L)
        pre = self.layernorm_positioning == "pre"
        scale = 1.0 / math.sqrt(float(hd))
        dh = dout.contiguous().view(M, E)
        if self.final_layernorm:
            ln = self.layer_norm
            dnew = mat("dh0", M, E)
            top = self.layers_num - 1
            ops.layernorm_bwd(dh, saved["h_final"], ln.gamma.data, saved["mf"], saved["rf"], dnew, partials, G[ln.gamma],
                              G[ln.beta], rows=M, D=E, mode=1, eps=ln.eps, dx_planes=pl("dff_p", M, E) if pre else None,
                              drop=drop(4 * top + 2) if pre else None)
            dh = dnew
        dff_ready = pre and self.final_layernorm
        flip = 1
        rc = _Reused(self, dev, "b16:") if saved.get("recompute") else None
        for i in reversed(range(self.layers_num)):
            layer, w, S = self.transformer[i], W[i], saved["layers"][i]
            if rc is not None:          # the saving forward of this layer alone (see _backward_train): same seed, sites, operands
                h_in = S["h_in"]
                h_b = None if pre else self._input_plane(h_in, rc, "h_p%d" % (i & 1), M, E)
                S = self._layer_fwd_train_bf16(i, w, h_in, h_b, rc, seg, saved["dims"], drop)[0]
            att, ffn = layer.self_attn, layer.feed_forward
            ln1, ln2 = layer.layer_norm_1, layer.layer_norm_2
            s0 = 4 * i
            dff_p, dz_b = pl("dff_p", M, E), ws.plane("bwd:dz_b", M, F)
            if pre:
                if not dff_ready:
                    ops.dropout_planes(dh, dff_p, drop(s0 + 2))
                ffn_in_b = S["x2_b"]
            else:
                d_t2 = mat("d_t2", M, E)
                ops.layernorm_bwd(dh, S["t2"], ln2.gamma.data, S["m2"], S["r2"], d_t2, partials, G[ln2.gamma], G[ln2.beta],
                                  rows=M, D=E, dx_planes=dff_p, drop=drop(s0 + 2), mode=1, eps=ln2.eps)
                ffn_in_b = S["inter_b"]
            wgrad(ws, dff_p, S["ff_b"], G[ffn.linear_2.weight], G[ffn.linear_2.bias], M, F, E)
            dgrad(dff_p, w["w2_t"], None, M, F, E, act=2, aux_z=S["z"], out_plane=dz_b)
            wgrad(ws, dz_b, ffn_in_b, G[ffn.linear_1.weight], G[ffn.linear_1.bias], M, E, F)
            d_t1, dao_p = mat("d_t1", M, E), pl("dao_p", M, E)
            if pre:
                d_x2 = mat("d_x2", M, E)
                dgrad(dz_b, w["w1_t"], d_x2, M, E, F)
                ops.layernorm_bwd(d_x2, S["t1"], ln2.gamma.data, S["m2"], S["r2"], d_t1, partials, G[ln2.gamma], G[ln2.beta],
                                  rows=M, D=E, resid_grad=dh, dx_planes=dao_p, drop=drop(s0 + 1), mode=1, eps=ln2.eps)
            else:
                d_inter = mat("d_x2", M, E)
                dgrad(dz_b, w["w1_t"], d_inter, M, E, F, resid=d_t2)
                ops.layernorm_bwd(d_inter, S["t1"], ln1.gamma.data, S["m1"], S["r1"], d_t1, partials, G[ln1.gamma], G[ln1.beta],
                                  rows=M, D=E, dx_planes=dao_p, drop=drop(s0 + 1), mode=1, eps=ln1.eps)
            if "qkv_b" in S:                # the single-plane attention (bf16_attention): do and dQ | dK | dV as ONE plane each
                wgrad(ws, dao_p, S["o_b"], G[att.final_linear.weight], G[att.final_linear.bias], M, E, E)
                do_b, dqkv_p = ws.plane("bwd:do_b", M, E), ws.plane("bwd:dqkv_b", M, 3 * E)
                dgrad(dao_p, w["wo_t"], None, M, E, E, out_plane=do_b)
                ops.self_attn_bwd_bf16(S["qkv_b"], do_b, seg, dqkv_p, ws.vec("attn_lse", B * H * L), dsum_ws, batch=B, heads=H, L=L,
                                       head_dim=hd, scale=scale, drop=drop(s0))
            else:
                wgrad(ws, dao_p, S["o_p"], G[att.final_linear.weight], G[att.final_linear.bias], M, E, E)
                do_p, dqkv_p = pl("do_p", M, E), pl("dqkv_p", M, 3 * E)
                dgrad(dao_p, w["wo_t"], None, M, E, E, out_planes=do_p)
                ops.self_attn_bwd(S["qkv_p"], do_p, seg, dqkv_p, S["lse"], dsum_ws, batch=B, heads=H, L=L, head_dim=hd, scale=scale,
                                  drop=drop(s0), o=S["o_p"])
            wgrad(ws, dqkv_p, S["x_b"], qkv_blocks[i][0], qkv_blocks[i][1], M, E, 3 * E)     # = the three gradients
            dprev = torch.empty(M, E, device=dev) if i == 0 else mat("dh%d" % flip, M, E)
            flip ^= 1
            if pre:
                d_x1 = mat("d_x1", M, E)
                dgrad(dqkv_p, w["wqkv_t"], d_x1, M, E, 3 * E)
                nxt = i > 0
                ops.layernorm_bwd(d_x1, S["h_in"], ln1.gamma.data, S["m1"], S["r1"], dprev, partials, G[ln1.gamma], G[ln1.beta],
                                  rows=M, D=E, resid_grad=d_t1, mode=1, eps=ln1.eps, dx_planes=dff_p if nxt else None,
                                  drop=drop(s0 - 4 + 2) if nxt else None)
                dff_ready = nxt
            else:
                dgrad(dqkv_p, w["wqkv_t"], dprev, M, E, 3 * E, resid=d_t1)
            dh = dprev
            saved["layers"][i] = None
        return dh.view(B, L, E), G


class _EncoderFn(torch.autograd.Function):
    """Coarse autograd node: the whole encoder stack forward / backward on the HIP kernels."""

    @staticmethod
    def forward(ctx, enc, emb, seg, *params):
        out, saved = enc._forward_train(emb, seg)
        ctx.enc, ctx.saved = enc, saved
        return out

    @staticmethod
    def backward(ctx, dout):
        demb, G = ctx.enc._backward_train(ctx.saved, dout.contiguous())
        ctx.saved = None
        return (None, demb, None) + tuple(G[q] if q.requires_grad else None for q in ctx.enc.parameters())


class _OneLayerStack(TransformerEncoder):
    """A TransformerLayer run on its own (`TransformerLayer.forward(hidden, mask)`, layers/transformer.py:50-73 upstream):
    the one-layer case of the encoder schedule, without the stack's final LayerNorm.  Shares the layer's parameters."""

    def __init__(self, layer):
        nn.Module.__init__(self)
        att = layer.self_attn
        self.mask, self.layers_num = "fully_visible", 1
        self.layernorm_positioning = layer.layernorm_positioning
        self.heads_num, self.hidden_size = att.heads_num, att.final_linear.out_features
        self.transformer = nn.ModuleList([layer])
        self.final_layernorm = False
        self._ws = None
        self._wplanes = None


def seg_from_additive_mask(mask):
    """[B, 1, L, L] additive mask of the 'fully_visible' form (0 where the KEY is visible, -10000 where it is padding, the
    same for every query row: encoders/transformer_encoder.py:62-68 upstream) -> seg [B, L] (1 visible / 0 padded).
    Other mask shapes (causal, per-query) are not on the HIP path."""
    if mask.dim() != 4 or mask.shape[1] != 1 or mask.shape[2] != mask.shape[3]:
        raise ValueError("mask must be [batch, 1, seq, seq]")
    row0 = mask[:, 0, 0, :]
    if not bool((mask[:, 0] == row0.unsqueeze(1)).all()):
        raise NotImplementedError("HIP attention takes key-padding masks only (mask='fully_visible'); use the reference "
                                  "for causal / per-query masks")
    if not bool(((row0 == 0) | (row0 == -10000.0)).all()):
        raise NotImplementedError("HIP attention supports additive masks with values 0 / -10000 only")
    return (row0 == 0).to(torch.int64)
