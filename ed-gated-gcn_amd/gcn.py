"""``GraphConvolution`` -- drop-in for ``models/gcn.py:9-45`` running on MI355X.

Same constructor ``(in_features, out_features, opt, bias=True)`` (``gcn.py:14``; ``opt``
is accepted and, as in the reference, not needed), same parameters ``weight [in,out]``
and ``bias [out]`` (``gcn.py:18,21``; left uninitialised like the reference --
``train.py:75-84`` initialises them), same ``forward(text, adj) -> [B,T,out]``
(``gcn.py:30-45``).  Underneath: dense adjacency -> batched CSR -> MFMA linear ->
one-wavefront-per-node gated aggregation, all in libggcn_hip.so.

Extras that the classifier block uses (``models/bert_amir5.py:621-640``):
``forward_gated`` fuses the per-sentence gate and the max-pool over tokens into the
aggregation pass, taking the gate as ``[B,H]`` instead of a materialised ``[B,T,H]``.
"""
import collections
import os

import torch
import torch.nn as nn

from . import _capi, dispatch, hostops, range_guard
from .csr import BatchedCSR, cached_from_dense
from .hostops import _opted_in, f32_rows
from .dispatch import BF16_PRECISIONS  # noqa: F401  (its home is dispatch.py; imported from here too)


def _require_gpu_f32(name, t, allow_half=False, allow_bf16=False):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise RuntimeError("%s is on %s: this layer only runs on the GPU (libggcn_hip.so); "
                           "there is no CPU fallback" % (name, t.device))
    if t.dtype != torch.float32 and not (allow_half and t.dtype == torch.float16) and not (allow_bf16 and t.dtype == torch.bfloat16):
        raise RuntimeError("%s must be float32%s%s, got %s" % (name, " or float16" if allow_half else "",
                                                               " or bfloat16" if allow_bf16 else "", t.dtype))


def _rows2d(text):
    """[B,T,K] features as [B*T,K] rows with unit column stride (a view where the layout allows it)."""
    B, T, K = text.shape
    x2d = text.reshape(B * T, K)
    return x2d if x2d.stride(1) == 1 else x2d.contiguous()


def _require_gate(name, g, B, F, wording):
    """A gate is a contiguous float32 [B,F] GPU tensor; else RuntimeError in the caller's ``wording`` (name, B, F, shape)."""
    if not (isinstance(g, torch.Tensor) and g.is_cuda and g.dtype == torch.float32 and tuple(g.shape) == (B, F) and g.is_contiguous()):
        raise RuntimeError(wording % {"name": name, "B": B, "F": F, "shape": tuple(getattr(g, "shape", ()))})


def _drop_args(dropout):
    """``(p, seed, stream_store, stream_a, stream_b)`` as the entries take them; no dropout: p = 0, every stream 0."""
    return (0.0, 0, 0, 0, 0) if dropout is None else (float(dropout[0]), int(dropout[1])) + tuple(dropout[2])


def _admit(launch, dropout, overlap):
    """Gate dropout and the overlap operands exist in the one-launch layers only: decided from the name of the launch the call takes."""
    if dropout is not None and launch not in dispatch.DROPOUT_LAUNCHES:
        raise RuntimeError("dropout= needs the one-launch layer (takes_dropout_path: takes_fused_path and B*T*F < 2^32)")
    if overlap and launch not in dispatch.OVERLAP_LAUNCHES:
        raise RuntimeError("overlap_partial / overlap_reduce need the one-launch layer (takes_fused_path)")


# One one-launch layer of _forward_gated.  Every entry takes ``X, ldx, weight image, <graph operands>, bias, [zero mid row], B, T, K, F,
# gates, outputs, [overlap x 3], [precision], [p, seed, keep streams], stream``.  image(layer, x2d, csr): the precision of the weight
# image (None: the layer's own); graph(csr, precision): the per-graph operands; mid: the zero row follows the bias; overlap: True the
# three overlap operands, False three NULLs, None no such arguments; precision / drop: the precision code / dropout arguments follow.
_LayerLaunch = collections.namedtuple("_LayerLaunch", "entry image graph mid overlap precision drop", defaults=(False, None, False, False))


def _weighted_image(layer, x2d, csr):
    return "bf16x3" if layer.precision == "bf16x3" else "f16mx8"


_LAYER_LAUNCHES = {   # dispatch.layer_launch's names but "two_launch" (linear + aggregate)
    "fused": _LayerLaunch("ggcn_layer_fused", lambda m, x2d, c: m.kernel_precision(x2d, c),
                          lambda c, prec: (c.rowmask, c.graph_ops if c.T <= 32 else dispatch.edge_lists(c)), overlap=True, precision=True),
    "fused_drop": _LayerLaunch("ggcn_layer_fused_drop", lambda m, x2d, c: "f16mx8" if m.precision == "f16mx6" else m.precision,
                               lambda c, prec: (c.rowmask, c.graph_ops), precision=True, drop=True),   # (the fp6 kernel has no dropout epilogue)
    # bfloat16 features, the bf16x3 image: <= 32 nodes on the operand blocks; 33..256 on the row masks, one entry (p = 0 draws nothing)
    "bf16": _LayerLaunch("ggcn_layer_fused_bf16", lambda m, x2d, c: "bf16x3", lambda c, prec: (c.graph_ops,), overlap=True),
    "bf16_drop": _LayerLaunch("ggcn_layer_fused_bf16_drop", lambda m, x2d, c: "bf16x3", lambda c, prec: (c.graph_ops,), overlap=True, drop=True),
    "bf16_wide": _LayerLaunch("ggcn_layer_fused_bf16_wide", lambda m, x2d, c: "bf16x3",
                              lambda c, prec: (c.rowmask, dispatch.edge_lists(c) if c.T > 128 else None), overlap=True, drop=True),
    # real-valued adjacency: D.A_w as one operand per graph of <= 32 nodes and plane type, or ceil(T/32)^2 blocks of 33..128 (weighted_max_t)
    "weighted": _LayerLaunch("ggcn_layer_fused_weighted", _weighted_image, lambda c, prec: (c.graph_ops_weighted(0 if prec == "bf16x3" else 1),),
                             mid=True, overlap=False, precision=True),
    "weighted_drop": _LayerLaunch("ggcn_layer_fused_weighted_drop", _weighted_image,
                                  lambda c, prec: (c.graph_ops_weighted(0 if prec == "bf16x3" else 1),), mid=True, precision=True, drop=True),
    "weighted_wide": _LayerLaunch("ggcn_layer_fused_weighted_wide", _weighted_image, lambda c, prec: (c.graph_ops_weighted_wide(),), precision=True),
    "weighted_wide_drop": _LayerLaunch("ggcn_layer_fused_weighted_wide_drop", _weighted_image, lambda c, prec: (c.graph_ops_weighted_wide(),),
                                       precision=True, drop=True),
    # long fp16 graphs (BASELINE configs[3]): linear + aggregation in one launch, hidden stays in LDS
    "long": _LayerLaunch("ggcn_layer_fused_h", lambda m, x2d, c: None, lambda c, prec: (c.rowptr, c.colidx, c.vals)),
}
_LAYER_LAUNCHES["bf16_wide_drop"] = _LAYER_LAUNCHES["bf16_wide"]

# One gate / pool backward launch of _GatedLayerFunction.backward, by dispatch.backward_launch's names.  graph(csr): the graph operands
# after d_pb; writes: "dH", "dY" (to memory, for ggcn_aggregate_t) or "both" (dH, and dY where an adjacency gradient wants it); tail: what
# follows d_bsum
_BackwardLaunch = collections.namedtuple("_BackwardLaunch", "entry graph writes tail")
_weighted_t = lambda c: (c.graph_ops_weighted_t(), c.inv_denominators())   # noqa: E731
_BACKWARD_LAUNCHES = {
    "mma": _BackwardLaunch("ggcn_gate_pool_backward_mma", lambda c: (c.graph_ops, c.graph_ops_t), "dH", ("amax",)),
    "one_pass": _BackwardLaunch("ggcn_gate_pool_backward_agg", lambda c: (c.rowmask,), "dH", ("drop", "amax")),
    "two_pass": _BackwardLaunch("ggcn_gate_pool_backward", lambda c: (), "dY", ()),
    "two_pass_drop": _BackwardLaunch("ggcn_gate_pool_backward_drop", lambda c: (), "dY", ("drop",)),
    "weighted": _BackwardLaunch("ggcn_gate_pool_backward_weighted", _weighted_t, "both", ()),
    "weighted_drop": _BackwardLaunch("ggcn_gate_pool_backward_weighted_drop", _weighted_t, "both", ("drop",)),
    "wide": _BackwardLaunch("ggcn_gate_pool_backward_wide", lambda c: (c.rowmask_t_wide, c.inv_denominators()), "dH", ()),
    "weighted_wide": _BackwardLaunch("ggcn_gate_pool_backward_weighted_wide",
                                     lambda c: (c.graph_ops_weighted_wide_t(), c.inv_denominators()), "both", ()),
}


class _GatedLayerFunction(torch.autograd.Function):
    """One gated layer under autograd (``train.py:115-121`` trains through gc1/gc2 and the gates).

    Forward = the inference kernels (fused layer or linear + aggregate, gate and max-pool in the
    epilogue).  Backward, for y = D.A.(X.W) + b, out = y*sg, pa = max_t y*ga, pb = max_t y*gb:

        dY, d_sg, d_ga, d_gb   HIP, one pass over the stored output (gate_pool_backward.hip)
        dH = A^T.(D.dY)        HIP, one wavefront per SOURCE node on the transposed CSR (0/1 graphs of <= 32 nodes: one launch with
                               the line above; real-valued ones with ``weighted_backward``:
                               ggcn_gate_pool_backward_weighted[_drop]; 0/1 graphs of 33..128 nodes with ``wide_backward``,
                               without gate dropout: ggcn_gate_pool_backward_wide; real-valued ones of 33..128 nodes with
                               ``weighted_wide_backward``: ggcn_gate_pool_backward_weighted_wide; dispatch.backward_launch names
                               the launch)
        dX = dH.W^T            HIP bf16x3 MFMA linear on the packed W^T (bfloat16 features: stored as bf16, RNE)
        dW = X^T.dH            HIP split-K: bf16x3 main loop on X^T and packed dH (dweight_bx3.hip; bfloat16 features:
                               X^T in bf16, ggcn_dweight_bf16), or the exact-fp32 MFMA form for precision 'fp32' (dweight_fp32.hip)
        db = sum_rows dY       HIP: per-graph sums from the gate/pool pass + ggcn_colsum
        dA = D.dY.H^T - c      HIP, only for a differentiable dense `adj` (``adj_t``; gcn.py:33-45 is differentiable in it): the
                               two-call form so that dY exists in memory, `hidden` H recomputed by the layer's linear, then
                               ggcn_adjacency_grad (bf16x3 MFMA; dense [B,T,T], zero entries and padding rows included)
    """

    @staticmethod
    def forward(ctx, text, weight, bias, store_gate, gate_a, gate_b, layer, csr, want_pa, want_pb, dropout=None, adj_t=None):
        with torch.no_grad():
            out, pa, pb = layer.forward_gated(text, csr, store_gate=store_gate, pool_gate_a=gate_a,
                                              pool_gate_b=gate_b, want_out=True, want_pool_a=want_pa,
                                              want_pool_b=want_pb, _internal=True, dropout=dropout)
        ctx.layer, ctx.csr, ctx.dropout = layer, csr, dropout
        ctx.save_for_backward(text, weight, out, store_gate, gate_a, gate_b)
        ctx.has_bias = bias is not None
        ctx.adj_dtype = None if adj_t is None else adj_t.dtype
        # an output the loss does not use arrives as None, not as a tensor of zeros: the [B,T,F] `out` of a layer whose pools alone
        # are used would otherwise cost a 400 MB fill AND a 400 MB read per step (every backward kernel takes d_out = NULL)
        ctx.set_materialize_grads(False)
        return out, pa, pb

    @staticmethod
    def backward(ctx, d_out, d_pa, d_pb):
        text, weight, out, store_gate, gate_a, gate_b = ctx.saved_tensors
        layer, csr = ctx.layer, ctx.csr
        if d_out is None and d_pa is None and d_pb is None:
            return (None,) * 12
        lib = _capi.load_library()
        (B, T, K), F, dev = text.shape, layer.out_features, text.device
        d_out2, d_pa, d_pb = f32_rows(d_out, (B * T, F)), f32_rows(d_pa, (B, F)), f32_rows(d_pb, (B, F))
        out2 = out.reshape(-1, F)
        ptr = _capi.ptr
        with torch.cuda.device(dev):
            st = _capi.stream_of(dev)
            need = ctx.needs_input_grad
            f32 = dict(dtype=torch.float32, device=dev)
            d_sg = torch.empty(B, F, **f32) if (store_gate is not None and need[3]) else None
            d_ga = torch.empty(B, F, **f32) if (gate_a is not None and need[4] and d_pa is not None) else None
            d_gb = torch.empty(B, F, **f32) if (gate_b is not None and need[5] and d_pb is not None) else None
            d_bsum = torch.empty(B, F, **f32) if (ctx.has_bias and need[2]) else None
            dh = torch.empty(B * T, F, **f32)
            need_adj = ctx.adj_dtype is not None and need[11]
            operands = (out2, store_gate, gate_a, gate_b, d_out2, d_pa, d_pb, dh, d_sg, d_ga, d_gb, d_bsum)
            launch, dx_form, dw_form = dispatch.backward_launch(layer, csr, text.dtype, B, K, F, need[0], need_adj, ctx.dropout, operands)
            entry, graph, writes, tail = _BACKWARD_LAUNCHES[launch]
            dh_amax = torch.zeros(1, **f32) if dx_form == "scaled" else None
            dy = torch.empty(B * T, F, **f32) if (writes == "dY" or (writes == "both" and need_adj)) else None
            # "drop": the keep factors of the forward launch, drawn again from (seed, element)
            after = {"drop": _drop_args(ctx.dropout), "amax": (ptr(dh_amax),)}
            grads = {"dH": (ptr(dh), F), "dY": (ptr(dy), F), "both": (ptr(dh), F, ptr(dy), F)}[writes]
            _capi.check(getattr(lib, entry)(
                ptr(out2), F, ptr(store_gate), ptr(gate_a), ptr(gate_b), ptr(d_out2), F, ptr(d_pa), ptr(d_pb),
                *(ptr(t) for t in graph(csr)), B, T, F, *grads,
                ptr(d_sg), ptr(d_ga), ptr(d_gb), ptr(d_bsum), *(a for name in tail for a in after[name]), st), entry)
            if writes == "dY":   # dY went to memory: dH = A^T.(D.dY) on the transposed CSR
                csr_t = csr.transposed()
                _capi.check(lib.ggcn_aggregate_t(ptr(dy), F, ptr(csr_t.rowptr), ptr(csr_t.colidx), ptr(csr_t.vals),
                                                 ptr(csr.inv_denominators()), B, T, F, ptr(dh), F, st), "ggcn_aggregate_t")
            d_adj = None
            if need_adj:   # dA = D.dY.H^T - c on `hidden` as the forward computed it (float32 for bfloat16 features too)
                hidden = layer.linear(_rows2d(text))
                d_adj = torch.empty(B, T, T, **f32)
                _capi.check(lib.ggcn_adjacency_grad(ptr(dy), F, ptr(hidden), hidden.stride(0), ptr(csr.inv_denominators()), ptr(csr.rowptr),
                                                    ptr(csr.colidx), ptr(csr.vals), B, T, F, ptr(d_adj), st), "ggcn_adjacency_grad")
                if ctx.adj_dtype != torch.float32:
                    d_adj = d_adj.to(ctx.adj_dtype)
            dx = dw = db = None
            if dx_form in ("bf16", "bf16x3"):
                # gradients can be far below fp16's range (f16mx8 would flush them): dX takes the bf16x3 linear, which keeps the fp32
                # exponent range; bfloat16 features: dX in bf16 (the reference's gradient dtype under autocast), rounded in the store
                dx = hostops.linear_packed(lib, st, dh, F, layer._packed_weight(lib, st, transposed=True), B * T, F, K,
                                           out_dtype=torch.bfloat16 if dx_form == "bf16" else torch.float32, tag="(dX)").view(B, T, K)
            elif dx_form is not None:
                dx = torch.empty(B, T, K, **f32)
                if dx_form == "scaled":
                    pack_t = layer._packed_weight(lib, st, transposed=True, precision="f16mx8")
                    _capi.check(lib.ggcn_linear_scaled(ptr(dh), F, ptr(pack_t), ptr(dx), K, B * T, F, K, ptr(dh_amax), st),
                                "ggcn_linear_scaled(dX)")
                else:   # exact-fp32 mode: W^T as a plain matrix, transposed once per weight update
                    wt = hostops.cached(layer, "_wt", hostops.param_key(weight), lambda: weight.detach().t().contiguous())
                    _capi.check(lib.ggcn_linear(ptr(dh), F, ptr(wt), K, None, ptr(dx), K, B * T, F, K, _capi.PREC["fp32"], st),
                                "ggcn_linear(dX)")
            if need[1]:
                x2d = _rows2d(text)
                if dw_form == "bf16":
                    dw = hostops.dweight_bf16(lib, st, x2d, x2d.stride(0), dh, F, B * T, K, F)
                else:
                    # split-precision layers: bf16x3 on the forward's main loop (fp32 exponent range, ~1e-5);
                    # precision "fp32": the exact fp32 MFMA form, which wants 16-byte aligned rows
                    dw = hostops.dweight(lib, st, x2d, x2d.stride(0), dh, F, B * T, K, F, dw_form)
            if d_bsum is not None:   # db = sum_rows dY: per-graph sums from the pass above, added over the graphs
                db = hostops.colsum(lib, st, d_bsum, F, B, F)
        return dx, dw, db, d_sg, d_ga, d_gb, None, None, None, None, None, d_adj


class GraphConvolution(nn.Module):
    """Mean-normalised GCN layer: ``(adj @ (text @ W)) / (rowsum(adj) + 1) + b``."""

    def __init__(self, in_features, out_features, opt=None, bias=True):
        super().__init__()
        self.in_features = in_features
        self.out_features = out_features
        self.weight = nn.Parameter(torch.empty(in_features, out_features, dtype=torch.float32))
        if bias:
            self.bias = nn.Parameter(torch.empty(out_features, dtype=torch.float32))
        else:
            self.register_parameter("bias", None)
        # arithmetic of the dense linear: "bf16x3" (3 bf16 MFMAs per product, ~1e-5 abs, the whole fp32 exponent range),
        # "f16mx8" (fp16 MFMA + one block-scaled fp8 correction MFMA) or "fp32" (exact fp32 MFMA).
        # Default "f16mx8" (26 % faster than "bf16x3", the arithmetic bench.py's headline is measured in).  It meets the
        # 1e-4 parity gate for activations of |x| <= 448 and hidden values below 65504, where the reference's fp32 matmul
        # has no limits -- so the kernels watch exactly that: a sticky device flag (overflow / accuracy window / hidden
        # bound, include/ggcn.h ggcn_range_bits), reported lazily without a device synchronisation (range_guard: after the
        # first forward and every 16th; check_range() asks now).  opt.ggcn_precision / GGCN_PRECISION = "bf16x3" lifts the limits.
        self.precision = getattr(opt, "ggcn_precision", None) or os.environ.get("GGCN_PRECISION", "f16mx8")
        # one-launch layer (fused_layer.hip) when the batch allows it: T <= fused_max_t, binary adjacency, split
        # precision.  128 by default; graphs of 193..256 nodes (ACE cased's ORI_ML = 231) take the eight-wavefront
        # form on their own (takes_fused_path); set 256 to send graphs of 129..192 nodes there as well.
        self.fused = bool(getattr(opt, "ggcn_fused", True)) and os.environ.get("GGCN_FUSED", "1") != "0"
        self.fused_max_t = int(getattr(opt, "ggcn_fused_max_t", None) or os.environ.get("GGCN_FUSED_MAX_T", "128"))
        # The boolean opt-ins, all off by default: each launch sums in another order than the launches it replaces (inside the parity
        # gate, but not bit-equal).  The predicate named beside each holds its rule and its measurements.
        self.bf16_block = _opted_in(opt, "bf16_block")                          # dispatch.takes_bf16_block_path / takes_bf16_folded_eval_path
        self.weighted_backward = _opted_in(opt, "weighted_backward")            # dispatch.takes_weighted_backward / takes_weighted_backward_drop
        self.weighted_dropout = _opted_in(opt, "weighted_dropout")              # dispatch.takes_weighted_dropout
        self.weighted_block = _opted_in(opt, "weighted_block")                  # dispatch.takes_weighted_block_path
        self.wide_backward = _opted_in(opt, "wide_backward")                    # dispatch.takes_wide_backward
        self.weighted_wide_backward = _opted_in(opt, "weighted_wide_backward")  # dispatch.takes_weighted_wide_backward
        # real-valued adjacency (a soft or learned graph), float32 features: graphs of up to weighted_max_t nodes run as ONE launch.
        # 32 by default (ggcn_layer_fused_weighted); 128 adds graphs of 33..128 nodes (ggcn_layer_fused_weighted_wide,
        # takes_weighted_path has the measurements); larger values mean 128.  Off by default: its sums differ from linear +
        # aggregate's in the last bits (both inside the parity gate).
        self.weighted_max_t = int(getattr(opt, "ggcn_weighted_max_t", None) or os.environ.get("GGCN_WEIGHTED_MAX_T", "32"))
        # dense adjacency handed to forward(): None = let the device detect edge weights (one 4-byte
        # read-back per conversion), True = promise 0/1 entries like the reference's (graph.py:66-74)
        # and stay sync-free, False = always keep the values
        self.binary_adj = getattr(opt, "ggcn_binary_adj", None)

    def extra_repr(self):
        return "in_features=%d, out_features=%d, bias=%s, precision=%s" % (
            self.in_features, self.out_features, self.bias is not None, self.precision)

    # -- weight image for the split-precision linears, rebuilt only when the weight changes ----------
    def _packed_weight(self, lib, stream, transposed=False, precision=None):
        """MFMA-order image of W (forward) or W^T (backward's dX) for `precision` (default: the layer's), rebuilt when W
        changes; one image per precision is kept ("f16mx6" layers also need the "f16mx8" image for the shapes the
        fp6 kernel does not take)."""
        w = self.weight
        # the transposed image serves the backward's dX linear: bf16x3 (full range) unless the caller names f16mx8 (the scaled form)
        name = precision or (self.precision if not transposed else "bf16x3")
        name = name if (name in _capi.PACKED and (not transposed or name == "f16mx8")) else "bf16x3"
        K, F = (self.out_features, self.in_features) if transposed else (self.in_features, self.out_features)
        return hostops.cached(self, "_pack", hostops.param_key(w), slot=(name, bool(transposed)), build=lambda: hostops.weight_pack(
            lib, stream, w.detach().contiguous(), self.out_features, K, F, name, transposed))

    def kernel_precision(self, x2d=None, csr=None):
        """The arithmetic a launch really uses: "f16mx6" is taken by the one-launch layer / block for graphs of <= 32
        nodes with K % 32 == 0 and 16-byte aligned fp32 rows; every other shape of such a layer runs "f16mx8" (the same
        scheme with fp8 corrections: same accuracy class, its own weight image)."""
        if self.precision != "f16mx6":
            return self.precision
        ok = (csr is not None and csr.T <= 32 and x2d is not None and x2d.dtype == torch.float32
              and self.in_features % 32 == 0 and x2d.stride(0) % 4 == 0 and x2d.data_ptr() % 16 == 0 and self.fused)
        return "f16mx6" if ok else "f16mx8"

    def _as_csr(self, adj, text):
        if isinstance(adj, BatchedCSR):
            if adj.B != text.shape[0] or adj.T != text.shape[1]:
                raise RuntimeError("CSR is for B=%d,T=%d but text is %s" % (adj.B, adj.T, tuple(text.shape)))
            if adj.device != text.device:
                raise RuntimeError("CSR and text are on different devices")
            return adj
        if not isinstance(adj, torch.Tensor):
            raise TypeError("adj must be a [B,T,T] tensor or a BatchedCSR")
        if adj.dim() != 3 or adj.shape[0] != text.shape[0] or adj.shape[1] != text.shape[1] \
                or adj.shape[2] != text.shape[1]:
            raise RuntimeError("adj %s does not match text %s" % (tuple(adj.shape), tuple(text.shape)))
        if adj.device != text.device:
            raise RuntimeError("adj and text are on different devices")
        return cached_from_dense(adj, binary=self.binary_adj)  # gcn.py:33 accepts any real dtype

    def _check(self, text):
        # float16 features (BASELINE configs[3]) are an extension: the reference itself raises a
        # dtype mismatch for half inputs.  Weights, bias, gates stay float32.
        # bfloat16 features: the layer under torch.autocast(dtype=torch.bfloat16) -- float32 out and pools (the reference's
        # `/ denom` promotes), bf16 dX; every split precision runs the bf16 pair form (BF16_PRECISIONS).
        _require_gpu_f32("text", text, allow_half=True, allow_bf16=True)
        bf16 = text.dtype == torch.bfloat16
        if bf16 and self.precision not in BF16_PRECISIONS:
            raise RuntimeError("bfloat16 features need precision 'bf16x3', 'f16mx8' or 'f16mx6' (all run the bf16 pair form); "
                               "precision=%r does not apply to them" % (self.precision,))
        if self.precision == "f16" and text.dtype != torch.float16:
            raise RuntimeError("precision='f16' (plain fp16 MFMA) is for float16 features only; float32 features take "
                               "'bf16x3', 'f16mx8' or 'fp32'")
        if text.dtype == torch.float16 and self.precision not in _capi.PACKED:
            raise RuntimeError("float16 features need precision='bf16x3' or 'f16mx8' (the exact-fp32 linear is "
                               "fp32 only)")
        if text.dim() != 3 or text.shape[2] != self.in_features:
            raise RuntimeError("text must be [B,T,%d], got %s" % (self.in_features, tuple(text.shape)))
        if self.weight.device != text.device:
            raise RuntimeError("weight is on %s but text is on %s" % (self.weight.device, text.device))
        if bf16:   # every split precision runs the bf16 pair form on the bf16x3 image: nothing below applies
            return
        if self.precision == "f16mx6" and not _capi.has_f16mx6():
            raise RuntimeError("precision='f16mx6' is an experiment this libggcn_hip.so was built without (make -C "
                               "ed-gated-gcn_amd/csrc F16MX6=1); use 'f16mx8'")
        if self.precision not in _capi.PREC:
            raise RuntimeError("unknown precision %r (use 'bf16x3', 'f16mx8', 'f16mx6', 'fp32', or 'f16' for float16 features)"
                               % (self.precision,))

    def validate_range(self, text=None):
        """On-demand range check for ``precision='f16mx8'`` (one pass over the data, one read-back: NOT part of
        ``forward``).  Returns ``{"text_absmax", "weight_absmax"}``; raises ``RuntimeError`` when the fp16 range
        (|v| < 65504, finite) is exceeded -- where f16mx8 would saturate silently (f16mx8_core.h)."""
        lib = _capi.load_library()
        rep = {}
        for name, t in (("weight", self.weight.detach()), ("text", text)):
            if t is None:
                continue
            _require_gpu_f32(name, t, allow_half=True)
            t2 = t.reshape(-1, t.shape[-1])
            if t2.stride(1) != 1:
                t2 = t2.contiguous()
            out = torch.empty(2, dtype=torch.float32, device=t.device)
            with torch.cuda.device(t.device):
                _capi.check(lib.ggcn_absmax(_capi.ptr(t2), 1 if t2.dtype == torch.float16 else 0, t2.stride(0),
                                            t2.shape[0], t2.shape[1], _capi.ptr(out), _capi.stream_of(t.device)),
                            "ggcn_absmax")
            amax, bad = out.tolist()
            rep[name + "_absmax"] = amax
            if bad or amax >= 65504.0:
                raise RuntimeError("%s is outside the range of precision='f16mx8' (max |v| = %g%s; needs finite "
                                   "|v| < 65504): use precision='bf16x3'" % (name, amax, ", non-finite entries" if bad else ""))
        return rep

    def linear(self, x2d):
        """``hidden = text @ W`` (``gcn.py:34``) on [N,in] -> [N,out]."""
        lib = _capi.load_library()
        dev = x2d.device
        with torch.cuda.device(dev):
            st = _capi.stream_of(dev)
            if x2d.dtype == torch.bfloat16:   # float32 hidden from bf16 features: two bf16 MFMAs per product on the bf16x3 image
                y = torch.empty(x2d.shape[0], self.out_features, dtype=torch.float32, device=dev)
                pack = self._packed_weight(lib, st, precision="bf16x3")
                _capi.check(lib.ggcn_linear_bf16(_capi.ptr(x2d), x2d.stride(0), _capi.ptr(pack), _capi.ptr(y), y.stride(0),
                                                 x2d.shape[0], self.in_features, self.out_features, st), "ggcn_linear_bf16")
                return y
            y = torch.empty(x2d.shape[0], self.out_features, dtype=x2d.dtype, device=dev)
            kprec = self.kernel_precision()   # "f16mx6" has no stand-alone linear: f16mx8
            if x2d.dtype == torch.float16:
                pack = self._packed_weight(lib, st, precision=kprec)  # noqa
                _capi.check(lib.ggcn_linear_h(_capi.ptr(x2d), x2d.stride(0), _capi.ptr(pack), _capi.ptr(y),
                                              y.stride(0), x2d.shape[0], self.in_features, self.out_features,
                                              _capi.PREC[kprec], st),
                            "ggcn_linear_h")
                return y
            w = self.weight.detach()
            if not w.is_contiguous():
                w = w.contiguous()
            pack = self._packed_weight(lib, st, precision=kprec) if kprec in _capi.PACKED else None
            _capi.check(lib.ggcn_linear(_capi.ptr(x2d), x2d.stride(0), _capi.ptr(w), w.stride(0),
                                        _capi.ptr(pack), _capi.ptr(y), y.stride(0), x2d.shape[0],
                                        self.in_features, self.out_features, _capi.PREC[kprec], st),
                        "ggcn_linear")
        return y

    def _zero_row(self, F, dev):
        """The all-zero ``mid`` row of the weighted launches of <= 32 nodes ([F] floats, made once per device)."""
        zmid = getattr(self, "_zero_mid", None)
        if zmid is None or zmid.device != dev or zmid.numel() < F:
            zmid = self._zero_mid = torch.zeros(F, dtype=torch.float32, device=dev)
        return zmid

    @staticmethod
    def _differentiable_adj(adj):
        """``adj`` itself when it is a dense floating-point tensor that wants a gradient under grad mode (a soft or learned graph:
        ``gcn.py:33-45`` is differentiable in it), else None.  A ``BatchedCSR`` has no tensor to differentiate."""
        if isinstance(adj, torch.Tensor) and adj.is_floating_point() and adj.requires_grad and torch.is_grad_enabled():
            return adj
        return None

    def _needs_grad(self, text, *gates, adj=None):
        return torch.is_grad_enabled() and (text.requires_grad or self.weight.requires_grad
                                            or (self.bias is not None and self.bias.requires_grad)
                                            or any(g is not None and g.requires_grad for g in gates)
                                            or self._differentiable_adj(adj) is not None)

    WIDE_AUTO_MIN_T = 193     # graphs of 193..256 nodes fill >= 75 % of the 256-row slot of the eight-wavefront kernel
    WIDE_AUTO_MIN_T_FULL = {"f16mx8": 129, "bf16x3": 161}   # shorter graphs: only batches that fill whole rounds of workgroups (one per CU)
    WIDE_AUTO_FILL = 0.9

    def takes_fused_path(self, text, csr):
        """True when ``forward_gated`` will run as ONE launch (``ggcn_layer_fused``): graphs of <= ``fused_max_t``
        nodes (row masks exist up to 256), 0/1 adjacency, float32 features, a split-precision linear.  Beyond
        ``fused_max_t`` (128 by default), graphs of 193..256 nodes (ACE cased: ``ORI_ML = 231``, ``constant.py:267``) take
        the eight-wavefront form (``layer_fused_wide8_kernel``: one workgroup per graph x 256 columns) on their own: it
        wins over linear + aggregate by 15 % on large batches (512 x 231 x 768: 418 vs 492 us) and ties on small ones
        (128 x 231 x 768: 128 vs 134 us).  Shorter graphs leave part of the 256-row slot empty: the second row group runs
        a main loop compiled for its 1-3 live 32-row blocks (f16mx8) and both row groups share the epilogue's row steps,
        which wins when the workgroups fill whole rounds (512 x 129 x 768: 296 vs 302 us, 512 x 160: 324 vs 346, 512 x 192:
        349 vs 416) and loses on a fraction of a round (128 x 129 x 768: 89 vs 79 us, 128 x 160: 95 vs 90) -- those keep the two
        launches (``tools/wide_timing.py``).  The choice depends on the batch size and the device's CU count, and the two
        paths sum in different orders (both inside the parity gate): ``fused_max_t = 256`` (always one launch) or
        ``fused = False`` (never) pin it where bit-reproducibility across batch sizes matters."""
        return dispatch.takes_fused(self, csr, dispatch.Input.of(text))

    def takes_bf16_fused_path(self, text, csr):
        """True when ``forward_gated`` (inference or the forward of training) runs bfloat16 features as ONE launch
        (``ggcn_layer_fused_bf16``): graphs of <= 32 nodes, 0/1 adjacency, a split precision (``BF16_PRECISIONS``).  Graphs of
        33..256 nodes: ``takes_bf16_wide_path``; gate dropout in either launch: ``takes_bf16_dropout_path``.  Anything else
        (longer graphs, weighted adjacencies) takes ``ggcn_linear_bf16`` + ``ggcn_aggregate``, which have no gate dropout: on a
        weighted adjacency ``dropout=`` is refused for bfloat16 features (``takes_weighted_dropout_path`` is float32 only)."""
        return dispatch.takes_bf16_fused(self, csr, dispatch.Input.of(text))

    BF16_WIDE_MIN_FILL = 0.75   # 33..128 nodes: one launch when the graph fills this share of its 64- or 128-row slot

    def takes_bf16_wide_path(self, text, csr):
        """True when ``forward_gated`` runs bfloat16 features of graphs of 33..256 nodes as ONE launch
        (``ggcn_layer_fused_bf16_wide``: the 64- / 128-row slot kernel up to 128 nodes, the eight-wavefront kernel beyond, both
        with the bf16 pair main loop on the bf16x3 image): ``fused``, a precision of ``BF16_PRECISIONS``, 0/1 adjacency, row
        masks on the device.  ``fused_max_t = 256`` sends every such graph there, ``fused = False`` none; in between the
        rule is the measured one (``tools/bf16_wide_timing.py``, H = 768, DESIGN.md 4.2bf: the one launch is the default only
        where its median beat ``ggcn_linear_bf16`` + ``ggcn_aggregate`` by more than the spread between the timing windows):

        * up to ``fused_max_t`` (128 by default) nodes, when the graph fills >= 75 % of its row slot -- 48..64 and 96..128
          nodes (512 x 48: 79 vs 105 us, 512 x 64: 90 vs 122, 512 x 96: 146 vs 187, 512 x 100: 160 vs 199, 512 x 128: 186 vs 261,
          4096 x 100: 1332 vs 1540, 128 x 100: 54 vs 64).  Emptier slots tie or lose on large batches (512 x 33: 74 vs 70,
          512 x 40: 76 vs 77, 4096 x 33: 549 vs 525, 512 x 65: 134 vs 135, 128 x 80: 50 vs 46) and keep the two launches;
        * 129..256 nodes (the 256-row slot), when the workgroups fill whole rounds of the device (``WIDE_AUTO_FILL``):
          512 x 129: 244 vs 265 us, 512 x 160: 262 vs 326, 512 x 192: 297 vs 385, 512 x 231: 352 vs 459, 512 x 256: 378 vs
          508, 256 x 231: 172 vs 236.  A fraction of a round loses or ties for EVERY length, 193..256 included (128 x 129:
          81 vs 68, 128 x 160: 85 vs 76, 128 x 193: 101 vs 96, 128 x 231: 110 vs 104, 128 x 256: 119 vs 115) -- unlike
          float32 bf16x3, whose 193..256 rule is unconditional and whose full-rounds threshold is 161; here it is 129.

        The choice depends on the batch size and the device's CU count, and the two paths sum in different orders (both
        inside the parity gate): ``fused_max_t = 256`` or ``fused = False`` pin it."""
        return dispatch.takes_bf16_wide(self, csr, dispatch.Input.of(text))

    def takes_bf16_dropout_path(self, text, csr):
        """True when the gates' training-mode dropout (``bert_amir5.py:621-625``) of bfloat16 features is drawn inside the
        layer launch (``ggcn_layer_fused_bf16_drop`` for graphs of <= 32 nodes, ``ggcn_layer_fused_bf16_wide`` up to 256):
        one of the two bf16 one-launch paths and an element index below 2^32."""
        return dispatch.takes_bf16_dropout(self, csr, dispatch.Input.of(text))

    def takes_weighted_path(self, text, csr):
        """True when ``forward_gated`` (inference, and the forward under autograd) will run a REAL-valued adjacency (``gcn.py:33``
        accepts any ``adj``) as ONE launch: ``fused``, float32 features on a GPU, a split-precision linear, and

        * graphs of <= 32 nodes (``ggcn_layer_fused_weighted``): every entry of D.A_w inside the plane type
          (``BatchedCSR.graph_ops_weighted``);
        * graphs of 33..``min(weighted_max_t, 128)`` nodes (``ggcn_layer_fused_weighted_wide``) -- ``weighted_max_t`` is 32 by
          default, so this is OPT-IN (``opt.ggcn_weighted_max_t = 128`` / ``GGCN_WEIGHTED_MAX_T=128``): every entry of D.A_w finite
          (``BatchedCSR.graph_ops_weighted_wide``: ceil(T/32)^2 blocks of hi / lo bf16 fragments per graph, built once per
          adjacency tensor, one read-back).  The option is looked at before the graph is asked for anything.

        Anything else takes linear + aggregate.  Gate dropout (``dropout=``) is refused on a real-valued adjacency unless
        ``takes_weighted_dropout_path`` holds (the opt-in ``weighted_dropout``).  The 33..128 launch WINS ON SPARSE AND ON DENSE graphs
        (``tools/weighted_wide_timing.py``, one MI355X, H = 768, f16mx8 / bf16x3, us): 512 x 100 with 3 edges per
        row 189 / 237 vs 226 / 251 (the 0/1 launch on the same pattern: 180 / 225), 1024 x 64: 195 / 235 vs 286 / 319, 512 x 128:
        203 / 248 vs 277 / 313; dense softmax rows 512 x 100: 197 / 244 vs 935 / 943, 1024 x 64: 197 / 243 vs 801 / 825, 512 x 128:
        222 / 268 vs 1389 / 1396.  The operand builder adds 10-15 us (sparse) or 62-229 us (dense) per NEW adjacency tensor -- a
        learned graph pays it every step and still wins (512 x 128 dense: 451 vs 1389).  It stays an option because the two
        paths sum in different orders (2.7e-6..1.2e-5 of the output scale apart, both inside the parity gate)."""
        return dispatch.takes_weighted(self, csr, dispatch.Input.of(text))

    def takes_weighted_dropout_path(self, text, csr):
        """True when ``forward_gated(..., dropout=...)`` on a REAL-valued adjacency draws the gates' keep factors inside the weighted
        launch (``ggcn_layer_fused_weighted_drop`` up to 32 nodes, ``ggcn_layer_fused_weighted_wide_drop`` for
        33..``weighted_max_t``) instead of raising: the option ``weighted_dropout`` (``opt.ggcn_weighted_dropout`` /
        ``GGCN_WEIGHTED_DROPOUT=1``; off by default), B*T*F < 2^32 and ``takes_weighted_path``.  Under autograd the backward is
        ``ggcn_gate_pool_backward_drop`` + ``ggcn_aggregate_t``, or with ``weighted_backward`` one
        ``ggcn_gate_pool_backward_weighted_drop`` launch (``dispatch.takes_weighted_backward_drop``).  Timings:
        ``dispatch.takes_weighted_dropout``."""
        return dispatch.takes_weighted_dropout(self, csr, dispatch.Input.of(text))

    LONG_MAX_T = 512   # include/ggcn.h GGCN_LONG_MAX_T

    def takes_long_path(self, text, csr):
        """True when ``forward_gated`` will run as ONE launch of ``ggcn_layer_fused_h``: half features with
        ``precision="f16"``, graphs of 129..512 nodes (shorter ones leave most of the 512 row slots empty and stay
        with linear + aggregate), K % 64 == 0, F % 8 == 0."""
        return dispatch.takes_long(self, csr, dispatch.Input.of(text))

    def takes_dropout_path(self, text, csr):
        """True when the gates' training-mode dropout (``bert_amir5.py:621-625``) can be drawn inside the layer launch:
        every one-launch form (graphs of <= 256 nodes on the fused path), element index below 2^32."""
        return dispatch.takes_dropout(self, csr, dispatch.Input.of(text))

    def forward_gated(self, text, adj, store_gate=None, pool_gate_a=None, pool_gate_b=None,
                      want_out=True, want_pool_a=False, want_pool_b=False, _internal=False,
                      overlap_partial=None, overlap_reduce=None, dropout=None):
        """``_forward_gated`` between the two halves of the lazy f16mx8 range report (``range_guard``: no device
        synchronisation; a violation of an EARLIER launch raises here)."""
        guarded = (not _internal and self.precision in ("f16mx8", "f16mx6") and isinstance(text, torch.Tensor) and text.is_cuda
                   and text.dtype != torch.bfloat16)   # (bf16 features run no fp16 arithmetic: no range to report)
        if guarded:
            range_guard.before(text.device)
        r = self._forward_gated(text, adj, store_gate, pool_gate_a, pool_gate_b, want_out, want_pool_a, want_pool_b, _internal,
                                overlap_partial, overlap_reduce, dropout)
        if guarded:
            range_guard.after(text.device)
        return r

    def check_range(self):
        """Synchronous verdict of the sticky f16mx8 range flag for this layer's device (one read-back): raises if an
        f16mx8 launch since the last report met |v| >= 65504 or an infinity, an activation beyond the accuracy window
        (|x| > 448), or weights and activations whose hidden values the one-launch layer cannot bound below 65504."""
        range_guard.check(self.weight.device)

    def _forward_gated(self, text, adj, store_gate=None, pool_gate_a=None, pool_gate_b=None,
                       want_out=True, want_pool_a=False, want_pool_b=False, _internal=False,
                       overlap_partial=None, overlap_reduce=None, dropout=None):
        """Layer + gate + max-pool in one aggregation pass.

        Returns ``(out [B,T,F] or None, pool_a [B,F] or None, pool_b [B,F] or None)`` with
        ``out = y * store_gate`` and ``pool_x = max_t (y * pool_gate_x)``, ``y`` being the
        plain layer output.  Gates are ``[B,F]`` (broadcast over tokens).

        One-launch path only (``takes_fused_path``; bfloat16 features: ``takes_bf16_fused_path`` / ``takes_bf16_wide_path``): ``overlap_partial`` (float32 ``[B, ceil(F/64)]``)
        receives this layer's share of ``sum_f pool_a*pool_b``; ``overlap_reduce=(partials, xy)`` makes
        this launch reduce the partials an earlier launch wrote into the scalar ``xy``
        (``bert_amir5.py:638`` without its own launches).

        ``dropout=(p, seed, (stream_store, stream_a, stream_b))`` (one-launch path: ``takes_dropout_path``, or
        ``takes_bf16_dropout_path`` for bfloat16 features): the three gates
        are dropped per (token, feature) like the reference's repeated ``[B,T,H]`` gates (``bert_amir5.py:621-625``);
        stream 0 = not dropped, 1 / 2 = the two independent Bernoulli streams of ``seed`` (``include/ggcn.h``).  Under autograd a
        dropped store gate (stream 1 / 2) wants every pool in use on its own stream (the block's layer 2: ``(2, 2, 0)`` with one
        pool): the backward reads y back from the stored output, and anything else is refused."""
        self._check(text)
        if text.shape[0] == 0:   # an empty batch is a valid input of the reference (gcn.py:30-45): empty outputs
            B, T, F = 0, text.shape[1], self.out_features
            z = text.new_zeros((0, T, F), dtype=torch.float32 if text.dtype == torch.bfloat16 else text.dtype)
            return ((z if want_out else None), (text.new_zeros((0, F), dtype=torch.float32) if want_pool_a else None),
                    (text.new_zeros((0, F), dtype=torch.float32) if want_pool_b else None))
        csr = self._as_csr(adj, text)
        training = not _internal and self._needs_grad(text, store_gate, pool_gate_a, pool_gate_b, adj=adj)
        x2d = None if training else _rows2d(text)
        launch = dispatch.layer_launch(self, text, csr, dropout is not None, x2d)
        if training:   # the same kernels, wrapped in an autograd Function with a HIP backward
            if text.dtype not in (torch.float32, torch.bfloat16):
                raise RuntimeError("training through the HIP layer needs float32 features (or bfloat16 ones)")
            _admit(launch, dropout, False)
            if dropout is not None:
                # the backward recovers y from the stored out = y*sg*k_store: a token whose store factor is 0 leaves nothing to
                # recover, which is exact only for pools that drop the same tokens (include/ggcn.h ggcn_gate_pool_backward_drop)
                ss, sa, sb = dropout[2]
                if ss != 0 and ((want_pool_a and sa != ss) or (want_pool_b and sb != ss)):
                    raise RuntimeError("dropout streams %r: under autograd a pool must share the store gate's keep stream (or the "
                                       "store gate stay undropped, stream 0) -- the backward reads y back from the stored output, "
                                       "which a dropped store gate zeroes" % ((ss, sa, sb),))
            adj_t = self._differentiable_adj(adj)   # a dense `adj` that wants its gradient: one more input, so autograd links it
            if adj_t is not None and csr.T > self.LONG_MAX_T:
                raise RuntimeError("adj.requires_grad with graphs of %d nodes: the adjacency gradient (ggcn_adjacency_grad) takes "
                                   "graphs of up to %d nodes; detach adj or shorten the graphs" % (csr.T, self.LONG_MAX_T))
            out, pa, pb = _GatedLayerFunction.apply(text, self.weight, self.bias, store_gate, pool_gate_a,
                                                    pool_gate_b, self, csr, want_pool_a, want_pool_b, dropout, adj_t)
            return (out if want_out else None), pa, pb
        lib = _capi.load_library()
        (B, T, K), F, dev = text.shape, self.out_features, text.device
        for name, g in (("store_gate", store_gate), ("pool_gate_a", pool_gate_a), ("pool_gate_b", pool_gate_b)):
            if g is not None:
                _require_gpu_f32(name, g)
                _require_gate(name, g, B, F, "%(name)s must be a contiguous [B,F]=[%(B)d,%(F)d] tensor, got %(shape)s")
        _admit(launch, dropout, overlap_partial is not None or overlap_reduce is not None)
        hidden = self.linear(x2d) if launch == "two_launch" else None
        ptr = _capi.ptr
        with torch.cuda.device(dev):
            st = _capi.stream_of(dev)
            out = torch.empty(B * T, F, dtype=torch.float32 if text.dtype == torch.bfloat16 else text.dtype, device=dev) if want_out else None
            pa = torch.empty(B, F, dtype=torch.float32, device=dev) if want_pool_a else None
            pb = torch.empty(B, F, dtype=torch.float32, device=dev) if want_pool_b else None
            bias = None if self.bias is None else self.bias.detach()
            # what every entry takes after its operands: the shape, the three gates, the outputs
            tail = (B, T, K, F, ptr(store_gate), ptr(pool_gate_a), ptr(pool_gate_b), ptr(out), F, ptr(pa), ptr(pb))
            if launch == "two_launch":   # the aggregation of `hidden`, gate and pools in its epilogue
                agg = lib.ggcn_aggregate_h if text.dtype == torch.float16 else lib.ggcn_aggregate
                _capi.check(agg(ptr(hidden), hidden.stride(0), ptr(csr.rowptr), ptr(csr.colidx), ptr(csr.vals), ptr(bias),
                                B, T, *tail[3:], st), "ggcn_aggregate")
            else:
                entry, image, graph, mid, overlap, precision, drop = _LAYER_LAUNCHES[launch]
                kprec = image(self, x2d, csr)
                args = [ptr(x2d), x2d.stride(0), ptr(self._packed_weight(lib, st, precision=kprec)), *map(ptr, graph(csr, kprec)), ptr(bias)]
                if mid:
                    args.append(ptr(self._zero_row(F, dev)))
                args += tail
                if overlap and (overlap_partial is not None or overlap_reduce):
                    args += (ptr(overlap_partial), ptr(overlap_reduce[0]) if overlap_reduce else None, ptr(overlap_reduce[1]) if overlap_reduce else None)
                elif overlap is not None:
                    args += (None, None, None)
                if precision:
                    args.append(_capi.PREC[kprec])
                if drop:
                    args += _drop_args(dropout)
                _capi.check(getattr(lib, entry)(*args, st), entry)
        return (None if out is None else out.view(B, T, F)), pa, pb

    def forward(self, text, adj):
        """``models/gcn.py:30-45``; ``adj`` is the reference's dense [B,T,T] (or a BatchedCSR).  A dense floating-point ``adj``
        with ``requires_grad`` receives its gradient, dense like the reference's (graphs of up to ``LONG_MAX_T`` nodes; longer
        ones raise); a ``BatchedCSR`` has no tensor to differentiate."""
        out, _, _ = self.forward_gated(text, adj)
        return out
