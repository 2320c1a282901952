"""The small pieces of ``BertAmir55.forward`` on either side of the gated block, each as one HIP launch.

* ``gate_mlps``   -- ``models/bert_amir5.py:562-571,621-622``: both gate MLPs from ``aspect`` (the ``[B,T,H]``
  repeat of ``:621-622`` is never made);
* ``scores_and_kl`` -- ``models/bert_amir5.py:645-648``: the ``fc`` / ``scores`` / ``kl`` head without its
  ``[B,T,2H]`` concat and ``[B,T,C]`` product.

Both are differentiable.  ``scores_and_kl``: when a gradient is wanted it runs as ``_ScoresAndKl``, whose backward is one launch
(``ggcn_scores_head_backward``) plus a fixed-order weight product (``ggcn_scores_head_dweight``).  ``gate_mlps``: when ``aspect``
or a gate parameter needs a gradient it runs as ``_GateMlps`` -- the forward launch in its saving form (``ggcn_gate_mlp_save``),
a backward of one launch (``ggcn_gate_mlp_backward``) plus the library's fixed-order ``ggcn_dweight`` / ``ggcn_colsum`` for the
parameters that train.  Without a gradient to compute both take the inference path they always took, bit for bit.  The
classifier takes them in training with ``opt.ggcn_head_backward`` / ``GGCN_HEAD_BACKWARD=1`` and ``opt.ggcn_gate_backward`` /
``GGCN_GATE_BACKWARD=1`` (both off by default: the fused sums differ from the PyTorch ops' in the last bits).
"""
import torch

from . import _capi, hostops
from .gcn import _rows2d


def _transposed(linear, lib, st):
    """[in,out] copy of an nn.Linear weight, rebuilt when the weight changes."""
    w = linear.weight

    def build():
        wc = w.detach().contiguous()
        wt = torch.empty(wc.shape[1], wc.shape[0], dtype=torch.float32, device=w.device)
        _capi.check(lib.ggcn_transpose(_capi.ptr(wc), wc.shape[0], wc.shape[1], wc.stride(0), _capi.ptr(wt), st),
                    "ggcn_transpose")
        return wt
    return hostops.cached(linear, "_ggcn_wt", hostops.param_key(w), build)


def _gate_linears(seq):
    """The two nn.Linear of ``Sequential(Sigmoid, Linear, Sigmoid, Linear, Sigmoid)`` (``bert_amir5.py:562-571``)."""
    mods = list(seq)
    ok = (len(mods) == 5 and all(isinstance(mods[i], torch.nn.Sigmoid) for i in (0, 2, 4))
          and all(isinstance(mods[i], torch.nn.Linear) for i in (1, 3)))
    if not ok:
        raise RuntimeError("gate MLP must be Sequential(Sigmoid, Linear, Sigmoid, Linear, Sigmoid) (bert_amir5.py:562-571)")
    return mods[1], mods[3]


class _GateMlps(torch.autograd.Function):
    """``gate_mlps`` under autograd: the forward is ``ggcn_gate_mlp_save`` (the gates are the bits of a ``no_grad`` call; the
    hidden activations are kept), the backward one ``ggcn_gate_mlp_backward`` launch and, for the parameters that train, the
    library's fixed-order products on what that launch left in ``Z``: ``ggcn_dweight`` (fp32) for ``dW1`` of both gates at
    once and for each ``dW2``, one ``ggcn_colsum`` for the four bias gradients."""

    @staticmethod
    def forward(ctx, aspect, w1a, b1a, w2a, b2a, w1b, b1b, w2b, b2b, linears):
        ctx.set_materialize_grads(False)     # a loss on one gate alone hands the launch a NULL, not zeros
        lib = _capi.load_library()
        a = aspect.detach()
        if a.stride(1) != 1:
            a = a.contiguous()
        B, H = a.shape
        dev = a.device
        ptr = _capi.ptr
        with torch.cuda.device(dev):
            st = _capi.stream_of(dev)
            g1, g2, hid_a, hid_b = (torch.empty(B, H, dtype=torch.float32, device=dev) for _ in range(4))
            wt = [_transposed(lin, lib, st) for lin in linears]
            bias = [None if b is None else b.detach() for b in (b1a, b2a, b1b, b2b)]
            _capi.check(lib.ggcn_gate_mlp_save(ptr(a), a.stride(0), B, H, ptr(wt[0]), ptr(bias[0]), ptr(wt[1]), ptr(bias[1]), ptr(g1),
                                               ptr(wt[2]), ptr(bias[2]), ptr(wt[3]), ptr(bias[3]), ptr(g2), ptr(hid_a), ptr(hid_b), st),
                        "ggcn_gate_mlp_save")
        weights = [w.detach() if w.is_contiguous() else w.detach().contiguous() for w in (w1a, w2a, w1b, w2b)]
        ctx.save_for_backward(a, *weights, hid_a, hid_b, g1, g2)
        ctx.has_bias = tuple(b is not None for b in (b1a, b2a, b1b, b2b))
        return g1, g2

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dg1, dg2):
        a, w1a, w2a, w1b, w2b, hid_a, hid_b, g1, g2 = ctx.saved_tensors
        none = (None,) * 10
        if dg1 is None and dg2 is None:
            return none
        B, H = a.shape
        Hp = (H + 3) & ~3
        need_a = ctx.needs_input_grad[0]
        # (w1, b1, w2, b2) of gate A, then of gate B; a gate that no gradient reached gets None (zero) for its parameters
        live = (dg1 is not None,) * 4 + (dg2 is not None,) * 4
        need = [n and l for n, l in zip(ctx.needs_input_grad[1:9], live)]
        need = [n and (i % 2 == 0 or ctx.has_bias[i // 2]) for i, n in enumerate(need)]
        if not need_a and not any(need):
            return none
        dg1, dg2 = hostops.f32_rows(dg1), hostops.f32_rows(dg2)
        lib = _capi.load_library()
        dev = a.device
        ptr = _capi.ptr
        with torch.cuda.device(dev):
            st = _capi.stream_of(dev)
            new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)   # noqa: E731
            da = new(B, H) if need_a else None
            Z = new(B, 5 * Hp) if any(need) else None
            ldz = 5 * Hp
            _capi.check(lib.ggcn_gate_mlp_backward(ptr(a), a.stride(0), B, H, ptr(w1a), ptr(w2a), ptr(hid_a), ptr(g1), ptr(dg1),
                                                   ptr(w1b), ptr(w2b), ptr(hid_b), ptr(g2), ptr(dg2), ptr(da), H, ptr(Z), ldz, st),
                        "ggcn_gate_mlp_backward")

            def product(x_col, K, other, ld_other):
                """``Z[:, x_col : x_col + K]^T . other`` -> ``[K, H]``, rows = the Linear's outputs: nn.Linear's layout."""
                return hostops.dweight(lib, st, Z[:, x_col:], ldz, other, ld_other, B, K, H, "fp32")

            grads = [None] * 8
            s = Z[:, 4 * Hp:] if Z is not None else None
            if need[0] and need[4] and Hp == H:          # [dz1_A | dz1_B]^T . s: dW1_A over dW1_B in one product
                dw1 = product(0, 2 * H, s, ldz)
                grads[0], grads[4] = dw1[:H], dw1[H:]
            else:
                for g in (0, 1):
                    if need[4 * g]:
                        grads[4 * g] = product(g * Hp, H, s, ldz)
            for g, hid in ((0, hid_a), (1, hid_b)):      # dz2^T . hid
                if need[4 * g + 2]:
                    grads[4 * g + 2] = product((2 + g) * Hp, H, hid, H)
            if need[1] or need[3] or need[5] or need[7]:
                db = hostops.colsum(lib, st, Z, ldz, B, 4 * Hp)
                for i, group in ((1, 0), (3, 2), (5, 1), (7, 3)):    # Z's groups: dz1_A | dz1_B | dz2_A | dz2_B
                    if need[i]:
                        grads[i] = db[group * Hp:group * Hp + H]
        return (da, *grads, None)


def gate_mlps(aspect, gate1_seq, gate2_seq):
    """``gate1(aspect), gate2(aspect)`` -> two contiguous ``[B,H]`` float32 tensors, one launch.  A bfloat16 ``aspect``
    (the BiLSTM under bf16 autocast) is taken as float32 here: [B,H], negligible next to the block.

    Differentiable: with grad enabled and ``aspect`` or any of the eight parameters requiring a gradient the call goes through
    ``_GateMlps`` -- the forward launch in its saving form (``ggcn_gate_mlp_save``: the same gate bits as under ``no_grad``,
    the hidden activations kept), and a backward of one launch (``ggcn_gate_mlp_backward``) plus, for the parameters that
    train, three ``ggcn_dweight`` and one ``ggcn_colsum`` on its ``Z`` output: five calls against about twenty PyTorch
    launches.  The same ``Sequential`` may be passed for both gates (autograd adds the two gradients); a gate that no gradient
    reaches gets ``None`` for its parameters.  The classifier takes it in training with ``opt.ggcn_gate_backward`` /
    ``GGCN_GATE_BACKWARD=1``.  Forward + backward of both gate MLPs alone against the two ``nn.Sequential``
    (``tools/gate_backward_timing.py``, MI355X; ``profiles/gate_backward_timing.txt``; the weights updated every step, so four
    ``ggcn_transpose`` per step are included): 360 against 861 us per step at 256 x 256 (23 against 38 device kernels), but 3183
    against 775 us at 4096 x 768 -- a negative result there: 2290 us of it is the exact-fp32 forward launch (the inference
    kernel, unchanged), 503 us the backward launch, and rocBLAS does the same products on the matrix cores."""
    if isinstance(aspect, torch.Tensor) and aspect.dtype == torch.bfloat16:
        aspect = aspect.float()
    if not (aspect.is_cuda and aspect.dtype == torch.float32 and aspect.dim() == 2):
        raise RuntimeError("aspect must be a float32 [B,H] GPU tensor (no CPU path exists)")
    lib = _capi.load_library()
    B, H = aspect.shape
    la1, la2 = _gate_linears(gate1_seq)
    lb1, lb2 = _gate_linears(gate2_seq)
    for lin in (la1, la2, lb1, lb2):
        if lin.in_features != H or lin.out_features != H:
            raise RuntimeError("gate linears must be %d -> %d" % (H, H))
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in
                                       (aspect,) + tuple(p for lin in (la1, la2, lb1, lb2) for p in (lin.weight, lin.bias))):
        return _GateMlps.apply(aspect, la1.weight, la1.bias, la2.weight, la2.bias, lb1.weight, lb1.bias, lb2.weight, lb2.bias,
                               (la1, la2, lb1, lb2))
    a = aspect if aspect.stride(1) == 1 else aspect.contiguous()
    dev = aspect.device
    with torch.cuda.device(dev):
        st = _capi.stream_of(dev)
        g1 = torch.empty(B, H, dtype=torch.float32, device=dev)
        g2 = torch.empty(B, H, dtype=torch.float32, device=dev)
        bias = lambda l: None if l.bias is None else l.bias.detach()   # noqa: E731
        _capi.check(lib.ggcn_gate_mlp(_capi.ptr(a), a.stride(0), B, H,
                                      _capi.ptr(_transposed(la1, lib, st)), _capi.ptr(bias(la1)),
                                      _capi.ptr(_transposed(la2, lib, st)), _capi.ptr(bias(la2)), _capi.ptr(g1),
                                      _capi.ptr(_transposed(lb1, lib, st)), _capi.ptr(bias(lb1)),
                                      _capi.ptr(_transposed(lb2, lib, st)), _capi.ptr(bias(lb2)), _capi.ptr(g2), st),
                    "ggcn_gate_mlp")
    return g1, g2


def _head_forward(x, aspect, logits, w, fb, dist):
    """The ``ggcn_scores_head`` + ``ggcn_overlap_reduce`` pair on detached float32 operands: ``(scores, kl, what the backward
    needs)``."""
    lib = _capi.load_library()
    B, T, H = x.shape
    C = logits.shape[1]
    x2 = _rows2d(x)
    a = aspect if aspect.stride(1) == 1 else aspect.contiguous()
    lg = logits if logits.stride(1) == 1 else logits.contiguous()
    d = dist.float()                                   # :648 `dist_to_target.float()`
    if d.stride(1) != 1:
        d = d.contiguous()
    if not w.is_contiguous():
        w = w.contiguous()
    dev = x.device
    with torch.cuda.device(dev):
        st = _capi.stream_of(dev)
        scores = torch.empty(B, T, dtype=torch.float32, device=dev)
        part = torch.empty(B, dtype=torch.float32, device=dev)
        kl = torch.empty((), dtype=torch.float32, device=dev)
        _capi.check(lib.ggcn_scores_head(_capi.ptr(x2), x2.stride(0), _capi.ptr(a), a.stride(0), _capi.ptr(lg),
                                         lg.stride(0), _capi.ptr(w), w.stride(0), _capi.ptr(fb), _capi.ptr(d),
                                         d.stride(0), B, T, H, C, _capi.ptr(scores), T, _capi.ptr(part), st),
                    "ggcn_scores_head")
        _capi.check(lib.ggcn_overlap_reduce(_capi.ptr(part), B, 1, _capi.ptr(kl), st), "ggcn_overlap_reduce")
    return scores, kl, (x2, a, lg, w, d, part)


class _ScoresAndKl(torch.autograd.Function):
    """``scores_and_kl`` under autograd: the forward is ``_head_forward`` (the bits of a ``no_grad`` call), the backward one
    ``ggcn_scores_head_backward`` launch and, when ``fc`` trains, the fixed-order weight product ``ggcn_scores_head_dweight``."""

    @staticmethod
    def forward(ctx, x, aspect, logits, weight, bias, dist):
        ctx.set_materialize_grads(False)     # a loss on kl alone (or on scores alone) hands the launch a NULL, not zeros
        scores, kl, (x2, a, lg, w, d, part) = _head_forward(x.detach(), aspect.detach(), logits.detach(), weight.detach(),
                                                            None if bias is None else bias.detach(), dist)
        ctx.save_for_backward(x2, a, lg, w, bias, d, scores, part)
        ctx.dims = tuple(x.shape) + (logits.shape[1],)
        return scores, kl

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_scores, g_kl):
        x2, a, lg, w, bias, d, scores, part = ctx.saved_tensors
        B, T, H, C = ctx.dims
        need_x, need_a, need_lg, need_w, need_b = ctx.needs_input_grad[:5]
        need_b = need_b and bias is not None
        if g_scores is None and g_kl is None:
            return None, None, None, None, None, None
        g_scores, g_kl = hostops.f32_rows(g_scores), hostops.f32_rows(g_kl)
        lib = _capi.load_library()
        dev = x2.device
        ptr = _capi.ptr
        fb = None if bias is None else bias.detach()
        with torch.cuda.device(dev):
            st = _capi.stream_of(dev)
            new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)   # noqa: E731
            dx = new(B, T, H) if need_x else None
            da = new(B, H) if need_a else None
            dlg = new(B, C) if need_lg else None
            G, dc0 = (new(B, 2 * H), new(B)) if (need_w or need_b) else (None, None)
            _capi.check(lib.ggcn_scores_head_backward(
                ptr(x2), x2.stride(0), ptr(a), a.stride(0), ptr(lg), lg.stride(0), ptr(w), w.stride(0), ptr(fb), ptr(d), d.stride(0),
                ptr(scores), T, ptr(part), ptr(g_scores), T, ptr(g_kl), B, T, H, C,
                ptr(dx), H, ptr(da), H, ptr(dlg), C, ptr(G), 2 * H, ptr(dc0), st), "ggcn_scores_head_backward")
            dw = db = None
            if need_w or need_b:
                dw = new(C, 2 * H)
                db = new(C) if bias is not None else None
                ws = torch.empty(lib.ggcn_scores_head_dweight_workspace_bytes(B, H, C), dtype=torch.uint8, device=dev)
                _capi.check(lib.ggcn_scores_head_dweight(ptr(lg), lg.stride(0), ptr(G), 2 * H, ptr(dc0), B, H, C, ptr(dw), 2 * H,
                                                         ptr(db), ptr(ws), st), "ggcn_scores_head_dweight")
        return dx, da, dlg, dw if need_w else None, db if need_b else None, None


def scores_and_kl(x, aspect, logits, fc_linear, dist):
    """``models/bert_amir5.py:645-648``: ``(scores [B,T], kl scalar)`` from the block's gated output ``x [B,T,H]``.
    bfloat16 operands (``aspect`` and ``logits`` under bf16 autocast) are taken as float32 here.

    Differentiable: with grad enabled and ``x``, ``aspect``, ``logits``, ``fc_linear.weight`` or ``fc_linear.bias`` requiring
    a gradient the call goes through ``_ScoresAndKl`` -- the same two forward launches (the same bits as under ``no_grad``),
    and a backward of one launch (``ggcn_scores_head_backward``: ``x`` read once, ``dX`` written once, nothing of size
    ``[B,T,2H]`` or ``[B,T,C]`` kept) plus the fixed-order weight product.  ``dist`` gets no gradient.  Forward + backward
    of the head alone against the literal PyTorch ops (``tools/head_backward_timing.py``, MI355X, taken with this change on top of
    ``af09ca0``; ``profiles/head_backward_timing.txt``): 587 against 1435 us per step at 4096 x 32 x 768 (C = 34), 145 against
    296 us at 256 x 31 x 256; peak memory on top of the inputs 429 against 1556 MiB and 9 against 33 MiB."""
    x, aspect, logits = (t.float() if isinstance(t, torch.Tensor) and t.dtype == torch.bfloat16 else t for t in (x, aspect, logits))
    for name, t in (("x", x), ("aspect", aspect), ("logits", logits)):
        if not (t.is_cuda and t.dtype == torch.float32):
            raise RuntimeError("%s must be a float32 GPU tensor (no CPU path exists)" % name)
    B, T, H = x.shape
    C = logits.shape[1]
    if fc_linear.in_features != 2 * H or fc_linear.out_features != C:
        raise RuntimeError("fc must be Linear(%d, %d)" % (2 * H, C))
    w, fb = fc_linear.weight, fc_linear.bias
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, aspect, logits, w, fb)):
        return _ScoresAndKl.apply(x, aspect, logits, w, fb, dist)
    scores, kl, _ = _head_forward(x, aspect, logits, w.detach(), None if fb is None else fb.detach(), dist)
    return scores, kl


def dense_head(pooled, wt, bias=None, partials=None, f_block=None, signal=None):
    """``logits = pooled @ wt (+ bias)`` -- the share of ``bert_amir5.py:643``'s ``dense`` that reads the block's pooled
    output -- as ONE launch; with ``partials`` (the regulariser's per-graph partial sums of the one-launch block,
    ``bert_amir5.py:638``) the same launch also finishes ``xy``.  ``wt`` is ``[H, C]`` (the ``nn.Linear`` weight slice
    transposed), ``C <= 64``.  Returns ``logits`` or ``(logits, xy)``.  A row's logits are the same bits whatever batch or
    shard the row sits in.  ``signal`` (two zeroed int32 words on the GPU): the launch counts itself done in ``signal[1]``
    (``ggcn_dense_head_signal``), so that another stream can be gated on it without an event (``shard.PooledGather``)."""
    for name, t in (("pooled", pooled), ("wt", wt)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1):
            raise RuntimeError("%s must be a float32 2-D GPU tensor with unit column stride (no CPU path exists)" % name)
    B, H = pooled.shape
    if wt.shape[0] != H:
        raise RuntimeError("wt must be [%d, C], got %s" % (H, tuple(wt.shape)))
    C = wt.shape[1]
    if bias is not None and not (bias.is_cuda and bias.dtype == torch.float32 and tuple(bias.shape) == (C,) and bias.is_contiguous()):
        raise RuntimeError("bias must be a contiguous float32 [%d] GPU tensor" % C)
    lib = _capi.load_library()
    dev = pooled.device
    with torch.cuda.device(dev):
        logits = torch.empty(B, C, dtype=torch.float32, device=dev)
        xy = torch.empty((), dtype=torch.float32, device=dev) if partials is not None else None
        if signal is not None:
            if not (signal.is_cuda and signal.dtype == torch.int32 and signal.numel() >= 2 and signal.is_contiguous()):
                raise RuntimeError("signal must be a contiguous int32 GPU tensor of two words")
            _capi.check(lib.ggcn_dense_head_signal(_capi.ptr(pooled), pooled.stride(0), _capi.ptr(wt), wt.stride(0), _capi.ptr(bias), B, H, C,
                                                   _capi.ptr(logits), C, _capi.ptr(partials), int(f_block or 0), _capi.ptr(xy),
                                                   _capi.ptr(signal), _capi.stream_of(dev)), "ggcn_dense_head_signal")
        else:
            _capi.check(lib.ggcn_dense_head(_capi.ptr(pooled), pooled.stride(0), _capi.ptr(wt), wt.stride(0), _capi.ptr(bias), B, H, C,
                                            _capi.ptr(logits), C, _capi.ptr(partials), int(f_block or 0), _capi.ptr(xy),
                                            _capi.stream_of(dev)), "ggcn_dense_head")
    return logits if partials is None else (logits, xy)
