"""Sub-word -> word pooling on the HIP path: ``x = torch.bmm(transform, x)``
(``models/bert_amir5.py:600``; the transform of ``data_utils.py:749-766`` holds ``1/l`` on the ``l``
sub-word positions of each word and zeros elsewhere, x is the 9216-wide concatenation of the 12
BERT layers, ``bert_amir5.py:596``).  ``ggcn_subword_pool`` multiplies only the non-zeros and reads
each selected row of x once; the backward ``dX = transformᵀ · dY`` is the same kernel with the
strides of ``transform`` swapped (``train.py:120`` back-propagates into BERT through this step).
No CPU fallback: CPU tensors raise.  ``x`` may be bfloat16 (BERT under ``torch.autocast(dtype=torch.bfloat16)``):
the sums run in fp32 and the result comes back in bf16, as ``torch.bmm`` gives under autocast.

``subword_pool_layers`` takes BERT's layer outputs as a list, before ``bert_amir5.py:596`` concatenates them:
``ggcn_subword_pool_layers`` pools every layer into its own columns of the result in one launch, so the ``[B,L,9216]`` copy that
``torch.cat`` writes only to have half of its rows read again is never made.  Same sums, same bits, same backward launch.

``anchor_pool_layers`` serves the baselines ``bert_ed`` / ``bertdm`` (``models/bert_ed.py:46-62``, ``models/bertdm.py:164-198``),
which keep of all pooled words only the anchor's row and two masked max-pools: ``ggcn_anchor_pool_layers`` goes from the layer
list to that ``[B, 3*n*Dl]`` in one launch and never forms ``[B,T,n*Dl]``; ``anchor_pool_formula`` is the same step as the
reference's PyTorch ops on pooled words that exist (the composed path: differentiable, same bits).
"""
import ctypes

import torch

from . import _capi

MAX_LAYERS = _capi.POOL_MAX_LAYERS   # layers per ggcn_subword_pool_layers launch


def _check(name, t, dims, allow_bf16=False):
    if not isinstance(t, torch.Tensor) or t.dim() != dims:
        raise TypeError("%s must be a %d-d tensor" % (name, dims))
    if not t.is_cuda:
        raise RuntimeError("%s is on %s: the HIP path has no CPU fallback" % (name, t.device))
    if t.dtype != torch.float32 and not (allow_bf16 and t.dtype == torch.bfloat16):
        raise RuntimeError("%s must be float32%s, got %s" % (name, " or bfloat16" if allow_bf16 else "", t.dtype))


def _launch(a, x, swap):
    """y[b] = a[b] @ x[b] (swap=False) or a[b].T @ x[b] (swap=True); a strided, x/y row-contiguous."""
    B, R, C = a.shape
    sb, sr, sc = a.stride()
    if swap:
        R, C, sr, sc = C, R, sc, sr
    D = x.shape[2]
    if B == 0 or R == 0 or C == 0 or D == 0:
        # torch.bmm takes empty operands: an empty result, or the empty sum (zeros) when only C is 0; nothing to launch
        return torch.zeros(B, R, D, dtype=x.dtype, device=x.device)
    lib = _capi.load_library()
    if x.stride(2) != 1:
        x = x.contiguous()
    y = torch.empty(B, R, D, dtype=x.dtype, device=x.device)
    fn = lib.ggcn_subword_pool_bf16 if x.dtype == torch.bfloat16 else lib.ggcn_subword_pool
    with torch.cuda.device(x.device):
        st = _capi.stream_of(x.device)
        _capi.check(fn(_capi.ptr(a), sb, sr, sc, _capi.ptr(x), x.stride(0), x.stride(1),
                                          _capi.ptr(y), y.stride(0), y.stride(1), B, R, C, D, st),
                    "ggcn_subword_pool")
    return y


class _SubwordPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, transform, x):
        ctx.save_for_backward(transform)
        return _launch(transform, x, False)

    @staticmethod
    def backward(ctx, dy):
        (transform,) = ctx.saved_tensors
        dx = _launch(transform, dy.contiguous(), True) if ctx.needs_input_grad[1] else None
        return None, dx    # the transform is data (data_utils.py:749-766), never a parameter


def subword_pool(transform, x):
    """``torch.bmm(transform, x)`` for a sparse ``transform [B,T,L]`` (any strides) and ``x [B,L,D]``.  Empty operands are taken
    as ``torch.bmm`` takes them, without a launch: B, T or D = 0 gives an empty ``[B,T,D]``, L = 0 gives zeros."""
    _check("transform", transform, 3)
    _check("x", x, 3, allow_bf16=True)
    if transform.shape[0] != x.shape[0] or transform.shape[2] != x.shape[1]:
        raise RuntimeError("transform %s does not match x %s" % (tuple(transform.shape), tuple(x.shape)))
    if transform.device != x.device:
        raise RuntimeError("transform and x are on different devices")
    if transform.requires_grad:
        raise RuntimeError("subword_pool does not differentiate with respect to the transform")
    return _SubwordPool.apply(transform, x)


def _one_layout(layers):
    """``(layers, x_batch, ldx)``: the layers where they lie when they share their strides (rows of unit stride, at least Dl
    apart), else contiguous copies -- the rare case: the entries take ONE x_batch and ldx for all layers."""
    x0 = layers[0]
    C, Dl = x0.shape[1], x0.shape[2]
    if x0.stride(2) != 1 or x0.stride(1) < Dl or any(x.stride() != x0.stride() for x in layers):
        return [x.contiguous() for x in layers], C * Dl, Dl
    return layers, x0.stride(0), x0.stride(1)


def _launch_layers(a, layers):
    """y[b][:, l*Dl:(l+1)*Dl] = a[b] @ layers[l][b] for every l: one launch per group of MAX_LAYERS layers, no concatenation."""
    B, R, C = a.shape
    n, Dl = len(layers), layers[0].shape[2]
    x0 = layers[0]
    if B == 0 or R == 0 or C == 0 or Dl == 0:
        return torch.zeros(B, R, n * Dl, dtype=x0.dtype, device=x0.device)   # as _launch: empty, or the empty sum
    lib = _capi.load_library()
    layers, x_batch, ldx = _one_layout(layers)
    y = torch.empty(B, R, n * Dl, dtype=x0.dtype, device=x0.device)
    sb, sr, sc = a.stride()
    with torch.cuda.device(x0.device):
        st = _capi.stream_of(x0.device)
        for l0 in range(0, n, MAX_LAYERS):
            group = layers[l0:l0 + MAX_LAYERS]
            ptrs = (ctypes.c_void_p * len(group))(*[x.data_ptr() for x in group])    # host array, read during the call
            y_cols = ctypes.c_void_p(y.data_ptr() + l0 * Dl * y.element_size())
            _capi.check(lib.ggcn_subword_pool_layers(_capi.ptr(a), sb, sr, sc, ptrs, len(group), int(x0.dtype == torch.bfloat16),
                                                     x_batch, ldx, y_cols, y.stride(0), y.stride(1), B, R, C, Dl, st),
                        "ggcn_subword_pool_layers")
    return y


class _SubwordPoolLayers(torch.autograd.Function):
    @staticmethod
    def forward(ctx, transform, *layers):
        ctx.save_for_backward(transform)
        ctx.width = layers[0].shape[2]
        return _launch_layers(transform, layers)

    @staticmethod
    def backward(ctx, dy):
        (transform,) = ctx.saved_tensors
        need = ctx.needs_input_grad[1:]
        if not any(need):
            return (None,) * (1 + len(need))
        # one transposed launch on the whole [B,T,n*Dl] gradient; a layer receives its columns of that buffer as a view -- what
        # the backward of torch.cat hands out after _SubwordPool's, with the same bits
        dx = _launch(transform, dy.contiguous(), True)
        w = ctx.width
        return (None,) + tuple(dx[:, :, l * w:(l + 1) * w] if k else None for l, k in enumerate(need))


def _check_layers(who, transform, layers):
    """The operand checks ``subword_pool_layers`` and ``anchor_pool_layers`` share."""
    _check("transform", transform, 3)
    if not isinstance(layers, (list, tuple)) or len(layers) == 0:
        raise TypeError("layers must be a non-empty list or tuple of 3-d tensors")
    for i, x in enumerate(layers):
        _check("layers[%d]" % i, x, 3, allow_bf16=True)
    x0 = layers[0]
    for i, x in enumerate(layers):
        if x.shape != x0.shape or x.dtype != x0.dtype:
            raise RuntimeError("layers[%d] %s %s does not match layers[0] %s %s"
                               % (i, tuple(x.shape), x.dtype, tuple(x0.shape), x0.dtype))
        if x.device != x0.device:
            raise RuntimeError("layers[%d] and layers[0] are on different devices" % i)
    if transform.shape[0] != x0.shape[0] or transform.shape[2] != x0.shape[1]:
        raise RuntimeError("transform %s does not match layers %s" % (tuple(transform.shape), tuple(x0.shape)))
    if transform.device != x0.device:
        raise RuntimeError("transform and layers are on different devices")
    if transform.requires_grad:
        raise RuntimeError("%s does not differentiate with respect to the transform" % who)


def subword_pool_layers(transform, layers):
    """``subword_pool(transform, torch.cat(layers, -1))`` bit for bit, without the concatenation (``bert_amir5.py:596,600``):
    ``layers`` is a list or tuple of n >= 1 tensors ``[B,L,Dl]`` of one shape, dtype (float32 or bfloat16) and device -- BERT's
    layer outputs as they are -- and the result is ``[B,T,n*Dl]``; one launch per 16 layers reads each layer where it lies.
    Layers that do not share their strides are made contiguous first.  Empty operands as ``subword_pool``, without a launch.
    The backward is ``subword_pool``'s single transposed launch; each layer that wants a gradient receives its columns of it."""
    _check_layers("subword_pool_layers", transform, layers)
    return _SubwordPoolLayers.apply(transform, *layers)


def _check_index(name, t, B, device):
    if not isinstance(t, torch.Tensor) or t.dim() != 1:
        raise TypeError("%s must be a 1-d tensor" % name)
    if t.dtype != torch.int64:
        raise RuntimeError("%s must be int64, got %s" % (name, t.dtype))
    if t.shape[0] != B:
        raise RuntimeError("%s %s does not match the %d sentences of the layers" % (name, tuple(t.shape), B))
    if t.device != device:
        raise RuntimeError("%s and layers are on different devices" % name)


def anchor_pool_formula(v, anchor, length=None, sides=True):
    """The composed path's second half, as PyTorch ops on the pooled words ``v [B,T,D]`` (differentiable): the anchor word's row
    (``bert_ed.py:55-62``) and, with ``sides``, ``bertdm.py:116-140,170-185`` -- multiply by the 0/1 masks "up to and including
    the anchor" and "after the anchor, inside the sentence", add ones, max over the words, subtract ones.  Returns the row
    ``[B,D]`` (in ``v``'s dtype), or ``(row, pooled [B,2*D] float32)``.  ``anchor`` and ``length`` are clamped to ``[0,T-1]`` and
    ``[0,T]`` as ``ggcn_anchor_pool_layers`` clamps them."""
    B, T, _ = v.shape
    a = anchor.clamp(0, T - 1)
    row = v[torch.arange(B, device=v.device), a]
    if not sides:
        return row
    m = torch.arange(T, device=v.device)[None, :]
    mask_l = (m < a[:, None] + 1).float()                                        # bertdm.py:123-131
    mask_r = (m > a[:, None]).float() * (m < length.clamp(0, T)[:, None]).float()
    left = v * mask_l[:, :, None] + 1.0                                          # :176-179 (bf16 v: promoted to float32)
    right = v * mask_r[:, :, None] + 1.0
    return row, torch.cat((left.max(dim=1)[0], right.max(dim=1)[0]), 1) - 1.0    # :182-185


def anchor_pool_layers(transform, layers, anchor, length=None, sides=True):
    """From BERT's layer list to what the baselines' final linear reads, in one launch (``ggcn_anchor_pool_layers``):
    ``bert_ed.py:46-62`` (``sides=False``: the anchor word's pooled row, ``[B,n*Dl]`` in the layers' dtype) and
    ``bertdm.py:164-198`` (``sides=True``: that row, the max-pool over the words up to and including the anchor and the one over
    the words after it and inside the sentence, ``[B,3*n*Dl]`` float32 -- the reference's type promotion under bf16 autocast
    too).  Bit for bit ``anchor_pool_formula(subword_pool_layers(transform, layers), anchor, length, sides)``, the composed
    path, but ``[B,T,n*Dl]`` is never formed.  ``transform`` and ``layers`` as ``subword_pool_layers`` takes and checks them;
    ``anchor`` and ``length`` are int64 ``[B]`` on the layers' device, read and clamped by the kernel (no host read: the call
    captures into a hipGraph); ``length`` is required with ``sides``.  More than 16 layers take one launch per group of 16.
    B = 0 or Dl = 0 gives an empty result and L = 0 zeros, without a launch; T = 0 raises (there is no anchor word).
    Forward only: BERT is frozen where the reference trains these models (``train.py:43-44``)."""
    _check_layers("anchor_pool_layers", transform, layers)
    x0 = layers[0]
    B, R, C = transform.shape
    n, Dl = len(layers), x0.shape[2]
    _check_index("anchor", anchor, B, x0.device)
    if sides:
        if length is None:
            raise TypeError("anchor_pool_layers needs length with sides=True")
        _check_index("length", length, B, x0.device)
    if any(x.requires_grad for x in layers):
        raise RuntimeError("anchor_pool_layers is forward only: for a layer that requires grad take the composed path, "
                           "anchor_pool_formula(subword_pool_layers(transform, layers), anchor, length, sides)")
    if R == 0:
        raise RuntimeError("transform %s has no words: there is no anchor row" % (tuple(transform.shape),))
    width = n * Dl
    out_dtype = torch.float32 if sides else x0.dtype
    if B == 0 or Dl == 0 or C == 0:
        return torch.zeros(B, (3 if sides else 1) * width, dtype=out_dtype, device=x0.device)   # empty, or the empty sums
    lib = _capi.load_library()
    layers, x_batch, ldx = _one_layout(layers)
    z = torch.empty(B, (3 if sides else 1) * width, dtype=torch.float32, device=x0.device)
    anchor = anchor.contiguous()
    length = length.contiguous() if sides else None
    sb, sr, sc = transform.stride()
    with torch.cuda.device(x0.device):
        st = _capi.stream_of(x0.device)
        for l0 in range(0, n, MAX_LAYERS):
            group = layers[l0:l0 + MAX_LAYERS]
            ptrs = (ctypes.c_void_p * len(group))(*[x.data_ptr() for x in group])    # host array, read during the call
            z_cols = ctypes.c_void_p(z.data_ptr() + l0 * Dl * 4)
            _capi.check(lib.ggcn_anchor_pool_layers(_capi.ptr(transform), sb, sr, sc, ptrs, len(group), int(x0.dtype == torch.bfloat16),
                                                    x_batch, ldx, _capi.ptr(anchor), _capi.ptr(length), int(bool(sides)),
                                                    z_cols, z.stride(0), width, B, R, C, Dl, st),
                        "ggcn_anchor_pool_layers")
    return z if sides else z.to(x0.dtype)      # (bf16 layers: Z is float32 at the C entry; one small elementwise kernel more)
