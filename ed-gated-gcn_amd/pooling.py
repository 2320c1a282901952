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


def _launch_layers(a, layers):
    """y[b][:, l*Dl:(l+1)*Dl] = a[b] @ layers[l][b] for every l: one launch per group of MAX_LAYERS layers, no concatenation."""
    B, R, C = a.shape
    n, Dl = len(layers), layers[0].shape[2]
    x0 = layers[0]
    if B == 0 or R == 0 or C == 0 or Dl == 0:
        return torch.zeros(B, R, n * Dl, dtype=x0.dtype, device=x0.device)   # as _launch: empty, or the empty sum
    lib = _capi.load_library()
    if x0.stride(2) != 1 or x0.stride(1) < Dl or any(x.stride() != x0.stride() for x in layers):
        layers = [x.contiguous() for x in layers]       # the rare case: the entry takes ONE x_batch and ldx for all layers
        x_batch, ldx = C * Dl, Dl
    else:
        x_batch, ldx = x0.stride(0), x0.stride(1)
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


def subword_pool_layers(transform, layers):
    """``subword_pool(transform, torch.cat(layers, -1))`` bit for bit, without the concatenation (``bert_amir5.py:596,600``):
    ``layers`` is a list or tuple of n >= 1 tensors ``[B,L,Dl]`` of one shape, dtype (float32 or bfloat16) and device -- BERT's
    layer outputs as they are -- and the result is ``[B,T,n*Dl]``; one launch per 16 layers reads each layer where it lies.
    Layers that do not share their strides are made contiguous first.  Empty operands as ``subword_pool``, without a launch.
    The backward is ``subword_pool``'s single transposed launch; each layer that wants a gradient receives its columns of it."""
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
        raise RuntimeError("subword_pool_layers does not differentiate with respect to the transform")
    return _SubwordPoolLayers.apply(transform, *layers)
