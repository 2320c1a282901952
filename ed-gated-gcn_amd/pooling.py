"""Sub-word -> word pooling on the HIP path: ``x = torch.bmm(transform, x)``
(``models/bert_amir5.py:600``; the transform of ``data_utils.py:749-766`` holds ``1/l`` on the ``l``
sub-word positions of each word and zeros elsewhere, x is the 9216-wide concatenation of the 12
BERT layers, ``bert_amir5.py:596``).  ``ggcn_subword_pool`` multiplies only the non-zeros and reads
each selected row of x once; the backward ``dX = transformᵀ · dY`` is the same kernel with the
strides of ``transform`` swapped (``train.py:120`` back-propagates into BERT through this step).
No CPU fallback: CPU tensors raise.  ``x`` may be bfloat16 (BERT under ``torch.autocast(dtype=torch.bfloat16)``):
the sums run in fp32 and the result comes back in bf16, as ``torch.bmm`` gives under autocast.
"""
import torch

from . import _capi


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
