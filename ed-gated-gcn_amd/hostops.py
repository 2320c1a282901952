"""What the autograd Functions of this package share on the host side of libggcn_hip.so: the caches of operands derived from
parameters, and the small library products of the backward passes (weight images, ``dW = X^T.dH``, column sums, the bf16x3 linear
on an image), each with its workspace and its return-code check in one place.

The products run inside the caller's ``with torch.cuda.device(dev)`` on the stream handle ``st`` it passes, and look their entry
up on ``lib`` at call time.  Pointers cross as ``ctypes.c_void_p`` (NULL: None), scalars as plain Python numbers.
"""
import os

import torch

from . import _capi
from .csr import tensor_version


def _opted_in(opt, name):
    """A boolean opt-in: on when ``opt.ggcn_<name>`` is true or the environment has ``GGCN_<NAME>=1``."""
    return bool(getattr(opt, "ggcn_" + name, False)) or os.environ.get("GGCN_" + name.upper(), "0") == "1"


def _unless_opted_out(opt, name):
    """A boolean that is on by default: off when ``opt.ggcn_<name>`` is set and false or the environment has ``GGCN_<NAME>=0``."""
    return bool(getattr(opt, "ggcn_" + name, True)) and os.environ.get("GGCN_" + name.upper(), "1") != "0"


def param_key(*tensors):
    """``(data_ptr, version, device)`` per tensor, None for an absent one: what a cache of something derived from them keys on.
    An in-place update moves the version, a re-assigned ``.data`` the pointer."""
    return tuple(None if t is None else (t.data_ptr(), tensor_version(t), t.device) for t in tensors)


def cached(owner, attr, key, build, slot=None):
    """The value kept as ``(key, value)`` under ``owner.<attr>`` -- with ``slot``: in a dict ``{slot: (key, value)}`` there --
    rebuilt by ``build()`` when ``key`` differs.  The attribute appears with the first use."""
    store = getattr(owner, attr, None)
    if slot is not None and not isinstance(store, dict):
        store = {}
        setattr(owner, attr, store)
    hit = store if slot is None else store.get(slot)
    if hit is None or hit[0] != key:
        hit = (key, build())
        if slot is None:
            setattr(owner, attr, hit)
        else:
            store[slot] = hit
    return hit[1]


def f32_rows(t, shape=None):
    """A gradient as contiguous float32 (reshaped to ``shape``): handed on as it lies where it already is, None stays None."""
    if t is None:
        return None
    if shape is not None:
        t = t.reshape(shape)
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()


def workspace(nbytes, dev):
    """Scratch bytes of a library entry, at least 16 (the allocator aligns them beyond the 16 bytes the entries ask for).  The
    ``..._workspace_bytes`` functions return 0 only for dimensions that their entries refuse."""
    return torch.empty(max(16, nbytes), dtype=torch.uint8, device=dev)


def weight_pack(lib, st, w, ldw, K, F, precision, transposed, tag=""):
    """The ``ggcn_weight_pack`` image of the [K,F] matrix ``w`` -- ``transposed``: of ``w^T``, ``w`` stored [F,K] -- for ``precision``."""
    prec = _capi.PREC[precision]
    pack = torch.empty(lib.ggcn_weight_pack_bytes(K, F, prec), dtype=torch.uint8, device=w.device)
    _capi.check(lib.ggcn_weight_pack(_capi.ptr(w), ldw, K, F, prec, 1 if transposed else 0, _capi.ptr(pack), st), "ggcn_weight_pack" + tag)
    return pack


def dweight(lib, st, x, ldx, dh, ldh, rows, K, F, precision):
    """``dW [K,F] = x[:, :K]^T . dh[:, :F]`` over ``rows`` rows, float32, fixed order: ``precision`` "bf16x3" or "fp32"."""
    prec = _capi.PREC[precision]
    dw = torch.empty(K, F, dtype=torch.float32, device=dh.device)
    ws = workspace(lib.ggcn_dweight_workspace_bytes(rows, K, F, prec), dh.device)
    _capi.check(lib.ggcn_dweight(_capi.ptr(x), ldx, _capi.ptr(dh), ldh, rows, K, F, _capi.ptr(dw), F, prec, _capi.ptr(ws), st), "ggcn_dweight")
    return dw


def dweight_bf16(lib, st, x, ldx, dh, ldh, rows, K, F):
    """``dweight`` for bfloat16 ``x`` (float32 ``dh`` and result): the bf16 pair form of the bf16x3 product."""
    dw = torch.empty(K, F, dtype=torch.float32, device=dh.device)
    ws = workspace(lib.ggcn_dweight_bf16_workspace_bytes(rows, K, F), dh.device)
    _capi.check(lib.ggcn_dweight_bf16(_capi.ptr(x), ldx, _capi.ptr(dh), ldh, rows, K, F, _capi.ptr(dw), F, _capi.ptr(ws), st), "ggcn_dweight_bf16")
    return dw


def colsum(lib, st, x, ld, rows, F):
    """``[F]`` float32 column sums of ``x[:rows, :F]``, fixed order."""
    out = torch.empty(F, dtype=torch.float32, device=x.device)
    ws = workspace(lib.ggcn_colsum_workspace_bytes(F), x.device)
    _capi.check(lib.ggcn_colsum(_capi.ptr(x), ld, rows, F, _capi.ptr(out), _capi.ptr(ws), st), "ggcn_colsum")
    return out


def linear_packed(lib, st, x, ldx, pack, rows, K, F, out_dtype=torch.float32, tag=""):
    """``[rows,F] = x[:, :K] . W`` on the bf16x3 image ``pack`` of W (the fp32 exponent range): ``ggcn_linear``, or for a bfloat16
    result ``ggcn_linear_out_bf16`` (rounded to nearest even in the store)."""
    y = torch.empty(rows, F, dtype=out_dtype, device=x.device)
    if out_dtype == torch.bfloat16:
        _capi.check(lib.ggcn_linear_out_bf16(_capi.ptr(x), ldx, _capi.ptr(pack), _capi.ptr(y), F, rows, K, F, st), "ggcn_linear_out_bf16" + tag)
    else:
        _capi.check(lib.ggcn_linear(_capi.ptr(x), ldx, None, 0, _capi.ptr(pack), _capi.ptr(y), F, rows, K, F, _capi.PREC["bf16x3"], st),
                    "ggcn_linear" + tag)
    return y
