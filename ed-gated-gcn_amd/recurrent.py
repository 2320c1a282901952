"""The classifier's BiLSTM (``models/bert_amir5.py:557,610``: ``nn.LSTM(9216, 128, bidirectional, batch_first)``) on the HIP path
in inference: ONE input projection and ONE recurrence launch.

* the projection ``G = X . [W_ih_f ; W_ih_r]^T`` (``[B*T, I] x [I, 8 hd]``) is the library's ``ggcn_linear`` at precision bf16x3
  (full fp32 range, no range flag) on a ``ggcn_weight_pack`` image of the two ``weight_ih`` matrices stacked: 1024 x I row-major is
  already the ``[F,K]`` matrix that ``transposed=1`` takes;
* the recurrence is ``ggcn_bilstm_recurrence``: all T steps and both directions in one launch, ``W_hh`` resident in registers,
  ``h`` and ``c`` on the chip, exact fp32.

Forward only.  A call that wants a gradient raises; the classifier takes this path with ``opt.ggcn_hip_lstm`` /
``GGCN_HIP_LSTM=1`` where ``takes_hip_lstm`` holds and keeps ``nn.LSTM`` everywhere else (training, bf16 autocast).  No CPU
fallback: CPU tensors raise.
"""
import torch

from . import _capi
from .csr import tensor_version
from .gcn import _rows2d

HIDDEN = 128                    # the kernel's hd (the reference hard-codes hidden_dim = 128, bert_amir5.py:551)
TILE = _capi.BILSTM_TILE        # sentences per workgroup of ggcn_bilstm_recurrence (include/ggcn.h GGCN_BILSTM_TILE)
PARAMS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0",
          "weight_ih_l0_reverse", "weight_hh_l0_reverse", "bias_ih_l0_reverse", "bias_hh_l0_reverse")


def _module_problem(lstm):
    """Why ``lstm`` is not the module the kernel is built for (None: it is)."""
    if not isinstance(lstm, torch.nn.LSTM):
        return "lstm must be a torch.nn.LSTM, got %s" % type(lstm).__name__
    if lstm.num_layers != 1 or not lstm.bidirectional or not lstm.batch_first or lstm.proj_size != 0:
        return ("lstm must be one bidirectional batch_first layer without projection, got num_layers=%d bidirectional=%s "
                "batch_first=%s proj_size=%d" % (lstm.num_layers, lstm.bidirectional, lstm.batch_first, lstm.proj_size))
    if lstm.hidden_size != HIDDEN:
        return "lstm.hidden_size must be %d, got %d" % (HIDDEN, lstm.hidden_size)
    for name in PARAMS:
        p = getattr(lstm, name, None)
        if p is not None and p.dtype != torch.float32:
            return "lstm.%s must be float32, got %s" % (name, p.dtype)
    return None


def _params(lstm):
    return [getattr(lstm, name, None) for name in PARAMS]


def _wants_grad(x, lstm):
    return torch.is_grad_enabled() and (x.requires_grad or any(p is not None and p.requires_grad for p in _params(lstm)))


def takes_hip_lstm(x, lstm):
    """``bilstm(x, lstm)`` would run: the conditions of its raises as a predicate (no side effect; CPU tensors answer False)."""
    if not (isinstance(x, torch.Tensor) and x.dim() == 3 and x.is_cuda and x.dtype == torch.float32):
        return False
    if _module_problem(lstm) is not None or x.shape[2] != lstm.input_size:
        return False
    if any(p is not None and p.device != x.device for p in _params(lstm)):
        return False
    return not _wants_grad(x, lstm)


def _operands(lstm, lib, st):
    """``(pack of [W_ih_f ; W_ih_r], W_hh_f, W_hh_r, bias_f, bias_r)`` cached on the module, rebuilt when a parameter changes."""
    ps = _params(lstm)
    key = tuple(None if p is None else (p.data_ptr(), tensor_version(p), p.device) for p in ps)
    cached = getattr(lstm, "_ggcn_lstm", None)
    if cached is None or cached[0] != key:
        wih_f, whh_f, bih_f, bhh_f, wih_r, whh_r, bih_r, bhh_r = (None if p is None else p.detach() for p in ps)
        I = lstm.input_size
        prec = _capi.PREC["bf16x3"]
        wcat = torch.cat([wih_f, wih_r], dim=0).contiguous()                     # [8 hd, I]: the [F,K] matrix of transposed=1
        pack = torch.empty(lib.ggcn_weight_pack_bytes(I, 8 * HIDDEN, prec), dtype=torch.uint8, device=wcat.device)
        _capi.check(lib.ggcn_weight_pack(_capi.ptr(wcat), I, I, 8 * HIDDEN, prec, 1, _capi.ptr(pack), st), "ggcn_weight_pack")
        bias_f = None if bih_f is None else (bih_f + bhh_f).contiguous()
        bias_r = None if bih_r is None else (bih_r + bhh_r).contiguous()
        cached = (key, (pack, whh_f.contiguous(), whh_r.contiguous(), bias_f, bias_r))
        lstm._ggcn_lstm = cached
    return cached[1]


def bilstm(x, lstm):
    """``lstm(x)[0]`` for ``x [B,T,I]`` float32 on the GPU and the classifier's ``nn.LSTM``: ``[B,T,2*128]`` float32, contiguous,
    from one ``ggcn_linear`` (bf16x3) and one ``ggcn_bilstm_recurrence`` launch; zero initial state, every one of the T rows run
    (the reference passes the padded batch).  The weight image, the two summed biases and the ``W_hh`` copies are cached on the
    module and rebuilt when a parameter changes.  ``B == 0`` or ``T == 0`` gives an empty tensor without a launch."""
    if not isinstance(x, torch.Tensor) or x.dim() != 3:
        raise TypeError("x must be a 3-d tensor")
    if x.dtype != torch.float32:
        raise RuntimeError("x must be float32, got %s" % x.dtype)
    problem = _module_problem(lstm)
    if problem is not None:
        raise RuntimeError(problem)
    if x.shape[2] != lstm.input_size:
        raise RuntimeError("x %s does not match lstm.input_size %d" % (tuple(x.shape), lstm.input_size))
    if _wants_grad(x, lstm):
        raise RuntimeError("bilstm is forward only: a gradient through the LSTM stays nn.LSTM (call it under torch.no_grad())")
    if not x.is_cuda:
        raise RuntimeError("x is on %s: the HIP path has no CPU fallback" % x.device)
    for name, p in zip(PARAMS, _params(lstm)):
        if p is not None and p.device != x.device:
            raise RuntimeError("lstm.%s is on %s, x on %s: the HIP path has no CPU fallback" % (name, p.device, x.device))
    B, T, I = x.shape
    dev = x.device
    y = torch.empty(B, T, 2 * HIDDEN, dtype=torch.float32, device=dev)
    if B == 0 or T == 0:
        return y
    lib = _capi.load_library()
    x2 = _rows2d(x.detach())
    with torch.cuda.device(dev):
        st = _capi.stream_of(dev)
        pack, whh_f, whh_r, bias_f, bias_r = _operands(lstm, lib, st)
        g = torch.empty(B * T, 8 * HIDDEN, dtype=torch.float32, device=dev)
        _capi.check(lib.ggcn_linear(_capi.ptr(x2), x2.stride(0), None, 0, _capi.ptr(pack), _capi.ptr(g), 8 * HIDDEN, B * T, I, 8 * HIDDEN,
                                    _capi.PREC["bf16x3"], st), "ggcn_linear")
        _capi.check(lib.ggcn_bilstm_recurrence(_capi.ptr(g), 8 * HIDDEN, _capi.ptr(whh_f), _capi.ptr(whh_r), _capi.ptr(bias_f),
                                               _capi.ptr(bias_r), _capi.ptr(y), 2 * HIDDEN, B, T, HIDDEN, st), "ggcn_bilstm_recurrence")
    return y
