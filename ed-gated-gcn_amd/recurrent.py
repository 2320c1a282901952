"""The classifier's BiLSTM (``models/bert_amir5.py:557,610``: ``nn.LSTM(9216, 128, bidirectional, batch_first)``) on the HIP path:
in inference ONE input projection and ONE recurrence launch (``bilstm``), in training the same two in their saving form and a
one-launch backward (``bilstm_train``).

* the projection ``G = X . [W_ih_f ; W_ih_r]^T`` (``[B*T, I] x [I, 8 hd]``) is the library's ``ggcn_linear`` at precision bf16x3
  (full fp32 range, no range flag) on a ``ggcn_weight_pack`` image of the two ``weight_ih`` matrices stacked: 1024 x I row-major is
  already the ``[F,K]`` matrix that ``transposed=1`` takes;
* the recurrence is ``ggcn_bilstm_recurrence``: all T steps and both directions in one launch, ``W_hh`` resident in registers,
  ``h`` and ``c`` on the chip, exact fp32.

``bilstm`` is forward only.  A call that wants a gradient raises; the classifier takes this path with ``opt.ggcn_hip_lstm`` /
``GGCN_HIP_LSTM=1`` where ``takes_hip_lstm`` holds and keeps ``nn.LSTM`` everywhere else (training, bf16 autocast).  No CPU
fallback: CPU tensors raise.

``bilstm_train`` is the differentiable form (``x`` and all eight parameters): ``ggcn_bilstm_recurrence_save`` writes the
activated gates over ``G`` and keeps ``c`` and the ``h`` each step read; the backward is ONE ``ggcn_bilstm_recurrence_backward``
launch (all T steps, both directions, time walked backwards, ``dc`` and the recurrent ``dh`` on the chip) whose ``dG`` feeds the
library's fixed-order products: ``ggcn_dweight`` for ``[W_ih_f ; W_ih_r]`` and the two ``W_hh``, ``ggcn_colsum`` for the biases,
``ggcn_linear`` for ``dX`` -- each skipped where no gradient is wanted.  The classifier takes it in training with
``opt.ggcn_hip_lstm_backward`` / ``GGCN_HIP_LSTM_BACKWARD=1`` where ``takes_hip_lstm_train`` holds (off by default).
"""
import ctypes

import torch

from . import _capi, hostops, pooling
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


def lstm_wants_grad(x, lstm):
    """A call on ``x`` and ``lstm`` wants a gradient: grad is enabled and ``x`` or a parameter of the module requires one."""
    return torch.is_grad_enabled() and (x.requires_grad or any(p is not None and p.requires_grad for p in _params(lstm)))


def takes_hip_lstm_train(x, lstm):
    """``bilstm_train(x, lstm)`` would run: the conditions of its raises as a predicate (no side effect; CPU tensors answer
    False).  Nothing about gradients: ``bilstm_train`` serves a call with and without one."""
    if not (isinstance(x, torch.Tensor) and x.dim() == 3 and x.is_cuda and x.dtype == torch.float32):
        return False
    if _module_problem(lstm) is not None or x.shape[2] != lstm.input_size:
        return False
    return not any(p is not None and p.device != x.device for p in _params(lstm))


def takes_hip_lstm(x, lstm):
    """``bilstm(x, lstm)`` would run: the conditions of its raises as a predicate (no side effect; CPU tensors answer False)."""
    return takes_hip_lstm_train(x, lstm) and not lstm_wants_grad(x, lstm)


def _operands(lstm, lib, st):
    """``(pack of [W_ih_f ; W_ih_r], W_hh_f, W_hh_r, bias_f, bias_r)`` cached on the module, rebuilt when a parameter changes."""
    ps = _params(lstm)

    def build():
        wih_f, whh_f, bih_f, bhh_f, wih_r, whh_r, bih_r, bhh_r = (None if p is None else p.detach() for p in ps)
        I = lstm.input_size
        wcat = torch.cat([wih_f, wih_r], dim=0).contiguous()                     # [8 hd, I]: the [F,K] matrix of transposed=1
        pack = hostops.weight_pack(lib, st, wcat, I, I, 8 * HIDDEN, "bf16x3", True)
        bias_f = None if bih_f is None else (bih_f + bhh_f).contiguous()
        bias_r = None if bih_r is None else (bih_r + bhh_r).contiguous()
        return pack, whh_f.contiguous(), whh_r.contiguous(), bias_f, bias_r
    return hostops.cached(lstm, "_ggcn_lstm", hostops.param_key(*ps), build)


def _check(x, lstm, forward_only):
    """The raises of ``bilstm`` (``forward_only``) and of ``bilstm_train``, in one order and with one set of texts."""
    if not isinstance(x, torch.Tensor) or x.dim() != 3:
        raise TypeError("x must be a 3-d tensor")
    if x.dtype != torch.float32:
        raise RuntimeError("x must be float32, got %s" % x.dtype)
    problem = _module_problem(lstm)
    if problem is not None:
        raise RuntimeError(problem)
    if x.shape[2] != lstm.input_size:
        raise RuntimeError("x %s does not match lstm.input_size %d" % (tuple(x.shape), lstm.input_size))
    if forward_only and lstm_wants_grad(x, lstm):
        raise RuntimeError("bilstm is forward only: a gradient through the LSTM stays nn.LSTM (call it under torch.no_grad())")
    if not x.is_cuda:
        raise RuntimeError("x is on %s: the HIP path has no CPU fallback" % x.device)
    for name, p in zip(PARAMS, _params(lstm)):
        if p is not None and p.device != x.device:
            raise RuntimeError("lstm.%s is on %s, x on %s: the HIP path has no CPU fallback" % (name, p.device, x.device))


def bilstm(x, lstm):
    """``lstm(x)[0]`` for ``x [B,T,I]`` float32 on the GPU and the classifier's ``nn.LSTM``: ``[B,T,2*128]`` float32, contiguous,
    from one ``ggcn_linear`` (bf16x3) and one ``ggcn_bilstm_recurrence`` launch; zero initial state, every one of the T rows run
    (the reference passes the padded batch).  The weight image, the two summed biases and the ``W_hh`` copies are cached on the
    module and rebuilt when a parameter changes.  ``B == 0`` or ``T == 0`` gives an empty tensor without a launch."""
    _check(x, lstm, forward_only=True)
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
        g = hostops.linear_packed(lib, st, x2, x2.stride(0), pack, B * T, I, 8 * HIDDEN)
        _capi.check(lib.ggcn_bilstm_recurrence(_capi.ptr(g), 8 * HIDDEN, _capi.ptr(whh_f), _capi.ptr(whh_r), _capi.ptr(bias_f),
                                               _capi.ptr(bias_r), _capi.ptr(y), 2 * HIDDEN, B, T, HIDDEN, st), "ggcn_bilstm_recurrence")
    return y


def _dx_operand(lstm, lib, st):
    """The ``ggcn_weight_pack`` image of ``[W_ih_f ; W_ih_r]`` as the ``[K = 8 hd, F = I]`` matrix it is (``transposed=0``): the
    operand of ``dX = dG . [W_ih_f ; W_ih_r]``.  Cached on the module under ``_operands``' key, built only when ``x`` wants a
    gradient."""
    ps = _params(lstm)
    I = lstm.input_size
    return hostops.cached(lstm, "_ggcn_lstm_dx", hostops.param_key(*ps), lambda: hostops.weight_pack(
        lib, st, torch.cat([ps[0].detach(), ps[4].detach()], dim=0).contiguous(), I, 8 * HIDDEN, I, "bf16x3", False))


class _BilstmTrain(torch.autograd.Function):
    """``bilstm`` under autograd: the projection, then ``ggcn_bilstm_recurrence_save`` in place on ``G`` (the bits of
    ``bilstm``'s ``y``); the backward is one ``ggcn_bilstm_recurrence_backward`` launch and, for what wants a gradient, the
    library's fixed-order products on its ``dG``."""

    @staticmethod
    def forward(ctx, x, lstm, *params):
        B, T, I = x.shape
        dev = x.device
        ctx.lstm, ctx.dims = lstm, (B, T, I)
        y = torch.empty(B, T, 2 * HIDDEN, dtype=torch.float32, device=dev)
        if B == 0 or T == 0:
            return y
        lib = _capi.load_library()
        ptr = _capi.ptr
        x2 = _rows2d(x.detach())
        with torch.cuda.device(dev):
            st = _capi.stream_of(dev)
            pack, whh_f, whh_r, bias_f, bias_r = _operands(lstm, lib, st)
            g = hostops.linear_packed(lib, st, x2, x2.stride(0), pack, B * T, I, 8 * HIDDEN)
            c = torch.empty(B * T, 2 * HIDDEN, dtype=torch.float32, device=dev)
            hprev = torch.empty(B * T, 2 * HIDDEN, dtype=torch.float32, device=dev)
            _capi.check(lib.ggcn_bilstm_recurrence_save(ptr(g), 8 * HIDDEN, ptr(whh_f), ptr(whh_r), ptr(bias_f), ptr(bias_r), ptr(y),
                                                        2 * HIDDEN, B, T, HIDDEN, ptr(g), ptr(c), ptr(hprev), st),
                        "ggcn_bilstm_recurrence_save")
        # what the backward reads of the module, under autograd's version check: W_hh always, the two W_ih only where dX is formed
        w_ih = (params[0], params[4]) if ctx.needs_input_grad[0] else ()
        ctx.save_for_backward(x2, g, c, hprev, whh_f, whh_r, *w_ih)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        B, T, I = ctx.dims
        lstm = ctx.lstm
        need_x, need = ctx.needs_input_grad[0], list(ctx.needs_input_grad[2:])
        ps = _params(lstm)
        need = [n and p is not None for n, p in zip(need, ps)]
        if B == 0 or T == 0:
            dev = dy.device
            return (torch.zeros(B, T, I, dtype=torch.float32, device=dev) if need_x else None, None,
                    *(torch.zeros_like(p) if n else None for n, p in zip(need, ps)))
        x2, g, c, hprev, whh_f, whh_r = ctx.saved_tensors[:6]     # (raises if a saved weight was updated in place since the forward)
        lib = _capi.load_library()
        ptr = _capi.ptr
        dev = g.device
        rows, W = B * T, 8 * HIDDEN
        # the entry takes rows with a leading dimension, no batch stride: an expanded or strided dY (a loss's gradient is often an
        # expanded scalar) is copied to [B*T, 2 hd] here, a contiguous one is handed over as it lies
        dy2 = hostops.f32_rows(dy, (rows, 2 * HIDDEN))
        grads = [None] * 8
        with torch.cuda.device(dev):
            st = _capi.stream_of(dev)
            new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)   # noqa: E731
            dg = new(rows, W)
            _capi.check(lib.ggcn_bilstm_recurrence_backward(ptr(dy2), dy2.stride(0), ptr(g), W, ptr(c), ptr(whh_f), ptr(whh_r),
                                                            ptr(dg), W, B, T, HIDDEN, st), "ggcn_bilstm_recurrence_backward")

            def product(xcols, K, dh, ldh, F):        # dW [K,F] = dG[:, xcols:xcols+K]^T . dh
                return hostops.dweight(lib, st, dg[:, xcols:], W, dh, ldh, rows, K, F, "bf16x3")

            if need[0] or need[4]:                    # d[W_ih_f ; W_ih_r], already in nn.LSTM layout
                dwih = product(0, W, x2, x2.stride(0), I)
                if need[0] and need[4]:               # the two halves of one buffer: disjoint rows
                    grads[0], grads[4] = dwih[:W // 2], dwih[W // 2:]
                else:                                 # one half alone gets storage of its own, not a hold on the whole product
                    grads[0 if need[0] else 4] = (dwih[:W // 2] if need[0] else dwih[W // 2:]).clone()
            for d in (0, 1):
                if need[4 * d + 1]:                   # dW_hh_d = da_d^T . Hprev_d
                    grads[4 * d + 1] = product(d * 4 * HIDDEN, 4 * HIDDEN, hprev[:, d * HIDDEN:], 2 * HIDDEN, HIDDEN)
            if any(need[i] for i in (2, 3, 6, 7)):    # both biases of a direction receive the column sums of its da
                db = hostops.colsum(lib, st, dg, W, rows, W)
                for i in (2, 3, 6, 7):                # a copy each: b_ih.grad and b_hh.grad must not share memory (autograd
                    if need[i]:                       # accumulates and optimizers clip in place)
                        grads[i] = (db[:W // 2] if i < 4 else db[W // 2:]).clone()
            dx = None
            if need_x:                                # dX = dG . [W_ih_f ; W_ih_r]
                dx = hostops.linear_packed(lib, st, dg, W, _dx_operand(lstm, lib, st), rows, W, I).view(B, T, I)
        return (dx, None, *grads)


def bilstm_train(x, lstm):
    """``lstm(x)[0]`` as ``bilstm`` gives it, differentiable in ``x`` and in all eight parameters of the module.

    With grad enabled and ``x`` or a parameter requiring a gradient the call goes through ``_BilstmTrain``: the same bf16x3
    projection, ``ggcn_bilstm_recurrence_save`` in place on ``G`` (the same ``y`` bits; the activated gates, ``c`` and the ``h``
    each step read are kept: ``[B*T, 8 hd + 2 hd + 2 hd]`` floats), and a backward of one ``ggcn_bilstm_recurrence_backward``
    launch plus, each only where a gradient is wanted, three ``ggcn_dweight`` (``[W_ih_f ; W_ih_r]`` in one, the two ``W_hh``),
    one ``ggcn_colsum`` (the biases) and one ``ggcn_linear`` (``dX``, on a second cached image), all bf16x3 / fixed order.
    Without a gradient wanted it is ``bilstm`` and saves nothing.  The raises are ``bilstm``'s, without the one on gradients;
    ``B == 0`` or ``T == 0`` gives an empty result and zero gradients without a launch.  Every gradient has storage of its own
    (``bias_ih`` and ``bias_hh`` receive equal values in two buffers).  A ``dY`` that is not contiguous (an expanded scalar, a
    slice) is copied to ``[B*T, 2 hd]`` first: the backward entry takes a leading dimension, no batch stride; a time-sliced ``x``
    is copied likewise, as in ``bilstm``.  The classifier takes it in training
    with ``opt.ggcn_hip_lstm_backward`` / ``GGCN_HIP_LSTM_BACKWARD=1``."""
    _check(x, lstm, forward_only=False)
    if not lstm_wants_grad(x, lstm):
        return bilstm(x, lstm)
    return _BilstmTrain.apply(x, lstm, *_params(lstm))


# ---- the projection straight from BERT's layer list ------------------------------------------------------------

def layers_want_grad(layers, lstm):
    """A call on ``layers`` and ``lstm`` wants a gradient: grad is enabled and a layer or a parameter of the module requires one."""
    return torch.is_grad_enabled() and (any(x.requires_grad for x in layers)
                                        or any(p is not None and p.requires_grad for p in _params(lstm)))


def _check_layers_call(transform, layers, lstm):
    """The raises of ``bilstm_layers``: first those that need no device (the module, the layer list, the gradient), with
    ``bilstm``'s texts where they apply, then ``pooling._check_layers`` (CPU tensors, shapes, devices, the transform)."""
    problem = _module_problem(lstm)
    if problem is not None:
        raise RuntimeError(problem)
    if not isinstance(layers, (list, tuple)) or len(layers) == 0 or not all(
            isinstance(x, torch.Tensor) and x.dim() == 3 for x in layers):
        raise TypeError("layers must be a non-empty list or tuple of 3-d tensors")
    if len(layers) > pooling.MAX_LAYERS:
        raise RuntimeError("bilstm_layers takes at most %d layers in its one projection launch, got %d (pool them with "
                           "subword_pool_layers and call bilstm)" % (pooling.MAX_LAYERS, len(layers)))
    for i, x in enumerate(layers):
        if x.dtype != torch.float32:
            raise RuntimeError("layers[%d] must be float32, got %s (bf16 layers: subword_pool_layers, then nn.LSTM under "
                               "autocast)" % (i, x.dtype))
    width = sum(x.shape[2] for x in layers)
    if width != lstm.input_size:
        raise RuntimeError("layers of %d columns in all do not match lstm.input_size %d" % (width, lstm.input_size))
    if layers_want_grad(layers, lstm):
        raise RuntimeError("bilstm_layers is forward only: a gradient through the LSTM stays nn.LSTM (call it under torch.no_grad())")
    pooling._check_layers("bilstm_layers", transform, layers)
    dev = layers[0].device
    for name, p in zip(PARAMS, _params(lstm)):
        if p is not None and p.device != dev:
            raise RuntimeError("lstm.%s is on %s, layers on %s: the HIP path has no CPU fallback" % (name, p.device, dev))


def _pooled_args(transform, layers, real):
    """The argument list of ``ggcn_linear_pooled_layers(_form)`` up to ``wpack``, and what must stay alive during the call.
    ``real=False`` (the predicate): layers that do not share their strides are not copied; the form is asked about the
    contiguous copies ``bilstm_layers`` would make (the allocator's alignment, contiguous strides)."""
    B, R, C = transform.shape
    Dl = layers[0].shape[2]
    x0 = layers[0]
    if real:
        layers, x_batch, ldx = pooling._one_layout(list(layers))
        addrs = [x.data_ptr() for x in layers]
    elif x0.stride(2) != 1 or x0.stride(1) < Dl or any(x.stride() != x0.stride() for x in layers):
        x_batch, ldx, addrs = C * Dl, Dl, [256] * len(layers)
    else:
        x_batch, ldx, addrs = x0.stride(0), x0.stride(1), [x.data_ptr() for x in layers]
    ptrs = (ctypes.c_void_p * len(addrs))(*addrs)            # host array, read during the call
    sb, sr, sc = transform.stride()
    return (_capi.ptr(transform), sb, sr, sc, ptrs, len(addrs), x_batch, ldx), (B, R, C, Dl), layers


# Rows B*T from which on ``takes_hip_lstm_layers`` answers True by default: the smallest row count at which the one projection
# launch was measured not slower than ``subword_pool_layers`` + ``ggcn_linear`` (4096 x 32; it lost at 256 x 31 and 32 x 31, where the
# grid does not fill the chip twice and nothing hides the loader's latency: profiles/lstm_layers_timing.txt).
LAYERS_MIN_ROWS = 4096 * 32


def takes_hip_lstm_layers(transform, layers, lstm, min_rows=None):
    """``bilstm_layers(transform, layers, lstm)`` would run and is worth taking: the conditions of its raises, the answer of
    ``ggcn_linear_pooled_layers_form`` and the measured row-count floor (``min_rows``, None: ``LAYERS_MIN_ROWS``; 0 for the
    memory saving at any size -- ``bilstm_layers`` itself runs at every size) as a predicate.  No side effect (nothing is copied,
    packed or launched); False for CPU tensors, bf16 layers, more than 16 layers, a layer that requires grad and a wanted
    gradient."""
    try:
        if any(isinstance(x, torch.Tensor) and x.requires_grad for x in layers):
            return False
        _check_layers_call(transform, layers, lstm)
    except (TypeError, RuntimeError):
        return False
    B, R, C = transform.shape
    if B == 0 or R == 0 or C == 0:
        return True                                          # served without the launch
    if B * R < (LAYERS_MIN_ROWS if min_rows is None else min_rows):
        return False
    head, (B, R, C, Dl), _ = _pooled_args(transform, layers, real=False)
    F = 8 * HIDDEN
    fake = ctypes.c_void_p(256)                              # the form reads no device memory: an aligned stand-in for wpack and Y
    return _capi.load_library().ggcn_linear_pooled_layers_form(*head, fake, fake, F, B, R, C, Dl, F) > 0


def bilstm_layers(transform, layers, lstm):
    """``bilstm(subword_pool_layers(transform, layers), lstm)`` bit for bit, without the pooled words: ``[B,T,2*128]`` float32
    from ONE ``ggcn_linear_pooled_layers`` launch -- the bf16x3 projection on the module's cached image whose loader pools
    BERT's layers where they lie, so that neither ``[B,L,n*Dl]`` nor ``[B,T,n*Dl]`` exists -- and one ``ggcn_bilstm_recurrence``
    launch.  ``transform [B,T,L]`` float32 with any strides, ``layers``: 1..16 float32 tensors ``[B,L,Dl]`` of one shape and
    device with ``n*Dl == lstm.input_size``; layers that do not share their strides are made contiguous first.  Forward only: a
    wanted gradient raises, as do CPU tensors; the module's raises are ``bilstm``'s.  A layout the launch has no form for
    (``Dl % 32 != 0``, rows off 16 bytes) raises with the library's message, which names the composed pair;
    ``takes_hip_lstm_layers`` is the predicate.  ``B == 0`` or ``T == 0`` gives an empty tensor and ``L == 0`` the LSTM of zeros,
    without the projection launch."""
    _check_layers_call(transform, layers, lstm)
    B, T, C = transform.shape
    dev = layers[0].device
    F = 8 * HIDDEN
    y = torch.empty(B, T, 2 * HIDDEN, dtype=torch.float32, device=dev)
    if B == 0 or T == 0:
        return y
    lib = _capi.load_library()
    with torch.cuda.device(dev):
        st = _capi.stream_of(dev)
        pack, whh_f, whh_r, bias_f, bias_r = _operands(lstm, lib, st)
        if C == 0:
            g = torch.zeros(B * T, F, dtype=torch.float32, device=dev)       # the empty sums
        else:
            g = torch.empty(B * T, F, dtype=torch.float32, device=dev)
            head, (B, T, C, Dl), keep = _pooled_args(transform, [x.detach() for x in layers], real=True)
            _capi.check(lib.ggcn_linear_pooled_layers(*head, _capi.ptr(pack), _capi.ptr(g), F, B, T, C, Dl, F, st),
                        "ggcn_linear_pooled_layers")
            del keep
        _capi.check(lib.ggcn_bilstm_recurrence(_capi.ptr(g), F, _capi.ptr(whh_f), _capi.ptr(whh_r), _capi.ptr(bias_f),
                                               _capi.ptr(bias_r), _capi.ptr(y), 2 * HIDDEN, B, T, HIDDEN, st), "ggcn_bilstm_recurrence")
    return y
