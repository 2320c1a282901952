"""float64 statement of the inference BiLSTM (``include/ggcn.h`` ``ggcn_bilstm_recurrence``; ``models/bert_amir5.py:557,610``) and the
seeded modules and inputs the two test files share (test infrastructure, NOT product code).

PyTorch's LSTM, gate order i, f, g, o, ``h0 = c0 = 0``; for direction d in {f, r} and sentence b, t runs 0..T-1 for f and T-1..0
for r::

    a = G[b, t, d*4hd:(d+1)*4hd] + bias_d + h . Whh_d^T
    i, f, o = sigmoid(a[0:hd]), sigmoid(a[hd:2hd]), sigmoid(a[3hd:4hd]);  g = tanh(a[2hd:3hd])
    c = f*c + i*g;  h = o * tanh(c);  Y[b, t, d*hd:(d+1)*hd] = h

``torch.nn.LSTM(...).double()`` on the CPU is the independent yardstick (``tests/test_bilstm_cpu.py`` holds the two together).
Parameters are set as ``train.py:75-84`` does: Xavier-uniform matrices, biases uniform +-1/sqrt(n); ``x ~ N(0,1)``.
"""
import math

import torch

HD = 128


def recurrence64(G, whh_f, whh_r, bias_f=None, bias_r=None):
    """The statement on ``G [B,T,8hd]`` (any float dtype; taken as float64): ``Y [B,T,2hd]`` float64."""
    G = G.double()
    B, T, W = G.shape
    hd = W // 8
    Y = torch.zeros(B, T, 2 * hd, dtype=torch.float64, device=G.device)
    for d, (whh, bias) in enumerate(((whh_f, bias_f), (whh_r, bias_r))):
        whh = whh.double()
        bias = torch.zeros(4 * hd, dtype=torch.float64, device=G.device) if bias is None else bias.double()
        h = torch.zeros(B, hd, dtype=torch.float64, device=G.device)
        c = torch.zeros_like(h)
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            a = G[:, t, d * 4 * hd:(d + 1) * 4 * hd] + bias + h @ whh.t()
            i, f, o = torch.sigmoid(a[:, :hd]), torch.sigmoid(a[:, hd:2 * hd]), torch.sigmoid(a[:, 3 * hd:])
            g = torch.tanh(a[:, 2 * hd:3 * hd])
            c = f * c + i * g
            h = o * torch.tanh(c)
            Y[:, t, d * hd:(d + 1) * hd] = h
    return Y


def operands64(lstm):
    """``(W_ih stacked [8hd, I], Whh_f, Whh_r, bias_f, bias_r)`` of an ``nn.LSTM`` in float64 (biases None without bias)."""
    p = {n: v.detach().double() for n, v in lstm.named_parameters()}
    wih = torch.cat([p["weight_ih_l0"], p["weight_ih_l0_reverse"]], dim=0)
    bias_f = p["bias_ih_l0"] + p["bias_hh_l0"] if "bias_ih_l0" in p else None
    bias_r = p["bias_ih_l0_reverse"] + p["bias_hh_l0_reverse"] if "bias_ih_l0" in p else None
    return wih, p["weight_hh_l0"], p["weight_hh_l0_reverse"], bias_f, bias_r


def bilstm_ref(x, lstm):
    """``lstm(x)[0]`` by the statement, in float64, on the module's float32 (or float64) parameters."""
    wih, whh_f, whh_r, bias_f, bias_r = operands64(lstm)
    return recurrence64(x.double() @ wih.t().to(x.device), whh_f.to(x.device), whh_r.to(x.device),
                        None if bias_f is None else bias_f.to(x.device), None if bias_r is None else bias_r.to(x.device))


def make_lstm(I, hd=HD, bias=True, seed=0, bias_scale=1.0):
    """A float32 CPU ``nn.LSTM(I, hd, bidirectional, batch_first)`` initialised as ``train.py:75-84``; ``bias_scale`` multiplies
    the biases (1e4: saturated gates)."""
    lstm = torch.nn.LSTM(I, hd, bidirectional=True, batch_first=True, num_layers=1, bias=bias)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in lstm.parameters():
            if p.dim() > 1:
                torch.nn.init.xavier_uniform_(p, generator=gen)
            else:
                bound = 1.0 / math.sqrt(p.shape[0])
                torch.nn.init.uniform_(p, -bound, bound, generator=gen)
                p.mul_(bias_scale)
    return lstm


def make_x(B, T, I, seed=0):
    return torch.randn(B, T, I, generator=torch.Generator().manual_seed(1000 + seed))


def lstm64(x, lstm):
    """The independent yardstick: a float64 copy of ``lstm`` on the CPU, run on ``x`` in float64."""
    ref = torch.nn.LSTM(lstm.input_size, lstm.hidden_size, bidirectional=True, batch_first=True, num_layers=1, bias=lstm.bias).double()
    ref.load_state_dict({k: v.detach().double().cpu() for k, v in lstm.state_dict().items()})
    with torch.no_grad():
        return ref(x.detach().double().cpu())[0]
