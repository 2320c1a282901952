"""float64 statement of the BiLSTM's saving forward and one-launch backward (``include/ggcn.h`` ``ggcn_bilstm_recurrence_save``,
``ggcn_bilstm_recurrence_backward``; ``recurrent.bilstm_train``) and the float64 autograd yardstick, on the seeded modules and
inputs of ``bilstm_ref`` (test infrastructure, NOT product code).

Per sentence and direction, the direction's time walked backwards, with ``dh = dY[b,t,d] + dh_rec`` and a carried ``dc``::

    tc = tanh(c_t)    do = dh*tc         dc += dh*o*(1-tc^2)
    di = dc*g         dg = dc*i          df = dc*c_{t-1}          dc <- dc*f
    da = [ di*i(1-i) | df*f(1-f) | dg*(1-g^2) | do*o(1-o) ]  -> dG[b, t, d*4hd:(d+1)*4hd]        dh_rec = da . Whh_d

and from ``dG``: ``d[W_ih_f ; W_ih_r] = dG^T . x``, ``dW_hh_d = da_d^T . Hprev_d``, ``d bias_d`` = the column sums of ``da_d`` (for
``b_ih`` and ``b_hh`` alike), ``dX = dG . [W_ih_f ; W_ih_r]``.  ``tests/test_bilstm_backward_cpu.py`` holds the statement to
float64 autograd of ``nn.LSTM(...).double()``.
"""
import torch

import bilstm_ref as br

HD = br.HD
PARAMS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0",
          "weight_ih_l0_reverse", "weight_hh_l0_reverse", "bias_ih_l0_reverse", "bias_hh_l0_reverse")
SHAPES = [(1, 1, 4, True), (17, 5, 64, True), (3, 33, 64, True), (17, 5, 64, False)]     # (B, T, I, bias)


def _first(d, T):
    """The t of direction d's first step."""
    return 0 if d == 0 else T - 1


def _order(d, T):
    return range(T) if d == 0 else range(T - 1, -1, -1)


def save64(G, whh_f, whh_r, bias_f=None, bias_r=None):
    """The saving forward on ``G [B,T,8hd]``: float64 ``(Y [B,T,2hd], gates [B,T,8hd], C [B,T,2hd], Hprev [B,T,2hd])``."""
    G = G.double()
    B, T, W = G.shape
    hd = W // 8
    Y, C, Hp = (torch.zeros(B, T, 2 * hd, dtype=torch.float64) for _ in range(3))
    gates = torch.zeros(B, T, W, dtype=torch.float64)
    for d, (whh, bias) in enumerate(((whh_f, bias_f), (whh_r, bias_r))):
        whh = whh.double()
        bias = torch.zeros(4 * hd, dtype=torch.float64) if bias is None else bias.double()
        h = torch.zeros(B, hd, dtype=torch.float64)
        c = torch.zeros_like(h)
        for t in _order(d, T):
            a = G[:, t, d * 4 * hd:(d + 1) * 4 * hd] + bias + h @ whh.t()
            i, f, o = torch.sigmoid(a[:, :hd]), torch.sigmoid(a[:, hd:2 * hd]), torch.sigmoid(a[:, 3 * hd:])
            g = torch.tanh(a[:, 2 * hd:3 * hd])
            Hp[:, t, d * hd:(d + 1) * hd] = h
            c = f * c + i * g
            h = o * torch.tanh(c)
            gates[:, t, d * 4 * hd:(d + 1) * 4 * hd] = torch.cat([i, f, g, o], dim=1)
            C[:, t, d * hd:(d + 1) * hd] = c
            Y[:, t, d * hd:(d + 1) * hd] = h
    return Y, gates, C, Hp


def backward64(dY, gates, C, whh_f, whh_r):
    """The backward of the recurrence on ``dY [B,T,2hd]``, the saved ``gates [B,T,8hd]`` and ``C [B,T,2hd]``: float64
    ``dG [B,T,8hd]``."""
    dY, gates, C = dY.double(), gates.double(), C.double()
    B, T, W = gates.shape
    hd = W // 8
    dG = torch.zeros(B, T, W, dtype=torch.float64)
    for d, whh in enumerate((whh_f, whh_r)):
        whh = whh.double()
        dc = torch.zeros(B, hd, dtype=torch.float64)
        dh_rec = torch.zeros_like(dc)
        for t in reversed(list(_order(d, T))):
            i, f, g, o = (gates[:, t, d * 4 * hd + n * hd:d * 4 * hd + (n + 1) * hd] for n in range(4))
            c = C[:, t, d * hd:(d + 1) * hd]
            tp = t - 1 if d == 0 else t + 1
            c_prev = torch.zeros_like(c) if t == _first(d, T) else C[:, tp, d * hd:(d + 1) * hd]
            dh = dY[:, t, d * hd:(d + 1) * hd] + dh_rec
            tc = torch.tanh(c)
            do = dh * tc
            dc = dc + dh * o * (1 - tc * tc)
            di, dg, df = dc * g, dc * i, dc * c_prev
            dc = dc * f
            da = torch.cat([di * i * (1 - i), df * f * (1 - f), dg * (1 - g * g), do * o * (1 - o)], dim=1)
            dG[:, t, d * 4 * hd:(d + 1) * 4 * hd] = da
            dh_rec = da @ whh
    return dG


def statement64(x, lstm, dY):
    """Everything ``bilstm_train`` computes, by the statement, in float64 on the module's parameters: a dict with ``Y``,
    ``gates``, ``C``, ``Hprev``, ``dG``, ``dX`` and the eight gradients under their parameter names (absent biases: absent)."""
    wih, whh_f, whh_r, bias_f, bias_r = br.operands64(lstm)
    x = x.detach().double()
    B, T, I = x.shape
    Y, gates, C, Hp = save64(x @ wih.t(), whh_f, whh_r, bias_f, bias_r)
    dG = backward64(dY, gates, C, whh_f, whh_r)
    r = {"Y": Y, "gates": gates, "C": C, "Hprev": Hp, "dG": dG, "dX": dG @ wih}
    dwih = dG.reshape(B * T, 8 * HD).t() @ x.reshape(B * T, I)
    db = dG.sum((0, 1))
    for d, suffix in enumerate(("", "_reverse")):
        r["weight_ih_l0" + suffix] = dwih[d * 4 * HD:(d + 1) * 4 * HD]
        r["weight_hh_l0" + suffix] = (dG[..., d * 4 * HD:(d + 1) * 4 * HD].reshape(B * T, 4 * HD).t()
                                      @ Hp[..., d * HD:(d + 1) * HD].reshape(B * T, HD))
        if lstm.bias:
            r["bias_ih_l0" + suffix] = r["bias_hh_l0" + suffix] = db[d * 4 * HD:(d + 1) * 4 * HD]
    return r


def autograd64(x, lstm, dY):
    """The independent yardstick: float64 autograd through a float64 copy of ``lstm`` on the CPU; ``Y``, ``dX`` and the
    parameters' gradients under their names."""
    ref = torch.nn.LSTM(lstm.input_size, lstm.hidden_size, bidirectional=True, batch_first=True, num_layers=1, bias=lstm.bias).double()
    ref.load_state_dict({k: v.detach().double().cpu() for k, v in lstm.state_dict().items()})
    xd = x.detach().double().cpu().requires_grad_(True)
    y = ref(xd)[0]
    y.backward(dY.double().cpu())
    r = {"Y": y.detach(), "dX": xd.grad}
    r.update({n: p.grad for n, p in ref.named_parameters()})
    return r


def make_dy(B, T, seed=0):
    return torch.randn(B, T, 2 * HD, generator=torch.Generator().manual_seed(2000 + seed))


def make_case(B, T, I, bias=True):
    """``(lstm, x, dY)`` on the CPU in float32, seeded by the shape."""
    return br.make_lstm(I, bias=bias, seed=I + T), br.make_x(B, T, I, seed=I + B), make_dy(B, T, seed=B + T)
