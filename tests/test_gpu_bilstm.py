"""The inference BiLSTM on the GPU: ``ggcn_bilstm_recurrence`` at the C ABI against the float64 statement (``bilstm_ref``), its
bit-level promises, saturated gates, ``bilstm`` against float64 ``nn.LSTM``, its launches and cache, and the classifier's opt-in.

The gate everywhere is the project's forward gate ``gates.gate(got, ref, what)`` (tol 1e-4 of max(1, max|ref|)); float32
``nn.LSTM`` itself sits at 1.2e-7 .. 1.5e-6 of float64 on these inputs, at 1.3e-7 with the biases x 1e4.  Parameters as
``train.py:75-84`` (``bilstm_ref.make_lstm``), ``x ~ N(0,1)``.
"""
import functools
import types

import pytest
import torch

from oracle import gates
from oracle.gpu_support import classifier_batch, count_calls, dev, pkg  # noqa: F401

import bilstm_ref as br

pytestmark = pytest.mark.gpu
ENTRY, PACK, LINEAR = "ggcn_bilstm_recurrence", "ggcn_weight_pack", "ggcn_linear"
HD = br.HD


def _tile():
    from ed_gated_gcn_amd import recurrent
    return recurrent.TILE


@functools.lru_cache(maxsize=None)
def _case(B, T, bias=True, bias_scale=1.0):
    """Seeded operands of the recurrence on the CPU, made once per case and never modified: ``(G [B,T,8hd], Whh_f, Whh_r,
    bias_f, bias_r, float64 reference Y)``."""
    lstm = br.make_lstm(4, bias=bias, seed=B * 1000 + T, bias_scale=bias_scale)
    _, whh_f, whh_r, bias_f, bias_r = br.operands64(lstm)
    f32 = lambda t: None if t is None else t.float()   # noqa: E731
    G = torch.randn(B, T, 8 * HD, generator=torch.Generator().manual_seed(7 * B + T))
    ops = (G, f32(whh_f), f32(whh_r), f32(bias_f), f32(bias_r))
    return ops + (br.recurrence64(*ops),)


def _recurrence(pkg, dev, G, whh_f, whh_r, bias_f, bias_r, pad_g=8, pad_y=8, guard=64):
    """One call of the entry on hostile buffers: ``G`` with NaN pad columns and a NaN row behind it, ``Y`` between NaN guard bands
    with NaN pad columns; returns ``Y [B,T,2hd]`` after checking that every NaN outside it is still there."""
    from ed_gated_gcn_amd import _capi
    B, T, W = G.shape
    gbuf = gates.hostile(G.reshape(B * T, W).to(dev), pad_g)
    whole, ybuf = gates.poisoned_rows(dev, B * T, 2 * HD + pad_y, guard)
    ops = [None if t is None else t.to(dev).contiguous() for t in (whh_f, whh_r, bias_f, bias_r)]
    _capi.check(pkg.load_library().ggcn_bilstm_recurrence(_capi.ptr(gbuf), gbuf.stride(0), *(_capi.ptr(t) for t in ops), _capi.ptr(ybuf),
                                                          ybuf.stride(0), B, T, HD, _capi.stream_of(dev)), ENTRY)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ybuf[:, 2 * HD:]).all()), "Y's pad columns were written"
    assert bool(torch.isnan(whole[:guard]).all()) and bool(torch.isnan(whole[-guard:]).all()), "a guard band of Y was written"
    assert bool(torch.isnan(gbuf[:, W:]).all()) and bool(torch.isnan(gbuf[-1]).all()), "G was written"
    return ybuf[:, :2 * HD].reshape(B, T, 2 * HD).clone()


def _shapes():
    S = _tile()
    return [(1, 1), (1, 2), (3, 5), (2, 100)] + [(B, T) for B in (S - 1, S, S + 1, 2 * S + 1) for T in (7, 33)]


# ---------------------------------------------------------------- 1. the recurrence against the statement
@pytest.mark.parametrize("shape", _shapes(), ids=lambda s: "x".join(map(str, s)))
def test_recurrence_within_the_gate(pkg, dev, shape):
    *ops, ref = _case(*shape)
    y = _recurrence(pkg, dev, *ops)
    gates.gate(y, ref, "Y %dx%d" % shape)


# ---------------------------------------------------------------- 2. bits
def test_two_calls_give_the_same_bits(pkg, dev):
    *ops, _ = _case(2 * _tile() + 1, 33)
    assert torch.equal(_recurrence(pkg, dev, *ops), _recurrence(pkg, dev, *ops))


def test_a_sentence_alone_equals_its_row_in_a_batch(pkg, dev):
    S = _tile()
    G, *rest, _ = _case(2 * S + 1, 7)
    batch = _recurrence(pkg, dev, G, *rest)
    for b in (0, 1, S - 1, S, 2 * S):                     # first and last place of a tile, the lone sentence of the last tile
        alone = _recurrence(pkg, dev, G[b:b + 1], *rest)
        assert torch.equal(alone[0], batch[b]), "sentence %d" % b


def test_flipped_time_and_swapped_directions(pkg, dev):
    G, whh_f, whh_r, bias_f, bias_r, _ = _case(_tile() + 1, 7)
    y = _recurrence(pkg, dev, G, whh_f, whh_r, bias_f, bias_r)
    Gs = torch.cat([G[..., 4 * HD:], G[..., :4 * HD]], dim=-1).flip(1)
    ys = _recurrence(pkg, dev, Gs, whh_r, whh_f, bias_r, bias_f)
    assert torch.equal(ys, torch.cat([y[..., HD:], y[..., :HD]], dim=-1).flip(1))


# ---------------------------------------------------------------- 3. saturation, no bias
def test_saturated_gates(pkg, dev):
    *ops, ref = _case(3, 5, True, 1e4)
    assert float(ops[3].abs().max()) > 100.0
    y = _recurrence(pkg, dev, *ops)
    assert not bool(torch.isnan(y).any())
    gates.gate(y, ref, "Y, biases x 1e4")


def test_without_bias_both_pointers_are_null(pkg, dev):
    *ops, ref = _case(3, 5, False)
    assert ops[3] is None and ops[4] is None
    gates.gate(_recurrence(pkg, dev, *ops), ref, "Y, bias=False")


# ---------------------------------------------------------------- 4. bilstm against float64 nn.LSTM
@functools.lru_cache(maxsize=None)
def _module_case(B, T, I, bias=True):
    lstm = br.make_lstm(I, bias=bias, seed=I + T).requires_grad_(False)
    x = br.make_x(B, T, I, seed=I + B)
    return lstm, x, br.lstm64(x, lstm)


def _on(dev, lstm):
    """A fresh GPU copy of a cached CPU module (its cache attribute stays off the shared one)."""
    m = torch.nn.LSTM(lstm.input_size, lstm.hidden_size, bidirectional=True, batch_first=True, num_layers=1, bias=lstm.bias)
    m.load_state_dict(lstm.state_dict())
    return m.to(dev).requires_grad_(False)


@pytest.mark.parametrize("I", [4, 64, 9216])
@pytest.mark.parametrize("BT", [(17, 5), (3, 33)], ids=lambda s: "x".join(map(str, s)))
def test_bilstm_against_float64_lstm(pkg, dev, BT, I):
    lstm, x, ref = _module_case(*BT, I)
    y = pkg.bilstm(x.to(dev), _on(dev, lstm))
    assert y.shape == (BT[0], BT[1], 2 * HD) and y.is_contiguous()
    gates.gate(y, ref, "bilstm %dx%dx%d" % (BT + (I,)))


def test_bilstm_on_a_time_sliced_view_and_without_bias(pkg, dev):
    lstm, x, ref = _module_case(3, 33, 64, False)
    longer = torch.cat([x, torch.full((3, 4, 64), float("nan"))], dim=1).to(dev)
    view = longer[:, :33]
    assert not view.is_contiguous()
    gates.gate(pkg.bilstm(view, _on(dev, lstm)), ref, "bilstm on x[:, :T]")


def test_bilstm_empty_input_makes_no_launch(pkg, dev, monkeypatch):
    lstm, _, _ = _module_case(3, 33, 64)
    m = _on(dev, lstm)
    calls = count_calls(monkeypatch, [ENTRY, PACK, LINEAR])
    for shape in ((0, 5, 64), (3, 0, 64)):
        y = pkg.bilstm(torch.zeros(shape, device=dev), m)
        assert y.shape == (shape[0], shape[1], 2 * HD) and y.dtype == torch.float32
    assert calls == {ENTRY: 0, PACK: 0, LINEAR: 0}


# ---------------------------------------------------------------- 5. launches and the cache
def test_launches_and_cache(pkg, dev, monkeypatch):
    lstm, x, ref = _module_case(3, 33, 64)
    m, xd = _on(dev, lstm), x.to(dev)
    calls = count_calls(monkeypatch, [ENTRY, PACK, LINEAR], prec_arg={LINEAR: 10})
    y1 = pkg.bilstm(xd, m)
    assert (calls[PACK], calls[LINEAR], calls[LINEAR + "/bf16x3"], calls[ENTRY]) == (1, 1, 1, 1)
    y2 = pkg.bilstm(xd, m)
    assert (calls[PACK], calls[LINEAR], calls[LINEAR + "/bf16x3"], calls[ENTRY]) == (1, 2, 2, 2), "the second call packs nothing"
    assert torch.equal(y1, y2)
    gates.gate(y1, ref, "before the update")
    # an optimizer's update: in place under no_grad, which moves the parameter's version counter (the cache key, as
    # heads._transposed's).  An edit through ``.data`` has a version counter of its own and is invisible to every such key.
    with torch.no_grad():
        m.weight_ih_l0.add_(0.05)
    y3 = pkg.bilstm(xd, m)
    assert (calls[PACK], calls[LINEAR], calls[ENTRY]) == (2, 3, 3), "an in-place weight update repacks"
    cpu = _on(torch.device("cpu"), m)
    gates.gate(y3, br.lstm64(x, cpu), "after the update")
    assert float((y3 - y1).abs().max()) > 1e-3, "the result follows the new weight"


# ---------------------------------------------------------------- 6. the classifier
class _Bert(torch.nn.Module):
    """Stands in for the encoder: twelve seeded [B,L,768] layers and a pooled vector."""

    def forward(self, ids_, seg, output_all_encoded_layers=True):
        gen = torch.Generator(device=ids_.device).manual_seed(1)
        return ([torch.randn(ids_.shape[0], ids_.shape[1], 768, device=ids_.device, generator=gen) for _ in range(12)],
                torch.zeros(ids_.shape[0], 768, device=ids_.device))


def _model(pkg, dev, cls_name, ncls, hip_lstm):
    opt = types.SimpleNamespace(dropout=0.0, polarities_dim=ncls, device=dev, ggcn_hip_lstm=hip_lstm)
    m = getattr(pkg, cls_name)(_Bert(), opt)
    assert m.hip_lstm is hip_lstm
    gen = torch.Generator().manual_seed(0)
    for p in m.parameters():
        if p.dim() > 1:
            torch.nn.init.xavier_uniform_(p, generator=gen)
        else:
            torch.nn.init.uniform_(p, -0.05, 0.05, generator=gen)
    return m.to(dev)


@pytest.mark.parametrize("cls_name", ["GatedGCNEventDetector", "GatedGCNEventDetector54", "GCNEventDetectorNoGate"])
def test_classifier_with_the_option(pkg, dev, cls_name, monkeypatch):
    monkeypatch.delenv("GGCN_HIP_LSTM", raising=False)
    inputs, ncls = classifier_batch(dev)
    calls = count_calls(monkeypatch, [ENTRY])
    off, on = _model(pkg, dev, cls_name, ncls, False).eval(), _model(pkg, dev, cls_name, ncls, True).eval()
    assert sorted(on.state_dict()) == sorted(off.state_dict())
    with torch.no_grad():
        ref = off(inputs)
        assert calls[ENTRY] == 0, "the option is off: line :610 is nn.LSTM"
        got = on(inputs)
    assert calls[ENTRY] == 1
    for g, r, what in zip(got, ref, ("logits", "xy", "kl", "scores")):
        g, r = (t if torch.is_tensor(t) else torch.tensor(float(t), device=dev) for t in (g, r))     # (the gateless variant: xy = 0.0)
        gates.gate(g, r, "%s %s" % (cls_name, what))
    # training with a gradient: nn.LSTM
    on.train()
    logits, xy, kl, scores = on(inputs)
    (logits.sum() + kl).backward()
    assert calls[ENTRY] == 1 and on.lstm.weight_hh_l0.grad is not None
    # bf16 autocast in inference: nn.LSTM, its float16 return handled as before
    on.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        res = on(inputs)
    assert calls[ENTRY] == 1 and bool(torch.isfinite(res[0].float()).all())
