"""The trainable BiLSTM on the GPU: ``ggcn_bilstm_recurrence_save`` and ``ggcn_bilstm_recurrence_backward`` at the C ABI against
the float64 statement (``bilstm_backward_ref``) with their bit-level promises, ``bilstm_train`` against float64 autograd of
``nn.LSTM(...).double()``, its launches, skipping and cache, and one training step of the three classifiers with the option on
against off.

The gate for every gradient is the project's gradient gate ``gates.close32(got, float64 ref, what, 2e-4)``.  It has room: float32
``nn.LSTM`` autograd on the CPU against float64, on these very modules and inputs, stays at 4e-7 .. 1.2e-6 of scale (the worst
case (33, 2, 9216)), two orders inside the gate; the bf16x3 projection's 1.4e-5 is the largest term expected.
Forward values (``Y``, the saved gates, ``C``, ``Hprev``) take the forward gate ``gates.gate(..., 1e-4)``; option on against off
takes the tree's on-against-off gate ``close32(..., 5e-4)``.  The worst ratio per quantity is printed when the module is done
(``-s``) and, with ``GGCN_GATES_REPORT=<file>``, written there (``profiles/bilstm_backward_gates.txt`` is such a file).
"""
import functools
import os
import types

import pytest
import torch

from oracle import gates
from oracle.gpu_support import classifier_batch, count_calls, dev, pkg  # noqa: F401

import bilstm_backward_ref as bb
import bilstm_ref as br

pytestmark = pytest.mark.gpu
PLAIN, SAVE, BACKWARD = "ggcn_bilstm_recurrence", "ggcn_bilstm_recurrence_save", "ggcn_bilstm_recurrence_backward"
PACK, LINEAR, DWEIGHT, COLSUM = "ggcn_weight_pack", "ggcn_linear", "ggcn_dweight", "ggcn_colsum"
ENTRIES = [PLAIN, SAVE, BACKWARD, PACK, LINEAR, DWEIGHT, COLSUM]
HD = br.HD
REL, ON_OFF = 2e-4, 5e-4
SHAPES = [(1, 1), (1, 2), (16, 3), (17, 5), (33, 2), (3, 33)]       # one tile short, full, one over, three tiles, a long sentence
ids = lambda s: "x".join(map(str, s))       # noqa: E731
WORST = {}


def _note(what, ratio):
    WORST[what] = max(WORST.get(what, 0.0), ratio)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    lines = ["%-28s worst error / gate %.4f" % (k, v) for k, v in sorted(WORST.items())]
    print("\n" + "\n".join(lines))
    if os.environ.get("GGCN_GATES_REPORT"):
        with open(os.environ["GGCN_GATES_REPORT"], "w") as f:
            f.write("\n".join(lines) + "\n")


def _close(got, ref, what, key, rel=REL):
    _note(key, gates.close32(got, ref, what, rel) / rel)


def _gate(got, ref, what, key):
    _note(key, gates.gate(got, ref, what, 1e-4))


# ================================================================ the C ABI
@functools.lru_cache(maxsize=None)
def _case(B, T, bias=True, bias_scale=1.0):
    """Seeded operands on the CPU, made once per case and never modified: a dict with ``G [B,T,8hd]``, the recurrent weights and
    biases, ``dY [B,T,2hd]`` (float32), the float64 statement of the saving forward, its ``gates`` and ``C`` rounded to float32
    (what the backward entry is handed) and the float64 ``dG`` of the statement on exactly those."""
    lstm = br.make_lstm(4, bias=bias, seed=B * 1000 + T, bias_scale=bias_scale)
    _, whh_f, whh_r, bias_f, bias_r = br.operands64(lstm)
    f32 = lambda t: None if t is None else t.float()   # noqa: E731
    c = dict(G=torch.randn(B, T, 8 * HD, generator=torch.Generator().manual_seed(7 * B + T)), whh_f=f32(whh_f), whh_r=f32(whh_r),
             bias_f=f32(bias_f), bias_r=f32(bias_r), dY=bb.make_dy(B, T, seed=B + T))
    c["Y"], c["gates"], c["C"], c["Hprev"] = bb.save64(c["G"], c["whh_f"], c["whh_r"], c["bias_f"], c["bias_r"])
    c["gates32"], c["C32"] = c["gates"].float(), c["C"].float()
    c["dG"] = bb.backward64(c["dY"], c["gates32"], c["C32"], c["whh_f"], c["whh_r"])
    return c


def _nan_all(t):
    return bool(torch.isnan(t).all())


def _forward(pkg, dev, c, save, in_place=False, pad_g=8, pad_y=8, guard=64):
    """One call of the plain or the saving entry on hostile buffers (NaN pad columns, a NaN row behind ``G``, NaN guard bands around
    every output); returns ``(Y, gates, C, Hprev)`` after checking that every NaN outside them is still there."""
    from ed_gated_gcn_amd import _capi
    G = c["G"]
    B, T, W = G.shape
    lib = pkg.load_library()
    gbuf = gates.hostile(G.reshape(B * T, W).to(dev), pad_g)
    ywhole, ybuf = gates.poisoned_rows(dev, B * T, 2 * HD + pad_y, guard)
    ops = [None if t is None else t.to(dev).contiguous() for t in (c["whh_f"], c["whh_r"], c["bias_f"], c["bias_r"])]
    head = (_capi.ptr(gbuf), gbuf.stride(0), *(_capi.ptr(t) for t in ops), _capi.ptr(ybuf), ybuf.stride(0), B, T, HD)
    saved = None
    if save:
        if in_place:
            gwhole, gout = gbuf, gbuf
        else:        # a buffer of its own with G's leading dimension
            gwhole, gout = gates.poisoned_rows(dev, B * T, W + pad_g, guard)
        cwhole, cbuf = gates.poisoned_rows(dev, B * T, 2 * HD, guard)
        hwhole, hbuf = gates.poisoned_rows(dev, B * T, 2 * HD, guard)
        _capi.check(lib.ggcn_bilstm_recurrence_save(*head, _capi.ptr(gout), _capi.ptr(cbuf), _capi.ptr(hbuf), _capi.stream_of(dev)), SAVE)
        torch.cuda.synchronize()
        for whole, what in ((cwhole, "C"), (hwhole, "Hprev")) + (() if in_place else ((gwhole, "gates"),)):
            assert _nan_all(whole[:guard]) and _nan_all(whole[-guard:]), "a guard band of %s was written" % what
        assert _nan_all(gout[:B * T, W:]), "the pad columns of gates were written"
        saved = (gout[:B * T, :W].reshape(B, T, W).clone(), cbuf.reshape(B, T, 2 * HD).clone(), hbuf.reshape(B, T, 2 * HD).clone())
    else:
        _capi.check(lib.ggcn_bilstm_recurrence(*head, _capi.stream_of(dev)), PLAIN)
        torch.cuda.synchronize()
    assert _nan_all(ybuf[:, 2 * HD:]), "Y's pad columns were written"
    assert _nan_all(ywhole[:guard]) and _nan_all(ywhole[-guard:]), "a guard band of Y was written"
    assert _nan_all(gbuf[:, W:]) and _nan_all(gbuf[-1]), "G's pads were written"
    if not (save and in_place):
        assert torch.equal(gbuf[:B * T, :W].cpu(), G.reshape(B * T, W)), "G was written"
    return (ybuf[:, :2 * HD].reshape(B, T, 2 * HD).clone(),) + (saved or (None, None, None))


@pytest.mark.parametrize("in_place", [False, True], ids=["own-buffer", "gates-is-G"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_save_keeps_the_plain_bits_and_saves_the_statement(pkg, dev, shape, in_place):
    c = _case(*shape)
    B, T = shape
    y_plain = _forward(pkg, dev, c, save=False)[0]
    y, g, cs, hp = _forward(pkg, dev, c, save=True, in_place=in_place)
    assert torch.equal(y, y_plain), "Y of the saving kernel differs from the plain kernel's"
    _gate(y, c["Y"], "Y %s" % ids(shape), "C ABI save: Y")
    _gate(g, c["gates"], "gates %s" % ids(shape), "C ABI save: gates")
    _gate(cs, c["C"], "C %s" % ids(shape), "C ABI save: C")
    _gate(hp, c["Hprev"], "Hprev %s" % ids(shape), "C ABI save: Hprev")
    assert float(hp[:, 0, :HD].abs().max()) == 0.0 and float(hp[:, T - 1, HD:].abs().max()) == 0.0, "Hprev of a first step is not zero"
    if T > 1:       # the h each later step read is the Y of the step before it, bit for bit
        assert torch.equal(hp[:, 1:, :HD], y[:, :-1, :HD]) and torch.equal(hp[:, :-1, HD:], y[:, 1:, HD:])


def test_save_without_bias(pkg, dev):
    c = _case(3, 5, False)
    assert c["bias_f"] is None and c["bias_r"] is None
    y, g, cs, hp = _forward(pkg, dev, c, save=True, in_place=True)
    assert torch.equal(y, _forward(pkg, dev, c, save=False)[0])
    _gate(g, c["gates"], "gates, bias=False", "C ABI save: gates")
    _gate(cs, c["C"], "C, bias=False", "C ABI save: C")


def _backward(pkg, dev, dY, g32, c32, whh_f, whh_r, pad=8, guard=64):
    """One call of the backward entry: ``dY`` and ``gates`` with NaN pad columns and a NaN row behind them, ``C`` with a NaN row
    behind it, ``dG`` between NaN guard bands with NaN pad columns; returns ``dG [B,T,8hd]`` after checking every NaN."""
    from ed_gated_gcn_amd import _capi
    B, T, W = g32.shape
    ybuf = gates.hostile(dY.reshape(B * T, 2 * HD).to(dev), pad)
    gbuf = gates.hostile(g32.reshape(B * T, W).to(dev), pad)
    cbuf = gates.hostile(c32.reshape(B * T, 2 * HD).to(dev), 0)
    whole, dbuf = gates.poisoned_rows(dev, B * T, W + pad, guard)
    wf, wr = whh_f.to(dev).contiguous(), whh_r.to(dev).contiguous()
    _capi.check(pkg.load_library().ggcn_bilstm_recurrence_backward(
        _capi.ptr(ybuf), ybuf.stride(0), _capi.ptr(gbuf), gbuf.stride(0), _capi.ptr(cbuf), _capi.ptr(wf), _capi.ptr(wr), _capi.ptr(dbuf),
        dbuf.stride(0), B, T, HD, _capi.stream_of(dev)), BACKWARD)
    torch.cuda.synchronize()
    assert _nan_all(dbuf[:, W:]), "dG's pad columns were written"
    assert _nan_all(whole[:guard]) and _nan_all(whole[-guard:]), "a guard band of dG was written"
    assert _nan_all(ybuf[:, 2 * HD:]) and _nan_all(ybuf[-1]) and _nan_all(gbuf[:, W:]) and _nan_all(gbuf[-1]) and _nan_all(cbuf[-1]), \
        "an input's pad was written"
    return dbuf[:, :W].reshape(B, T, W).clone()


def _backward_of(pkg, dev, c, **kw):
    a = dict(dY=c["dY"], g32=c["gates32"], c32=c["C32"], whh_f=c["whh_f"], whh_r=c["whh_r"])
    a.update(kw)
    return _backward(pkg, dev, a["dY"], a["g32"], a["c32"], a["whh_f"], a["whh_r"])


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_backward_within_the_gate(pkg, dev, shape):
    c = _case(*shape)
    dg = _backward_of(pkg, dev, c)
    assert not bool(torch.isnan(dg).any())
    _close(dg, c["dG"], "dG %s" % ids(shape), "C ABI backward: dG")
    for d in (0, 1):        # each direction against its own scale
        _close(dg[..., d * 4 * HD:(d + 1) * 4 * HD], c["dG"][..., d * 4 * HD:(d + 1) * 4 * HD], "dG %s d=%d" % (ids(shape), d),
               "C ABI backward: dG")


def test_backward_two_calls_give_the_same_bits(pkg, dev):
    c = _case(33, 2)
    assert torch.equal(_backward_of(pkg, dev, c), _backward_of(pkg, dev, c))
    c = _case(3, 33)
    assert torch.equal(_backward_of(pkg, dev, c), _backward_of(pkg, dev, c))


def test_backward_a_sentence_alone_equals_its_row_in_a_batch(pkg, dev):
    c = _case(17, 5)
    batch = _backward_of(pkg, dev, c)
    for b in (0, 1, 15, 16):                     # first and last place of a tile, the lone sentence of the last tile
        alone = _backward_of(pkg, dev, c, dY=c["dY"][b:b + 1], g32=c["gates32"][b:b + 1], c32=c["C32"][b:b + 1])
        assert torch.equal(alone[0], batch[b]), "sentence %d" % b


def _swap(t, half):
    return torch.cat([t[..., half:], t[..., :half]], dim=-1).flip(1)


def test_backward_flipped_time_and_swapped_directions(pkg, dev):
    c = _case(17, 5)
    dg = _backward_of(pkg, dev, c)
    dgs = _backward_of(pkg, dev, c, dY=_swap(c["dY"], HD), g32=_swap(c["gates32"], 4 * HD), c32=_swap(c["C32"], HD), whh_f=c["whh_r"],
                       whh_r=c["whh_f"])
    assert torch.equal(dgs, _swap(dg, 4 * HD))


def test_backward_saturated_gates_stay_finite(pkg, dev):
    c = _case(3, 5, True, 1e4)
    assert float(c["bias_f"].abs().max()) > 100.0
    sat = ((c["gates32"].abs() < 1e-6) | (c["gates32"].abs() > 1 - 1e-6)).double().mean()
    assert float(sat) > 0.5, "biases x 1e4 were meant to saturate the gates"
    _, g, cs, _ = _forward(pkg, dev, c, save=True, in_place=True)
    dg = _backward(pkg, dev, c["dY"], g.cpu(), cs.cpu(), c["whh_f"], c["whh_r"])      # on the kernel's own saved values
    assert bool(torch.isfinite(dg).all()), "NaN or inf under saturated gates"
    dg = _backward_of(pkg, dev, c)
    assert bool(torch.isfinite(dg).all())


@pytest.mark.parametrize("d", [0, 1], ids=["forward-zero", "reverse-zero"])
def test_backward_a_direction_without_gradient_gives_exact_zeros(pkg, dev, d):
    c = _case(17, 5)
    dY = c["dY"].clone()
    dY[..., d * HD:(d + 1) * HD] = 0.0
    dg = _backward_of(pkg, dev, c, dY=dY)
    assert float(dg[..., d * 4 * HD:(d + 1) * 4 * HD].abs().max()) == 0.0
    other = 1 - d
    assert torch.equal(dg[..., other * 4 * HD:(other + 1) * 4 * HD], _backward_of(pkg, dev, c)[..., other * 4 * HD:(other + 1) * 4 * HD])


# ================================================================ bilstm_train against float64 autograd
@functools.lru_cache(maxsize=None)
def _module_case(B, T, I, bias=True):
    lstm, x, dY = bb.make_case(B, T, I, bias)
    return lstm, x, dY, bb.autograd64(x, lstm, dY)


def _on(dev, lstm, requires_grad=True):
    """A fresh GPU copy of a cached CPU module (its cache attributes stay off the shared one)."""
    m = torch.nn.LSTM(lstm.input_size, lstm.hidden_size, bidirectional=True, batch_first=True, num_layers=1, bias=lstm.bias)
    m.load_state_dict(lstm.state_dict())
    return m.to(dev).requires_grad_(requires_grad)


def _hold(y, xgrad, m, dY, ref, what):
    _gate(y, ref["Y"], "Y " + what, "bilstm_train: Y")
    _close(xgrad, ref["dX"], "dX " + what, "bilstm_train: dX")
    names = [n for n, _ in m.named_parameters()]
    assert sorted(names) == sorted(k for k in ref if k not in ("Y", "dX"))
    for n, p in m.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, n
        _close(p.grad, ref[n], "d %s %s" % (n, what), "bilstm_train: d " + n.replace("_reverse", "").replace("_l0", ""))


@pytest.mark.parametrize("case", [(17, 5, 4), (3, 33, 4), (17, 5, 64), (3, 33, 64), (17, 5, 9216)], ids=ids)
def test_bilstm_train_against_float64_autograd(pkg, dev, case):
    lstm, x, dY, ref = _module_case(*case)
    m, xd = _on(dev, lstm), x.to(dev).requires_grad_(True)
    y = pkg.bilstm_train(xd, m)
    assert y.shape == (case[0], case[1], 2 * HD) and y.is_contiguous() and y.requires_grad
    y.backward(dY.to(dev))
    _hold(y.detach(), xd.grad, m, dY, ref, ids(case))
    with torch.no_grad():
        assert torch.equal(y.detach(), pkg.bilstm(xd, m)), "the saving forward's y differs from bilstm's"


def test_bilstm_train_without_bias(pkg, dev):
    lstm, x, dY, ref = _module_case(17, 5, 64, False)
    m, xd = _on(dev, lstm), x.to(dev).requires_grad_(True)
    assert len(list(m.parameters())) == 4
    y = pkg.bilstm_train(xd, m)
    y.backward(dY.to(dev))
    _hold(y.detach(), xd.grad, m, dY, ref, "17x5x64, bias=False")


def test_bilstm_train_on_a_time_sliced_view(pkg, dev):
    lstm, x, dY, ref = _module_case(3, 33, 64)
    longer = torch.cat([x, torch.full((3, 4, 64), float("nan"))], dim=1).to(dev).requires_grad_(True)
    view = longer[:, :33]
    assert not view.is_contiguous()
    m = _on(dev, lstm)
    y = pkg.bilstm_train(view, m)
    y.backward(dY.to(dev))
    assert float(longer.grad[:, 33:].abs().max()) == 0.0
    _hold(y.detach(), longer.grad[:, :33], m, dY, ref, "on x[:, :T]")


def test_one_step_has_no_recurrent_gradient(pkg, dev):
    lstm, x, dY, ref = _module_case(17, 1, 64)
    m, xd = _on(dev, lstm), x.to(dev).requires_grad_(True)
    y = pkg.bilstm_train(xd, m)
    y.backward(dY.to(dev))
    assert float(m.weight_hh_l0.grad.abs().max()) == 0.0 and float(m.weight_hh_l0_reverse.grad.abs().max()) == 0.0
    _hold(y.detach(), xd.grad, m, dY, ref, "17x1x64")


# ================================================================ launches, skipping, the cache
def _counts(calls):
    return tuple(calls[n] for n in (LINEAR, PLAIN, SAVE, BACKWARD, DWEIGHT, COLSUM))


def test_launches_with_every_gradient_wanted(pkg, dev, monkeypatch):
    lstm, x, dY, _ = _module_case(3, 33, 64)
    m, dYd = _on(dev, lstm), dY.to(dev)
    calls = count_calls(monkeypatch, ENTRIES, prec_arg={LINEAR: 10, DWEIGHT: 9})
    xd = x.to(dev).requires_grad_(True)
    y = pkg.bilstm_train(xd, m)
    assert _counts(calls) == (1, 0, 1, 0, 0, 0) and calls[PACK] == 1
    y.backward(dYd)
    assert _counts(calls) == (2, 0, 1, 1, 3, 1) and calls[PACK] == 2, "dX takes one further ggcn_linear on a second image"
    assert calls[LINEAR + "/bf16x3"] == 2 and calls[DWEIGHT + "/bf16x3"] == 3
    # x without a gradient, as in the classifier: no further linear, no second image
    m2 = _on(dev, lstm)
    for k in calls:
        calls[k] = 0
    pkg.bilstm_train(x.to(dev), m2).backward(dYd)
    assert _counts(calls) == (1, 0, 1, 1, 3, 1) and calls[PACK] == 1
    assert not hasattr(m2, "_ggcn_lstm_dx")


def test_frozen_recurrent_weights_skip_their_products(pkg, dev, monkeypatch):
    lstm, x, dY, ref = _module_case(3, 33, 64)
    m = _on(dev, lstm)
    m.weight_hh_l0.requires_grad_(False)
    m.weight_hh_l0_reverse.requires_grad_(False)
    calls = count_calls(monkeypatch, ENTRIES)
    pkg.bilstm_train(x.to(dev), m).backward(dY.to(dev))
    assert _counts(calls) == (1, 0, 1, 1, 1, 1)
    assert m.weight_hh_l0.grad is None and m.weight_hh_l0_reverse.grad is None
    _close(m.weight_ih_l0.grad, ref["weight_ih_l0"], "d weight_ih, W_hh frozen", "bilstm_train: d weight_ih")
    _close(m.bias_hh_l0_reverse.grad, ref["bias_hh_l0_reverse"], "d bias_hh_reverse, W_hh frozen", "bilstm_train: d bias_hh")
    # only x wants a gradient: the backward launch and the dX linear
    frozen = _on(dev, lstm, requires_grad=False)
    for k in calls:
        calls[k] = 0
    xd = x.to(dev).requires_grad_(True)
    pkg.bilstm_train(xd, frozen).backward(dY.to(dev))
    assert _counts(calls) == (2, 0, 1, 1, 0, 0)
    _close(xd.grad, ref["dX"], "dX, module frozen", "bilstm_train: dX")


def test_nothing_wanted_runs_the_plain_path(pkg, dev, monkeypatch):
    lstm, x, _, ref = _module_case(3, 33, 64)
    m, xd = _on(dev, lstm, requires_grad=False), x.to(dev)
    calls = count_calls(monkeypatch, ENTRIES)
    y = pkg.bilstm_train(xd, m)
    assert _counts(calls) == (1, 1, 0, 0, 0, 0) and not y.requires_grad
    trainable = _on(dev, lstm)
    with torch.no_grad():
        y2 = pkg.bilstm_train(xd.clone().requires_grad_(True), trainable)
    assert _counts(calls) == (2, 2, 0, 0, 0, 0) and not y2.requires_grad and torch.equal(y, y2)
    _gate(y, ref["Y"], "Y, nothing wanted", "bilstm_train: Y")


def test_retain_graph_gives_a_second_backward_with_the_same_bits(pkg, dev):
    lstm, x, dY, _ = _module_case(3, 33, 64)
    m, xd, dYd = _on(dev, lstm), x.to(dev).requires_grad_(True), dY.to(dev)
    y = pkg.bilstm_train(xd, m)
    y.backward(dYd, retain_graph=True)
    first = [xd.grad.clone()] + [p.grad.clone() for p in m.parameters()]
    xd.grad = None
    for p in m.parameters():
        p.grad = None
    y.backward(dYd)
    second = [xd.grad] + [p.grad for p in m.parameters()]
    assert len(first) == 9 and all(torch.equal(a, b) for a, b in zip(first, second))


def _extent(t):
    return t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()


def test_accumulated_gradients_are_twice_the_first_and_share_no_memory(pkg, dev):
    """Gradient accumulation: a second backward WITHOUT clearing adds into ``.grad`` in place, so two gradients in one storage
    (``bias_ih`` and ``bias_hh`` receive equal values) would count each other's share."""
    lstm, x, dY, _ = _module_case(3, 33, 64)
    m, xd, dYd = _on(dev, lstm), x.to(dev).requires_grad_(True), dY.to(dev)
    pkg.bilstm_train(xd, m).backward(dYd)
    first = [xd.grad.clone()] + [p.grad.clone() for p in m.parameters()]
    pkg.bilstm_train(xd, m).backward(dYd)
    second = [xd.grad] + [p.grad for p in m.parameters()]
    assert len(first) == 9
    for (n, _), a, b in zip([("x", None)] + list(m.named_parameters()), first, second):
        assert torch.equal(b, 2 * a), "d %s after two backwards is not twice the first" % n
    spans = sorted(_extent(g) for g in second)
    assert all(hi <= lo for (_, hi), (lo, _) in zip(spans, spans[1:])), "two gradients overlap in memory"
    assert torch.equal(m.bias_ih_l0.grad, m.bias_hh_l0.grad) and torch.equal(m.bias_ih_l0_reverse.grad, m.bias_hh_l0_reverse.grad)
    # an in-place edit of one bias gradient (a clip) leaves its twin alone
    before = m.bias_hh_l0.grad.clone()
    m.bias_ih_l0.grad.mul_(0.5)
    assert torch.equal(m.bias_hh_l0.grad, before)


def test_one_input_weight_alone_keeps_only_its_own_gradient_alive(pkg, dev):
    lstm, x, dY, ref = _module_case(3, 33, 64)
    m = _on(dev, lstm)
    m.weight_ih_l0.requires_grad_(False)
    pkg.bilstm_train(x.to(dev), m).backward(dY.to(dev))
    g = m.weight_ih_l0_reverse.grad
    assert m.weight_ih_l0.grad is None and g.untyped_storage().nbytes() == g.numel() * 4
    _close(g, ref["weight_ih_l0_reverse"], "d weight_ih_reverse alone", "bilstm_train: d weight_ih")


@pytest.mark.parametrize("name", ["weight_ih_l0", "weight_ih_l0_reverse", "weight_hh_l0", "weight_hh_l0_reverse"])
def test_a_weight_updated_between_forward_and_backward_is_an_error(pkg, dev, name):
    """dX and dh_rec are formed from the weights of the forward: autograd's version check on the saved tensors says so, as for
    ``nn.LSTM``."""
    lstm, x, dY, _ = _module_case(3, 33, 64)
    m, xd = _on(dev, lstm), x.to(dev).requires_grad_(True)
    y = pkg.bilstm_train(xd, m)
    with torch.no_grad():
        getattr(m, name).add_(0.05)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.backward(dY.to(dev))


def test_the_cache_is_rebuilt_after_an_optimizer_step(pkg, dev, monkeypatch):
    lstm, x, dY, _ = _module_case(3, 33, 64)
    m, dYd = _on(dev, lstm), dY.to(dev)
    sgd = torch.optim.SGD(m.parameters(), lr=0.05)
    calls = count_calls(monkeypatch, [PACK])

    def step():
        xd = x.to(dev).requires_grad_(True)
        y = pkg.bilstm_train(xd, m)
        y.backward(dYd)
        return y.detach(), xd.grad

    y1, dx1 = step()
    assert calls[PACK] == 2
    sgd.zero_grad()
    y2, dx2 = step()
    assert calls[PACK] == 2 and torch.equal(y1, y2) and torch.equal(dx1, dx2), "unchanged parameters pack nothing"
    sgd.step()
    y3, dx3 = step()
    assert calls[PACK] == 4, "an optimizer step repacks both images"
    cpu = _on(torch.device("cpu"), m)
    ref = bb.autograd64(x, cpu, dY)
    _gate(y3, ref["Y"], "Y after the step", "bilstm_train: Y")
    _close(dx3, ref["dX"], "dX after the step", "bilstm_train: dX")
    assert float((y3 - y1).abs().max()) > 1e-4, "the result follows the new weights"


def test_empty_inputs_make_no_launch(pkg, dev, monkeypatch):
    lstm, _, _, _ = _module_case(3, 33, 64)
    m = _on(dev, lstm)
    calls = count_calls(monkeypatch, ENTRIES)
    for shape in ((0, 5, 64), (3, 0, 64)):
        xd = torch.zeros(shape, device=dev, requires_grad=True)
        y = pkg.bilstm_train(xd, m)
        assert y.shape == (shape[0], shape[1], 2 * HD) and y.dtype == torch.float32 and y.requires_grad
        y.sum().backward()
        assert xd.grad.shape == shape
        for p in m.parameters():
            assert p.grad is not None and float(p.grad.abs().max()) == 0.0
    assert all(v == 0 for v in calls.values()), calls


# ================================================================ the three classifiers
class _Bert(torch.nn.Module):
    """Stands in for the encoder: twelve seeded [B,L,768] layers and a pooled vector."""

    def forward(self, ids_, seg, output_all_encoded_layers=True):
        gen = torch.Generator(device=ids_.device).manual_seed(1)
        return ([torch.randn(ids_.shape[0], ids_.shape[1], 768, device=ids_.device, generator=gen) for _ in range(12)],
                torch.zeros(ids_.shape[0], 768, device=ids_.device))


def _training_step(pkg, dev, cls_name, inputs, ncls, option):
    opt = types.SimpleNamespace(dropout=0.0, polarities_dim=ncls, device=dev, ggcn_hip_lstm_backward=option)
    m = getattr(pkg, cls_name)(_Bert(), opt)
    assert m.hip_lstm_backward is option and m.hip_lstm is False and m.gate_backward is False and m.head_backward is False
    gen = torch.Generator().manual_seed(0)
    for p in m.parameters():
        if p.dim() > 1:
            torch.nn.init.xavier_uniform_(p, generator=gen)
        else:
            torch.nn.init.uniform_(p, -0.05, 0.05, generator=gen)
    m = m.to(dev).train()
    torch.manual_seed(11)
    logits, xy, kl, scores = m(inputs)
    r = torch.randn(scores.shape, generator=torch.Generator().manual_seed(4)).to(dev)
    target = torch.arange(logits.shape[0], device=dev) % ncls
    loss = torch.nn.functional.cross_entropy(logits, target) + xy + kl + (scores * r).mean()
    loss.backward()
    grads = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
    return loss.detach(), grads, m


@pytest.mark.parametrize("cls_name", ["GatedGCNEventDetector", "GatedGCNEventDetector54", "GCNEventDetectorNoGate"])
def test_classifier_training_step_with_the_option(pkg, dev, cls_name, monkeypatch):
    for k in ("GGCN_HIP_LSTM_BACKWARD", "GGCN_HIP_LSTM", "GGCN_GATE_BACKWARD", "GGCN_HEAD_BACKWARD"):
        monkeypatch.delenv(k, raising=False)
    inputs, ncls = classifier_batch(dev)
    calls = count_calls(monkeypatch, [PLAIN, SAVE, BACKWARD])
    loss_off, g_off, _ = _training_step(pkg, dev, cls_name, inputs, ncls, False)
    assert (calls[PLAIN], calls[SAVE], calls[BACKWARD]) == (0, 0, 0), "the option is off: line :610 is nn.LSTM"
    loss_on, g_on, on = _training_step(pkg, dev, cls_name, inputs, ncls, True)
    assert (calls[PLAIN], calls[SAVE], calls[BACKWARD]) == (0, 1, 1)
    _close(loss_on, loss_off, "%s loss" % cls_name, "classifier on / off: loss", ON_OFF)
    assert sorted(g_on) == sorted(g_off) and sum(n.startswith("lstm.") for n in g_on) == 8
    for n in sorted(g_on):
        _close(g_on[n], g_off[n], "%s d %s" % (cls_name, n), "classifier on / off: d " + n.split(".")[0], ON_OFF)
    # inference and bf16 autocast keep the lines they ran before
    with torch.no_grad():
        on(inputs)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        res = on(inputs)                 # (train mode, a gradient wanted: only the autocast keeps nn.LSTM here)
    assert (calls[PLAIN], calls[SAVE], calls[BACKWARD]) == (0, 1, 1) and bool(torch.isfinite(res[0].float()).all())
