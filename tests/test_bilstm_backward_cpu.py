"""Host side of the trainable BiLSTM (``ggcn_bilstm_recurrence_save``, ``ggcn_bilstm_recurrence_backward``,
``recurrent.bilstm_train``): the float64 statement of the backward against float64 autograd of ``nn.LSTM(...).double()``, the two
entries on all three sides of the ABI, their refusals with the exact ``ggcn_last_error`` text (every check comes before a launch:
the pointers handed in are never dereferenced, so no GPU is needed), the raises of ``bilstm_train``, the truth table of
``takes_hip_lstm_train`` and the classifier's opt-in ``hip_lstm_backward``."""
import ctypes
import re
import types

import numpy as np
import pytest
import torch

import ed_gated_gcn_amd as pkg
from ed_gated_gcn_amd import _capi, classifier, recurrent
from oracle.gpu_support import ace_batch
from oracle.host_support import header as _header, msg as _msg

import bilstm_backward_ref as bb

EINVAL, EUNSUPPORTED = 1, 3
SAVE, BACKWARD, PLAIN = "ggcn_bilstm_recurrence_save", "ggcn_bilstm_recurrence_backward", "ggcn_bilstm_recurrence"
P = ctypes.c_void_p(1 << 20)           # non-null, 16-byte aligned, never dereferenced
FAR = ctypes.c_void_p(1 << 30)         # another buffer, far from P
OFF = ctypes.c_void_p((1 << 20) + 4)


# ---------------------------------------------------------------- the statement
def _same(got, ref, what):
    """1e-11 relative to max|ref| (sums of up to 33 x 17 float64 products in two orders); where the reference is identically zero,
    below 1e-13 outright."""
    assert got.shape == ref.shape, "%s: %s vs %s" % (what, tuple(got.shape), tuple(ref.shape))
    scale = float(ref.abs().max())
    if scale < 1e-13:
        assert float(got.abs().max()) < 1e-13, "%s: %.3g where the reference is zero" % (what, float(got.abs().max()))
    else:
        err = float((got - ref).abs().max())
        assert err <= 1e-11 * scale, "%s: %.3g vs scale %.3g" % (what, err, scale)


@pytest.mark.parametrize("shape", bb.SHAPES, ids=lambda s: "x".join(map(str, s[:3])) + ("" if s[3] else "-nobias"))
def test_statement_equals_float64_autograd_of_the_lstm(shape):
    B, T, I, bias = shape
    lstm, x, dY = bb.make_case(B, T, I, bias)
    st, ref = bb.statement64(x, lstm, dY), bb.autograd64(x, lstm, dY)
    _same(st["Y"], ref["Y"], "Y")
    _same(st["dX"], ref["dX"], "dX")
    names = [n for n in bb.PARAMS if bias or not n.startswith("bias")]
    assert sorted(names) == sorted(k for k in ref if k not in ("Y", "dX"))
    for n in names:
        _same(st[n], ref[n], "d " + n)
    # what the saving forward keeps
    assert st["gates"].shape == st["dG"].shape == (B, T, 8 * bb.HD) and st["C"].shape == st["Hprev"].shape == (B, T, 2 * bb.HD)
    assert float(st["Hprev"][:, 0, :bb.HD].abs().max()) == 0.0 and float(st["Hprev"][:, T - 1, bb.HD:].abs().max()) == 0.0
    if T > 1:
        assert torch.equal(st["Hprev"][:, 1:, :bb.HD], st["Y"][:, :-1, :bb.HD])          # forward: the h of t - 1
        assert torch.equal(st["Hprev"][:, :-1, bb.HD:], st["Y"][:, 1:, bb.HD:])          # reverse: the h of t + 1


def test_t_equal_one_has_no_recurrent_gradient():
    lstm, x, dY = bb.make_case(3, 1, 4)
    st = bb.statement64(x, lstm, dY)
    assert float(st["weight_hh_l0"].abs().max()) == 0.0 and float(st["weight_hh_l0_reverse"].abs().max()) == 0.0
    assert float(st["weight_ih_l0"].abs().max()) > 0.0


# ---------------------------------------------------------------- the ABI
def test_declared_bound_exported_and_abi_unchanged():
    lib = ctypes.CDLL(pkg.lib_path())
    header = _header()
    for name in (SAVE, BACKWARD):
        assert "int %s(" % name in header and name in _capi.PROTOTYPES and hasattr(lib, name), name
        res, args = _capi.PROTOTYPES[name]
        assert res is _capi.c_i32 and ctypes.c_float not in args and ctypes.c_double not in args, name
        decl = header[header.index("int %s(" % name):]
        decl = decl[:decl.index(";")]
        assert "float " not in decl.replace("float *", ""), "%s takes a float by value" % name
        assert decl.count(",") + 1 == len(args), name
    assert _capi.ABI_VERSION == 14 and pkg.load_library().ggcn_abi_version() == 14
    vp, i64, i32 = _capi.c_vp, _capi.c_i64, _capi.c_i32
    plain = _capi.PROTOTYPES[PLAIN][1]
    assert _capi.PROTOTYPES[SAVE][1] == plain[:-1] + [vp, vp, vp] + plain[-1:]           # the plain entry's, then gates, C, Hprev, the stream
    assert _capi.PROTOTYPES[BACKWARD][1] == [vp, i64, vp, i64, vp, vp, vp, vp, i64, i32, i32, i32, vp]


def test_the_package_exports_the_two_functions():
    assert pkg.bilstm_train is recurrent.bilstm_train and pkg.takes_hip_lstm_train is recurrent.takes_hip_lstm_train
    assert "bilstm_train" in pkg.__all__ and "takes_hip_lstm_train" in pkg.__all__


# ---------------------------------------------------------------- the refusals
def _save(lib, entry=SAVE, **kw):
    a = dict(G=P, ldg=1024, wf=P, wr=P, bf=P, br=P, Y=P, ldy=256, B=3, T=5, hd=128, gates=P, C=P, Hprev=P)
    a.update(kw)
    args = [a[k] for k in ("G", "ldg", "wf", "wr", "bf", "br", "Y", "ldy", "B", "T", "hd")]
    if entry == SAVE:
        args += [a["gates"], a["C"], a["Hprev"]]
    return getattr(lib, entry)(*args, None)


LEADING = "leading dimension too small"
UNBUILT = "(the kernel is built for hd = 128, bert_amir5.py:551)"
ALIGNED = "Whh_f and Whh_r must be 16-byte aligned"
SHARED_REFUSALS = [
    (dict(G=None), EINVAL, "null pointer"), (dict(wf=None), EINVAL, "null pointer"), (dict(wr=None), EINVAL, "null pointer"),
    (dict(Y=None), EINVAL, "null pointer"),
    (dict(B=0), EINVAL, "B=0 T=5 must be positive"), (dict(B=-1), EINVAL, "B=-1 T=5 must be positive"),
    (dict(T=0), EINVAL, "B=3 T=0 must be positive"), (dict(T=-7), EINVAL, "B=3 T=-7 must be positive"),
    (dict(hd=64, ldg=512, ldy=128), EUNSUPPORTED, "hd=64 " + UNBUILT), (dict(hd=256, ldg=2048, ldy=512), EUNSUPPORTED, "hd=256 " + UNBUILT),
    (dict(hd=0), EUNSUPPORTED, "hd=0 " + UNBUILT),
    (dict(ldg=1023), EINVAL, LEADING), (dict(ldy=255), EINVAL, LEADING),
    (dict(B=1 << 16, T=1 << 15), EUNSUPPORTED, "B*T=2147483648 rows (at most 2^31 - 1)"),
    (dict(wf=OFF), EINVAL, ALIGNED), (dict(wr=OFF), EINVAL, ALIGNED),
    (dict(G=None, B=0, hd=5), EINVAL, "null pointer"),                      # the order of the checks: pointers first
    (dict(B=0, hd=5), EINVAL, "B=0 T=5 must be positive"),
]


@pytest.mark.parametrize("kw, code, text", SHARED_REFUSALS + [
    (dict(gates=None), EINVAL, "null pointer"), (dict(C=None), EINVAL, "null pointer"), (dict(Hprev=None), EINVAL, "null pointer"),
    (dict(Hprev=None, T=0), EINVAL, "null pointer"),
])
def test_save_refuses_before_it_launches(kw, code, text):
    lib = pkg.load_library()
    assert _msg(lib, _save(lib, **kw), code, SAVE) == "%s: %s" % (SAVE, text)


@pytest.mark.parametrize("kw, code, text", SHARED_REFUSALS)
def test_the_plain_entry_keeps_its_refusals(kw, code, text):
    lib = pkg.load_library()
    assert _msg(lib, _save(lib, entry=PLAIN, **kw), code, PLAIN) == "%s: %s" % (PLAIN, text)


def _backward(lib, **kw):
    a = dict(dY=P, lddy=256, gates=P, ldg=1024, C=P, wf=P, wr=P, dG=FAR, lddg=1024, B=3, T=5, hd=128)
    a.update(kw)
    return lib.ggcn_bilstm_recurrence_backward(*[a[k] for k in ("dY", "lddy", "gates", "ldg", "C", "wf", "wr", "dG", "lddg", "B", "T", "hd")],
                                               None)


ALIAS = "dG must not alias gates"
LAST = (3 * 5 - 1) * 1024 * 4 + 1024 * 4     # bytes from the first to behind the last element of a [15, 1024] buffer


@pytest.mark.parametrize("kw, code, text", [
    (dict(dY=None), EINVAL, "null pointer"), (dict(gates=None), EINVAL, "null pointer"), (dict(C=None), EINVAL, "null pointer"),
    (dict(wf=None), EINVAL, "null pointer"), (dict(wr=None), EINVAL, "null pointer"), (dict(dG=None), EINVAL, "null pointer"),
    (dict(B=0), EINVAL, "B=0 T=5 must be positive"), (dict(B=-1), EINVAL, "B=-1 T=5 must be positive"),
    (dict(T=0), EINVAL, "B=3 T=0 must be positive"), (dict(T=-7), EINVAL, "B=3 T=-7 must be positive"),
    (dict(hd=64, ldg=512, lddg=512, lddy=128), EUNSUPPORTED, "hd=64 " + UNBUILT), (dict(hd=0), EUNSUPPORTED, "hd=0 " + UNBUILT),
    (dict(lddy=255), EINVAL, LEADING), (dict(ldg=1023), EINVAL, LEADING), (dict(lddg=1023), EINVAL, LEADING),
    (dict(B=1 << 16, T=1 << 15), EUNSUPPORTED, "B*T=2147483648 rows (at most 2^31 - 1)"),
    (dict(wf=OFF), EINVAL, ALIGNED), (dict(wr=OFF), EINVAL, ALIGNED),
    (dict(dG=P), EINVAL, ALIAS),                                                              # the same buffer
    (dict(dG=ctypes.c_void_p((1 << 20) + LAST - 4)), EINVAL, ALIAS),                          # its first element on gates' last
    (dict(dG=ctypes.c_void_p((1 << 20) - LAST + 4)), EINVAL, ALIAS),                          # its last element on gates' first
    (dict(dG=None, B=0, hd=5), EINVAL, "null pointer"),                      # the order of the checks: pointers first
    (dict(dG=P, wf=OFF), EINVAL, ALIGNED),                                   # ... and the alias check last
])
def test_backward_refuses_before_it_launches(kw, code, text):
    lib = pkg.load_library()
    assert _msg(lib, _backward(lib, **kw), code, BACKWARD) == "%s: %s" % (BACKWARD, text)


# ---------------------------------------------------------------- bilstm_train's raises and the predicate
def _lstm(**kw):
    a = dict(input_size=8, hidden_size=128, bidirectional=True, batch_first=True, num_layers=1)
    a.update(kw)
    return torch.nn.LSTM(**a)


SHAPE = "lstm must be one bidirectional batch_first layer without projection, got num_layers=%d bidirectional=%s batch_first=%s proj_size=%d"
RAISES = [
    ("not a tensor", lambda: ([[1.0]], _lstm()), TypeError, "x must be a 3-d tensor"),
    ("2-d", lambda: (torch.zeros(3, 8), _lstm()), TypeError, "x must be a 3-d tensor"),
    ("float64 x", lambda: (torch.zeros(2, 3, 8, dtype=torch.float64), _lstm()), RuntimeError, "x must be float32, got torch.float64"),
    ("bf16 x", lambda: (torch.zeros(2, 3, 8, dtype=torch.bfloat16), _lstm()), RuntimeError, "x must be float32, got torch.bfloat16"),
    ("not an LSTM", lambda: (torch.zeros(2, 3, 8), torch.nn.GRU(8, 128)), RuntimeError, "lstm must be a torch.nn.LSTM, got GRU"),
    ("two layers", lambda: (torch.zeros(2, 3, 8), _lstm(num_layers=2)), RuntimeError, SHAPE % (2, True, True, 0)),
    ("one direction", lambda: (torch.zeros(2, 3, 8), _lstm(bidirectional=False)), RuntimeError, SHAPE % (1, False, True, 0)),
    ("time first", lambda: (torch.zeros(2, 3, 8), _lstm(batch_first=False)), RuntimeError, SHAPE % (1, True, False, 0)),
    ("projected", lambda: (torch.zeros(2, 3, 8), _lstm(proj_size=32)), RuntimeError, SHAPE % (1, True, True, 32)),
    ("hidden 64", lambda: (torch.zeros(2, 3, 8), _lstm(hidden_size=64)), RuntimeError, "lstm.hidden_size must be 128, got 64"),
    ("float64 module", lambda: (torch.zeros(2, 3, 8), _lstm().double()), RuntimeError, "lstm.weight_ih_l0 must be float32, got torch.float64"),
    ("width", lambda: (torch.zeros(2, 3, 9), _lstm()), RuntimeError, "x (2, 3, 9) does not match lstm.input_size 8"),
    ("cpu, training", lambda: (torch.zeros(2, 3, 8), _lstm()), RuntimeError, "x is on cpu: the HIP path has no CPU fallback"),
    ("cpu, x wants grad", lambda: (torch.zeros(2, 3, 8, requires_grad=True), _lstm().requires_grad_(False)), RuntimeError,
     "x is on cpu: the HIP path has no CPU fallback"),
    ("cpu, frozen", lambda: (torch.zeros(2, 3, 8), _lstm().requires_grad_(False)), RuntimeError, "x is on cpu: the HIP path has no CPU fallback"),
    ("cpu, empty", lambda: (torch.zeros(0, 3, 8), _lstm()), RuntimeError, "x is on cpu: the HIP path has no CPU fallback"),
]


@pytest.mark.parametrize("what, make, exc, text", RAISES, ids=[r[0] for r in RAISES])
def test_bilstm_train_raises(what, make, exc, text):
    x, lstm = make()
    with pytest.raises(exc, match=re.escape(text)):
        pkg.bilstm_train(x, lstm)
    assert pkg.takes_hip_lstm_train(x, lstm) is False


def test_bilstm_itself_stays_forward_only():
    with pytest.raises(RuntimeError, match="bilstm is forward only"):
        pkg.bilstm(torch.zeros(2, 3, 8), _lstm())


def _fake_gpu(t):
    """A stand-in for a GPU tensor: what the predicate asks of ``x`` and of a parameter, answered by ``t`` with ``is_cuda``."""
    class Fake(torch.Tensor):
        is_cuda = True
        device = torch.device("cuda:0")
    return t.as_subclass(Fake)


def _on_gpu(lstm):
    for n in recurrent.PARAMS:
        if getattr(lstm, n, None) is not None:
            lstm._parameters[n] = _fake_gpu(lstm._parameters[n])
    return lstm


def test_lstm_wants_grad_is_the_gradient_condition_of_both_predicates():
    x, frozen = torch.zeros(2, 3, 8), _lstm().requires_grad_(False)
    assert recurrent.lstm_wants_grad(x, _lstm()) is True and recurrent.lstm_wants_grad(x, frozen) is False
    assert recurrent.lstm_wants_grad(torch.zeros(2, 3, 8, requires_grad=True), frozen) is True
    with torch.no_grad():
        assert recurrent.lstm_wants_grad(torch.zeros(2, 3, 8, requires_grad=True), _lstm()) is False
    assert classifier.lstm_wants_grad is recurrent.lstm_wants_grad


def test_takes_hip_lstm_train_truth_table():
    x = _fake_gpu(torch.zeros(2, 3, 8))
    assert pkg.takes_hip_lstm_train(x, _on_gpu(_lstm())) is True                        # the parameters want a gradient
    assert pkg.takes_hip_lstm(x, _on_gpu(_lstm())) is False                             # ... which the inference predicate refuses
    assert pkg.takes_hip_lstm_train(x, _on_gpu(_lstm(bias=False))) is True
    assert pkg.takes_hip_lstm_train(x, _on_gpu(_lstm().requires_grad_(False))) is True  # no gradient wanted: bilstm_train is bilstm
    assert pkg.takes_hip_lstm_train(_fake_gpu(torch.zeros(2, 3, 8)).requires_grad_(True), _on_gpu(_lstm())) is True
    with torch.no_grad():
        assert pkg.takes_hip_lstm_train(x, _on_gpu(_lstm())) is True
    assert pkg.takes_hip_lstm_train(x, _lstm()) is False                                # the module is on another device
    assert pkg.takes_hip_lstm_train(torch.zeros(2, 3, 8), _on_gpu(_lstm())) is False    # x on the CPU
    assert pkg.takes_hip_lstm_train(_fake_gpu(torch.zeros(2, 3, 8, dtype=torch.bfloat16)), _on_gpu(_lstm())) is False
    assert pkg.takes_hip_lstm_train(_fake_gpu(torch.zeros(2, 3, 8, dtype=torch.float16)), _on_gpu(_lstm())) is False
    assert pkg.takes_hip_lstm_train(_fake_gpu(torch.zeros(3, 8)), _on_gpu(_lstm())) is False
    assert pkg.takes_hip_lstm_train(_fake_gpu(torch.zeros(2, 3, 9)), _on_gpu(_lstm())) is False
    for kw in (dict(num_layers=2), dict(bidirectional=False), dict(batch_first=False), dict(proj_size=32), dict(hidden_size=64)):
        assert pkg.takes_hip_lstm_train(x, _on_gpu(_lstm(**kw))) is False, kw
    assert pkg.takes_hip_lstm_train(x, torch.nn.GRU(8, 128)) is False and pkg.takes_hip_lstm_train(None, _lstm()) is False
    m = _on_gpu(_lstm())
    pkg.takes_hip_lstm_train(x, m)
    assert not hasattr(m, "_ggcn_lstm") and not hasattr(m, "_ggcn_lstm_dx"), "the predicate has no side effect"


# ---------------------------------------------------------------- the classifier's option
CLASSIFIERS = ["GatedGCNEventDetector", "GatedGCNEventDetector54", "GCNEventDetectorNoGate"]
ENV = ("GGCN_HIP_LSTM_BACKWARD", "GGCN_HIP_LSTM", "GGCN_GATE_BACKWARD", "GGCN_HEAD_BACKWARD")


class _Bert(torch.nn.Module):
    """Stands in for the encoder: twelve seeded [B,L,768] layers and a pooled vector."""

    def forward(self, ids_, seg, output_all_encoded_layers=True):
        gen = torch.Generator().manual_seed(1)
        return ([torch.randn(ids_.shape[0], ids_.shape[1], 768, generator=gen) for _ in range(12)], torch.zeros(ids_.shape[0], 768))


def _classifier(cls, **opt):
    return cls(_Bert(), types.SimpleNamespace(dropout=0.0, polarities_dim=5, **opt))


@pytest.mark.parametrize("cls_name", CLASSIFIERS)
def test_option_is_off_by_default_and_read_from_opt_and_environment(monkeypatch, cls_name):
    cls = getattr(pkg, cls_name)
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    assert _classifier(cls).hip_lstm_backward is False
    assert _classifier(cls, ggcn_hip_lstm_backward=True).hip_lstm_backward is True
    assert _classifier(cls, ggcn_hip_lstm_backward=False).hip_lstm_backward is False
    on = _classifier(cls, ggcn_hip_lstm_backward=True)
    assert on.hip_lstm is False and on.gate_backward is False and on.head_backward is False, "the options are independent"
    assert _classifier(cls, ggcn_hip_lstm=True, ggcn_gate_backward=True, ggcn_head_backward=True).hip_lstm_backward is False
    monkeypatch.setenv("GGCN_HIP_LSTM_BACKWARD", "1")
    assert _classifier(cls).hip_lstm_backward is True and _classifier(cls).hip_lstm is False
    monkeypatch.setenv("GGCN_HIP_LSTM_BACKWARD", "0")
    assert _classifier(cls).hip_lstm_backward is False
    assert sorted(on.state_dict()) == sorted(_classifier(cls).state_dict()), "the option adds nothing to the state_dict"


class _Reached(Exception):
    """``bilstm_train`` was called at line :610."""


class _Kept(Exception):
    """``nn.LSTM`` was called at line :610."""


def _line_610(model, inputs):
    """Which of the two runs at :610 (the forward is cut short there: what follows has no CPU path)."""
    try:
        model(inputs)
    except _Reached:
        return "bilstm_train"
    except _Kept:
        return "nn.LSTM"
    raise AssertionError("the forward passed line :610 without either")


@pytest.mark.parametrize("cls_name", CLASSIFIERS)
def test_option_reaches_bilstm_train_only_in_training_on_float32_without_autocast(monkeypatch, cls_name):
    cls = getattr(pkg, cls_name)
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    inputs = ace_batch(np.random.default_rng(3), 4, 9, 20, vocab=100)
    seen = []

    def train_stub(x, lstm):
        seen.append((tuple(x.shape), x.dtype, lstm))
        raise _Reached()

    def kept(module, args):
        raise _Kept()

    monkeypatch.setattr(classifier, "subword_pool", lambda tr, x: torch.bmm(tr, x))     # (:600 has no CPU path either)
    monkeypatch.setattr(classifier, "bilstm_train", train_stub)
    on, off = _classifier(cls, ggcn_hip_lstm_backward=True), _classifier(cls)
    both = _classifier(cls, ggcn_hip_lstm_backward=True, ggcn_hip_lstm=True)
    for m in (on, off, both):
        m.lstm.register_forward_pre_hook(kept)
    # CPU tensors: the real predicate is False, so the option changes nothing
    assert _line_610(on, inputs) == "nn.LSTM" and _line_610(off, inputs) == "nn.LSTM" and not seen
    # from here on the predicate answers as it would for float32 GPU tensors
    monkeypatch.setattr(classifier, "takes_hip_lstm_train", lambda x, lstm: True)
    assert _line_610(off, inputs) == "nn.LSTM" and not seen, "the option is off"
    assert _line_610(on, inputs) == "bilstm_train" and len(seen) == 1
    assert seen[0][0][2] == 12 * 768 and seen[0][1] == torch.float32 and seen[0][2] is on.lstm
    assert _line_610(both, inputs) == "bilstm_train", "independent of ggcn_hip_lstm"
    with torch.no_grad():
        assert _line_610(on, inputs) == "nn.LSTM", "no gradient wanted"
    on.lstm.requires_grad_(False)
    assert _line_610(on, inputs) == "nn.LSTM", "a frozen LSTM on features without a gradient wants none"
    on.lstm.requires_grad_(True)
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)
    assert _line_610(on, inputs) == "nn.LSTM", "autocast keeps nn.LSTM"
    monkeypatch.undo()
