"""Host side of the BiLSTM projection on BERT's layer list (``ggcn_linear_pooled_layers``, ``ggcn_linear_pooled_layers_form``,
``recurrent.bilstm_layers``, ``recurrent.takes_hip_lstm_layers``, the classifier's ``lstm_layers``): the two entries on all three
sides of the ABI, every refusal with its status and exact ``ggcn_last_error`` text (every check comes before a launch: the
pointers handed in are never dereferenced, so no GPU is needed), the raises of ``bilstm_layers`` that need no device, the
predicate, the classifier's option and its choice of path with the entry points replaced, and a numpy statement of the launch
against float64."""
import ctypes
import re
import types

import numpy as np
import pytest
import torch

import ed_gated_gcn_amd as pkg
import linear_ref as lr
from ed_gated_gcn_amd import _capi, classifier, pooling, recurrent
from oracle.gpu_support import ace_batch
from oracle.host_support import header as _header, msg as _msg

EINVAL, EUNSUPPORTED = 1, 3
ENTRY, FORM = "ggcn_linear_pooled_layers", "ggcn_linear_pooled_layers_form"
A, X, W, Y = 1 << 20, 1 << 24, 1 << 27, 1 << 28   # fake addresses, 512-byte aligned like a fresh device allocation; never dereferenced
NAMES = ("A", "sa_b", "sa_r", "sa_c", "layers", "n_layers", "x_batch", "ldx", "wpack", "Y", "ldy", "B", "R", "C", "Dl", "F")


def _args(**kw):
    """The argument list of ``..._form`` (the entry's without the stream) for 12 layers [2, 9, 768] into Y [6, 1024]; ``ptrs``
    overrides the layers' addresses (None: a NULL entry), every other keyword the argument of that name."""
    n = kw.get("n_layers", 12)
    a = dict(A=A, sa_b=27, sa_r=9, sa_c=1, n_layers=n, x_batch=9 * 768, ldx=768, wpack=W, Y=Y, ldy=1024, B=2, R=3, C=9, Dl=768, F=1024)
    ptrs = kw.pop("ptrs", None)
    a.update(kw)
    if ptrs is None:
        ptrs = [X + l * a["B"] * a["x_batch"] * 4 for l in range(min(max(n, 0), 64))]
    a.setdefault("layers", (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs))
    return [None if a[k] is None else (ctypes.c_void_p(a[k]) if k in ("A", "Y", "wpack") else a[k]) for k in NAMES]


# ---------------------------------------------------------------- the ABI
def test_declared_bound_exported_and_abi_unchanged():
    lib = ctypes.CDLL(pkg.lib_path())
    header = _header()
    for name in (ENTRY, FORM):
        assert "int %s(" % name in header and name in _capi.PROTOTYPES and hasattr(lib, name), name
        res, args = _capi.PROTOTYPES[name]
        decl = header[header.index("int %s(" % name):]
        decl = decl[:decl.index(";")]
        assert res is _capi.c_i32 and decl.count(",") + 1 == len(args), name
    vp, i64, i32 = _capi.c_vp, _capi.c_i64, _capi.c_i32
    form = [vp, i64, i64, i64, vp, i32, i64, i64, vp, vp, i64, i32, i32, i32, i32, i32]
    assert _capi.PROTOTYPES[FORM][1] == form and _capi.PROTOTYPES[ENTRY][1] == form + [vp]      # ... and the stream
    assert "#define GGCN_ABI_VERSION 14" in header
    assert _capi.ABI_VERSION == 14 and pkg.load_library().ggcn_abi_version() == 14


def test_the_package_exports_the_functions():
    for name in ("bilstm_layers", "takes_hip_lstm_layers"):
        assert getattr(pkg, name) is getattr(recurrent, name) and name in pkg.__all__
        assert getattr(classifier, name) is getattr(recurrent, name)


# ---------------------------------------------------------------- the refusals
NULL = "null pointer"
LEADING = "leading dimension too small"
LAYOUT = ("needs Dl % 32 == 0, ldx, x_batch, F and ldy multiples of 4 and 16-byte aligned layers and Y "
          "(use ggcn_subword_pool_layers, then ggcn_linear with GGCN_PREC_BF16X3)")
POSITIVE = "B=%d R=%d C=%d Dl=%d F=%d must be positive"
REFUSALS = [
    (dict(A=None), EINVAL, NULL), (dict(layers=None), EINVAL, NULL), (dict(wpack=None), EINVAL, NULL), (dict(Y=None), EINVAL, NULL),
    (dict(ptrs=[X] * 5 + [None] + [X] * 6), EINVAL, "layers[5] is a null pointer"),
    (dict(n_layers=0), EINVAL, "n_layers=0 must be positive"), (dict(n_layers=-3), EINVAL, "n_layers=-3 must be positive"),
    (dict(B=0), EINVAL, POSITIVE % (0, 3, 9, 768, 1024)), (dict(R=-1), EINVAL, POSITIVE % (2, -1, 9, 768, 1024)),
    (dict(C=0), EINVAL, POSITIVE % (2, 3, 0, 768, 1024)), (dict(Dl=0), EINVAL, POSITIVE % (2, 3, 9, 0, 1024)),
    (dict(F=0), EINVAL, POSITIVE % (2, 3, 9, 768, 0)),
    (dict(n_layers=17), EUNSUPPORTED, "n_layers=17 > 16 layers a launch"),
    (dict(C=2049), EUNSUPPORTED, "C=2049 > 2048 columns"),
    (dict(B=1 << 16, R=1 << 15), EUNSUPPORTED, "too many rows"),
    (dict(ldx=767), EINVAL, LEADING), (dict(ldy=1023), EINVAL, LEADING),
    (dict(A=A + 2), EINVAL, "A or Y not aligned to its element"), (dict(Y=Y + 2), EINVAL, "A or Y not aligned to its element"),
    (dict(ptrs=[X] * 11 + [X + 2]), EINVAL, "layers[11] not aligned to its element"),
    (dict(wpack=W + 8), EINVAL, "wpack must be 16-byte aligned"),
    (dict(n_layers=16, Dl=65536, ldx=65536), EUNSUPPORTED, "K=n_layers*Dl=1048576 too large for ggcn_weight_pack"),
    # the layouts the kernel has no form for: the message names the composed pair
    (dict(Dl=16, n_layers=2), EUNSUPPORTED, LAYOUT), (dict(Dl=760), EUNSUPPORTED, LAYOUT),
    (dict(ldx=770), EUNSUPPORTED, LAYOUT), (dict(x_batch=9 * 768 + 2), EUNSUPPORTED, LAYOUT),
    (dict(F=1022), EUNSUPPORTED, LAYOUT), (dict(ldy=1026), EUNSUPPORTED, LAYOUT),
    (dict(Y=Y + 4), EUNSUPPORTED, LAYOUT), (dict(ptrs=[X] * 3 + [X + 8] + [X] * 8), EUNSUPPORTED, LAYOUT),
    # the order of the checks: pointers, the number of layers (its cap before any layers[l] is read), the layers, the sizes
    (dict(A=None, n_layers=0, B=0), EINVAL, NULL),
    (dict(n_layers=0, B=0), EINVAL, "n_layers=0 must be positive"),
    (dict(n_layers=17, ptrs=[None] * 17, B=0), EUNSUPPORTED, "n_layers=17 > 16 layers a launch"),
    (dict(ptrs=[None] * 12, B=0), EINVAL, "layers[0] is a null pointer"),
    (dict(B=0, C=4096), EINVAL, POSITIVE % (0, 3, 4096, 768, 1024)),
]


@pytest.mark.parametrize("kw, code, text", REFUSALS)
def test_entry_refuses_before_it_launches_and_form_negates_the_status(kw, code, text):
    lib = pkg.load_library()
    assert _msg(lib, lib.ggcn_linear_pooled_layers(*_args(**kw), None), code, ENTRY) == "%s: %s" % (ENTRY, text)
    assert lib.ggcn_linear_pooled_layers_form(*_args(**kw)) == -code
    assert lib.ggcn_last_error().decode() == "%s: %s" % (ENTRY, text)


def test_form_takes_what_the_kernel_has_a_form_for():
    form = lambda **kw: pkg.load_library().ggcn_linear_pooled_layers_form(*_args(**kw))   # noqa: E731
    assert form() == 1 and form(n_layers=1) == 1 and form(n_layers=16) == 1
    assert form(Dl=32, n_layers=3) == 1 and form(Dl=64) == 1 and form(Dl=96) == 1
    assert form(ldx=772) == 1 and form(x_batch=9 * 768 + 4) == 1 and form(ldy=1028) == 1 and form(F=260, ldy=260) == 1
    assert form(Y=Y + 16) == 1 and form(ptrs=[X + 16 * l for l in range(12)]) == 1
    assert form(n_layers=16, Dl=65504, ldx=65504) == 1            # 65504 k-steps: the most ggcn_weight_pack takes is 65535
    assert form(C=2048) == 1 and form(sa_b=1, sa_r=3, sa_c=7) == 1   # the strides of A play no part


# ---------------------------------------------------------------- bilstm_layers' raises and the predicate
class _Fake0(torch.Tensor):
    """A stand-in for a GPU tensor: what the checks ask of a tensor, answered by a CPU tensor with ``is_cuda``."""
    is_cuda = True
    device = torch.device("cuda:0")


def _g(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).as_subclass(_Fake0)


def _lstm(input_size=24, **kw):
    kw = dict(dict(hidden_size=128, bidirectional=True, batch_first=True, num_layers=1), **kw)
    m = torch.nn.LSTM(input_size, **kw)
    for p in m.parameters():
        p.requires_grad_(False)
    return m


def _trainable(m):
    for p in m.parameters():
        p.requires_grad_(True)
    return m


L3 = lambda: [_g(2, 5, 8) for _ in range(3)]   # noqa: E731
RAISES = [
    ("not an LSTM", lambda: (_g(2, 3, 5), L3(), torch.nn.GRU(24, 128)), RuntimeError, "lstm must be a torch.nn.LSTM, got GRU"),
    ("hidden size", lambda: (_g(2, 3, 5), L3(), _lstm(hidden_size=64)), RuntimeError, "lstm.hidden_size must be 128, got 64"),
    ("one direction", lambda: (_g(2, 3, 5), L3(), _lstm(bidirectional=False)), RuntimeError,
     "lstm must be one bidirectional batch_first layer without projection"),
    ("a tensor, not a list", lambda: (_g(2, 3, 5), _g(2, 5, 24), _lstm()), TypeError,
     "layers must be a non-empty list or tuple of 3-d tensors"),
    ("empty list", lambda: (_g(2, 3, 5), [], _lstm()), TypeError, "layers must be a non-empty list or tuple of 3-d tensors"),
    ("2-d layer", lambda: (_g(2, 3, 5), [_g(5, 24)], _lstm()), TypeError, "layers must be a non-empty list or tuple of 3-d tensors"),
    ("seventeen layers", lambda: (_g(2, 3, 5), [_g(2, 5, 8) for _ in range(17)], _lstm(136)), RuntimeError,
     "bilstm_layers takes at most 16 layers in its one projection launch, got 17"),
    ("bf16 layers", lambda: (_g(2, 3, 5), [_g(2, 5, 8, dtype=torch.bfloat16) for _ in range(3)], _lstm()), RuntimeError,
     "layers[0] must be float32, got torch.bfloat16"),
    ("width", lambda: (_g(2, 3, 5), L3(), _lstm(32)), RuntimeError, "layers of 24 columns in all do not match lstm.input_size 32"),
    ("a parameter wants a gradient", lambda: (_g(2, 3, 5), L3(), _trainable(_lstm())), RuntimeError,
     "bilstm_layers is forward only: a gradient through the LSTM stays nn.LSTM (call it under torch.no_grad())"),
    ("a layer wants a gradient", lambda: (_g(2, 3, 5), [_g(2, 5, 8).requires_grad_(True)] + L3()[:2], _lstm()), RuntimeError,
     "bilstm_layers is forward only"),
    ("cpu tensors", lambda: (torch.zeros(2, 3, 5), [torch.zeros(2, 5, 8)] * 3, _lstm()), RuntimeError,
     "transform is on cpu: the HIP path has no CPU fallback"),
    ("a cpu layer", lambda: (_g(2, 3, 5), [_g(2, 5, 8), torch.zeros(2, 5, 8), _g(2, 5, 8)], _lstm()), RuntimeError,
     "layers[1] is on cpu: the HIP path has no CPU fallback"),
    ("mixed shapes", lambda: (_g(2, 3, 5), [_g(2, 5, 8), _g(2, 5, 4), _g(2, 5, 12)], _lstm()), RuntimeError,
     "layers[1] (2, 5, 4) torch.float32 does not match layers[0] (2, 5, 8) torch.float32"),
    ("transform does not match", lambda: (_g(2, 3, 6), L3(), _lstm()), RuntimeError, "transform (2, 3, 6) does not match layers (2, 5, 8)"),
    ("transform wants a gradient", lambda: (_g(2, 3, 5).requires_grad_(True), L3(), _lstm()), RuntimeError,
     "bilstm_layers does not differentiate with respect to the transform"),
    ("parameters on the cpu", lambda: (_g(2, 3, 5), L3(), _lstm()), RuntimeError,
     "lstm.weight_ih_l0 is on cpu, layers on cuda:0: the HIP path has no CPU fallback"),
]


@pytest.mark.parametrize("what, make, exc, text", RAISES, ids=[r[0] for r in RAISES])
def test_bilstm_layers_raises(what, make, exc, text):
    transform, layers, lstm = make()
    with pytest.raises(exc, match=re.escape(text)):
        pkg.bilstm_layers(transform, layers, lstm)
    assert pkg.takes_hip_lstm_layers(transform, layers, lstm) is False


def test_a_wanted_gradient_raises_only_with_grad_enabled():
    with torch.no_grad(), pytest.raises(RuntimeError, match="transform is on cpu"):    # past the gradient check, to the next one
        pkg.bilstm_layers(torch.zeros(2, 3, 5), [torch.zeros(2, 5, 8)] * 3, _trainable(_lstm()))


def _params_on_fake_gpu(monkeypatch):
    """The module's parameters answering as GPU tensors where the checks and the predicate read them (``recurrent._params``)."""
    monkeypatch.setattr(recurrent, "_params", lambda lstm: [None if p is None else p.detach().as_subclass(_Fake0)
                                                            for p in (getattr(lstm, n, None) for n in recurrent.PARAMS)])


def test_predicate(monkeypatch):
    forms = []

    class _Lib:
        def ggcn_linear_pooled_layers_form(self, *a):
            forms.append(a)
            return pkg.load_library().ggcn_linear_pooled_layers_form(*a)
    monkeypatch.setattr(recurrent._capi, "load_library", lambda: _Lib())
    _params_on_fake_gpu(monkeypatch)
    lstm = _lstm(96)
    transform, layers = _g(2, 3, 5), [_g(2, 5, 32) for _ in range(3)]
    assert pkg.takes_hip_lstm_layers(transform, layers, lstm, 0) is True and len(forms) == 1
    a = forms[0]
    assert (a[5], a[6], a[7], a[10]) == (3, 5 * 32, 32, 1024) and tuple(a[11:]) == (2, 3, 5, 32, 1024)
    assert pkg.takes_hip_lstm_layers(transform, tuple(layers), lstm, 0) is True
    # the form's answer is part of it: Dl = 24 has no form (the entry would refuse), three layers of 8 do not either
    assert pkg.takes_hip_lstm_layers(transform, [_g(2, 5, 24) for _ in range(4)], lstm, 0) is False
    # layers that do not share their strides are asked about as the contiguous copies bilstm_layers makes; nothing is copied
    wide = _g(2, 5, 40)[:, :, :32]
    assert pkg.takes_hip_lstm_layers(transform, [layers[0], wide, layers[2]], lstm, 0) is True
    assert forms[-1][6] == 5 * 32 and forms[-1][7] == 32
    # a layer that requires grad answers False even where grad is disabled; so does a wanted gradient; CPU tensors; bf16
    with torch.no_grad():
        assert pkg.takes_hip_lstm_layers(transform, [layers[0].clone().as_subclass(_Fake0).requires_grad_(True)] + layers[1:], lstm, 0) is False
    assert pkg.takes_hip_lstm_layers(torch.zeros(2, 3, 5), [torch.zeros(2, 5, 32)] * 3, lstm, 0) is False
    assert pkg.takes_hip_lstm_layers(transform, [_g(2, 5, 32, dtype=torch.bfloat16) for _ in range(3)], lstm, 0) is False
    assert pkg.takes_hip_lstm_layers(transform, [_g(2, 5, 32) for _ in range(17)], _lstm(17 * 32), 0) is False
    assert pkg.takes_hip_lstm_layers(transform, None, lstm, 0) is False and pkg.takes_hip_lstm_layers(None, layers, lstm, 0) is False
    # the measured floor on the rows B*T: below it the answer is False unless the caller lowers it; the form is not asked
    n = len(forms)
    assert pkg.takes_hip_lstm_layers(transform, layers, lstm) is False and pkg.takes_hip_lstm_layers(transform, layers, lstm, 7) is False
    assert len(forms) == n and pkg.takes_hip_lstm_layers(transform, layers, lstm, 6) is True
    big = torch.zeros(1).expand(4096, 32, 5).as_subclass(_Fake0)
    assert pkg.takes_hip_lstm_layers(big, [torch.zeros(1).expand(4096, 5, 32).as_subclass(_Fake0) for _ in range(3)], lstm) is True
    # empty operands are served without the launch: no question to the form
    n = len(forms)
    assert pkg.takes_hip_lstm_layers(_g(0, 3, 5), [_g(0, 5, 32) for _ in range(3)], lstm, 0) is True and len(forms) == n


# ---------------------------------------------------------------- the classifier's option
CLASSIFIERS = ["GatedGCNEventDetector", "GatedGCNEventDetector54", "GCNEventDetectorNoGate"]
ENV = ("GGCN_LSTM_LAYERS", "GGCN_POOL_LAYERS", "GGCN_HIP_LSTM_BACKWARD", "GGCN_HIP_LSTM", "GGCN_GATE_BACKWARD", "GGCN_HEAD_BACKWARD")


class _Bert(torch.nn.Module):
    """Stands in for the encoder: thirteen seeded [B,L,768] layers (one more than the classifier takes) and a pooled vector."""

    def __init__(self, as_tuple=False, as_tensor=False):
        super().__init__()
        self.as_tuple, self.as_tensor, self.last = as_tuple, as_tensor, None

    def forward(self, ids_, seg, output_all_encoded_layers=True):
        gen = torch.Generator().manual_seed(1)
        self.last = [torch.randn(ids_.shape[0], ids_.shape[1], 768, generator=gen) for _ in range(13)]
        out = tuple(self.last) if self.as_tuple else list(self.last)
        return (torch.stack(self.last) if self.as_tensor else out), torch.zeros(ids_.shape[0], 768)


def _classifier(cls, bert=None, **opt):
    return cls(bert or _Bert(), types.SimpleNamespace(dropout=0.0, polarities_dim=5, **opt))


@pytest.mark.parametrize("cls_name", CLASSIFIERS)
def test_option_is_off_by_default_and_read_from_opt_and_environment(monkeypatch, cls_name):
    cls = getattr(pkg, cls_name)
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    assert _classifier(cls).lstm_layers is False
    assert _classifier(cls, ggcn_lstm_layers=True).lstm_layers is True
    assert _classifier(cls, ggcn_lstm_layers=False).lstm_layers is False
    on = _classifier(cls, ggcn_lstm_layers=True)
    assert on.hip_lstm is False and on.pool_layers is False and on.hip_lstm_backward is False, "the options are independent"
    others = _classifier(cls, ggcn_hip_lstm=True, ggcn_pool_layers=True, ggcn_hip_lstm_backward=True)
    assert others.lstm_layers is False
    monkeypatch.setenv("GGCN_LSTM_LAYERS", "1")
    assert _classifier(cls).lstm_layers is True and _classifier(cls).hip_lstm is False and _classifier(cls).pool_layers is False
    monkeypatch.setenv("GGCN_LSTM_LAYERS", "0")
    assert _classifier(cls).lstm_layers is False
    assert sorted(on.state_dict()) == sorted(_classifier(cls).state_dict()), "the option adds nothing to the state_dict"


class _Taken(Exception):
    """``bilstm_layers`` was called."""


class _Cat(Exception):
    """``subword_pool`` was called at line :600."""


def _path(model, inputs):
    try:
        model(inputs)
    except _Taken:
        return "bilstm_layers"
    except _Cat:
        return "subword_pool"
    raise AssertionError("the forward passed line :610 without either")


@pytest.mark.parametrize("cls_name", CLASSIFIERS)
def test_path_choice(monkeypatch, cls_name):
    cls = getattr(pkg, cls_name)
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    inputs = ace_batch(np.random.default_rng(3), 4, 9, 20, vocab=100)
    inputs["transform"] = inputs["transform"].double()          # the classifier hands both entry points a float32 transform
    T, L = int(inputs["sentence_length"].max()), int(inputs["cls_text_sep_length"].max())
    answer, asked, anchors, taken = [True], [], [], []

    def predicate(transform, layers, lstm, min_rows):
        asked.append((transform, layers, lstm, min_rows))
        return answer[0]

    def anchor_stub(transform, layers, anchor, length, sides):
        anchors.append((transform, layers, anchor, length, sides))
        return torch.zeros(transform.shape[0], 12 * 768)

    def lstm_stub(transform, layers, lstm):
        taken.append((transform, layers, lstm))
        raise _Taken()

    def cat_stub(transform, x):
        raise _Cat()

    monkeypatch.setattr(classifier, "takes_hip_lstm_layers", predicate)
    monkeypatch.setattr(classifier, "anchor_pool_layers", anchor_stub)
    monkeypatch.setattr(classifier, "bilstm_layers", lstm_stub)
    monkeypatch.setattr(classifier, "subword_pool", cat_stub)
    off = _classifier(cls)
    assert _path(off, inputs) == "subword_pool" and not asked, "the option is off: the predicate is not even asked"
    for as_tuple in (False, True):
        on = _classifier(cls, _Bert(as_tuple=as_tuple), ggcn_lstm_layers=True)
        assert _path(on, inputs) == "bilstm_layers"
        transform, layers, lstm = taken[-1]
        assert transform.dtype == torch.float32 and torch.equal(transform, inputs["transform"][:, :T, :L].float())
        assert isinstance(layers, tuple if as_tuple else list) and len(layers) == 12 and lstm is on.lstm
        assert all(got is want for got, want in zip(layers, on.bert.last[-12:])), "the last twelve layers, as they are"
        assert asked[-1][1] is layers and asked[-1][2] is on.lstm and asked[-1][3] == recurrent.LAYERS_MIN_ROWS == 4096 * 32
        a_transform, a_layers, a_anchor, a_length, a_sides = anchors[-1]
        assert a_layers is layers and torch.equal(a_transform, transform) and a_length is None and a_sides is False
        assert a_anchor.dtype == torch.int64 and torch.equal(a_anchor, inputs["anchor_index"].long())
    floor = _classifier(cls, ggcn_lstm_layers=True, ggcn_lstm_layers_min_rows=0)
    assert _path(floor, inputs) == "bilstm_layers" and asked[-1][3] == 0 and floor.lstm_layers_min_rows == 0
    taken.pop()
    n_taken = len(taken)
    both = _classifier(cls, ggcn_lstm_layers=True, ggcn_hip_lstm=True, ggcn_pool_layers=True)
    assert _path(both, inputs) == "bilstm_layers", "independent of hip_lstm and pool_layers"
    # the predicate says no (training through the LSTM, bf16 layers, CPU tensors ...): today's path
    answer[0] = False
    assert _path(_classifier(cls, ggcn_lstm_layers=True), inputs) == "subword_pool"
    answer[0] = True
    # BERT returns one tensor, not a list: today's path, the predicate not asked
    n_asked = len(asked)
    with pytest.raises(Exception) as e:
        _classifier(cls, _Bert(as_tensor=True), ggcn_lstm_layers=True)(inputs)
    assert not isinstance(e.value, _Taken) and len(asked) == n_asked
    # cuda autocast: today's path, the predicate not asked
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)
    assert _path(_classifier(cls, ggcn_lstm_layers=True), inputs) == "subword_pool"
    assert len(asked) == n_asked and len(taken) == n_taken + 1


# ---------------------------------------------------------------- the statement of the launch, in numpy
def _fma32(a, b, c):
    """float32 ``fma(a, b, c)``: the product of two float32 is exact in float64; the sum is rounded to float64 and then to
    float32, which differs from one rounding only on a float32 tie that the float64 rounding created -- inside every bound here."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def statement(a, layers, w):
    """``Y = P . W`` with ``P[b, r, l*Dl + k] = `` the float32 FMA chain over the non-zeros of ``a[b, r]`` in ascending column,
    from 0.0f, absent entries skipped; the product with ``w [n*Dl, F]`` in float64.  numpy in, float64 ``[B*R, F]`` out."""
    B, R, C = a.shape
    x = np.concatenate(layers, axis=-1)
    pooled = np.zeros((B, R, x.shape[2]), dtype=np.float32)
    for b in range(B):
        for r in range(R):
            for c in range(C):
                if a[b, r, c] != 0:
                    pooled[b, r] = _fma32(np.full_like(x[b, c], a[b, r, c]), x[b, c], pooled[b, r])
    return pooled.reshape(B * R, -1).astype(np.float64) @ w.astype(np.float64)


def test_statement_against_float64():
    rng = np.random.default_rng(11)
    B, R, C, Dl, n, F = 3, 7, 20, 32, 3, 24
    a = np.zeros((B, R, C), dtype=np.float32)
    for b in range(B):
        off = 1
        for r in range(R - 1):                       # runs of 1/l, the last word without a sub-word
            l = int(rng.integers(1, 4))
            a[b, r, off:off + l] = np.float32(1.0 / l)
            off += l
    a[1, 2, :] = rng.uniform(-1, 1, size=C).astype(np.float32)        # a dense row of negative and unequal weights
    layers = [rng.standard_normal((B, C, Dl)).astype(np.float32) for _ in range(n)]
    a[:, :, 0] = a[:, :, C - 1] = 0.0                # [CLS] and the last position: no word selects them
    for x in layers:
        x[:, 0, :] = np.nan
        x[:, C - 1, :] = np.inf
    w = rng.uniform(-0.1, 0.1, size=(n * Dl, F)).astype(np.float32)
    y = statement(a, layers, w)
    assert np.isfinite(y).all(), "a row that no word selects reached the result"
    assert not y.reshape(B, R, F)[:, R - 1].any(), "a word without a sub-word: exact zeros"
    xc = np.where(np.isfinite(np.concatenate(layers, -1)), np.concatenate(layers, -1), 0.0).astype(np.float64)
    a64 = a.astype(np.float64)
    ref = (a64 @ xc).reshape(B * R, -1) @ w.astype(np.float64)
    S = (np.abs(a64) @ np.abs(xc)).reshape(B * R, -1) @ np.abs(w.astype(np.float64))
    K = n * Dl
    bound = lr.gate_bx3(S, K)
    err = np.abs(y - ref)
    assert (err <= bound).all(), "worst %.3g of the bound" % float((err / np.maximum(bound, 1e-300)).max())
    assert float(err.max()) > 0.0, "float32 pooling leaves a trace against float64: the statement is not the reference itself"
