"""Host side of the layer-list pooling (``ggcn_subword_pool_layers``, ``ggcn_subword_pool_layers_form``,
``pooling.subword_pool_layers``): the two entries on all three sides of the ABI, every refusal with its status and exact
``ggcn_last_error`` text (every check comes before a launch: the pointers handed in are never dereferenced, so no GPU is needed),
the vector / scalar rule on fake pointer values, the raises of ``subword_pool_layers`` and the classifier's opt-in ``pool_layers``."""
import ctypes
import re
import types

import numpy as np
import pytest
import torch

import ed_gated_gcn_amd as pkg
from ed_gated_gcn_amd import _capi, classifier, pooling
from oracle.gpu_support import ace_batch
from oracle.host_support import header as _header, msg as _msg

EINVAL, EUNSUPPORTED = 1, 3
ENTRY, FORM = "ggcn_subword_pool_layers", "ggcn_subword_pool_layers_form"
A, X, Y = 1 << 20, 1 << 24, 1 << 28          # fake addresses, 512-byte aligned like a fresh device allocation; never dereferenced
NAMES = ("A", "sa_b", "sa_r", "sa_c", "layers", "n_layers", "is_bf16", "x_batch", "ldx", "Y", "y_batch", "ldy", "B", "R", "C", "Dl")


def _args(**kw):
    """The argument list of ``..._form`` (the entry's without the stream) for 12 layers [2, 9, 768] into Y [2, 3, 9216]; ``ptrs``
    overrides the layers' addresses (None: a NULL entry), every other keyword the argument of that name."""
    n = kw.get("n_layers", 12)
    a = dict(A=A, sa_b=27, sa_r=9, sa_c=1, n_layers=n, is_bf16=0, x_batch=9 * 768, ldx=768, Y=Y, y_batch=3 * n * 768,
             ldy=n * 768, B=2, R=3, C=9, Dl=768)
    ptrs = kw.pop("ptrs", None)
    a.update(kw)
    if ptrs is None:
        size = 2 if a["is_bf16"] else 4
        ptrs = [X + l * a["B"] * a["x_batch"] * size for l in range(max(n, 0))]
    a.setdefault("layers", (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs))
    return [None if a[k] is None else (ctypes.c_void_p(a[k]) if k in ("A", "Y") else a[k]) for k in NAMES]


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
    form = [vp, i64, i64, i64, vp, i32, i32, i64, i64, vp, i64, i64, i32, i32, i32, i32]
    assert _capi.PROTOTYPES[FORM][1] == form and _capi.PROTOTYPES[ENTRY][1] == form + [vp]      # ... and the stream
    assert "#define GGCN_ABI_VERSION 14" in header and "#define GGCN_POOL_MAX_LAYERS 16" in header
    assert _capi.ABI_VERSION == 14 and pkg.load_library().ggcn_abi_version() == 14
    assert _capi.POOL_MAX_LAYERS == pooling.MAX_LAYERS == 16


def test_the_package_exports_the_function():
    assert pkg.subword_pool_layers is pooling.subword_pool_layers and "subword_pool_layers" in pkg.__all__
    assert classifier.subword_pool_layers is pooling.subword_pool_layers


# ---------------------------------------------------------------- the refusals
NULL = "null pointer"
LEADING = "leading dimension too small"
SPLIT = "n_layers=%d > 16 layers a launch (split the layers into groups of 16, each into its own columns of Y)"
REFUSALS = [
    (dict(A=None), EINVAL, NULL), (dict(layers=None), EINVAL, NULL), (dict(Y=None), EINVAL, NULL),
    (dict(ptrs=[X] * 5 + [None] + [X] * 6), EINVAL, "layers[5] is a null pointer"),
    (dict(ptrs=[None] + [X] * 11), EINVAL, "layers[0] is a null pointer"),
    (dict(n_layers=0), EINVAL, "n_layers=0 must be positive"), (dict(n_layers=-3), EINVAL, "n_layers=-3 must be positive"),
    (dict(B=0), EINVAL, "B=0 R=3 C=9 Dl=768 must be positive"), (dict(R=-1), EINVAL, "B=2 R=-1 C=9 Dl=768 must be positive"),
    (dict(C=0), EINVAL, "B=2 R=3 C=0 Dl=768 must be positive"), (dict(Dl=0), EINVAL, "B=2 R=3 C=9 Dl=0 must be positive"),
    (dict(ldx=767), EINVAL, LEADING), (dict(ldy=12 * 768 - 1), EINVAL, LEADING),
    (dict(ldy=768), EINVAL, LEADING),                                        # wide enough for one layer, not for twelve
    (dict(A=A + 2), EINVAL, "A or Y not aligned to its element"), (dict(Y=Y + 2), EINVAL, "A or Y not aligned to its element"),
    (dict(Y=Y + 1, is_bf16=1), EINVAL, "A or Y not aligned to its element"),
    (dict(ptrs=[X] * 11 + [X + 2]), EINVAL, "layers[11] not aligned to its element"),
    (dict(ptrs=[X, X + 1] + [X] * 10, is_bf16=1), EINVAL, "layers[1] not aligned to its element"),
    (dict(n_layers=17), EUNSUPPORTED, SPLIT % 17), (dict(n_layers=1 << 20, ptrs=[X]), EUNSUPPORTED, SPLIT % (1 << 20)),
    (dict(C=2049), EUNSUPPORTED, "C=2049 > 2048 columns"),
    (dict(B=1 << 16, R=1 << 15), EUNSUPPORTED, "too many rows"),
    (dict(n_layers=16, Dl=1 << 22, ldx=1 << 22, ldy=1 << 26), EUNSUPPORTED,
     "n_layers=16 Dl=4194304 needs more than 65535 workgroups a row"),
    (dict(A=None, n_layers=0, B=0), EINVAL, NULL),                           # the order of the checks: pointers first,
    (dict(n_layers=0, B=0), EINVAL, "n_layers=0 must be positive"),          # then the number of layers,
    (dict(n_layers=17, ptrs=[None] * 17, B=0), EUNSUPPORTED, SPLIT % 17),    # its cap before any layers[l] is read,
    (dict(ptrs=[None] * 12, B=0), EINVAL, "layers[0] is a null pointer"),    # the layers before the sizes
    (dict(B=0, C=4096), EINVAL, "B=0 R=3 C=4096 Dl=768 must be positive"),
]


@pytest.mark.parametrize("kw, code, text", REFUSALS)
def test_entry_refuses_before_it_launches_and_form_negates_the_status(kw, code, text):
    lib = pkg.load_library()
    assert _msg(lib, lib.ggcn_subword_pool_layers(*_args(**kw), None), code, ENTRY) == "%s: %s" % (ENTRY, text)
    assert lib.ggcn_subword_pool_layers_form(*_args(**kw)) == -code
    assert lib.ggcn_last_error().decode() == "%s: %s" % (ENTRY, text)


def test_the_largest_grid_is_accepted_by_form():
    lib = pkg.load_library()
    # 16 layers x 16383 units of 256 features = 65532 workgroups a row; one more unit a layer makes 65536
    Dl = 16383 * 256
    assert lib.ggcn_subword_pool_layers_form(*_args(n_layers=16, Dl=Dl, ldx=Dl, ldy=16 * Dl, x_batch=9 * Dl, y_batch=48 * Dl)) == 1
    Dl += 4
    assert lib.ggcn_subword_pool_layers_form(*_args(n_layers=16, Dl=Dl, ldx=Dl, ldy=16 * Dl, x_batch=9 * Dl, y_batch=48 * Dl)) == -EUNSUPPORTED


# ---------------------------------------------------------------- the vector / scalar rule
def _form(**kw):
    return pkg.load_library().ggcn_subword_pool_layers_form(*_args(**kw))


def test_form_vector_scalar_rule():
    twelve = [X + l * 2 * 9 * 768 * 4 for l in range(12)]
    assert _form() == 1 and _form(is_bf16=1) == 1 and _form(n_layers=1) == 1 and _form(n_layers=16) == 1
    for k in range(12):                                     # one misaligned layer among twelve
        assert _form(ptrs=twelve[:k] + [twelve[k] + 4] + twelve[k + 1:]) == 0, k
        assert _form(ptrs=twelve[:k] + [twelve[k] + 8] + twelve[k + 1:]) == 0, k
        assert _form(ptrs=twelve[:k] + [twelve[k] + 16] + twelve[k + 1:]) == 1, k
        # four bf16 are 8 bytes
        assert _form(ptrs=twelve[:k] + [twelve[k] + 2] + twelve[k + 1:], is_bf16=1) == 0, k
        assert _form(ptrs=twelve[:k] + [twelve[k] + 8] + twelve[k + 1:], is_bf16=1) == 1, k
    assert _form(Y=Y + 4) == 0 and _form(Y=Y + 16) == 1 and _form(Y=Y + 8, is_bf16=1) == 1 and _form(Y=Y + 4, is_bf16=1) == 0
    # each size alone
    assert _form(Dl=766) == 0 and _form(Dl=764) == 1                           # Dl % 4 (ldx, ldy stay 768 and 9216)
    assert _form(ldx=770) == 0 and _form(ldx=772) == 1
    assert _form(x_batch=9 * 768 + 2) == 0 and _form(x_batch=9 * 768 + 4) == 1
    assert _form(y_batch=3 * 9216 + 1) == 0 and _form(y_batch=3 * 9216 + 4) == 1
    assert _form(ldy=9217) == 0 and _form(ldy=9220) == 1
    # the strides of A play no part
    assert _form(sa_b=1, sa_r=3, sa_c=7) == 1


# ---------------------------------------------------------------- subword_pool_layers' raises
def _fake_gpu(t, device="cuda:0"):
    """A stand-in for a GPU tensor: what the checks ask of a tensor, answered by ``t`` with ``is_cuda``."""
    return t.as_subclass(_FAKES[device])


class _Fake0(torch.Tensor):
    is_cuda = True
    device = torch.device("cuda:0")


class _Fake1(_Fake0):
    device = torch.device("cuda:1")


_FAKES = {"cuda:0": _Fake0, "cuda:1": _Fake1}


def _g(*shape, dtype=torch.float32, device="cuda:0"):
    return _fake_gpu(torch.zeros(*shape, dtype=dtype), device)


RAISES = [
    ("transform not a tensor", lambda: ([[1.0]], [_g(2, 5, 8)]), TypeError, "transform must be a 3-d tensor"),
    ("transform 2-d", lambda: (_g(3, 5), [_g(2, 5, 8)]), TypeError, "transform must be a 3-d tensor"),
    ("transform on the cpu", lambda: (torch.zeros(2, 3, 5), [_g(2, 5, 8)]), RuntimeError,
     "transform is on cpu: the HIP path has no CPU fallback"),
    ("transform bf16", lambda: (_g(2, 3, 5, dtype=torch.bfloat16), [_g(2, 5, 8)]), RuntimeError,
     "transform must be float32, got torch.bfloat16"),
    ("empty list", lambda: (_g(2, 3, 5), []), TypeError, "layers must be a non-empty list or tuple of 3-d tensors"),
    ("empty tuple", lambda: (_g(2, 3, 5), ()), TypeError, "layers must be a non-empty list or tuple of 3-d tensors"),
    ("a tensor, not a list", lambda: (_g(2, 3, 5), _g(2, 5, 8)), TypeError, "layers must be a non-empty list or tuple of 3-d tensors"),
    ("not a tensor in the list", lambda: (_g(2, 3, 5), [_g(2, 5, 8), None]), TypeError, "layers[1] must be a 3-d tensor"),
    ("2-d layer", lambda: (_g(2, 3, 5), [_g(5, 8)]), TypeError, "layers[0] must be a 3-d tensor"),
    ("layer on the cpu", lambda: (_g(2, 3, 5), [_g(2, 5, 8), torch.zeros(2, 5, 8)]), RuntimeError,
     "layers[1] is on cpu: the HIP path has no CPU fallback"),
    ("float16 layer", lambda: (_g(2, 3, 5), [_g(2, 5, 8, dtype=torch.float16)]), RuntimeError,
     "layers[0] must be float32 or bfloat16, got torch.float16"),
    ("mixed shapes", lambda: (_g(2, 3, 5), [_g(2, 5, 8), _g(2, 5, 8), _g(2, 5, 9)]), RuntimeError,
     "layers[2] (2, 5, 9) torch.float32 does not match layers[0] (2, 5, 8) torch.float32"),
    ("mixed dtypes", lambda: (_g(2, 3, 5), [_g(2, 5, 8), _g(2, 5, 8, dtype=torch.bfloat16)]), RuntimeError,
     "layers[1] (2, 5, 8) torch.bfloat16 does not match layers[0] (2, 5, 8) torch.float32"),
    ("layers on two devices", lambda: (_g(2, 3, 5), [_g(2, 5, 8), _g(2, 5, 8, device="cuda:1")]), RuntimeError,
     "layers[1] and layers[0] are on different devices"),
    ("batch mismatch", lambda: (_g(3, 3, 5), [_g(2, 5, 8)]), RuntimeError, "transform (3, 3, 5) does not match layers (2, 5, 8)"),
    ("length mismatch", lambda: (_g(2, 3, 6), [_g(2, 5, 8)]), RuntimeError, "transform (2, 3, 6) does not match layers (2, 5, 8)"),
    ("transform on another device", lambda: (_g(2, 3, 5, device="cuda:1"), [_g(2, 5, 8)]), RuntimeError,
     "transform and layers are on different devices"),
    ("transform wants a gradient", lambda: (_g(2, 3, 5).requires_grad_(True), [_g(2, 5, 8)]), RuntimeError,
     "subword_pool_layers does not differentiate with respect to the transform"),
]


@pytest.mark.parametrize("what, make, exc, text", RAISES, ids=[r[0] for r in RAISES])
def test_subword_pool_layers_raises(what, make, exc, text):
    transform, layers = make()
    with pytest.raises(exc, match=re.escape(text)):
        pkg.subword_pool_layers(transform, layers)


# ---------------------------------------------------------------- the classifier's option
CLASSIFIERS = ["GatedGCNEventDetector", "GatedGCNEventDetector54", "GCNEventDetectorNoGate"]
ENV = ("GGCN_POOL_LAYERS", "GGCN_HIP_LSTM_BACKWARD", "GGCN_HIP_LSTM", "GGCN_GATE_BACKWARD", "GGCN_HEAD_BACKWARD")


class _Bert(torch.nn.Module):
    """Stands in for the encoder: thirteen seeded [B,L,768] layers (one more than the classifier takes) and a pooled vector;
    ``wrap`` is applied to every layer, ``as_tuple`` returns the layers as a tuple."""

    def __init__(self, wrap=lambda t: t, as_tuple=False):
        super().__init__()
        self.wrap, self.as_tuple, self.last = wrap, as_tuple, None

    def forward(self, ids_, seg, output_all_encoded_layers=True):
        gen = torch.Generator().manual_seed(1)
        self.last = [self.wrap(torch.randn(ids_.shape[0], ids_.shape[1], 768, generator=gen)) for _ in range(13)]
        return (tuple(self.last) if self.as_tuple else list(self.last)), torch.zeros(ids_.shape[0], 768)


def _classifier(cls, bert=None, **opt):
    return cls(bert or _Bert(), types.SimpleNamespace(dropout=0.0, polarities_dim=5, **opt))


@pytest.mark.parametrize("cls_name", CLASSIFIERS)
def test_option_is_off_by_default_and_read_from_opt_and_environment(monkeypatch, cls_name):
    cls = getattr(pkg, cls_name)
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    assert _classifier(cls).pool_layers is False
    assert _classifier(cls, ggcn_pool_layers=True).pool_layers is True
    assert _classifier(cls, ggcn_pool_layers=False).pool_layers is False
    on = _classifier(cls, ggcn_pool_layers=True)
    assert on.hip_lstm is False and on.hip_lstm_backward is False and on.gate_backward is False and on.head_backward is False, \
        "the options are independent"
    others = _classifier(cls, ggcn_hip_lstm=True, ggcn_hip_lstm_backward=True, ggcn_gate_backward=True, ggcn_head_backward=True)
    assert others.pool_layers is False
    monkeypatch.setenv("GGCN_POOL_LAYERS", "1")
    assert _classifier(cls).pool_layers is True and _classifier(cls).hip_lstm is False
    monkeypatch.setenv("GGCN_POOL_LAYERS", "0")
    assert _classifier(cls).pool_layers is False
    assert sorted(on.state_dict()) == sorted(_classifier(cls).state_dict()), "the option adds nothing to the state_dict"


class _Layers(Exception):
    """``subword_pool_layers`` was called at lines :596-600."""


class _Cat(Exception):
    """``subword_pool`` was called at line :600."""


def _lines_596_600(model, inputs):
    """Which of the two runs (the forward is cut short there: what follows has no CPU path)."""
    try:
        model(inputs)
    except _Layers:
        return "subword_pool_layers"
    except _Cat:
        return "subword_pool"
    raise AssertionError("the forward passed line :600 without either")


@pytest.mark.parametrize("as_tuple", [False, True], ids=["list", "tuple"])
@pytest.mark.parametrize("cls_name", CLASSIFIERS)
def test_option_reaches_subword_pool_layers_only_when_on_and_on_gpu_layers(monkeypatch, cls_name, as_tuple):
    cls = getattr(pkg, cls_name)
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    inputs = ace_batch(np.random.default_rng(3), 4, 9, 20, vocab=100)
    inputs["transform"] = inputs["transform"].double()          # the classifier hands the pooling a float32 transform
    T, L = int(inputs["sentence_length"].max()), int(inputs["cls_text_sep_length"].max())
    seen_layers, seen_cat = [], []

    def layers_stub(transform, layers):
        seen_layers.append((transform, layers))
        raise _Layers()

    def cat_stub(transform, x):
        seen_cat.append((transform, x))
        raise _Cat()

    monkeypatch.setattr(classifier, "subword_pool_layers", layers_stub)
    monkeypatch.setattr(classifier, "subword_pool", cat_stub)
    # CPU layers: the option changes nothing
    cpu_on, cpu_off = _classifier(cls, _Bert(as_tuple=as_tuple), ggcn_pool_layers=True), _classifier(cls, _Bert(as_tuple=as_tuple))
    assert _lines_596_600(cpu_on, inputs) == "subword_pool" and _lines_596_600(cpu_off, inputs) == "subword_pool"
    assert not seen_layers and len(seen_cat) == 2
    assert tuple(seen_cat[0][1].shape) == (4, L, 12 * 768) and seen_cat[0][0].dtype == torch.float32
    # from here on BERT's layers answer as GPU tensors would
    on = _classifier(cls, _Bert(_fake_gpu, as_tuple), ggcn_pool_layers=True)
    off = _classifier(cls, _Bert(_fake_gpu, as_tuple))
    both = _classifier(cls, _Bert(_fake_gpu, as_tuple), ggcn_pool_layers=True, ggcn_hip_lstm=True, ggcn_hip_lstm_backward=True)
    assert _lines_596_600(off, inputs) == "subword_pool" and not seen_layers, "the option is off"
    assert _lines_596_600(on, inputs) == "subword_pool_layers" and len(seen_layers) == 1
    transform, layers = seen_layers[0]
    assert transform.dtype == torch.float32 and tuple(transform.shape) == (4, T, L)
    assert torch.equal(transform, inputs["transform"][:, :T, :L].float())
    assert isinstance(layers, tuple if as_tuple else list) and len(layers) == 12
    assert all(got is want for got, want in zip(layers, on.bert.last[-12:])), "the last twelve layers, as they are"
    assert _lines_596_600(both, inputs) == "subword_pool_layers", "independent of the other options"
    with torch.no_grad():
        assert _lines_596_600(on.eval(), inputs) == "subword_pool_layers", "inference and training alike"
    # one layer that is not a GPU tensor, or layers that are no list: today's two lines
    mixed = _classifier(cls, _Bert(lambda t, c=[0]: (c.__setitem__(0, c[0] + 1), t if c[0] == 7 else _fake_gpu(t))[1], as_tuple),
                        ggcn_pool_layers=True)
    assert _lines_596_600(mixed, inputs) == "subword_pool"
    assert len(seen_layers) == 3
