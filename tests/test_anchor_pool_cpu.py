"""Host side of the baselines' one-launch step (``ggcn_anchor_pool_layers``, ``ggcn_anchor_pool_layers_form``,
``pooling.anchor_pool_layers``, ``AnchorEventDetector``, ``DynamicMultiPoolEventDetector``): the statement of the header against
the reference's formula evaluated with torch CPU ops (``torch.equal``), the margin of the GPU test held by a float32 emulation in
the kernel's order, the two entries on all three sides of the ABI, every refusal with its status and exact ``ggcn_last_error``
text (every check comes before a launch: the pointers handed in are never dereferenced, so no GPU is needed), the vector /
scalar rule on fake pointer values, the raises of ``anchor_pool_layers``, the classifiers' ``state_dict`` and their path choice."""
import ctypes
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import ed_gated_gcn_amd as pkg
from ed_gated_gcn_amd import _capi, classifier, pooling
from oracle.gpu_support import ace_batch
from oracle.host_support import header as _header, msg as _msg
import anchor_pool_ref as ar

EINVAL, EUNSUPPORTED = 1, 3
ENTRY, FORM = "ggcn_anchor_pool_layers", "ggcn_anchor_pool_layers_form"
A, X, Z, AN, LN = 1 << 20, 1 << 24, 1 << 28, 1 << 29, 1 << 30      # fake addresses, 512-byte aligned; never dereferenced
NAMES = ("A", "sa_b", "sa_r", "sa_c", "layers", "n_layers", "is_bf16", "x_batch", "ldx", "anchor", "length", "sides", "Z", "ldz",
         "z_section", "B", "R", "C", "Dl")
POINTERS = ("A", "anchor", "length", "Z")


def _args(**kw):
    """The argument list of ``..._form`` (the entry's without the stream) for 12 layers [2, 9, 768], 3 words, into Z [2, 3*9216];
    ``ptrs`` overrides the layers' addresses (None: a NULL entry), every other keyword the argument of that name."""
    n = kw.get("n_layers", 12)
    a = dict(A=A, sa_b=27, sa_r=9, sa_c=1, n_layers=n, is_bf16=0, x_batch=9 * 768, ldx=768, anchor=AN, length=LN, sides=1, Z=Z,
             ldz=3 * n * 768, z_section=n * 768, B=2, R=3, C=9, Dl=768)
    ptrs = kw.pop("ptrs", None)
    a.update(kw)
    if ptrs is None:
        size = 2 if a["is_bf16"] else 4
        ptrs = [X + l * a["B"] * a["x_batch"] * size for l in range(max(n, 0))]
    a.setdefault("layers", (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs))
    return [None if a[k] is None else (ctypes.c_void_p(a[k]) if k in POINTERS else a[k]) for k in NAMES]


# ---------------------------------------------------------------- the statement against the reference's formula
def _pooled_words(seed, B, T, W, scale, bf16):
    rng = np.random.default_rng(seed)
    v = torch.from_numpy((rng.standard_normal((B, T, W)) * scale).astype(np.float32))
    return v.bfloat16() if bf16 else v


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("scale", [1e-8, 1.0, 300.0])
def test_statement_equals_the_reference_formula_bit_for_bit(scale, bf16):
    """Anchors at both ends and inside, lengths 1..T (shorter than the anchor too), T = 1, all-negative values."""
    for T in (1, 2, 5, 6):
        for negative in (False, True):
            v = _pooled_words(T, T * T, T, 11, scale, bf16)
            if negative:
                v = -v.abs()
            anchor = torch.arange(T).repeat_interleave(T)
            length = torch.arange(1, T + 1).repeat(T)
            want = ar.formula_torch(v, anchor, length)
            assert want.dtype == torch.float32 and tuple(want.shape) == (T * T, 33)
            got = torch.from_numpy(ar.statement(v.float().numpy(), anchor.numpy(), length.numpy()))
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (T, negative)
            alone = torch.from_numpy(ar.statement(v.float().numpy(), anchor.numpy(), None, sides=False))
            assert torch.equal(alone, want[:, :11])


def test_statement_propagates_a_pooled_nan_and_never_reads_a_masked_row():
    v = _pooled_words(1, 2, 5, 4, 1.0, False)
    v[0, 1, 2] = float("nan")                 # sentence 0: word 1, left of the anchor
    v[1, 4, :] = float("inf")                 # sentence 1: word 4, outside the sentence
    anchor, length = torch.tensor([2, 1]), torch.tensor([5, 4])
    z = ar.statement(v.numpy(), anchor.numpy(), length.numpy())
    want = ar.formula_torch(v[:1], anchor[:1], length[:1]).numpy()
    # (on the right side that word is masked: the reference makes NaN of NaN * 0 there, the statement never reads it)
    assert np.isnan(want[0, 8 + 2]) and int(np.isnan(want[0]).sum()) == 2
    want[0, 8 + 2] = z[0, 8 + 2]
    assert np.array_equal(z[0], want[0], equal_nan=True) and np.isnan(z[0, 4 + 2]) and int(np.isnan(z[0]).sum()) == 1
    assert np.isfinite(z[1]).all(), "a masked row that is not finite is ignored (the reference makes NaN of inf * 0)"
    assert np.isnan(ar.formula_torch(v[1:], anchor[1:], length[1:]).numpy()[:, 4:]).any()


def test_statement_clamps_anchor_and_length():
    v = _pooled_words(2, 3, 5, 4, 1.0, False).numpy()
    got = ar.statement(v, [-7, 99, 2], [-1, 3, 1 << 40])
    assert np.array_equal(got, ar.statement(v, [0, 4, 2], [0, 3, 5]))


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", ar.CASES, ids=ar.CASE_IDS)
def test_float32_emulation_in_the_kernels_order_holds_the_margin(case, bf16):
    """The margin the GPU test asks of the kernel, asked first of numpy: pooled in ascending column in float32, rounded to
    bfloat16 once for bf16 layers, then the statement -- against float64 pooling + formula."""
    a, vals, anchor, length = ar.build(case, torch.bfloat16 if bf16 else torch.float32)
    layers = [vals[l] for l in range(case.n)]
    z = ar.statement(ar.emulate_float32(a, layers, bf16), anchor.numpy(), length.numpy())
    ref, bound = ar.ref64_and_bound(a, layers, anchor.numpy(), length.numpy(), bf16)
    ar.assert_within(z, ref, bound, case.name)
    W = case.n * case.Dl
    if case.values == "negative":
        assert not z[:, W:].any() and (z[:, :W] <= 0).all(), "the 1.0f floor decides both sides"
    if case.values == "tiny":
        assert not z[:, W:].any() and z[:, :W].any(), "v + 1 rounds to 1"
    if case.values == "nan":
        assert np.isnan(z).any() and not np.isnan(z).all()


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
    form = [vp, i64, i64, i64, vp, i32, i32, i64, i64, vp, vp, i32, vp, i64, i64, i32, i32, i32, i32]
    assert _capi.PROTOTYPES[FORM][1] == form and _capi.PROTOTYPES[ENTRY][1] == form + [vp]      # ... and the stream
    assert "#define GGCN_ABI_VERSION 14" in header
    assert _capi.ABI_VERSION == 14 and pkg.load_library().ggcn_abi_version() == 14


def test_the_package_exports_the_names():
    for name in ("anchor_pool_layers", "anchor_pool_formula", "AnchorEventDetector", "DynamicMultiPoolEventDetector"):
        assert name in pkg.__all__ and hasattr(pkg, name), name
    assert pkg.anchor_pool_layers is pooling.anchor_pool_layers and classifier.anchor_pool_layers is pooling.anchor_pool_layers
    assert pkg.AnchorEventDetector is classifier.AnchorEventDetector


# ---------------------------------------------------------------- the refusals
NULL = "null pointer"
LEADING = "leading dimension too small"
ALIGN = "A, Z, anchor or length not aligned to its element"
SPLIT = "n_layers=%d > 16 layers a launch (split the layers into groups of 16, each into its own columns of Z)"
REFUSALS = [
    (dict(A=None), EINVAL, NULL), (dict(layers=None), EINVAL, NULL), (dict(Z=None), EINVAL, NULL), (dict(anchor=None), EINVAL, NULL),
    (dict(length=None), EINVAL, "length is a null pointer with sides"),
    (dict(ptrs=[X] * 5 + [None] + [X] * 6), EINVAL, "layers[5] is a null pointer"),
    (dict(ptrs=[None] + [X] * 11), EINVAL, "layers[0] is a null pointer"),
    (dict(n_layers=0), EINVAL, "n_layers=0 must be positive"), (dict(n_layers=-3), EINVAL, "n_layers=-3 must be positive"),
    (dict(B=0), EINVAL, "B=0 R=3 C=9 Dl=768 must be positive"), (dict(R=-1), EINVAL, "B=2 R=-1 C=9 Dl=768 must be positive"),
    (dict(C=0), EINVAL, "B=2 R=3 C=0 Dl=768 must be positive"), (dict(Dl=0), EINVAL, "B=2 R=3 C=9 Dl=0 must be positive"),
    (dict(ldx=767), EINVAL, LEADING), (dict(ldz=3 * 9216 - 1), EINVAL, LEADING),
    (dict(ldz=9216), EINVAL, LEADING),                                        # wide enough for the anchor part alone
    (dict(ldz=9215, sides=0, length=None), EINVAL, LEADING),
    (dict(z_section=9215), EINVAL, "z_section=9215 < n_layers*Dl=9216"),
    (dict(z_section=9220), EINVAL, LEADING),                                  # the third part would pass the end of the row
    (dict(A=A + 2), EINVAL, ALIGN), (dict(Z=Z + 2), EINVAL, ALIGN), (dict(Z=Z + 2, is_bf16=1), EINVAL, ALIGN),
    (dict(anchor=AN + 4), EINVAL, ALIGN), (dict(length=LN + 4), EINVAL, ALIGN),
    (dict(ptrs=[X] * 11 + [X + 2]), EINVAL, "layers[11] not aligned to its element"),
    (dict(ptrs=[X, X + 1] + [X] * 10, is_bf16=1), EINVAL, "layers[1] not aligned to its element"),
    (dict(n_layers=17), EUNSUPPORTED, SPLIT % 17), (dict(n_layers=1 << 20, ptrs=[X]), EUNSUPPORTED, SPLIT % (1 << 20)),
    (dict(C=2049), EUNSUPPORTED, "C=2049 > 2048 columns"),
    (dict(B=1 << 16, R=1 << 15), EUNSUPPORTED, "too many rows"),
    (dict(n_layers=16, Dl=1 << 22, ldx=1 << 22, ldz=3 << 26, z_section=1 << 26), EUNSUPPORTED,
     "n_layers=16 Dl=4194304 needs more than 65535 workgroups a sentence"),
    (dict(A=None, n_layers=0, B=0), EINVAL, NULL),                           # the order of the checks: pointers first,
    (dict(length=None, n_layers=0), EINVAL, "length is a null pointer with sides"),
    (dict(n_layers=0, B=0), EINVAL, "n_layers=0 must be positive"),          # then the number of layers,
    (dict(n_layers=17, ptrs=[None] * 17, B=0), EUNSUPPORTED, SPLIT % 17),    # its cap before any layers[l] is read,
    (dict(ptrs=[None] * 12, B=0), EINVAL, "layers[0] is a null pointer"),    # the layers before the sizes
    (dict(B=0, C=4096), EINVAL, "B=0 R=3 C=4096 Dl=768 must be positive"),
]


@pytest.mark.parametrize("kw, code, text", REFUSALS)
def test_entry_refuses_before_it_launches_and_form_negates_the_status(kw, code, text):
    lib = pkg.load_library()
    assert _msg(lib, lib.ggcn_anchor_pool_layers(*_args(**kw), None), code, ENTRY) == "%s: %s" % (ENTRY, text)
    assert lib.ggcn_anchor_pool_layers_form(*_args(**kw)) == -code
    assert lib.ggcn_last_error().decode() == "%s: %s" % (ENTRY, text)


def _form(**kw):
    return pkg.load_library().ggcn_anchor_pool_layers_form(*_args(**kw))


def test_without_sides_length_and_z_section_play_no_part():
    assert _form(sides=0, length=None, ldz=9216, z_section=0) == 1
    assert _form(sides=0, length=LN + 3, ldz=9216, z_section=-5) == 1, "never touched: neither read nor checked"
    assert _form(sides=0, length=None, ldz=9216, z_section=3) == 1, "z_section % 4 matters with sides only"


def test_the_largest_grid_is_accepted_by_form():
    Dl = 16383 * 256                       # 16 layers x 16383 units = 65532 workgroups a sentence; one more unit makes 65536
    kw = dict(n_layers=16, sides=0, length=None, z_section=0)
    assert _form(Dl=Dl, ldx=Dl, ldz=16 * Dl, x_batch=9 * Dl, **kw) == 1
    Dl += 4
    assert _form(Dl=Dl, ldx=Dl, ldz=16 * Dl, x_batch=9 * Dl, **kw) == -EUNSUPPORTED


def test_form_vector_scalar_rule():
    twelve = [X + l * 2 * 9 * 768 * 4 for l in range(12)]
    assert _form() == 1 and _form(is_bf16=1) == 1 and _form(n_layers=1) == 1 and _form(n_layers=16) == 1
    for k in (0, 5, 11):                                    # one misaligned layer among twelve
        assert _form(ptrs=twelve[:k] + [twelve[k] + 4] + twelve[k + 1:]) == 0, k
        assert _form(ptrs=twelve[:k] + [twelve[k] + 16] + twelve[k + 1:]) == 1, k
        assert _form(ptrs=twelve[:k] + [twelve[k] + 2] + twelve[k + 1:], is_bf16=1) == 0, k      # four bf16 are 8 bytes
        assert _form(ptrs=twelve[:k] + [twelve[k] + 8] + twelve[k + 1:], is_bf16=1) == 1, k
    # Z is float32 for both dtypes of the layers: 16 bytes
    assert _form(Z=Z + 4) == 0 and _form(Z=Z + 16) == 1 and _form(Z=Z + 8, is_bf16=1) == 0 and _form(Z=Z + 16, is_bf16=1) == 1
    # each size alone
    assert _form(Dl=766) == 0 and _form(Dl=764) == 1                           # Dl % 4 (ldx, ldz, z_section stay)
    assert _form(ldx=770) == 0 and _form(ldx=772) == 1
    assert _form(x_batch=9 * 768 + 2) == 0 and _form(x_batch=9 * 768 + 4) == 1
    assert _form(ldz=3 * 9216 + 1) == 0 and _form(ldz=3 * 9216 + 4) == 1
    assert _form(ldz=3 * 9216 + 8, z_section=9217) == 0 and _form(ldz=3 * 9216 + 8, z_section=9220) == 1
    # the strides of A, and the alignment of the two index vectors beyond their element, play no part
    assert _form(sa_b=1, sa_r=3, sa_c=7) == 1 and _form(anchor=AN + 8, length=LN + 8) == 1


# ---------------------------------------------------------------- anchor_pool_layers' raises
class _Fake0(torch.Tensor):
    is_cuda = True
    device = torch.device("cuda:0")


class _Fake1(_Fake0):
    device = torch.device("cuda:1")


_FAKES = {"cuda:0": _Fake0, "cuda:1": _Fake1}


def _fake_gpu(t, device="cuda:0"):
    """A stand-in for a GPU tensor: what the checks ask of a tensor, answered by ``t`` with ``is_cuda``."""
    return t.as_subclass(_FAKES[device])


def _g(*shape, dtype=torch.float32, device="cuda:0"):
    return _fake_gpu(torch.zeros(*shape, dtype=dtype), device)


def _i(n, dtype=torch.int64, device="cuda:0"):
    return _g(n, dtype=dtype, device=device)


RAISES = [
    ("transform 2-d", lambda: (_g(3, 5), [_g(2, 5, 8)], _i(2), _i(2)), TypeError, "transform must be a 3-d tensor"),
    ("transform on the cpu", lambda: (torch.zeros(2, 3, 5), [_g(2, 5, 8)], _i(2), _i(2)), RuntimeError,
     "transform is on cpu: the HIP path has no CPU fallback"),
    ("a tensor, not a list", lambda: (_g(2, 3, 5), _g(2, 5, 8), _i(2), _i(2)), TypeError,
     "layers must be a non-empty list or tuple of 3-d tensors"),
    ("layer on the cpu", lambda: (_g(2, 3, 5), [_g(2, 5, 8), torch.zeros(2, 5, 8)], _i(2), _i(2)), RuntimeError,
     "layers[1] is on cpu: the HIP path has no CPU fallback"),
    ("float16 layer", lambda: (_g(2, 3, 5), [_g(2, 5, 8, dtype=torch.float16)], _i(2), _i(2)), RuntimeError,
     "layers[0] must be float32 or bfloat16, got torch.float16"),
    ("mixed shapes", lambda: (_g(2, 3, 5), [_g(2, 5, 8), _g(2, 5, 9)], _i(2), _i(2)), RuntimeError,
     "layers[1] (2, 5, 9) torch.float32 does not match layers[0] (2, 5, 8) torch.float32"),
    ("batch mismatch", lambda: (_g(3, 3, 5), [_g(2, 5, 8)], _i(2), _i(2)), RuntimeError,
     "transform (3, 3, 5) does not match layers (2, 5, 8)"),
    ("transform wants a gradient", lambda: (_g(2, 3, 5).requires_grad_(True), [_g(2, 5, 8)], _i(2), _i(2)), RuntimeError,
     "anchor_pool_layers does not differentiate with respect to the transform"),
    ("anchor not a tensor", lambda: (_g(2, 3, 5), [_g(2, 5, 8)], [0, 1], _i(2)), TypeError, "anchor must be a 1-d tensor"),
    ("anchor 2-d", lambda: (_g(2, 3, 5), [_g(2, 5, 8)], _g(2, 1, dtype=torch.int64), _i(2)), TypeError, "anchor must be a 1-d tensor"),
    ("anchor int32", lambda: (_g(2, 3, 5), [_g(2, 5, 8)], _i(2, torch.int32), _i(2)), RuntimeError,
     "anchor must be int64, got torch.int32"),
    ("anchor of another batch", lambda: (_g(2, 3, 5), [_g(2, 5, 8)], _i(3), _i(2)), RuntimeError,
     "anchor (3,) does not match the 2 sentences of the layers"),
    ("anchor on the cpu", lambda: (_g(2, 3, 5), [_g(2, 5, 8)], torch.zeros(2, dtype=torch.int64), _i(2)), RuntimeError,
     "anchor and layers are on different devices"),
    ("length missing", lambda: (_g(2, 3, 5), [_g(2, 5, 8)], _i(2), None), TypeError, "anchor_pool_layers needs length with sides=True"),
    ("length float", lambda: (_g(2, 3, 5), [_g(2, 5, 8)], _i(2), _g(2)), RuntimeError, "length must be int64, got torch.float32"),
    ("length on another device", lambda: (_g(2, 3, 5), [_g(2, 5, 8)], _i(2), _i(2, device="cuda:1")), RuntimeError,
     "length and layers are on different devices"),
    ("a layer wants a gradient", lambda: (_g(2, 3, 5), [_g(2, 5, 8), _g(2, 5, 8).requires_grad_(True)], _i(2), _i(2)), RuntimeError,
     "anchor_pool_layers is forward only: for a layer that requires grad take the composed path, "
     "anchor_pool_formula(subword_pool_layers(transform, layers), anchor, length, sides)"),
    ("no words", lambda: (_g(2, 0, 5), [_g(2, 5, 8)], _i(2), _i(2)), RuntimeError,
     "transform (2, 0, 5) has no words: there is no anchor row"),
]


@pytest.mark.parametrize("what, make, exc, text", RAISES, ids=[r[0] for r in RAISES])
def test_anchor_pool_layers_raises(what, make, exc, text):
    transform, layers, anchor, length = make()
    with pytest.raises(exc, match=re.escape(text)):
        pkg.anchor_pool_layers(transform, layers, anchor, length)


def test_without_sides_length_is_not_looked_at():
    with pytest.raises(RuntimeError, match=re.escape("transform (2, 0, 5) has no words")):      # the last check: all others passed
        pkg.anchor_pool_layers(_g(2, 0, 5), [_g(2, 5, 8)], _i(2), "not a tensor", sides=False)


# ---------------------------------------------------------------- the classifiers
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "baseline_state_dicts.json")


class _Bert(torch.nn.Module):
    """Stands in for the encoder: thirteen seeded [B,L,768] layers (one more than a classifier takes) and a pooled vector;
    ``wrap`` is applied to every layer, ``as_tuple`` / ``as_tensor`` change what comes back in the list's place."""

    def __init__(self, wrap=lambda t: t, returns="list"):
        super().__init__()
        self.wrap, self.returns, self.last = wrap, returns, None
        self.embeddings = torch.nn.Embedding(7, 3)          # (a parameter, so that ``bert.*`` shows in the state_dict)

    def forward(self, ids_, seg, output_all_encoded_layers=True):
        gen = torch.Generator().manual_seed(1)
        self.last = [self.wrap(torch.randn(ids_.shape[0], ids_.shape[1], 768, generator=gen)) for _ in range(13)]
        pooled = torch.zeros(ids_.shape[0], 768)
        if self.returns == "tensor":
            return self.wrap(torch.cat(self.last[-4:], -1)), pooled
        return (tuple(self.last) if self.returns == "tuple" else list(self.last)), pooled


def _opt(**kw):
    return types.SimpleNamespace(**dict(dict(dropout=0.0, polarities_dim=34, n_layer=4, bert_dim=768, hidden_dim=128, device="cpu"), **kw))


def test_state_dicts_are_the_reference_models(monkeypatch):
    monkeypatch.delenv("GGCN_ANCHOR_POOL", raising=False)
    want = json.load(open(GOLDEN))
    for name in ("AnchorEventDetector", "DynamicMultiPoolEventDetector"):
        m = getattr(pkg, name)(_Bert(), _opt())
        got = {k: list(v.shape) for k, v in m.state_dict().items()}
        assert got == want[name], name
        assert list(got) == list(want[name]), "the reference's construction order"
        assert m.anchor_pool is True and m.dropout.p == 0.0
    assert pkg.AnchorEventDetector(_Bert(), _opt()).n_layer == 12 and pkg.AnchorEventDetector(_Bert(), _opt()).hidden_dim == 128
    dm = pkg.DynamicMultiPoolEventDetector(_Bert(), _opt(n_layer=2))
    assert dm.n_layer == 2 and tuple(dm.dense.weight.shape) == (34, 2 * 768 * 3)
    assert not list(dm.buffers()), "the reference's self.m is a plain attribute"


@pytest.mark.parametrize("name", ["AnchorEventDetector", "DynamicMultiPoolEventDetector"])
def test_option_is_on_by_default_and_read_from_opt_and_environment(monkeypatch, name):
    cls = getattr(pkg, name)
    monkeypatch.delenv("GGCN_ANCHOR_POOL", raising=False)
    assert cls(_Bert(), _opt()).anchor_pool is True
    assert cls(_Bert(), _opt(ggcn_anchor_pool=False)).anchor_pool is False
    assert cls(_Bert(), _opt(ggcn_anchor_pool=True)).anchor_pool is True
    monkeypatch.setenv("GGCN_ANCHOR_POOL", "0")
    assert cls(_Bert(), _opt()).anchor_pool is False
    monkeypatch.setenv("GGCN_ANCHOR_POOL", "1")
    assert cls(_Bert(), _opt()).anchor_pool is True
    assert sorted(cls(_Bert(), _opt(ggcn_anchor_pool=False)).state_dict()) == sorted(cls(_Bert(), _opt()).state_dict())


class _Reached(Exception):
    def __init__(self, which, args):
        super().__init__(which)
        self.which, self.operands = which, args


def _path(model, inputs):
    """Which of the three pooling calls the forward reaches (it is cut short there: none has a CPU path)."""
    try:
        model(inputs)
    except _Reached as e:
        return e
    raise AssertionError("the forward passed the pooling without any of the three calls")


@pytest.mark.parametrize("name, n, sides", [("AnchorEventDetector", 12, False), ("DynamicMultiPoolEventDetector", 4, True)])
def test_path_choice(monkeypatch, name, n, sides):
    cls = getattr(pkg, name)
    monkeypatch.delenv("GGCN_ANCHOR_POOL", raising=False)
    inputs = ace_batch(np.random.default_rng(3), 4, 9, 20, vocab=100)
    inputs["transform"] = inputs["transform"].double()          # the classifier hands the pooling a float32 transform
    T, L = int(inputs["sentence_length"].max()), int(inputs["cls_text_sep_length"].max())

    def stub(which):
        def f(*args, **kw):
            raise _Reached(which, (args, kw))
        return f
    for which in ("anchor_pool_layers", "subword_pool_layers", "subword_pool"):
        monkeypatch.setattr(classifier, which, stub(which))
    # CPU layers: torch.cat + subword_pool (which raises on the CPU: no fallback)
    e = _path(cls(_Bert(), _opt()), inputs)
    assert e.which == "subword_pool" and tuple(e.operands[0][1].shape) == (4, L, n * 768) and e.operands[0][0].dtype == torch.float32
    for returns in ("list", "tuple"):
        on = cls(_Bert(_fake_gpu, returns), _opt())
        e = _path(on, inputs)
        assert e.which == "anchor_pool_layers", "a list or tuple of GPU tensors none of which requires grad: the one launch"
        (transform, layers, anchor, length), kw = e.operands
        assert kw == {"sides": sides}
        assert transform.dtype == torch.float32 and torch.equal(transform, inputs["transform"][:, :T, :L].float())
        assert isinstance(layers, tuple if returns == "tuple" else list) and len(layers) == n
        assert all(got is want for got, want in zip(layers, on.bert.last[-n:])), "the last n layers, as they are"
        assert anchor.dtype == torch.int64 and torch.equal(anchor, inputs["anchor_index"])
        assert (length is None) if not sides else torch.equal(length, inputs["sentence_length"])
        with torch.no_grad():
            assert _path(on.eval(), inputs).which == "anchor_pool_layers", "inference and training alike"
    # the option off: the composed path, still without the concatenation
    assert _path(cls(_Bert(_fake_gpu), _opt(ggcn_anchor_pool=False)), inputs).which == "subword_pool_layers"
    # a fine-tuned BERT: one layer that requires grad
    tuned = cls(_Bert(lambda t, c=[0]: (c.__setitem__(0, c[0] + 1), _fake_gpu(t).requires_grad_(c[0] == 12))[1]), _opt())
    assert _path(tuned, inputs).which == "subword_pool_layers"
    # a tensor in place of the list: already concatenated
    e = _path(cls(_Bert(_fake_gpu, "tensor"), _opt()), inputs)
    assert e.which == "subword_pool" and tuple(e.operands[0][1].shape) == (4, L, 4 * 768)
    # one layer that is not a GPU tensor
    mixed = cls(_Bert(lambda t, c=[0]: (c.__setitem__(0, c[0] + 1), t if c[0] == 12 else _fake_gpu(t))[1]), _opt())
    assert _path(mixed, inputs).which == "subword_pool"


def test_formula_on_cpu_tensors_equals_the_statement_and_differentiates():
    """``anchor_pool_formula`` -- the composed path's second half -- is plain PyTorch: on the CPU it gives the statement's bits,
    with out-of-range indices clamped, and a gradient reaches ``v``."""
    for bf16 in (False, True):
        v = _pooled_words(5, 4, 6, 10, 1.0, bf16)
        anchor, length = torch.tensor([0, 5, 2, 99]), torch.tensor([6, 6, 1, -3])
        row, pooled = pkg.anchor_pool_formula(v, anchor, length)
        want = torch.from_numpy(ar.statement(v.float().numpy(), anchor.numpy(), length.numpy()))
        assert row.dtype == v.dtype and pooled.dtype == torch.float32
        assert torch.equal(torch.cat((row.float(), pooled), 1), want)
        assert torch.equal(pkg.anchor_pool_formula(v, anchor, sides=False), row)
    v = _pooled_words(6, 2, 4, 3, 1.0, False).requires_grad_(True)
    row, pooled = pkg.anchor_pool_formula(v, torch.tensor([1, 3]), torch.tensor([4, 4]))
    (row.sum() + pooled.sum()).backward()
    assert v.grad is not None and float(v.grad.abs().sum()) > 0
