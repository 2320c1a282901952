"""The baselines' one-launch step (``ggcn_anchor_pool_layers``, ``pooling.anchor_pool_layers``, ``AnchorEventDetector``,
``DynamicMultiPoolEventDetector``) on the GPU.

(a) the C entry on the cases of ``tests/anchor_pool_ref.py``: every layer a view into a NaN buffer, Z between NaN guard bands
    with NaN columns between and behind its three parts, the form asked of ``ggcn_anchor_pool_layers_form``, twice with the same
    bits; compared (1) ``equal`` against the numpy statement applied to ``subword_pool_layers``' output, (2) the anchor columns
    ``torch.equal`` to ``subword_pool_layers`` on the one-row transform, (3) against float64 pooling + formula inside
    ``bound_pool + 2^-24 (|ref + 1| + |ref|)`` per element; and once more without ``sides``.
(b) the Python function against the composed path, its launch counts, 17 layers, a sentence alone, empty operands.
(c) the two classifiers with the option on against off: eval, a training step, under bf16 autocast, and captured into a hipGraph.
"""
import ctypes
import types

import numpy as np
import pytest
import torch

import anchor_pool_ref as ar
from oracle import gates
from oracle import subword_pool_cases as sc
from oracle.gpu_support import classifier_batch, count_calls, dev, pkg  # noqa: F401

pytestmark = pytest.mark.gpu

NEW, LAYERS, OLD, OLD_BF16 = "ggcn_anchor_pool_layers", "ggcn_subword_pool_layers", "ggcn_subword_pool", "ggcn_subword_pool_bf16"
ENTRIES = (NEW, LAYERS, OLD, OLD_BF16)
DTYPES = (torch.float32, torch.bfloat16)
DTYPE_IDS = ("f32", "bf16")
GUARD = 8          # floats of NaN on either side of Z (32 bytes: the view keeps its alignment)
ZGAP = 4           # NaN columns between the three parts of a row of Z, and behind the last
GAP = 16           # elements of NaN between two layers in their buffer


# ---------------------------------------------------------------------------------------------------------- (a) the C entry
def _layers(vals, dev, ldx=None, x_gap=0, shift=None):
    """``vals`` [n, B, C, Dl] as n views [B, C, Dl] into ONE NaN buffer: rows ``ldx`` apart, batches ``C * ldx + x_gap``, layers
    ``GAP`` or more NaN apart (a multiple of 8 elements: every layer keeps the buffer's alignment), layer ``shift`` one element
    further; NaN behind the last layer."""
    n, B, C, Dl = vals.shape
    ldx = Dl if ldx is None else ldx
    x_batch = C * ldx + x_gap
    step = (B * x_batch + GAP + 7) // 8 * 8
    buf = torch.full((n * step + 8,), float("nan"), dtype=vals.dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    views = []
    for l in range(n):
        v = buf.as_strided((B, C, Dl), (x_batch, ldx, 1), l * step + (1 if l == shift else 0))
        v.copy_(vals[l])
        views.append(v)
    return views, x_batch, ldx


def _z(dev, B, W, parts):
    z_section = W + ZGAP
    ldz = W + (parts - 1) * z_section + ZGAP
    buf = torch.full((GUARD + B * ldz + GUARD,), float("nan"), dtype=torch.float32, device=dev)
    inside = torch.zeros_like(buf, dtype=torch.bool)
    for p in range(parts):
        inside.as_strided((B, W), (ldz, 1), GUARD + p * z_section).fill_(True)
    return buf, inside, ldz, z_section


def _call(pkg, dev, ad, layers, x_batch, ldx, anchor, length, sides, vector, bf16):
    """Two calls of the entry into two NaN buffers -> Z [B, parts * W] (the parts gathered), after the checks on what was not to
    be written and on the form."""
    from ed_gated_gcn_amd import _capi
    lib = pkg.load_library()
    B, R, C = ad.shape
    n, Dl = len(layers), layers[0].shape[2]
    W, parts = n * Dl, 3 if sides else 1
    ptrs = (ctypes.c_void_p * n)(*[v.data_ptr() for v in layers])
    out = []
    for _ in range(2):
        buf, inside, ldz, z_section = _z(dev, B, W, parts)
        z0 = ctypes.c_void_p(buf.data_ptr() + GUARD * 4)
        args = [_capi.ptr(ad), ad.stride(0), ad.stride(1), ad.stride(2), ptrs, n, int(bf16), x_batch, ldx, _capi.ptr(anchor),
                _capi.ptr(length) if sides else None, int(sides), z0, ldz, z_section if sides else 0, B, R, C, Dl]
        assert lib.ggcn_anchor_pool_layers_form(*args) == int(vector), lib.ggcn_last_error()
        with torch.cuda.device(dev):
            _capi.check(lib.ggcn_anchor_pool_layers(*args, _capi.stream_of(dev)), NEW)
        out.append(buf)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[0][~inside]).all()), "a guard band, a gap or a pad column was written"
    assert torch.equal(out[0].view(torch.int32), out[1].view(torch.int32)), "two calls, different bits"
    return torch.cat([out[0].as_strided((B, W), (ldz, 1), GUARD + p * z_section) for p in range(parts)], 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("case", ar.CASES, ids=ar.CASE_IDS)
def test_c_entry_on_every_case(pkg, dev, case, dtype):
    bf16 = dtype == torch.bfloat16
    a, vals, anchor, length = ar.build(case, dtype)
    B, T, W = case.B, case.T, case.n * case.Dl
    layers, x_batch, ldx = _layers(vals.to(dev), dev, **case.layout)
    ad = sc.on_device(a, dev)
    assert ad.stride() == a.stride() and ad.is_contiguous() != case.strided
    an, ln = anchor.to(dev), length.to(dev)
    z = _call(pkg, dev, ad, layers, x_batch, ldx, an, ln, True, case.vector, bf16)
    alone = _call(pkg, dev, ad, layers, x_batch, ldx, an, None, False, case.vector, bf16)
    assert torch.equal(alone.view(torch.int32), z[:, :W].view(torch.int32)), "without sides: the anchor part, the same bits"
    # (1) the statement on the words subword_pool_layers pools
    words = pkg.subword_pool_layers(ad, layers)
    want = ar.statement(words.float().cpu().numpy(), anchor.numpy(), length.numpy())
    got = z.cpu().numpy()
    assert np.array_equal(got, want, equal_nan=True), "%d elements differ from the statement" % int((got != want).sum())
    if case.values == "nan":
        assert np.isnan(got).any() and not np.isnan(got).all()
    else:
        assert not np.isnan(got).any()
    # (2) the anchor columns: the one-row transform
    a_clamped = torch.from_numpy(ar.clamp(anchor.numpy(), None, T)[0]).to(dev)
    one_row = ad[torch.arange(B, device=dev), a_clamped][:, None]
    row = pkg.subword_pool_layers(one_row, layers)[:, 0].float()
    assert torch.equal(z[:, :W].view(torch.int32), row.view(torch.int32))
    # (3) float64
    ref, bound = ar.ref64_and_bound(a, [vals[l] for l in range(case.n)], anchor.numpy(), length.numpy(), bf16)
    ar.assert_within(got, ref, bound, "%s %s" % (case.name, DTYPE_IDS[bf16]))
    if case.values in ("negative", "tiny"):
        assert not got[:, W:].any(), "both sides: exact zeros"


# ----------------------------------------------------------------------------------------------------- (b) the Python function
def _operands(dev, dtype, B, T, L, Dl, n, seed=0):
    rng = np.random.default_rng(seed)
    full = torch.from_numpy(sc.transform_like_reference(B, T, L, rng, T + 3, L + 5)).to(dev)
    layers = [torch.from_numpy(rng.standard_normal((B, L, Dl)).astype(np.float32)).to(dev, dtype) for _ in range(n)]
    anchor = torch.from_numpy(rng.integers(0, T, size=B)).to(dev)
    length = torch.from_numpy(rng.integers(1, T + 1, size=B)).to(dev)
    return full[:, :T, :L], layers, anchor, length


def _composed(pkg, transform, layers, anchor, length, sides):
    v = pkg.subword_pool_layers(transform, layers)
    if not sides:
        return pkg.anchor_pool_formula(v, anchor, sides=False)
    row, pooled = pkg.anchor_pool_formula(v, anchor, length)
    return torch.cat((row.float(), pooled), 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("Dl,n", [(768, 12), (768, 4), (37, 3)], ids=["768x12", "768x4", "37x3"])
def test_python_equals_the_composed_path_in_one_launch(pkg, dev, monkeypatch, Dl, n, dtype):
    transform, layers, anchor, length = _operands(dev, dtype, 5, 7, 40, Dl, n)
    assert not transform.is_contiguous()
    calls = count_calls(monkeypatch, ENTRIES)
    for sides in (True, False):
        want = _composed(pkg, transform, layers, anchor, length, sides)
        before = dict(calls)
        got = pkg.anchor_pool_layers(transform, tuple(layers) if sides else layers, anchor, length if sides else None, sides=sides)
        assert {k: calls[k] - before[k] for k in calls} == {NEW: 1, LAYERS: 0, OLD: 0, OLD_BF16: 0}
        assert got.dtype == (torch.float32 if sides else dtype) and tuple(got.shape) == (5, (3 if sides else 1) * n * Dl)
        assert got.is_contiguous() and torch.equal(got, want), "%d elements differ" % int((got != want).sum())


def test_seventeen_layers_take_two_launches(pkg, dev, monkeypatch):
    transform, layers, anchor, length = _operands(dev, torch.float32, 3, 5, 20, 64, 17)
    want = _composed(pkg, transform, layers, anchor, length, True)
    calls = count_calls(monkeypatch, ENTRIES)
    got = pkg.anchor_pool_layers(transform, layers, anchor, length)
    assert calls == {NEW: 2, LAYERS: 0, OLD: 0, OLD_BF16: 0}
    assert torch.equal(got, want)
    assert torch.equal(pkg.anchor_pool_layers(transform, layers, anchor, sides=False), want[:, :17 * 64]) and calls[NEW] == 4


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_a_sentence_alone_gives_the_bits_it_gives_in_a_batch(pkg, dev, dtype):
    transform, layers, anchor, length = _operands(dev, dtype, 6, 7, 40, 260, 3, seed=4)
    batch = pkg.anchor_pool_layers(transform, layers, anchor, length)
    for b in (0, 3, 5):
        one = pkg.anchor_pool_layers(transform[b:b + 1], [x[b:b + 1] for x in layers], anchor[b:b + 1], length[b:b + 1])
        assert torch.equal(one.view(torch.int32), batch[b:b + 1].view(torch.int32)), b


def test_layers_with_differing_strides_are_copied(pkg, dev):
    transform, layers, anchor, length = _operands(dev, torch.float32, 2, 5, 20, 64, 3)
    want = pkg.anchor_pool_layers(transform, layers, anchor, length)
    turned = layers[2].transpose(1, 2).contiguous().transpose(1, 2)           # the feature stride is not 1
    assert turned.stride(2) != 1
    assert torch.equal(pkg.anchor_pool_layers(transform, [layers[0], layers[1], turned], anchor, length), want)
    noncontig = torch.stack([anchor, anchor], 1)[:, 0]
    assert not noncontig.is_contiguous() and torch.equal(pkg.anchor_pool_layers(transform, layers, noncontig, length), want)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("B,L,D", [(0, 5, 8), (2, 0, 8), (2, 5, 0), (0, 0, 0)], ids=["B0", "L0", "D0", "all0"])
def test_empty_operands_make_no_launch(pkg, dev, monkeypatch, B, L, D, dtype):
    a = torch.ones(B, 3, L, device=dev)
    layers = [torch.ones(B, L, D, device=dev, dtype=dtype) for _ in range(3)]
    anchor, length = torch.zeros(B, dtype=torch.int64, device=dev), torch.full((B,), 3, dtype=torch.int64, device=dev)
    calls = count_calls(monkeypatch, ENTRIES)
    z = pkg.anchor_pool_layers(a, layers, anchor, length)
    assert tuple(z.shape) == (B, 9 * D) and z.dtype == torch.float32 and z.device == a.device and not bool(z.any())
    z = pkg.anchor_pool_layers(a, layers, anchor, sides=False)
    assert tuple(z.shape) == (B, 3 * D) and z.dtype == dtype and not bool(z.any())
    assert calls == {NEW: 0, LAYERS: 0, OLD: 0, OLD_BF16: 0}


# ------------------------------------------------------------------------------------------------------- (c) the classifiers
CLASSIFIERS = [("AnchorEventDetector", 12), ("DynamicMultiPoolEventDetector", 4)]
CLS_IDS = [c[0] for c in CLASSIFIERS]
REL = 2e-4         # the project's gradient gate (oracle/gates.py close32)


class _Bert(torch.nn.Module):
    """Stands in for a frozen encoder: twelve seeded [B,L,768] outputs, none of which requires grad."""

    def __init__(self, B, L, dev, dtype=torch.float32, seed=1):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        self.outputs = [torch.randn(B, L, 768, generator=gen).to(dev, dtype) for _ in range(12)]
        self.pooled = torch.zeros(B, 768, device=dev)

    def forward(self, ids_, seg, output_all_encoded_layers=True):
        assert tuple(ids_.shape) == tuple(self.outputs[0].shape[:2])
        return list(self.outputs), self.pooled


def _model(pkg, dev, cls_name, n_layer, ncls, bert, on, dropout=0.0):
    opt = types.SimpleNamespace(dropout=dropout, polarities_dim=ncls, device=dev, n_layer=n_layer, bert_dim=768, hidden_dim=128,
                                ggcn_anchor_pool=on)
    m = getattr(pkg, cls_name)(bert, opt)
    assert m.anchor_pool is on
    gen = torch.Generator().manual_seed(0)
    for p in m.parameters():
        if p.dim() > 1:
            torch.nn.init.xavier_uniform_(p, generator=gen)
        else:
            torch.nn.init.uniform_(p, -0.05, 0.05, generator=gen)
    return m.to(dev)


def _pair(pkg, dev, cls, monkeypatch, dtype=torch.float32, dropout=0.0):
    monkeypatch.delenv("GGCN_ANCHOR_POOL", raising=False)
    cls_name, n_layer = cls
    inputs, ncls = classifier_batch(dev)
    B, L = inputs["sentence_length"].shape[0], int(inputs["cls_text_sep_length"].max())
    off = _model(pkg, dev, cls_name, n_layer, ncls, _Bert(B, L, dev, dtype), False, dropout)
    on = _model(pkg, dev, cls_name, n_layer, ncls, _Bert(B, L, dev, dtype), True, dropout)
    return inputs, off, on


def _tail(out, cls_name):
    assert out[1:] == ((0, 0, None) if cls_name == "AnchorEventDetector" else (0.0, 0.0, 0.0))


@pytest.mark.parametrize("cls", CLASSIFIERS, ids=CLS_IDS)
def test_classifier_eval_with_the_option_equals_without(pkg, dev, cls, monkeypatch):
    inputs, off, on = _pair(pkg, dev, cls, monkeypatch)
    calls = count_calls(monkeypatch, ENTRIES)
    with torch.no_grad():
        ref = off.eval()(inputs)
        assert calls == {NEW: 0, LAYERS: 1, OLD: 0, OLD_BF16: 0}, "the option is off: the composed path"
        got = on.eval()(inputs)
    torch.cuda.synchronize()
    assert calls == {NEW: 1, LAYERS: 1, OLD: 0, OLD_BF16: 0}, "one launch of the new entry"
    assert tuple(got[0].shape) == (8, 34) and torch.equal(got[0], ref[0]), "%d logits differ" % int((got[0] != ref[0]).sum())
    _tail(got, cls[0]), _tail(ref, cls[0])


@pytest.mark.parametrize("cls", CLASSIFIERS, ids=CLS_IDS)
def test_classifier_training_step_with_the_option_equals_without(pkg, dev, cls, monkeypatch):
    inputs, off, on = _pair(pkg, dev, cls, monkeypatch, dropout=0.5)
    calls = count_calls(monkeypatch, ENTRIES)
    logits = []
    for m in (off, on):
        torch.manual_seed(5)
        m.train()
        out = m(inputs)
        out[0].square().sum().backward()
        logits.append(out[0])
    torch.cuda.synchronize()
    assert calls == {NEW: 1, LAYERS: 1, OLD: 0, OLD_BF16: 0}, "BERT is frozen: no backward launch on either path"
    assert torch.equal(logits[1], logits[0]), "%d logits differ" % int((logits[1] != logits[0]).sum())
    for (name, p), (_, q) in zip(on.named_parameters(), off.named_parameters()):
        assert p.grad is not None and float(q.grad.abs().max()) > 0
        gates.close32(p.grad, q.grad, "%s d %s" % (cls[0], name), REL)


@pytest.mark.parametrize("cls", CLASSIFIERS, ids=CLS_IDS)
def test_classifier_under_bf16_autocast(pkg, dev, cls, monkeypatch):
    inputs, off, on = _pair(pkg, dev, cls, monkeypatch, dtype=torch.bfloat16)
    calls = count_calls(monkeypatch, ENTRIES)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        ref = off.eval()(inputs)
        got = on.eval()(inputs)
    torch.cuda.synchronize()
    assert calls == {NEW: 1, LAYERS: 1, OLD: 0, OLD_BF16: 0}
    assert got[0].dtype == ref[0].dtype and bool(torch.isfinite(got[0].float()).all())
    assert torch.equal(got[0], ref[0]), "%d logits differ" % int((got[0] != ref[0]).sum())


@pytest.mark.parametrize("cls", CLASSIFIERS, ids=CLS_IDS)
def test_captured_eval_forward_replays_the_same_bits(pkg, dev, cls, monkeypatch):
    """The entry only enqueues: anchor and length are read by the kernel, the layers' pointers travel in its argument block.  The
    two length vectors the forward reads on the host stay on the host (pinned: the copy of ``sentence_length`` to the device is
    captured), so nothing in the captured region synchronises; a replay on new layer values gives the bits of an eager forward."""
    inputs, off, on = _pair(pkg, dev, cls, monkeypatch)
    del off
    inputs["sentence_length"] = inputs["sentence_length"].cpu().pin_memory()
    inputs["cls_text_sep_length"] = inputs["cls_text_sep_length"].cpu()
    on.eval()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(2):          # fills the allocator before capture
            on(inputs)
    torch.cuda.current_stream(dev).wait_stream(side)
    calls = count_calls(monkeypatch, ENTRIES)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        out = on(inputs)
    assert calls == {NEW: 1, LAYERS: 0, OLD: 0, OLD_BF16: 0}
    gen = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for x in on.bert.outputs:
            x.copy_(torch.randn(x.shape, generator=gen))
        ref = on(inputs)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], ref[0]), "%d logits differ" % int((out[0] != ref[0]).sum())
