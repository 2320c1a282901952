"""Sub-word pooling straight from BERT's layer list (``ggcn_subword_pool_layers``, ``pooling.subword_pool_layers``, the
classifier's ``pool_layers``) on the GPU.

(a) the C entry, bit for bit what n calls of ``ggcn_subword_pool`` / ``_bf16`` write into the same column ranges: every layer a
    view into a NaN buffer, Y between NaN guard bands with NaN pad columns, both forms (the form is asked of
    ``ggcn_subword_pool_layers_form``, never assumed from the shape), twice with the same bits, and per element inside the bound
    of oracle/subword_pool_cases.py against float64 on the concatenated operand.
(b) the Python function against ``subword_pool(transform, torch.cat(layers, -1))``: values, launches, strides, empty operands and
    gradients, ``torch.equal`` throughout.
(c) the three classifiers with the option on against off, in inference, in a training step, under bf16 autocast and captured.
"""
import ctypes
import types

import numpy as np
import pytest
import torch

from oracle import subword_pool_cases as sc
from oracle.gpu_support import classifier_batch, count_calls, dev, pkg  # noqa: F401

pytestmark = pytest.mark.gpu

NEW, OLD, OLD_BF16 = "ggcn_subword_pool_layers", "ggcn_subword_pool", "ggcn_subword_pool_bf16"
ENTRIES = (NEW, OLD, OLD_BF16)
DTYPES = (torch.float32, torch.bfloat16)
DTYPE_IDS = ("f32", "bf16")
GUARD = 8          # elements of NaN on either side of Y: 32 bytes of float, 16 of bfloat16 -- the view keeps its alignment
YPAD = 4           # NaN columns behind the n * Dl of every row of Y
GAP = 16           # elements of NaN between two layers in their buffer


# ---------------------------------------------------------------------------------------------------------- (a) the C entry
def _transform(B, R, C, seed, full=()):
    """[B, R, C] with row 1 empty in every batch and the rows ``full`` without a zero."""
    rng = np.random.default_rng(seed)
    return torch.from_numpy(sc.dense_transform(B, R, C, 0.5, rng, scale=sc.value_scale(C), empty=(1,), full=full))


def _layers(vals, dev, dtype, ldx, x_gap, shift):
    """``vals`` [n, B, C, Dl] as n views [B, C, Dl] into ONE NaN buffer: rows ``ldx`` apart, batches ``C * ldx + x_gap``, layers
    ``GAP`` or more NaN apart (a multiple of 8 elements, so that every layer keeps the buffer's alignment), layer ``shift`` one
    element further."""
    n, B, C, Dl = vals.shape
    x_batch = C * ldx + x_gap
    step = (B * x_batch + GAP + 7) // 8 * 8
    buf = torch.full((n * step + 8,), float("nan"), dtype=dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    views = []
    for l in range(n):
        v = buf.as_strided((B, C, Dl), (x_batch, ldx, 1), l * step + (1 if l == shift else 0))
        v.copy_(vals[l])
        views.append(v)
    assert int((~torch.isnan(buf)).sum()) == vals.numel()
    return views, x_batch


def _y(dev, dtype, B, R, n, Dl):
    ldy = n * Dl + YPAD
    y_batch = R * ldy + 8
    buf = torch.full((GUARD + B * y_batch + GUARD,), float("nan"), dtype=dtype, device=dev)
    return buf, buf.as_strided((B, R, n * Dl), (y_batch, ldy, 1), GUARD), y_batch, ldy


def _run_c_case(pkg, dev, dtype, a, Dl, n, vector, ldx=None, x_gap=0, shift=None, empty_row=1):
    """One call of the new entry and n of the old into two identical NaN buffers: the same bits everywhere (the guard bands and
    the pads included, which are still NaN), the form ``vector`` as ``..._form`` answers, the same bits on a second call, exact
    zeros from the empty row, and every element inside the float64 bound."""
    from ed_gated_gcn_amd import _capi
    bf16 = dtype == torch.bfloat16
    B, R, C = a.shape
    ldx = Dl if ldx is None else ldx
    rng = np.random.default_rng(1000 * n + Dl)
    vals = torch.from_numpy(rng.standard_normal((n, B, C, Dl)).astype(np.float32)).to(dtype)
    layers, x_batch = _layers(vals.to(dev), dev, dtype, ldx, x_gap, shift)
    ad = sc.on_device(a, dev)           # the view as it lies in its buffer: shape, strides and offset survive
    assert ad.stride() == a.stride()
    lib = pkg.load_library()
    ptrs = (ctypes.c_void_p * n)(*[v.data_ptr() for v in layers])
    bits = torch.int16 if bf16 else torch.int32
    got = []
    for _ in range(2):
        ybuf, y, y_batch, ldy = _y(dev, dtype, B, R, n, Dl)
        args = [_capi.ptr(ad), ad.stride(0), ad.stride(1), ad.stride(2), ptrs, n, int(bf16), x_batch, ldx, _capi.ptr(y), y_batch, ldy,
                B, R, C, Dl]
        assert lib.ggcn_subword_pool_layers_form(*args) == int(vector)
        with torch.cuda.device(dev):
            _capi.check(lib.ggcn_subword_pool_layers(*args, _capi.stream_of(dev)), NEW)
        got.append((ybuf, y))
    ybuf1, y1, _, _ = _y(dev, dtype, B, R, n, Dl)
    one = getattr(lib, OLD_BF16 if bf16 else OLD)
    with torch.cuda.device(dev):
        for l in range(n):
            col = ctypes.c_void_p(y1.data_ptr() + l * Dl * y1.element_size())
            _capi.check(one(_capi.ptr(ad), ad.stride(0), ad.stride(1), ad.stride(2), _capi.ptr(layers[l]), x_batch, ldx, col, y_batch, ldy,
                            B, R, C, Dl, _capi.stream_of(dev)), OLD)
    torch.cuda.synchronize()
    (ybuf, y), (ybuf2, _) = got
    inside = torch.zeros_like(ybuf, dtype=torch.bool)
    inside.as_strided(tuple(y.shape), tuple(y.stride()), GUARD).fill_(True)
    assert int(inside.sum()) == B * R * n * Dl
    assert bool(torch.isnan(ybuf[~inside]).all()), "a guard band or a pad column was written"
    assert not bool(torch.isnan(y).any()), "NaN in the result"
    assert torch.equal(ybuf.view(bits), ybuf1.view(bits)), \
        "%d elements differ from the per-layer calls" % int((ybuf.view(bits) != ybuf1.view(bits)).sum())
    assert torch.equal(ybuf.view(bits), ybuf2.view(bits)), "two calls, different bits"
    if empty_row is not None:
        assert float(y[:, empty_row].float().abs().max()) == 0.0, "the empty row: exact zeros in every layer's columns"
    cat = torch.cat([vals[l] for l in range(n)], dim=-1)
    err = (y.double().cpu() - sc.ref64(a, cat)).abs()
    bound = sc.bound(a, cat, bf16=bf16)
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print("  Dl=%d n=%d %s: max err / bound %.3f (max err %.3g)" % (Dl, n, DTYPE_IDS[bf16], ratio, float(err.max())))
    assert not bool((err > bound).any()), "%d elements outside the bound, the worst %.3f times it" % (int((err > bound).sum()), ratio)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("n", (1, 2, 12, 16))
@pytest.mark.parametrize("Dl", (4, 768, 1020, 1024, 1028))
def test_vector_form_equals_per_layer_calls(pkg, dev, Dl, n, dtype):
    _run_c_case(pkg, dev, dtype, _transform(2, 3, 9, Dl + n), Dl, n, vector=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("n", (1, 3))
@pytest.mark.parametrize("Dl", (1, 3, 257, 1025))
def test_scalar_form_equals_per_layer_calls(pkg, dev, Dl, n, dtype):
    _run_c_case(pkg, dev, dtype, _transform(2, 3, 9, Dl + n), Dl, n, vector=False)


# (id, Dl, n, the form, what differs)
LAYOUTS = (("scalar-by-one-shifted-layer", 768, 12, False, dict(shift=5)),
           ("scalar-by-ldx", 768, 12, False, dict(ldx=769)),
           ("scalar-by-xbatch", 768, 12, False, dict(x_gap=2)),
           ("vector-padded-rows-and-batch-gap", 768, 12, True, dict(ldx=776, x_gap=8)),
           ("scalar-padded-rows-and-batch-gap", 257, 3, False, dict(ldx=265, x_gap=8)))


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("layout", LAYOUTS, ids=[c[0] for c in LAYOUTS])
def test_layouts_equal_per_layer_calls(pkg, dev, layout, dtype):
    _, Dl, n, vector, kw = layout
    _run_c_case(pkg, dev, dtype, _transform(2, 3, 9, 77), Dl, n, vector, **kw)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("C", (255, 256, 257, 2048))
def test_compaction_rounds_equal_per_layer_calls(pkg, dev, C, dtype):
    """One, one, two and eight rounds of the compaction; at the capacity one row holds 2048 non-zeros."""
    B = 1 if C == sc.MAX_COLS else 2
    a = _transform(B, 3, C, C, full=(0,) if C == sc.MAX_COLS else ())
    if C == sc.MAX_COLS:
        assert int((a[0, 0] != 0).sum()) == sc.MAX_COLS
    _run_c_case(pkg, dev, dtype, a, 8, 3, vector=True)
    _run_c_case(pkg, dev, dtype, a, 5, 2, vector=False)


def test_a_strided_transform_at_the_c_entry(pkg, dev):
    """A with element strides (the reference's slice of a padded buffer), reference-like values."""
    rng = np.random.default_rng(5)
    full = torch.from_numpy(sc.transform_like_reference(3, 7, 40, rng, 10, 45))
    a = full[:, :7, :40]
    assert not a.is_contiguous()
    _run_c_case(pkg, dev, torch.float32, a, 768, 12, vector=True, empty_row=None)


# ----------------------------------------------------------------------------------------------------- (b) the Python function
def _reference_operands(dev, dtype, B, T, L, Dl, n, seed=0):
    rng = np.random.default_rng(seed)
    full = torch.from_numpy(sc.transform_like_reference(B, T, L, rng, T + 3, L + 5)).to(dev)
    layers = [torch.from_numpy(rng.standard_normal((B, L, Dl)).astype(np.float32)).to(dev, dtype) for _ in range(n)]
    return full, layers


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("Dl,n", [(768, 12), (37, 3), (1028, 1)], ids=["768x12", "37x3", "1028x1"])
def test_python_equals_cat_then_pool(pkg, dev, monkeypatch, Dl, n, dtype):
    full, layers = _reference_operands(dev, dtype, 3, 7, 40, Dl, n)
    calls = count_calls(monkeypatch, ENTRIES)
    for transform in (full[:, :7, :40].contiguous(), full[:, :7, :40]):       # contiguous, and the reference's sliced view
        want = pkg.subword_pool(transform, torch.cat(layers, -1))
        for arg in (layers, tuple(layers)):
            got = pkg.subword_pool_layers(transform, arg)
            assert got.dtype == dtype and tuple(got.shape) == (3, 7, n * Dl) and got.is_contiguous()
            assert torch.equal(got, want), "%d elements differ" % int((got != want).sum())
    torch.cuda.synchronize()
    assert calls[NEW] == 4 and calls[OLD] + calls[OLD_BF16] == 2


def test_seventeen_layers_take_two_launches(pkg, dev, monkeypatch):
    full, layers = _reference_operands(dev, torch.float32, 2, 5, 20, 64, 17)
    transform = full[:, :5, :20]
    want = pkg.subword_pool(transform, torch.cat(layers, -1))
    calls = count_calls(monkeypatch, ENTRIES)
    got = pkg.subword_pool_layers(transform, layers)
    assert calls == {NEW: 2, OLD: 0, OLD_BF16: 0}
    assert torch.equal(got, want)
    assert torch.equal(pkg.subword_pool_layers(transform, layers[:16]), want[:, :, :16 * 64]) and calls[NEW] == 3


def test_layers_with_differing_strides_are_copied(pkg, dev, monkeypatch):
    full, layers = _reference_operands(dev, torch.float32, 2, 5, 20, 64, 3)
    transform = full[:, :5, :20]
    want = pkg.subword_pool(transform, torch.cat(layers, -1))
    wide = torch.full((2, 20, 70), float("nan"), device=dev)
    wide[:, :, :64] = layers[1]
    turned = layers[2].transpose(1, 2).contiguous().transpose(1, 2)           # the feature stride is not 1
    assert turned.stride(2) != 1 and torch.equal(turned, layers[2])
    calls = count_calls(monkeypatch, ENTRIES)
    for arg in ([layers[0], wide[:, :, :64], layers[2]], [layers[0], layers[1], turned], [turned, turned, turned]):
        want_arg = want if arg[0] is layers[0] else pkg.subword_pool(transform, torch.cat(arg, -1))
        assert torch.equal(pkg.subword_pool_layers(transform, arg), want_arg)
    assert calls[NEW] == 3
    # the same strides in every layer, rows wider than Dl: taken where they lie
    views = [torch.full((2, 20, 72), float("nan"), device=dev) for _ in range(3)]
    for v, x in zip(views, layers):
        v[:, :, :64] = x
    assert torch.equal(pkg.subword_pool_layers(transform, [v[:, :, :64] for v in views]), want) and calls[NEW] == 4


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("B,T,L,D", [(0, 3, 5, 8), (2, 0, 5, 8), (2, 3, 0, 8), (2, 3, 5, 0), (0, 0, 0, 0)],
                         ids=["B0", "T0", "L0", "D0", "all0"])
def test_empty_operands_make_no_launch(pkg, dev, monkeypatch, B, T, L, D, dtype):
    a = torch.ones(B, T, L, device=dev)
    layers = [torch.ones(B, L, D, device=dev, dtype=dtype, requires_grad=True) for _ in range(3)]
    want = torch.bmm(torch.ones(B, T, L, dtype=dtype), torch.ones(B, L, 3 * D, dtype=dtype))
    calls = count_calls(monkeypatch, ENTRIES)
    y = pkg.subword_pool_layers(a, layers)
    assert tuple(y.shape) == (B, T, 3 * D) and y.dtype == dtype and y.device == layers[0].device
    assert torch.equal(y.detach().cpu(), want) and y.requires_grad
    y.sum().backward()
    torch.cuda.synchronize()
    for x in layers:
        assert x.grad is not None and x.grad.shape == x.shape and x.grad.dtype == dtype
        assert torch.equal(x.grad.cpu(), torch.full((B, L, D), float(T), dtype=dtype))
    assert calls == {NEW: 0, OLD: 0, OLD_BF16: 0}


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_gradients_equal_the_cat_form(pkg, dev, monkeypatch, dtype):
    bf16 = dtype == torch.bfloat16
    full, values = _reference_operands(dev, dtype, 3, 7, 40, 768, 12)
    transform = full[:, :7, :40]
    dy = torch.randn(3, 7, 12 * 768 + 3, device=dev, generator=torch.Generator(device=dev).manual_seed(2)).to(dtype)[..., :12 * 768]
    assert not dy.is_contiguous()
    frozen = 4                                                     # one layer wants no gradient
    ours = [v.clone().requires_grad_(l != frozen) for l, v in enumerate(values)]
    theirs = [v.clone().requires_grad_(l != frozen) for l, v in enumerate(values)]
    pkg.subword_pool(transform, torch.cat(theirs, -1)).backward(dy)
    calls = count_calls(monkeypatch, ENTRIES)
    y = pkg.subword_pool_layers(transform, ours)
    assert y.requires_grad and calls[NEW] == 1 and calls[OLD] + calls[OLD_BF16] == 0
    y.backward(dy)
    torch.cuda.synchronize()
    assert calls[NEW] == 1 and calls[OLD_BF16 if bf16 else OLD] == 1 and calls[OLD if bf16 else OLD_BF16] == 0, \
        "the backward is one transposed launch"
    assert transform.grad is None and full.grad is None
    for l, (x, ref) in enumerate(zip(ours, theirs)):
        if l == frozen:
            assert x.grad is None and ref.grad is None
        else:
            assert x.grad.dtype == dtype and torch.equal(x.grad, ref.grad), "layer %d" % l


def test_autograd_launches_only_what_is_needed(pkg, dev, monkeypatch):
    from ed_gated_gcn_amd.pooling import _SubwordPoolLayers
    full, layers = _reference_operands(dev, torch.float32, 2, 5, 20, 64, 3)
    transform = full[:, :5, :20]
    calls = count_calls(monkeypatch, ENTRIES)
    y = pkg.subword_pool_layers(transform, layers)                 # no layer requires a gradient: nothing to go back through
    assert not y.requires_grad and calls[NEW] == 1

    class Ctx:
        saved_tensors = (transform,)
        needs_input_grad = (False, False, False, False)
        width = 64
    assert _SubwordPoolLayers.backward(Ctx, torch.ones_like(y)) == (None,) * 4 and calls[OLD] == 0
    Ctx.needs_input_grad = (False, False, True, False)
    grads = _SubwordPoolLayers.backward(Ctx, torch.ones_like(y))
    assert [g is None for g in grads] == [True, True, False, True] and tuple(grads[2].shape) == (2, 20, 64) and calls[OLD] == 1


# ------------------------------------------------------------------------------------------------------- (c) the classifiers
CLASSIFIERS = ["GatedGCNEventDetector", "GatedGCNEventDetector54", "GCNEventDetectorNoGate"]
OUTPUTS = ("logits", "xy", "kl", "scores")


class _Bert(torch.nn.Module):
    """Stands in for the encoder: its twelve [B,L,768] outputs are leaves, so their ``.grad`` is what BERT would receive."""

    def __init__(self, B, L, dev, dtype=torch.float32, seed=1):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        self.outputs = [torch.randn(B, L, 768, generator=gen).to(dev, dtype).requires_grad_(True) for _ in range(12)]
        self.pooled = torch.zeros(B, 768, device=dev)

    def forward(self, ids_, seg, output_all_encoded_layers=True):
        assert tuple(ids_.shape) == tuple(self.outputs[0].shape[:2])
        return list(self.outputs), self.pooled


def _model(pkg, dev, cls_name, ncls, bert, pool_layers, **opt):
    opt = types.SimpleNamespace(dropout=0.0, polarities_dim=ncls, device=dev, ggcn_pool_layers=pool_layers, **opt)
    m = getattr(pkg, cls_name)(bert, opt)
    assert m.pool_layers is pool_layers
    gen = torch.Generator().manual_seed(0)
    for p in m.parameters():
        if p.dim() > 1:
            torch.nn.init.xavier_uniform_(p, generator=gen)
        else:
            torch.nn.init.uniform_(p, -0.05, 0.05, generator=gen)
    return m.to(dev)


def _pair(pkg, dev, cls_name, monkeypatch, dtype=torch.float32, **opt):
    monkeypatch.delenv("GGCN_POOL_LAYERS", raising=False)
    inputs, ncls = classifier_batch(dev)
    B, L = inputs["sentence_length"].shape[0], int(inputs["cls_text_sep_length"].max())
    off = _model(pkg, dev, cls_name, ncls, _Bert(B, L, dev, dtype), False, **opt)
    on = _model(pkg, dev, cls_name, ncls, _Bert(B, L, dev, dtype), True, **opt)
    assert sorted(on.state_dict()) == sorted(off.state_dict())
    return inputs, off, on


def _same(got, ref, what):
    for g, r, name in zip(got, ref, OUTPUTS):
        if torch.is_tensor(r):
            assert torch.equal(g, r), "%s %s: %d elements differ" % (what, name, int((g != r).sum()))
        else:
            assert g == r, "%s %s" % (what, name)        # (the gateless variant: xy = 0.0)


@pytest.mark.parametrize("cls_name", CLASSIFIERS)
def test_classifier_inference_with_the_option_equals_without(pkg, dev, cls_name, monkeypatch):
    inputs, off, on = _pair(pkg, dev, cls_name, monkeypatch)
    calls = count_calls(monkeypatch, ENTRIES)
    with torch.no_grad():
        ref = off.eval()(inputs)
        assert calls == {NEW: 0, OLD: 1, OLD_BF16: 0}, "the option is off: torch.cat and subword_pool"
        got = on.eval()(inputs)
    torch.cuda.synchronize()
    assert calls == {NEW: 1, OLD: 1, OLD_BF16: 0}, "one launch of the new entry, none of the old"
    _same(got, ref, cls_name)


@pytest.mark.parametrize("cls_name", CLASSIFIERS)
def test_classifier_training_step_with_the_option_equals_without(pkg, dev, cls_name, monkeypatch):
    inputs, off, on = _pair(pkg, dev, cls_name, monkeypatch)
    calls = count_calls(monkeypatch, ENTRIES)
    results = []
    for m in (off, on):
        torch.manual_seed(5)
        m.train()
        out = m(inputs)
        loss = out[0].sum() + out[2] + (out[1] if torch.is_tensor(out[1]) else 0.0)
        loss.backward()
        results.append((out, loss))
    torch.cuda.synchronize()
    assert calls == {NEW: 1, OLD: 3, OLD_BF16: 0}, "off: forward and backward; on: the new forward and the same backward launch"
    (ref, ref_loss), (got, got_loss) = results
    assert torch.equal(got_loss, ref_loss)
    _same(got, ref, cls_name)
    for l, (x, r) in enumerate(zip(on.bert.outputs, off.bert.outputs)):
        assert x.grad is not None and torch.equal(x.grad, r.grad), "layer %d: %d elements differ" % (l, int((x.grad != r.grad).sum()))


@pytest.mark.parametrize("cls_name", CLASSIFIERS)
def test_classifier_under_bf16_autocast(pkg, dev, cls_name, monkeypatch):
    inputs, off, on = _pair(pkg, dev, cls_name, monkeypatch, dtype=torch.bfloat16)
    calls = count_calls(monkeypatch, ENTRIES)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        got = on.eval()(inputs)
    torch.cuda.synchronize()
    assert calls == {NEW: 1, OLD: 0, OLD_BF16: 0}
    for g, name in zip(got, OUTPUTS):
        if torch.is_tensor(g):
            assert bool(torch.isfinite(g.float()).all()), name


def test_captured_eval_forward_replays_the_same_bits(pkg, dev, monkeypatch):
    """The new entry only enqueues (the layers' pointers travel in the kernel's argument block): the eval forward captures into a
    hipGraph and a replay on new layer values gives the bits of an eager forward.  What the forward reads on the host (the two
    length vectors) stays on the host, the graph arrives as a CSR built once, the precision is named and the BiLSTM is the
    project's own: nothing in the captured region synchronises."""
    inputs, off, on = _pair(pkg, dev, "GatedGCNEventDetector", monkeypatch, ggcn_precision="bf16x3", ggcn_hip_lstm=True)
    del off
    T = int(inputs["sentence_length"].max())
    inputs["sentence_length"], inputs["cls_text_sep_length"] = inputs["sentence_length"].cpu(), inputs["cls_text_sep_length"].cpu()
    inputs["dependency_graph"] = pkg.BatchedCSR.from_dense(inputs["dependency_graph"][:, :T, :T])
    on.eval()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(2):          # packs weights, builds the graph operands, fills the allocator before capture
            on(inputs)
    torch.cuda.current_stream(dev).wait_stream(side)
    calls = count_calls(monkeypatch, ENTRIES)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        out = on(inputs)
    assert calls == {NEW: 1, OLD: 0, OLD_BF16: 0}
    gen = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for x in on.bert.outputs:
            x.copy_(torch.randn(x.shape, generator=gen))
        ref = on(inputs)
    graph.replay()
    torch.cuda.synchronize()
    _same(out, ref, "replay")
