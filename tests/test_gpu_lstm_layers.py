"""The BiLSTM projection straight from BERT's layer list (``ggcn_linear_pooled_layers``, ``recurrent.bilstm_layers``, the
classifier's ``lstm_layers``) on the GPU.

(a) the C entry against the composed pair -- ``ggcn_subword_pool_layers`` into a pooled buffer, then ``ggcn_linear`` (bf16x3) on
    the same weight image -- on raw bits (a propagated NaN counts as equal), Y between NaN guard bands with NaN pad columns, every
    layer a view into a NaN buffer, NaN in every sub-word row that no word selects; one case also per element against float64.
(b) ``bilstm_layers`` against ``bilstm(subword_pool_layers(...))``: ``torch.equal``, the launches, strides, empty operands, the
    raise on a wanted gradient, and the allocation high-water mark (the pooled words are never allocated).
(c) the three classifiers with the option on: inference against ``pool_layers`` + ``hip_lstm`` (same bits) and against all
    options off (the forward gate), a training step and bf16 autocast (the path is not taken), and a captured eval forward.
"""
import ctypes
import types

import numpy as np
import pytest
import torch

import linear_ref as lr
from oracle import subword_pool_cases as sc
from oracle.gates import gate
from oracle.gpu_support import classifier_batch, count_calls, dev, pkg  # noqa: F401

pytestmark = pytest.mark.gpu

NEW, POOL_LAYERS, POOL, LINEAR, RECURRENCE = ("ggcn_linear_pooled_layers", "ggcn_subword_pool_layers", "ggcn_subword_pool",
                                              "ggcn_linear", "ggcn_bilstm_recurrence")
ENTRIES = (NEW, POOL_LAYERS, POOL, "ggcn_subword_pool_bf16", LINEAR, RECURRENCE, "ggcn_anchor_pool_layers")
GUARD = 8          # floats of NaN on either side of Y: the view keeps its 16-byte alignment
YPAD = 4           # NaN columns behind the F of every row of Y
GAP = 16           # floats of NaN between two layers in their buffer
U = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------- (a) the C entry
def _layers(vals, dev, ldx, x_gap):
    """``vals`` [n, B, C, Dl] as n views [B, C, Dl] into ONE NaN buffer: rows ``ldx`` apart, batches ``C * ldx + x_gap``, layers
    ``GAP`` or more NaN apart (a multiple of 8 floats: every layer keeps the buffer's 16-byte alignment)."""
    n, B, C, Dl = vals.shape
    x_batch = C * ldx + x_gap
    step = (B * x_batch + GAP + 7) // 8 * 8
    buf = torch.full((n * step + 8,), float("nan"), dtype=torch.float32, device=dev)
    views = []
    for l in range(n):
        v = buf.as_strided((B, C, Dl), (x_batch, ldx, 1), l * step)
        v.copy_(vals[l])
        views.append(v)
    return views, x_batch


def _y(dev, M, F):
    ldy = F + YPAD
    buf = torch.full((GUARD + M * ldy + GUARD,), float("nan"), dtype=torch.float32, device=dev)
    return buf, buf.as_strided((M, F), (ldy, 1), GUARD), ldy


def _weight(K, F, seed):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.uniform(-1.0, 1.0, size=(K, F)).astype(np.float32) / np.float32(np.sqrt(K)))


def _run_c_case(pkg, dev, a, Dl, n, F, ldx=None, x_gap=0, nan_selected=None, float64=False):
    """One call of the new entry and the composed pair into two identical NaN buffers: the same bits everywhere (the guard bands
    and pad columns included, which are still NaN) and no NaN in the result -- or, with ``nan_selected = (b, c)`` (one selected
    sub-word row made NaN), NaN in exactly the rows of Y in which the composed pair has it.  Returns Y."""
    from ed_gated_gcn_amd import _capi, hostops
    B, R, C = a.shape
    M, K = B * R, n * Dl
    ldx = Dl if ldx is None else ldx
    rng = np.random.default_rng(1000 * n + Dl + F)
    vals = torch.from_numpy(rng.standard_normal((n, B, C, Dl)).astype(np.float32))
    unselected = ~(a != 0).any(dim=1)                                  # [B, C]: sub-word rows that no word selects
    vals[:, unselected] = float("nan")
    if nan_selected is not None:
        b, c = nan_selected
        assert not bool(unselected[b, c])
        vals[n // 2, b, c, Dl // 2] = float("nan")
    layers, x_batch = _layers(vals.to(dev), dev, ldx, x_gap)
    ad = sc.on_device(a, dev)                                          # the view as it lies in its buffer
    assert ad.stride() == a.stride()
    w = _weight(K, F, K + F).to(dev)
    lib = pkg.load_library()
    ptrs = (ctypes.c_void_p * n)(*[v.data_ptr() for v in layers])
    head = [_capi.ptr(ad), ad.stride(0), ad.stride(1), ad.stride(2), ptrs, n]
    with torch.cuda.device(dev):
        st = _capi.stream_of(dev)
        pack = hostops.weight_pack(lib, st, w, F, K, F, "bf16x3", False)
        ybuf, y, ldy = _y(dev, M, F)
        args = head + [x_batch, ldx, _capi.ptr(pack), _capi.ptr(y), ldy, B, R, C, Dl, F]
        assert lib.ggcn_linear_pooled_layers_form(*args) == 1, lib.ggcn_last_error().decode()
        _capi.check(lib.ggcn_linear_pooled_layers(*args, st), NEW)
        # the composed pair
        pooled = torch.full((B, R, K), float("nan"), dtype=torch.float32, device=dev)
        _capi.check(lib.ggcn_subword_pool_layers(*head, 0, x_batch, ldx, _capi.ptr(pooled), R * K, K, B, R, C, Dl, st), POOL_LAYERS)
        ybuf1, y1, _ = _y(dev, M, F)
        _capi.check(lib.ggcn_linear(_capi.ptr(pooled), K, None, 0, _capi.ptr(pack), _capi.ptr(y1), ldy, M, K, F, _capi.PREC["bf16x3"], st),
                    LINEAR)
    torch.cuda.synchronize()
    inside = torch.zeros_like(ybuf, dtype=torch.bool)
    inside.as_strided((M, F), (ldy, 1), GUARD).fill_(True)
    assert bool(torch.isnan(ybuf[~inside]).all()), "a guard band or a pad column was written"
    differ = int((ybuf.view(torch.int32) != ybuf1.view(torch.int32)).sum())
    assert differ == 0, "%d elements differ from ggcn_subword_pool_layers + ggcn_linear" % differ
    if nan_selected is None:
        assert not bool(torch.isnan(y).any()), "NaN in the result: a row that no word selects arrived"
    else:
        rows = torch.isnan(y).any(dim=1)
        want = (a[nan_selected[0], :, nan_selected[1]] != 0).nonzero().flatten() + nan_selected[0] * R
        assert rows.nonzero().flatten().tolist() == want.tolist() and want.numel() > 0
    if float64:
        cat = torch.cat([torch.nan_to_num(vals[l], nan=0.0) for l in range(n)], dim=-1).double()
        a64, w64 = a.double(), w.double().cpu()
        ref = (a64 @ cat).reshape(M, K) @ w64
        S = (a64.abs() @ cat.abs()).reshape(M, K) @ w64.abs()
        nmax = int((a != 0).sum(dim=2).max())
        # the pooled value carries (nmax + 1) u of |A||X| (oracle/subword_pool_cases.bound); the bf16x3 product of THAT value is
        # inside linear_ref's gate at this K; both scaled by S = (|A| |X|) |W|
        coef = lr.gate_bx3(1.0, K)
        bound = (coef * (1.0 + (nmax + 1) * U) + (nmax + 1) * U) * S
        err = (y.double().cpu() - ref).abs()
        ratio = float((err / bound.clamp_min(1e-300)).max())
        print("  Dl=%d n=%d F=%d: max err / bound %.3f (max err %.3g)" % (Dl, n, F, ratio, float(err.max())))
        assert not bool((err > bound).any()), "%d elements outside the bound, the worst %.3f times it" % (int((err > bound).sum()), ratio)
    return y


def _reference_transform(B, R, C, seed):
    """Runs of 1/l as data_utils.py:749-766 makes them; every sentence's last word has no sub-word."""
    a = torch.from_numpy(sc.transform_like_reference(B, R, C, np.random.default_rng(seed)))
    a[:, R - 1] = 0.0
    return a


# (Dl, n, B, R, F): Dl = 32, 64, 96 put a layer boundary at every, every second and every third stage; M = B*R = 15, 128, 129 and
# 279 = 9 x 31 (tiles that straddle sentences, a ragged last tile); F below, at and past one 256-column workgroup, and four
SHAPES = [(32, 1, 3, 5, 32), (64, 2, 4, 32, 256), (96, 3, 3, 43, 260), (768, 12, 9, 31, 1024), (32, 16, 9, 31, 260),
          (768, 1, 3, 43, 32), (64, 12, 3, 5, 1024), (96, 16, 4, 32, 256), (32, 3, 4, 32, 1024), (768, 2, 3, 5, 260),
          (64, 3, 9, 31, 32), (96, 12, 3, 43, 256)]


@pytest.mark.parametrize("Dl,n,B,R,F", SHAPES, ids=["Dl%d-n%d-M%d-F%d" % (s[0], s[1], s[2] * s[3], s[4]) for s in SHAPES])
def test_c_entry_equals_the_composed_pair(pkg, dev, Dl, n, B, R, F):
    _run_c_case(pkg, dev, _reference_transform(B, R, 40, Dl + n + F), Dl, n, F)


NNZ = (1, 2, 3, 4, 5, 8, 9, 16, 17, 33, 65)


def _counted_transform(C=70):
    """[2, 13, C]: rows of NNZ non-zeros (negative and unequal weights, scattered columns), a row without any, and one more of
    two; column 0 and the last are selected by no row."""
    rng = np.random.default_rng(4)
    a = np.zeros((2, len(NNZ) + 2, C), dtype=np.float32)
    for b in range(2):
        for r, k in enumerate(NNZ):
            cols = rng.choice(np.arange(1, C - 1), size=k, replace=False)
            a[b, r, cols] = (rng.uniform(0.25, 1.0, size=k) * rng.choice([-1.0, 1.0], size=k)).astype(np.float32)
        a[b, len(NNZ) + 1, [3, C - 2]] = (0.5, -0.25)
    return torch.from_numpy(a)


@pytest.mark.parametrize("Dl,n,F", [(32, 2, 256), (768, 12, 1024)], ids=["Dl32", "Dl768"])
def test_rows_of_every_count_of_non_zeros(pkg, dev, Dl, n, F):
    a = _counted_transform()
    assert sorted(set((a[0] != 0).sum(dim=1).tolist())) == sorted(set(NNZ + (0,)))
    y = _run_c_case(pkg, dev, a, Dl, n, F, float64=(Dl == 32))
    assert float(y[len(NNZ)].abs().max()) == 0.0, "the word without a sub-word: exact zeros"


@pytest.mark.parametrize("C,R", [(300, 3), (2048, 2)], ids=["C300", "C2048"])
def test_fully_dense_rows(pkg, dev, C, R):
    rng = np.random.default_rng(C)
    a = torch.from_numpy(sc.dense_transform(1, R, C, 0.02, rng, scale=sc.value_scale(C), full=(0,)))
    assert int((a[0, 0] != 0).sum()) == C
    _run_c_case(pkg, dev, a, 32, 1 if C == 2048 else 2, 32, float64=True)


def test_the_strided_slice_of_a_larger_buffer(pkg, dev):
    full = torch.from_numpy(sc.transform_like_reference(3, 7, 40, np.random.default_rng(5), 10, 45))
    a = full[:, :7, :40]
    assert not a.is_contiguous()
    _run_c_case(pkg, dev, a, 768, 12, 1024)


@pytest.mark.parametrize("ldx,x_gap", [(776, 0), (768, 8), (100, 12)], ids=["ldx", "batch-gap", "both"])
def test_layer_layouts(pkg, dev, ldx, x_gap):
    Dl = 96 if ldx == 100 else 768
    _run_c_case(pkg, dev, _reference_transform(3, 7, 40, 9), Dl, 3, 260, ldx=ldx, x_gap=x_gap)


def test_a_nan_in_a_selected_row_lands_where_the_composed_pair_puts_it(pkg, dev):
    a = _reference_transform(4, 32, 40, 21)
    b = 2
    c = int((a[b] != 0).any(dim=0).nonzero().flatten()[3])
    _run_c_case(pkg, dev, a, 64, 3, 256, nan_selected=(b, c))


# ----------------------------------------------------------------------------------------------------- (b) bilstm_layers
def _lstm(dev, width, seed=0):
    m = torch.nn.LSTM(width, 128, bidirectional=True, batch_first=True, num_layers=1)
    gen = torch.Generator().manual_seed(seed)
    for p in m.parameters():
        torch.nn.init.uniform_(p, -0.08, 0.08, generator=gen)
        p.requires_grad_(False)
    return m.to(dev)


def _operands(dev, B, T, L, Dl, n, seed=0):
    rng = np.random.default_rng(seed)
    full = torch.from_numpy(sc.transform_like_reference(B, T, L, rng, T + 3, L + 5)).to(dev)
    layers = [torch.from_numpy(rng.standard_normal((B, L, Dl)).astype(np.float32)).to(dev) for _ in range(n)]
    return full, layers


@pytest.mark.parametrize("Dl,n", [(768, 12), (32, 3)], ids=["768x12", "32x3"])
def test_bilstm_layers_equals_the_composed_call(pkg, dev, monkeypatch, Dl, n):
    full, layers = _operands(dev, 5, 31, 64, Dl, n)
    lstm = _lstm(dev, n * Dl)
    with torch.no_grad():
        pkg.bilstm(pkg.subword_pool_layers(full[:, :31, :64], layers), lstm)          # (the weight image is cached from here on)
    calls = count_calls(monkeypatch, ENTRIES)
    for transform in (full[:, :31, :64].contiguous(), full[:, :31, :64]):             # contiguous, and the reference's sliced view
        for arg in (layers, tuple(layers)):
            got = pkg.bilstm_layers(transform, arg, lstm)
            assert got.dtype == torch.float32 and tuple(got.shape) == (5, 31, 256) and got.is_contiguous() and not got.requires_grad
    assert calls[NEW] == 4 and calls[RECURRENCE] == 4, "one projection and one recurrence launch a call"
    assert calls[POOL_LAYERS] == calls[POOL] == calls[LINEAR] == 0, "no pooling launch and no ggcn_linear"
    want = pkg.bilstm(pkg.subword_pool_layers(transform, layers), lstm)
    assert torch.equal(got, want), "%d elements differ" % int((got != want).sum())
    assert pkg.takes_hip_lstm_layers(transform, layers, lstm, 0) is True and pkg.takes_hip_lstm_layers(transform, layers, lstm) is False


def test_layers_with_differing_strides(pkg, dev):
    full, layers = _operands(dev, 2, 5, 20, 32, 3)
    transform, lstm = full[:, :5, :20], _lstm(dev, 96)
    want = pkg.bilstm(pkg.subword_pool_layers(transform, layers), lstm)
    wide = torch.full((2, 20, 40), float("nan"), device=dev)
    wide[:, :, :32] = layers[1]
    turned = layers[2].transpose(1, 2).contiguous().transpose(1, 2)                   # the feature stride is not 1
    assert turned.stride(2) != 1
    arg = [layers[0], wide[:, :, :32], turned]
    assert pkg.takes_hip_lstm_layers(transform, arg, lstm, 0) is True
    assert torch.equal(pkg.bilstm_layers(transform, arg, lstm), want)
    views = [torch.full((2, 20, 40), float("nan"), device=dev) for _ in range(3)]     # shared strides, rows wider than Dl: as they lie
    for v, x in zip(views, layers):
        v[:, :, :32] = x
    assert torch.equal(pkg.bilstm_layers(transform, [v[:, :, :32] for v in views], lstm), want)


@pytest.mark.parametrize("B,T,L", [(0, 3, 5), (2, 0, 5), (2, 3, 0)], ids=["B0", "T0", "L0"])
def test_empty_operands(pkg, dev, monkeypatch, B, T, L):
    lstm = _lstm(dev, 96)
    a, layers = torch.ones(B, T, L, device=dev), [torch.ones(B, L, 32, device=dev) for _ in range(3)]
    want = pkg.bilstm(pkg.subword_pool_layers(a, layers), lstm)
    calls = count_calls(monkeypatch, ENTRIES)
    y = pkg.bilstm_layers(a, layers, lstm)
    assert tuple(y.shape) == (B, T, 256) and y.dtype == torch.float32 and torch.equal(y, want)
    assert calls[NEW] == calls[POOL_LAYERS] == calls[LINEAR] == 0
    assert pkg.takes_hip_lstm_layers(a, layers, lstm) is True          # (no rows: the floor does not apply)


def test_a_wanted_gradient_raises(pkg, dev):
    full, layers = _operands(dev, 2, 5, 20, 32, 3)
    transform, lstm = full[:, :5, :20], _lstm(dev, 96)
    with pytest.raises(RuntimeError, match="bilstm_layers is forward only"):
        pkg.bilstm_layers(transform, [layers[0].clone().requires_grad_(True)] + layers[1:], lstm)
    lstm.weight_hh_l0.requires_grad_(True)
    with pytest.raises(RuntimeError, match="bilstm_layers is forward only"):
        pkg.bilstm_layers(transform, layers, lstm)
    assert pkg.takes_hip_lstm_layers(transform, layers, lstm, 0) is False
    with torch.no_grad():
        assert pkg.takes_hip_lstm_layers(transform, layers, lstm, 0) is True
        assert tuple(pkg.bilstm_layers(transform, layers, lstm).shape) == (2, 5, 256)


def test_the_pooled_words_are_never_allocated(pkg, dev):
    """B = 16, T = 20, L = 40, n = 12, Dl = 768: the pooled words would be B*T*n*Dl*4 = 11.8 MB.  What a call allocates is G
    [B*T, 1024] and y [B*T, 256] float32 (1.6 MB): under a fifth of that."""
    B, T, L, n, Dl = 16, 20, 40, 12, 768
    full, layers = _operands(dev, B, T, L, Dl, n)
    transform, lstm = full[:, :T, :L], _lstm(dev, n * Dl)
    with torch.no_grad():
        pkg.bilstm_layers(transform, layers, lstm)                                     # warm: the weight image is cached
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        y = pkg.bilstm_layers(transform, layers, lstm)
        torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(dev) - before
    print("  peak above the operands: %.2f MB (the pooled words: %.2f MB)" % (rise / 1e6, B * T * n * Dl * 4 / 1e6))
    assert rise < B * T * n * Dl * 4 and y.numel() == B * T * 256


# ------------------------------------------------------------------------------------------------------- (c) the classifiers
CLASSIFIERS = ["GatedGCNEventDetector", "GatedGCNEventDetector54", "GCNEventDetectorNoGate"]
OUTPUTS = ("logits", "xy", "kl", "scores")
OPTION_ENV = ("GGCN_LSTM_LAYERS", "GGCN_POOL_LAYERS", "GGCN_HIP_LSTM", "GGCN_HIP_LSTM_BACKWARD")


class _Bert(torch.nn.Module):
    """Stands in for the encoder: twelve [B,L,768] outputs; ``trainable``: they are leaves that require grad (BERT fine-tuned)."""

    def __init__(self, B, L, dev, dtype=torch.float32, trainable=False, seed=1):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        self.outputs = [torch.randn(B, L, 768, generator=gen).to(dev, dtype).requires_grad_(trainable) for _ in range(12)]
        self.pooled = torch.zeros(B, 768, device=dev)

    def forward(self, ids_, seg, output_all_encoded_layers=True):
        assert tuple(ids_.shape) == tuple(self.outputs[0].shape[:2])
        return list(self.outputs), self.pooled


def _model(pkg, dev, cls_name, ncls, bert, **opt):
    m = getattr(pkg, cls_name)(bert, types.SimpleNamespace(dropout=0.0, polarities_dim=ncls, device=dev, **opt))
    gen = torch.Generator().manual_seed(0)
    for p in m.parameters():
        if p.dim() > 1:
            torch.nn.init.xavier_uniform_(p, generator=gen)
        else:
            torch.nn.init.uniform_(p, -0.05, 0.05, generator=gen)
    return m.to(dev)


def _models(pkg, dev, cls_name, monkeypatch, options, dtype=torch.float32, trainable=False):
    for k in OPTION_ENV:
        monkeypatch.delenv(k, raising=False)
    inputs, ncls = classifier_batch(dev)
    B, L = inputs["sentence_length"].shape[0], int(inputs["cls_text_sep_length"].max())
    models = [_model(pkg, dev, cls_name, ncls, _Bert(B, L, dev, dtype, trainable), **opt) for opt in options]
    assert all(sorted(m.state_dict()) == sorted(models[0].state_dict()) for m in models)
    return inputs, models


def _same(got, ref, what):
    for g, r, name in zip(got, ref, OUTPUTS):
        if torch.is_tensor(r):
            assert torch.equal(g, r), "%s %s: %d elements differ" % (what, name, int((g != r).sum()))
        else:
            assert g == r, "%s %s" % (what, name)        # (the gateless variant: xy = 0.0)


ON = dict(ggcn_lstm_layers=True, ggcn_lstm_layers_min_rows=0)    # (8 sentences: far below the measured floor of the default)


@pytest.mark.parametrize("cls_name", CLASSIFIERS)
def test_classifier_inference(pkg, dev, cls_name, monkeypatch):
    inputs, (on, composed, plain) = _models(pkg, dev, cls_name, monkeypatch,
                                            [ON, dict(ggcn_pool_layers=True, ggcn_hip_lstm=True), dict()])
    assert on.lstm_layers and not on.pool_layers and not on.hip_lstm and not plain.lstm_layers
    with torch.no_grad():
        ref = composed.eval()(inputs)
        default = plain.eval()(inputs)
        calls = count_calls(monkeypatch, ENTRIES)
        got = on.eval()(inputs)
    torch.cuda.synchronize()
    assert calls[NEW] == 1 and calls[RECURRENCE] == 1 and calls["ggcn_anchor_pool_layers"] == 1
    assert calls[POOL_LAYERS] == calls[POOL] == 0, "neither [B,L,9216] nor [B,T,9216] is formed"
    _same(got, ref, cls_name)
    for g, r, name in zip(got, default, OUTPUTS):
        if torch.is_tensor(r):
            gate(g, r, "%s %s against all options off" % (cls_name, name), tol=1e-4)


@pytest.mark.parametrize("cls_name", CLASSIFIERS)
def test_classifier_training_step_does_not_take_the_path(pkg, dev, cls_name, monkeypatch):
    inputs, (on, off) = _models(pkg, dev, cls_name, monkeypatch, [ON, dict()], trainable=True)
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
    assert calls[NEW] == 0 and calls["ggcn_anchor_pool_layers"] == 0
    (ref, ref_loss), (got, got_loss) = results
    assert torch.equal(got_loss, ref_loss)
    _same(got, ref, cls_name)
    for l, (x, r) in enumerate(zip(on.bert.outputs, off.bert.outputs)):
        assert x.grad is not None and torch.equal(x.grad, r.grad), "layer %d" % l
    for (k, p), q in zip(on.named_parameters(), off.parameters()):
        assert (p.grad is None) == (q.grad is None) and (p.grad is None or torch.equal(p.grad, q.grad)), k


@pytest.mark.parametrize("cls_name", CLASSIFIERS)
def test_classifier_under_bf16_autocast_does_not_take_the_path(pkg, dev, cls_name, monkeypatch):
    inputs, (on, off) = _models(pkg, dev, cls_name, monkeypatch, [ON, dict()], dtype=torch.bfloat16)
    calls = count_calls(monkeypatch, ENTRIES)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        got = on.eval()(inputs)
        ref = off.eval()(inputs)
    torch.cuda.synchronize()
    assert calls[NEW] == 0 and calls["ggcn_anchor_pool_layers"] == 0
    _same(got, ref, cls_name)


def test_captured_eval_forward_replays_the_same_bits(pkg, dev, monkeypatch):
    """Both new calls only enqueue (the layers' pointers travel in the kernels' argument blocks, the anchor is read on the
    device): the eval forward captures into a hipGraph and a replay on new layer values gives the bits of an eager forward."""
    inputs, (on,) = _models(pkg, dev, "GatedGCNEventDetector", monkeypatch, [dict(ggcn_precision="bf16x3", **ON)])
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
    assert calls[NEW] == 1 and calls[RECURRENCE] == 1 and calls[POOL_LAYERS] == calls[POOL] == 0
    gen = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for x in on.bert.outputs:
            x.copy_(torch.randn(x.shape, generator=gen))
        ref = on(inputs)
    graph.replay()
    torch.cuda.synchronize()
    _same(out, ref, "replay")
