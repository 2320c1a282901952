"""bfloat16 features on graphs of 33..256 nodes in one launch (ggcn_layer_fused_bf16_wide) and gate dropout drawn inside the bf16
launches (ggcn_layer_fused_bf16_drop for <= 32 nodes), against the float64 oracle (oracle/ref_dense) on text_bf16.double(), which
is exact: a bf16 value is a float64 value.

Gates (the project's own, oracle/gates.py): 1e-4 * max(1, max|ref|) for float32 results;
|dx - ref| <= 2^-8 |ref| + 1e-4 max|ref| for the bf16 dX; for the dropout cases the gates of
test_block_layers_with_gate_dropout_vs_oracle_on_the_exported_masks with TOL["bf16x3"] = 1e-4 (forward: 2 * TOL absolute;
float32 gradients: 5e-4 of the reference's largest entry; xy: 1e-3 relative), the bf16 dX by its own gate above.

Every case asserts the path it ran by counting the library calls, so a silent fall-back to linear + aggregate fails."""
import types

import numpy as np
import pytest
import torch

from oracle import ref_dense
from oracle.backward_ref import TOL
from oracle.gates import close32, gate as _gate, gate_dx as _gate_dx
from oracle.gpu_support import classifier_batch as _classifier_batch, count_calls, dev, drop_mask as _drop_mask, make_layer, pkg  # noqa: F401

pytestmark = pytest.mark.gpu

TOL_BF16X3 = TOL["bf16x3"]
WIDE, DROP, NARROW, LINEAR = "ggcn_layer_fused_bf16_wide", "ggcn_layer_fused_bf16_drop", "ggcn_layer_fused_bf16", "ggcn_linear_bf16"
COUNTED = (WIDE, DROP, NARROW, LINEAR)
ALL_T = [33, 64, 65, 100, 128, 129, 160, 192, 193, 231, 256]


def _adj(B, T, seed, directed=False):
    from ed_gated_gcn_amd import synth
    rng = np.random.default_rng(seed)
    lengths = rng.integers(max(1, T // 3), T + 1, size=B)
    lengths[0] = T                                   # one graph fills every row of its slot
    a = synth.dependency_batch(B, T, 3.5, seed=seed, lengths=lengths).astype(np.float32)
    if directed:
        a = np.triu(a)
    return torch.from_numpy(a)


def _layer(pkg, dev, K, F, seed, precision="bf16x3", bias=True):
    from ed_gated_gcn_amd import synth
    w, b = synth.layer_params(K, F, seed=seed)
    return make_layer(pkg, dev, w, b if bias else None, precision=precision)


def _x(B, T, K, dev, seed, pad=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, K + pad, generator=g).to(torch.bfloat16).to(dev)
    return x[:, :, :K] if pad else x


def _ref_layer(x, adj, m):
    b = None if m.bias is None else m.bias.detach().double()
    return ref_dense.graph_convolution(x.double(), adj.to(x.device).double(), m.weight.detach().double(), b, dtype=torch.float64)


def _forward_on_announced_path(m, x, adj_d, calls):
    """m(x, adj) with the launch counted: the path taken is the one takes_bf16_wide_path announces."""
    csr = m._as_csr(adj_d, x)
    wide = m.takes_bf16_wide_path(x, csr)
    assert not m.takes_fused_path(x, csr) and not m.takes_bf16_fused_path(x, csr)   # the existing predicates: untouched
    before = dict(calls)
    with torch.no_grad():
        out = m(x, adj_d)
    assert calls[WIDE] - before[WIDE] == (1 if wide else 0)
    assert calls[LINEAR] - before[LINEAR] == (0 if wide else 1)
    return out, wide


# ---------------------------------------------------------------- 1. layer forward
@pytest.mark.parametrize("T", ALL_T)
def test_layer_forward_vs_float64_every_slot(pkg, dev, T, monkeypatch):
    """H = 256, B = 5: the last workgroup of the 64-row slot kernel holds one graph of its two.  Run on the default rule (whatever
    it says for this shape), then with fused_max_t = 256 (always one launch), then with fused = False (never)."""
    B, K, F = 5, 256, 256
    calls = count_calls(monkeypatch, COUNTED)
    m = _layer(pkg, dev, K, F, seed=1)
    x, adj = _x(B, T, K, dev, seed=2), _adj(B, T, seed=3)
    ref = _ref_layer(x, adj, m)
    out, wide = _forward_on_announced_path(m, x, adj.to(dev), calls)
    # the measured default rule (GraphConvolution.takes_bf16_wide_path): a slot filled to >= 75 % up to 128 nodes; longer
    # graphs only in whole rounds of workgroups, which 5 graphs never fill
    assert wide == (48 <= T <= 64 or 96 <= T <= 128)
    assert out.dtype == torch.float32 and out.shape == (B, T, F)
    _gate(out, ref, "out T=%d default" % T)
    m.fused_max_t = 256
    out, wide = _forward_on_announced_path(m, x, adj.to(dev), calls)
    assert wide
    _gate(out, ref, "out T=%d one launch" % T)
    m.fused = False
    out, wide = _forward_on_announced_path(m, x, adj.to(dev), calls)
    assert not wide
    _gate(out, ref, "out T=%d linear + aggregate" % T)


@pytest.mark.parametrize("B,T,K,F,pad,bias,directed", [
    (6, 100, 768, 768, 0, True, False),      # H = 768
    (3, 231, 768, 768, 0, True, False),
    (5, 100, 300, 300, 0, True, False),      # K % 32 != 0, F not a multiple of the 256-column tile
    (5, 200, 300, 300, 0, True, False),
    (7, 60, 256, 192, 3, True, False),       # a view with row stride K + 3: element loads
    (7, 100, 256, 192, 3, False, False),     # ... and no bias
    (3, 231, 256, 192, 3, False, False),
    (9, 100, 256, 256, 0, True, True),       # directed graphs
    (4, 231, 256, 256, 0, True, True),
], ids=["H768-T100", "H768-T231", "K300-T100", "K300-T200", "view-T60", "view-nobias-T100", "view-nobias-T231", "directed-T100",
        "directed-T231"])
def test_layer_forward_shapes(pkg, dev, B, T, K, F, pad, bias, directed, monkeypatch):
    calls = count_calls(monkeypatch, COUNTED)
    m = _layer(pkg, dev, K, F, seed=4, bias=bias)
    m.fused_max_t = 256                               # the kernels are under test here, not the default rule
    x, adj = _x(B, T, K, dev, seed=5, pad=pad), _adj(B, T, seed=6, directed=directed)
    assert x.is_contiguous() == (pad == 0)
    out, wide = _forward_on_announced_path(m, x, adj.to(dev), calls)
    assert wide
    _gate(out, _ref_layer(x, adj, m), "out")


@pytest.mark.parametrize("precision", ["f16mx8", "f16mx6"])
def test_every_split_precision_means_the_bf16_pair_form(pkg, dev, precision, monkeypatch):
    from ed_gated_gcn_amd import _capi
    if precision == "f16mx6" and not _capi.has_f16mx6():
        precision = "f16mx8"
    calls = count_calls(monkeypatch, COUNTED)
    B, T, K, F = 6, 100, 256, 256
    x, adj = _x(B, T, K, dev, seed=2), _adj(B, T, seed=3).to(dev)
    ref = _layer(pkg, dev, K, F, seed=1, precision="bf16x3")
    m = _layer(pkg, dev, K, F, seed=1, precision=precision)
    with torch.no_grad():
        assert torch.equal(m(x, adj), ref(x, adj))
    assert calls[WIDE] == 2


# ---------------------------------------------------------------- 2. one launch vs linear + aggregate
@pytest.mark.parametrize("T", [64, 100, 160, 231])
def test_one_launch_agrees_with_linear_plus_aggregate(pkg, dev, T, monkeypatch):
    calls = count_calls(monkeypatch, COUNTED)
    B, K, F = 6, 256, 256
    m = _layer(pkg, dev, K, F, seed=1)
    m.fused_max_t = 256
    x, adj = _x(B, T, K, dev, seed=2), _adj(B, T, seed=3).to(dev)
    with torch.no_grad():
        one = m(x, adj)
        m.fused = False
        two = m(x, adj)
    assert calls[WIDE] == 1 and calls[LINEAR] == 1
    _gate(one, two.double(), "one launch vs two, T=%d" % T)


# ---------------------------------------------------------------- 3. forward_gated: gates, pools, overlap
@pytest.mark.parametrize("T", [60, 100, 231])
def test_forward_gated_gates_pools_and_overlap(pkg, dev, T, monkeypatch):
    calls = count_calls(monkeypatch, COUNTED)
    B, K, F = 6, 256, 256
    m = _layer(pkg, dev, K, F, seed=11)
    m.fused_max_t = 256
    x, adj = _x(B, T, K, dev, seed=12), _adj(B, T, seed=13)
    g = torch.Generator().manual_seed(14)
    sg, ga, gb = (torch.rand(B, F, generator=g).to(dev) for _ in range(3))
    gb = gb - 0.5                                     # negative gate entries: the pool takes the minimum there
    part = torch.empty(B, (F + 63) // 64, dtype=torch.float32, device=dev)
    xy = torch.empty((), dtype=torch.float32, device=dev)
    with torch.no_grad():
        out, pa, pb = m.forward_gated(x, adj.to(dev), store_gate=sg, pool_gate_a=ga, pool_gate_b=gb, want_pool_a=True,
                                      want_pool_b=True, overlap_partial=part)
        m.forward_gated(x, adj.to(dev), pool_gate_a=ga, want_out=False, want_pool_a=True, overlap_reduce=(part, xy))
    assert calls[WIDE] == 2 and calls[LINEAR] == 0
    y = _ref_layer(x, adj, m)
    ra, rb = (y * ga.double()[:, None]).max(1)[0], (y * gb.double()[:, None]).max(1)[0]
    _gate(out, y * sg.double()[:, None], "out")
    _gate(pa, ra, "pool_a")
    _gate(pb, rb, "pool_b")
    _gate(xy, (ra * rb).sum(1).mean(), "xy")


def test_overlap_and_dropout_refused_off_the_one_launch_path(pkg, dev):
    B, T, K, F = 4, 100, 64, 64
    m = _layer(pkg, dev, K, F, seed=1)
    m.fused = False
    x, adj = _x(B, T, K, dev, seed=2), _adj(B, T, seed=3).to(dev)
    part = torch.empty(B, 1, dtype=torch.float32, device=dev)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="overlap_partial / overlap_reduce need the one-launch layer"):
            m.forward_gated(x, adj, overlap_partial=part)
        with pytest.raises(RuntimeError, match="dropout= needs the one-launch layer"):
            m.forward_gated(x, adj, dropout=(0.5, 1, (0, 1, 2)))


# ---------------------------------------------------------------- 4. gate dropout inside the launches
@pytest.mark.parametrize("T", [31, 60, 100, 200], ids=["T31", "T60-64row", "T100-128row", "T200-eight-wavefronts"])
def test_block_layers_with_gate_dropout_bf16_vs_oracle_on_the_exported_masks(pkg, dev, T, monkeypatch):
    """bert_amir5.py:621-640 in training mode on bf16 features: the two layer launches draw the keep factors themselves (stream 1 =
    gate1, stream 2 = gate2 in both layers); the float64 oracle gets the same factors from ggcn_dropout_mask -- forward and, through
    torch autograd, backward.  gc1 reads the bf16 x (the new launches), gc2 the float32 gcn1 (ggcn_layer_fused_drop)."""
    calls = count_calls(monkeypatch, COUNTED)
    B, H, p, seed = 12, 128, 0.5, 2 ** 40 + 99
    rng = np.random.default_rng(5)
    from ed_gated_gcn_amd import synth
    adj = synth.dependency_batch(B, T, 3.5, seed=8, lengths=rng.integers(4, T + 1, size=B))
    t = torch.from_numpy
    x = t(rng.standard_normal((B, T, H)).astype(np.float32)).to(torch.bfloat16)
    g1 = torch.sigmoid(t(rng.standard_normal((B, H)).astype(np.float32)))
    g2 = torch.sigmoid(t(rng.standard_normal((B, H)).astype(np.float32)))
    w1, b1 = synth.layer_params(H, H, seed=1)
    w2, b2 = synth.layer_params(H, H, seed=2)
    R1 = t(rng.standard_normal((B, H)).astype(np.float32))
    R2 = t(rng.standard_normal((B, T, H)).astype(np.float32))
    gc1, gc2 = _layer(pkg, dev, H, H, seed=1).train(), _layer(pkg, dev, H, H, seed=2).train()
    gc1.fused_max_t = 256                             # (12 graphs of 200 nodes fill no round of workgroups: one launch on request)
    xg, g1g, g2g = (v.to(dev).requires_grad_() for v in (x, g1, g2))
    adj_d = t(adj).to(dev)
    csr = gc1._as_csr(adj_d, xg)
    assert gc1.takes_bf16_dropout_path(xg, csr) and not gc1.takes_dropout_path(xg, csr)
    gcn1, x1, y1 = gc1.forward_gated(xg, adj_d, pool_gate_a=g1g, pool_gate_b=g2g, want_pool_a=True, want_pool_b=True,
                                     dropout=(p, seed, (0, 1, 2)))
    xo, out, _ = gc2.forward_gated(gcn1, adj_d, store_gate=g2g, pool_gate_a=g2g, want_pool_a=True, dropout=(p, seed, (2, 2, 0)))
    assert gcn1.dtype == x1.dtype == xo.dtype == torch.float32
    assert calls[DROP if T <= 32 else WIDE] == 1 and calls[LINEAR] == 0 and calls[NARROW] == 0
    xy = (x1 * y1).sum(1).mean()
    ((out * R1.to(dev)).sum() + 0.1 * (xo * R2.to(dev)).sum() + 0.01 * xy).backward()

    k1 = _drop_mask(pkg, dev, B * T, H, p, seed, 1).view(B, T, H).cpu().double()
    k2 = _drop_mask(pkg, dev, B * T, H, p, seed, 2).view(B, T, H).cpu().double()
    R1, R2 = R1.double(), R2.double()
    xr, g1r, g2r = x.double().requires_grad_(), g1.double().requires_grad_(), g2.double().requires_grad_()
    w1r, b1r, w2r, b2r = (t(v).double().requires_grad_() for v in (w1, b1, w2, b2))
    a = t(adj).double()
    gate1 = g1r[:, None, :] * k1                                           # :621-624: repeat, then dropout
    gate2 = g2r[:, None, :] * k2
    gcn1_r = ref_dense.graph_convolution(xr, a, w1r, b1r, dtype=torch.float64)   # :626
    # a max-pool routes its gradient to the argmax row and a ~1e-5 forward difference can flip a near-tie: the reference
    # takes the rows the GPU forward selected (that they are maxima of the reference values too is checked below)
    with torch.no_grad():
        i1 = (gcn1.detach().cpu().double() * gate1).argmax(1)
        i2 = (gcn1.detach().cpu().double() * gate2).argmax(1)
        io = xo.detach().cpu().argmax(1)
    x1_r = (gcn1_r * gate1).gather(1, i1[:, None, :])[:, 0]                # :627-635
    y1_r = (gcn1_r * gate2).gather(1, i2[:, None, :])[:, 0]                # :631-636
    xy_r = (x1_r * y1_r).sum(1).mean()                                     # :638
    xo_r = gate2 * ref_dense.graph_convolution(gcn1_r, a, w2r, b2r, dtype=torch.float64)   # :639
    out_r = xo_r.gather(1, io[:, None, :])[:, 0]                           # :640
    ((out_r * R1).sum() + 0.1 * (xo_r * R2).sum() + 0.01 * xy_r).backward()
    tol = TOL_BF16X3
    for name, got, want in (("gcn1", gcn1, gcn1_r), ("x1", x1, x1_r), ("y1", y1, y1_r), ("x", xo, xo_r), ("out", out, out_r)):
        err = float((got.detach().cpu().double() - want.detach()).abs().max())
        print("%s: max|diff| %.3g (gate %.3g)" % (name, err, 2 * tol))
        assert err <= 2 * tol, "%s: max|diff| %.3g" % (name, err)
    with torch.no_grad():   # the gathered rows are maxima of the reference's own values (up to the tolerance)
        assert float(((gcn1_r * gate1).max(1)[0] - x1_r).abs().max()) <= 2 * tol
        assert float((xo_r.max(1)[0] - out_r).abs().max()) <= 2 * tol
    assert abs(float(xy.detach()) - float(xy_r.detach())) <= 1e-3 * max(1.0, abs(float(xy_r.detach())))
    assert xg.grad.dtype == torch.bfloat16
    _gate_dx(xg.grad, xr.grad)
    for name, got, want in (("d gate1", g1g.grad, g1r.grad), ("d gate2", g2g.grad, g2r.grad),
                            ("d W1", gc1.weight.grad, w1r.grad), ("d b1", gc1.bias.grad, b1r.grad),
                            ("d W2", gc2.weight.grad, w2r.grad), ("d b2", gc2.bias.grad, b2r.grad)):
        close32(got, want, name, rel=5e-4)
    assert 0.45 < float((k1 == 0).double().mean()) < 0.55


# ---------------------------------------------------------------- 5. determinism
@pytest.mark.parametrize("T,dropout", [(100, None), (100, (0.25, 77, (1, 1, 2))), (231, (0.25, 77, (1, 1, 2))), (31, (0.25, 77, (1, 1, 2)))])
def test_forward_and_backward_are_deterministic(pkg, dev, T, dropout):
    B, K, F = 6, 256, 256
    adj = _adj(B, T, seed=51).to(dev)

    def run():
        m = _layer(pkg, dev, K, F, seed=52)
        m.fused_max_t = 256
        x = _x(B, T, K, dev, seed=53).requires_grad_()
        g = torch.Generator().manual_seed(54)
        sg, ga = (torch.rand(B, F, generator=g).to(dev).requires_grad_() for _ in range(2))
        out, pa, _ = m.forward_gated(x, adj, store_gate=sg, pool_gate_a=ga, want_pool_a=True, dropout=dropout)
        (out.sum() + pa.sum()).backward()
        return [t.detach().clone() for t in (out, pa, x.grad, m.weight.grad, m.bias.grad, sg.grad, ga.grad)]
    r1, r2 = run(), run()
    for a, b in zip(r1, r2):
        assert torch.equal(a, b)


# ---------------------------------------------------------------- 6. the block and the classifier under bf16 autocast
@pytest.mark.parametrize("T", [100, 231])
def test_gated_block_inference_under_autocast(pkg, dev, T, monkeypatch):
    calls = count_calls(monkeypatch, COUNTED)
    B, H = 6, 256
    gc1, gc2 = _layer(pkg, dev, H, H, seed=31), _layer(pkg, dev, H, H, seed=32)
    gc1.fused_max_t = gc2.fused_max_t = 256           # (6 graphs of 231 nodes: one launch on request)
    x, adj = _x(B, T, H, dev, seed=33), _adj(B, T, seed=34)
    g = torch.Generator().manual_seed(35)
    g1, g2 = torch.rand(B, H, generator=g).to(dev), torch.rand(B, H, generator=g).to(dev)
    d = lambda t: t.detach().double()   # noqa: E731
    ref = ref_dense.gated_block(x.double(), adj.to(dev).double(), d(g1), d(g2), d(gc1.weight), d(gc1.bias), d(gc2.weight),
                                d(gc2.bias), dtype=torch.float64)
    csr = gc1._as_csr(adj.to(dev), x)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        r = pkg.gated_gcn_block(x, csr, g1, g2, gc1, gc2, want_gcn1=True)
        r_out = pkg.gated_gcn_block(x, csr, g1, g2, gc1, gc2, want=("out",))
    assert calls[WIDE] == 2 and calls[LINEAR] == 0
    for k in ("gcn1", "x1", "y1", "xy", "x", "out"):
        assert r[k].dtype == torch.float32, k
        _gate(r[k], ref[k], k)
    _gate(r_out["out"], ref["out"], "want=out")


@pytest.mark.parametrize("ORI_ML,BERT_ML", [(31, 65), (100, 128)], ids=["T31", "T100"])
def test_classifier_trains_with_dropout_under_bf16_autocast(pkg, dev, ORI_ML, BERT_ML, monkeypatch):
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(5)
    inputs, NCLS = _classifier_batch(dev, ORI_ML, BERT_ML)
    opt = types.SimpleNamespace(device=dev, dropout=0.25, polarities_dim=NCLS)
    model = pkg.GatedGCNEventDetector(pkg.LegacyBertAdapter(transformers.BertModel(transformers.BertConfig())), opt)
    ref_dense.reset_params_like_train([p for n, p in model.named_parameters() if not n.startswith("bert.")],
                                      torch.Generator().manual_seed(9))
    model = model.to(dev)
    seen = []
    orig = model.gc1.forward_gated

    def spy(text, *a, **k):   # (the autograd Function re-enters forward_gated with _internal=True: the classifier's own call is counted)
        if not k.get("_internal"):
            seen.append((text.dtype, k.get("dropout")))
        return orig(text, *a, **k)
    monkeypatch.setattr(model.gc1, "forward_gated", spy)
    dims = []
    model.dropout.register_forward_hook(lambda mod, inp, out: dims.append(inp[0].dim()))   # the classifier's own dropout module
    calls = count_calls(monkeypatch, COUNTED)
    model.train()
    assert model.dropout.p == 0.25
    with torch.autocast("cuda", dtype=torch.bfloat16):
        logits, xy, kl, scores = model(inputs)
        loss = torch.nn.functional.cross_entropy(logits.float(), torch.arange(logits.shape[0], device=dev) % NCLS)
        loss = loss + torch.as_tensor(xy, device=dev).float() + kl.float()
    loss.backward()
    assert torch.isfinite(loss)
    assert len(seen) == 1 and seen[0][0] == torch.bfloat16
    p, seed, streams = seen[0][1]
    assert p == 0.25 and tuple(streams) == (0, 1, 2)
    assert calls[DROP if ORI_ML <= 32 else WIDE] == 1 and calls[LINEAR] == 0 and calls[NARROW] == 0
    assert dims and all(d < 3 for d in dims), "a [B,T,H] tensor went through the classifier's dropout: %s" % dims
    for name in ("gc1", "gc2"):
        gw = getattr(model, name).weight.grad
        assert gw is not None and torch.isfinite(gw).all() and float(gw.abs().max()) > 0, name
    for name in ("gate1", "gate2"):
        gws = [q.grad for q in getattr(model, name).parameters()]
        assert all(q is not None and torch.isfinite(q).all() for q in gws), name
