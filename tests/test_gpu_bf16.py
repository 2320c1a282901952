"""bfloat16 features on the MI355X (include/ggcn.h "bfloat16 features"): the layer, its backward, the gated block and the
classifier under torch.autocast(dtype=torch.bfloat16), against the float64 oracle (oracle/ref_dense) on text_bf16.double(),
which is exact: a bf16 value is a float64 value.

Gates: the existing bf16x3 tests' 1e-4 * max(1, max|ref|) for float32 results (out, pools, dW, db, gate gradients); for the
bf16 dX, |dx - ref| <= 2^-8 |ref| + 1e-4 max|ref| (one bf16 rounding of the stored value on top of the bf16x3 error)."""
import types

import numpy as np
import pytest
import torch

from oracle import ref_dense
from oracle.gates import gate as _gate, gate_dx as _gate_dx
from oracle.gpu_support import classifier_batch as _classifier_batch, count_calls, dev, make_layer, pkg  # noqa: F401

pytestmark = pytest.mark.gpu


def _adj(B, T, seed, weighted=False, directed=False):
    from ed_gated_gcn_amd import synth
    rng = np.random.default_rng(seed)
    a = synth.dependency_batch(B, T, 3.5, seed=seed, lengths=rng.integers(max(1, T // 3), T + 1, size=B)).astype(np.float32)
    if directed:
        a = np.triu(a)
    if weighted:
        a = a * rng.uniform(0.25, 2.0, size=a.shape).astype(np.float32)
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


# ---------------------------------------------------------------- 1. layer forward
@pytest.mark.parametrize("B,T,K,F", [(64, 31, 256, 256), (4096, 32, 768, 768), (7, 17, 300, 300), (8, 100, 256, 256),
                                     (4, 231, 256, 256)])
def test_layer_forward_vs_float64(pkg, dev, B, T, K, F):
    m = _layer(pkg, dev, K, F, seed=1)
    x = _x(B, T, K, dev, seed=2)
    adj = _adj(B, T, seed=3)
    csr = m._as_csr(adj.to(dev), x)
    assert m.takes_bf16_fused_path(x, csr) == (T <= 32)
    assert not m.takes_fused_path(x, csr)            # the float32 predicate is untouched
    with torch.no_grad():
        out = m(x, adj.to(dev))
    assert out.dtype == torch.float32 and out.shape == (B, T, F)
    _gate(out, _ref_layer(x, adj, m), "out")


@pytest.mark.parametrize("precision", ["f16mx8", "f16mx6"])
def test_every_split_precision_means_the_bf16_pair_form(pkg, dev, precision):
    from ed_gated_gcn_amd import _capi
    if precision == "f16mx6" and not _capi.has_f16mx6():
        precision = "f16mx8"
    B, T, K, F = 64, 31, 256, 256
    x, adj = _x(B, T, K, dev, seed=2), _adj(B, T, seed=3).to(dev)
    ref = _layer(pkg, dev, K, F, seed=1, precision="bf16x3")
    m = _layer(pkg, dev, K, F, seed=1, precision=precision)
    with torch.no_grad():
        assert torch.equal(m(x, adj), ref(x, adj))


def test_fp32_and_f16_precisions_refuse_bf16(pkg, dev):
    x, adj = _x(2, 8, 64, dev, seed=1), _adj(2, 8, seed=1).to(dev)
    for precision in ("fp32", "f16"):
        m = _layer(pkg, dev, 64, 64, seed=1, precision=precision)
        with pytest.raises(RuntimeError, match="bfloat16 features need precision"):
            m(x, adj)


def test_noncontiguous_view_bias_none_and_empty_batch(pkg, dev):
    B, T, K, F = 16, 29, 256, 192
    x = _x(B, T, K, dev, seed=4, pad=3)              # row stride K + 3: the element-load form of the main loop
    assert not x.is_contiguous()
    adj = _adj(B, T, seed=5)
    for bias in (True, False):
        m = _layer(pkg, dev, K, F, seed=6, bias=bias)
        with torch.no_grad():
            out = m(x, adj.to(dev))
        _gate(out, _ref_layer(x, adj, m), "out bias=%s" % bias)
    with torch.no_grad():
        e = m(x[:0], adj[:0].to(dev))
    assert e.shape == (0, T, F) and e.dtype == torch.float32


@pytest.mark.parametrize("T", [24, 60])
def test_weighted_adjacency(pkg, dev, T):
    B, K, F = 32, 256, 256
    m = _layer(pkg, dev, K, F, seed=7)
    x = _x(B, T, K, dev, seed=8)
    adj = _adj(B, T, seed=9, weighted=True)
    csr = m._as_csr(adj.to(dev), x)
    assert not csr.is_binary and not m.takes_bf16_fused_path(x, csr)   # linear_bf16 + aggregate
    with torch.no_grad():
        out = m(x, adj.to(dev))
    _gate(out, _ref_layer(x, adj, m), "out")


def test_one_launch_agrees_with_linear_plus_aggregate(pkg, dev):
    B, T, K, F = 64, 31, 256, 256
    m = _layer(pkg, dev, K, F, seed=1)
    x, adj = _x(B, T, K, dev, seed=2), _adj(B, T, seed=3).to(dev)
    with torch.no_grad():
        one = m(x, adj)
        m.fused = False
        two = m(x, adj)
    _gate(one, two.double(), "one launch vs two")


# ---------------------------------------------------------------- 2. forward_gated
def test_forward_gated_gates_pools_and_overlap(pkg, dev):
    B, T, K, F = 64, 31, 256, 256
    m = _layer(pkg, dev, K, F, seed=11)
    x, adj = _x(B, T, K, dev, seed=12), _adj(B, T, seed=13)
    g = torch.Generator().manual_seed(14)
    sg, ga, gb = (torch.rand(B, F, generator=g).to(dev) for _ in range(3))
    part = torch.empty(B, (F + 63) // 64, dtype=torch.float32, device=dev)
    xy = torch.empty((), dtype=torch.float32, device=dev)
    with torch.no_grad():
        out, pa, pb = m.forward_gated(x, adj.to(dev), store_gate=sg, pool_gate_a=ga, pool_gate_b=gb, want_pool_a=True,
                                      want_pool_b=True, overlap_partial=part)
        m.forward_gated(x, adj.to(dev), pool_gate_a=ga, want_out=False, want_pool_a=True, overlap_reduce=(part, xy))
    y = _ref_layer(x, adj, m)
    ra, rb = (y * ga.double()[:, None]).max(1)[0], (y * gb.double()[:, None]).max(1)[0]
    _gate(out, y * sg.double()[:, None], "out")
    _gate(pa, ra, "pool_a")
    _gate(pb, rb, "pool_b")
    _gate(xy, (ra * rb).sum(1).mean(), "xy")


# ---------------------------------------------------------------- 3. backward
def _backward_case(pkg, dev, B, T, K, F, adj, seed):
    m = _layer(pkg, dev, K, F, seed=seed)
    x = _x(B, T, K, dev, seed=seed + 1).requires_grad_()
    g = torch.Generator().manual_seed(seed + 2)
    sg, ga, gb = (torch.rand(B, F, generator=g).to(dev).requires_grad_() for _ in range(3))
    r1, r2, r3 = torch.randn(B, T, F, generator=g).double(), torch.randn(B, F, generator=g).double(), torch.randn(B, F, generator=g).double()
    out, pa, pb = m.forward_gated(x, adj.to(dev), store_gate=sg, pool_gate_a=ga, pool_gate_b=gb, want_pool_a=True, want_pool_b=True)
    assert out.dtype == pa.dtype == torch.float32
    ((out.double() * r1.to(dev)).sum() + (pa.double() * r2.to(dev)).sum() + (pb.double() * r3.to(dev)).sum()).backward()
    # float64 autograd on the same (exact) inputs
    x64 = x.detach().double().requires_grad_()
    w64 = m.weight.detach().double().requires_grad_()
    b64 = m.bias.detach().double().requires_grad_()
    s64, a64, bb64 = (t.detach().double().requires_grad_() for t in (sg, ga, gb))
    y = ref_dense.graph_convolution(x64, adj.to(dev).double(), w64, b64, dtype=torch.float64)
    ro, ra, rb = y * s64[:, None], (y * a64[:, None]).max(1)[0], (y * bb64[:, None]).max(1)[0]
    ((ro * r1.to(dev)).sum() + (ra * r2.to(dev)).sum() + (rb * r3.to(dev)).sum()).backward()
    _gate_dx(x.grad, x64.grad)
    for got, ref, what in ((m.weight.grad, w64.grad, "dW"), (m.bias.grad, b64.grad, "db"), (sg.grad, s64.grad, "d store gate"),
                           (ga.grad, a64.grad, "d gate a"), (gb.grad, bb64.grad, "d gate b")):
        assert got.dtype == torch.float32, what
        _gate(got, ref, what)


@pytest.mark.parametrize("form", ["mma", "one_pass"])
def test_backward_t31(pkg, dev, form, monkeypatch):
    if form == "one_pass":
        monkeypatch.setenv("GGCN_BACKWARD_SCALAR", "1")
    _backward_case(pkg, dev, 64, 31, 256, 256, _adj(64, 31, seed=21), seed=22)


def test_backward_t100_two_pass(pkg, dev):
    _backward_case(pkg, dev, 16, 100, 256, 256, _adj(16, 100, seed=23), seed=24)


def test_backward_directed_graph(pkg, dev):
    _backward_case(pkg, dev, 32, 31, 256, 256, _adj(32, 31, seed=25, directed=True), seed=26)


def test_backward_weighted_adjacency(pkg, dev):
    _backward_case(pkg, dev, 32, 24, 256, 256, _adj(32, 24, seed=27, weighted=True), seed=28)


# ---------------------------------------------------------------- 4. the gated block
def test_gated_block_bf16_inference_and_training(pkg, dev):
    B, T, H = 64, 31, 256
    gc1, gc2 = _layer(pkg, dev, H, H, seed=31), _layer(pkg, dev, H, H, seed=32)
    x, adj = _x(B, T, H, dev, seed=33), _adj(B, T, seed=34)
    g = torch.Generator().manual_seed(35)
    g1, g2 = torch.rand(B, H, generator=g).to(dev), torch.rand(B, H, generator=g).to(dev)
    d = lambda t: t.detach().double()   # noqa: E731
    ref = ref_dense.gated_block(x.double(), adj.to(dev).double(), d(g1), d(g2), d(gc1.weight), d(gc1.bias), d(gc2.weight),
                                d(gc2.bias), dtype=torch.float64)
    csr = gc1._as_csr(adj.to(dev), x)
    with torch.no_grad():
        r = pkg.gated_gcn_block(x, csr, g1, g2, gc1, gc2, want_gcn1=True)
        r_out = pkg.gated_gcn_block(x, csr, g1, g2, gc1, gc2, want=("out",))
    for k in ("gcn1", "x1", "y1", "xy", "x", "out"):
        assert r[k].dtype == torch.float32, k
        _gate(r[k], ref[k], k)
    assert r_out["x"] is None and r_out["xy"] is None
    _gate(r_out["out"], ref["out"], "want=out")
    # training: gradients of both layers' weights and of the gates
    g1r, g2r = g1.clone().requires_grad_(), g2.clone().requires_grad_()
    rt = pkg.gated_gcn_block(x, csr, g1r, g2r, gc1, gc2)
    (rt["out"].sum() + rt["xy"]).backward()
    w = [t.detach().double().requires_grad_() for t in (g1, g2, gc1.weight, gc1.bias, gc2.weight, gc2.bias)]
    rr = ref_dense.gated_block(x.double(), adj.to(dev).double(), *w[:2], w[2], w[3], w[4], w[5], dtype=torch.float64)
    (rr["out"].sum() + rr["xy"]).backward()
    for got, ref64, what in ((g1r.grad, w[0].grad, "d gate1"), (g2r.grad, w[1].grad, "d gate2"), (gc1.weight.grad, w[2].grad, "dW1"),
                             (gc1.bias.grad, w[3].grad, "db1"), (gc2.weight.grad, w[4].grad, "dW2"), (gc2.bias.grad, w[5].grad, "db2")):
        _gate(got, ref64, what)


# ---------------------------------------------------------------- 5. the classifier under bf16 autocast
@pytest.mark.parametrize("cls_name", ["GatedGCNEventDetector", "GatedGCNEventDetector54", "GCNEventDetectorNoGate"])
def test_classifier_under_bf16_autocast(pkg, dev, cls_name, monkeypatch):
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(5)
    inputs, NCLS = _classifier_batch(dev)
    opt = types.SimpleNamespace(device=dev, dropout=0.25, polarities_dim=NCLS)
    model = getattr(pkg, cls_name)(pkg.LegacyBertAdapter(transformers.BertModel(transformers.BertConfig())), opt)
    # Instructor._reset_params (train.py:75-84) on everything but BERT: the layers leave their parameters uninitialised
    ref_dense.reset_params_like_train([p for n, p in model.named_parameters() if not n.startswith("bert.")],
                                      torch.Generator().manual_seed(9))
    model = model.to(dev)
    seen = []
    orig = model.gc1.forward_gated

    def spy(text, *a, **k):   # every path to gc1 (module call or the block) goes through forward_gated
        seen.append(text.dtype)
        return orig(text, *a, **k)
    monkeypatch.setattr(model.gc1, "forward_gated", spy)
    calls = count_calls(monkeypatch, ["ggcn_layer_fused_bf16", "ggcn_dweight_bf16", "ggcn_linear_out_bf16"])
    # eval: the full forward and the logits-only form
    model.eval()
    for logits_only in (False, True):
        model.eval_logits_only = logits_only
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            res = model(inputs)
        assert torch.isfinite(res[0].float()).all()
        if not logits_only:
            assert all(torch.isfinite(torch.as_tensor(t).float()).all() for t in res[1:])
    assert seen and all(d == torch.bfloat16 for d in seen) and calls["ggcn_layer_fused_bf16"] > 0
    model.eval_logits_only = False
    # training, with the module's dropout (0.25) and without
    for p_drop in (0.25, 0.0):
        model.train()
        model.dropout.p = p_drop
        model.zero_grad(set_to_none=True)
        seen.clear()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            logits, xy, kl, scores = model(inputs)
            loss = torch.nn.functional.cross_entropy(logits.float(), torch.arange(logits.shape[0], device=dev) % NCLS)
            loss = loss + torch.as_tensor(xy, device=dev).float() + kl.float()
        loss.backward()
        assert torch.isfinite(loss)
        assert seen and all(d == torch.bfloat16 for d in seen)
        for name in ("gc1", "gc2"):
            gw = getattr(model, name).weight.grad
            assert gw is not None and torch.isfinite(gw).all() and float(gw.abs().max()) > 0, (name, p_drop)
    assert calls["ggcn_dweight_bf16"] >= 2 and calls["ggcn_linear_out_bf16"] >= 2


# ---------------------------------------------------------------- 6. sub-word pooling
def test_subword_pool_bf16(pkg, dev):
    from ed_gated_gcn_amd.pooling import subword_pool
    B, T, L, D = 4, 31, 65, 9216
    g = torch.Generator().manual_seed(41)
    a = torch.zeros(B, T, L)
    for b in range(B):
        pos = 1
        for t in range(T):
            n = int(torch.randint(1, 3, (1,), generator=g))
            if pos + n > L:
                break
            a[b, t, pos:pos + n] = 1.0 / n
            pos += n
    x = torch.randn(B, L, D, generator=g).to(torch.bfloat16).to(dev)
    for xv in (x, x[:, :, : D - 4]):   # the 8-byte form and a row stride that is not D
        y = subword_pool(a.to(dev), xv)
        assert y.dtype == torch.bfloat16
        ref = torch.bmm(a.double().to(dev), xv.double())
        ulp = torch.where(ref == 0, torch.zeros_like(ref), 2.0 ** (torch.floor(torch.log2(ref.abs())) - 7))
        assert bool(((y.double() - ref).abs() <= ulp + 1e-30).all())
    xg = x.clone().requires_grad_()
    subword_pool(a.to(dev), xg).float().sum().backward()
    assert xg.grad.dtype == torch.bfloat16
    _gate(xg.grad.float(), a.double().sum(1)[:, :, None].expand(B, L, D).to(dev), "dX")


# ---------------------------------------------------------------- 7. determinism
def test_bf16_forward_and_backward_are_deterministic(pkg, dev):
    B, T, K, F = 64, 31, 256, 256
    adj = _adj(B, T, seed=51).to(dev)

    def run():
        m = _layer(pkg, dev, K, F, seed=52)
        x = _x(B, T, K, dev, seed=53).requires_grad_()
        ga = torch.rand(B, F, generator=torch.Generator().manual_seed(54)).to(dev).requires_grad_()
        out, pa, _ = m.forward_gated(x, adj, pool_gate_a=ga, want_pool_a=True)
        (out.sum() + pa.sum()).backward()
        return [t.detach().clone() for t in (out, pa, x.grad, m.weight.grad, m.bias.grad, ga.grad)]
    r1, r2 = run(), run()
    for a, b in zip(r1, r2):
        assert torch.equal(a, b)
