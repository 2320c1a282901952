"""bfloat16 features, inference, with ``GraphConvolution.bf16_block`` on (opt.ggcn_bf16_block / GGCN_BF16_BLOCK=1; off by default):
the whole gated block as ONE launch for graphs of <= 32 nodes (ggcn_block_fused_bf16), its eval forms, and the folded evaluation
of graphs of 33..256 nodes (ggcn_aggregate_bf16 + one ggcn_layer_fused_prebias launch, W1 never multiplied).

Oracle: oracle/ref_dense.gated_block in float64 on x.double() (exact: a bf16 value is a float64 value).  Gate: the project's own
1e-4 * max(1, max|ref|) (``gate`` of oracle/gates.py) for every output."""
import types

import numpy as np
import pytest
import torch

from oracle import ref_dense
from oracle.gates import gate as _gate
from oracle.gpu_support import classifier_batch as _classifier_batch, count_calls, dev, make_layer, pkg  # noqa: F401

pytestmark = pytest.mark.gpu

LAYER_ENTRIES = ("ggcn_layer_fused_bf16", "ggcn_layer_fused_bf16_drop", "ggcn_layer_fused_bf16_wide", "ggcn_layer_fused",
                 "ggcn_layer_fused_prebias", "ggcn_linear_bf16", "ggcn_aggregate", "ggcn_block_fused")
COUNTED = LAYER_ENTRIES + ("ggcn_block_fused_bf16", "ggcn_aggregate_bf16", "ggcn_overlap_reduce", "ggcn_dense_head")


def _adj(B, T, seed, weighted=False, directed=False):
    from ed_gated_gcn_amd import synth
    rng = np.random.default_rng(seed)
    a = synth.dependency_batch(B, T, 3.5, seed=seed, lengths=rng.integers(max(1, T // 3), T + 1, size=B)).astype(np.float32)
    if directed:
        a = np.triu(a)
    if weighted:
        a = a * rng.uniform(0.25, 2.0, size=a.shape).astype(np.float32)
    return torch.from_numpy(a)


def _layer(pkg, dev, K, F, seed, precision="bf16x3", bias=True, block=True):
    from ed_gated_gcn_amd import synth
    w, b = synth.layer_params(K, F, seed=seed)
    return make_layer(pkg, dev, w, b if bias else None, precision=precision, bf16_block=block)


def _x(B, T, K, dev, seed, pad=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, K + pad, generator=g).to(torch.bfloat16).to(dev)
    return x[:, :, :K] if pad else x


def _gates(B, H, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, H, generator=g).to(dev), torch.rand(B, H, generator=g).to(dev)


def _ref(x, adj, g1, g2, gc1, gc2):
    d = lambda t: None if t is None else t.detach().double()   # noqa: E731
    return ref_dense.gated_block(x.double(), adj.to(x.device).double(), d(g1), d(g2), d(gc1.weight), d(gc1.bias), d(gc2.weight),
                                 d(gc2.bias), dtype=torch.float64)


def _setup(pkg, dev, B, T, H, seed=31, precision="bf16x3", bias1=True, bias2=True, pad=0, directed=False, block=True):
    gc1 = _layer(pkg, dev, H, H, seed=seed, precision=precision, bias=bias1, block=block)
    gc2 = _layer(pkg, dev, H, H, seed=seed + 1, precision=precision, bias=bias2, block=block)
    x, adj = _x(B, T, H, dev, seed=seed + 2, pad=pad), _adj(B, T, seed=seed + 3, directed=directed)
    g1, g2 = _gates(B, H, dev, seed + 4)
    csr = gc1._as_csr(adj.to(dev), x)
    return gc1, gc2, x, adj, csr, g1, g2


# ---------------------------------------------------------------- 1. every output of the one launch vs float64
CASES = {
    "64x31x256": dict(B=64, T=31, H=256),
    "4096x32x768": dict(B=4096, T=32, H=768),              # whole tiles
    "13x32x256": dict(B=13, T=32, H=256),                  # ragged last tile
    "7x17x300": dict(B=7, T=17, H=300),                    # K % 8 != 0: no 16-byte rows of X, a ragged column tile
    "5x9x302": dict(B=5, T=9, H=302),                      # K % 4 != 0, F % 4 != 0: element loads and element stores
    "noncontiguous": dict(B=16, T=29, H=256, pad=3),       # row stride K + 3: element loads
    "gc1_no_bias": dict(B=64, T=31, H=256, bias1=False),   # mid = zeros
    "gc2_no_bias": dict(B=64, T=31, H=256, bias2=False),
    "directed": dict(B=32, T=31, H=256, directed=True),    # triangular adjacency
}


@pytest.mark.parametrize("case", list(CASES))
def test_block_all_outputs_vs_float64(pkg, dev, case, monkeypatch):
    from ed_gated_gcn_amd.gated_block import takes_bf16_block_path
    gc1, gc2, x, adj, csr, g1, g2 = _setup(pkg, dev, **CASES[case])
    if CASES[case].get("pad"):
        assert not x.is_contiguous()
    assert takes_bf16_block_path(x, csr, gc1, gc2)
    calls = count_calls(monkeypatch, COUNTED)
    with torch.no_grad():
        r = pkg.gated_gcn_block(x, csr, g1, g2, gc1, gc2, want_gcn1=True)
    assert calls["ggcn_block_fused_bf16"] == 1 and calls["ggcn_overlap_reduce"] == 1
    assert all(calls[n] == 0 for n in LAYER_ENTRIES), calls
    ref = _ref(x, adj, g1, g2, gc1, gc2)
    for k in ("gcn1", "x1", "y1", "xy", "x", "out"):
        assert r[k].dtype == torch.float32 and r[k].shape == ref[k].shape, k
        _gate(r[k], ref[k], "%s %s" % (case, k))
    with torch.no_grad():
        r2 = pkg.gated_gcn_block(x, csr, g1, g2, gc1, gc2)   # gcn1 only on request; the other outputs are the same bits
    assert r2["gcn1"] is None and calls["ggcn_block_fused_bf16"] == 2
    for k in ("x1", "y1", "xy", "x", "out"):
        assert torch.equal(r2[k], r[k]), k


def test_empty_batch(pkg, dev):
    gc1, gc2, x, adj, csr, g1, g2 = _setup(pkg, dev, 4, 17, 64)
    with torch.no_grad():
        r = pkg.gated_gcn_block(x[:0], adj[:0].to(dev), g1[:0], g2[:0], gc1, gc2, want_gcn1=True)
    assert r["out"].shape == (0, 64) and r["x"].shape == (0, 17, 64) and r["gcn1"].shape == (0, 17, 64)
    assert all(r[k].dtype == torch.float32 for k in ("gcn1", "x1", "y1", "xy", "x", "out"))


# ---------------------------------------------------------------- 2. every split precision means the bf16 pair form
@pytest.mark.parametrize("precision", ["f16mx8", "f16mx6"])
def test_every_split_precision_is_the_bf16x3_block(pkg, dev, precision):
    ref_l = _setup(pkg, dev, 64, 31, 256)
    gc1, gc2, x, adj, csr, g1, g2 = _setup(pkg, dev, 64, 31, 256, precision=precision)
    with torch.no_grad():
        a = pkg.gated_gcn_block(x, csr, g1, g2, gc1, gc2, want_gcn1=True)
        b = pkg.gated_gcn_block(x, csr, g1, g2, ref_l[0], ref_l[1], want_gcn1=True)
    for k in ("gcn1", "x1", "y1", "xy", "x", "out"):
        assert torch.equal(a[k], b[k]), k


# ---------------------------------------------------------------- 3. the eval forms
@pytest.mark.parametrize("B,T,H", [(64, 31, 256), (4096, 32, 768), (13, 32, 256), (7, 17, 300)])
def test_eval_form_is_the_full_blocks_bit_for_bit(pkg, dev, B, T, H, monkeypatch):
    gc1, gc2, x, adj, csr, g1, g2 = _setup(pkg, dev, B, T, H)
    calls = count_calls(monkeypatch, COUNTED)
    with torch.no_grad():
        full = pkg.gated_gcn_block(x, csr, g1, g2, gc1, gc2)
        ev = pkg.gated_gcn_block(x, csr, g1, g2, gc1, gc2, want=("out",))
        ev_nog1 = pkg.gated_gcn_block(x, csr, None, g2, gc1, gc2, want=("out",))   # the eval form never reads gate1
        xo = pkg.gated_gcn_block(x, csr, g1, g2, gc1, gc2, want=("x", "out"))
    assert calls["ggcn_block_fused_bf16"] == 4 and calls["ggcn_overlap_reduce"] == 1
    assert all(calls[n] == 0 for n in LAYER_ENTRIES), calls
    for r in (ev, ev_nog1):
        assert all(r[k] is None for k in ("x1", "y1", "xy", "x", "gcn1"))
        assert torch.equal(r["out"], full["out"])
    assert all(xo[k] is None for k in ("x1", "y1", "xy", "gcn1"))
    assert torch.equal(xo["out"], full["out"]) and torch.equal(xo["x"], full["x"])
    _gate(ev["out"], _ref(x, adj, g1, g2, gc1, gc2)["out"], "eval out")


# ---------------------------------------------------------------- 4. the dense head finishes the regulariser
def test_dense_head_two_launches(pkg, dev, monkeypatch):
    B, T, H, C = 64, 31, 256, 34
    gc1, gc2, x, adj, csr, g1, g2 = _setup(pkg, dev, B, T, H)
    wt = (torch.randn(H, C, generator=torch.Generator().manual_seed(7)) / H ** 0.5).to(dev)
    bias = torch.randn(C, generator=torch.Generator().manual_seed(8)).to(dev)
    calls = count_calls(monkeypatch, COUNTED)
    with torch.no_grad():
        r = pkg.gated_gcn_block(x, csr, g1, g2, gc1, gc2, dense_head=(wt, bias))
    assert calls["ggcn_block_fused_bf16"] == 1 and calls["ggcn_dense_head"] == 1 and calls["ggcn_overlap_reduce"] == 0
    assert sum(calls.values()) == 2, calls
    ref = _ref(x, adj, g1, g2, gc1, gc2)
    _gate(r["logits"], ref["out"] @ wt.double() + bias.double(), "logits")
    _gate(r["xy"], ref["xy"], "xy")
    for k in ("x1", "y1", "x", "out"):
        _gate(r[k], ref[k], k)


# ---------------------------------------------------------------- 5. determinism, graph capture
def test_two_calls_and_a_captured_replay_are_bit_identical(pkg, dev):
    from ed_gated_gcn_amd.graphs import CapturedGatedBlock
    gc1, gc2, x, adj, csr, g1, g2 = _setup(pkg, dev, 256, 31, 256)
    with torch.no_grad():
        a = pkg.gated_gcn_block(x, csr, g1, g2, gc1, gc2)
        b = pkg.gated_gcn_block(x, csr, g1, g2, gc1, gc2)
    for k in ("x1", "y1", "xy", "x", "out"):
        assert torch.equal(a[k], b[k]), k
    cap = CapturedGatedBlock(x, csr, g1, g2, gc1, gc2)
    x2, (h1, h2) = _x(256, 31, 256, dev, seed=77), _gates(256, 256, dev, 78)
    with torch.no_grad():
        eager = pkg.gated_gcn_block(x2, csr, h1, h2, gc1, gc2)
    rep = cap(x2, h1, h2)
    torch.cuda.synchronize()
    for k in ("x1", "y1", "xy", "x", "out"):
        assert torch.equal(rep[k], eager[k]), k


# ---------------------------------------------------------------- 6. off by default; one_launch=False
def test_option_off_and_one_launch_false_keep_todays_launches(pkg, dev, monkeypatch):
    from ed_gated_gcn_amd.gated_block import takes_bf16_block_path
    gc1, gc2, x, adj, csr, g1, g2 = _setup(pkg, dev, 64, 31, 256)
    fresh = pkg.GraphConvolution(256, 256)
    assert fresh.bf16_block is False                       # the default
    calls = count_calls(monkeypatch, COUNTED)
    with torch.no_grad():
        on = pkg.gated_gcn_block(x, csr, g1, g2, gc1, gc2)
        two = pkg.gated_gcn_block(x, csr, g1, g2, gc1, gc2, one_launch=False)
    assert calls["ggcn_block_fused_bf16"] == 1 and calls["ggcn_layer_fused_bf16"] == 1 and calls["ggcn_layer_fused"] == 1
    gc1.bf16_block = gc2.bf16_block = False
    assert not takes_bf16_block_path(x, csr, gc1, gc2)
    for n in calls:
        calls[n] = 0
    with torch.no_grad():
        off = pkg.gated_gcn_block(x, csr, g1, g2, gc1, gc2)
        off_ev = pkg.gated_gcn_block(x, csr, g1, g2, gc1, gc2, want=("out",))
    assert calls["ggcn_block_fused_bf16"] == 0 and calls["ggcn_aggregate_bf16"] == 0
    assert calls["ggcn_layer_fused_bf16"] == 2 and calls["ggcn_layer_fused"] == 2
    for k in ("x1", "y1", "xy", "x", "out"):
        assert torch.equal(off[k], two[k]), k              # one_launch=False IS the default path
    _gate(off_ev["out"], off["out"], "off, want=out")
    ref = _ref(x, adj, g1, g2, gc1, gc2)
    for k in ("x1", "y1", "xy", "x", "out"):
        _gate(off[k], ref[k], "off " + k)
        _gate(on[k], ref[k], "on " + k)


# ---------------------------------------------------------------- 7. autograd keeps the two layer launches
def test_training_with_the_option_on_takes_two_layer_launches(pkg, dev, monkeypatch):
    gc1, gc2, x, adj, csr, g1, g2 = _setup(pkg, dev, 64, 31, 256)
    calls = count_calls(monkeypatch, COUNTED)
    g1r, g2r = g1.clone().requires_grad_(), g2.clone().requires_grad_()
    rt = pkg.gated_gcn_block(x, csr, g1r, g2r, gc1, gc2)
    assert calls["ggcn_block_fused_bf16"] == 0 and calls["ggcn_layer_fused_bf16"] == 1 and calls["ggcn_layer_fused"] >= 1
    (rt["out"].sum() + rt["xy"]).backward()
    w = [t.detach().double().requires_grad_() for t in (g1, g2, gc1.weight, gc1.bias, gc2.weight, gc2.bias)]
    rr = ref_dense.gated_block(x.double(), adj.to(dev).double(), *w, dtype=torch.float64)
    (rr["out"].sum() + rr["xy"]).backward()
    for got, ref64, what in ((g1r.grad, w[0].grad, "d gate1"), (g2r.grad, w[1].grad, "d gate2"), (gc1.weight.grad, w[2].grad, "dW1"),
                             (gc1.bias.grad, w[3].grad, "db1"), (gc2.weight.grad, w[4].grad, "dW2"), (gc2.bias.grad, w[5].grad, "db2")):
        _gate(got, ref64, what)


# ---------------------------------------------------------------- 8. graphs of 33..256 nodes: the folded eval form
def _aggregate_pair(dev, x, csr):
    """(ggcn_aggregate_bf16 on x, ggcn_aggregate on x.float()): Z [B*T, K] each."""
    from ed_gated_gcn_amd import _capi
    lib = _capi.load_library()
    B, T, K = x.shape
    x2d = x.reshape(B * T, K)
    xf = x.float().contiguous().view(B * T, K)
    zb = torch.full((B * T, K), float("nan"), dtype=torch.float32, device=dev)
    zf = torch.full((B * T, K), float("nan"), dtype=torch.float32, device=dev)
    st = _capi.stream_of(dev)
    _capi.check(lib.ggcn_aggregate_bf16(_capi.ptr(x2d), x2d.stride(0), _capi.ptr(csr.rowptr), _capi.ptr(csr.colidx), _capi.ptr(csr.vals),
                                        B, T, K, _capi.ptr(zb), K, st), "ggcn_aggregate_bf16")
    _capi.check(lib.ggcn_aggregate(_capi.ptr(xf), K, _capi.ptr(csr.rowptr), _capi.ptr(csr.colidx), _capi.ptr(csr.vals), None, B, T, K,
                                   None, None, None, _capi.ptr(zf), K, None, None, st), "ggcn_aggregate")
    torch.cuda.synchronize()
    return zb, zf


@pytest.mark.parametrize("B,T,H", [(8, 100, 256), (4, 231, 256), (16, 60, 256)])
@pytest.mark.parametrize("want", [("out",), ("x", "out")])
def test_folded_eval_of_longer_graphs(pkg, dev, B, T, H, want, monkeypatch):
    from ed_gated_gcn_amd.gated_block import takes_bf16_folded_eval_path
    gc1, gc2, x, adj, csr, g1, g2 = _setup(pkg, dev, B, T, H)
    assert takes_bf16_folded_eval_path(x, csr, gc1, gc2)
    zb, zf = _aggregate_pair(dev, x, csr)
    assert torch.equal(zb, zf)
    _gate(zb.view(B, T, H), torch.bmm(adj.to(dev).double(), x.double()) / (adj.to(dev).double().sum(2, keepdim=True) + 1), "Z")
    calls = count_calls(monkeypatch, COUNTED)
    with torch.no_grad():
        r = pkg.gated_gcn_block(x, csr, g1, g2, gc1, gc2, want=want)
    assert calls["ggcn_aggregate_bf16"] == 1 and calls["ggcn_layer_fused_prebias"] == 1
    assert sum(calls.values()) == 2, calls                 # no ggcn_layer_fused_bf16_wide, no ggcn_linear_bf16: W1 is never multiplied
    ref = _ref(x, adj, g1, g2, gc1, gc2)
    assert all(r[k] is None for k in ("x1", "y1", "xy", "gcn1"))
    for k in want:
        assert r[k].dtype == torch.float32
        _gate(r[k], ref[k], "folded " + k)
    if "x" not in want:
        assert r["x"] is None
    # the float32 folded form on x.float() with bf16x3 layers: the same Z, the same launch
    f1, f2 = _layer(pkg, dev, H, H, seed=31, block=False), _layer(pkg, dev, H, H, seed=32, block=False)
    f1.fused_max_t = f2.fused_max_t = 256
    with torch.no_grad():
        rf = pkg.gated_gcn_block(x.float(), adj.to(dev), g1, g2, f1, f2, want=want)
    assert calls["ggcn_aggregate"] == 1 and calls["ggcn_layer_fused_prebias"] == 2
    for k in want:
        assert torch.equal(r[k], rf[k]), k
    # layers that name f16mx8 still run the folded launch in bf16x3 (bf16 features acquire no fp16 range contract)
    h1, h2 = _layer(pkg, dev, H, H, seed=31, precision="f16mx8"), _layer(pkg, dev, H, H, seed=32, precision="f16mx8")
    with torch.no_grad():
        rh = pkg.gated_gcn_block(x, csr, g1, g2, h1, h2, want=want)
    for k in want:
        assert torch.equal(r[k], rh[k]), k


@pytest.mark.parametrize("B,T,K,pad,weighted", [(3, 50, 100, 0, False), (3, 40, 90, 0, False), (5, 33, 256, 8, False), (4, 48, 256, 0, False),
                                                  (5, 70, 256, 3, False), (4, 100, 256, 0, True), (4, 20, 64, 0, True),
                                                  (2, 256, 768, 0, False)])
def test_aggregate_bf16_equals_aggregate_on_the_float32_copy(pkg, dev, B, T, K, pad, weighted):
    """Every load form (16-, 8- and 2-byte), both launch shapes (tiled up to 48 nodes, chunked beyond), 0/1 and weighted."""
    x = _x(B, T, K, dev, seed=61, pad=pad)
    adj = _adj(B, T, seed=62, weighted=weighted)
    csr = pkg.BatchedCSR.from_dense(adj.to(dev))
    assert csr.is_binary == (not weighted)
    zb, zf = _aggregate_pair(dev, x, csr)
    assert torch.equal(zb, zf)
    a = adj.to(dev).double()
    _gate(zb.view(B, T, K), torch.bmm(a, x.double()) / (a.sum(2, keepdim=True) + 1), "Z")


def test_folded_eval_off_by_default(pkg, dev, monkeypatch):
    gc1, gc2, x, adj, csr, g1, g2 = _setup(pkg, dev, 8, 100, 256, block=False)
    calls = count_calls(monkeypatch, COUNTED)
    with torch.no_grad():
        pkg.gated_gcn_block(x, csr, g1, g2, gc1, gc2, want=("out",))
    assert calls["ggcn_aggregate_bf16"] == 0 and calls["ggcn_layer_fused_prebias"] == 0
    assert calls["ggcn_layer_fused_bf16_wide"] == 1 and calls["ggcn_layer_fused"] == 1


# ---------------------------------------------------------------- 9. the classifiers under bf16 autocast
@pytest.mark.parametrize("cls_name", ["GatedGCNEventDetector", "GatedGCNEventDetector54", "GCNEventDetectorNoGate"])
def test_classifier_under_bf16_autocast_with_the_block(pkg, dev, cls_name, monkeypatch):
    """Logits within 2^-6 * max(1, max|logits|) of the same model with the option off: the autocast `dense` rounds its input and
    its output to bf16 (2^-8 relative each), so a last-bit change of `out` may move a logit by a few bf16 ulps; a wiring error
    moves it by O(1)."""
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(5)
    inputs, NCLS = _classifier_batch(dev)
    opt = types.SimpleNamespace(device=dev, dropout=0.25, polarities_dim=NCLS, ggcn_bf16_block=True)
    model = getattr(pkg, cls_name)(pkg.LegacyBertAdapter(transformers.BertModel(transformers.BertConfig())), opt)
    ref_dense.reset_params_like_train([p for n, p in model.named_parameters() if not n.startswith("bert.")],
                                      torch.Generator().manual_seed(9))
    model = model.to(dev).eval()
    assert model.gc1.bf16_block and model.gc2.bf16_block
    calls = count_calls(monkeypatch, COUNTED)
    for logits_only in (False, True):
        model.eval_logits_only = logits_only
        res = {}
        for on in (True, False):
            model.gc1.bf16_block = model.gc2.bf16_block = on
            for n in calls:
                calls[n] = 0
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                res[on] = model(inputs)
            assert torch.isfinite(res[on][0].float()).all()
            if not logits_only:
                assert all(torch.isfinite(torch.as_tensor(t).float()).all() for t in res[on][1:])
            assert calls["ggcn_block_fused_bf16"] == (1 if on else 0), (on, calls)
            assert (calls["ggcn_layer_fused_bf16"] == 0) == on, (on, calls)
        a, b = res[True][0].double(), res[False][0].double()
        tol = 2.0 ** -6 * max(1.0, float(b.abs().max()))
        err = float((a - b).abs().max())
        print("%s logits_only=%s: max|logits on - off| %.3g (bound %.3g)" % (cls_name, logits_only, err, tol))
        assert err <= tol
