"""The gradient with respect to a real-valued adjacency on the GPU (run with ``-m gpu -s`` on an MI355X to see the figures).

First half: ``ggcn_adjacency_grad`` through the C ABI against the float64 closed form of the same float32 inputs,

    G_ij = inv_i (dY_i . H_j),   c_i = inv_i sum_k A_ik G_ik,   dA_ij = G_ij - c_i   for every (i, j),

in a hostile state: strided operands whose pad columns are NaN, the row after the last graph's last row NaN, ``d_adj`` pre-filled
with NaN, each call made twice and compared bit for bit.  Gate: the project's float32-gradient gate, 2e-4 * max|ref|.

Second half: ``GraphConvolution.forward_gated`` and ``gated_gcn_block`` with ``adj.requires_grad_()`` against
``oracle/backward_ref.py`` (float64, torch autograd with a float64 ``adj`` leaf) on its recipes: ``adj.grad`` at 2e-4 * max|ref|
(5e-4 under gate dropout and for the block), every other gradient at the gates of ``tests/test_gpu_backward.py`` AND bit-identical
to a run of the same case with a non-differentiable ``adj`` under ``GGCN_BACKWARD_TWO_PASS=1`` (the same kernels: asking for the
adjacency gradient moves nothing else).  Near-tie pools are masked by ``backward_ref.pool_tie_mask`` as everywhere; at most 3 % of
a case's pools, asserted in every case.
"""
import pytest
import torch

from oracle import backward_ref as br
from oracle import gates
from oracle.gpu_support import count_calls, dev, drop_mask as _drop_mask, make_layer, pkg  # noqa: F401

pytestmark = pytest.mark.gpu

NAN = float("nan")
_hostile, _close32, _gate, _gate_dx = gates.hostile, gates.close32, gates.gate, gates.gate_dx
ADJ_GRAD = "ggcn_adjacency_grad"
MMA, AGG, GPB, GPB_DROP, AGG_T = ("ggcn_gate_pool_backward_mma", "ggcn_gate_pool_backward_agg", "ggcn_gate_pool_backward",
                                   "ggcn_gate_pool_backward_drop", "ggcn_aggregate_t")
COUNTED = (ADJ_GRAD, MMA, AGG, GPB, GPB_DROP, AGG_T, "ggcn_linear_scaled", "ggcn_linear", "ggcn_linear_out_bf16", "ggcn_dweight",
           "ggcn_dweight_bf16", "ggcn_colsum", "ggcn_layer_fused", "ggcn_layer_fused_drop", "ggcn_layer_fused_bf16",
           "ggcn_layer_fused_bf16_drop", "ggcn_layer_fused_bf16_wide", "ggcn_layer_fused_weighted", "ggcn_linear_bf16", "ggcn_aggregate")


def closed_form64(dy, hidden, adj):
    """dA [B,T,T] in float64 from float32 dY, H [B,T,F] and A [B,T,T]."""
    dy, hidden, adj = dy.double(), hidden.double(), adj.double()
    inv = 1.0 / (adj.sum(2) + 1.0)
    g = inv[:, :, None] * torch.einsum("bif,bjf->bij", dy, hidden)
    return g - (inv * (adj * g).sum(2))[:, :, None]


# ================================================================ 1. the kernel through the C ABI
SHAPES = [(1, 1, 8), (3, 5, 8), (5, 17, 20), (6, 20, 30), (4, 31, 96), (4, 32, 256), (3, 33, 64), (2, 64, 40), (2, 65, 48),
          (2, 100, 300), (2, 129, 64), (1, 231, 256), (1, 256, 32), (1, 257, 24), (1, 512, 16)]
KINDS = ("tree", "directed", "isolated", "weighted")
# (B, T, F, graph, pad_dy, pad_h): the kinds rotated over the shapes, ldy = F + 3 and ldh = F + 1 on every second case, len1 once,
# and one case whose padded rows stay 16-byte aligned (ld = F + 4, F + 8: the 16-byte loads next to NaN pad columns)
SWEEP = [(B, T, F, KINDS[n % 4], 3 * (n % 2), n % 2) for n, (B, T, F) in enumerate(SHAPES)] + [
    (5, 17, 20, "len1", 3, 1), (3, 33, 64, "weighted", 4, 8)]


def _abi_case(pkg, dev, B, T, F, graph, pad_dy, pad_h, seed):
    from ed_gated_gcn_amd import _capi
    lib = pkg.load_library()
    adj = br.case_adjacency(B, T, seed, graph).to(dev)
    csr = pkg.BatchedCSR.from_dense(adj)
    assert csr.is_binary == (graph != "weighted")
    inv = csr.inv_denominators()
    g = torch.Generator(device=dev).manual_seed(seed + 1)
    dy = torch.randn(B * T, F, device=dev, generator=g)
    hidden = torch.randn(B * T, F, device=dev, generator=g)
    dyb, hb = _hostile(dy, pad_dy), _hostile(hidden, pad_h)
    outs = []
    for _ in range(2):
        d_adj = torch.full((B, T, T), NAN, device=dev)
        _capi.check(lib.ggcn_adjacency_grad(_capi.ptr(dyb), F + pad_dy, _capi.ptr(hb), F + pad_h, _capi.ptr(inv), _capi.ptr(csr.rowptr),
                                            _capi.ptr(csr.colidx), _capi.ptr(csr.vals), B, T, F, _capi.ptr(d_adj), _capi.stream_of(dev)),
                    ADJ_GRAD)
        outs.append(d_adj)
    torch.cuda.synchronize()
    ref = closed_form64(dy.view(B, T, F), hidden.view(B, T, F), adj)
    return outs, ref


@pytest.mark.parametrize("B,T,F,graph,pad_dy,pad_h", SWEEP)
def test_adjacency_grad_vs_float64(pkg, dev, B, T, F, graph, pad_dy, pad_h):
    outs, ref = _abi_case(pkg, dev, B, T, F, graph, pad_dy, pad_h, seed=11 * T + F)
    what = "%dx%dx%d %s ldy=F+%d ldh=F+%d" % (B, T, F, graph, pad_dy, pad_h)
    assert not bool(torch.isnan(outs[0]).any()), "%s: NaN in d_adj" % what
    assert torch.equal(outs[0], outs[1]), "%s: two runs differ" % what
    scale = float(ref.abs().max())
    err = float((outs[0].double() - ref).abs().max())
    print("dA %s: max|diff| %.3g vs scale %.3g (gate %.3g)" % (what, err, scale, 2e-4 * scale))
    assert err == err and err <= 2e-4 * scale, "%s: max|diff| %.3g vs scale %.3g" % (what, err, scale)


def test_adjacency_grad_keeps_the_float32_exponent_range(pkg, dev):
    """Gradients have no range contract: dY at 3e-12 and at 2e9 of its scale gives the same relative error (bf16 planes)."""
    from ed_gated_gcn_amd import _capi
    lib = pkg.load_library()
    B, T, F = 3, 40, 64
    adj = br.case_adjacency(B, T, 5, "weighted").to(dev)
    csr = pkg.BatchedCSR.from_dense(adj)
    g = torch.Generator(device=dev).manual_seed(6)
    dy0, hidden = torch.randn(B * T, F, device=dev, generator=g), torch.randn(B * T, F, device=dev, generator=g)
    for scale in (3e-12, 2e9):
        dy = dy0 * scale
        d_adj = torch.full((B, T, T), NAN, device=dev)
        _capi.check(lib.ggcn_adjacency_grad(_capi.ptr(dy), F, _capi.ptr(hidden), F, _capi.ptr(csr.inv_denominators()),
                                            _capi.ptr(csr.rowptr), _capi.ptr(csr.colidx), _capi.ptr(csr.vals), B, T, F, _capi.ptr(d_adj),
                                            _capi.stream_of(dev)), ADJ_GRAD)
        ref = closed_form64(dy.view(B, T, F), hidden.view(B, T, F), adj)
        err, top = float((d_adj.double() - ref).abs().max()), float(ref.abs().max())
        print("dA scale %g: max|diff| %.3g vs scale %.3g" % (scale, err, top))
        assert err == err and err <= 2e-4 * top


# ================================================================ 2. through the module under autograd
def _layer(pkg, dev, w, b, precision, fused_max_t=None):
    return make_layer(pkg, dev, w, b, precision=precision, fused_max_t=fused_max_t)


STREAMS = (0, 1, 2)      # the block's layer-1 streams: all three gates, the store gate undropped
_REF = {}                # (name, bf16) -> the float64 reference of a case, computed once and left unchanged


def _reference(pkg, dev, name, bf16, precision):
    """Inputs on the device, tie-masked upstream gradients and the float64 gradients (adj among them) of one recipe."""
    key = (name, bf16, precision if precision == "fp32" else "split")     # (TOL, and with it the tie mask, has two classes)
    if key in _REF:
        return _REF[key]
    _, B, T, K, F, _, _, p = br.RECIPE[name]
    c = {k: (v.to(dev) if v is not None else None) for k, v in br.recipe_inputs(name, bf16=bf16).items()}
    dropout = (p, 2 ** 40 + 99, STREAMS) if p else None
    keep = None
    if dropout is not None:
        keep = tuple(None if s == 0 else _drop_mask(pkg, dev, B * T, F, p, dropout[1], s).view(B, T, F).double() for s in STREAMS)
    ma, mb = br.layer_tie_masks(c["x"], c["adj"], c["w"], c["b"], c["ga"], c["gb"], br.tie_delta(precision, p), keep=keep)
    share = br.masked_share(ma, mb)
    print("%s/%s: %.2f %% of the pools masked" % (name, "bf16" if bf16 else precision, 100 * share))
    assert share <= br.MAX_MASKED
    r1, r2, r3 = c["r1"], c["r2"] * (~ma), c["r3"] * (~mb)
    ref = {k: c[k].double().requires_grad_() for k in ("x", "w", "b", "sg", "ga", "gb", "adj")}
    o64, a64, b64 = br.gated_layer_ref(ref["x"], ref["adj"], ref["w"], ref["b"], ref["sg"], ref["ga"], ref["gb"], keep=keep)
    ((o64 * r1).sum() + (a64 * r2).sum() + (b64 * r3).sum()).backward()
    grads = {k: v.grad.clone() for k, v in ref.items()}
    _REF[key] = (c, (r1, r2, r3), dropout, grads)
    return _REF[key]


def _run(pkg, dev, c, rs, dropout, precision, fused_max_t, adj):
    """forward_gated + backward of the backward tests' loss; returns the gradients of x, w, b and the three gates."""
    m = _layer(pkg, dev, c["w"], c["b"], precision, fused_max_t)
    leaves = {k: c[k].clone().requires_grad_() for k in ("x", "sg", "ga", "gb")}
    out, pa, pb = m.forward_gated(leaves["x"], adj, store_gate=leaves["sg"], pool_gate_a=leaves["ga"], pool_gate_b=leaves["gb"],
                                  want_pool_a=True, want_pool_b=True, dropout=dropout)
    ((out * rs[0]).sum() + (pa * rs[1]).sum() + (pb * rs[2]).sum()).backward()
    torch.cuda.synchronize()
    g = {k: v.grad for k, v in leaves.items()}
    g["w"], g["b"] = m.weight.grad, m.bias.grad
    return g


def _module_case(pkg, dev, monkeypatch, name, precision="f16mx8", bf16=False):
    _, B, T, K, F, _, _, p = br.RECIPE[name]
    what = "%s/%s" % (name, "bf16" if bf16 else precision)
    c, rs, dropout, ref = _reference(pkg, dev, name, bf16, precision)
    fused_max_t = 256 if T > 32 else None      # (as tests/test_gpu_backward.py: one-launch forward up to 256 nodes; dropout needs it)
    calls = count_calls(monkeypatch, COUNTED)
    adj = c["adj"].clone().requires_grad_()
    got = _run(pkg, dev, c, rs, dropout, precision, fused_max_t, adj)
    assert calls[ADJ_GRAD] == 1 and calls[MMA] == 0 and calls[AGG] == 0 and calls[AGG_T] == 1, "%s: %s" % (what, calls)
    assert calls[GPB_DROP if p else GPB] == 1, "%s: %s" % (what, calls)
    # ---- the adjacency gradient: dense, float32 like adj, against float64
    rel = 5e-4 if p else 2e-4
    assert adj.grad is not None and adj.grad.shape == (B, T, T) and adj.grad.dtype == c["adj"].dtype
    assert not bool(torch.isnan(adj.grad).any())
    _close32(adj.grad, ref["adj"], what + " d adj", rel)
    # ---- every other gradient at its own gate ...
    for k, label in (("x", "dX"), ("w", "dW"), ("b", "db"), ("sg", "d store gate"), ("ga", "d gate a"), ("gb", "d gate b")):
        if k == "x" and bf16:
            _gate_dx(got[k], ref[k])
        elif bf16:
            _gate(got[k], ref[k], label)
        else:
            _close32(got[k], ref[k], label, rel)
    # ---- ... and bit for bit what the two calls give without the adjacency gradient
    monkeypatch.setenv("GGCN_BACKWARD_TWO_PASS", "1")
    before = calls[ADJ_GRAD]
    plain = _run(pkg, dev, c, rs, dropout, precision, fused_max_t, c["adj"])
    assert calls[ADJ_GRAD] == before
    for k in ("x", "w", "b", "sg", "ga", "gb"):
        assert torch.equal(got[k], plain[k]), "%s: asking for d adj moved the gradient of %s" % (what, k)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "f16mx8"])
@pytest.mark.parametrize("name", ["weighted", "square"])
def test_every_precision(pkg, dev, monkeypatch, name, precision):
    _module_case(pkg, dev, monkeypatch, name, precision)


@pytest.mark.parametrize("name", ["directed", "isolated", "ragged17", "f30", "one", "wide33", "wide65", "wide129", "wide231", "long300"])
def test_recipes(pkg, dev, monkeypatch, name):
    _module_case(pkg, dev, monkeypatch, name)


@pytest.mark.parametrize("name", ["drop24", "drop100"])
def test_gate_dropout(pkg, dev, monkeypatch, name):
    _module_case(pkg, dev, monkeypatch, name)


@pytest.mark.parametrize("name", ["weighted", "square", "wide129"])
def test_bfloat16_features(pkg, dev, monkeypatch, name):
    _module_case(pkg, dev, monkeypatch, name, bf16=True)


def test_adjacency_dtype_and_non_leaf(pkg, dev):
    """A float64 adj gets a float64 gradient; a non-leaf adj (a function of trainable edge logits) passes its gradient on."""
    c, rs, dropout, ref = _reference(pkg, dev, "weighted", False, "f16mx8")
    m = _layer(pkg, dev, c["w"], c["b"], "f16mx8")
    a64 = c["adj"].double().requires_grad_()
    m.forward_gated(c["x"], a64)[0].mul(rs[0]).sum().backward()
    assert a64.grad is not None and a64.grad.dtype == torch.float64
    logits = torch.zeros_like(c["adj"]).requires_grad_()
    soft = c["adj"] * torch.sigmoid(logits) * 2.0        # = adj at logits = 0
    m.forward_gated(c["x"], soft)[0].mul(rs[0]).sum().backward()
    assert torch.equal(logits.grad, (a64.grad.float() * c["adj"] * 0.5))


def test_longer_than_512_nodes_raises(pkg, dev):
    """long513: a differentiable adj raises the RuntimeError that names the limit; without it the recipe trains as before."""
    c = {k: (v.to(dev) if v is not None else None) for k, v in br.recipe_inputs("long513").items()}
    m = _layer(pkg, dev, c["w"], c["b"], "f16mx8")
    x = c["x"].clone().requires_grad_()
    with pytest.raises(RuntimeError, match="512"):
        m.forward_gated(x, c["adj"].clone().requires_grad_())
    out, _, _ = m.forward_gated(x, c["adj"])
    (out * c["r1"]).sum().backward()
    assert x.grad is not None and bool(torch.isfinite(x.grad).all()) and m.weight.grad is not None


@pytest.mark.parametrize("name,batch", [("block32", 16), ("block231", 4)])
def test_gated_block(pkg, dev, monkeypatch, name, batch):
    """gated_gcn_block with a differentiable adj: both layers run under autograd and adj.grad is the SUM of their contributions
    (block_ref autograd with a float64 adj leaf), 5e-4 * max|ref| like the block's other gradients."""
    precision = "f16mx8"
    c = {k: v.to(dev) for k, v in br.block_inputs(name, batch=batch).items()}
    B = c["x"].shape[0]
    m1, my, mo = br.block_tie_masks(c["x"], c["adj"], c["g1"], c["g2"], c["w1"], c["b1"], c["w2"], c["b2"], br.tie_delta(precision))
    share = br.masked_share(m1, my, mo)
    print("%s: %.2f %% of the pools masked" % (name, 100 * share))
    assert share <= br.MAX_MASKED
    unmasked, r1, r2 = ~(m1 | my), c["r1"] * (~mo), c["r2"]

    def loss_of(r):
        return (r["out"] * r1).sum() + 0.1 * (r["x"] * r2).sum() + 0.01 * (r["x1"] * r["y1"] * unmasked).sum() / B

    names = ("x", "adj", "g1", "g2", "w1", "b1", "w2", "b2")
    ref = {k: c[k].double().requires_grad_() for k in names}
    loss_of(br.block_ref(*[ref[k] for k in names])).backward()

    gc1, gc2 = _layer(pkg, dev, c["w1"], c["b1"], precision, 256), _layer(pkg, dev, c["w2"], c["b2"], precision, 256)
    xg, g1g, g2g, adj = (c[k].clone().requires_grad_() for k in ("x", "g1", "g2", "adj"))
    calls = count_calls(monkeypatch, COUNTED)
    r = pkg.gated_gcn_block(xg, adj, g1g, g2g, gc1, gc2)
    loss_of(r).backward()
    torch.cuda.synchronize()
    assert calls[ADJ_GRAD] == 2 and calls[GPB] == 2 and calls[AGG_T] == 2 and calls[MMA] == 0, calls
    assert adj.grad is not None and not bool(torch.isnan(adj.grad).any())
    _close32(adj.grad, ref["adj"].grad, name + " d adj", 5e-4)
    got = {"x": xg.grad, "g1": g1g.grad, "g2": g2g.grad, "w1": gc1.weight.grad, "b1": gc1.bias.grad, "w2": gc2.weight.grad,
           "b2": gc2.bias.grad}
    for k in got:
        _close32(got[k], ref[k].grad, "d " + k, 5e-4)


def test_without_an_adjacency_gradient_nothing_changes(pkg, dev, monkeypatch):
    """requires_grad=False: the backward of "square" is the matrix-core pass, the scaled dX, dW and the bias sums, as in
    tests/test_gpu_backward.py, and ggcn_adjacency_grad is never called.  Under no_grad a differentiable adj runs the inference
    launch alone."""
    c, rs, dropout, ref = _reference(pkg, dev, "square", False, "f16mx8")
    calls = count_calls(monkeypatch, COUNTED)
    _run(pkg, dev, c, rs, None, "f16mx8", None, c["adj"])
    want = {k: 0 for k in COUNTED}
    want.update({"ggcn_layer_fused": 1, MMA: 1, "ggcn_linear_scaled": 1, "ggcn_dweight": 1, "ggcn_colsum": 1})
    assert calls == want, {k: v for k, v in calls.items() if v}
    for k in calls:
        calls[k] = 0
    m = _layer(pkg, dev, c["w"], c["b"], "f16mx8")
    adj = c["adj"].clone().requires_grad_()
    with torch.no_grad():
        out, pa, _ = m.forward_gated(c["x"], adj, store_gate=c["sg"], pool_gate_a=c["ga"], want_pool_a=True)
    assert not out.requires_grad and not pa.requires_grad and adj.grad is None
    want = {k: 0 for k in COUNTED}
    want["ggcn_layer_fused"] = 1
    assert calls == want, {k: v for k, v in calls.items() if v}
    # a BatchedCSR has no tensor to differentiate: it behaves as before
    csr = pkg.BatchedCSR.from_dense(c["adj"])
    for k in calls:
        calls[k] = 0
    x = c["x"].clone().requires_grad_()
    m.forward_gated(x, csr)[0].mul(rs[0]).sum().backward()
    assert calls[ADJ_GRAD] == 0 and calls[MMA] == 1 and x.grad is not None
