"""A real-valued adjacency of graphs of 33..128 nodes as ONE launch (``ggcn_layer_fused_weighted_wide`` on
``ggcn_graph_operands_weighted_wide`` blocks; opt-in ``GraphConvolution.weighted_max_t = 128``).  Run with ``-m gpu -s`` on an
MI355X to see the figures.

1. forward against the float64 oracle at the project's parity gate, ``TOL[precision] * max(1, max|y|)``; the distance to
   linear + aggregate is printed, not gated;
2. which entries ran, with the option on and at its default (then: the parent's launches and the parent's bits);
3. the C entry in a hostile state: outputs pre-filled with NaN, operand buffer sized exactly, out = NULL / pools NULL, refusals;
4. a row with rowsum + 1 == 0: the builder's flag, no operand, two launches, the parent's bits;
5. under autograd: the forward takes the new launch, every gradient (adj's among them) stays inside the gates of
   ``tests/test_gpu_adjacency_grad.py``;
6. ``gated_gcn_block`` on a weighted adjacency, both layers through the new launch.
"""
import numpy as np
import pytest
import torch

from oracle import backward_ref as br
from oracle import ref_dense
from oracle.gates import close32 as _close32
from oracle.gpu_support import count_calls, dev, make_layer, pkg  # noqa: F401

pytestmark = pytest.mark.gpu

TOL = br.TOL                                    # the forward parity gate per arithmetic
NAN = float("nan")
WIDE, NARROW, LINEAR, AGGREGATE = "ggcn_layer_fused_weighted_wide", "ggcn_layer_fused_weighted", "ggcn_linear", "ggcn_aggregate"
COUNTED = (WIDE, NARROW, LINEAR, AGGREGATE, "ggcn_layer_fused", "ggcn_graph_operands_weighted_wide", "ggcn_adjacency_grad",
           "ggcn_aggregate_t", "ggcn_gate_pool_backward")


def _layer(pkg, dev, w, b, precision, weighted_max_t=128):
    return make_layer(pkg, dev, w, b, precision=precision, weighted_max_t=weighted_max_t)


def _adjacency(B, T, kind, rng, lens):
    """float32 [B,T,T], zero outside each graph's length: sparse / signed = dependency trees x U(0.05, 2) weights (signed: 20 % of
    them x -0.25), dense = a row-softmax of standard normals over the graph's own nodes."""
    from ed_gated_gcn_amd import synth
    if kind == "dense":
        a = np.zeros((B, T, T), dtype=np.float32)
        for g, n in enumerate(lens):
            z = rng.standard_normal((n, n))
            e = np.exp(z - z.max(1, keepdims=True))
            a[g, :n, :n] = (e / e.sum(1, keepdims=True)).astype(np.float32)
        return a
    a = synth.dependency_batch(B, T, 3.0, seed=B + T, lengths=lens).astype(np.float32)
    wts = rng.uniform(0.05, 2.0, size=a.shape).astype(np.float32)
    if kind == "signed":
        wts *= np.where(rng.random(a.shape) < 0.2, -0.25, 1.0).astype(np.float32)
    return a * wts


# ================================================================ 1. forward against the float64 oracle
CASES = [(5, 33, 64, 64, "sparse"),      # one node in the second block; odd B with two graphs per workgroup
         (3, 64, 256, 256, "dense"),     # full 64-row slot
         (4, 65, 96, 100, "signed"),     # 128-row slot with three blocks; column-tile guard; non-vector row stores
         (2, 96, 34, 20, "sparse"),      # the general main loop
         (7, 47, 64, 96, "dense"),
         (3, 100, 768, 768, "dense"),
         (2, 128, 128, 384, "signed")]
_CASE = {}     # case -> inputs and the float64 reference, computed once and left unchanged


def _case(B, T, K, F, kind):
    from ed_gated_gcn_amd import synth
    key = (B, T, K, F, kind)
    if key not in _CASE:
        rng = np.random.default_rng(B * 1000 + T)
        lens = rng.integers(max(1, T // 3), T + 1, size=B)
        lens[0] = T
        adj = _adjacency(B, T, kind, rng, lens)
        x = rng.standard_normal((B, T, K)).astype(np.float32)
        w, b = synth.layer_params(K, F, seed=3)
        gates = [torch.sigmoid(torch.from_numpy(rng.standard_normal((B, F)).astype(np.float32))) for _ in range(3)]
        t = torch.from_numpy
        y = ref_dense.graph_convolution(t(x).double(), t(adj).double(), t(w).double(), t(b).double(), dtype=torch.float64)
        assert y.dtype == torch.float64
        _CASE[key] = (x, adj, w, b, gates, lens, y)
    return _CASE[key]


@pytest.mark.parametrize("precision", ["bf16x3", "f16mx8"])
@pytest.mark.parametrize("B,T,K,F,kind", CASES)
def test_forward_vs_float64_oracle(pkg, dev, precision, B, T, K, F, kind):
    x, adj, w, b, gates, lens, y = _case(B, T, K, F, kind)
    gs, ga, gb = (g.to(dev) for g in gates)
    m = _layer(pkg, dev, w, b, precision)
    xd, ad = torch.from_numpy(x).to(dev), torch.from_numpy(adj).to(dev)
    csr = pkg.BatchedCSR.from_dense(ad)
    assert not csr.is_binary and m.takes_weighted_path(xd, csr) and not m.takes_fused_path(xd, csr)
    with torch.no_grad():
        out, pa, pb = m.forward_gated(xd, csr, store_gate=gs, pool_gate_a=ga, pool_gate_b=gb, want_pool_a=True, want_pool_b=True)
        plain = m(xd, ad)
        m.fused = False
        out2, pa2, pb2 = m.forward_gated(xd, csr, store_gate=gs, pool_gate_a=ga, pool_gate_b=gb, want_pool_a=True, want_pool_b=True)
    torch.cuda.synchronize()
    scale = max(1.0, float(y.abs().max()))
    tol = TOL[precision] * scale
    g64 = [g.double() for g in gates]
    want = {"plain": (plain, y), "out": (out, y * g64[0][:, None, :]), "pool a": (pa, (y * g64[1][:, None, :]).max(1).values),
            "pool b": (pb, (y * g64[2][:, None, :]).max(1).values)}
    what = "%dx%dx%dx%d %s %s" % (B, T, K, F, kind, precision)
    errs = {k: float((got.double().cpu() - ref).abs().max()) for k, (got, ref) in want.items()}
    two = max(float((out - out2).abs().max()), float((pa - pa2).abs().max()), float((pb - pb2).abs().max()))
    print("%s: scale %.3g gate %.3g | vs float64: %s | vs linear + aggregate: %.3g (%.3g of the scale)" % (
        what, scale, tol, ", ".join("%s %.3g" % kv for kv in errs.items()), two, two / scale))
    for k, (got, ref) in want.items():
        assert got.dtype == torch.float32 and got.shape == ref.shape
        assert errs[k] == errs[k] and errs[k] <= tol, "%s %s: max|diff| %.3g > %.3g" % (what, k, errs[k], tol)


# ================================================================ 2. which launches ran
@pytest.mark.parametrize("precision", ["bf16x3", "f16mx8"])
def test_which_launches_ran(pkg, dev, monkeypatch, precision):
    x, adj, w, b, gates, lens, y = _case(4, 65, 96, 100, "signed")
    gs, ga, gb = (g.to(dev) for g in gates)
    xd, ad = torch.from_numpy(x).to(dev), torch.from_numpy(adj).to(dev)
    kw = dict(store_gate=gs, pool_gate_a=ga, pool_gate_b=gb, want_pool_a=True, want_pool_b=True)
    calls = count_calls(monkeypatch, COUNTED)
    on = _layer(pkg, dev, w, b, precision)
    with torch.no_grad():
        on.forward_gated(xd, ad, **kw)
    assert calls[WIDE] == 1 and calls[LINEAR] == 0 and calls[AGGREGATE] == 0 and calls[NARROW] == 0, calls
    assert calls["ggcn_graph_operands_weighted_wide"] == 1
    with torch.no_grad():
        on.forward_gated(xd, ad, **kw)          # the same adjacency tensor: its operand blocks are cached
    assert calls[WIDE] == 2 and calls["ggcn_graph_operands_weighted_wide"] == 1, calls
    for k in calls:
        calls[k] = 0
    default = _layer(pkg, dev, w, b, precision, weighted_max_t=32)
    unfused = _layer(pkg, dev, w, b, precision, weighted_max_t=32)
    unfused.fused = False
    with torch.no_grad():
        got = default.forward_gated(xd, ad, **kw)
        assert calls[WIDE] == 0 and calls[LINEAR] == 1 and calls[AGGREGATE] == 1 and calls["ggcn_graph_operands_weighted_wide"] == 0, calls
        ref = unfused.forward_gated(xd, ad, **kw)
    for g, r in zip(got, ref):
        assert torch.equal(g, r)
    assert not default.takes_weighted_path(xd, pkg.BatchedCSR.from_dense(ad))


# ================================================================ 3. the C entry in a hostile state
def _decode(ops, B, T):
    """The device blocks back as M [B, 32 W, 32 W] in float64 (hi + lo), by the documented layout."""
    W = -(-T // 32)
    raw = ops.cpu().numpy().view(np.uint16).reshape(B, W, W, 2, 2, 64, 8)          # [g][io][ii][plane][ks][lane][j]
    val = (raw.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    val = val[:, :, :, 0] + val[:, :, :, 1]                                          # hi + lo: [g][io][ii][ks][lane][j]
    M = np.zeros((B, 32 * W, 32 * W))
    lane, j = np.meshgrid(np.arange(64), np.arange(8), indexing="ij")
    r, h = lane & 31, lane >> 5
    for io in range(W):
        for ii in range(W):
            for ks in range(2):
                col = 16 * ks + 8 * (j >> 2) + 4 * h + (j & 3)
                M[:, 32 * io + r, 32 * ii + col] = val[:, io, ii, ks]
    return M


@pytest.mark.parametrize("T", [33, 64, 65, 96, 97, 128])
def test_c_entries_in_a_hostile_state(pkg, dev, T):
    from ed_gated_gcn_amd import _capi, synth
    lib = pkg.load_library()
    p, st = _capi.ptr, _capi.stream_of(dev)
    B, K, F = 3, 64, 72
    rng = np.random.default_rng(T)
    lens = np.array([T, max(1, T // 3), T - 1])
    adj = _adjacency(B, T, "signed", rng, lens)
    for g, n in enumerate(lens):                         # rows past a graph's length without a single edge (not even the self loop)
        adj[g, n:, :] = 0.0
        adj[g, :, n:] = 0.0
    csr = pkg.BatchedCSR.from_dense(torch.from_numpy(adj).to(dev))
    # ---- the builder: exactly _bytes, every byte written, values = w / (rowsum + 1), zero rows and columns past T
    nbytes = lib.ggcn_graph_operands_weighted_wide_bytes(B, T)
    buf = torch.full((nbytes + 64,), 0xFF, dtype=torch.uint8, device=dev)              # 0xFFFF = a bf16 NaN; 64 guard bytes
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    _capi.check(lib.ggcn_graph_operands_weighted_wide(p(csr.rowptr), p(csr.colidx), p(csr.vals), B, T, p(buf), p(flag), st), "builder")
    torch.cuda.synchronize()
    assert int(flag.item()) == 0 and bool((buf[nbytes:] == 0xFF).all()), "T=%d: the builder wrote past _bytes" % T
    ops = buf[:nbytes]
    M = _decode(ops, B, T)
    assert not np.isnan(M).any()
    want = adj.astype(np.float64) / (adj.astype(np.float64).sum(2, keepdims=True) + 1.0)
    assert np.abs(M[:, :T, :T] - want).max() <= 2.0 ** -16 * np.abs(want).max()         # two bf16 parts: 2^-17 relative, and float32 D
    assert not M[:, T:, :].any() and not M[:, :, T:].any()
    # ---- the layer: NaN everywhere it may write, one guard row after the last
    x = torch.from_numpy(rng.standard_normal((B * T, K)).astype(np.float32)).to(dev)
    w, b = synth.layer_params(K, F, seed=5)
    m = _layer(pkg, dev, w, b, "f16mx8")
    gs, ga, gb = (torch.sigmoid(torch.from_numpy(rng.standard_normal((B, F)).astype(np.float32))).to(dev) for _ in range(3))
    y = ref_dense.graph_convolution(x.view(B, T, K).double().cpu(), torch.from_numpy(adj).double(), torch.from_numpy(w).double(),
                                    torch.from_numpy(b).double(), dtype=torch.float64)
    tol = TOL["f16mx8"] * max(1.0, float(y.abs().max()))
    for precision in ("f16mx8", "bf16x3"):
        m.precision = precision
        with torch.cuda.device(dev):
            pack = m._packed_weight(lib, st, precision=precision)
        # ldo = F + 3: rows at odd offsets, the scalar store form; F + 4: 16-byte rows, the vector store form; pad columns stay NaN
        for with_out, with_pools, ldo in ((True, True, F + 3), (True, True, F + 4), (False, True, F), (True, False, F + 4)):
            out = torch.full((B * T + 1, ldo), NAN, device=dev)
            pa, pb = torch.full((B + 1, F), NAN, device=dev), torch.full((B + 1, F), NAN, device=dev)
            rc = lib.ggcn_layer_fused_weighted_wide(p(x), K, p(pack), p(ops), p(m.bias.detach()), B, T, K, F, p(gs), p(ga), p(gb),
                                                    p(out) if with_out else None, ldo, p(pa) if with_pools else None,
                                                    p(pb) if with_pools else None, _capi.PREC[precision], st)
            _capi.check(rc, WIDE)
            torch.cuda.synchronize()
            what = "T=%d %s out=%s pools=%s" % (T, precision, with_out, with_pools)
            if with_out:
                got = out[:B * T, :F].view(B, T, F)
                assert not bool(torch.isnan(got).any()), what + ": NaN in out"
                assert bool(torch.isnan(out[B * T]).all()) and bool(torch.isnan(out[:, F:]).all()), what + ": wrote outside [B*T, F]"
                assert float((got.double().cpu() - y * gs.double().cpu()[:, None, :]).abs().max()) <= tol, what
                for g, n in enumerate(lens):                                            # rows past a graph's length: bias * gate
                    if n < T:
                        assert torch.equal(got[g, n:], (m.bias.detach() * gs[g]).expand(T - n, F)), what + ": padding rows"
            else:
                assert bool(torch.isnan(out).all()), what + ": out = NULL was written"
            if with_pools:
                assert not bool(torch.isnan(pa[:B]).any()) and not bool(torch.isnan(pb[:B]).any()), what + ": NaN in a pool"
                assert bool(torch.isnan(pa[B]).all()) and bool(torch.isnan(pb[B]).all()), what + ": wrote past B pool rows"
                assert float((pa[:B].double().cpu() - (y * ga.double().cpu()[:, None, :]).max(1).values).abs().max()) <= tol, what
                assert float((pb[:B].double().cpu() - (y * gb.double().cpu()[:, None, :]).max(1).values).abs().max()) <= tol, what
            else:
                assert bool(torch.isnan(pa).all()) and bool(torch.isnan(pb).all()), what + ": a NULL pool was written"


def test_refusals_launch_nothing(pkg, dev):
    from ed_gated_gcn_amd import _capi
    lib = pkg.load_library()
    p, st = _capi.ptr, _capi.stream_of(dev)
    EINVAL, EUNSUPPORTED = 1, 3
    B, T, K, F = 2, 64, 64, 64
    adj = torch.rand(B, T, T, device=dev)
    csr = pkg.BatchedCSR.from_dense(adj)
    ops = torch.full((lib.ggcn_graph_operands_weighted_wide_bytes(B, T),), 0xFF, dtype=torch.uint8, device=dev)
    before = ops.clone()
    a = (p(csr.rowptr), p(csr.colidx), p(csr.vals))
    assert lib.ggcn_graph_operands_weighted_wide(*a, B, 32, p(ops), None, st) == EUNSUPPORTED
    assert b"ggcn_graph_operands_weighted" in lib.ggcn_last_error()
    assert lib.ggcn_graph_operands_weighted_wide(*a, B, 129, p(ops), None, st) == EUNSUPPORTED
    assert lib.ggcn_graph_operands_weighted_wide(None, a[1], a[2], B, T, p(ops), None, st) == EINVAL
    assert lib.ggcn_graph_operands_weighted_wide(a[0], None, a[2], B, T, p(ops), None, st) == EINVAL
    assert lib.ggcn_graph_operands_weighted_wide(*a, B, T, None, None, st) == EINVAL
    x = torch.randn(B * T, K, device=dev)
    m = _layer(pkg, dev, torch.randn(K, F), torch.zeros(F), "f16mx8")
    with torch.cuda.device(dev):
        pack = m._packed_weight(lib, st, precision="f16mx8")
    out = torch.full((B * T, F), NAN, device=dev)

    def layer(T=T, ldx=K, ldo=F, pack=pack, ops=ops, prec=_capi.PREC["f16mx8"]):
        return lib.ggcn_layer_fused_weighted_wide(p(x), ldx, p(pack), p(ops), None, B, T, K, F, None, None, None, p(out), ldo, None, None, prec, st)
    assert layer(T=32) == EUNSUPPORTED and layer(T=129) == EUNSUPPORTED and layer(prec=_capi.PREC["fp32"]) == EUNSUPPORTED
    assert layer(ldx=K - 1) == EINVAL and layer(ldo=F - 1) == EINVAL and layer(ops=None) == EINVAL and layer(pack=None) == EINVAL
    assert layer(pack=pack[4:]) == EINVAL
    torch.cuda.synchronize()
    assert torch.equal(ops, before) and bool(torch.isnan(out).all())


# ================================================================ 4. a non-finite operand
def test_non_finite_operand_keeps_two_launches(pkg, dev, monkeypatch):
    from ed_gated_gcn_amd import _capi, synth
    lib = pkg.load_library()
    B, T, H = 3, 70, 64
    rng = np.random.default_rng(4)
    adj = _adjacency(B, T, "sparse", rng, np.array([T, 50, 40]))
    adj[1, 7, :] = 0.0
    adj[1, 7, 7], adj[1, 7, 40] = 2.0, -3.0                        # rowsum + 1 == 0 exactly
    ad = torch.from_numpy(adj).to(dev)
    csr = pkg.BatchedCSR.from_dense(ad)
    ops = torch.empty(lib.ggcn_graph_operands_weighted_wide_bytes(B, T), dtype=torch.uint8, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    _capi.check(lib.ggcn_graph_operands_weighted_wide(_capi.ptr(csr.rowptr), _capi.ptr(csr.colidx), _capi.ptr(csr.vals), B, T,
                                                      _capi.ptr(ops), _capi.ptr(flag), _capi.stream_of(dev)), "builder")
    assert int(flag.item()) & 1
    assert csr.graph_ops_weighted_wide() is None and csr.graph_ops_weighted_wide() is None
    x = torch.from_numpy(rng.standard_normal((B, T, H)).astype(np.float32)).to(dev)
    w, b = synth.layer_params(H, H, seed=8)
    on, parent = _layer(pkg, dev, w, b, "f16mx8"), _layer(pkg, dev, w, b, "f16mx8", weighted_max_t=32)
    assert not on.takes_weighted_path(x, csr)
    calls = count_calls(monkeypatch, COUNTED)
    with torch.no_grad():
        got = on.forward_gated(x, csr, want_pool_a=True)
        assert calls[WIDE] == 0 and calls[LINEAR] == 1 and calls[AGGREGATE] == 1, calls
        ref = parent.forward_gated(x, pkg.BatchedCSR.from_dense(ad), want_pool_a=True)
    ok = torch.ones(B, T, dtype=torch.bool, device=dev)
    ok[1, 7] = False                                                 # (that row is inf / NaN on both paths, as in the reference)
    assert bool(torch.isfinite(got[0][ok]).all())
    for g, r in zip(got[:2], ref[:2]):                               # out and pool a, bit for bit (NaN where the parent has NaN)
        assert torch.equal(g.isnan(), r.isnan()) and torch.equal(g.nan_to_num(), r.nan_to_num())


# ================================================================ 5. under autograd
_REF = {}


def _reference(dev, T):
    """tests/test_gpu_adjacency_grad.py ``_reference`` on case_inputs(5, T, 256, 256, 7000 + T, graph="weighted"): inputs on the
    device, tie-masked upstream gradients, float64 gradients; once per T (both split precisions share TOL and the tie mask)."""
    if T not in _REF:
        c = {k: v.to(dev) for k, v in br.case_inputs(5, T, 256, 256, 7000 + T, graph="weighted").items()}
        ma, mb = br.layer_tie_masks(c["x"], c["adj"], c["w"], c["b"], c["ga"], c["gb"], br.tie_delta("f16mx8", 0.0))
        assert br.tie_delta("f16mx8", 0.0) == br.tie_delta("bf16x3", 0.0)
        share = br.masked_share(ma, mb)
        print("T=%d: %.2f %% of the pools masked" % (T, 100 * share))
        assert share <= br.MAX_MASKED
        r1, r2, r3 = c["r1"], c["r2"] * (~ma), c["r3"] * (~mb)
        ref = {k: c[k].double().requires_grad_() for k in ("x", "w", "b", "sg", "ga", "gb", "adj")}
        o64, a64, b64 = br.gated_layer_ref(ref["x"], ref["adj"], ref["w"], ref["b"], ref["sg"], ref["ga"], ref["gb"])
        ((o64 * r1).sum() + (a64 * r2).sum() + (b64 * r3).sum()).backward()
        _REF[T] = (c, (r1, r2, r3), {k: v.grad.clone() for k, v in ref.items()})
    return _REF[T]


@pytest.mark.parametrize("precision", ["f16mx8", "bf16x3"])
@pytest.mark.parametrize("T", [33, 65, 100, 128])
def test_under_autograd(pkg, dev, monkeypatch, T, precision):
    c, rs, ref = _reference(dev, T)
    m = _layer(pkg, dev, c["w"], c["b"], precision)
    leaves = {k: c[k].clone().requires_grad_() for k in ("x", "sg", "ga", "gb", "adj")}
    calls = count_calls(monkeypatch, COUNTED)
    out, pa, pb = m.forward_gated(leaves["x"], leaves["adj"], store_gate=leaves["sg"], pool_gate_a=leaves["ga"], pool_gate_b=leaves["gb"],
                                  want_pool_a=True, want_pool_b=True)
    assert calls[WIDE] == 1 and calls[LINEAR] == 0 and calls[AGGREGATE] == 0, calls
    ((out * rs[0]).sum() + (pa * rs[1]).sum() + (pb * rs[2]).sum()).backward()
    torch.cuda.synchronize()
    assert calls[WIDE] == 1 and calls["ggcn_adjacency_grad"] == 1 and calls["ggcn_aggregate_t"] == 1 and calls["ggcn_gate_pool_backward"] == 1, calls
    what = "T=%d %s" % (T, precision)
    got = {k: v.grad for k, v in leaves.items()}
    got["w"], got["b"] = m.weight.grad, m.bias.grad
    assert got["adj"].shape == c["adj"].shape and not bool(torch.isnan(got["adj"]).any())
    for k, label in (("adj", "d adj"), ("x", "dX"), ("w", "dW"), ("b", "db"), ("sg", "d store gate"), ("ga", "d gate a"), ("gb", "d gate b")):
        _close32(got[k], ref[k], what + " " + label, 2e-4)


# ================================================================ 6. the gated block
def test_gated_block_on_a_weighted_adjacency(pkg, dev, monkeypatch):
    from ed_gated_gcn_amd import synth
    B, T, H = 4, 100, 128
    rng = np.random.default_rng(61)
    lens = np.array([T, 34, 77, 99])
    adj = _adjacency(B, T, "sparse", rng, lens)
    x = rng.standard_normal((B, T, H)).astype(np.float32)
    g1 = torch.sigmoid(torch.from_numpy(rng.standard_normal((B, H)).astype(np.float32)))
    g2 = torch.sigmoid(torch.from_numpy(rng.standard_normal((B, H)).astype(np.float32)))
    w1, b1 = synth.layer_params(H, H, seed=1)
    w2, b2 = synth.layer_params(H, H, seed=2)
    t = torch.from_numpy
    ref = ref_dense.gated_block(t(x).double(), t(adj).double(), g1.double(), g2.double(), t(w1).double(), t(b1).double(), t(w2).double(),
                                t(b2).double(), dtype=torch.float64)
    for precision in ("f16mx8", "bf16x3"):
        l1, l2 = _layer(pkg, dev, w1, b1, precision), _layer(pkg, dev, w2, b2, precision)
        calls = count_calls(monkeypatch, COUNTED)
        with torch.no_grad():
            r = pkg.gated_gcn_block(t(x).to(dev), t(adj).to(dev), g1.to(dev), g2.to(dev), l1, l2)
        torch.cuda.synchronize()
        assert calls[WIDE] == 2 and calls[LINEAR] == 0 and calls[AGGREGATE] == 0, calls
        for k in ("x1", "y1", "x", "out"):
            gate = TOL[precision] * max(1.0, float(ref[k].abs().max()))
            err = float((r[k].double().cpu() - ref[k]).abs().max())
            print("block %s %s: max|diff| %.3g (gate %.3g)" % (precision, k, err, gate))
            assert err == err and err <= gate, (precision, k, err, gate)
        assert abs(float(r["xy"]) - float(ref["xy"])) <= 1e-4 * abs(float(ref["xy"]))
        monkeypatch.undo()
