"""The one-launch backward for a real-valued adjacency of graphs of <= 32 nodes (``ggcn_graph_operands_weighted_t`` +
``ggcn_gate_pool_backward_weighted``; opt-in ``GraphConvolution.weighted_backward``).  Run with ``-m gpu -s`` on an MI355X to see
the figures.

1. The builder: the blocks decoded on the host, p0 + p1 + p2 = A_w^T within 2^-24 |a| per entry, rows and columns >= T exactly 0.
2. The kernel through the C ABI against the float64 statement (oracle/gates.py) of the formulas in csrc/gate_pool_backward_mma.hip's header
   (dY, then dH = A_w^T . (inv . dY)); the pools' winners are taken from the float32 values the kernel itself compares (the first
   maximum in ascending row order), everything else is float64.  Outputs pre-filled with NaN, pad columns and the row after the
   last one checked untouched, each call made twice and compared bit for bit.  Gates: dH and dY 2e-6 * max|ref|; d_sg, d_ga,
   d_gb, d_bsum 2e-6 * max|ref| (the tolerances of test_gate_pool_backward_on_the_matrix_cores); dH against
   ggcn_gate_pool_backward + ggcn_aggregate_t 4e-6 * max|ref|.
3. ``forward_gated`` under autograd with the option on against ``oracle/backward_ref.py`` (float64 autograd, near-tie pools
   masked, at most 3 % of them), float32 and bfloat16 features, with and without ``adj.requires_grad``: gradients at the gates of
   tests/test_gpu_backward.py (2e-4 * max|ref|; bf16: its dX form), d_adj at tests/test_gpu_adjacency_grad.py's (2e-4 * max|ref|),
   and a call counter: the new entry once per layer backward, ggcn_gate_pool_backward / ggcn_aggregate_t / ggcn_csr_transpose
   never, no transposed CSR built.
4. Where the option steps aside, with the same counter and gates.
5. ``gated_gcn_block`` under autograd on a weighted graph: both layers take the new entry on ONE operand block (5e-4).
"""
import numpy as np
import pytest
import torch

from oracle import backward_ref as br
from oracle import gates
from oracle.gpu_support import count_calls, dev, drop_mask as _drop_mask, make_layer, pkg  # noqa: F401

pytestmark = pytest.mark.gpu

NAN = float("nan")
_hostile, _close32, _gate, _gate_dx = gates.hostile, gates.close32, gates.gate, gates.gate_dx
_statement64 = gates.gate_pool_backward_statement64      # keep=None: the kernel without dropout
BUILD, WEIGHTED, ADJ_GRAD, TRANSPOSE = ("ggcn_graph_operands_weighted_t", "ggcn_gate_pool_backward_weighted", "ggcn_adjacency_grad",
                                        "ggcn_csr_transpose")
MMA, AGG, GPB, GPB_DROP, AGG_T = ("ggcn_gate_pool_backward_mma", "ggcn_gate_pool_backward_agg", "ggcn_gate_pool_backward",
                                   "ggcn_gate_pool_backward_drop", "ggcn_aggregate_t")
COUNTED = (BUILD, WEIGHTED, ADJ_GRAD, TRANSPOSE, MMA, AGG, GPB, GPB_DROP, AGG_T)
BLOCK_BYTES = 6144


# ================================================================ 1. the builder
def decode(ops, B):
    """uint8 [B * 6144] -> float64 [B, 3 planes, 32, 32]: plane p, k-step s at (2 p + s) * 1024, lane l = row l & 31 with h = l >> 5,
    element j = column 16 s + 8 (j >> 2) + 4 h + (j & 3)."""
    raw = ops.cpu().numpy().reshape(B, 3, 2, 64, 8, 2).copy().view(np.uint16)[..., 0]      # [B, p, s, lane, j]
    val = (raw.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    n = np.full((B, 3, 32, 32), np.nan)
    for s in range(2):
        for lane in range(64):
            for j in range(8):
                n[:, :, lane & 31, 16 * s + 8 * (j >> 2) + 4 * (lane >> 5) + (j & 3)] = val[:, :, s, lane, j]
    assert not np.isnan(n).any()
    return n


def _build(pkg, dev, csr, vals=True):
    from ed_gated_gcn_amd import _capi
    lib = pkg.load_library()
    ops = torch.full((lib.ggcn_graph_operands_weighted_t_bytes(csr.B),), 0xFF, dtype=torch.uint8, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    _capi.check(lib.ggcn_graph_operands_weighted_t(_capi.ptr(csr.rowptr), _capi.ptr(csr.colidx), _capi.ptr(csr.vals) if vals else None,
                                                   csr.B, csr.T, _capi.ptr(ops), _capi.ptr(flag), _capi.stream_of(dev)), BUILD)
    return ops, int(flag.item())


def _signed_adjacency(B, T, seed):
    """case_adjacency "weighted" with half of the weights negated."""
    adj = br.case_adjacency(B, T, seed, "weighted")
    sign = torch.from_numpy(np.where(np.random.default_rng(seed + 1).random(tuple(adj.shape)) < 0.5, -1.0, 1.0).astype(np.float32))
    return adj * sign


@pytest.mark.parametrize("T", [1, 5, 31, 32])
def test_builder_planes(pkg, dev, T):
    B = 3
    adj = _signed_adjacency(B, T, 70 + T)
    assert bool((adj < 0).any()) or T == 1
    csr = pkg.BatchedCSR.from_dense(adj.to(dev), binary=False)
    assert lib_bytes(pkg, B) == B * BLOCK_BYTES
    ops, flag = _build(pkg, dev, csr)
    assert flag == 0
    n = decode(ops, B)
    want = np.zeros((B, 32, 32))
    want[:, :T, :T] = adj.double().numpy().transpose(0, 2, 1)        # N[s][t] = A_w[t][s]
    got = n.sum(1)
    err = np.abs(got - want)
    print("T=%d: max |p0+p1+p2 - a| / |a| = %.3g (gate %.3g)" % (T, float((err / np.maximum(np.abs(want), 1e-300)).max()), 2.0 ** -24))
    assert (err <= 2.0 ** -24 * np.abs(want)).all()
    assert (n[:, :, T:, :] == 0).all() and (n[:, :, :, T:] == 0).all()                 # rows and columns >= T: exactly zero
    assert (n[:, :, :T, :T][np.broadcast_to((want[:, :T, :T] == 0)[:, None], (B, 3, T, T))] == 0).all()
    # the leading plane is the bf16 rounding of the entry
    assert np.array_equal(n[:, 0], torch.from_numpy(want).float().to(torch.bfloat16).double().numpy())
    # vals == NULL: the 0/1 transpose
    ops1, flag1 = _build(pkg, dev, csr, vals=False)
    n1 = decode(ops1, B)
    assert flag1 == 0 and np.array_equal(n1[:, 0], (want != 0).astype(np.float64)) and (n1[:, 1:] == 0).all()
    # the cached form is the same block, built once
    cached = csr.graph_ops_weighted_t()
    assert cached is csr.graph_ops_weighted_t() and torch.equal(cached, ops)


def lib_bytes(pkg, B):
    return pkg.load_library().ggcn_graph_operands_weighted_t_bytes(B)


def test_builder_flags_an_entry_that_is_not_finite(pkg, dev):
    adj = br.case_adjacency(3, 17, 5, "weighted")
    adj[1, 4, 2] = float("inf")
    csr = pkg.BatchedCSR.from_dense(adj.to(dev), binary=False)
    _, flag = _build(pkg, dev, csr)
    assert flag & 1
    assert csr.graph_ops_weighted_t() is None and csr.graph_ops_weighted_t() is None
    assert pkg.BatchedCSR.from_dense(br.case_adjacency(3, 33, 5, "weighted").to(dev), binary=False).graph_ops_weighted_t() is None


# ================================================================ 2. the kernel through the C ABI
VARIANTS = ("full", "no-store-gate", "no-pool-a", "no-pool-b", "no-d_out", "no-dY")


def _kernel_case(pkg, dev, B, T, F):
    from ed_gated_gcn_amd import _capi
    lib = pkg.load_library()
    p, st = _capi.ptr, _capi.stream_of(dev)
    adj = br.case_adjacency(B, T, 300 + T + F, "weighted").to(dev)
    csr = pkg.BatchedCSR.from_dense(adj, binary=False)
    ops, inv = csr.graph_ops_weighted_t(), csr.inv_denominators()
    assert ops is not None and ops.data_ptr() % 16 == 0
    g = torch.Generator(device=dev).manual_seed(1000 * T + F + B)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)     # noqa: E731
    out, d_out = rn(B * T, F), rn(B * T, F)
    sg = torch.sigmoid(rn(B, F)) * torch.where(torch.rand(B, F, device=dev, generator=g) < 0.25, -1.0, 1.0)   # gates of negative sign
    ga = torch.rand(B, F, device=dev, generator=g) * 2.0 - 1.0
    gb = torch.sigmoid(rn(B, F))
    d_pa, d_pb = rn(B, F), rn(B, F)
    worst = {}
    for pad in (0, 4):
        ld = F + pad
        ob, db = _hostile(out, pad), _hostile(d_out, pad)
        for variant in VARIANTS if pad else ("full",):
            use = dict(sg=sg, ga=ga, gb=gb, d_out=d_out, d_pa=d_pa, d_pb=d_pb)
            if variant == "no-store-gate":
                use["sg"] = None
            if variant == "no-pool-a":
                use["ga"] = use["d_pa"] = None
            if variant == "no-pool-b":
                use["gb"] = use["d_pb"] = None
            if variant == "no-d_out":
                use["d_out"] = None
            want_dy = variant != "no-dY"
            what = "%dx%dx%d ld=F+%d %s" % (B, T, F, pad, variant)
            runs = []
            for _ in range(2):
                dh = torch.full((B * T + 1, ld), NAN, device=dev)
                dy = torch.full((B * T + 1, ld), NAN, device=dev) if want_dy else None
                o = {k: torch.full((B, F), NAN, device=dev) for k in ("d_sg", "d_ga", "d_gb", "d_bsum")}
                _capi.check(lib.ggcn_gate_pool_backward_weighted(
                    p(ob), ld, p(use["sg"]), p(use["ga"]), p(use["gb"]), p(db) if use["d_out"] is not None else None, ld, p(use["d_pa"]),
                    p(use["d_pb"]), p(ops), p(inv), B, T, F, p(dh), ld, p(dy), ld, p(o["d_sg"]) if use["sg"] is not None else None,
                    p(o["d_ga"]) if use["d_pa"] is not None else None, p(o["d_gb"]) if use["d_pb"] is not None else None, p(o["d_bsum"]), st),
                    WEIGHTED)
                o["dH"], o["dY"] = dh, dy
                runs.append(o)
            torch.cuda.synchronize()
            a, b2 = runs
            for k in a:
                if a[k] is not None:
                    assert torch.equal(torch.nan_to_num(a[k], nan=-7.0), torch.nan_to_num(b2[k], nan=-7.0)), "%s: two runs differ in %s" % (what, k)
            ref = _statement64(out.view(B, T, F), use["sg"], use["ga"], use["gb"], None if use["d_out"] is None else d_out.view(B, T, F),
                               use["d_pa"], use["d_pb"], adj, inv)
            for k in ("dH", "dY"):
                if a[k] is None:
                    continue
                assert bool(torch.isnan(a[k][B * T]).all()) and bool(torch.isnan(a[k][:, F:]).all()), "%s: %s written outside its rows" % (what, k)
                got = a[k][:B * T, :F].reshape(B, T, F).double()
                top = float(ref[k].abs().max())
                err = float((got - ref[k]).abs().max())
                assert err == err and err <= 2e-6 * top, "%s: %s max|diff| %.3g > %.3g" % (what, k, err, 2e-6 * top)
                worst[k] = max(worst.get(k, 0.0), err / (top + 1e-300))
            used = {"d_sg": use["sg"] is not None, "d_ga": use["d_pa"] is not None, "d_gb": use["d_pb"] is not None, "d_bsum": True}
            for k, on in used.items():
                if not on:
                    assert bool(torch.isnan(a[k]).all()), "%s: %s written without being asked for" % (what, k)
                    continue
                top = float(ref[k].abs().max()) + 1e-30
                err = float((a[k].double() - ref[k]).abs().max())
                assert err == err and err <= 2e-6 * top, "%s: %s max|diff| %.3g > %.3g" % (what, k, err, 2e-6 * top)
                worst[k] = max(worst.get(k, 0.0), err / top)
            if variant == "full" and pad == 0:      # the two calls it replaces, on the same inputs
                dy2, dh2 = torch.empty(B * T, F, device=dev), torch.empty(B * T, F, device=dev)
                csr_t = csr.transposed()
                _capi.check(lib.ggcn_gate_pool_backward(p(out), F, p(sg), p(ga), p(gb), p(d_out), F, p(d_pa), p(d_pb), B, T, F, p(dy2), F,
                                                        None, None, None, None, st), GPB)
                _capi.check(lib.ggcn_aggregate_t(p(dy2), F, p(csr_t.rowptr), p(csr_t.colidx), p(csr_t.vals), p(inv), B, T, F, p(dh2), F, st), AGG_T)
                top = float(ref["dH"].abs().max())
                err = float((a["dH"][:B * T, :F].double() - dh2.double()).abs().max())
                assert err <= 4e-6 * top, "%s: dH against the two calls: max|diff| %.3g > %.3g" % (what, err, 4e-6 * top)
                err = float((a["dY"][:B * T, :F].double() - dy2.double()).abs().max())
                assert err <= 4e-6 * float(ref["dY"].abs().max()), "%s: dY against ggcn_gate_pool_backward: max|diff| %.3g" % (what, err)
    print("%dx%dx%d: worst |diff| / max|ref| %s (gate 2e-6)" % (B, T, F, {k: "%.2g" % v for k, v in worst.items()}))


@pytest.mark.parametrize("F", [4, 64, 260])
@pytest.mark.parametrize("T", [1, 5, 31, 32])
def test_kernel_vs_float64(pkg, dev, T, F):
    _kernel_case(pkg, dev, 3, T, F)


def test_kernel_more_graphs_than_compute_units(pkg, dev):
    assert 300 > torch.cuda.get_device_properties(dev).multi_processor_count
    _kernel_case(pkg, dev, 300, 31, 64)


# ================================================================ 3. under autograd
def _layer(pkg, dev, w, b, option, precision="f16mx8", fused_max_t=None):
    return make_layer(pkg, dev, w, b, expect_defaults={"weighted_backward": False}, precision=precision, weighted_backward=option,
                      fused_max_t=fused_max_t)


STREAMS = (0, 1, 2)
_REF = {}      # case -> the float64 reference, computed once and left unchanged


def _reference(pkg, dev, key, make, bf16, p=0.0, precision="f16mx8"):
    """Inputs on the device, tie-masked upstream gradients, the dropout triple and the float64 gradients (adj among them)."""
    key = (key, bf16)
    if key in _REF:
        return _REF[key]
    c = {k: (v.to(dev) if v is not None else None) for k, v in make().items()}
    B, T, F = c["x"].shape[0], c["x"].shape[1], c["w"].shape[1]
    dropout = (p, 2 ** 40 + 99, STREAMS) if p else None
    keep = None
    if dropout is not None:
        keep = tuple(None if s == 0 else _drop_mask(pkg, dev, B * T, F, p, dropout[1], s).view(B, T, F).double() for s in STREAMS)
    ma, mb = br.layer_tie_masks(c["x"], c["adj"], c["w"], c["b"], c["ga"], c["gb"], br.tie_delta(precision, p), keep=keep)
    share = br.masked_share(ma, mb)
    print("%s%s: %.2f %% of the pools masked" % (key[0], " bf16" if bf16 else "", 100 * share))
    assert share <= br.MAX_MASKED
    rs = (c["r1"], c["r2"] * (~ma), c["r3"] * (~mb))
    ref = {k: c[k].double().requires_grad_() for k in ("x", "w", "b", "sg", "ga", "gb", "adj")}
    o64, a64, b64 = br.gated_layer_ref(ref["x"], ref["adj"], ref["w"], ref["b"], ref["sg"], ref["ga"], ref["gb"], keep=keep)
    ((o64 * rs[0]).sum() + (a64 * rs[1]).sum() + (b64 * rs[2]).sum()).backward()
    _REF[key] = (c, rs, dropout, {k: v.grad.clone() for k, v in ref.items()})
    return _REF[key]


def _run(pkg, dev, c, rs, dropout, adj_grad, option, fused_max_t=None):
    """forward_gated + backward of the backward tests' loss; returns (gradients, adj.grad, the layer's BatchedCSR)."""
    from ed_gated_gcn_amd import csr as csr_mod
    m = _layer(pkg, dev, c["w"], c["b"], option, fused_max_t=fused_max_t)
    leaves = {k: c[k].clone().requires_grad_() for k in ("x", "sg", "ga", "gb")}
    adj = c["adj"].clone().requires_grad_(adj_grad)
    out, pa, pb = m.forward_gated(leaves["x"], adj, store_gate=leaves["sg"], pool_gate_a=leaves["ga"], pool_gate_b=leaves["gb"],
                                  want_pool_a=True, want_pool_b=True, dropout=dropout)
    ((out * rs[0]).sum() + (pa * rs[1]).sum() + (pb * rs[2]).sum()).backward()
    torch.cuda.synchronize()
    g = {k: v.grad for k, v in leaves.items()}
    g["w"], g["b"] = m.weight.grad, m.bias.grad
    return g, adj.grad, csr_mod.cached_from_dense(adj, binary=m.binary_adj)


def _check_grads(got, d_adj, ref, bf16, what, rel=2e-4):
    for k, label in (("x", "dX"), ("w", "dW"), ("b", "db"), ("sg", "d store gate"), ("ga", "d gate a"), ("gb", "d gate b")):
        assert got[k] is not None, "%s: %s is missing" % (what, label)
        if k == "x" and bf16:
            _gate_dx(got[k], ref[k])
        elif bf16:
            _gate(got[k], ref[k], label)
        else:
            _close32(got[k], ref[k], label, rel)
    if d_adj is not None:
        assert d_adj.shape == ref["adj"].shape and not bool(torch.isnan(d_adj).any())
        _close32(d_adj, ref["adj"], what + " d adj", rel)


def _weighted_inputs(B, T, K, F, gates, bf16):
    return lambda: br.case_inputs(B, T, K, F, 5000 + 13 * B + 7 * T + F, bf16=bf16, gates=gates, graph="weighted")


SHAPES = [(5, 17, 34, 20, "u01"), (7, 30, 300, 200, "u01"), (3, 1, 8, 8, "u01"), (16, 32, 128, 96, "sym"), (32, 24, 256, 256, "u01"),
          (6, 31, 64, 260, "sym"), (4, 5, 32, 4, "u01")]


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,T,K,F,gates", SHAPES)
def test_under_autograd_the_new_entry_replaces_the_two_calls(pkg, dev, monkeypatch, B, T, K, F, gates, bf16):
    what = "%dx%dx%dx%d%s" % (B, T, K, F, " bf16" if bf16 else "")
    c, rs, _, ref = _reference(pkg, dev, (B, T, K, F), _weighted_inputs(B, T, K, F, gates, bf16), bf16)
    calls = count_calls(monkeypatch, COUNTED)
    for adj_grad in (False, True):
        before = dict(calls)
        got, d_adj, csr = _run(pkg, dev, c, rs, None, adj_grad, option=True)
        made = {k: calls[k] - before[k] for k in calls}
        want = {k: 0 for k in COUNTED}
        want.update({BUILD: 1, WEIGHTED: 1, ADJ_GRAD: 1 if adj_grad else 0})
        assert made == want, "%s adj.requires_grad=%s: the backward made %s" % (what, adj_grad, {k: v for k, v in made.items() if v})
        assert not csr.is_binary and csr._t is None, "%s: a transposed CSR was built" % what
        assert (d_adj is not None) == adj_grad
        _check_grads(got, d_adj, ref, bf16, what)


# ================================================================ 4. where it steps aside
def _steps_aside(pkg, dev, monkeypatch, key, make, expect, option=True, p=0.0, adj_grad=False, bf16=False):
    c, rs, dropout, ref = _reference(pkg, dev, key, make, bf16, p=p)
    calls = count_calls(monkeypatch, COUNTED)
    got, d_adj, csr = _run(pkg, dev, c, rs, dropout, adj_grad, option, fused_max_t=256 if c["x"].shape[1] > 32 else None)
    want = {k: 0 for k in COUNTED}
    want.update(expect)
    assert calls == want, "%s: the backward made %s, not %s" % (key, {k: v for k, v in calls.items() if v}, expect)
    _check_grads(got, d_adj, ref, bf16, str(key), rel=5e-4 if p else 2e-4)
    return csr


def test_option_off_is_the_default_path(pkg, dev, monkeypatch):
    csr = _steps_aside(pkg, dev, monkeypatch, (5, 17, 34, 20), _weighted_inputs(5, 17, 34, 20, "u01", False), {GPB: 1, AGG_T: 1}, option=False)
    assert csr._t is not None and csr._graph_ops_wt is None


def test_33_nodes(pkg, dev, monkeypatch):
    _steps_aside(pkg, dev, monkeypatch, "T33", lambda: br.case_inputs(3, 33, 64, 64, 6001, graph="weighted"), {GPB: 1, AGG_T: 1})


def test_f30(pkg, dev, monkeypatch):
    _steps_aside(pkg, dev, monkeypatch, "F30", lambda: br.case_inputs(6, 20, 64, 30, 6002, graph="weighted"), {GPB: 1, AGG_T: 1})


def test_two_pass_switch(pkg, dev, monkeypatch):
    monkeypatch.setenv("GGCN_BACKWARD_TWO_PASS", "1")
    _steps_aside(pkg, dev, monkeypatch, (5, 17, 34, 20), _weighted_inputs(5, 17, 34, 20, "u01", False), {GPB: 1, AGG_T: 1})


def test_binary_adjacency_takes_the_0_1_kernel(pkg, dev, monkeypatch):
    _steps_aside(pkg, dev, monkeypatch, "ragged17", lambda: br.recipe_inputs("ragged17"), {MMA: 1})


def test_gate_dropout(pkg, dev, monkeypatch):
    """Gate dropout exists in the one-launch 0/1 layers only: with the option on, a 0/1 graph under gate dropout and an adjacency
    gradient keeps ggcn_gate_pool_backward_drop + ggcn_aggregate_t (recipe drop24, 5e-4 as in tests/test_gpu_adjacency_grad.py),
    and a real-valued adjacency with gate dropout is refused in the forward, as it is without the option."""
    _steps_aside(pkg, dev, monkeypatch, "drop24", lambda: br.recipe_inputs("drop24"), {GPB_DROP: 1, AGG_T: 1, ADJ_GRAD: 1}, p=0.25,
                 adj_grad=True)
    c, rs, _, _ = _reference(pkg, dev, (5, 17, 34, 20), _weighted_inputs(5, 17, 34, 20, "u01", False), False)
    for option in (False, True):
        m = _layer(pkg, dev, c["w"], c["b"], option)
        with pytest.raises(RuntimeError, match="dropout= needs the one-launch layer"):
            m.forward_gated(c["x"].clone().requires_grad_(), c["adj"], store_gate=c["sg"], dropout=(0.25, 7, STREAMS))


# ================================================================ 5. the block of two layers
def test_gated_block_on_a_weighted_graph(pkg, dev, monkeypatch):
    """16 x 24 x 128: both layers take the new entry, the operand block is built once (the layers share one BatchedCSR)."""
    from ed_gated_gcn_amd import synth
    B, T, H, precision = 16, 24, 128, "f16mx8"
    g = torch.Generator().manual_seed(7100)
    (w1, b1), (w2, b2) = synth.layer_params(H, H, seed=7101), synth.layer_params(H, H, seed=7102)
    t = torch.from_numpy
    c = {"x": torch.randn(B, T, H, generator=g), "adj": br.case_adjacency(B, T, 7103, "weighted"), "g1": torch.rand(B, H, generator=g),
         "g2": torch.rand(B, H, generator=g), "w1": t(w1), "b1": t(b1), "w2": t(w2), "b2": t(b2),
         "r1": torch.randn(B, H, generator=g), "r2": torch.randn(B, T, H, generator=g)}
    c = {k: v.to(dev) for k, v in c.items()}
    m1, my, mo = br.block_tie_masks(c["x"], c["adj"], c["g1"], c["g2"], c["w1"], c["b1"], c["w2"], c["b2"], br.tie_delta(precision))
    share = br.masked_share(m1, my, mo)
    print("block 16x24x128 weighted: %.2f %% of the pools masked" % (100 * share))
    assert share <= br.MAX_MASKED
    unmasked, r1, r2 = ~(m1 | my), c["r1"] * (~mo), c["r2"]

    def loss_of(r):
        return (r["out"] * r1).sum() + 0.1 * (r["x"] * r2).sum() + 0.01 * (r["x1"] * r["y1"] * unmasked).sum() / B

    names = ("x", "g1", "g2", "w1", "b1", "w2", "b2")
    ref = {k: c[k].double().requires_grad_() for k in names}
    loss_of(br.block_ref(ref["x"], c["adj"], *[ref[k] for k in names[1:]])).backward()

    gc1, gc2 = _layer(pkg, dev, c["w1"], c["b1"], True, precision), _layer(pkg, dev, c["w2"], c["b2"], True, precision)
    xg, g1g, g2g = (c[k].clone().requires_grad_() for k in ("x", "g1", "g2"))
    calls = count_calls(monkeypatch, COUNTED)
    r = pkg.gated_gcn_block(xg, c["adj"], g1g, g2g, gc1, gc2)
    loss_of(r).backward()
    torch.cuda.synchronize()
    want = {k: 0 for k in COUNTED}
    want.update({BUILD: 1, WEIGHTED: 2})
    assert calls == want, {k: v for k, v in calls.items() if v}
    got = {"x": xg.grad, "g1": g1g.grad, "g2": g2g.grad, "w1": gc1.weight.grad, "b1": gc1.bias.grad, "w2": gc2.weight.grad,
           "b2": gc2.bias.grad}
    for k in names:
        _close32(got[k], ref[k].grad, "d " + k, 5e-4)
