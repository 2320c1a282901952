"""The one-launch backward for real-valued adjacencies of 33..128 nodes (``ggcn_graph_operands_weighted_wide_t`` +
``ggcn_gate_pool_backward_weighted_wide``; opt-in ``GraphConvolution.weighted_wide_backward``; no form under gate dropout).  Run
with ``-m gpu -s`` on an MI355X to see the figures.  Cases, inputs, the numpy statements and the elementwise bounds are
``tests/weighted_wide_backward_ref.py``'s (``tests/test_weighted_wide_backward_cpu.py`` holds a numpy emulation of the kernel's
arithmetic to the same bounds on the same cases).

1. The builder against the numpy statement of the operand, bit for bit, in a buffer of 0xFF whose bytes behind the operand stay
   untouched; graphs from ``from_dense`` and from ``from_arrays``; a NaN and an inf entry raise the flag, the cached method answers
   None and the layer keeps the two passes; the operand is built once per adjacency tensor.
2. The kernel through the C ABI against the float64 statement (``oracle/gates.py``) within the derived bounds: dH
   (7 n_s + 8) u sum_t |A[t,s]| |inv_t| absdY[t,f], d_sg / d_bsum (T + 4) u sum |terms|, d_ga / d_gb / dY 4 u |ref|, u = 2^-23, and
   dH / dY within 2e-6 max|ref|.  Outputs lie in NaN between NaN guard bands, pad columns and guards are checked untouched, every
   call is made twice and compared bit for bit, dH is bit-identical with and without the dY store.  Measured: worst element at
   0.130 (dH), 0.125 (dY), 0.024 (d_sg), 0.021 (d_bsum), 0.273 (d_ga), 0.275 (d_gb) of its bound; dH at most 0.177 and dY 0.025 of
   the 2e-6 gate.
3. ``forward_gated`` under autograd with the option on against ``oracle/backward_ref.py`` (float64 autograd, near-tie pools
   masked, at most 3 %), float32 and bfloat16 features, ``adj`` as data and as ``requires_grad``: the gates of
   tests/test_gpu_weighted_backward.py (2e-4 max|ref|; bf16: ``gates.gate_dx`` / ``gates.gate``) and a call counter.
4. Where the option steps aside, with the same counter and gates; under gate dropout against the float64 reference with the keep
   factors replayed from ``ggcn_dropout_mask``, at 5e-4.
5. ``gated_gcn_block`` under autograd on a weighted graph of 40 nodes: both layers take the new entry on ONE cached operand.
6. One training step of ``GatedGCNEventDetector`` on a weighted batch of 40 words, option on against off.
"""
import types

import numpy as np
import pytest
import torch

import weighted_wide_backward_ref as ww
from oracle import backward_ref as br
from oracle import gates
from oracle.gpu_support import ace_batch, count_calls, dev, drop_mask, make_layer, pkg  # noqa: F401

pytestmark = pytest.mark.gpu

NAN = float("nan")
BUILD, KERNEL = "ggcn_graph_operands_weighted_wide_t", "ggcn_gate_pool_backward_weighted_wide"
(WIDE, WEIGHTED, MMA, AGG, GPB, GPB_DROP, AGG_T, TRANSPOSE, ADJ_GRAD) = (
    "ggcn_gate_pool_backward_wide", "ggcn_gate_pool_backward_weighted", "ggcn_gate_pool_backward_mma", "ggcn_gate_pool_backward_agg",
    "ggcn_gate_pool_backward", "ggcn_gate_pool_backward_drop", "ggcn_aggregate_t", "ggcn_csr_transpose", "ggcn_adjacency_grad")
COUNTED = (BUILD, KERNEL, WIDE, WEIGHTED, "ggcn_graph_operands_weighted_t", "ggcn_rowmask_transpose_wide", MMA, AGG, GPB, GPB_DROP, AGG_T,
           TRANSPOSE, ADJ_GRAD)
GUARD = 64


# ================================================================ 1. the builder
def _build_into_poison(pkg, dev, csr, Bn, T):
    from ed_gated_gcn_amd import _capi
    lib = pkg.load_library()
    nbytes = lib.ggcn_graph_operands_weighted_wide_t_bytes(Bn, T)
    assert nbytes == ww.operand_bytes(Bn, T)
    buf = gates.poisoned(nbytes + 4096, dev)
    assert buf.data_ptr() % 16 == 0 and buf.numel() >= nbytes + 4096
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    _capi.check(lib.ggcn_graph_operands_weighted_wide_t(_capi.ptr(csr.rowptr), _capi.ptr(csr.colidx), _capi.ptr(csr.vals), Bn, T,
                                                        _capi.ptr(buf), _capi.ptr(flag), _capi.stream_of(dev)), BUILD)
    got = buf.cpu().numpy()
    assert (got[nbytes:] == 0xFF).all(), "bytes behind the operand were written"
    return got[:nbytes], int(flag.item())


@pytest.mark.parametrize("T", ww.BUILDER_T)
def test_builder_is_the_numpy_statement(pkg, dev, monkeypatch, T):
    W = (T + 31) // 32
    for graph in ww.BUILDER_GRAPHS:
        adj = ww.adjacency(T, graph, 400 + T)
        want = ww.operand_buffer_np(adj.numpy())
        csr = pkg.BatchedCSR.from_dense(adj.to(dev), binary=False)
        got, flag = _build_into_poison(pkg, dev, csr, ww.B, T)
        assert flag == 0, graph
        blocks = W * W * ww.BLOCK_BYTES
        for b in range(ww.B):
            assert np.array_equal(got[b * blocks:(b + 1) * blocks], want[b * blocks:(b + 1) * blocks]), "%s: the blocks of graph %d" % (graph, b)
        assert np.array_equal(got[ww.B * blocks:], want[ww.B * blocks:]), "%s: the summary words" % graph
    calls = count_calls(monkeypatch, (BUILD,))
    cached = csr.graph_ops_weighted_wide_t()
    assert cached is csr.graph_ops_weighted_wide_t() and calls[BUILD] == 1 and cached.data_ptr() % 16 == 0
    assert np.array_equal(cached.cpu().numpy(), want)


def test_builder_on_a_graph_from_arrays(pkg, dev):
    T = 65
    adj = ww.adjacency(T, "hub", 77).numpy()
    rows, cols = np.nonzero(adj.reshape(ww.B * T, T))
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=ww.B * T))]).astype(np.int32)
    colidx = (cols + (rows // T) * T).astype(np.int32)
    csr = pkg.BatchedCSR.from_arrays(rowptr, colidx, ww.B, T, dev, vals=adj.reshape(ww.B * T, T)[rows, cols])
    assert not csr.is_binary and csr._dense is None
    got, flag = _build_into_poison(pkg, dev, csr, ww.B, T)
    assert flag == 0 and np.array_equal(got, ww.operand_buffer_np(adj))
    assert np.array_equal(csr.graph_ops_weighted_wide_t().cpu().numpy(), got)


def test_the_cached_operand_exists_only_where_the_kernel_runs(pkg, dev):
    for T, expect in ((32, False), (33, True), (128, True), (129, False)):
        csr = pkg.BatchedCSR.from_dense(br.case_adjacency(2, T, 5, "weighted").to(dev), binary=False)
        assert (csr.graph_ops_weighted_wide_t() is not None) == expect, T


@pytest.mark.parametrize("bad", [NAN, float("inf"), -float("inf"), 3.0e38, -3.2e38], ids=["nan", "inf", "-inf", "3.0e38", "-3.2e38"])
def test_a_non_finite_entry_raises_the_flag_and_the_layer_keeps_the_two_passes(pkg, dev, monkeypatch, bad):
    """Not finite, or finite and not below 3.0e38 in magnitude (include/ggcn.h); 2.9e38 is an entry like any other."""
    c = {k: (v.to(dev) if v is not None else None) for k, v in ww.autograd_inputs("t65", False, False).items()}
    adj = c["adj"].clone()
    adj[1, 40, 3] = 2.9e38 if bad != bad or bad > 0 else -2.9e38
    _, flag = _build_into_poison(pkg, dev, pkg.BatchedCSR.from_dense(adj, binary=False), adj.shape[0], adj.shape[1])
    assert flag == 0
    adj[1, 40, 3] = bad
    csr = pkg.BatchedCSR.from_dense(adj, binary=False)
    _, flag = _build_into_poison(pkg, dev, csr, adj.shape[0], adj.shape[1])
    assert flag & 1
    calls = count_calls(monkeypatch, COUNTED)
    assert csr.graph_ops_weighted_wide_t() is None and csr.graph_ops_weighted_wide_t() is None and calls[BUILD] == 1      # cached: one read-back
    m = _layer(pkg, dev, c["w"], c["b"], True)
    x = c["x"].clone().requires_grad_()
    out, pa, pb = m.forward_gated(x, adj, store_gate=c["sg"], pool_gate_a=c["ga"], pool_gate_b=c["gb"], want_pool_a=True, want_pool_b=True)
    (out.sum() + pa.sum() + pb.sum()).backward()
    torch.cuda.synchronize()
    assert calls[KERNEL] == 0 and calls[GPB] == 1 and calls[AGG_T] == 1 and calls[BUILD] == 2, {k: v for k, v in calls.items() if v}


# ================================================================ 2. the kernel through the C ABI
def _kernel_case(pkg, dev, T, F, graph="sparse", variant="full"):
    """One case of weighted_wide_backward_ref.KERNEL_CASES at ld = F and F + 12; returns the worst error / bound per output."""
    from ed_gated_gcn_amd import _capi
    lib = pkg.load_library()
    p, st = _capi.ptr, _capi.stream_of(dev)
    c = {k: (None if v is None else v.to(dev)) for k, v in ww.kernel_inputs(T, F, graph, variant).items()}
    Bn = ww.B
    csr = pkg.BatchedCSR.from_dense(c["adj"], binary=False)
    ops, inv = csr.graph_ops_weighted_wide_t(), csr.inv_denominators()
    assert ops is not None and ops.data_ptr() % 16 == 0
    # the library's 1 / (rowsum + 1): float32 sums in CSR order, at most T u sum|a| from the exact rowsum
    slack = T * ww.U * (c["adj"].double().abs().sum(2) + 1.0) * c["inv"].double().abs()
    assert bool(((inv.view(Bn, T).double() - c["inv"].double()).abs() <= (slack + 2 * ww.U) * c["inv"].double().abs()).all())
    c["inv"] = inv.view(Bn, T)      # the operand the kernel reads is the reference's and the bounds'
    ref = ww.statement(c)
    bound = ww.bounds(c, ref)
    what0 = "%dx%dx%d %s %s" % (Bn, T, F, graph, variant)
    worst = {}
    used = {"d_sg": c["sg"] is not None, "d_ga": c["d_pa"] is not None, "d_gb": c["d_pb"] is not None, "d_bsum": True}
    out2, dout2 = c["out"].reshape(Bn * T, F), (None if c["d_out"] is None else c["d_out"].reshape(Bn * T, F))
    for pad in (0, 12):
        ld = F + pad
        what = "%s ld=F+%d" % (what0, pad)
        ob, db = gates.hostile(out2, pad), (None if dout2 is None else gates.hostile(dout2, pad))
        runs = []
        for want_dy in (True, True, False):
            whole, o = {}, {}
            whole["dH"], o["dH"] = gates.poisoned_rows(dev, Bn * T, ld, GUARD)
            whole["dY"], o["dY"] = gates.poisoned_rows(dev, Bn * T, ld, GUARD)
            for k in used:
                whole[k], o[k] = gates.poisoned_rows(dev, Bn, F, GUARD)
            _capi.check(getattr(lib, KERNEL)(
                p(ob), ld, p(c["sg"]), p(c["ga"]), p(c["gb"]), p(db), ld, p(c["d_pa"]), p(c["d_pb"]), p(ops), p(inv), Bn, T, F, p(o["dH"]), ld,
                p(o["dY"]) if want_dy else None, ld if want_dy else 0,
                *(p(o[k]) if used[k] else None for k in ("d_sg", "d_ga", "d_gb", "d_bsum")), st), KERNEL)
            runs.append((whole, o))
        torch.cuda.synchronize()
        (whole, a), (whole2, _), (whole3, a3) = runs
        same = lambda x, y: torch.equal(torch.nan_to_num(x, nan=-7.0), torch.nan_to_num(y, nan=-7.0))     # noqa: E731
        for k in whole:
            assert same(whole[k], whole2[k]), "%s: two runs differ in %s" % (what, k)
            n = a[k].numel()
            assert bool(torch.isnan(whole[k][:GUARD]).all()) and bool(torch.isnan(whole[k][GUARD + n:]).all()), "%s: %s: a guard band was written" % (what, k)
            if k != "dY":
                assert same(whole[k], whole3[k]), "%s: %s differs without the dY store" % (what, k)
        assert bool(torch.isnan(whole3["dY"]).all()), "%s: dY written without being asked for" % what
        assert bool(torch.isnan(a["dH"][:, F:]).all()) and bool(torch.isnan(a["dY"][:, F:]).all()), "%s: pad columns were written" % what
        got = {"dH": a["dH"][:, :F].reshape(Bn, T, F), "dY": a["dY"][:, :F].reshape(Bn, T, F)}
        for k, on in used.items():
            if on:
                got[k] = a[k]
            else:
                assert bool(torch.isnan(a[k]).all()), "%s: %s written without being asked for" % (what, k)
        for k, g in got.items():
            assert not bool(torch.isnan(g).any()), "%s: NaN in %s" % (what, k)
            err = (g.double() - ref[k]).abs()
            ratio = float((err / (bound[k] + 1e-300)).max()) if bool((bound[k] > 0).any()) else 0.0
            worst[k] = max(worst.get(k, 0.0), ratio)
            top = float(ref[k].abs().max())
            if k in ("dH", "dY"):
                worst[k + " gate"] = max(worst.get(k + " gate", 0.0), float(err.max()) / (ww.GATE * top + 1e-300))
            print("  %s: %s worst %.3f of its bound, max|err| %.3g of max|ref|" % (what, k, ratio, float(err.max()) / (top + 1e-300)))
            bad = err > bound[k]
            assert not bool(bad.any()), "%s: %s: %d elements outside the bound, worst %.3g of it (max|err| %.3g, max|ref| %.3g)" % (
                what, k, int(bad.sum()), ratio, float(err.max()), top)
            if k in ("dH", "dY"):
                assert float(err.max()) <= ww.GATE * top, "%s: %s max|diff| %.3g > %.3g" % (what, k, float(err.max()), ww.GATE * top)
    print("%s: worst |diff| / bound %s" % (what0, {k: "%.3f" % v for k, v in worst.items()}))
    return worst


@pytest.mark.parametrize("F", ww.KERNEL_F)
@pytest.mark.parametrize("T", ww.KERNEL_T)
def test_kernel_vs_float64(pkg, dev, T, F):
    assert (T, F, "sparse", "full") in ww.KERNEL_CASES
    _kernel_case(pkg, dev, T, F)


@pytest.mark.parametrize("graph", ww.GRAPHS)
@pytest.mark.parametrize("T", ww.GRAPH_T)
def test_kernel_graphs_and_variants(pkg, dev, T, graph):
    for variant in ww.VARIANTS:
        if (graph, variant) != ("sparse", "full"):      # (that one is in the sweep above)
            assert (T, ww.GRAPH_F, graph, variant) in ww.KERNEL_CASES
            _kernel_case(pkg, dev, T, ww.GRAPH_F, graph, variant)


def test_more_graphs_than_compute_units(pkg, dev):
    """600 graphs of 33 nodes (more workgroups than CUs x 2): every graph of the batch is the same one, and so are its dH and dY."""
    from ed_gated_gcn_amd import _capi
    lib = pkg.load_library()
    p, st = _capi.ptr, _capi.stream_of(dev)
    Bn, T, F = 600, 33, 4
    assert Bn > 2 * torch.cuda.get_device_properties(dev).multi_processor_count
    c = {k: v.to(dev) for k, v in ww.kernel_inputs(T, F).items()}
    r = {k: v[:1].expand(Bn, *v.shape[1:]).contiguous() for k, v in c.items()}      # (held until the launch has run)
    csr = pkg.BatchedCSR.from_dense(r["adj"], binary=False)
    dh, dy = torch.full((Bn * T, F), NAN, device=dev), torch.full((Bn * T, F), NAN, device=dev)
    _capi.check(getattr(lib, KERNEL)(p(r["out"]), F, p(r["sg"]), p(r["ga"]), p(r["gb"]), p(r["d_out"]), F,
                                     p(r["d_pa"]), p(r["d_pb"]), p(csr.graph_ops_weighted_wide_t()), p(csr.inv_denominators()),
                                     Bn, T, F, p(dh), F, p(dy), F, None, None, None, None, st), KERNEL)
    torch.cuda.synchronize()
    for t in (dh.view(Bn, T, F), dy.view(Bn, T, F)):
        assert not bool(torch.isnan(t).any()) and bool((t == t[:1]).all())
    one = {k: v[:1] for k, v in c.items()}
    one["inv"] = csr.inv_denominators().view(Bn, T)[:1]
    ref = ww.statement(one)
    assert bool(((dh.view(Bn, T, F)[:1].double() - ref["dH"]).abs() <= ww.bounds(one, ref)["dH"]).all())


# ================================================================ 3. under autograd
def _layer(pkg, dev, w, b, option, precision="f16mx8", fused_max_t=256, **more):
    return make_layer(pkg, dev, w, b, expect_defaults={"weighted_wide_backward": False}, precision=precision,
                      weighted_wide_backward=option, fused_max_t=fused_max_t, **more)


_REF = {}      # case -> the float64 reference, computed once and left unchanged


DROPOUT = (0.25, 2 ** 40 + 99, (0, 1, 2))      # (p, seed, the streams of the three gates; stream 0: that gate is not dropped)


def _reference(dev, key, make, bf16, precision="f16mx8", pkg=None):
    """Inputs on the device, tie-masked upstream gradients and the float64 gradients (adj among them).  ``pkg`` given: under
    the gate dropout of ``DROPOUT``, with the keep factors replayed from ``ggcn_dropout_mask`` in the tie masks and the reference."""
    key = (key, bf16, pkg is not None)
    if key in _REF:
        return _REF[key]
    c = {k: (v.to(dev) if v is not None else None) for k, v in make(bf16).items()}
    keep, p = None, 0.0
    if pkg is not None:
        p, seed, streams = DROPOUT
        Bn, T, F = c["x"].shape[0], c["x"].shape[1], c["w"].shape[1]
        keep = tuple(None if s == 0 else drop_mask(pkg, dev, Bn * T, F, p, seed, s).view(Bn, T, F).double() for s in streams)
    ma, mb = br.layer_tie_masks(c["x"], c["adj"], c["w"], c["b"], c["ga"], c["gb"], br.tie_delta(precision, p), keep=keep)
    share = br.masked_share(ma, mb)
    print("%s%s: %.2f %% of the pools masked" % (key[0], " bf16" if bf16 else "", 100 * share))
    assert share <= br.MAX_MASKED
    rs = (c["r1"], c["r2"] * (~ma), c["r3"] * (~mb))
    ref = {k: c[k].double().requires_grad_() for k in ("x", "w", "b", "sg", "ga", "gb", "adj")}
    o64, a64, b64 = br.gated_layer_ref(ref["x"], ref["adj"], ref["w"], ref["b"], ref["sg"], ref["ga"], ref["gb"], keep=keep)
    ((o64 * rs[0]).sum() + (a64 * rs[1]).sum() + (b64 * rs[2]).sum()).backward()
    _REF[key] = (c, rs, {k: v.grad.clone() for k, v in ref.items()})
    return _REF[key]


def _offset_leaf(t):
    """(leaf buffer, contiguous view of it at storage offset 1 holding t): a [B,F] operand that is only 4-byte aligned."""
    buf = torch.cat([torch.full((1,), NAN, device=t.device), t.reshape(-1)]).requires_grad_()
    view = buf[1:].view(t.shape)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return buf, view


def _run(pkg, dev, c, rs, option, adj_grad=False, offset_gate=False, dropout=None, **more):
    """forward_gated + backward of the backward tests' loss; returns (gradients, adj.grad, the layer's BatchedCSR)."""
    from ed_gated_gcn_amd import csr as csr_mod
    m = _layer(pkg, dev, c["w"], c["b"], option, **more)
    leaves = {k: c[k].clone().requires_grad_() for k in ("x", "sg", "ga", "gb")}
    use = dict(leaves)
    if offset_gate:
        leaves["sg"], use["sg"] = _offset_leaf(c["sg"])
    adj = c["adj"].clone().requires_grad_(adj_grad)
    out, pa, pb = m.forward_gated(use["x"], adj, store_gate=use["sg"], pool_gate_a=use["ga"], pool_gate_b=use["gb"],
                                  want_pool_a=True, want_pool_b=True, dropout=dropout)
    ((out * rs[0]).sum() + (pa * rs[1]).sum() + (pb * rs[2]).sum()).backward()
    torch.cuda.synchronize()
    g = {k: v.grad for k, v in leaves.items()}
    if offset_gate:
        g["sg"] = g["sg"][1:].view(c["sg"].shape)
    g["w"], g["b"] = m.weight.grad, m.bias.grad
    return g, adj.grad, csr_mod.cached_from_dense(adj, binary=m.binary_adj)


def _check_grads(got, d_adj, ref, bf16, what, rel=2e-4):
    for k, label in (("x", "dX"), ("w", "dW"), ("b", "db"), ("sg", "d store gate"), ("ga", "d gate a"), ("gb", "d gate b")):
        assert got[k] is not None, "%s: %s is missing" % (what, label)
        if k == "x" and bf16:
            gates.gate_dx(got[k], ref[k])
        elif bf16:
            gates.gate(got[k], ref[k], label)
        else:
            gates.close32(got[k], ref[k], label, rel)
    if d_adj is not None:
        assert d_adj.shape == ref["adj"].shape and not bool(torch.isnan(d_adj).any())
        gates.close32(d_adj, ref["adj"], what + " d adj", rel)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("dense", [False, True], ids=["sparse", "softmax"])
@pytest.mark.parametrize("name", sorted(ww.AUTOGRAD))
def test_under_autograd_the_new_entry_replaces_the_two_calls(pkg, dev, monkeypatch, name, dense, bf16):
    what = "%s %s%s" % (name, "softmax" if dense else "sparse", " bf16" if bf16 else "")
    c, rs, ref = _reference(dev, (name, dense), lambda b: ww.autograd_inputs(name, b, dense), bf16)
    calls = count_calls(monkeypatch, COUNTED)
    for adj_grad in (False, True):
        before = dict(calls)
        got, d_adj, csr = _run(pkg, dev, c, rs, True, adj_grad=adj_grad)
        made = {k: calls[k] - before[k] for k in calls}
        want = {k: 0 for k in COUNTED}
        want.update({BUILD: 1, KERNEL: 1, ADJ_GRAD: 1 if adj_grad else 0})
        assert made == want, "%s adj.requires_grad=%s: the backward made %s" % (what, adj_grad, {k: v for k, v in made.items() if v})
        assert not csr.is_binary and csr._t is None, "%s: a transposed CSR was built" % what
        assert (d_adj is not None) == adj_grad
        _check_grads(got, d_adj, ref, bf16, what)


@pytest.mark.parametrize("adj_grad", [False, True], ids=["data", "requires_grad"])
def test_option_off_is_the_default_path(pkg, dev, monkeypatch, adj_grad):
    c, rs, ref = _reference(dev, ("t100", False), lambda b: ww.autograd_inputs("t100", b, False), False)
    calls = count_calls(monkeypatch, COUNTED)
    got, d_adj, csr = _run(pkg, dev, c, rs, False, adj_grad=adj_grad)
    want = {k: 0 for k in COUNTED}
    want.update({GPB: 1, AGG_T: 1, ADJ_GRAD: 1 if adj_grad else 0})
    assert calls == want, {k: v for k, v in calls.items() if v}
    assert csr._t is not None and csr._graph_ops_wwt is None
    _check_grads(got, d_adj, ref, False, "t100 off")


# ================================================================ 4. where it steps aside
def _steps_aside(pkg, dev, monkeypatch, key, make, expect, offset_gate=False, **more):
    c, rs, ref = _reference(dev, key, make, False)
    calls = count_calls(monkeypatch, COUNTED)
    got, d_adj, csr = _run(pkg, dev, c, rs, True, offset_gate=offset_gate, **more)
    want = {k: 0 for k in COUNTED}
    want.update(expect)
    assert calls == want, "%s: the backward made %s, not %s" % (key, {k: v for k, v in calls.items() if v}, expect)
    _check_grads(got, d_adj, ref, False, str(key))
    assert csr._graph_ops_wwt is None
    return csr


TWO = {GPB: 1, AGG_T: 1}
_T100 = ("t100", False), (lambda b: ww.autograd_inputs("t100", b, False))


def test_f30(pkg, dev, monkeypatch):
    _steps_aside(pkg, dev, monkeypatch, "F30", lambda b: br.case_inputs(3, 40, 64, 30, 9630, graph="weighted"), TWO)


def test_operand_at_an_odd_storage_offset(pkg, dev, monkeypatch):
    _steps_aside(pkg, dev, monkeypatch, *_T100, TWO, offset_gate=True)


def test_two_pass_switch(pkg, dev, monkeypatch):
    monkeypatch.setenv("GGCN_BACKWARD_TWO_PASS", "1")
    _steps_aside(pkg, dev, monkeypatch, *_T100, TWO)


def test_32_nodes(pkg, dev, monkeypatch):
    make = lambda b: br.case_inputs(3, 32, 64, 64, 9632, graph="weighted")     # noqa: E731
    _steps_aside(pkg, dev, monkeypatch, "T32", make, TWO)
    _steps_aside(pkg, dev, monkeypatch, "T32", make, {"ggcn_graph_operands_weighted_t": 1, WEIGHTED: 1}, weighted_backward=True)


def test_129_nodes(pkg, dev, monkeypatch):
    _steps_aside(pkg, dev, monkeypatch, "T129", lambda b: br.case_inputs(3, 129, 64, 64, 9729, graph="weighted"), TWO)


def test_binary_adjacency(pkg, dev, monkeypatch):
    csr = _steps_aside(pkg, dev, monkeypatch, "T100b", lambda b: br.case_inputs(3, 100, 64, 64, 9700), TWO)
    assert csr.is_binary


def test_gate_dropout(pkg, dev, monkeypatch):
    """Under gate dropout the predicate is False and, with the option on, ggcn_gate_pool_backward_drop + ggcn_aggregate_t stay,
    by call counts and against the float64 reference with the keep factors replayed (5e-4, the dropout gate of
    tests/test_gpu_wide_backward.py and tests/test_gpu_weighted_dropout.py): a 0/1 graph of 100 nodes (recipe drop100), and a
    real-valued one of 100 nodes whose forward draws the keep factors inside the weighted launch (weighted_dropout,
    weighted_max_t = 128; the 3 x 100 x 128 x 256 case of tests/test_gpu_weighted_dropout.py), without and with an adjacency
    gradient.  Without weighted_dropout a real-valued adjacency under gate dropout is refused in the forward, as without the
    option."""
    assert br.RECIPE["drop100"][7] == DROPOUT[0]
    runs = (("drop100", lambda b: br.recipe_inputs("drop100", bf16=b, batch=3), {}, True),
            ("T100w-drop", lambda b: br.case_inputs(3, 100, 128, 256, 5000 + 13 * 3 + 7 * 100 + 256, bf16=b, graph="weighted"),
             dict(weighted_dropout=True, weighted_max_t=128), False))
    for key, make, more, binary in runs:
        c, rs, ref = _reference(dev, key, make, False, pkg=pkg)
        calls = count_calls(monkeypatch, COUNTED)
        for adj_grad in (False, True):
            before = dict(calls)
            got, d_adj, csr = _run(pkg, dev, c, rs, True, adj_grad=adj_grad, dropout=DROPOUT, **more)
            made = {k: calls[k] - before[k] for k in calls}
            want = {k: 0 for k in COUNTED}
            want.update({GPB_DROP: 1, AGG_T: 1, ADJ_GRAD: 1 if adj_grad else 0})
            assert made == want, "%s adj.requires_grad=%s: %s" % (key, adj_grad, {k: v for k, v in made.items() if v})
            assert csr.is_binary == binary and csr._graph_ops_wwt is None and (d_adj is not None) == adj_grad
            _check_grads(got, d_adj, ref, False, "%s adj.requires_grad=%s" % (key, adj_grad), rel=5e-4)
    c, rs, _ = _reference(dev, *_T100, False)
    for option in (False, True):
        m = _layer(pkg, dev, c["w"], c["b"], option)
        with pytest.raises(RuntimeError, match="dropout= needs the one-launch layer"):
            m.forward_gated(c["x"].clone().requires_grad_(), c["adj"], store_gate=c["sg"], dropout=(0.25, 7, (0, 1, 2)))


# ================================================================ 5. the block of two layers
def test_gated_block_on_a_weighted_graph_of_40_nodes(pkg, dev, monkeypatch):
    """4 x 40 x 128: both layers take the new entry, the operand is built once (the layers share one BatchedCSR)."""
    from ed_gated_gcn_amd import csr as csr_mod, synth
    Bn, T, Hd, precision = 4, 40, 128, "f16mx8"
    g = torch.Generator().manual_seed(7300)
    (w1, b1), (w2, b2) = synth.layer_params(Hd, Hd, seed=7301), synth.layer_params(Hd, Hd, seed=7302)
    t = torch.from_numpy
    c = {"x": torch.randn(Bn, T, Hd, generator=g), "adj": br.case_adjacency(Bn, T, 7303, "weighted"), "g1": torch.rand(Bn, Hd, generator=g),
         "g2": torch.rand(Bn, Hd, generator=g), "w1": t(w1), "b1": t(b1), "w2": t(w2), "b2": t(b2),
         "r1": torch.randn(Bn, Hd, generator=g), "r2": torch.randn(Bn, T, Hd, generator=g)}
    c = {k: v.to(dev) for k, v in c.items()}
    m1, my, mo = br.block_tie_masks(c["x"], c["adj"], c["g1"], c["g2"], c["w1"], c["b1"], c["w2"], c["b2"], br.tie_delta(precision))
    share = br.masked_share(m1, my, mo)
    print("block %dx%dx%d weighted: %.2f %% of the pools masked" % (Bn, T, Hd, 100 * share))
    assert share <= br.MAX_MASKED
    unmasked, r1, r2 = ~(m1 | my), c["r1"] * (~mo), c["r2"]

    def loss_of(r):
        return (r["out"] * r1).sum() + 0.1 * (r["x"] * r2).sum() + 0.01 * (r["x1"] * r["y1"] * unmasked).sum() / Bn

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
    want.update({BUILD: 1, KERNEL: 2})
    assert calls == want, {k: v for k, v in calls.items() if v}
    csr = csr_mod.cached_from_dense(c["adj"], binary=gc1.binary_adj)
    assert csr._graph_ops_wwt is not None and csr._t is None
    got = {"x": xg.grad, "g1": g1g.grad, "g2": g2g.grad, "w1": gc1.weight.grad, "b1": gc1.bias.grad, "w2": gc2.weight.grad,
           "b2": gc2.bias.grad}
    for k in names:
        gates.close32(got[k], ref[k].grad, "d " + k, 5e-4)


# ================================================================ 6. the classifier
class _Bert(torch.nn.Module):
    """The stand-in BERT of the classifier tests: twelve seeded [B,L,768] layers, a zero pooled output."""

    def forward(self, ids_, seg, output_all_encoded_layers=True):
        gen = torch.Generator(device=ids_.device).manual_seed(1)
        return ([torch.randn(ids_.shape[0], ids_.shape[1], 768, device=ids_.device, generator=gen) for _ in range(12)],
                torch.zeros(ids_.shape[0], 768, device=ids_.device))


def _training_step(pkg, dev, inputs, ncls, option):
    opt = types.SimpleNamespace(dropout=0.0, polarities_dim=ncls, device=dev, ggcn_weighted_wide_backward=option)
    m = pkg.GatedGCNEventDetector(_Bert(), opt)
    assert m.gc1.weighted_wide_backward is option and m.gc2.weighted_wide_backward is option
    gen = torch.Generator().manual_seed(0)
    for prm in m.parameters():
        if prm.dim() > 1:
            torch.nn.init.xavier_uniform_(prm, generator=gen)
        else:
            torch.nn.init.uniform_(prm, -0.05, 0.05, generator=gen)
    m = m.to(dev).train()
    torch.manual_seed(11)
    logits, xy, kl, scores = m(inputs)
    r = torch.randn(scores.shape, generator=torch.Generator().manual_seed(4)).to(dev)
    target = torch.arange(logits.shape[0], device=dev) % ncls
    loss = torch.nn.functional.cross_entropy(logits, target) + xy + kl + (scores * r).mean()
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: prm.grad for n, prm in m.named_parameters() if n.split(".")[0] in ("fc", "dense", "lstm", "gc1", "gc2", "gate1", "gate2")}
    return loss.detach(), grads


def test_classifier_training_step_with_the_option(pkg, dev, monkeypatch):
    monkeypatch.delenv("GGCN_WEIGHTED_WIDE_BACKWARD", raising=False)
    inputs = {k: v.to(dev) for k, v in ace_batch(np.random.default_rng(3), 8, 40, 65, vocab=30522, weights=(0.25, 2.0)).items()}
    ncls = 34
    assert int(inputs["sentence_length"].max()) == 40
    calls = count_calls(monkeypatch, COUNTED)
    loss_off, g_off = _training_step(pkg, dev, inputs, ncls, False)
    assert calls[KERNEL] == 0 and calls[GPB] == 2 and calls[AGG_T] == 2, calls
    before = dict(calls)
    loss_on, g_on = _training_step(pkg, dev, inputs, ncls, True)
    made = {k: calls[k] - before[k] for k in calls}
    want = {k: 0 for k in COUNTED}
    want.update({BUILD: 1, KERNEL: 2})
    assert made == want, {k: v for k, v in made.items() if v}
    gates.close32(loss_on.reshape(1), loss_off.reshape(1), "loss", 5e-4)
    assert sorted(g_on) == sorted(g_off) and len(g_on) >= 16
    for n in sorted(g_on):
        assert g_on[n] is not None and g_off[n] is not None, n
        gates.close32(g_on[n], g_off[n], "d " + n, 5e-4)
