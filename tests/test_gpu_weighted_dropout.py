"""Gate dropout inside the launches on a real-valued adjacency (opt-in ``GraphConvolution.weighted_dropout``; with
``weighted_backward`` also the one-launch backward).  Run with ``-m gpu -s`` on an MI355X to see the figures.

Inputs: ``br.case_inputs(B, T, K, F, 5000 + 13 B + 7 T + F, gates=..., graph="weighted")``, p = 0.25, seed 2^40 + 99, keep masks
from ``ggcn_dropout_mask``, the float64 reference ``br.gated_layer_ref(..., keep=...)``.  Under autograd (4.) near-tie pools get a zero
upstream gradient: ``br.layer_tie_masks`` with ``br.tie_delta(precision, p)``, under ``br.MAX_MASKED``.  The forward cases (1.)
compare every pooled value, masked or not; they only assert that the share of near-tie pools stays under ``br.MAX_MASKED`` for
every stream triple, so that the shapes serve the gradient cases as well.

1. Forward against float64: both entries, both precisions, the stream triples (0,1,2), (2,2,0), (1,1,1); ``out`` and both pools
   within ``br.TOL[precision] / (1 - p) * max(1, max|ref|)`` (the forward gate under dropout of tests/test_gpu_backward.py);
   exactly one call of the new entry, none of ``ggcn_linear`` / ``ggcn_aggregate``; through the C ABI with ``ldo = F + 4`` and NaN
   padding.
2. p = 0 is bit-identical to the launch without dropout; the same seed twice is bit-identical; another seed differs.
3. ``ggcn_gate_pool_backward_weighted_drop`` through the C ABI against a float64 statement of its formulas
   (``gate_pool_backward_statement64`` of oracle/gates.py with keep factors): dH, dY, gate gradients and bias sums 2e-6 of their scale, dY = NULL
   writes nothing but dH, two runs bit-identical, 4e-6 against ``ggcn_gate_pool_backward_drop`` + ``ggcn_aggregate_t``.
4. ``forward_gated`` under autograd, float32: every gradient (and ``adj.grad``) within 5e-4 of its scale, with call counts, for
   ``adj.requires_grad`` off / on and ``weighted_backward`` off / on; two of the 33..128 shapes with the two-call backward.
5. Where it steps aside.
6. The classifier in train mode on a weighted graph.
"""
import numpy as np
import pytest
import torch

from oracle import backward_ref as br
from oracle import gates
from oracle.gpu_support import ace_batch, count_calls, dev, drop_mask, make_layer, pkg  # noqa: F401

pytestmark = pytest.mark.gpu

NAN = float("nan")
_gate, _close32, _hostile, _statement64 = gates.gate, gates.close32, gates.hostile, gates.gate_pool_backward_statement64
P_DROP, SEED = 0.25, 2 ** 40 + 99
TRIPLES = ((0, 1, 2), (2, 2, 0), (1, 1, 1))
FWD, WIDE, BWD = "ggcn_layer_fused_weighted_drop", "ggcn_layer_fused_weighted_wide_drop", "ggcn_gate_pool_backward_weighted_drop"
BUILD_T, GPB, GPB_DROP, AGG_T, ADJ_GRAD = ("ggcn_graph_operands_weighted_t", "ggcn_gate_pool_backward", "ggcn_gate_pool_backward_drop",
                                           "ggcn_aggregate_t", "ggcn_adjacency_grad")
COUNTED = (FWD, WIDE, BWD, BUILD_T, GPB, GPB_DROP, AGG_T, ADJ_GRAD, "ggcn_gate_pool_backward_weighted", "ggcn_layer_fused_weighted",
           "ggcn_layer_fused_weighted_wide", "ggcn_layer_fused_drop", "ggcn_layer_fused", "ggcn_linear", "ggcn_aggregate")

SHAPES32 = [(5, 17, 34, 20, "u01"), (7, 30, 300, 200, "u01"), (3, 1, 8, 8, "u01"), (16, 32, 128, 96, "sym"), (32, 24, 256, 256, "u01"),
            (6, 31, 64, 260, "sym"), (6, 16, 32, 4, "u01")]
SHAPES_WIDE = [(3, 33, 64, 64, "u01"), (4, 64, 96, 72, "sym"), (2, 65, 40, 36, "u01"), (3, 100, 128, 256, "u01"), (3, 97, 256, 128, "u01"),
               (2, 128, 64, 260, "sym")]


def _layer(pkg, dev, w, b, precision="f16mx8", dropout=True, backward=False, max_t=None):
    off = {"weighted_dropout": False, "weighted_backward": False, "weighted_max_t": 32}                 # all off by default
    return make_layer(pkg, dev, w, b, expect_defaults=off, precision=precision, weighted_dropout=dropout, weighted_backward=backward,
                      weighted_max_t=max_t)


def _made(calls, before=None):
    return {k: v - (before or {}).get(k, 0) for k, v in calls.items() if v - (before or {}).get(k, 0)}


_INPUTS, _MASKS, _Y64 = {}, {}, {}


def _inputs(dev, B, T, K, F, gates):
    key = (B, T, K, F)
    if key not in _INPUTS:
        c = br.case_inputs(B, T, K, F, 5000 + 13 * B + 7 * T + F, gates=gates, graph="weighted")
        _INPUTS[key] = {k: v.to(dev) for k, v in c.items()}
    return _INPUTS[key]


def _keep_factors(pkg, dev, B, T, F, stream, p=P_DROP, seed=SEED):
    """Keep factors [B,T,F] of one stream as ``ggcn_dropout_mask`` writes them (float64); stream 0: None."""
    if stream == 0:
        return None
    key = (B, T, F, stream, p, seed)
    if key not in _MASKS:
        m = drop_mask(pkg, dev, B * T, F, p, seed, stream)
        assert set(m.unique().tolist()) <= {0.0, float(np.float32(1.0) / np.float32(1.0 - p))}
        _MASKS[key] = m.view(B, T, F).double()
    return _MASKS[key]


def _keep(pkg, dev, B, T, F, triple):
    return tuple(_keep_factors(pkg, dev, B, T, F, s) for s in triple)


def _y64(dev, c, key):
    if key not in _Y64:
        _Y64[key] = br.layer_output(c["x"], c["adj"], c["w"], c["b"])
    return _Y64[key]


# ================================================================ 1. forward against float64
@pytest.mark.parametrize("precision", ["f16mx8", "bf16x3"])
@pytest.mark.parametrize("B,T,K,F,gates", SHAPES32 + SHAPES_WIDE)
def test_forward_vs_float64(pkg, dev, monkeypatch, B, T, K, F, gates, precision):
    c = _inputs(dev, B, T, K, F, gates)
    m = _layer(pkg, dev, c["w"], c["b"], precision, max_t=128 if T > 32 else None)
    csr = pkg.BatchedCSR.from_dense(c["adj"], binary=False)
    assert m.takes_weighted_dropout_path(c["x"], csr)
    y = _y64(dev, c, (B, T, K, F))
    tol = br.TOL[precision] / (1.0 - P_DROP)
    entry, other = (WIDE, FWD) if T > 32 else (FWD, WIDE)
    calls = count_calls(monkeypatch, COUNTED)
    worst = 0.0
    for triple in TRIPLES:
        ks, ka, kb = _keep(pkg, dev, B, T, F, triple)
        delta = br.tie_delta(precision, P_DROP)      # (the share alone is checked: the pools below are compared unmasked)
        share = br.masked_share(br.pool_tie_mask(br.gated(y, c["ga"], ka), delta), br.pool_tie_mask(br.gated(y, c["gb"], kb), delta))
        print("%dx%dx%dx%d %s %s: %.2f %% of the pools within the tie distance" % (B, T, K, F, precision, triple, 100 * share))
        assert share <= br.MAX_MASKED
        before = dict(calls)
        with torch.no_grad():
            out, pa, pb = m.forward_gated(c["x"], csr, store_gate=c["sg"], pool_gate_a=c["ga"], pool_gate_b=c["gb"], want_pool_a=True,
                                          want_pool_b=True, dropout=(P_DROP, SEED, triple))
        torch.cuda.synchronize()
        assert _made(calls, before) == {entry: 1}, "%s: the forward made %s" % (triple, _made(calls, before))
        worst = max(worst, _gate(out, br.gated(y, c["sg"], ks), "out %s" % (triple,), tol))
        worst = max(worst, _gate(pa, torch.max(br.gated(y, c["ga"], ka), 1)[0], "pool a %s" % (triple,), tol))
        worst = max(worst, _gate(pb, torch.max(br.gated(y, c["gb"], kb), 1)[0], "pool b %s" % (triple,), tol))
    assert calls[other] == 0 and calls["ggcn_linear"] == 0 and calls["ggcn_aggregate"] == 0
    print("%dx%dx%dx%d %s: worst |diff| / gate %.3f" % (B, T, K, F, precision, worst))


@pytest.mark.parametrize("B,T,K,F,gates", [SHAPES32[0], SHAPES_WIDE[0]])
def test_forward_through_the_c_abi_leaves_the_padding_alone(pkg, dev, B, T, K, F, gates):
    """ldo = F + 4, the pad columns and the row after the last one NaN before and after; without `out`, the pools alone."""
    from ed_gated_gcn_amd import _capi
    lib = pkg.load_library()
    p, st = _capi.ptr, _capi.stream_of(dev)
    c = _inputs(dev, B, T, K, F, gates)
    m = _layer(pkg, dev, c["w"], c["b"], "f16mx8", max_t=128)
    csr = pkg.BatchedCSR.from_dense(c["adj"], binary=False)
    pack = m._packed_weight(lib, st, precision="f16mx8")
    x2d = c["x"].reshape(B * T, K)
    triple = (2, 1, 2)
    ks, ka, kb = _keep(pkg, dev, B, T, F, triple)
    y = _y64(dev, c, (B, T, K, F))
    tol = br.TOL["f16mx8"] / (1.0 - P_DROP)
    ld = F + 4
    for with_out in (True, False):
        out = torch.full((B * T + 1, ld), NAN, device=dev)
        pa, pb = torch.full((B + 1, F), NAN, device=dev), torch.full((B + 1, F), NAN, device=dev)
        tail = (B, T, K, F, p(c["sg"]), p(c["ga"]), p(c["gb"]), p(out) if with_out else None, ld, p(pa), p(pb), _capi.PREC["f16mx8"],
                P_DROP, SEED) + triple + (st,)
        if T > 32:
            _capi.check(lib.ggcn_layer_fused_weighted_wide_drop(p(x2d), K, p(pack), p(csr.graph_ops_weighted_wide()), p(m.bias.detach()), *tail), WIDE)
        else:
            zero = torch.zeros(F, device=dev)
            _capi.check(lib.ggcn_layer_fused_weighted_drop(p(x2d), K, p(pack), p(csr.graph_ops_weighted(1)), p(m.bias.detach()), p(zero), *tail), FWD)
        torch.cuda.synchronize()
        if with_out:
            assert bool(torch.isnan(out[B * T]).all()) and bool(torch.isnan(out[:, F:]).all()), "out written outside its rows"
            _gate(out[:B * T, :F].reshape(B, T, F), br.gated(y, c["sg"], ks), "out (ldo = F + 4)", tol)
        else:
            assert bool(torch.isnan(out).all())
        assert bool(torch.isnan(pa[B]).all()) and bool(torch.isnan(pb[B]).all())
        _gate(pa[:B], torch.max(br.gated(y, c["ga"], ka), 1)[0], "pool a", tol)
        _gate(pb[:B], torch.max(br.gated(y, c["gb"], kb), 1)[0], "pool b", tol)


# ================================================================ 2. p = 0, the same seed, another seed
@pytest.mark.parametrize("precision", ["f16mx8", "bf16x3"])
@pytest.mark.parametrize("B,T,K,F,gates", [SHAPES32[1], SHAPES32[3], SHAPES_WIDE[3], SHAPES_WIDE[2]])
def test_p0_is_the_launch_without_dropout_and_a_seed_is_a_seed(pkg, dev, monkeypatch, B, T, K, F, gates, precision):
    c = _inputs(dev, B, T, K, F, gates)
    m = _layer(pkg, dev, c["w"], c["b"], precision, max_t=128)
    csr = pkg.BatchedCSR.from_dense(c["adj"], binary=False)
    calls = count_calls(monkeypatch, COUNTED)

    def run(dropout):
        with torch.no_grad():
            r = m.forward_gated(c["x"], csr, store_gate=c["sg"], pool_gate_a=c["ga"], pool_gate_b=c["gb"], want_pool_a=True, want_pool_b=True,
                                dropout=dropout)
        torch.cuda.synchronize()
        return r
    plain = run(None)
    assert _made(calls) == {"ggcn_layer_fused_weighted_wide" if T > 32 else "ggcn_layer_fused_weighted": 1}
    p0 = run((0.0, SEED, (0, 1, 2)))
    assert calls[WIDE if T > 32 else FWD] == 1
    for a, b, name in zip(plain, p0, ("out", "pool a", "pool b")):
        assert torch.equal(a, b), "p = 0: %s differs from the launch without dropout" % name
    first, again, other = run((P_DROP, SEED, (2, 1, 2))), run((P_DROP, SEED, (2, 1, 2))), run((P_DROP, SEED + 1, (2, 1, 2)))
    for a, b, name in zip(first, again, ("out", "pool a", "pool b")):
        assert torch.equal(a, b), "the same seed twice: %s differs" % name
    assert not torch.equal(first[0], other[0]) and not torch.equal(first[0], plain[0])
    dropped = float((first[0] == 0).float().mean())
    assert abs(dropped - P_DROP) < 0.05, "share of zeros in out %.3f" % dropped


# ================================================================ 3. the backward kernel through the C ABI
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
    plan = [(0, "full", t) for t in TRIPLES] + [(4, v, TRIPLES[i % 3]) for i, v in enumerate(VARIANTS)]
    for pad, variant, triple in plan:
        ld = F + pad
        ob, db = _hostile(out, pad), _hostile(d_out, pad)
        keep = _keep(pkg, dev, B, T, F, triple)
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
        what = "%dx%dx%d ld=F+%d %s streams %s" % (B, T, F, pad, variant, triple)
        runs = []
        for _ in range(2):
            dh = torch.full((B * T + 1, ld), NAN, device=dev)
            dy = torch.full((B * T + 1, ld), NAN, device=dev) if want_dy else None
            o = {k: torch.full((B, F), NAN, device=dev) for k in ("d_sg", "d_ga", "d_gb", "d_bsum")}
            _capi.check(lib.ggcn_gate_pool_backward_weighted_drop(
                p(ob), ld, p(use["sg"]), p(use["ga"]), p(use["gb"]), p(db) if use["d_out"] is not None else None, ld, p(use["d_pa"]),
                p(use["d_pb"]), p(ops), p(inv), B, T, F, p(dh), ld, p(dy), ld, p(o["d_sg"]) if use["sg"] is not None else None,
                p(o["d_ga"]) if use["d_pa"] is not None else None, p(o["d_gb"]) if use["d_pb"] is not None else None, p(o["d_bsum"]),
                P_DROP, SEED, *triple, st), BWD)
            o["dH"], o["dY"] = dh, dy
            runs.append(o)
        torch.cuda.synchronize()
        a, b2 = runs
        for k in a:
            if a[k] is not None:
                assert torch.equal(torch.nan_to_num(a[k], nan=-7.0), torch.nan_to_num(b2[k], nan=-7.0)), "%s: two runs differ in %s" % (what, k)
        ref = _statement64(out.view(B, T, F), use["sg"], use["ga"], use["gb"], None if use["d_out"] is None else d_out.view(B, T, F),
                           use["d_pa"], use["d_pb"], adj, inv, keep)
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
            _capi.check(lib.ggcn_gate_pool_backward_drop(p(out), F, p(sg), p(ga), p(gb), p(d_out), F, p(d_pa), p(d_pb), B, T, F, p(dy2), F,
                                                         None, None, None, None, P_DROP, SEED, *triple, st), GPB_DROP)
            _capi.check(lib.ggcn_aggregate_t(p(dy2), F, p(csr_t.rowptr), p(csr_t.colidx), p(csr_t.vals), p(inv), B, T, F, p(dh2), F, st), AGG_T)
            top = float(ref["dH"].abs().max())
            err = float((a["dH"][:B * T, :F].double() - dh2.double()).abs().max())
            assert err <= 4e-6 * top, "%s: dH against the two calls: max|diff| %.3g > %.3g" % (what, err, 4e-6 * top)
            err = float((a["dY"][:B * T, :F].double() - dy2.double()).abs().max())
            assert err <= 4e-6 * float(ref["dY"].abs().max()), "%s: dY against ggcn_gate_pool_backward_drop: max|diff| %.3g" % (what, err)
    print("%dx%dx%d: worst |diff| / max|ref| %s (gate 2e-6)" % (B, T, F, {k: "%.2g" % v for k, v in worst.items()}))


@pytest.mark.parametrize("F", [4, 64, 260])
@pytest.mark.parametrize("T", [1, 5, 31, 32])
def test_backward_kernel_vs_float64(pkg, dev, T, F):
    _kernel_case(pkg, dev, 3, T, F)


def test_backward_kernel_more_graphs_than_compute_units(pkg, dev):
    assert 300 > torch.cuda.get_device_properties(dev).multi_processor_count
    _kernel_case(pkg, dev, 300, 31, 64)


def test_backward_kernel_p0_is_the_kernel_without_dropout(pkg, dev):
    from ed_gated_gcn_amd import _capi
    lib = pkg.load_library()
    p, st = _capi.ptr, _capi.stream_of(dev)
    B, T, F = 5, 17, 68
    csr = pkg.BatchedCSR.from_dense(br.case_adjacency(B, T, 11, "weighted").to(dev), binary=False)
    g = torch.Generator(device=dev).manual_seed(3)
    out, d_out = torch.randn(B * T, F, device=dev, generator=g), torch.randn(B * T, F, device=dev, generator=g)
    gates = [torch.rand(B, F, device=dev, generator=g) for _ in range(3)]
    d_pa, d_pb = torch.randn(B, F, device=dev, generator=g), torch.randn(B, F, device=dev, generator=g)
    res = []
    for tail in ((), (0.0, SEED, 2, 1, 2)):
        o = [torch.full((B * T, F), NAN, device=dev) for _ in range(2)] + [torch.full((B, F), NAN, device=dev) for _ in range(4)]
        entry = BWD if tail else "ggcn_gate_pool_backward_weighted"
        _capi.check(getattr(lib, entry)(p(out), F, *(p(t) for t in gates), p(d_out), F, p(d_pa), p(d_pb), p(csr.graph_ops_weighted_t()),
                                        p(csr.inv_denominators()), B, T, F, p(o[0]), F, p(o[1]), F, *(p(t) for t in o[2:]), *tail, st), entry)
        res.append(o)
    torch.cuda.synchronize()
    for a, b in zip(*res):
        assert torch.equal(a, b) and not bool(torch.isnan(a).any())


# ================================================================ 4. under autograd
STREAMS = (0, 1, 2)
_REF = {}      # case -> the float64 reference, computed once and left unchanged


def _reference(pkg, dev, B, T, K, F, gates, precision="f16mx8"):
    key = (B, T, K, F)
    if key in _REF:
        return _REF[key]
    c = _inputs(dev, B, T, K, F, gates)
    keep = _keep(pkg, dev, B, T, F, STREAMS)
    ma, mb = br.layer_tie_masks(c["x"], c["adj"], c["w"], c["b"], c["ga"], c["gb"], br.tie_delta(precision, P_DROP), keep=keep)
    share = br.masked_share(ma, mb)
    print("%s: %.2f %% of the pools masked" % (key, 100 * share))
    assert share <= br.MAX_MASKED
    if key == (6, 16, 32, 4):
        assert share == 0.0
    rs = (c["r1"], c["r2"] * (~ma), c["r3"] * (~mb))
    ref = {k: c[k].double().requires_grad_() for k in ("x", "w", "b", "sg", "ga", "gb", "adj")}
    o64, a64, b64 = br.gated_layer_ref(ref["x"], ref["adj"], ref["w"], ref["b"], ref["sg"], ref["ga"], ref["gb"], keep=keep)
    ((o64 * rs[0]).sum() + (a64 * rs[1]).sum() + (b64 * rs[2]).sum()).backward()
    _REF[key] = (c, rs, {k: v.grad.clone() for k, v in ref.items()})
    return _REF[key]


def _run(pkg, dev, c, rs, adj_grad, backward, max_t=None):
    """forward_gated + backward of the backward tests' loss; returns (gradients, adj.grad, the layer's BatchedCSR)."""
    from ed_gated_gcn_amd import csr as csr_mod
    m = _layer(pkg, dev, c["w"], c["b"], "f16mx8", dropout=True, backward=backward, max_t=max_t)
    leaves = {k: c[k].clone().requires_grad_() for k in ("x", "sg", "ga", "gb")}
    adj = c["adj"].clone().requires_grad_(adj_grad)
    out, pa, pb = m.forward_gated(leaves["x"], adj, store_gate=leaves["sg"], pool_gate_a=leaves["ga"], pool_gate_b=leaves["gb"],
                                  want_pool_a=True, want_pool_b=True, dropout=(P_DROP, SEED, STREAMS))
    ((out * rs[0]).sum() + (pa * rs[1]).sum() + (pb * rs[2]).sum()).backward()
    torch.cuda.synchronize()
    g = {k: v.grad for k, v in leaves.items()}
    g["w"], g["b"] = m.weight.grad, m.bias.grad
    return g, adj.grad, csr_mod.cached_from_dense(adj, binary=m.binary_adj)


def _check_grads(got, d_adj, ref, what, rel=5e-4):
    worst = 0.0
    for k, label in (("x", "dX"), ("w", "dW"), ("b", "db"), ("sg", "d store gate"), ("ga", "d gate a"), ("gb", "d gate b")):
        assert got[k] is not None, "%s: %s is missing" % (what, label)
        worst = max(worst, _close32(got[k], ref[k], label, rel))
    if d_adj is not None:
        assert d_adj.shape == ref["adj"].shape and not bool(torch.isnan(d_adj).any())
        worst = max(worst, _close32(d_adj, ref["adj"], what + " d adj", rel))
    return worst


@pytest.mark.parametrize("B,T,K,F,gates", SHAPES32)
def test_under_autograd(pkg, dev, monkeypatch, B, T, K, F, gates):
    what = "%dx%dx%dx%d" % (B, T, K, F)
    c, rs, ref = _reference(pkg, dev, B, T, K, F, gates)
    calls = count_calls(monkeypatch, COUNTED)
    worst = 0.0
    for backward in (True, False):
        for adj_grad in (False, True):
            before = dict(calls)
            got, d_adj, csr = _run(pkg, dev, c, rs, adj_grad, backward)
            made = _made(calls, before)
            linear = made.pop("ggcn_linear", 0)        # dX, and `hidden` again for an adjacency gradient
            assert linear == (2 if adj_grad else 1), "%s: %d calls of ggcn_linear" % (what, linear)
            want = {FWD: 1}
            want.update({BUILD_T: 1, BWD: 1} if backward else {GPB_DROP: 1, AGG_T: 1})
            if adj_grad:
                want[ADJ_GRAD] = 1
            assert made == want, "%s adj.requires_grad=%s weighted_backward=%s: %s" % (what, adj_grad, backward, made)
            assert not csr.is_binary and (csr._t is None) == backward, "%s: the transposed CSR" % what
            assert (d_adj is not None) == adj_grad
            worst = max(worst, _check_grads(got, d_adj, ref, what))
    print("%s: worst gradient |diff| / scale %.3g (gate 5e-4)" % (what, worst))


@pytest.mark.parametrize("B,T,K,F,gates", [SHAPES_WIDE[0], SHAPES_WIDE[3]])
def test_under_autograd_33_to_128_nodes_keep_the_two_call_backward(pkg, dev, monkeypatch, B, T, K, F, gates):
    what = "%dx%dx%dx%d" % (B, T, K, F)
    c, rs, ref = _reference(pkg, dev, B, T, K, F, gates)
    calls = count_calls(monkeypatch, COUNTED)
    for adj_grad in (False, True):
        before = dict(calls)
        got, d_adj, csr = _run(pkg, dev, c, rs, adj_grad, True, max_t=128)
        made = _made(calls, before)
        made.pop("ggcn_linear")
        want = {WIDE: 1, GPB_DROP: 1, AGG_T: 1}
        if adj_grad:
            want[ADJ_GRAD] = 1
        assert made == want, "%s adj.requires_grad=%s: %s" % (what, adj_grad, made)
        _check_grads(got, d_adj, ref, what)


# ================================================================ 5. where it steps aside
def test_where_it_steps_aside(pkg, dev, monkeypatch):
    B, T, K, F, gates = SHAPES32[0]
    c = _inputs(dev, B, T, K, F, gates)
    dropout = (P_DROP, SEED, STREAMS)
    kw = dict(store_gate=c["sg"], pool_gate_a=c["ga"], pool_gate_b=c["gb"], want_pool_a=True, want_pool_b=True)
    refusal = "dropout= needs the one-launch layer"
    # the option off: refused as before, with and without autograd
    off = _layer(pkg, dev, c["w"], c["b"], dropout=False, backward=True)
    with pytest.raises(RuntimeError, match=refusal):
        off.forward_gated(c["x"].clone().requires_grad_(), c["adj"], dropout=dropout, **kw)
    with torch.no_grad(), pytest.raises(RuntimeError, match=refusal):
        off.forward_gated(c["x"], c["adj"], dropout=dropout, **kw)
    on = _layer(pkg, dev, c["w"], c["b"])
    # bfloat16 features: the weighted launches take float32 only
    with torch.no_grad(), pytest.raises(RuntimeError, match=refusal):
        on.forward_gated(c["x"].to(torch.bfloat16), c["adj"], dropout=dropout, **kw)
    # 33 nodes with weighted_max_t = 32
    c33 = _inputs(dev, *SHAPES_WIDE[0])
    on33 = _layer(pkg, dev, c33["w"], c33["b"])
    with torch.no_grad(), pytest.raises(RuntimeError, match=refusal):
        on33.forward_gated(c33["x"], c33["adj"], dropout=dropout, store_gate=c33["sg"])
    # under autograd a dropped store gate wants its pools on the same stream
    with pytest.raises(RuntimeError, match="dropout streams"):
        on.forward_gated(c["x"].clone().requires_grad_(), c["adj"], dropout=(P_DROP, SEED, (1, 2, 0)), **kw)
    # a 0/1 adjacency takes ggcn_layer_fused_drop as ever
    calls = count_calls(monkeypatch, COUNTED)
    binary = (c["adj"] != 0).float()
    with torch.no_grad():
        on.forward_gated(c["x"], binary, dropout=dropout, **kw)
    torch.cuda.synchronize()
    assert _made(calls) == {"ggcn_layer_fused_drop": 1}


# ================================================================ 6. the classifier
def test_classifier_trains_a_weighted_graph_inside_the_launches(pkg, dev, monkeypatch):
    import types

    class _Bert(torch.nn.Module):
        def forward(self, ids, seg, output_all_encoded_layers=True):
            gen = torch.Generator(device=ids.device).manual_seed(1)
            return ([torch.randn(ids.shape[0], ids.shape[1], 768, device=ids.device, generator=gen) for _ in range(12)],
                    torch.zeros(ids.shape[0], 768, device=ids.device))
    opt = types.SimpleNamespace(dropout=0.5, polarities_dim=34, device=dev, ggcn_weighted_dropout=True, ggcn_weighted_backward=True)
    m = pkg.GatedGCNEventDetector(_Bert(), opt)
    assert m.gc1.weighted_dropout and m.gc2.weighted_dropout and m.gc1.weighted_backward and m.gc2.weighted_backward
    gen = torch.Generator().manual_seed(0)
    for p in m.parameters():
        if p.dim() > 1:
            torch.nn.init.xavier_uniform_(p, generator=gen)
        else:
            torch.nn.init.uniform_(p, -0.05, 0.05, generator=gen)
    m = m.to(dev)
    with torch.no_grad():
        m.gc1.bias.fill_(5.0)                              # gcn1 > 0 everywhere: x1 = 0 iff every token's gate entry was dropped
    inputs = {k: v.to(dev) for k, v in ace_batch(np.random.default_rng(0), 32, 31, 60, weights=(0.25, 2.0)).items()}
    seen = {}
    orig = m.gc1.forward_gated

    def spy(*a, **k):                                      # x1 = the first pool of layer 1 (bert_amir5.py:627-635)
        r = orig(*a, **k)
        seen["dropout"] = k.get("dropout")
        seen["x1"] = None if r[1] is None else r[1].detach()
        return r
    m.train()
    m.gc1.forward_gated = spy
    calls = count_calls(monkeypatch, COUNTED)
    try:
        for on in (True, False):
            for layer in (m.gc1, m.gc2):
                layer.weighted_dropout = layer.weighted_backward = on
            m.zero_grad()
            seen.clear()
            before = dict(calls)
            logits, xy, kl, scores = m(inputs)
            fwd = _made(calls, before)
            (logits.sum() + xy + kl).backward()
            torch.cuda.synchronize()
            made = _made(calls, before)
            for layer in (m.gc1, m.gc2):
                assert layer.weight.grad is not None and bool(torch.isfinite(layer.weight.grad).all())
            if on:
                assert fwd == {FWD: 2}, "the forward made %s" % fwd
                assert made[BWD] == 2 and made[BUILD_T] == 1 and not any(k in made for k in (GPB, GPB_DROP, AGG_T, "ggcn_aggregate")), made
                assert seen["dropout"] is not None and seen["dropout"][2] == (0, 1, 2), "the layer launch draws the gates' keep factors"
                zero_frac = float((seen["x1"] == 0).float().mean())
                assert zero_frac < 0.02, "pooled features vanish with probability %.2f: the dropout mask is shared by the tokens" % zero_frac
            else:
                assert not any(k in made for k in (FWD, WIDE, BWD)), made
                assert seen["dropout"] is None
    finally:
        m.gc1.forward_gated = orig
