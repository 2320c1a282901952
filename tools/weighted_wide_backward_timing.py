#!/usr/bin/env python3
"""The backward of a layer on a REAL-valued adjacency of graphs of 33..128 nodes, without gate dropout:
GraphConvolution.weighted_wide_backward off (ggcn_gate_pool_backward + a transposed CSR + ggcn_aggregate_t: the path of every
commit before the option) against on (ggcn_graph_operands_weighted_wide_t + ONE launch, ggcn_gate_pool_backward_weighted_wide),
in one process, each form ALONE in steady state: a warm-up, then the timed groups back to back (medians over the groups,
min..max beside them), then the next form.  Two graph kinds: sparse (a dependency parse, 3 edges per row, real weights) and
dense (softmax rows over the whole graph, a learned graph).

Everything is timed with the per-adjacency builders INSIDE ("built": the transposed CSR / the operand are dropped before every
call), since a learned graph is a new tensor each step and pays them every step:
  stage off / on / on + dY   the replaced stage through the C ABI (on + dY: with the dY store an adjacency gradient wants)
  transposed CSR / operand   the two builders alone (the operand's includes the read-back of its flag)
  backward off / on          the WHOLE layer backward under autograd (forward_gated once, then its backward again and again)
  backward + d adj off / on  the same with ``adj.requires_grad``
The "cached" stage columns (builders outside) say what the launch alone costs.

usage: weighted_wide_backward_timing.py [output file]   (writes profiles/weighted_wide_backward_timing.txt by default)"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ed_gated_gcn_amd as pkg  # noqa: E402
from ed_gated_gcn_amd import _capi, synth  # noqa: E402
from ed_gated_gcn_amd import csr as csr_mod  # noqa: E402

CASES = ((512, 100), (1024, 64), (512, 128), (64, 100))
KINDS = ("sparse", "dense")
H = 768
WARM, GROUPS, REPS = 3, 7, 5


def adjacency(B, T, kind, rng):
    if kind == "dense":   # softmax rows over the whole graph: nnz_row = T, the transposed aggregation's worst case
        z = rng.standard_normal((B, T, T))
        e = np.exp(z - z.max(2, keepdims=True))
        return (e / e.sum(2, keepdims=True)).astype(np.float32)
    a = synth.dependency_batch(B, T, 3.0).astype(np.float32)
    return a * rng.uniform(0.1, 2.0, size=a.shape).astype(np.float32)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e3


def alone(fn):
    """``fn`` alone in steady state: (median, min, max) us over the timed groups."""
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    v = [timed(fn) for _ in range(GROUPS)]
    return statistics.median(v), min(v), max(v)


def fresh(csr):
    """What a new adjacency tensor has not got yet: the transposed CSR and the A_w^T operand.  These are BatchedCSR's
    private cache slots: the class has ``__slots__``, so a renamed slot raises here instead of leaving the cache in place, and
    ``used`` checks after every timed call that the builder did run."""
    csr._t = None
    csr._graph_ops_wwt = None


def used(csr, slot):
    """The builder behind ``slot`` ran in the call just made."""
    assert getattr(csr, slot) is not None, "%s was not built by this call: the 'built' columns would be the cached path" % slot


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "weighted_wide_backward_timing.txt")
    dev = torch.device("cuda:0")
    lib = pkg.load_library()
    p, st = _capi.ptr, _capi.stream_of(dev)
    rng = np.random.default_rng(0)
    lines = ["# %s, H = %d, f16mx8; us per call: median (min..max) over %d groups of %d calls, each form alone in steady state" % (
        torch.cuda.get_device_name(0), H, GROUPS, REPS)]
    for (B, T), kind in ((c, k) for c in CASES for k in KINDS):
        F = H
        adj = torch.from_numpy(adjacency(B, T, kind, rng)).to(dev)
        x = torch.randn(B, T, H, device=dev)
        sg, ga, gb = (torch.rand(B, H, device=dev) for _ in range(3))
        r1, r2, r3 = torch.randn(B, T, H, device=dev), torch.randn(B, H, device=dev), torch.randn(B, H, device=dev)
        w, b = synth.layer_params(H, H, seed=1)
        m = pkg.GraphConvolution(H, H, None).to(dev)
        with torch.no_grad():
            m.weight.copy_(torch.from_numpy(w))
            m.bias.copy_(torch.from_numpy(b))

        csr = pkg.BatchedCSR.from_dense(adj, binary=False)
        assert not csr.is_binary and csr.graph_ops_weighted_wide_t() is not None
        inv = csr.inv_denominators()
        with torch.no_grad():
            out = m.forward_gated(x, csr, store_gate=sg)[0].reshape(B * T, F)
        d_out = r1.reshape(B * T, F)
        dy, dh = torch.empty(B * T, F, device=dev), torch.empty(B * T, F, device=dev)
        d = [torch.empty(B, F, device=dev) for _ in range(4)]

        def stage_off(built):
            if built:
                fresh(csr)
            _capi.check(lib.ggcn_gate_pool_backward(p(out), F, p(sg), p(ga), p(gb), p(d_out), F, p(r2), p(r3), B, T, F, p(dy), F,
                                                    p(d[0]), p(d[1]), p(d[2]), p(d[3]), st), "ggcn_gate_pool_backward")
            t = csr.transposed()
            _capi.check(lib.ggcn_aggregate_t(p(dy), F, p(t.rowptr), p(t.colidx), p(t.vals), p(inv), B, T, F, p(dh), F, st), "ggcn_aggregate_t")
            used(csr, "_t")

        def stage_on(built, store_dy):
            if built:
                fresh(csr)
            _capi.check(lib.ggcn_gate_pool_backward_weighted_wide(
                p(out), F, p(sg), p(ga), p(gb), p(d_out), F, p(r2), p(r3), p(csr.graph_ops_weighted_wide_t()), p(inv), B, T, F, p(dh), F,
                p(dy) if store_dy else None, F, p(d[0]), p(d[1]), p(d[2]), p(d[3]), st), "ggcn_gate_pool_backward_weighted_wide")
            used(csr, "_graph_ops_wwt")

        def build_t():
            fresh(csr)
            return csr.transposed().rowptr

        def build_operand():
            fresh(csr)
            return csr.graph_ops_weighted_wide_t()

        variants = {"stage off": lambda: stage_off(True), "stage on": lambda: stage_on(True, False), "stage on + dY": lambda: stage_on(True, True),
                    "stage off cached": lambda: stage_off(False), "stage on cached": lambda: stage_on(False, False),
                    "stage on + dY cached": lambda: stage_on(False, True),
                    "transposed CSR alone": build_t, "operand alone": build_operand}

        # ---- the whole layer backward under autograd, builders inside
        for need_adj in (False, True):
            for on in (False, True):
                m.weighted_wide_backward = on
                leaves = [x.clone().requires_grad_(), sg.clone().requires_grad_(), ga.clone().requires_grad_(), gb.clone().requires_grad_()]
                a = adj.clone().requires_grad_(need_adj)
                o, pa, pb = m.forward_gated(leaves[0], a, store_gate=leaves[1], pool_gate_a=leaves[2], pool_gate_b=leaves[3],
                                            want_pool_a=True, want_pool_b=True)
                loss = (o * r1).sum() + (pa * r2).sum() + (pb * r3).sum()
                inputs = leaves + [m.weight, m.bias] + ([a] if need_adj else [])
                layer_csr = csr_mod.cached_from_dense(a, binary=m.binary_adj)

                def backward(loss=loss, inputs=inputs, layer_csr=layer_csr, on=on):
                    m.weighted_wide_backward = on      # (read by the backward, not by the forward)
                    fresh(layer_csr)
                    grads = torch.autograd.grad(loss, inputs, retain_graph=True)
                    used(layer_csr, "_graph_ops_wwt" if on else "_t")
                    return grads

                variants["backward%s %s" % (" + d adj" if need_adj else "", "on" if on else "off")] = backward

        res = {k: alone(fn) for k, fn in variants.items()}
        stage_off(False)
        ref = dh.clone()
        stage_on(False, False)
        diff = float((dh - ref).abs().max()) / float(ref.abs().max())
        line = "B=%d T=%d H=%d %s: " % (B, T, H, kind)
        line += "   ".join("%s %.1f (%.1f..%.1f)" % ((k,) + v) for k, v in res.items())
        line += "   | dH on vs off: max|diff| %.3g of its scale" % diff
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
