#!/usr/bin/env python3
"""The backward of a layer on a real-valued adjacency of graphs of <= 32 nodes: GraphConvolution.weighted_backward off (the two
calls: ggcn_gate_pool_backward + a transposed CSR + ggcn_aggregate_t) against on (ggcn_graph_operands_weighted_t + ONE launch,
ggcn_gate_pool_backward_weighted), in one process, the variants ALTERNATING group by group after a warm-up (medians over the timed
groups, min..max beside them).

Two things are timed per case.  The replaced STAGE through the C ABI INCLUDING the per-adjacency builders, which a learned graph
pays every step (its adjacency is a new tensor each step): off = BatchedCSR.transposed() with its arrays + the two calls; on =
BatchedCSR.graph_ops_weighted_t() (the builder and the read-back of its flag) + the new launch, without and with the dY store an
adjacency gradient wants.  And the WHOLE layer backward under autograd (forward_gated once, then its backward again and again
with the graph's cached transposed CSR / operand block dropped before every call), without and with adj.requires_grad.

usage: weighted_backward_timing.py [output file]   (writes profiles/weighted_backward_timing.txt by default)"""
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

CASES = ((4096, 32, "sparse"), (4096, 32, "dense"), (512, 24, "sparse"))
H = 768
WARM, GROUPS, SKIP, REPS = 5, 10, 2, 10


def adjacency(B, T, kind, rng):
    if kind == "dense":   # softmax rows over the whole graph: nnz_row = T, ggcn_aggregate_t's worst case
        z = rng.standard_normal((B, T, T))
        e = np.exp(z - z.max(2, keepdims=True))
        return (e / e.sum(2, keepdims=True)).astype(np.float32)
    a = synth.dependency_batch(B, T, 3.0).astype(np.float32)   # a weighted dependency tree
    return a * rng.uniform(0.1, 2.0, size=a.shape).astype(np.float32)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e3


def fresh(csr):
    """What a new adjacency tensor has not got yet: the transposed CSR and the A_w^T operand block."""
    csr._t = None
    csr._graph_ops_wt = None


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "weighted_backward_timing.txt")
    dev = torch.device("cuda:0")
    lib = pkg.load_library()
    p, st = _capi.ptr, _capi.stream_of(dev)
    lines = ["# %s, H = %d, f16mx8; us per call: median (min..max) over %d groups of %d calls, variants alternating" % (
        torch.cuda.get_device_name(0), H, GROUPS - SKIP, REPS)]
    rng = np.random.default_rng(0)
    for B, T, kind in CASES:
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

        # ---- the replaced stage through the C ABI, per-adjacency builders included
        csr = pkg.BatchedCSR.from_dense(adj)
        assert not csr.is_binary and csr.graph_ops_weighted_t() is not None
        inv = csr.inv_denominators()
        with torch.no_grad():
            out = m.forward_gated(x, csr, store_gate=sg)[0].reshape(B * T, F)
        d_out = r1.reshape(B * T, F)
        dy, dh = torch.empty(B * T, F, device=dev), torch.empty(B * T, F, device=dev)
        d = [torch.empty(B, F, device=dev) for _ in range(4)]

        def stage_off():
            fresh(csr)
            _capi.check(lib.ggcn_gate_pool_backward(p(out), F, p(sg), p(ga), p(gb), p(d_out), F, p(r2), p(r3), B, T, F, p(dy), F,
                                                    p(d[0]), p(d[1]), p(d[2]), p(d[3]), st), "ggcn_gate_pool_backward")
            t = csr.transposed()
            _capi.check(lib.ggcn_aggregate_t(p(dy), F, p(t.rowptr), p(t.colidx), p(t.vals), p(inv), B, T, F, p(dh), F, st), "ggcn_aggregate_t")

        def stage_on(with_dy):
            fresh(csr)
            _capi.check(lib.ggcn_gate_pool_backward_weighted(p(out), F, p(sg), p(ga), p(gb), p(d_out), F, p(r2), p(r3),
                                                             p(csr.graph_ops_weighted_t()), p(inv), B, T, F, p(dh), F,
                                                             p(dy) if with_dy else None, F, p(d[0]), p(d[1]), p(d[2]), p(d[3]), st),
                        "ggcn_gate_pool_backward_weighted")

        def build_t():
            fresh(csr)
            t = csr.transposed()
            return t.rowptr

        def build_wt():
            fresh(csr)
            return csr.graph_ops_weighted_t()

        variants = {"stage off (transposed CSR + 2 calls)": stage_off, "stage on": lambda: stage_on(False),
                    "stage on + dY": lambda: stage_on(True), "transposed CSR alone": build_t, "A_w^T operand alone": build_wt}

        # ---- the whole layer backward under autograd
        for adj_grad in (False, True):
            for on in (False, True):
                m.weighted_backward = on
                leaves = [x.clone().requires_grad_(), sg.clone().requires_grad_(), ga.clone().requires_grad_(), gb.clone().requires_grad_()]
                a = adj.clone().requires_grad_(adj_grad)
                o, pa, pb = m.forward_gated(leaves[0], a, store_gate=leaves[1], pool_gate_a=leaves[2], pool_gate_b=leaves[3],
                                            want_pool_a=True, want_pool_b=True)
                loss = (o * r1).sum() + (pa * r2).sum() + (pb * r3).sum()
                inputs = leaves + [m.weight, m.bias] + ([a] if adj_grad else [])
                layer_csr = csr_mod.cached_from_dense(a, binary=m.binary_adj)

                def backward(loss=loss, inputs=inputs, layer_csr=layer_csr, on=on):
                    m.weighted_backward = on      # (read by the backward, not by the forward)
                    fresh(layer_csr)
                    return torch.autograd.grad(loss, inputs, retain_graph=True)

                variants["backward %s%s" % ("on" if on else "off", ", d adj" if adj_grad else "")] = backward

        res = {k: [] for k in variants}
        for _ in range(WARM):
            for fn in variants.values():
                fn()
        torch.cuda.synchronize()
        for group in range(GROUPS):
            for name, fn in variants.items():
                t = timed(fn)
                if group >= SKIP:
                    res[name].append(t)
        stage_off()
        ref = dh.clone()
        stage_on(False)
        diff = float((dh - ref).abs().max()) / float(ref.abs().max())
        line = "B=%d T=%d H=%d %s (nnz/row %.1f): " % (B, T, H, kind, int(csr.rowptr[-1].item()) / float(B * T))
        line += "   ".join("%s %.1f (%.1f..%.1f)" % (k, statistics.median(v), min(v), max(v)) for k, v in res.items())
        line += "   | dH on vs off: max|diff| %.3g of its scale" % diff
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
