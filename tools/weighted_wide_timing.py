#!/usr/bin/env python3
"""A real-valued adjacency on graphs of 33..128 nodes (GraphConvolution.weighted_max_t = 128): the one-launch layer on
ggcn_graph_operands_weighted_wide blocks against ggcn_linear + ggcn_aggregate on the same weighted graph, in one process, the
variants ALTERNATING group by group after a warm-up (medians over the timed groups, min..max beside them); for sparse graphs the
0/1 ggcn_layer_fused on the same sparsity pattern as the yardstick of what the real-valued operand costs; and the operand builder
on its own -- a learned graph pays it every step.  f16mx8 unless a precision is named.

usage: weighted_wide_timing.py [precision] [output file]   (writes profiles/weighted_wide_timing.txt by default)"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ed_gated_gcn_amd as pkg  # noqa: E402
from ed_gated_gcn_amd import _capi, synth  # noqa: E402

CASES = ((512, 100, 768), (1024, 64, 768), (512, 128, 768))
WARM, GROUPS, SKIP, REPS = 30, 12, 2, 20


def adjacency(B, T, kind, rng):
    if kind == "dense":   # softmax rows over the whole graph: nnz_row = T, the aggregation kernel's worst case
        z = rng.standard_normal((B, T, T))
        e = np.exp(z - z.max(2, keepdims=True))
        return (e / e.sum(2, keepdims=True)).astype(np.float32), None
    a = synth.dependency_batch(B, T, 3.0).astype(np.float32)
    return a * rng.uniform(0.1, 2.0, size=a.shape).astype(np.float32), a


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e3


def main():
    precision = sys.argv[1] if len(sys.argv) > 1 else "f16mx8"
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "weighted_wide_timing.txt")
    dev = torch.device("cuda:0")
    lib = pkg.load_library()
    lines = ["# %s, %s; us per call: median (min..max) over %d groups of %d calls, variants alternating" % (
        torch.cuda.get_device_name(0), precision, GROUPS - SKIP, REPS)]
    rng = np.random.default_rng(0)
    for B, T, H in CASES:
        x = torch.randn(B, T, H, device=dev)
        g1, g2 = torch.rand(B, H, device=dev), torch.rand(B, H, device=dev)
        w, b = synth.layer_params(H, H, seed=1)
        m = pkg.GraphConvolution(H, H, None).to(dev)
        m.precision = precision
        with torch.no_grad():
            m.weight.copy_(torch.from_numpy(w))
            m.bias.copy_(torch.from_numpy(b))
        for kind in ("sparse", "dense"):
            wadj, pattern = adjacency(B, T, kind, rng)
            csr_w = pkg.BatchedCSR.from_dense(torch.from_numpy(wadj).to(dev))
            csr_b = None if pattern is None else pkg.BatchedCSR.from_dense(torch.from_numpy(pattern).to(dev))
            assert not csr_w.is_binary and csr_w.graph_ops_weighted_wide() is not None

            def layer(csr, fused, max_t):
                m.fused, m.weighted_max_t = fused, max_t
                return m.forward_gated(x, csr, store_gate=g2, pool_gate_a=g1, pool_gate_b=g2, want_pool_a=True, want_pool_b=True)

            ops = torch.empty(lib.ggcn_graph_operands_weighted_wide_bytes(B, T), dtype=torch.uint8, device=dev)
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
            st = _capi.stream_of(dev)

            def build():
                _capi.check(lib.ggcn_graph_operands_weighted_wide(_capi.ptr(csr_w.rowptr), _capi.ptr(csr_w.colidx), _capi.ptr(csr_w.vals),
                                                                  B, T, _capi.ptr(ops), _capi.ptr(flag), st), "builder")

            variants = {"weighted, one launch": lambda: layer(csr_w, True, 128),
                        "weighted, linear + aggregate": lambda: layer(csr_w, True, 32),
                        "operand builder": build}
            if csr_b is not None:
                variants["0/1, one launch"] = lambda: layer(csr_b, True, 32)
            m.fused, m.weighted_max_t = True, 128
            assert m.takes_weighted_path(x, csr_w)
            res = {k: [] for k in variants}
            with torch.no_grad():
                for _ in range(WARM):
                    for fn in variants.values():
                        fn()
                torch.cuda.synchronize()
                for group in range(GROUPS):
                    for name, fn in variants.items():
                        t = timed(fn)
                        if group >= SKIP:
                            res[name].append(t)
                one, two = layer(csr_w, True, 128), layer(csr_w, True, 32)
            diff = max(float((a - c).abs().max()) for a, c in zip(one, two))
            scale = max(1.0, float(two[0].abs().max()))
            line = "B=%d T=%d H=%d %s (nnz/row %.1f): " % (B, T, H, kind, int(csr_w.rowptr[-1].item()) / float(B * T))
            line += "   ".join("%s %.1f (%.1f..%.1f)" % (k, statistics.median(v), min(v), max(v)) for k, v in res.items())
            line += "   | one launch vs two: max|diff| %.3g of the scale" % (diff / scale)
            print(line, flush=True)
            lines.append(line)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
