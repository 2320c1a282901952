#!/usr/bin/env python3
"""One gated layer's TRAINING step (forward + backward) on a real-valued adjacency under the gates' dropout, in one process, the
variants ALTERNATING group by group after a warm-up (medians over the timed groups, min..max beside them), H = 768, f16mx8.

off  what the classifier does without GraphConvolution.weighted_dropout (classifier.py, the `elif dropping:` branch): the plain
     weighted layer launch under autograd, then the reference's own ops -- both gates repeated to [B,T,H], two F.dropout, the
     [B,T,H] products and torch.max -- and PyTorch autograd through them.
on   the new launches: forward_gated(..., dropout=(p, seed, (0, 1, 2))) draws the keep factors inside ggcn_layer_fused_weighted_drop
     (33..128 nodes: ggcn_layer_fused_weighted_wide_drop); the backward is ggcn_gate_pool_backward_drop + a transposed CSR +
     ggcn_aggregate_t, or with weighted_backward ("on + wb", <= 32 nodes) one ggcn_gate_pool_backward_weighted_drop launch.

A learned graph is a new tensor every step, so the graph's cached operand blocks and transposed CSR are dropped before every call:
the per-adjacency builders are inside every figure.  Each shape runs on a sparse weighted tree and on dense softmax rows, without
and with adj.requires_grad.

usage: weighted_dropout_timing.py [output file]   (writes profiles/weighted_dropout_timing.txt by default)"""
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ed_gated_gcn_amd as pkg  # noqa: E402
from ed_gated_gcn_amd import synth  # noqa: E402
from ed_gated_gcn_amd import csr as csr_mod  # noqa: E402

CASES = ((4096, 32, 32, (False, True)), (512, 100, 128, (False,)))   # B, T, weighted_max_t, the weighted_backward settings
H, P_DROP = 768, 0.25
WARM, GROUPS, REPS = 3, 8, 10


def adjacency(B, T, kind, rng):
    if kind == "dense":   # softmax rows over the whole graph: nnz_row = T
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
    """What a new adjacency tensor has not got yet: its operand blocks and its transposed CSR."""
    csr._t = csr._graph_ops_w = csr._graph_ops_ww = csr._graph_ops_wt = None


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "weighted_dropout_timing.txt")
    dev = torch.device("cuda:0")
    pkg.load_library()
    lines = ["# %s, H = %d, f16mx8, p = %g; us per training step of one gated layer (forward + backward, per-adjacency builders "
             "included): median (min..max) over %d groups of %d calls, variants alternating" % (
                 torch.cuda.get_device_name(0), H, P_DROP, GROUPS, REPS)]
    rng = np.random.default_rng(0)
    for B, T, max_t, backwards in CASES:
        x0 = torch.randn(B, T, H, device=dev)
        g1, g2 = torch.rand(B, H, device=dev), torch.rand(B, H, device=dev)
        r1, r2, r3 = torch.randn(B, T, H, device=dev), torch.randn(B, H, device=dev), torch.randn(B, H, device=dev)
        w, b = synth.layer_params(H, H, seed=1)
        m = pkg.GraphConvolution(H, H, None).to(dev)
        m.precision, m.weighted_max_t = "f16mx8", max_t
        with torch.no_grad():
            m.weight.copy_(torch.from_numpy(w))
            m.bias.copy_(torch.from_numpy(b))
        for kind in ("sparse", "dense"):
            adj0 = torch.from_numpy(adjacency(B, T, kind, rng)).to(dev)
            variants = {}
            for adj_grad in (False, True):
                leaves = [x0.clone().requires_grad_(), g1.clone().requires_grad_(), g2.clone().requires_grad_()]
                a = adj0.clone().requires_grad_(adj_grad)
                inputs = leaves + [m.weight, m.bias] + ([a] if adj_grad else [])
                layer_csr = csr_mod.cached_from_dense(a, binary=m.binary_adj)
                assert not layer_csr.is_binary
                tag = ", d adj" if adj_grad else ""

                def off(leaves=leaves, a=a, inputs=inputs, layer_csr=layer_csr):
                    m.weighted_dropout = m.weighted_backward = False
                    fresh(layer_csr)
                    y = m(leaves[0], a)                                                   # the plain weighted layer launch
                    gate1 = F_.dropout(leaves[1][:, None, :].expand(-1, T, -1), P_DROP)   # classifier.py: repeat, then dropout
                    gate2 = F_.dropout(leaves[2][:, None, :].expand(-1, T, -1), P_DROP)
                    x1, y1 = torch.max(y * gate1, 1)[0], torch.max(y * gate2, 1)[0]
                    loss = (y * r1).sum() + (x1 * r2).sum() + (y1 * r3).sum()
                    return torch.autograd.grad(loss, inputs)

                def on(wb, leaves=leaves, a=a, inputs=inputs, layer_csr=layer_csr):
                    m.weighted_dropout, m.weighted_backward = True, wb
                    fresh(layer_csr)
                    y, x1, y1 = m.forward_gated(leaves[0], a, pool_gate_a=leaves[1], pool_gate_b=leaves[2], want_pool_a=True,
                                                want_pool_b=True, dropout=(P_DROP, 2 ** 40 + 99, (0, 1, 2)))
                    loss = (y * r1).sum() + (x1 * r2).sum() + (y1 * r3).sum()
                    return torch.autograd.grad(loss, inputs)

                variants["off" + tag] = off
                for wb in backwards:
                    variants["on%s%s" % (" + wb" if wb else "", tag)] = lambda wb=wb, on=on: on(wb)
            m.weighted_dropout = True
            assert m.takes_weighted_dropout_path(x0, csr_mod.cached_from_dense(adj0, binary=m.binary_adj))
            res = {k: [] for k in variants}
            for _ in range(WARM):
                for fn in variants.values():
                    fn()
            torch.cuda.synchronize()
            for _ in range(GROUPS):
                for name, fn in variants.items():
                    res[name].append(timed(fn))
            nnz = int(csr_mod.cached_from_dense(adj0, binary=m.binary_adj).rowptr[-1].item()) / float(B * T)
            line = "B=%d T=%d H=%d %s (nnz/row %.1f): " % (B, T, H, kind, nnz)
            line += "   ".join("%s %.1f (%.1f..%.1f)" % (k, statistics.median(v), min(v), max(v)) for k, v in res.items())
            print(line, flush=True)
            lines.append(line)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
