#!/usr/bin/env python3
"""The inference block on a real-valued adjacency, option GraphConvolution.weighted_block off against on, in one process, H = 768,
f16mx8 and bf16x3, each form ALONE in steady state: a form is repeated in windows of REPS calls until two consecutive windows agree
within 2 % (the chip has then settled on the clock it holds under that form's load), and the median of the next WINDOWS windows is
the figure (min..max beside it).

off  what gated_gcn_block runs today: two ggcn_layer_fused_weighted launches (gcn1 written and read back) + ggcn_gate_overlap;
     want=("out",): the two launches without the pools of layer 1.
on   ggcn_block_fused_weighted (+ ggcn_overlap_reduce); want=("out",): its W12 column tiles only.

Two figures per form: "built" drops the graph's cached operand blocks before every call (a learned graph is a new tensor every
step: ggcn_graph_operands_weighted for both, ggcn_graph_operands2_weighted and its flag read-back for "on"), "cached" keeps them
(one graph evaluated on many batches of features).

usage: weighted_block_timing.py [output file]   (writes profiles/weighted_block_timing.txt by default)"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ed_gated_gcn_amd as pkg  # noqa: E402
from ed_gated_gcn_amd import synth  # noqa: E402
from ed_gated_gcn_amd import csr as csr_mod  # noqa: E402

CASES = ((4096, 32, "sparse"), (4096, 32, "dense"), (512, 24, "sparse"))
H = 768
REPS, WINDOWS, MAX_SETTLE, AGREE = 10, 5, 20, 0.02


def adjacency(B, T, kind, rng):
    if kind == "dense":   # softmax rows over the whole graph: nnz_row = T
        z = rng.standard_normal((B, T, T))
        e = np.exp(z - z.max(2, keepdims=True))
        return (e / e.sum(2, keepdims=True)).astype(np.float32)
    a = synth.dependency_batch(B, T, 3.0).astype(np.float32)   # a weighted dependency tree
    return a * rng.uniform(0.1, 2.0, size=a.shape).astype(np.float32)


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e3


def steady(fn):
    """us per call: windows until two in a row agree, then the median (min, max) of the next WINDOWS."""
    last = window(fn)
    for _ in range(MAX_SETTLE):
        now = window(fn)
        agreed = abs(now - last) <= AGREE * last
        last = now
        if agreed:
            break
    v = [window(fn) for _ in range(WINDOWS)]
    return statistics.median(v), min(v), max(v)


def fresh(csr):
    """What a new adjacency tensor has not got yet: its operand blocks."""
    csr._graph_ops_w = csr._graph_ops2_w = None


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "weighted_block_timing.txt")
    dev = torch.device("cuda:0")
    pkg.load_library()
    lines = ["# %s, H = %d; us per call of gated_gcn_block without autograd on a real-valued adjacency, each form alone in steady "
             "state: median (min..max) of %d windows of %d calls after two windows agreed within %g %%" % (
                 torch.cuda.get_device_name(0), H, WINDOWS, REPS, 100 * AGREE)]
    rng = np.random.default_rng(0)
    (w1, b1), (w2, b2) = synth.layer_params(H, H, seed=1), synth.layer_params(H, H, seed=2)
    for B, T, kind in CASES:
        x = torch.randn(B, T, H, device=dev)
        g1, g2 = torch.rand(B, H, device=dev), torch.rand(B, H, device=dev)
        adj = torch.from_numpy(adjacency(B, T, kind, rng)).to(dev)
        csr = csr_mod.cached_from_dense(adj)
        assert not csr.is_binary
        nnz = int(csr.rowptr[-1].item()) / float(B * T)
        for precision in ("f16mx8", "bf16x3"):
            layers = []
            for w, b in ((w1, b1), (w2, b2)):
                m = pkg.GraphConvolution(H, H, None).to(dev)
                m.precision = precision
                with torch.no_grad():
                    m.weight.copy_(torch.from_numpy(w))
                    m.bias.copy_(torch.from_numpy(b))
                layers.append(m)
            for want in (None, ("out",)):
                res = {}
                for on in (False, True):
                    for built in (True, False):
                        def call(on=on, built=built):
                            for m in layers:
                                m.weighted_block = on
                            if built:
                                fresh(csr)
                            with torch.no_grad():
                                return pkg.gated_gcn_block(x, csr, g1, g2, *layers, want=want)
                        for m in layers:
                            m.weighted_block = on
                        assert pkg.gated_block.takes_weighted_block_path(x, csr, *layers) == on
                        res["%s, %s" % ("on" if on else "off", "built" if built else "cached")] = steady(call)
                line = "B=%d T=%d H=%d %s (nnz/row %.1f) %s %s: " % (B, T, H, kind, nnz, precision, "all outputs" if want is None else "want=(out,)")
                line += "   ".join("%s %.1f (%.1f..%.1f)" % ((k,) + v) for k, v in res.items())
                print(line, flush=True)
                lines.append(line)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
