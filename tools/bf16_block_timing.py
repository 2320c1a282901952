#!/usr/bin/env python3
"""bfloat16 features, inference: the gated block with GraphConvolution.bf16_block off (the default: one launch per layer) and on
(ggcn_block_fused_bf16 for graphs of <= 32 nodes; ggcn_aggregate_bf16 + one folded layer launch for 33..256), measured
(DESIGN.md 4.2bf).

    full     gated_gcn_block(want=None) at 4096 x 32 x 768, 512 x 32 x 768, 256 x 31 x 256
    eval     gated_gcn_block(want=("out",)) at the same three shapes
    folded   gated_gcn_block(want=("out",)) at 512 x 100 x 768, 512 x 231 x 768, 128 x 231 x 768

The option off and on ALTERNATE in one process on the same tensors: >= 100 untimed calls of each side, then 7 rounds of
(10 untimed + a window of 50 calls) per side, off and on in turn; the median window is reported with the spread (max - min, in us)
between a side's windows.  A difference counts when the medians differ by more than the larger spread of the two sides.  For scale
the float32 blocks (f16mx8 and bf16x3) run on x.float() afterwards, each on its own.  Per <= 32-node shape the tool also prints
whether the bf16 block is torch.equal to the float32 bf16x3 block on x.float() (recorded, not asserted).
Development tool; one line per case and a JSON summary."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

WARM, WINDOWS, PER, REWARM = 100, 7, 50, 10
dev = torch.device("cuda:0")


def window(fn, per=PER):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(per):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / per   # us per call


def alternating(fns):
    """{name: (median us, spread us)} of callables timed in turn, window by window."""
    for fn in fns.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for _ in range(WINDOWS):
        for k, fn in fns.items():
            for _ in range(REWARM):
                fn()
            torch.cuda.synchronize()
            res[k].append(window(fn))
    return {k: (statistics.median(v), max(v) - min(v)) for k, v in res.items()}


def layer(pkg, synth, H, seed, precision):
    w, b = synth.layer_params(H, H, seed=seed)
    m = pkg.GraphConvolution(H, H).to(dev)
    m.precision = precision
    with torch.no_grad():
        m.weight.copy_(torch.from_numpy(w))
        m.bias.copy_(torch.from_numpy(b))
    return m


def batch(pkg, synth, B, T, H, seed):
    adj = synth.dependency_batch(B, T, 4.0, lengths=np.random.default_rng(seed).integers(max(5, T // 2), T + 1, size=B))
    rp, ci, _ = synth.csr_from_dense_host(adj)
    csr = pkg.BatchedCSR.from_arrays(rp, ci, B, T, dev)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, H, generator=g).to(torch.bfloat16).to(dev)
    gates = [torch.sigmoid(torch.randn(B, H, generator=g)).to(dev) for _ in range(2)]
    return csr, x, gates


def verdict(on, off):
    (u1, s1), (u0, s0) = on, off
    if u0 - u1 > max(s0, s1):
        return "WINS"
    return "loses" if u1 - u0 > max(s0, s1) else "ties"


def case(pkg, synth, form, B, T, H):
    csr, x, (g1, g2) = batch(pkg, synth, B, T, H, seed=1)
    xf = x.float()
    want = None if form == "full" else ("out",)
    bf = [layer(pkg, synth, H, s, "bf16x3") for s in (1, 2)]
    scale = {p: [layer(pkg, synth, H, s, p) for s in (1, 2)] for p in ("f16mx8", "bf16x3")}

    def run(layers, xin, on):
        def fn():
            layers[0].bf16_block = layers[1].bf16_block = on
            with torch.no_grad():
                return pkg.gated_gcn_block(xin, csr, g1, g2, layers[0], layers[1], want=want)
        return fn
    res = alternating({"off": run(bf, x, False), "on": run(bf, x, True)})
    for p in scale:
        res["float32 " + p] = alternating({p: run(scale[p], xf, False)})[p]
    key = "%s %dx%dx%d" % (form, B, T, H)
    line = "%-24s" % key
    out = {}
    for name, (us, sp) in res.items():
        line += "  %s %7.1f us (+-%.1f)" % (name, us, sp)
        out["%s %s" % (key, name)] = [round(us, 1), round(sp, 1)]
    v = verdict(res["on"], res["off"])
    line += "  option on %s" % v
    out[key + " verdict"] = v
    if T <= 32:
        a, b = run(bf, x, True)(), run(scale["bf16x3"], xf, False)()
        same = all(torch.equal(a[k], b[k]) for k in a if a[k] is not None)
        line += "  equal to float32 bf16x3 on x.float(): %s" % same
        out[key + " equal float32 bf16x3"] = same
    print(line, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--cases", default=None, help="form,B,T,H;...  (form: full, eval or folded)")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import ed_gated_gcn_amd as pkg
    from ed_gated_gcn_amd import synth
    print("package from %s" % os.path.dirname(pkg.__file__), flush=True)
    small = [(4096, 32, 768), (512, 32, 768), (256, 31, 256)]
    cases = ([(c.split(",")[0],) + tuple(int(v) for v in c.split(",")[1:]) for c in a.cases.split(";")] if a.cases else
             [("full",) + s for s in small] + [("eval",) + s for s in small]
             + [("folded",) + s for s in ((512, 100, 768), (512, 231, 768), (128, 231, 768))])
    out = {}
    for form, B, T, H in cases:
        out.update(case(pkg, synth, form, B, T, H))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
