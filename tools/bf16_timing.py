#!/usr/bin/env python3
"""bfloat16 features, measured: the one-launch layer on bf16 X (ggcn_layer_fused_bf16, two bf16 MFMAs per product) against the
float32 one-launch layer in bf16x3 (three) and f16mx8, with a store gate and both pools, at 4096 x 32 x 768 and 4096 x 31 x 256;
then one training step (forward + backward) of the gated block with bf16 against float32 features.  One process, steady state:
>= 100 untimed launches per case, then several timed windows (events around N launches each) whose medians must agree.
Development tool; prints one line per case and a JSON summary."""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ed_gated_gcn_amd as pkg  # noqa: E402
from ed_gated_gcn_amd import synth  # noqa: E402

dev = torch.device("cuda:0")
WARM, WINDOWS, PER = 100, 7, 50


def timed(fn, per=PER):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    res = []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(per):
            fn()
        b.record()
        torch.cuda.synchronize()
        res.append(a.elapsed_time(b) * 1000.0 / per)   # us per call
    return statistics.median(res), (max(res) - min(res)) / statistics.median(res)


def layer(K, F, seed, precision):
    w, b = synth.layer_params(K, F, seed=seed)
    m = pkg.GraphConvolution(K, F).to(dev)
    m.precision = precision
    with torch.no_grad():
        m.weight.copy_(torch.from_numpy(w))
        m.bias.copy_(torch.from_numpy(b))
    return m


def main():
    out = {}
    for B, T, H in ((4096, 32, 768), (4096, 31, 256)):
        adj = synth.dependency_batch(B, T, 4.0, lengths=None if T == 32 else np.random.default_rng(1).integers(5, T + 1, size=B))
        rp, ci, _ = synth.csr_from_dense_host(adj)
        csr = pkg.BatchedCSR.from_arrays(rp, ci, B, T, dev)
        g = torch.Generator().manual_seed(1)
        x32 = torch.randn(B, T, H, generator=g).to(dev)
        xb = x32.to(torch.bfloat16)
        sg, ga, gb = (torch.sigmoid(torch.randn(B, H, generator=g)).to(dev) for _ in range(3))
        for name, x, prec in (("bf16 features", xb, "bf16x3"), ("fp32 bf16x3", x32, "bf16x3"), ("fp32 f16mx8", x32, "f16mx8")):
            m = layer(H, H, 1, prec)
            assert (m.takes_bf16_fused_path(x, csr) if x.dtype == torch.bfloat16 else m.takes_fused_path(x, csr))

            def run(m=m, x=x):
                with torch.no_grad():
                    m.forward_gated(x, csr, store_gate=sg, pool_gate_a=ga, pool_gate_b=gb, want_pool_a=True, want_pool_b=True)
            us, spread = timed(run)
            key = "layer %dx%dx%d %s" % (B, T, H, name)
            out[key] = round(us, 1)
            print("%-44s %8.1f us   (window spread %.1f %%)" % (key, us, 100 * spread), flush=True)
    # one training step of the block (forward + backward), 512 graphs x 31 x 256 (the classifier's block)
    B, T, H = 512, 31, 256
    adj = synth.dependency_batch(B, T, 3.5, lengths=np.random.default_rng(2).integers(5, T + 1, size=B))
    rp, ci, _ = synth.csr_from_dense_host(adj)
    csr = pkg.BatchedCSR.from_arrays(rp, ci, B, T, dev)
    g = torch.Generator().manual_seed(2)
    x32 = torch.randn(B, T, H, generator=g).to(dev)
    g1, g2 = (torch.sigmoid(torch.randn(B, H, generator=g)).to(dev).requires_grad_() for _ in range(2))
    for name, x in (("bf16 features", x32.to(torch.bfloat16)), ("fp32 bf16x3", x32)):
        gc1, gc2 = layer(H, H, 1, "bf16x3"), layer(H, H, 2, "bf16x3")
        xr = x.clone().requires_grad_()

        def step(gc1=gc1, gc2=gc2, xr=xr):
            r = pkg.gated_gcn_block(xr, csr, g1, g2, gc1, gc2)
            (r["out"].sum() + r["xy"]).backward()
        us, spread = timed(step, per=20)
        key = "block train step %dx%dx%d %s" % (B, T, H, name)
        out[key] = round(us, 1)
        print("%-44s %8.1f us   (window spread %.1f %%)" % (key, us, 100 * spread), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
