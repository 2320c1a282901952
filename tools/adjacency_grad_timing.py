#!/usr/bin/env python3
"""The adjacency gradient (ggcn_adjacency_grad, DESIGN.md "Gradient with respect to the adjacency") beside the same quantity
through torch.bmm plus elementwise ops on the same tensors -- a yardstick that is not this project's code:

    G = bmm(dY, H^T) * inv[:, :, None];   c = (A * G).sum(2) * inv;   dA = G - c[:, :, None]

at 4096 x 32 x 768, 512 x 100 x 768 and 512 x 231 x 768 (B x T x F), weighted dependency graphs.  Both sides ALTERNATE in one process:
>= 100 untimed calls of each, then 7 rounds of (10 untimed + a window of 50 calls) per side in turn; the median window is reported
with the spread (max - min, in us) between a side's windows, and the achieved bytes/s against the kernel's compulsory traffic
2*N*F*4 (dY and H read once) + B*T*T*4 (d_adj written once).  Per shape the tool also prints the largest difference between the
two results relative to max|dA| (recorded, not asserted).  Development tool; one line per case and a JSON summary.
--out FILE also writes the lines there."""
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


def case(pkg, synth, _capi, B, T, F):
    lib = pkg.load_library()
    rng = np.random.default_rng(1)
    adj = synth.dependency_batch(B, T, 4.0, lengths=rng.integers(max(5, T // 2), T + 1, size=B)).astype(np.float32)
    adj = torch.from_numpy(adj * rng.uniform(0.25, 2.0, size=adj.shape).astype(np.float32)).to(dev)
    csr = pkg.BatchedCSR.from_dense(adj)
    inv, rowptr, colidx, vals = csr.inv_denominators(), csr.rowptr, csr.colidx, csr.vals
    g = torch.Generator(device=dev).manual_seed(2)
    dy = torch.randn(B * T, F, device=dev, generator=g)
    hidden = torch.randn(B * T, F, device=dev, generator=g)
    d_adj = torch.empty(B, T, T, device=dev)
    st = _capi.stream_of(dev)
    args = (_capi.ptr(dy), F, _capi.ptr(hidden), F, _capi.ptr(inv), _capi.ptr(rowptr), _capi.ptr(colidx), _capi.ptr(vals), B, T, F,
            _capi.ptr(d_adj), st)

    def kernel():
        _capi.check(lib.ggcn_adjacency_grad(*args), "ggcn_adjacency_grad")
        return d_adj
    dy3, ht, inv2 = dy.view(B, T, F), hidden.view(B, T, F).transpose(1, 2), inv.view(B, T)

    def baseline():
        gm = torch.bmm(dy3, ht) * inv2[:, :, None]
        return gm - ((adj * gm).sum(2) * inv2)[:, :, None]
    res = alternating({"kernel": kernel, "torch.bmm + elementwise": baseline})
    a, b = kernel().clone(), baseline()
    diff = float((a - b).abs().max() / b.abs().max())
    nbytes = 2.0 * B * T * F * 4 + 4.0 * B * T * T
    key = "%dx%dx%d" % (B, T, F)
    line, out = "%-14s" % key, {}
    for name, (us, sp) in res.items():
        line += "  %s %7.1f us (+-%.1f) %5.2f TB/s" % (name, us, sp, nbytes / us * 1e-6)
        out["%s %s" % (key, name)] = [round(us, 1), round(sp, 1), round(nbytes / us * 1e-6, 3)]
    line += "  max|kernel - baseline| / max|dA| %.2g" % diff
    out[key + " rel diff"] = diff
    print(line, flush=True)
    return line, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--cases", default="4096,32,768;512,100,768;512,231,768", help="B,T,F;...")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import ed_gated_gcn_amd as pkg
    from ed_gated_gcn_amd import _capi, synth
    print("package from %s" % os.path.dirname(pkg.__file__), flush=True)
    lines, out = [], {}
    for c in a.cases.split(";"):
        line, o = case(pkg, synth, _capi, *[int(v) for v in c.split(",")])
        lines.append(line)
        out.update(o)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines + [json.dumps(out)]) + "\n")


if __name__ == "__main__":
    main()
