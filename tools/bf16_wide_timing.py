#!/usr/bin/env python3
"""bfloat16 features on graphs of 33..256 nodes, measured.

    layers   the one-launch layer (ggcn_layer_fused_bf16_wide, forced with fused_max_t = 256) against the two launches
             (ggcn_linear_bf16 + ggcn_aggregate, fused = False) at H = 768 for B x T in {512, 128} x {33 .. 256} and 4096 x 100,
             store gate and both pools; a verdict per shape: the one launch is the default only where its median beats the two
             launches by more than the spread between the windows of either.
    train    one classifier-shaped training step of the gated block under dropout 0.25 (gates -> gc1 -> gc2 -> pools ->
             backward; what classifier.py runs for bf16 features): the in-launch dropout of both layers where the tree has
             it (takes_bf16_dropout_path), else the eager branch (gates expanded to [B,T,H], torch dropout, torch.max pools).

--root DIR imports the package from another checkout (a build of the parent commit), so that both trees run the SAME script.
One process, steady state: >= 100 untimed launches per case, then 7 windows of 50 (training steps: 20) whose median is
reported with the spread (max - min, in us) between the windows.  Development tool; one line per case and a JSON summary."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

WARM, WINDOWS, PER = 100, 7, 50
dev = torch.device("cuda:0")


def timed(fn, per=PER, warm=WARM):
    for _ in range(warm):
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
    return statistics.median(res), max(res) - min(res)


def layer(pkg, synth, K, F, seed):
    w, b = synth.layer_params(K, F, seed=seed)
    m = pkg.GraphConvolution(K, F).to(dev)
    m.precision = "bf16x3"
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
    gates = [torch.sigmoid(torch.randn(B, H, generator=g)).to(dev) for _ in range(3)]
    return csr, x, gates


def layers(pkg, synth, shapes):
    out = {}
    H = 768
    for B, T in shapes:
        csr, x, (sg, ga, gb) = batch(pkg, synth, B, T, H, seed=1)
        m = layer(pkg, synth, H, H, 1)
        res = {}
        for name, fused in (("one launch", True), ("linear+aggregate", False)):
            m.fused, m.fused_max_t = fused, 256
            if fused and not hasattr(m, "takes_bf16_wide_path"):
                continue   # a tree without the one-launch form times the two launches only
            assert not fused or m.takes_bf16_wide_path(x, csr)

            def run():
                with torch.no_grad():
                    m.forward_gated(x, csr, store_gate=sg, pool_gate_a=ga, pool_gate_b=gb, want_pool_a=True, want_pool_b=True)
            res[name] = timed(run)
        m.fused, m.fused_max_t = True, 128   # what the default rule says for this shape
        default = bool(getattr(m, "takes_bf16_wide_path", lambda *a: False)(x, csr))
        key = "%dx%dx%d" % (B, T, H)
        line = "layer %-14s" % key
        for name, (us, sp) in res.items():
            line += "  %s %7.1f us (windows +-%.1f)" % (name, us, sp)
            out["%s %s" % (key, name)] = [round(us, 1), round(sp, 1)]
        if len(res) == 2:
            (u1, s1), (u2, s2) = res["one launch"], res["linear+aggregate"]
            wins = u2 - u1 > max(s1, s2)
            line += "  one launch %s  default rule: %s" % ("WINS" if wins else ("loses" if u1 - u2 > max(s1, s2) else "ties"),
                                                          "one launch" if default else "two launches")
            out["%s verdict" % key] = ["win" if wins else "no", "one launch" if default else "two launches"]
        print(line, flush=True)
    return out


def train(pkg, synth, shapes, p=0.25):
    out = {}
    for B, T, H in shapes:
        csr, x, (g1, g2, _) = batch(pkg, synth, B, T, H, seed=2)
        g1, g2 = g1.requires_grad_(), g2.requires_grad_()
        gc1, gc2 = layer(pkg, synth, H, H, 1).train(), layer(pkg, synth, H, H, 2).train()
        xr = x.clone().requires_grad_()
        drop = torch.nn.Dropout(p)
        gcn1_like = torch.zeros(1, dtype=torch.float32, device=dev).expand(B, T, H)
        in_launch = (hasattr(gc1, "takes_bf16_dropout_path") and gc1.takes_bf16_dropout_path(xr, csr)
                     and gc2.takes_dropout_path(gcn1_like, csr))
        torch.manual_seed(3)

        def step():   # classifier.py, training with dropout: the block only
            if in_launch:
                seed = int(torch.randint(0, 2 ** 62, (1,)).item())
                gcn1, x1, y1 = gc1.forward_gated(xr, csr, pool_gate_a=g1, pool_gate_b=g2, want_pool_a=True, want_pool_b=True,
                                                 dropout=(p, seed, (0, 1, 2)))
                xy = (x1 * y1).sum(1).mean()
                xg, o, _ = gc2.forward_gated(gcn1, csr, store_gate=g2, pool_gate_a=g2, want_pool_a=True, dropout=(p, seed, (2, 2, 0)))
            else:
                gate1 = drop(g1[:, None, :].expand(-1, T, -1))
                gate2 = drop(g2[:, None, :].expand(-1, T, -1))
                gcn1 = gc1(xr, csr)
                x1 = torch.max(gcn1 * gate1, 1)[0]
                y1 = torch.max(gcn1 * gate2, 1)[0]
                xy = (x1 * y1).sum(1).mean()
                xg = gate2 * gc2(gcn1, csr)
                o = torch.max(xg, dim=1)[0]
            (o.sum() + 0.01 * xg.sum() + xy).backward()
        us, sp = timed(step, per=20, warm=40)
        key = "train step dropout %.2f %dx%dx%d" % (p, B, T, H)
        out[key] = [round(us, 1), round(sp, 1), "in-launch dropout" if in_launch else "eager gates"]
        print("%-44s %9.1f us (windows +-%.1f)  %s" % (key, us, sp, out[key][2]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["layers", "train"])
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--shapes", default=None, help="layers: B,T;B,T...   train: B,T,H;...")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import ed_gated_gcn_amd as pkg
    from ed_gated_gcn_amd import synth
    print("package from %s" % os.path.dirname(pkg.__file__), flush=True)
    if a.mode == "layers":
        shapes = ([tuple(int(v) for v in s.split(",")) for s in a.shapes.split(";")] if a.shapes else
                  [(B, T) for B in (512, 128) for T in (33, 64, 100, 128, 129, 160, 192, 193, 231, 256)] + [(4096, 100)])
        out = layers(pkg, synth, shapes)
    else:
        shapes = ([tuple(int(v) for v in s.split(",")) for s in a.shapes.split(";")] if a.shapes else
                  [(512, 31, 256), (512, 100, 256), (256, 231, 768)])
        out = train(pkg, synth, shapes)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
