#!/usr/bin/env python3
"""What the Python layer of the package hands to libggcn_hip.so, and what comes back, at the smallest shapes that reach every
host path of the four autograd Functions and of the operand caches: per case one line per library call (the entry, its scalar
arguments, every pointer only as ``NULL`` or ``ptr``), then the sha256 of every output and gradient.  Two trees of the package
that do the same on ONE library print the same listing, line for line:

    GGCN_LIB=$PWD/ed-gated-gcn_amd/libggcn_hip.so python tools/host_digest.py --tree /path/to/other/checkout > other.txt
    GGCN_LIB=$PWD/ed-gated-gcn_amd/libggcn_hip.so python tools/host_digest.py > this.txt && cmp other.txt this.txt

Cases (seeds fixed, B <= 3): the gated layer forward + backward with three gates and both pools at K = F = 64 (T = 5 at bf16x3,
f16mx8, fp32; T = 40, the two-pass backward; bfloat16 features; a real-valued dense adjacency that wants its gradient; no bias),
three steps of the first of them (nothing changed: no ggcn_weight_pack; after an in-place weight update: one per image in use),
the inference block at f16mx8 then bf16x3 (twice, and after an in-place edit of gc1.weight), the gate MLPs (H = 8: the fused dW1
product; H = 6: the separate ones; one Sequential for both gates), the scores / kl head with and without fc.bias, and the BiLSTM
(inference, training with and without a gradient for x, and with weight_ih_l0 alone wanting one)."""
import argparse
import ctypes
import hashlib
import os
import sys

import torch

B, K, F = 3, 64, 64


def sha(t):
    return "None" if t is None else hashlib.sha256(t.detach().float().cpu().contiguous().numpy().tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose package to import")
    sys.path.insert(0, os.path.abspath(ap.parse_args().tree))
    import ed_gated_gcn_amd as pkg
    from ed_gated_gcn_amd import _capi

    dev = torch.device("cuda:0")
    lib = pkg.load_library()
    log = []
    for name in _capi.PROTOTYPES:      # a recorder on every entry of the loaded library (the package looks them up per call)
        def wrap(*a, _fn=getattr(lib, name), _n=name):
            log.append(" ".join([_n] + [("ptr" if v.value else "NULL") if isinstance(v, ctypes.c_void_p) else "NULL" if v is None else repr(v)
                                        for v in a]))
            return _fn(*a)
        setattr(lib, name, wrap)

    def report(case, **tensors):
        """Print and forget the calls since the last report, then the digests; returns the number of ggcn_weight_pack among them."""
        torch.cuda.synchronize()
        print("case %s" % case)
        for line in log:
            print("  call %s" % line)
        for name, t in tensors.items():
            print("  sha256 %s %s" % (name, sha(t)))
        sys.stdout.flush()
        packs = sum(line.startswith("ggcn_weight_pack ") for line in log)
        del log[:]
        return packs

    def rand(gen, *shape, scale=1.0):
        return (scale * torch.randn(shape, generator=gen)).to(dev)

    def grads(*ts):
        return {"d_%d" % i: (None if t is None else t.grad) for i, t in enumerate(ts)}

    # ---- the gated layer under autograd
    def layer_step(case, m, x, adj, gates, gen):
        for t in (x, adj, m.weight, m.bias) + tuple(gates):
            if t is not None and torch.is_tensor(t):
                t.grad = None
        out, pa, pb = m.forward_gated(x, adj, store_gate=gates[0], pool_gate_a=gates[1], pool_gate_b=gates[2], want_out=True,
                                      want_pool_a=True, want_pool_b=True)
        torch.autograd.backward([out, pa, pb], [rand(gen, *out.shape), rand(gen, *pa.shape), rand(gen, *pb.shape)])
        return report(case, out=out, pa=pa, pb=pb, **grads(x, m.weight, m.bias, *gates, adj if torch.is_tensor(adj) else None))

    def layer_case(case, T, precision, dtype=torch.float32, dense_adj=False, bias=True, steps=1):
        gen = torch.Generator().manual_seed(1000 + T)
        m = pkg.GraphConvolution(K, F, opt=None, bias=bias).to(dev)
        m.precision = precision
        with torch.no_grad():
            m.weight.copy_(rand(gen, K, F, scale=0.05))
            if bias:
                m.bias.copy_(rand(gen, F, scale=0.1))
        x = rand(gen, B, T, K).to(dtype).requires_grad_()
        gates = [torch.rand(B, F, generator=gen).to(dev).requires_grad_() for _ in range(3)]
        a = (torch.rand(B, T, T, generator=gen) < 3.0 / T).float()
        a = ((a + a.transpose(1, 2) + torch.eye(T)) > 0).float()
        if dense_adj:
            adj = (a * (0.25 + 0.5 * torch.rand(B, T, T, generator=gen))).to(dev).requires_grad_()
        else:
            adj = pkg.BatchedCSR.from_dense(a.to(dev), binary=True)
        packs = []
        for s in range(steps):       # step 2: nothing changed; step 3: after an in-place weight update
            if s == 2:
                with torch.no_grad():
                    m.weight.mul_(0.5)
            name = case if steps == 1 else "%s step %d%s" % (case, s + 1, " (weight updated in place)" if s == 2 else "")
            packs.append(layer_step(name, m, x, adj, gates, gen))
        return packs

    for precision in ("bf16x3", "f16mx8", "fp32"):
        layer_case("layer T=5 %s" % precision, 5, precision)
    layer_case("layer T=40 bf16x3 (two-pass backward)", 40, "bf16x3")
    layer_case("layer T=5 bf16x3 bfloat16 features", 5, "bf16x3", dtype=torch.bfloat16)
    layer_case("layer T=5 bf16x3 real-valued dense adj with requires_grad", 5, "bf16x3", dense_adj=True)
    layer_case("layer T=5 bf16x3 no bias", 5, "bf16x3", bias=False)
    packs = layer_case("layer T=5 bf16x3", 5, "bf16x3", steps=3)
    assert packs == [2, 0, 2], packs      # the forward's image and the backward's W^T image; none; both again
    layer_case("layer T=5 fp32", 5, "fp32", steps=3)      # (exact fp32 reads W itself, and a cached W^T as a plain matrix)

    # ---- the inference block: two precisions side by side under gc2._block_ops, one refold after an edit of gc1.weight
    gen = torch.Generator().manual_seed(2000)
    gc1, gc2 = (pkg.GraphConvolution(K, F, opt=None).to(dev) for _ in range(2))
    with torch.no_grad():
        for m in (gc1, gc2):
            m.weight.copy_(rand(gen, K, F, scale=0.05))
            m.bias.copy_(rand(gen, F, scale=0.1))
    x = rand(gen, B, 5, K)
    g1, g2 = (torch.rand(B, F, generator=gen).to(dev) for _ in range(2))
    a = (torch.rand(B, 5, 5, generator=gen) < 0.6).float()
    csr = pkg.BatchedCSR.from_dense(((a + a.transpose(1, 2) + torch.eye(5)) > 0).float().to(dev), binary=True)
    packs = []
    for edit in (False, False, True):
        if edit:
            with torch.no_grad():
                gc1.weight.mul_(0.5)
        for precision in ("f16mx8", "bf16x3"):
            gc1.precision = gc2.precision = precision
            with torch.no_grad():
                r = pkg.gated_gcn_block(x, csr, g1, g2, gc1, gc2)
            packs.append(report("block T=5 %s%s" % (precision, " (gc1.weight edited in place)" if edit else ""), **r))
    assert packs == [2, 2, 0, 0, 2, 2] and len(gc2._block_ops) == 2, (packs, gc2._block_ops.keys())   # W1 and W12 per precision

    # ---- the gate MLPs under autograd
    def gate_seq(H):
        return torch.nn.Sequential(torch.nn.Sigmoid(), torch.nn.Linear(H, H), torch.nn.Sigmoid(), torch.nn.Linear(H, H), torch.nn.Sigmoid()).to(dev)

    for case, H, shared in (("H=8", 8, False), ("H=6", 6, False), ("H=8 one Sequential for both gates", 8, True)):
        torch.manual_seed(3000 + H)
        gen = torch.Generator().manual_seed(3000 + H)
        s1 = gate_seq(H)
        s2 = s1 if shared else gate_seq(H)
        aspect = rand(gen, 3, H).requires_grad_()
        o1, o2 = pkg.gate_mlps(aspect, s1, s2)
        torch.autograd.backward([o1, o2], [rand(gen, 3, H), rand(gen, 3, H)])
        report("gate_mlps B=3 %s" % case, g1=o1, g2=o2, **grads(aspect, *s1.parameters(), *s2.parameters()))

    # ---- the scores / kl head under autograd
    for bias in (True, False):
        torch.manual_seed(4000)
        gen = torch.Generator().manual_seed(4000)
        T, H, C = 5, 8, 3
        fc = torch.nn.Linear(2 * H, C, bias=bias).to(dev)
        xs, aspect, logits = rand(gen, 3, T, H).requires_grad_(), rand(gen, 3, H).requires_grad_(), rand(gen, 3, C).requires_grad_()
        dist = torch.randint(0, 6, (3, T), generator=gen).to(dev)
        scores, kl = pkg.scores_and_kl(xs, aspect, logits, fc, dist)
        torch.autograd.backward([scores, kl], [rand(gen, 3, T), rand(gen)])
        report("scores_and_kl B=3 T=5 H=8 C=3%s" % ("" if bias else " no fc.bias"), scores=scores, kl=kl,
               **grads(xs, aspect, logits, *fc.parameters()))

    # ---- the BiLSTM: one module throughout, so that the later calls find its operands cached
    torch.manual_seed(5000)
    gen = torch.Generator().manual_seed(5000)
    lstm = torch.nn.LSTM(64, 128, bidirectional=True, batch_first=True, num_layers=1).to(dev)
    x = rand(gen, 2, 3, 64)
    with torch.no_grad():
        report("bilstm B=2 T=3 I=64", y=pkg.bilstm(x, lstm))
    dy = rand(gen, 2, 3, 256)
    for case, x_grad, only in (("x and parameters", True, None), ("parameters", False, None), ("weight_ih_l0 alone", False, "weight_ih_l0")):
        for name, p in lstm.named_parameters():
            p.grad = None
            p.requires_grad_(only is None or name == only)
        xi = x.clone().requires_grad_(x_grad)
        y = pkg.bilstm_train(xi, lstm)
        y.backward(dy)
        report("bilstm_train B=2 T=3 I=64, gradient for %s" % case, y=y, **grads(xi, *lstm.parameters()))


if __name__ == "__main__":
    main()
