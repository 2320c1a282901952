#!/usr/bin/env python3
"""Forward + backward of the two gate MLPs ALONE (models/bert_amir5.py:562-571): the two nn.Sequential as PyTorch ops (what the
classifier's training branches run without opt.ggcn_gate_backward) against heads.gate_mlps (ggcn_transpose of the four updated
weights + ggcn_gate_mlp_save forward; ggcn_gate_mlp_backward + three ggcn_dweight + one ggcn_colsum backward), in one process.
Each form runs ALONE in steady state: a warm-up, then windows of REPS steps between events that were created before the first
step; the forms take turns window group by window group, so a drift of the clocks shows in both.  A step is an in-place touch
of the four weights (an optimizer's update: gate_mlps transposes a weight again when its version changed), forward,
loss = (g1 * r1).sum() + (g2 * r2).sum(), backward into aspect and the eight parameters.  Beside the time: the device kernels
of one step of each form (torch.profiler; the library calls of the HIP form are counted at the binding), and the largest
difference of the two forms' gradients relative to each gradient's scale.  Last line: one classifier training step without an
encoder (``classifier_step``) with ``ggcn_gate_backward`` off and on -- the gate MLPs' share of what this package runs of a step.

usage: gate_backward_timing.py [output file]   (writes profiles/gate_backward_timing.txt by default)"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ed_gated_gcn_amd as pkg  # noqa: E402

SHAPES = ((4096, 768), (256, 256))   # the benchmark's batch and width; the reference model's (batch 256, 2 x 128)
WARM, GROUPS, SKIP, WINDOWS, REPS = 20, 6, 1, 5, 20
ENTRIES = ("ggcn_transpose", "ggcn_gate_mlp_save", "ggcn_gate_mlp_backward", "ggcn_dweight", "ggcn_colsum")


def literal(aspect, gate1, gate2):
    return gate1(aspect), gate2(aspect)


def device_kernels(step):
    """Device kernels of one ``step()`` as torch.profiler sees them (None where it cannot tell)."""
    try:
        from torch.autograd import DeviceType
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA)
        return n or None
    except Exception as exc:   # the count is a side figure: the timings stand without it
        print("torch.profiler: %s" % exc, flush=True)
        return None


class _NoEncoder(torch.nn.Module):
    """Stands where BERT stands and returns twelve fixed random layers: the classifier step below has no encoder in it."""

    def forward(self, ids_, seg, output_all_encoded_layers=True):
        if not hasattr(self, "layers"):
            gen = torch.Generator(device=ids_.device).manual_seed(1)
            self.layers = [torch.randn(ids_.shape[0], ids_.shape[1], 768, device=ids_.device, generator=gen) for _ in range(12)]
            self.pooled = torch.zeros(ids_.shape[0], 768, device=ids_.device)
        return self.layers, self.pooled


def classifier_step(dev, B=256, words=31, pieces=65, classes=34):
    """One training step of ``GatedGCNEventDetector`` WITHOUT an encoder (sub-word pooling, BiLSTM, gate MLPs, gated block, dense,
    head, loss, backward, SGD update; dropout 0) with ``ggcn_gate_backward`` off and on: the two models take turns in windows of 10
    steps; returns the report line."""
    import types

    import numpy as np

    from oracle.gpu_support import ace_batch
    inputs = {k: v.to(dev) for k, v in ace_batch(np.random.default_rng(3), B, words, pieces, vocab=30522).items()}
    models = {}
    for on in (False, True):
        opt = types.SimpleNamespace(dropout=0.0, polarities_dim=classes, device=dev, ggcn_gate_backward=on)
        torch.manual_seed(0)
        m = pkg.GatedGCNEventDetector(_NoEncoder(), opt).to(dev).train()
        models[on] = (m, torch.optim.SGD(m.parameters(), lr=1e-3))
    target = torch.arange(B, device=dev) % classes

    def step(on):
        m, o = models[on]
        o.zero_grad(set_to_none=True)
        logits, xy, kl, _ = m(inputs)
        (torch.nn.functional.cross_entropy(logits, target) + xy + kl).backward()
        o.step()

    for on in (False, True):
        for _ in range(10):
            step(on)
    torch.cuda.synchronize()
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(WINDOWS)]
    res = {False: [], True: []}
    for group in range(GROUPS):
        for on in (False, True):
            for e0, e1 in events:
                e0.record()
                for _ in range(10):
                    step(on)
                e1.record()
            torch.cuda.synchronize()
            if group >= SKIP:
                res[on] += [e0.elapsed_time(e1) / 10 * 1e3 for e0, e1 in events]
    return ("classifier training step without an encoder, %d sentences of up to %d words, H=256: gate MLPs as PyTorch ops %.0f (%.0f..%.0f) us, "
            "with ggcn_gate_backward %.0f (%.0f..%.0f) us" % (B, words, statistics.median(res[False]), min(res[False]), max(res[False]),
                                                              statistics.median(res[True]), min(res[True]), max(res[True])))


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "gate_backward_timing.txt")
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    lib = pkg.load_library()
    events = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(WINDOWS)] for _ in range(2)]
    lines = ["# %s; forward + backward of the two gate MLPs alone, us per step: median (min..max) over %d windows of %d steps, each form "
             "alone in its windows, the forms taking turns" % (torch.cuda.get_device_name(0), (GROUPS - SKIP) * WINDOWS, REPS)]
    nn = torch.nn
    for B, H in SHAPES:
        g = torch.Generator().manual_seed(B + H)
        aspect, r1, r2 = (torch.randn(B, H, generator=g).to(dev) for _ in range(3))
        aspect.requires_grad_()
        gate1, gate2 = (nn.Sequential(nn.Sigmoid(), nn.Linear(H, H), nn.Sigmoid(), nn.Linear(H, H), nn.Sigmoid()).to(dev) for _ in range(2))
        weights = [m.weight for s in (gate1, gate2) for m in (s[1], s[3])]
        leaves = [aspect] + list(gate1.parameters()) + list(gate2.parameters())

        def step(form):
            with torch.no_grad():
                torch._foreach_mul_(weights, 1.0)           # one launch; bumps the four version counters like an optimizer step
            g1, g2 = form(aspect, gate1, gate2)
            return torch.autograd.grad((g1 * r1).sum() + (g2 * r2).sum(), leaves)

        forms = (("PyTorch ops", literal), ("gate_mlps", pkg.gate_mlps))
        res, grads, kernels = {n: [] for n, _ in forms}, {}, {}
        for name, form in forms:
            for _ in range(WARM):
                step(form)
            torch.cuda.synchronize()
            grads[name] = step(form)
        for group in range(GROUPS):
            for k, (name, form) in enumerate(forms):
                for e0, e1 in events[k]:
                    e0.record()
                    for _ in range(REPS):
                        step(form)
                    e1.record()
                torch.cuda.synchronize()
                if group >= SKIP:
                    res[name] += [e0.elapsed_time(e1) / REPS * 1e3 for e0, e1 in events[k]]
        # library calls of one HIP step, counted at the binding
        counts, originals = {n: 0 for n in ENTRIES}, {n: getattr(lib, n) for n in ENTRIES}
        for n in ENTRIES:
            def wrap(*a, _fn=originals[n], _n=n):
                counts[_n] += 1
                return _fn(*a)
            setattr(lib, n, wrap)
        step(pkg.gate_mlps)
        for n in ENTRIES:
            setattr(lib, n, originals[n])
        for name, form in forms:
            kernels[name] = device_kernels(lambda: step(form))
        diff = max(float((a - b).abs().max()) / (float(b.abs().max()) + 1e-30) for a, b in zip(grads["gate_mlps"], grads["PyTorch ops"]))
        line = "B=%d H=%d: " % (B, H)
        line += "   ".join("%s %.1f (%.1f..%.1f) us, %s device kernels" % (n, statistics.median(v), min(v), max(v), kernels[n]) for n, v in res.items())
        line += "   | ratio %.2f   | library calls of a gate_mlps step: %s   | gradients, HIP against ops: max|diff| %.3g of a gradient's scale" % (
            statistics.median(res["PyTorch ops"]) / statistics.median(res["gate_mlps"]),
            ", ".join("%d %s" % (c, n) for n, c in counts.items()), diff)
        print(line, flush=True)
        lines.append(line)
    lines.append(classifier_step(dev))
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
