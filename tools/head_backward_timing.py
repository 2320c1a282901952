#!/usr/bin/env python3
"""Forward + backward of the scores / kl head ALONE (models/bert_amir5.py:645-648): the literal PyTorch ops (cat, fc, multiply,
sum, two softmaxes, mean -- what the classifier's training branch runs without opt.ggcn_head_backward) against
heads.scores_and_kl (ggcn_scores_head + ggcn_overlap_reduce forward, ggcn_scores_head_backward + ggcn_scores_head_dweight
backward), in one process.  Each form runs ALONE in steady state: a warm-up, then windows of REPS steps between events that
were created before the first step; the forms take turns window group by window group, so a drift of the clocks shows in both.
A step is forward, loss = (scores * r).sum() + kl, backward into x, aspect, logits, fc.weight and fc.bias.  Beside the time:
the peak memory the form allocates on top of its inputs (torch.cuda.max_memory_allocated over one step), and the largest
difference of the two forms' gradients relative to each gradient's scale.

usage: head_backward_timing.py [output file]   (writes profiles/head_backward_timing.txt by default)"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ed_gated_gcn_amd as pkg  # noqa: E402

SHAPES = ((4096, 32, 768, 34), (256, 31, 256, 34))   # the benchmark's shape; the reference model's (batch 256, 31 words, 2 x 128)
WARM, GROUPS, SKIP, WINDOWS, REPS = 20, 6, 1, 5, 20


def literal(x, aspect, logits, fc, dist):
    T = x.shape[1]
    output_w = fc(torch.cat([x, aspect[:, None, :].expand(-1, T, -1)], dim=2))                    # :645
    scores = (logits[:, None, :] * output_w).sum(2)                                               # :646
    kl = (torch.softmax(scores, 1) * torch.softmax(dist.float(), 1)).sum(1).mean()                # :648
    return scores, kl


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "head_backward_timing.txt")
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    pkg.load_library()
    events = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(WINDOWS)] for _ in range(2)]
    lines = ["# %s; forward + backward of the head alone, us per step: median (min..max) over %d windows of %d steps, each form alone "
             "in its windows, the forms taking turns" % (torch.cuda.get_device_name(0), (GROUPS - SKIP) * WINDOWS, REPS)]
    for B, T, H, C in SHAPES:
        g = torch.Generator().manual_seed(B + T + H + C)
        x, aspect, logits, r = (torch.randn(*s, generator=g).to(dev).requires_grad_(i < 3)
                                for i, s in enumerate(((B, T, H), (B, H), (B, C), (B, T))))
        dist = torch.randint(0, 6, (B, T), generator=g).to(dev)
        fc = torch.nn.Linear(2 * H, C).to(dev)
        leaves = [x, aspect, logits, fc.weight, fc.bias]

        def step(form):
            scores, kl = form(x, aspect, logits, fc, dist)
            return torch.autograd.grad((scores * r).sum() + kl, leaves)

        forms = (("PyTorch ops", literal), ("scores_and_kl", pkg.scores_and_kl))
        res, peak, grads = {n: [] for n, _ in forms}, {}, {}
        for name, form in forms:
            for _ in range(WARM):
                step(form)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            grads[name] = step(form)
            torch.cuda.synchronize()
            peak[name] = (torch.cuda.max_memory_allocated(dev) - base) / 2.0 ** 20
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
        diff = max(float((a - b).abs().max()) / (float(b.abs().max()) + 1e-30) for a, b in zip(grads["scores_and_kl"], grads["PyTorch ops"]))
        line = "B=%d T=%d H=%d C=%d: " % (B, T, H, C)
        line += "   ".join("%s %.1f (%.1f..%.1f) us, peak +%.0f MiB" % (n, statistics.median(v), min(v), max(v), peak[n]) for n, v in res.items())
        line += "   | ratio %.2f   | gradients, HIP against ops: max|diff| %.3g of a gradient's scale" % (
            statistics.median(res["PyTorch ops"]) / statistics.median(res["scores_and_kl"]), diff)
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
