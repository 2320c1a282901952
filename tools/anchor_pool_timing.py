#!/usr/bin/env python3
"""The baselines' step from BERT's layer list to what their final linear reads (models/bert_ed.py:46-62 with ``sides=False``,
models/bertdm.py:164-198 with ``sides=True``), every form in one process:

  (a) dense       what the reference computes, as dense PyTorch: ``torch.cat``, ``torch.bmm``, then the formula as PyTorch ops
                  (``anchor_pool_formula``: 0/1 masks, multiply, add one, max over the words, subtract one, the anchor's row)
  (b) composed    ``anchor_pool_formula(subword_pool_layers(transform, layers), ...)``: this package's composed path
  (c) one launch  ``anchor_pool_layers(transform, layers, ...)``: ``ggcn_anchor_pool_layers``
  (d) one row     ``sides=False`` only: ``subword_pool_layers`` on the gathered one-row transform ``transform[rows, anchor][:, None]``

on reference-like transforms (``oracle.subword_pool_cases.transform_like_reference``), anchors uniform inside each sentence,
768 features a layer; n = 12 layers (both models) and n = 4 (``bertdm``'s default ``--n_layer``), float32 and bfloat16.  Each form
is warmed per shape, then runs ALONE in windows of REPS calls between two device events that end in a synchronise; the forms
take turns window group by window group, and REPS is chosen per form so that its timed windows add up to at least MIN_SECONDS.
Every form allocates its results in every call.  Beside the median time: the bytes the form must move by its shapes (every
elementwise op reads its operands and writes its result once; a pooling reads every selected row of a layer once per word it
belongs to; (c) reads only the rows it walks, ``0 .. max(anchor, length - 1)``), and the peak of
``torch.cuda.max_memory_allocated`` above the inputs.  (b), (c) and (d) are compared bit for bit first; the largest difference of (a), whose dense product sums in another order, is printed.

usage: anchor_pool_timing.py [output file]   (writes profiles/anchor_pool_timing.txt by default)"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ed_gated_gcn_amd as pkg  # noqa: E402
from oracle.subword_pool_cases import transform_like_reference  # noqa: E402

SHAPES = ((32, 31, 64), (256, 31, 64), (4096, 32, 65))
DL = 768
WARM, GROUPS, WINDOWS, MIN_SECONDS = 3, 3, 3, 0.5


def window(step, reps):
    """Seconds of ``reps`` calls of ``step`` between two device events, read after a synchronise."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def take_turns(forms):
    """{name: ([us per call of every window], seconds timed)}: every form warmed, then GROUPS x WINDOWS windows each, in turns."""
    reps = {}
    for name, step in forms.items():
        for _ in range(WARM):
            step()
        torch.cuda.synchronize()
        per_call = window(step, 20) / 20
        reps[name] = max(2, int(np.ceil(1.25 * MIN_SECONDS / (GROUPS * WINDOWS) / per_call)))
    res, total = {n: [] for n in forms}, {n: 0.0 for n in forms}
    group = 0
    while group < GROUPS or min(total.values()) < MIN_SECONDS:      # further groups until every form has its MIN_SECONDS
        for name, step in forms.items():
            for _ in range(WINDOWS):
                t = window(step, reps[name])
                total[name] += t
                res[name].append(t / reps[name] * 1e6)
        group += 1
    return {n: (res[n], total[n]) for n in forms}


def peak_above_inputs(step):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    y = step()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del y
    return peak


def dense_ops(a, layers, anchor, length, sides):
    """The dense PyTorch form: the concatenation, the dense product, then the formula as PyTorch ops."""
    v = torch.bmm(a.to(layers[0].dtype), torch.cat(layers, dim=-1))
    if not sides:
        return pkg.anchor_pool_formula(v, anchor, sides=False)
    row, pooled = pkg.anchor_pool_formula(v, anchor, length)
    return torch.cat((row.float(), pooled), 1)


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "anchor_pool_timing.txt")
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    pkg.load_library()
    lines = ["# %s; from BERT's layer list (n x %d features) to the baselines' [B, k*n*%d] vector, no_grad; us per call: median "
             "(min..max) over %d or more windows of at least %.1f s together, each form alone in its windows, the forms taking "
             "turns; GB: what the form must move, by its shapes; peak: allocation above the inputs"
             % (torch.cuda.get_device_name(0), DL, DL, GROUPS * WINDOWS, MIN_SECONDS)]
    for sides, n in ((False, 12), (True, 12), (True, 4)):
        for B, T, L in SHAPES:
            for dtype in (torch.float32, torch.bfloat16):
                rng = np.random.default_rng(B * 1000 + L)
                tr = transform_like_reference(B, T, L, rng)
                words = np.maximum(1, (tr != 0).any(axis=2).sum(axis=1))
                anchor_np = (rng.random(B) * words).astype(np.int64)
                a = torch.from_numpy(tr).to(dev)
                anchor, length = torch.from_numpy(anchor_np).to(dev), torch.from_numpy(words.astype(np.int64)).to(dev)
                gen = torch.Generator(device=dev).manual_seed(1)
                layers = [torch.randn(B, L, DL, device=dev, generator=gen).to(dtype) for _ in range(n)]
                rows = torch.arange(B, device=dev)
                s, D = layers[0].element_size(), n * DL
                nnz_row = (tr != 0).sum(axis=2)
                nnz = int(nnz_row.sum())
                last = np.maximum(anchor_np, words - 1) if sides else anchor_np
                first = np.zeros_like(last) if sides else anchor_np
                walked = int(sum(nnz_row[b, first[b]:last[b] + 1].sum() for b in range(B)))
                nnz_anchor = int(nnz_row[np.arange(B), anchor_np].sum())

                def ref():
                    with torch.no_grad():
                        return dense_ops(a, layers, anchor, length, sides)

                def composed():
                    with torch.no_grad():
                        v = pkg.subword_pool_layers(a, layers)
                        if not sides:
                            return pkg.anchor_pool_formula(v, anchor, sides=False)
                        row, pooled = pkg.anchor_pool_formula(v, anchor, length)
                        return torch.cat((row.float(), pooled), 1)

                def one_launch():
                    with torch.no_grad():
                        return pkg.anchor_pool_layers(a, layers, anchor, length if sides else None, sides=sides)

                def one_row():
                    with torch.no_grad():
                        return pkg.subword_pool_layers(a[rows, anchor][:, None], layers)[:, 0]

                forms = {"(a) dense": ref, "(b) composed": composed, "(c) one launch": one_launch}
                if not sides:
                    forms["(d) one row"] = one_row
                out = {k: f() for k, f in forms.items()}
                torch.cuda.synchronize()
                same = all(torch.equal(out["(b) composed"], out[k]) for k in out if k != "(a) dense")
                ref_err = float((out["(a) dense"].float() - out["(c) one launch"].float()).abs().max())
                del out
                v_b, m_b, a_b = B * T * D * s, B * T * D * 4, B * T * L * 4       # pooled words, a float32 [B,T,D], the transform
                z_b = B * D * 4
                dense = 2 * B * L * D * s + (B * L * D * s + v_b + a_b)          # torch.cat, torch.bmm
                pool = nnz * D * s + v_b + a_b
                moved = {"(a) dense": dense + 2 * B * D * s + (2 * v_b + 8 * m_b + 8 * z_b if sides else 0),
                         "(b) composed": pool + 2 * B * D * s + (2 * v_b + 8 * m_b + 8 * z_b if sides else 0),
                         "(c) one launch": walked * D * s + a_b + (3 if sides else 1) * z_b,
                         "(d) one row": nnz_anchor * D * s + 2 * B * L * 4 + a_b + B * D * s}
                peaks = {k: peak_above_inputs(f) for k, f in forms.items()}
                res = take_turns(forms)
                med = {k: statistics.median(v) for k, (v, _) in res.items()}
                parts = []
                for k, (v, seconds) in res.items():
                    parts.append("%s %.1f (%.1f..%.1f) us, %.4f GB, %.2f TB/s, peak %.4f GB [%.2f s timed]"
                                 % (k, med[k], min(v), max(v), moved[k] / 1e9, moved[k] / med[k] / 1e6, peaks[k] / 1e9, seconds))
                line = "%s n=%d B=%d T=%d L=%d %s (%d non-zeros, %d in the rows (c) walks): " % (
                    "bertdm sides=True " if sides else "bert_ed sides=False", n, B, T, L, str(dtype).replace("torch.", ""), nnz, walked)
                line += "   ".join(parts)
                line += "   | (a) / (c) %.2f   (b) / (c) %.2f" % (med["(a) dense"] / med["(c) one launch"],
                                                              med["(b) composed"] / med["(c) one launch"])
                if not sides:
                    line += "   (d) / (c) %.2f" % (med["(d) one row"] / med["(c) one launch"])
                line += "   | (b), (c)%s %s; max |(a) - (c)| %.3g" % ("" if sides else ", (d)", "agree bit for bit" if same else "DIFFER", ref_err)
                print(line, flush=True)
                lines.append(line)
                del layers, a
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
