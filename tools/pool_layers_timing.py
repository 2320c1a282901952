#!/usr/bin/env python3
"""Sub-word pooling from BERT's twelve layer outputs (models/bert_amir5.py:596,600), three forms in one process:

  (a) cat+pool    ``subword_pool(transform, torch.cat(layers, -1))``: what the classifier runs by default
  (b) 12 calls    twelve ``ggcn_subword_pool`` calls at the C ABI, layer l into columns l*768 .. of one Y (no concatenation)
  (c) one launch  ``subword_pool_layers(transform, layers)``: ``ggcn_subword_pool_layers``

on reference-like transforms (``oracle.subword_pool_cases.transform_like_reference``), 12 x 768 features, float32 at every shape
and bfloat16 at the largest.  Each form is warmed per shape, then runs ALONE in windows of REPS calls between two device events
that end in a synchronise; the forms take turns window group by window group, and REPS is chosen per form so that its timed
windows add up to at least MIN_SECONDS.  Every form allocates its result in every call.  Beside the median time: the bytes the
form must move, computed from the shapes and the transform's non-zeros (every selected row of x once per word it belongs to,
Y once, the transform once; for (a) the concatenation's read and write of every element of the layers on top), the resulting
TB/s, and for (a) and (c) the peak of ``torch.cuda.max_memory_allocated`` above the inputs.  The three results are compared bit
for bit first.

usage: pool_layers_timing.py [output file]   (writes profiles/pool_layers_timing.txt by default)"""
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ed_gated_gcn_amd as pkg  # noqa: E402
from ed_gated_gcn_amd import _capi  # noqa: E402
from oracle.subword_pool_cases import transform_like_reference  # noqa: E402

SHAPES = ((32, 31, 64, torch.float32), (256, 31, 64, torch.float32), (4096, 32, 65, torch.float32), (4096, 32, 65, torch.bfloat16))
N_LAYERS, DL = 12, 768
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
        reps[name] = max(2, int(np.ceil(1.25 * MIN_SECONDS / (GROUPS * WINDOWS) / per_call)))   # (a steady call is faster than these)
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


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pool_layers_timing.txt")
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    lib = pkg.load_library()
    lines = ["# %s; sub-word pooling of %d x %d features from BERT's layer list, no_grad; us per call: median (min..max) over %d or more windows of "
             "at least %.1f s together, each form alone in its windows, the forms taking turns; GB: what the form must move, from the "
             "shapes and the transform's non-zeros" % (torch.cuda.get_device_name(0), N_LAYERS, DL, GROUPS * WINDOWS, MIN_SECONDS)]
    for B, T, L, dtype in SHAPES:
        rng = np.random.default_rng(B * 1000 + L)
        tr = transform_like_reference(B, T, L, rng)
        nnz = int(np.count_nonzero(tr))
        a = torch.from_numpy(tr).to(dev)
        gen = torch.Generator(device=dev).manual_seed(1)
        layers = [torch.randn(B, L, DL, device=dev, generator=gen).to(dtype) for _ in range(N_LAYERS)]
        s, D = layers[0].element_size(), N_LAYERS * DL
        bf16 = dtype == torch.bfloat16
        one = lib.ggcn_subword_pool_bf16 if bf16 else lib.ggcn_subword_pool
        st = _capi.stream_of(dev)
        sb, sr, sc = a.stride()

        def cat_pool():
            with torch.no_grad():
                return pkg.subword_pool(a, torch.cat(layers, -1))

        def twelve_calls():
            y = torch.empty(B, T, D, dtype=dtype, device=dev)
            for l, x in enumerate(layers):
                _capi.check(one(_capi.ptr(a), sb, sr, sc, _capi.ptr(x), x.stride(0), x.stride(1), ctypes.c_void_p(y.data_ptr() + l * DL * s),
                                T * D, D, B, T, L, DL, st), "ggcn_subword_pool")
            return y

        def one_launch():
            with torch.no_grad():
                return pkg.subword_pool_layers(a, layers)

        ya, yb, yc = cat_pool(), twelve_calls(), one_launch()
        torch.cuda.synchronize()
        same = torch.equal(ya, yb) and torch.equal(ya, yc)
        del ya, yb, yc
        pool_bytes = nnz * D * s + B * T * D * s + B * T * L * 4
        cat_bytes = 2 * B * L * D * s
        moved = {"(a) cat+pool": cat_bytes + pool_bytes, "(b) 12 calls": pool_bytes, "(c) one launch": pool_bytes}
        peaks = {"(a) cat+pool": peak_above_inputs(cat_pool), "(c) one launch": peak_above_inputs(one_launch)}
        res = take_turns({"(a) cat+pool": cat_pool, "(b) 12 calls": twelve_calls, "(c) one launch": one_launch})
        parts = []
        for name, (v, seconds) in res.items():
            med = statistics.median(v)
            text = "%s %.1f (%.1f..%.1f) us, %.3f GB, %.2f TB/s" % (name, med, min(v), max(v), moved[name] / 1e9, moved[name] / med / 1e6)
            if name in peaks:
                text += ", peak above the inputs %.3f GB" % (peaks[name] / 1e9)
            parts.append(text + " [%.2f s timed]" % seconds)
        med = {n: statistics.median(v) for n, (v, _) in res.items()}
        line = "B=%d T=%d L=%d %s (%d non-zeros; the concatenation alone moves %.3f GB): " % (
            B, T, L, str(dtype).replace("torch.", ""), nnz, cat_bytes / 1e9) + "   ".join(parts)
        line += "   | (a) / (c) %.2f, (a) - (c) %.1f us   (b) / (c) %.2f   | the three results %s" % (
            med["(a) cat+pool"] / med["(c) one launch"], med["(a) cat+pool"] - med["(c) one launch"],
            med["(b) 12 calls"] / med["(c) one launch"], "agree bit for bit" if same else "DIFFER")
        print(line, flush=True)
        lines.append(line)
        del layers, a
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
