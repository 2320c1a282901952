#!/usr/bin/env python3
"""From BERT's twelve layer outputs to the BiLSTM's output and the anchor word's row (models/bert_amir5.py:596-610), three forms
in one process:

  (a) cat+pool+bilstm     ``torch.cat`` + ``subword_pool`` + the row gather ``x[rows, anchor]`` + ``bilstm``
  (b) pool_layers+bilstm  ``subword_pool_layers`` + the row gather + ``bilstm``            (the best path before ``bilstm_layers``)
  (c) bilstm_layers       ``anchor_pool_layers(sides=False)`` + ``bilstm_layers``: no [B,L,9216], no [B,T,9216]

on reference-like transforms (``oracle.subword_pool_cases.transform_like_reference``), 12 x 768 features, float32.  Each form is
warmed per shape, then runs ALONE in windows of REPS calls between two device events that end in a synchronise; the forms take
turns window group by window group, and REPS is chosen per form so that its timed windows add up to at least MIN_SECONDS.  Every
form allocates its results in every call.  The launches a form is made of are timed the same way, each alone on operands made
beforehand, in the same turns.  Beside the median: min..max over the windows (the spread that decides whether (c) - (b) means
anything) and the peak of ``torch.cuda.max_memory_allocated`` above the inputs.  The three results are compared bit for bit first.

usage: lstm_layers_timing.py [output file]   (writes profiles/lstm_layers_timing.txt by default)"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ed_gated_gcn_amd as pkg  # noqa: E402
from ed_gated_gcn_amd import _capi, hostops, recurrent  # noqa: E402
from oracle.subword_pool_cases import transform_like_reference  # noqa: E402

SHAPES = ((32, 31, 64), (256, 31, 64), (4096, 32, 65))
N_LAYERS, DL, HD = 12, 768, 128
WARM, GROUPS, WINDOWS, MIN_SECONDS = 3, 3, 3, 0.5
A, B_, C = "(a) cat+pool+bilstm", "(b) pool_layers+bilstm", "(c) bilstm_layers"


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
        per_call = window(step, 10) / 10
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
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "lstm_layers_timing.txt")
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    lib = pkg.load_library()
    lines = ["# %s; %d x %d features from BERT's layer list to the BiLSTM's output [B,T,256] and the anchor row [B,9216], float32, "
             "no_grad; us per call: median (min..max) over %d or more windows of at least %.1f s together, each form and each "
             "launch alone in its windows, all taking turns; peak: max_memory_allocated above the inputs"
             % (torch.cuda.get_device_name(0), N_LAYERS, DL, GROUPS * WINDOWS, MIN_SECONDS)]
    lstm = torch.nn.LSTM(N_LAYERS * DL, HD, bidirectional=True, batch_first=True, num_layers=1).to(dev)
    for p in lstm.parameters():
        p.requires_grad_(False)
    for Bn, T, L in SHAPES:
        rng = np.random.default_rng(Bn * 1000 + L)
        tr = transform_like_reference(Bn, T, L, rng)
        counts = np.count_nonzero(tr, axis=2)
        a = torch.from_numpy(tr).to(dev)
        anchor = torch.from_numpy(rng.integers(0, T, size=Bn)).to(dev)
        rows = torch.arange(Bn, device=dev)
        gen = torch.Generator(device=dev).manual_seed(1)
        layers = [torch.randn(Bn, L, DL, device=dev, generator=gen) for _ in range(N_LAYERS)]
        st = _capi.stream_of(dev)
        F = 8 * HD

        def form_a():
            with torch.no_grad():
                x = pkg.subword_pool(a, torch.cat(layers, -1))
                return x[rows, anchor], pkg.bilstm(x, lstm)

        def form_b():
            with torch.no_grad():
                x = pkg.subword_pool_layers(a, layers)
                return x[rows, anchor], pkg.bilstm(x, lstm)

        def form_c():
            with torch.no_grad():
                return pkg.anchor_pool_layers(a, layers, anchor, None, sides=False), pkg.bilstm_layers(a, layers, lstm)

        ra, rb, rc = form_a(), form_b(), form_c()
        torch.cuda.synchronize()
        same = all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(ra, rb, rc))
        del ra, rb, rc
        assert pkg.takes_hip_lstm_layers(a, layers, lstm, 0)
        peaks = {A: peak_above_inputs(form_a), B_: peak_above_inputs(form_b), C: peak_above_inputs(form_c)}
        # the launches, each on operands made beforehand
        with torch.no_grad():
            xcat = torch.cat(layers, -1)
            pooled = pkg.subword_pool_layers(a, layers)
            pack, whh_f, whh_r, bias_f, bias_r = recurrent._operands(lstm, lib, st)
            g = hostops.linear_packed(lib, st, pooled.view(Bn * T, -1), N_LAYERS * DL, pack, Bn * T, N_LAYERS * DL, F)
        y = torch.empty(Bn, T, 2 * HD, device=dev)
        head, dims, _ = recurrent._pooled_args(a, layers, real=True)

        def pooled_projection():
            out = torch.empty(Bn * T, F, device=dev)
            _capi.check(lib.ggcn_linear_pooled_layers(*head, _capi.ptr(pack), _capi.ptr(out), F, *dims, F, st), "ggcn_linear_pooled_layers")
            return out

        def recurrence():
            _capi.check(lib.ggcn_bilstm_recurrence(_capi.ptr(g), F, _capi.ptr(whh_f), _capi.ptr(whh_r), _capi.ptr(bias_f), _capi.ptr(bias_r),
                                                   _capi.ptr(y), 2 * HD, Bn, T, HD, st), "ggcn_bilstm_recurrence")

        parts = {
            "torch.cat": lambda: torch.cat(layers, -1),
            "subword_pool": lambda: pkg.subword_pool(a, xcat),
            "subword_pool_layers": lambda: pkg.subword_pool_layers(a, layers),
            "row gather": lambda: pooled[rows, anchor],
            "ggcn_linear": lambda: hostops.linear_packed(lib, st, pooled.view(Bn * T, -1), N_LAYERS * DL, pack, Bn * T, N_LAYERS * DL, F),
            "ggcn_bilstm_recurrence": recurrence,
            "anchor_pool_layers": lambda: pkg.anchor_pool_layers(a, layers, anchor, None, sides=False),
            "ggcn_linear_pooled_layers": pooled_projection,
        }
        with torch.no_grad():
            res = take_turns(dict({A: form_a, B_: form_b, C: form_c}, **parts))
        med = {n: statistics.median(v) for n, (v, _) in res.items()}
        text = []
        for name in (A, B_, C):
            v, seconds = res[name]
            text.append("%s %.1f (%.1f..%.1f) us, peak above the inputs %.3f GB [%.2f s timed]"
                        % (name, med[name], min(v), max(v), peaks[name] / 1e9, seconds))
        split = {A: ("torch.cat", "subword_pool", "row gather", "ggcn_linear", "ggcn_bilstm_recurrence"),
                 B_: ("subword_pool_layers", "row gather", "ggcn_linear", "ggcn_bilstm_recurrence"),
                 C: ("anchor_pool_layers", "ggcn_linear_pooled_layers", "ggcn_bilstm_recurrence")}
        for name in (A, B_, C):
            text.append("%s = %s" % (name[:3], " + ".join("%s %.1f (%.1f..%.1f)" % (p, med[p], min(res[p][0]), max(res[p][0]))
                                                           for p in split[name])))
        vb = res[B_][0]
        spread = max(vb) - min(vb)
        diff = med[C] - med[B_]
        verdict = "(c) is faster" if diff < 0 else ("(c) is slower, inside the spread of (b)" if diff <= spread else "(c) is SLOWER than (b) by more than its spread")
        line = ("B=%d T=%d L=%d (%d words, non-zeros a word: mean %.2f, %d words of more than two, the most %d): "
                % (Bn, T, L, int((counts > 0).sum()), counts[counts > 0].mean(), int((counts > 2).sum()), int(counts.max()))
                + "   ".join(text)
                + "   | (c) - (b) %+.1f us, (b) / (c) %.2f, spread of (b) between its windows %.1f us: %s   | the three results %s"
                % (diff, med[B_] / med[C], spread, verdict, "agree bit for bit" if same else "DIFFER"))
        print(line, flush=True)
        lines.append(line)
        del layers, a, xcat, pooled, g, y
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
