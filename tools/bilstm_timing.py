#!/usr/bin/env python3
"""The inference BiLSTM (models/bert_amir5.py:557,610) ALONE: ``nn.LSTM`` (MIOpen / rocBLAS, what the classifier runs by default)
against ``recurrent.bilstm`` (one ``ggcn_linear`` at bf16x3 + one ``ggcn_bilstm_recurrence``), and the two launches of the HIP
form each by itself, in one process, under ``torch.no_grad()``.
Each form runs ALONE in steady state: warmed per shape, then windows of REPS steps between events that were created before the
first step; the forms take turns window group by window group, so a drift of the clocks shows in all of them.  Beside the time:
the largest difference of the two forms' outputs.  Last line: one evaluation step of the classifier without an encoder with
``ggcn_hip_lstm`` off and on.

``--train``: the TRAINING step of the BiLSTM alone, forward + backward with ``dX`` off as in the reference (BERT is frozen,
train.py:44): ``nn.LSTM`` under autograd against ``recurrent.bilstm_train``, and the plain recurrence launch, the saving one and the backward
launch each by itself, on the same shapes in one process.  Every step of both forms begins with an in-place update of ``weight_ih_l0``
and drops the gradients, so the HIP form packs its weight image every step, as after an optimizer step.  Beside the time: the
largest difference of the two forms' gradients, relative to the gradient's largest entry.

usage: bilstm_timing.py [--train] [output file]   (writes profiles/bilstm_timing.txt, with --train
profiles/bilstm_backward_timing.txt, by default)"""
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ed_gated_gcn_amd as pkg  # noqa: E402
from ed_gated_gcn_amd import _capi, recurrent  # noqa: E402

SHAPES = ((4096, 32), (512, 100), (512, 231), (256, 31), (8, 31))   # B x T, features 9216 wide
I = 9216
WARM, GROUPS, SKIP, WINDOWS = 3, 4, 1, 3


class _NoEncoder(torch.nn.Module):
    """Stands where BERT stands and returns twelve fixed random layers: the classifier step below has no encoder in it."""

    def forward(self, ids_, seg, output_all_encoded_layers=True):
        if not hasattr(self, "layers"):
            gen = torch.Generator(device=ids_.device).manual_seed(1)
            self.layers = [torch.randn(ids_.shape[0], ids_.shape[1], 768, device=ids_.device, generator=gen) for _ in range(12)]
            self.pooled = torch.zeros(ids_.shape[0], 768, device=ids_.device)
        return self.layers, self.pooled


def take_turns(forms, reps):
    """{name: [us per step of every kept window]} for ``forms`` {name: step()}: each alone in its windows, taking turns."""
    for step in forms.values():
        for _ in range(WARM):
            step()
    torch.cuda.synchronize()
    events = {n: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(WINDOWS)] for n in forms}
    res = {n: [] for n in forms}
    for group in range(GROUPS):
        for name, step in forms.items():
            for e0, e1 in events[name]:
                e0.record()
                for _ in range(reps):
                    step()
                e1.record()
            torch.cuda.synchronize()
            if group >= SKIP:
                res[name] += [e0.elapsed_time(e1) / reps * 1e3 for e0, e1 in events[name]]
    return res


def fmt(v):
    return "%.0f (%.0f..%.0f) us" % (statistics.median(v), min(v), max(v))


def classifier_step(dev, B=256, words=31, pieces=65, classes=34):
    """One evaluation step of ``GatedGCNEventDetector`` WITHOUT an encoder (sub-word pooling, BiLSTM, gate MLPs, gated block, dense,
    head) with ``ggcn_hip_lstm`` off and on; returns the report line."""
    import numpy as np

    from oracle.gpu_support import ace_batch
    inputs = {k: v.to(dev) for k, v in ace_batch(np.random.default_rng(3), B, words, pieces, vocab=30522).items()}
    models = {}
    for on in (False, True):
        opt = types.SimpleNamespace(dropout=0.0, polarities_dim=classes, device=dev, ggcn_hip_lstm=on)
        m = pkg.GatedGCNEventDetector(_NoEncoder(), opt)
        gen = torch.Generator().manual_seed(0)          # train.py:75-84 (the layers leave their parameters uninitialised)
        for p in m.parameters():
            if p.dim() > 1:
                torch.nn.init.xavier_uniform_(p, generator=gen)
            else:
                torch.nn.init.uniform_(p, -0.05, 0.05, generator=gen)
        models[on] = m.to(dev).eval()

    def step(on):
        with torch.no_grad():
            return models[on](inputs)

    res = take_turns({"off": lambda: step(False), "on": lambda: step(True)}, 10)
    diff = float((step(True)[0] - step(False)[0]).abs().max())
    return ("classifier evaluation step without an encoder, %d sentences of up to %d words: BiLSTM as nn.LSTM %s, with ggcn_hip_lstm %s"
            "   | logits, on against off: max|diff| %.3g" % (B, words, fmt(res["off"]), fmt(res["on"]), diff))


def train_main(path):
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    lib = pkg.load_library()
    lines = ["# %s; the BiLSTM's training step alone (forward + backward, dX off, float32, features %d wide), us per step: median "
             "(min..max) over %d windows, each form alone in its windows, the forms taking turns" % (
                 torch.cuda.get_device_name(0), I, (GROUPS - SKIP) * WINDOWS)]
    torch.manual_seed(0)
    lstm = torch.nn.LSTM(I, recurrent.HIDDEN, bidirectional=True, batch_first=True, num_layers=1).to(dev)
    for p in lstm.parameters():
        if p.dim() > 1:
            torch.nn.init.xavier_uniform_(p)
    H8, H2 = 8 * recurrent.HIDDEN, 2 * recurrent.HIDDEN
    ptr = _capi.ptr
    for B, T in SHAPES:
        x = torch.randn(B, T, I, device=dev)
        dy = torch.randn(B, T, H2, device=dev)

        def begin():
            lstm.zero_grad(set_to_none=True)
            with torch.no_grad():
                lstm.weight_ih_l0.add_(0.0)          # moves the version counter: the cached image is rebuilt

        def torch_form():
            begin()
            lstm(x)[0].backward(dy)

        def hip_form():
            begin()
            pkg.bilstm_train(x, lstm).backward(dy)

        torch_form()
        ref = {n: p.grad.clone() for n, p in lstm.named_parameters()}
        hip_form()
        diff = max(float((p.grad - ref[n]).abs().max()) / (float(ref[n].abs().max()) + 1e-30) for n, p in lstm.named_parameters())
        st = _capi.stream_of(dev)
        pack, whh_f, whh_r, bias_f, bias_r = recurrent._operands(lstm, lib, st)
        g = torch.empty(B * T, H8, device=dev)
        _capi.check(lib.ggcn_linear(ptr(x.view(B * T, I)), I, None, 0, ptr(pack), ptr(g), H8, B * T, I, H8, _capi.PREC["bf16x3"], st), "ggcn_linear")
        saved, dg = torch.empty(B * T, H8, device=dev), torch.empty(B * T, H8, device=dev)
        y, c, hprev = (torch.empty(B * T, H2, device=dev) for _ in range(3))

        def save():            # (gates in a buffer of their own here, so that every call reads the same G)
            _capi.check(lib.ggcn_bilstm_recurrence_save(ptr(g), H8, ptr(whh_f), ptr(whh_r), ptr(bias_f), ptr(bias_r), ptr(y), H2, B, T,
                                                        recurrent.HIDDEN, ptr(saved), ptr(c), ptr(hprev), st), "ggcn_bilstm_recurrence_save")

        def plain():           # the inference launch, for the cost of the three stores
            _capi.check(lib.ggcn_bilstm_recurrence(ptr(g), H8, ptr(whh_f), ptr(whh_r), ptr(bias_f), ptr(bias_r), ptr(y), H2, B, T,
                                                   recurrent.HIDDEN, st), "ggcn_bilstm_recurrence")

        def backward():
            _capi.check(lib.ggcn_bilstm_recurrence_backward(ptr(dy), H2, ptr(saved), H8, ptr(c), ptr(whh_f), ptr(whh_r), ptr(dg), H8, B, T,
                                                            recurrent.HIDDEN, st), "ggcn_bilstm_recurrence_backward")

        save()
        reps = 3 if B * T >= 50000 else 10
        res = take_turns({"nn.LSTM": torch_form, "bilstm_train": hip_form, "plain launch": plain, "save launch": save,
                          "backward launch": backward}, reps)
        line = "B=%d T=%d: " % (B, T) + "   ".join("%s %s" % (n, fmt(v)) for n, v in res.items())
        line += "   | nn.LSTM / bilstm_train %.2f   | gradients, bilstm_train against nn.LSTM: max|diff| / max|grad| %.3g" % (
            statistics.median(res["nn.LSTM"]) / statistics.median(res["bilstm_train"]), diff)
        print(line, flush=True)
        lines.append(line)
        del x, dy, g, saved, dg, y, c, hprev, ref
        lstm.zero_grad(set_to_none=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    if "--train" in sys.argv[1:]:
        rest = [a for a in sys.argv[1:] if a != "--train"]
        return train_main(rest[0] if rest else os.path.join(ROOT, "profiles", "bilstm_backward_timing.txt"))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bilstm_timing.txt")
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    lib = pkg.load_library()
    lines = ["# %s; the BiLSTM forward alone (no_grad, float32, features %d wide), us per call: median (min..max) over %d windows, each form "
             "alone in its windows, the forms taking turns" % (torch.cuda.get_device_name(0), I, (GROUPS - SKIP) * WINDOWS)]
    torch.manual_seed(0)
    lstm = torch.nn.LSTM(I, recurrent.HIDDEN, bidirectional=True, batch_first=True, num_layers=1).to(dev).requires_grad_(False)
    for p in lstm.parameters():
        if p.dim() > 1:
            torch.nn.init.xavier_uniform_(p)
    H8, H2 = 8 * recurrent.HIDDEN, 2 * recurrent.HIDDEN
    ptr = _capi.ptr
    for B, T in SHAPES:
        x = torch.randn(B, T, I, device=dev)
        with torch.no_grad():
            y_ref = lstm(x)[0]
            y_hip = pkg.bilstm(x, lstm)
        diff = float((y_hip - y_ref).abs().max())
        st = _capi.stream_of(dev)
        pack, whh_f, whh_r, bias_f, bias_r = recurrent._operands(lstm, lib, st)
        x2 = x.view(B * T, I)
        g = torch.empty(B * T, H8, device=dev)
        y = torch.empty(B, T, H2, device=dev)

        def torch_form():
            with torch.no_grad():
                return lstm(x)[0]

        def hip_form():
            with torch.no_grad():
                return pkg.bilstm(x, lstm)

        def projection():
            _capi.check(lib.ggcn_linear(ptr(x2), I, None, 0, ptr(pack), ptr(g), H8, B * T, I, H8, _capi.PREC["bf16x3"], st), "ggcn_linear")

        def recurrence():
            _capi.check(lib.ggcn_bilstm_recurrence(ptr(g), H8, ptr(whh_f), ptr(whh_r), ptr(bias_f), ptr(bias_r), ptr(y), H2, B, T,
                                                   recurrent.HIDDEN, st), "ggcn_bilstm_recurrence")

        projection()
        reps = 3 if B * T >= 50000 else 10
        res = take_turns({"nn.LSTM": torch_form, "bilstm": hip_form, "projection": projection, "recurrence": recurrence}, reps)
        line = "B=%d T=%d: " % (B, T) + "   ".join("%s %s" % (n, fmt(v)) for n, v in res.items())
        line += "   | nn.LSTM / bilstm %.2f   | bilstm against nn.LSTM: max|diff| %.3g" % (
            statistics.median(res["nn.LSTM"]) / statistics.median(res["bilstm"]), diff)
        print(line, flush=True)
        lines.append(line)
        del x, x2, g, y, y_ref, y_hip
        torch.cuda.empty_cache()
    lines.append(classifier_step(dev))
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
