"""The differentiable gate MLPs on the GPU (``heads.gate_mlps`` under autograd: ``ggcn_gate_mlp_save`` forward,
``ggcn_gate_mlp_backward`` + ``ggcn_dweight`` / ``ggcn_colsum`` backward).

The reference everywhere is float64 autograd through the ``nn.Sequential`` ops (``gate_mlp_ref.literal``:
``bert_amir5.py:562-571``) on the same float32 inputs; the gate is the project's gradient gate ``close32(got, ref, what, 2e-4)`` on
``d aspect`` and the eight parameter gradients, ``gates.gate`` on the gates themselves.  Shapes: ``gate_mlp_ref.SHAPES``.  A
parameter the loss does not reach (a loss on one gate only) may come back as ``None``; the reference must then be zero.
"""
import functools
import types

import pytest
import torch

from oracle import gates
from oracle.gpu_support import call_log, classifier_batch, dev, pkg  # noqa: F401

import gate_mlp_ref as gm

pytestmark = pytest.mark.gpu
REL = 2e-4                                   # tests/test_gpu_backward.py: the gradient gate
SAVE, BACKWARD, DWEIGHT, COLSUM = "ggcn_gate_mlp_save", "ggcn_gate_mlp_backward", "ggcn_dweight", "ggcn_colsum"
ids = lambda s: "x".join(map(str, s))        # noqa: E731


@functools.lru_cache(maxsize=None)
def _inputs(shape, variant="plain"):
    """Seeded inputs on the GPU, made once per (shape, variant) and never modified."""
    t = gm.make_inputs(shape, seed=sum(shape), device="cuda:0")
    if variant == "aspect30":
        t["aspect"] = t["aspect"] * 30.0
    elif variant == "weights20":
        for k in gm.PARAMS:
            t[k] = t[k] * 20.0
    elif variant == "shared":
        for p in ("w1", "b1", "w2", "b2"):
            t[p + "_b"] = t[p + "_a"]
    elif variant == "bf16":
        t["aspect"] = t["aspect"].to(torch.bfloat16).float()
    return t


@functools.lru_cache(maxsize=None)
def _reference(shape, which, variant="plain"):
    return gm.autograd64(_inputs(shape, variant), which)


def _seq(t, gate):
    H = t["aspect"].shape[1]
    nn = torch.nn
    seq = nn.Sequential(nn.Sigmoid(), nn.Linear(H, H), nn.Sigmoid(), nn.Linear(H, H), nn.Sigmoid()).to(t["aspect"].device)
    with torch.no_grad():
        for lin, p in ((seq[1], "1"), (seq[3], "2")):
            lin.weight.copy_(t["w%s_%s" % (p, gate)])
            lin.bias.copy_(t["b%s_%s" % (p, gate)])
    return seq


def _params(s1, s2):
    return {"w1_a": s1[1].weight, "b1_a": s1[1].bias, "w2_a": s1[3].weight, "b2_a": s1[3].bias,
            "w1_b": s2[1].weight, "b1_b": s2[1].bias, "w2_b": s2[3].weight, "b2_b": s2[3].bias}


def _run(pkg, t, which, need=gm.NAMES, shared=False, strided=False, aspect=None):
    """One forward + backward through ``gate_mlps``: ``(g1, g2, {name: gradient or None})``."""
    s1 = _seq(t, "a")
    s2 = s1 if shared else _seq(t, "b")
    params = _params(s1, s2)
    for k, p in params.items():
        p.requires_grad_(k in need)
    a = (t["aspect"] if aspect is None else aspect).detach().clone().requires_grad_("aspect" in need)
    g1, g2 = pkg.gate_mlps(a, s1, s2)
    assert g1.grad_fn is not None and g2.grad_fn is not None, "gate_mlps returned gates without a grad_fn"
    names = [k for k in gm.NAMES if k in need and not (shared and k.endswith("_b"))]
    wanted = [a if k == "aspect" else params[k] for k in names]
    if strided:        # the gradients of the loss "both", handed over explicitly: dG_A = r1 with strides (1, B)
        assert which == "both"
        r1 = t["r1"].t().contiguous().t()
        assert (not r1.is_contiguous() or min(r1.shape) == 1) and torch.equal(r1, t["r1"])
        grads = torch.autograd.grad([g1, g2], wanted, grad_outputs=[r1, t["r2"]], allow_unused=True)
    else:
        grads = torch.autograd.grad(gm.loss_of(g1, g2, t["r1"], t["r2"], which), wanted, allow_unused=True)
    return g1.detach(), g2.detach(), dict(zip(names, grads))


def _gate_all(got, ref, what, names=gm.NAMES):
    for k in names:
        r = ref["d" + k]
        if got[k] is None:
            assert float(r.abs().max()) == 0.0, "%s d %s: None where the reference is not zero" % (what, k)
            continue
        assert got[k].shape == r.shape, (what, k)
        gates.close32(got[k], r, "%s d %s" % (what, k), REL)


# ================================================================ 1. the feature: gradients against float64 autograd
@pytest.mark.parametrize("which", gm.LOSSES)
@pytest.mark.parametrize("shape", gm.SHAPES, ids=ids)
def test_gradients_against_float64_autograd(pkg, dev, shape, which):
    t, ref = _inputs(shape), _reference(shape, which)
    g1, g2, got = _run(pkg, t, which)
    gates.gate(g1, ref["g1"], "g1")
    gates.gate(g2, ref["g2"], "g2")
    _gate_all(got, ref, "%s/%s" % (ids(shape), which))
    assert got["aspect"].is_contiguous() and got["aspect"].shape == t["aspect"].shape
    reached = {"g1": "_a", "g2": "_b", "both": ""}[which]
    assert all(got[k] is not None for k in gm.PARAMS if k.endswith(reached)), "a parameter the loss reaches got no gradient"


# ================================================================ 2. the forward is today's
@pytest.mark.parametrize("shape", gm.SHAPES, ids=ids)
def test_forward_is_bitwise_the_no_grad_call(pkg, dev, shape):
    t = _inputs(shape)
    s1, s2 = _seq(t, "a"), _seq(t, "b")
    with torch.no_grad():
        a0, b0 = pkg.gate_mlps(t["aspect"], s1, s2)
    assert a0.grad_fn is None and b0.grad_fn is None
    a1, b1, _ = _run(pkg, t, "both")
    assert torch.equal(a0, a1) and torch.equal(b0, b1)
    for p in list(s1.parameters()) + list(s2.parameters()):      # nothing requires grad: today's path, with grad enabled too
        p.requires_grad_(False)
    a2, b2 = pkg.gate_mlps(t["aspect"], s1, s2)
    assert a2.grad_fn is None and b2.grad_fn is None and torch.equal(a0, a2) and torch.equal(b0, b2)


# ================================================================ 3. the same bits on every call
@pytest.mark.parametrize("shape", gm.SHAPES, ids=ids)
def test_backward_is_bit_repeatable(pkg, dev, shape):
    t = _inputs(shape)
    _, _, a = _run(pkg, t, "both")
    _, _, b = _run(pkg, t, "both")
    for k in gm.NAMES:
        assert torch.equal(a[k], b[k]), k


# ================================================================ 4. hostile memory at the C call
HOSTILE = [(3, 64), (17, 30), (9, 256)]


@pytest.mark.parametrize("which", ["both", "g2"])
@pytest.mark.parametrize("shape", HOSTILE, ids=ids)
def test_c_call_reads_a_padded_aspect_and_writes_inside_its_columns_only(pkg, dev, shape, which):
    from ed_gated_gcn_amd import _capi
    lib, ptr, st = pkg.load_library(), _capi.ptr, _capi.stream_of(dev)
    B, H = shape
    Hp = (H + 3) & ~3
    t, ref = _inputs(shape), _reference(shape, which)
    a = gates.hostile(t["aspect"], 3)[:B, :H]                    # row stride H + 3; NaN beside and below
    assert a.stride(0) == H + 3
    wt = {k: t[k].t().contiguous() for k in ("w1_a", "w2_a", "w1_b", "w2_b")}
    g1, g2, hid_a, hid_b = (torch.empty(B, H, device=dev) for _ in range(4))
    _capi.check(lib.ggcn_gate_mlp_save(ptr(a), a.stride(0), B, H, ptr(wt["w1_a"]), ptr(t["b1_a"]), ptr(wt["w2_a"]), ptr(t["b2_a"]), ptr(g1),
                                       ptr(wt["w1_b"]), ptr(t["b1_b"]), ptr(wt["w2_b"]), ptr(t["b2_b"]), ptr(g2), ptr(hid_a), ptr(hid_b), st),
                SAVE)
    gates.gate(g1, ref["g1"], "C call g1")
    gates.gate(g2, ref["g2"], "C call g2")
    st64 = gm.statement64(t, None, None)
    GUARD, PAD = 64, 3
    da_whole, da = gates.poisoned_rows(dev, B, H + PAD, GUARD)
    z_whole, Z = gates.poisoned_rows(dev, B, 5 * Hp + PAD, GUARD)
    dg_a = None if which == "g2" else t["r1"]
    _capi.check(lib.ggcn_gate_mlp_backward(ptr(a), a.stride(0), B, H, ptr(t["w1_a"]), ptr(t["w2_a"]), ptr(hid_a), ptr(g1), ptr(dg_a),
                                           ptr(t["w1_b"]), ptr(t["w2_b"]), ptr(hid_b), ptr(g2), ptr(t["r2"]),
                                           ptr(da), H + PAD, ptr(Z), 5 * Hp + PAD, st), BACKWARD)
    torch.cuda.synchronize()
    for name, whole, view, width in (("d_aspect", da_whole, da, H), ("Z", z_whole, Z, 5 * Hp)):
        assert bool(torch.isnan(whole[:GUARD]).all()) and bool(torch.isnan(whole[-GUARD:]).all()), "%s: a guard band was written" % name
        assert bool(torch.isnan(view[:, width:]).all()), "%s: padding columns were written" % name
        assert bool(torch.isfinite(view[:, :width]).all()), name
    group = lambda g: Z[:, g * Hp:g * Hp + H].contiguous()          # noqa: E731
    for g in range(5):
        assert not bool(Z[:, g * Hp + H:(g + 1) * Hp].any()), "the columns behind group %d's H are not zeros" % g
    if which == "g2":
        assert not bool(group(0).any()) and not bool(group(2).any()), "gate A got no gradient: its groups must be zeros"
    gates.close32(da[:, :H], ref["daspect"], "C call d aspect", REL)
    gates.gate(group(4), st64["Z"][:, 4 * H:], "C call s")
    s, hid = group(4), {"a": hid_a, "b": hid_b}
    for i, gate in enumerate("ab"):                                # what the library's products would give, as torch products
        gates.close32(group(i).t() @ s, ref["dw1_" + gate], "C call dz1^T . s " + gate, REL)
        gates.close32(group(2 + i).t() @ hid[gate], ref["dw2_" + gate], "C call dz2^T . hid " + gate, REL)
        gates.close32(group(i).sum(0), ref["db1_" + gate], "C call sum dz1 " + gate, REL)
        gates.close32(group(2 + i).sum(0), ref["db2_" + gate], "C call sum dz2 " + gate, REL)


# ================================================================ 5. needs_input_grad: what gets launched and returned
NIG = (9, 256)
D_GATE_A, D_GATE_B, D_ASPECT, Z_ARG = 8, 13, 14, 16              # positions in ggcn_gate_mlp_backward's arguments


def test_everything_trains_in_five_calls(pkg, dev, monkeypatch):
    t = _inputs(NIG)
    calls = call_log(monkeypatch, [SAVE, "ggcn_gate_mlp", BACKWARD, DWEIGHT, COLSUM])
    _run(pkg, t, "both")
    assert [n for n, _ in calls] == [SAVE, BACKWARD, DWEIGHT, DWEIGHT, DWEIGHT, COLSUM]
    assert calls[2][1][5] == 2 * NIG[1], "dW1 of both gates is one product with K = 2 H"


def test_only_aspect_needs_a_gradient(pkg, dev, monkeypatch):
    t, ref = _inputs(NIG), _reference(NIG, "both")
    calls = call_log(monkeypatch, [BACKWARD, DWEIGHT, COLSUM])
    _, _, got = _run(pkg, t, "both", need=("aspect",))
    _gate_all(got, ref, "aspect only", ("aspect",))
    assert [n for n, _ in calls] == [BACKWARD]
    assert calls[0][1][D_ASPECT] is not None and calls[0][1][Z_ARG] is None


def test_frozen_gate1_gets_none_and_no_product(pkg, dev, monkeypatch):
    t, ref = _inputs(NIG), _reference(NIG, "both")
    s1, s2 = _seq(t, "a"), _seq(t, "b")
    for p in s1.parameters():
        p.requires_grad_(False)
    calls = call_log(monkeypatch, [BACKWARD, DWEIGHT, COLSUM])
    g1, g2 = pkg.gate_mlps(t["aspect"], s1, s2)                   # aspect detached too: the W1 pass is skipped
    gm.loss_of(g1, g2, t["r1"], t["r2"], "both").backward()
    assert [n for n, _ in calls] == [BACKWARD, DWEIGHT, DWEIGHT, COLSUM]
    assert calls[0][1][D_ASPECT] is None and calls[0][1][Z_ARG] is not None
    assert all(p.grad is None for p in s1.parameters())
    params = _params(s1, s2)
    for k in ("w1_b", "b1_b", "w2_b", "b2_b"):
        gates.close32(params[k].grad, ref["d" + k], "frozen gate1 d " + k, REL)


def test_a_loss_on_one_gate_hands_the_launch_a_null(pkg, dev, monkeypatch):
    t = _inputs(NIG)
    calls = call_log(monkeypatch, [BACKWARD])
    for which in gm.LOSSES:
        _run(pkg, t, which)
    (a, b, both) = (c[1] for c in calls)
    assert a[D_GATE_A] is not None and a[D_GATE_B] is None
    assert b[D_GATE_A] is None and b[D_GATE_B] is not None
    assert both[D_GATE_A] is not None and both[D_GATE_B] is not None


@pytest.mark.parametrize("shape", [(9, 256), (17, 30)], ids=ids)
def test_the_same_sequential_for_both_gates(pkg, dev, shape):
    t, ref = _inputs(shape, "shared"), _reference(shape, "both", "shared")
    g1, g2, got = _run(pkg, t, "both", shared=True)
    assert torch.equal(g1, g2)
    gates.close32(got["aspect"], ref["daspect"], "shared d aspect", REL)
    for p in ("w1", "b1", "w2", "b2"):                             # autograd adds the two gates' gradients
        gates.close32(got[p + "_a"], ref["d%s_a" % p] + ref["d%s_b" % p], "shared d " + p, REL)


@pytest.mark.parametrize("shape", [(3, 64), (17, 30)], ids=ids)
def test_strided_incoming_gradient(pkg, dev, shape, monkeypatch):
    t = _inputs(shape)
    seen = []
    from ed_gated_gcn_amd import heads
    orig = heads._GateMlps.backward

    def spy(ctx, dg1, dg2):
        seen.append(dg1.is_contiguous())
        return orig(ctx, dg1, dg2)
    monkeypatch.setattr(heads._GateMlps, "backward", staticmethod(spy))
    _, _, a = _run(pkg, t, "both")
    _, _, b = _run(pkg, t, "both", strided=True)
    assert seen == [True, False], "the second gradient was meant to arrive strided: %s" % seen
    for k in gm.NAMES:
        assert torch.equal(a[k], b[k]), k


def test_bf16_aspect_under_autocast(pkg, dev):
    """A bfloat16 ``aspect`` is cast by a differentiable ``.float()``: its gradient comes back as bfloat16, one rounding of the
    float32 value (``gates.gate_dx``: 2^-8 |ref| + 1e-4 max|ref|); the parameters' gradients stay float32."""
    shape = (9, 256)
    t, ref = _inputs(shape, "bf16"), _reference(shape, "both", "bf16")
    s1, s2 = _seq(t, "a"), _seq(t, "b")
    a = t["aspect"].to(torch.bfloat16).requires_grad_()
    assert torch.equal(a.detach().float(), t["aspect"])
    with torch.autocast("cuda", dtype=torch.bfloat16):
        g1, g2 = pkg.gate_mlps(a, s1, s2)
    assert g1.grad_fn is not None and g2.grad_fn is not None
    gates.gate(g1.detach(), ref["g1"], "g1")
    gates.gate(g2.detach(), ref["g2"], "g2")
    gm.loss_of(g1, g2, t["r1"], t["r2"], "both").backward()
    gates.gate_dx(a.grad, ref["daspect"], "d aspect")
    for k, p in _params(s1, s2).items():
        gates.close32(p.grad, ref["d" + k], "bf16 aspect d " + k, REL)


# ================================================================ 6. extremes, with the summed loss
@pytest.mark.parametrize("variant", ["aspect30", "weights20"])
@pytest.mark.parametrize("shape", [(9, 256), (5, 300)], ids=ids)
def test_extremes(pkg, dev, shape, variant):
    t, ref = _inputs(shape, variant), _reference(shape, "both", variant)
    if variant == "weights20":
        sat = ((ref["g1"] < 1e-3) | (ref["g1"] > 1 - 1e-3)).double().mean()
        assert float(sat) > 0.5, "weights * 20 were meant to saturate the gates"
    g1, g2, got = _run(pkg, t, "both")
    assert not any(bool(torch.isnan(v).any()) for v in (g1, g2) + tuple(got.values()))
    gates.gate(g1, ref["g1"], "g1")
    gates.gate(g2, ref["g2"], "g2")
    _gate_all(got, ref, "%s/%s" % (ids(shape), variant))


# ================================================================ 7. the classifier with the option on
class _Bert(torch.nn.Module):
    """The stand-in BERT of the classifier tests: twelve seeded [B,L,768] layers, a zero pooled output."""

    def forward(self, ids_, seg, output_all_encoded_layers=True):
        gen = torch.Generator(device=ids_.device).manual_seed(1)
        return ([torch.randn(ids_.shape[0], ids_.shape[1], 768, device=ids_.device, generator=gen) for _ in range(12)],
                torch.zeros(ids_.shape[0], 768, device=ids_.device))


def _training_step(pkg, dev, cls_name, inputs, ncls, gate_backward):
    opt = types.SimpleNamespace(dropout=0.0, polarities_dim=ncls, device=dev, ggcn_gate_backward=gate_backward)
    m = getattr(pkg, cls_name)(_Bert(), opt)
    assert m.gate_backward is gate_backward and m.head_backward is False
    gen = torch.Generator().manual_seed(0)
    for p in m.parameters():
        if p.dim() > 1:
            torch.nn.init.xavier_uniform_(p, generator=gen)
        else:
            torch.nn.init.uniform_(p, -0.05, 0.05, generator=gen)
    m = m.to(dev).train()
    torch.manual_seed(11)
    logits, xy, kl, scores = m(inputs)
    r = torch.randn(scores.shape, generator=torch.Generator().manual_seed(4)).to(dev)
    target = torch.arange(logits.shape[0], device=dev) % ncls
    loss = torch.nn.functional.cross_entropy(logits, target) + xy + kl + (scores * r).mean()
    loss.backward()
    grads = {n: p.grad for n, p in m.named_parameters() if n.split(".")[0] in ("fc", "dense", "lstm", "gc1", "gc2", "gate1", "gate2")}
    xy = xy.detach() if torch.is_tensor(xy) else torch.tensor(float(xy), device=dev)     # (the gateless variant: xy = 0.0)
    return (logits.detach(), xy, kl.detach(), scores.detach()), grads


@pytest.mark.parametrize("cls_name", ["GatedGCNEventDetector", "GatedGCNEventDetector54"])
def test_classifier_training_step_with_the_option(pkg, dev, cls_name, monkeypatch):
    monkeypatch.delenv("GGCN_GATE_BACKWARD", raising=False)
    monkeypatch.delenv("GGCN_HEAD_BACKWARD", raising=False)
    inputs, ncls = classifier_batch(dev)
    calls = call_log(monkeypatch, ["ggcn_gate_mlp", SAVE, BACKWARD])
    out_off, g_off = _training_step(pkg, dev, cls_name, inputs, ncls, False)
    assert calls == [], "the option is off: the gate MLPs are the two nn.Sequential"
    out_on, g_on = _training_step(pkg, dev, cls_name, inputs, ncls, True)
    assert [n for n, _ in calls] == [SAVE, BACKWARD]
    for got, ref, what in zip(out_on, out_off, ("logits", "xy", "kl", "scores")):
        gates.gate(got, ref, "%s %s" % (cls_name, what))
    assert sorted(g_on) == sorted(g_off) and len(g_on) >= 16
    for n in sorted(g_on):
        assert g_on[n] is not None and g_off[n] is not None, n
        gates.close32(g_on[n], g_off[n], "%s d %s" % (cls_name, n), REL)


def test_the_gateless_classifier_is_unaffected(pkg, dev, monkeypatch):
    monkeypatch.delenv("GGCN_GATE_BACKWARD", raising=False)
    monkeypatch.delenv("GGCN_HEAD_BACKWARD", raising=False)
    inputs, ncls = classifier_batch(dev)
    calls = call_log(monkeypatch, ["ggcn_gate_mlp", SAVE, BACKWARD])
    out_off, _ = _training_step(pkg, dev, "GCNEventDetectorNoGate", inputs, ncls, False)
    out_on, g_on = _training_step(pkg, dev, "GCNEventDetectorNoGate", inputs, ncls, True)
    assert calls == [], "55nogate has no gates to compute"
    for got, ref, what in zip(out_on, out_off, ("logits", "xy", "kl", "scores")):
        gates.gate(got, ref, "55nogate " + what)
    assert all(g is None for n, g in g_on.items() if n.startswith("gate"))
