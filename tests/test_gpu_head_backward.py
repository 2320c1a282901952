"""The differentiable scores / kl head on the GPU (``heads.scores_and_kl`` under autograd: ``ggcn_scores_head`` +
``ggcn_overlap_reduce`` forward, ``ggcn_scores_head_backward`` + ``ggcn_scores_head_dweight`` backward).

The reference everywhere is float64 autograd through the reference's literal ops (``head_backward_ref.literal``:
``bert_amir5.py:645-648``) on the same float32 inputs; the gate is the project's gradient gate ``close32(got, ref, what, 2e-4)``
on ``dX``, ``d aspect``, ``d logits``, ``d fc.weight`` and ``d fc.bias``.  Shapes: ``head_backward_ref.SHAPES``.

The extremes (a saturated softmax, ``dist`` all equal or with one large entry) are run with the loss that uses both outputs:
there the gradient of ``kl`` alone is zero or next to it by cancellation (``q_t - kl_b`` with every ``q_t`` equal; ``p_t`` of
``e^-100``) while the float32 scores it is recomputed from carry an absolute rounding of ~1e-5 at a magnitude in the hundreds, so
a gate relative to that gradient's own maximum would measure the forward's scores, not the backward.  ``kl`` alone is gated
on every shape at ordinary magnitudes (case 1).
"""
import functools
import types

import pytest
import torch

from oracle import gates
from oracle.gpu_support import call_log, classifier_batch, dev, pkg  # noqa: F401

import head_backward_ref as hb

pytestmark = pytest.mark.gpu
NAMES = ("x", "aspect", "logits", "weight", "bias")
REL = 2e-4                                   # tests/test_gpu_backward.py: the gradient gate
BACKWARD, DWEIGHT = "ggcn_scores_head_backward", "ggcn_scores_head_dweight"
ids = lambda s: "x".join(map(str, s))        # noqa: E731


@functools.lru_cache(maxsize=None)
def _inputs(shape, variant="plain"):
    """Seeded inputs on the GPU, made once per (shape, variant) and never modified."""
    t = hb.make_inputs(shape, seed=sum(shape), device="cuda:0")
    if variant == "x30":
        t["x"] = t["x"] * 30.0
    elif variant == "dist_equal":
        t["dist"] = torch.full_like(t["dist"], 2)
    elif variant == "dist_spike":
        t["dist"] = torch.zeros_like(t["dist"])
        t["dist"][:, shape[1] // 2] = 60
    return t


@functools.lru_cache(maxsize=None)
def _reference(shape, which, variant="plain"):
    return hb.autograd64(_inputs(shape, variant), which)


def _fc(t, bias=True):
    C, H2 = t["weight"].shape
    fc = torch.nn.Linear(H2, C, bias=bias).to(t["weight"].device)
    with torch.no_grad():
        fc.weight.copy_(t["weight"])
        if bias:
            fc.bias.copy_(t["bias"])
    return fc


def _run(pkg, t, which, x=None, need=NAMES, strided_gs=False):
    """One forward + backward through ``scores_and_kl``: ``(scores, kl, {name: gradient or None})``."""
    fc = _fc(t)
    fc.weight.requires_grad_("weight" in need)
    fc.bias.requires_grad_("bias" in need)
    leaf = {"x": (t["x"] if x is None else x).detach().requires_grad_("x" in need),
            "aspect": t["aspect"].detach().clone().requires_grad_("aspect" in need),
            "logits": t["logits"].detach().clone().requires_grad_("logits" in need)}
    scores, kl = pkg.scores_and_kl(leaf["x"], leaf["aspect"], leaf["logits"], fc, t["dist"])
    assert scores.grad_fn is not None and kl.grad_fn is not None, "scores_and_kl returned outputs without a grad_fn"
    wanted = [leaf[k] for k in ("x", "aspect", "logits") if k in need] + [p for k, p in (("weight", fc.weight), ("bias", fc.bias)) if k in need]
    if strided_gs:     # the gradients of the loss "both", handed over explicitly: g_s = r with strides (1, B)
        assert which == "both"
        g_s = t["r"].t().contiguous().t()
        assert not g_s.is_contiguous() and torch.equal(g_s, t["r"])
        grads = torch.autograd.grad([scores, kl], wanted, grad_outputs=[g_s, torch.full_like(kl, 3.0)])
    else:
        grads = torch.autograd.grad(hb.loss_of(scores, kl, t["r"], which), wanted)
    return scores.detach(), kl.detach(), dict(zip([k for k in NAMES if k in need], grads))


def _gate_all(got, ref, what, need=NAMES):
    for k in need:
        assert got[k] is not None and got[k].shape == ref["d" + k].shape, (what, k)
        gates.close32(got[k], ref["d" + k], "%s d %s" % (what, k), REL)


# ================================================================ 1. the feature: gradients against float64 autograd
@pytest.mark.parametrize("which", hb.LOSSES)
@pytest.mark.parametrize("shape", hb.SHAPES, ids=ids)
def test_gradients_against_float64_autograd(pkg, dev, shape, which):
    t, ref = _inputs(shape), _reference(shape, which)
    scores, kl, got = _run(pkg, t, which)
    gates.gate(scores, ref["scores"], "scores")
    gates.gate(kl, ref["kl"], "kl")
    _gate_all(got, ref, "%s/%s" % (ids(shape), which))
    assert got["x"].is_contiguous() and got["x"].shape == t["x"].shape and got["x"].dtype == torch.float32


# ================================================================ 2. the forward is today's
@pytest.mark.parametrize("shape", hb.SHAPES, ids=ids)
def test_forward_is_bitwise_the_no_grad_call(pkg, dev, shape):
    t = _inputs(shape)
    fc = _fc(t)
    with torch.no_grad():
        s0, k0 = pkg.scores_and_kl(t["x"], t["aspect"], t["logits"], fc, t["dist"])
    assert s0.grad_fn is None and k0.grad_fn is None
    s1, k1, _ = _run(pkg, t, "both")
    assert torch.equal(s0, s1) and torch.equal(k0, k1)
    for p in fc.parameters():                                    # nothing requires grad: today's path, with grad enabled too
        p.requires_grad_(False)
    s2, k2 = pkg.scores_and_kl(t["x"], t["aspect"], t["logits"], fc, t["dist"])
    assert s2.grad_fn is None and torch.equal(s0, s2) and torch.equal(k0, k2)


# ================================================================ 3. the same bits on every call
@pytest.mark.parametrize("shape", hb.SHAPES, ids=ids)
def test_backward_is_bit_repeatable(pkg, dev, shape):
    t = _inputs(shape)
    _, _, a = _run(pkg, t, "both")
    _, _, b = _run(pkg, t, "both")
    for k in NAMES:
        assert torch.equal(a[k], b[k]), k


# ================================================================ 4. hostile views
HOSTILE = [(3, 7, 64, 5), (9, 31, 256, 34), (5, 9, 30, 3)]


def _padded_x(t, pad=3):
    B, T, H = t["x"].shape
    return gates.hostile(t["x"].reshape(B * T, H), pad)[:B * T, :H].view(B, T, H)      # row stride H + pad; NaN around


def _offset_x(t):
    B, T, H = t["x"].shape
    base = torch.full((B * T * H + 1,), gates.NAN, dtype=torch.float32, device=t["x"].device)
    base[1:] = t["x"].reshape(-1)
    return base[1:].view(B, T, H)                                                      # contiguous, 4 bytes off 16-byte alignment


@pytest.mark.parametrize("view", ["padded", "offset"])
@pytest.mark.parametrize("shape", HOSTILE, ids=ids)
def test_hostile_x_views(pkg, dev, shape, view):
    t, ref = _inputs(shape), _reference(shape, "both")
    x = _padded_x(t) if view == "padded" else _offset_x(t)
    assert (x.stride(1) != shape[2]) if view == "padded" else (x.is_contiguous() and x.data_ptr() % 16 == 4)
    scores, kl, got = _run(pkg, t, "both", x=x)
    gates.gate(scores, ref["scores"], "scores")
    assert all(bool(torch.isfinite(g).all()) for g in got.values())
    _gate_all(got, ref, "%s/%s" % (ids(shape), view))
    assert got["x"].is_contiguous() and got["x"].shape == t["x"].shape


@pytest.mark.parametrize("shape", HOSTILE, ids=ids)
def test_c_call_writes_inside_its_rows_only(pkg, dev, shape):
    from ed_gated_gcn_amd import _capi
    lib, ptr, st = pkg.load_library(), _capi.ptr, _capi.stream_of(dev)
    B, T, H, C = shape
    t, ref = _inputs(shape), _reference(shape, "both")
    x = _padded_x(t).reshape(B * T, H)
    assert x.stride(0) == H + 3
    w, d, gs = t["weight"], t["dist"].float(), t["r"].contiguous()
    gk = torch.full((), 3.0, device=dev)
    scores, part = torch.empty(B, T, device=dev), torch.empty(B, device=dev)
    _capi.check(lib.ggcn_scores_head(ptr(x), x.stride(0), ptr(t["aspect"]), H, ptr(t["logits"]), C, ptr(w), 2 * H, ptr(t["bias"]), ptr(d), T,
                                     B, T, H, C, ptr(scores), T, ptr(part), st), "ggcn_scores_head")
    GUARD, PAD = 64, 3
    bufs = {"dx": gates.poisoned_rows(dev, B * T, H + PAD, GUARD), "da": gates.poisoned_rows(dev, B, H + PAD, GUARD),
            "dlg": gates.poisoned_rows(dev, B, C + PAD, GUARD), "G": gates.poisoned_rows(dev, B, 2 * H + PAD, GUARD)}
    dc0 = torch.empty(B, device=dev)
    _capi.check(lib.ggcn_scores_head_backward(
        ptr(x), x.stride(0), ptr(t["aspect"]), H, ptr(t["logits"]), C, ptr(w), 2 * H, ptr(t["bias"]), ptr(d), T, ptr(scores), T, ptr(part),
        ptr(gs), T, ptr(gk), B, T, H, C, ptr(bufs["dx"][1]), H + PAD, ptr(bufs["da"][1]), H + PAD, ptr(bufs["dlg"][1]), C + PAD,
        ptr(bufs["G"][1]), 2 * H + PAD, ptr(dc0), st), BACKWARD)
    torch.cuda.synchronize()
    for k, width in (("dx", H), ("da", H), ("dlg", C), ("G", 2 * H)):
        whole, view = bufs[k]
        assert bool(torch.isnan(whole[:GUARD]).all()) and bool(torch.isnan(whole[-GUARD:]).all()), "%s: a guard band was written" % k
        assert bool(torch.isnan(view[:, width:]).all()), "%s: padding columns were written" % k
        assert bool(torch.isfinite(view[:, :width]).all()), k
    gates.close32(bufs["dx"][1][:, :H].reshape(B, T, H), ref["dx"], "C call dX", REL)
    gates.close32(bufs["da"][1][:, :H], ref["daspect"], "C call d aspect", REL)
    gates.close32(bufs["dlg"][1][:, :C], ref["dlogits"], "C call d logits", REL)
    gates.close32(t["logits"].t() @ bufs["G"][1][:, :2 * H].contiguous(), ref["dweight"], "C call logits^T . G", REL)
    gates.close32(t["logits"].t() @ dc0, ref["dbias"], "C call logits^T . dc0", REL)


# ================================================================ 5. needs_input_grad
NIG = (9, 31, 256, 34)


def test_detached_x_stores_no_dx(pkg, dev, monkeypatch):
    t, ref = _inputs(NIG), _reference(NIG, "both")
    calls = call_log(monkeypatch, [BACKWARD, DWEIGHT])
    need = ("aspect", "logits", "weight", "bias")
    _, _, got = _run(pkg, t, "both", need=need)
    _gate_all(got, ref, "detached x", need)
    assert [n for n, _ in calls] == [BACKWARD, DWEIGHT]
    args = calls[0][1]
    assert args[0] is not None and args[21] is None, "the launch was handed a dX to store although x needs no gradient"
    assert args[23] is not None and args[25] is not None and args[27] is not None and args[29] is not None


def test_frozen_fc_runs_no_weight_product(pkg, dev, monkeypatch):
    t, ref = _inputs(NIG), _reference(NIG, "both")
    calls = call_log(monkeypatch, [BACKWARD, DWEIGHT])
    need = ("x", "aspect", "logits")
    _, _, got = _run(pkg, t, "both", need=need)
    _gate_all(got, ref, "frozen fc", need)
    assert [n for n, _ in calls] == [BACKWARD]
    assert calls[0][1][21] is not None and calls[0][1][27] is None and calls[0][1][29] is None


def test_one_output_unused_hands_the_launch_a_null(pkg, dev, monkeypatch):
    t = _inputs(NIG)
    calls = call_log(monkeypatch, [BACKWARD])
    _run(pkg, t, "scores")
    _run(pkg, t, "kl")
    _run(pkg, t, "both")
    (s, k, b) = (c[1] for c in calls)
    assert s[14] is not None and s[16] is None           # g_scores, g_kl
    assert k[14] is None and k[16] is not None
    assert b[14] is not None and b[16] is not None


def test_integer_dist_gets_no_gradient(pkg, dev):
    t = _inputs(NIG)
    assert t["dist"].dtype == torch.int64
    fc = _fc(t)
    x = t["x"].detach().requires_grad_()
    scores, kl = pkg.scores_and_kl(x, t["aspect"], t["logits"], fc, t["dist"])
    (scores.sum() + kl).backward()
    assert x.grad is not None and t["dist"].grad is None and not t["dist"].requires_grad
    d = t["dist"].float().requires_grad_()               # a float dist that asks for one gets none either
    scores, kl = pkg.scores_and_kl(x, t["aspect"], t["logits"], fc, d)
    kl.backward()
    assert d.grad is None


# ================================================================ 6. extremes
@pytest.mark.parametrize("variant", ["x30", "dist_equal", "dist_spike"])
@pytest.mark.parametrize("shape", [(9, 31, 256, 34), (2, 100, 96, 12)], ids=ids)
def test_extremes(pkg, dev, shape, variant):
    t, ref = _inputs(shape, variant), _reference(shape, "both", variant)
    if variant == "x30":
        assert float(ref["scores"].abs().max()) > 100.0, "x * 30 was meant to give scores in the hundreds"
        assert float(torch.softmax(ref["scores"], 1).max(1)[0].mean()) > 0.9, "the softmax was meant to be saturated"
    scores, kl, got = _run(pkg, t, "both")
    assert not any(bool(torch.isnan(v).any()) for v in (scores, kl) + tuple(got.values()))
    gates.gate(scores, ref["scores"], "scores")
    gates.gate(kl, ref["kl"], "kl")
    _gate_all(got, ref, "%s/%s" % (ids(shape), variant))


# ================================================================ 7. a strided incoming gradient
@pytest.mark.parametrize("shape", [(3, 7, 64, 5), (2, 65, 96, 12)], ids=ids)
def test_strided_incoming_gradient(pkg, dev, shape, monkeypatch):
    t = _inputs(shape)
    seen = []
    from ed_gated_gcn_amd import heads
    orig = heads._ScoresAndKl.backward

    def spy(ctx, g_scores, g_kl):
        seen.append(g_scores.is_contiguous())
        return orig(ctx, g_scores, g_kl)
    monkeypatch.setattr(heads._ScoresAndKl, "backward", staticmethod(spy))
    _, _, a = _run(pkg, t, "both")
    _, _, b = _run(pkg, t, "both", strided_gs=True)
    assert seen == [True, False], "the second gradient was meant to arrive strided: %s" % seen
    for k in NAMES:
        assert torch.equal(a[k], b[k]), k


# ================================================================ 8. the classifier with the option on
class _Bert(torch.nn.Module):
    """The stand-in BERT of the classifier tests: twelve seeded [B,L,768] layers, a zero pooled output."""

    def forward(self, ids_, seg, output_all_encoded_layers=True):
        gen = torch.Generator(device=ids_.device).manual_seed(1)
        return ([torch.randn(ids_.shape[0], ids_.shape[1], 768, device=ids_.device, generator=gen) for _ in range(12)],
                torch.zeros(ids_.shape[0], 768, device=ids_.device))


def _training_step(pkg, dev, cls_name, inputs, ncls, head_backward):
    opt = types.SimpleNamespace(dropout=0.0, polarities_dim=ncls, device=dev, ggcn_head_backward=head_backward)
    m = getattr(pkg, cls_name)(_Bert(), opt)
    assert m.head_backward is head_backward
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
    grads = {n: p.grad for n, p in m.named_parameters() if n.split(".")[0] in ("fc", "dense", "gc1", "gc2", "gate1", "gate2")}
    return (logits.detach(), xy.detach(), kl.detach(), scores.detach()), grads


@pytest.mark.parametrize("cls_name", ["GatedGCNEventDetector", "GatedGCNEventDetector54"])
def test_classifier_training_step_with_the_option(pkg, dev, cls_name, monkeypatch):
    monkeypatch.delenv("GGCN_HEAD_BACKWARD", raising=False)
    inputs, ncls = classifier_batch(dev)
    calls = call_log(monkeypatch, ["ggcn_scores_head", BACKWARD])
    out_off, g_off = _training_step(pkg, dev, cls_name, inputs, ncls, False)
    assert calls == [], "the option is off: the head is the reference's PyTorch ops"
    out_on, g_on = _training_step(pkg, dev, cls_name, inputs, ncls, True)
    assert [n for n, _ in calls] == ["ggcn_scores_head", BACKWARD]
    for got, ref, what in zip(out_on, out_off, ("logits", "xy", "kl", "scores")):
        gates.gate(got, ref, "%s %s" % (cls_name, what))
    assert sorted(g_on) == sorted(g_off) and len(g_on) >= 12
    for n in sorted(g_on):
        assert g_on[n] is not None and g_off[n] is not None, n
        gates.close32(g_on[n], g_off[n], "%s d %s" % (cls_name, n), REL)
