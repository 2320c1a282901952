"""The two gate MLPs (``models/bert_amir5.py:562-571``) twice, as plain torch (a helper of the tests, NOT a test file):

* ``literal`` -- the ``nn.Sequential`` ops (Sigmoid, Linear, Sigmoid, Linear, Sigmoid) in a given dtype;
* ``statement64`` -- the float64 statement of the forward and of the backward formulas that ``ggcn_gate_mlp_backward`` and the
  weight products on its ``Z`` output implement (``include/ggcn.h``).

``autograd64`` runs float64 autograd through ``literal`` on float32 inputs: the reference of every gradient test.
"""
import torch

# (B, H): the smallest shapes at which each part of the backward can go wrong
SHAPES = [
    (1, 8),          # one sentence
    (3, 64),         # fewer columns than threads
    (9, 256),        # the model's own width; one full workgroup plus one row
    (17, 30),        # H % 4 != 0 (the scalar form, padded Z groups); two full workgroups plus one row
    (5, 300),        # the columns loop twice, the second round partial
    (2, 768),        # three full rounds of columns
    (300, 64),       # the sum over B crosses the weight product's row chunks
    (5, 1024),       # the LDS bound: 64 KiB exactly
]
LOSSES = ("g1", "g2", "both")
PARAMS = tuple("%s_%s" % (p, g) for g in "ab" for p in ("w1", "b1", "w2", "b2"))     # gate A's four, then gate B's
NAMES = ("aspect",) + PARAMS


def make_inputs(shape, seed, device="cpu"):
    """Seeded float32 ``dict(aspect, w1_a, b1_a, w2_a, b2_a, w1_b, ..., r1, r2)``: weights ``[out,in]`` as nn.Linear keeps them,
    ``r1`` / ``r2`` the random weights of a loss on each gate."""
    B, H = shape
    g = torch.Generator().manual_seed(seed)
    t = {"aspect": torch.randn(B, H, generator=g)}
    for gate in "ab":
        t["w1_" + gate] = torch.randn(H, H, generator=g) / H ** 0.5
        t["b1_" + gate] = torch.randn(H, generator=g) * 0.1
        t["w2_" + gate] = torch.randn(H, H, generator=g) / H ** 0.5
        t["b2_" + gate] = torch.randn(H, generator=g) * 0.1
    t["r1"] = torch.randn(B, H, generator=g)
    t["r2"] = torch.randn(B, H, generator=g)
    return {k: v.to(device) for k, v in t.items()}


def literal(aspect, w1, b1, w2, b2, dtype=None):
    """One gate as ``bert_amir5.py:562-566`` writes it: ``Sigmoid(Linear(Sigmoid(Linear(Sigmoid(aspect)))))`` in ``dtype``."""
    if dtype is not None:
        aspect, w1, b1, w2, b2 = (None if v is None else v.to(dtype) for v in (aspect, w1, b1, w2, b2))
    lin = torch.nn.functional.linear
    return torch.sigmoid(lin(torch.sigmoid(lin(torch.sigmoid(aspect), w1, b1)), w2, b2))


def loss_of(g1, g2, r1, r2, which):
    """The three losses of the tests: ``(g1 * r1).sum()``, ``(g2 * r2).sum()`` and their sum."""
    r1, r2 = r1.to(g1.dtype), r2.to(g2.dtype)
    return {"g1": lambda: (g1 * r1).sum(), "g2": lambda: (g2 * r2).sum(), "both": lambda: (g1 * r1).sum() + (g2 * r2).sum()}[which]()


def incoming(r1, r2, which):
    """``(dG_A, dG_B)`` of ``loss_of`` in float64 (None: no gradient reaches that gate)."""
    return {"g1": (r1.double(), None), "g2": (None, r2.double()), "both": (r1.double(), r2.double())}[which]


def autograd64(t, which):
    """float64 autograd through ``literal`` on the (float32) inputs ``t``: ``dict(g1, g2, d<name> for name in NAMES)``; a
    parameter the loss does not reach gets zeros."""
    leaf = {k: t[k].detach().double().requires_grad_() for k in NAMES}
    g1 = literal(leaf["aspect"], *(leaf[p + "_a"] for p in ("w1", "b1", "w2", "b2")))
    g2 = literal(leaf["aspect"], *(leaf[p + "_b"] for p in ("w1", "b1", "w2", "b2")))
    loss_of(g1, g2, t["r1"], t["r2"], which).backward()
    out = {"g1": g1.detach(), "g2": g2.detach()}
    out.update({"d" + k: (torch.zeros_like(leaf[k]) if leaf[k].grad is None else leaf[k].grad) for k in NAMES})
    return out


def statement64(t, dg_a, dg_b):
    """float64 statement of section "the gate MLPs under autograd" of ``include/ggcn.h``: ``dict(g1, g2, daspect, d<param>, Z)``
    with ``Z = [dz1_A | dz1_B | dz2_A | dz2_B | s]`` (unpadded groups); ``dg_*`` None: that gate contributes nothing."""
    a = t["aspect"].double()
    s = torch.sigmoid(a)
    ds_sum = torch.zeros_like(a)
    out, groups = {}, {}
    for gate, name, dg in (("a", "g1", dg_a), ("b", "g2", dg_b)):
        w1, b1, w2, b2 = (t["%s_%s" % (p, gate)].double() for p in ("w1", "b1", "w2", "b2"))
        h = torch.sigmoid(s @ w1.t() + b1)
        g = torch.sigmoid(h @ w2.t() + b2)
        out[name] = g
        if dg is None:
            dz1 = dz2 = torch.zeros_like(a)
        else:
            dz2 = dg.double() * g * (1 - g)
            dz1 = (dz2 @ w2) * h * (1 - h)
            ds_sum = ds_sum + dz1 @ w1            # gate A first, then gate B
        groups[gate] = (dz1, dz2)
        out["dw2_" + gate], out["dw1_" + gate] = dz2.t() @ h, dz1.t() @ s
        out["db2_" + gate], out["db1_" + gate] = dz2.sum(0), dz1.sum(0)
    out["daspect"] = ds_sum * s * (1 - s)
    out["Z"] = torch.cat([groups["a"][0], groups["b"][0], groups["a"][1], groups["b"][1], s], dim=1)
    return out
