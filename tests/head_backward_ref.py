"""The scores / kl head (``models/bert_amir5.py:645-648``) twice, as plain torch (a helper of the tests, NOT a test file):

* ``literal`` -- the reference's own ops (``cat``, ``fc``, multiply, sum, two softmaxes, mean) in a given dtype;
* ``statement64`` -- the float64 statement of the factored forward and of the backward formulas that
  ``ggcn_scores_head_backward`` and ``ggcn_scores_head_dweight`` implement (``include/ggcn.h``).

``autograd64`` runs float64 autograd through ``literal`` on float32 inputs: the reference of every gradient test.
"""
import torch

# (B, T, H, C): the smallest shapes at which each part of the backward can go wrong
SHAPES = [
    (1, 1, 8, 2),        # one sentence, one token
    (3, 7, 64, 5),       # fewer tokens than two rounds of the four wavefronts
    (9, 31, 256, 34),    # the model's own widths
    (2, 65, 96, 12),     # the softmax lanes loop: one token past 64
    (2, 100, 96, 12),    # ... and well past it
    (5, 9, 30, 3),       # H % 4 != 0: the scalar form
    (300, 4, 64, 34),    # the sum over B crosses the weight product's slices of 128 sentences (twice)
]
LOSSES = ("scores", "kl", "both")


def make_inputs(shape, seed, device="cpu", dtype=torch.float32):
    """Seeded ``dict(x, aspect, logits, weight, bias, dist, r)``: ``dist`` the integer distances of the data loader, ``r`` the
    random weights of a loss on ``scores``."""
    B, T, H, C = shape
    g = torch.Generator().manual_seed(seed)
    t = {
        "x": torch.randn(B, T, H, generator=g),
        "aspect": torch.randn(B, H, generator=g),
        "logits": torch.randn(B, C, generator=g),
        "weight": torch.randn(C, 2 * H, generator=g) / (2 * H) ** 0.5,
        "bias": torch.randn(C, generator=g) * 0.1,
        "r": torch.randn(B, T, generator=g),
    }
    t = {k: v.to(dtype).to(device) for k, v in t.items()}
    t["dist"] = torch.randint(0, 6, (B, T), generator=g).to(device)
    return t


def literal(x, aspect, logits, weight, bias, dist, dtype=None):
    """``bert_amir5.py:645-648`` as written there: ``(scores [B,T], kl)`` in ``dtype`` (None: the operands' own)."""
    if dtype is not None:
        x, aspect, logits, weight = (t.to(dtype) for t in (x, aspect, logits, weight))
        bias = None if bias is None else bias.to(dtype)
    T = x.shape[1]
    output_w = torch.nn.functional.linear(torch.cat([x, aspect[:, None, :].expand(-1, T, -1)], dim=2), weight, bias)   # :645
    scores = (logits[:, None, :] * output_w).sum(2)                                                                   # :646
    dist = dist.float() if dtype is None else dist.to(dtype)
    kl = (torch.softmax(scores, 1) * torch.softmax(dist, 1)).sum(1).mean()                                             # :648
    return scores, kl


def loss_of(scores, kl, r, which):
    """The three losses of the tests: ``scores`` only (random ``g_s`` = r), ``kl`` only, ``(scores * r).sum() + 3 kl``."""
    r = r.to(scores.dtype)
    return {"scores": lambda: (scores * r).sum(), "kl": lambda: kl, "both": lambda: (scores * r).sum() + 3 * kl}[which]()


def incoming(r, which):
    """``(g_s, g_k)`` of ``loss_of`` in float64 (None: absent)."""
    r = r.double()
    return {"scores": (r, None), "kl": (None, r.new_tensor(1.0)), "both": (r, r.new_tensor(3.0))}[which]


def autograd64(t, which, need=("x", "aspect", "logits", "weight", "bias")):
    """float64 autograd through ``literal`` on the (float32) inputs ``t``: ``dict(scores, kl, d<name> for name in need)``."""
    leaf = {k: t[k].detach().double().requires_grad_(k in need) for k in ("x", "aspect", "logits", "weight", "bias")}
    scores, kl = literal(leaf["x"], leaf["aspect"], leaf["logits"], leaf["weight"], leaf["bias"], t["dist"], dtype=torch.float64)
    loss_of(scores, kl, t["r"], which).backward()
    out = {"scores": scores.detach(), "kl": kl.detach()}
    out.update({"d" + k: leaf[k].grad for k in need})
    return out


def statement64(x, aspect, logits, weight, bias, dist, g_s=None, g_k=None):
    """float64 statement of the factored head and its backward: ``dict(scores, kl, kl_b, dx, daspect, dlogits, dweight, dbias,
    G, dc0)``.  ``g_s`` [B,T] / ``g_k`` scalar: the incoming gradients (None: that term is zero)."""
    x, a, lg, w = x.double(), aspect.double(), logits.double(), weight.double()
    B, T, H = x.shape
    fb = torch.zeros(w.shape[0], dtype=torch.float64, device=x.device) if bias is None else bias.double()
    wx, wa = w[:, :H], w[:, H:]
    v = lg @ wx                                   # [B,H]   v_b = Wx^T . lg_b
    u = a @ wa.t() + fb                           # [B,C]   u_b = Wa . a_b + fb
    c0 = (lg * u).sum(1)                          # [B]
    scores = torch.einsum("bth,bh->bt", x, v) + c0[:, None]
    p, q = torch.softmax(scores, 1), torch.softmax(dist.double(), 1)
    kl_b = (p * q).sum(1)
    ds = torch.zeros_like(scores)
    if g_s is not None:
        ds = ds + g_s.double()
    if g_k is not None:
        ds = ds + (g_k.double() / B) * p * (q - kl_b[:, None])
    dv = torch.einsum("bt,bth->bh", ds, x)
    dc0 = ds.sum(1)
    G = torch.cat([dv, dc0[:, None] * a], dim=1)  # [B,2H]
    return {
        "scores": scores, "kl": kl_b.mean(), "kl_b": kl_b,
        "dx": ds[:, :, None] * v[:, None, :],
        "dlogits": dv @ wx.t() + dc0[:, None] * u,
        "daspect": dc0[:, None] * (lg @ wa),
        "dweight": lg.t() @ G,
        "dbias": lg.t() @ dc0,
        "G": G, "dc0": dc0,
    }
