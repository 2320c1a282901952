"""THE STATEMENT OF ``ggcn_anchor_pool_layers`` IN NUMPY AND THE CASES ITS TESTS SHARE (test infrastructure, NOT product code).

``statement`` is the header's text on pooled words ``v [B, R, W]`` that already exist (float32 values; for bfloat16 layers the
values rounded to bfloat16): the anchor word's row, and with ``sides`` the two maxima over ``v + 1`` with their ``1.0f`` floors,
minus one.  ``formula_torch`` is the arithmetic of ``models/bertdm.py`` on the same ``v`` with torch CPU ops -- multiply by a 0/1 mask, add
one, max over the words, subtract one, select the anchor's row -- in broadcast form, for ``torch.equal`` against the statement.  ``emulate_float32`` pools in the kernel's order (ascending column, zeros skipped, float32 products and sums) and
``ref64_and_bound`` gives the float64 reference with the per-element margin the GPU test holds against it.  ``CASES`` names every shape and edge the C-entry
test runs.  numpy and torch on CPU tensors only: nothing here calls the library.
"""
from collections import namedtuple

import numpy as np
import torch

from oracle import subword_pool_cases as sc

ONE = np.float32(1.0)
U32 = 2.0 ** -24


def clamp(anchor, length, R):
    a = np.clip(np.asarray(anchor, dtype=np.int64), 0, R - 1)
    n = None if length is None else np.clip(np.asarray(length, dtype=np.int64), 0, R)
    return a, n


def statement(v, anchor, length=None, sides=True):
    """float32 numpy ``[B, (3 or 1) * W]`` from ``v [B, R, W]`` float32, ``anchor`` / ``length`` integer ``[B]`` (clamped here as
    the entry clamps them).  Rows that the statement masks are never read (a NaN there does not show); a NaN in a row that is
    pooled propagates (``np.max`` keeps it, like ``torch.max``)."""
    v = np.asarray(v, dtype=np.float32)
    B, R, W = v.shape
    a, n = clamp(anchor, length if sides else None, R)
    z = np.empty((B, (3 if sides else 1) * W), dtype=np.float32)
    for b in range(B):
        ab = int(a[b])
        z[b, :W] = v[b, ab]
        if not sides:
            continue
        nb = int(n[b])
        with np.errstate(invalid="ignore"):
            left = (v[b, :ab + 1] + ONE).max(axis=0)
            if ab < R - 1:
                left = np.maximum(np.float32(1.0), left)
            right = np.full(W, 1.0, dtype=np.float32)
            if nb > ab + 1:
                right = np.maximum(right, (v[b, ab + 1:nb] + ONE).max(axis=0))
            z[b, W:2 * W] = left - ONE
            z[b, 2 * W:] = right - ONE
    return z


def formula_torch(v, anchor, length):
    """The arithmetic the issue names, with torch CPU ops on ``v [B, T, W]`` (float32 or bfloat16), ``anchor`` and ``length``
    int64 ``[B]`` in range: multiply by a 0/1 float32 mask (which promotes a bfloat16 ``v``), add one, take the max over the
    words, subtract one; the anchor's row by index.  ``[B, 3 * W]`` float32 = (anchor row, left, right)."""
    B, T, W = v.shape
    word = torch.arange(T)[None, :]                                           # [1, T]
    keep_left = (word <= anchor[:, None]).to(torch.float32)                    # words up to and including the anchor
    keep_right = ((word > anchor[:, None]) & (word < length[:, None])).to(torch.float32)     # after it, inside the sentence
    sides = [(v * keep[:, :, None] + 1.0).amax(dim=1) - 1.0 for keep in (keep_left, keep_right)]
    row = v[torch.arange(B), anchor].to(torch.float32)
    return torch.cat([row] + sides, dim=1)


def emulate_float32(a, layers, bf16):
    """The pooled words as a float32 machine forms them in the kernel's order, ``[B, R, n * Dl]`` float32 numpy; ``bf16``: rounded
    to bfloat16 once (numpy rounds the products too: one more rounding per term than an fmaf, inside the same bound)."""
    cat = torch.cat([x.float() for x in layers], dim=-1)
    v = torch.from_numpy(sc.ascending_float32(a, cat))
    return (v.bfloat16().float() if bf16 else v).numpy()


def ref64_and_bound(a, layers, anchor, length, bf16):
    """``(ref, bound)``, float64 numpy ``[B, 3 * W]``: float64 pooling + the formula in float64, and per element
    ``bound_pool + 2^-24 (|ref + 1| + |ref|)``.  ``bound_pool`` is the derived bound of ``oracle/subword_pool_cases.py`` on the
    pooled words -- for the anchor part the anchor's row, for a side the largest bound among the rows of that side (a max moves
    by no more than its arguments do; the floor 1.0 does not move) -- and the second term pays for the two roundings, of
    ``v + 1`` and of ``m - 1`` (the anchor part has neither and gets the same allowance, for one rule)."""
    cat = torch.cat([x for x in layers], dim=-1)
    # a NaN feature belongs to the words whose row of `a` is non-zero at its sub-word, and to no other (a dense product would
    # spread it through 0 * NaN): pool with zeros in its place, then mark those words
    nan_x = torch.isnan(cat)
    hit = (((a != 0).double() @ nan_x.double()) > 0).numpy()
    cat = torch.where(nan_x, torch.zeros_like(cat), cat)
    v = sc.ref64(a, cat).numpy()
    pb = sc.bound(a, cat, bf16=bf16).numpy()
    v[hit], pb[hit] = np.nan, 0.0
    B, R, W = v.shape
    an, n = clamp(anchor, length, R)
    ref, bound = np.empty((B, 3 * W)), np.empty((B, 3 * W))
    for b in range(B):
        ab, nb = int(an[b]), int(n[b])
        ref[b, :W], bound[b, :W] = v[b, ab], pb[b, ab]
        with np.errstate(invalid="ignore"):
            left = (v[b, :ab + 1] + 1.0).max(axis=0)
            if ab < R - 1:
                left = np.maximum(1.0, left)
            ref[b, W:2 * W], bound[b, W:2 * W] = left - 1.0, pb[b, :ab + 1].max(axis=0)
            right, rb = np.ones(W), np.zeros(W)
            if nb > ab + 1:
                right, rb = np.maximum(1.0, (v[b, ab + 1:nb] + 1.0).max(axis=0)), pb[b, ab + 1:nb].max(axis=0)
            ref[b, 2 * W:], bound[b, 2 * W:] = right - 1.0, rb
    with np.errstate(invalid="ignore"):
        bound = bound + U32 * (np.abs(ref + 1.0) + np.abs(ref))
    return ref, bound


def assert_within(got, ref, bound, what=""):
    """``got`` (numpy) inside ``bound`` of ``ref`` wherever ``ref`` is a number, NaN exactly where ``ref`` is NaN."""
    got = np.asarray(got, dtype=np.float64)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), "%s: NaN in %d places, the reference in %d" % (what, int(np.isnan(got).sum()), int(nan.sum()))
    err = np.where(nan, 0.0, np.abs(got - np.where(nan, 0.0, ref)))
    lim = np.where(nan, 1.0, bound)
    ratio = float((err / np.maximum(lim, 1e-300)).max())
    print("  %s: max err / bound %.3f (max err %.3g)" % (what, ratio, float(err.max())))
    assert not (err > lim).any(), "%s: %d elements outside the bound, the worst %.3f times it" % (what, int((err > lim).sum()), ratio)


# ------------------------------------------------------------------------------------------------------------------ the cases
# name; Dl, n; the launch form; B, T (= R), L (= C); what is special: "anchor" / "length" per sentence (None: the default mix),
# "values" ("normal" | "negative" | "tiny" | "nan"), "layout" (dict for the layers: shift / ldx / x_gap), "strided" transform,
# "empty_word" (a word without sub-words).
Case = namedtuple("Case", "name Dl n vector B T L anchor length values layout strided")


def _case(name, Dl, n, vector, B=3, T=5, L=9, anchor=None, length=None, values="normal", layout=None, strided=False):
    return Case(name, Dl, n, vector, B, T, L, anchor, length, values, dict(layout or {}), strided)


def _cases():
    c = []
    for Dl, n, vec in ((768, 12, True), (260, 3, True), (4, 1, True), (5, 2, False), (1025, 1, False), (8, 16, True)):
        c.append(_case("shape-%dx%d" % (Dl, n), Dl, n, vec))
    c.append(_case("scalar-by-one-shifted-layer", 768, 12, False, layout=dict(shift=5)))
    c.append(_case("vector-padded-rows-and-batch-gap", 768, 12, True, layout=dict(ldx=772, x_gap=8)))
    c.append(_case("scalar-padded-rows-and-batch-gap", 260, 3, False, layout=dict(ldx=261, x_gap=3)))
    c.append(_case("anchor-first", 260, 3, True, anchor=[0, 0, 0], length=[5, 1, 3]))
    c.append(_case("anchor-last", 260, 3, True, anchor=[4, 4, 4], length=[5, 5, 2]))
    c.append(_case("right-side-empty", 260, 3, True, anchor=[0, 2, 4], length=[1, 3, 5]))
    c.append(_case("length-full", 260, 3, True, anchor=[0, 2, 3], length=[5, 5, 5]))
    c.append(_case("one-word", 260, 3, True, T=1, anchor=[0, 0, 0], length=[1, 1, 1]))
    c.append(_case("all-negative", 260, 3, True, values="negative"))
    c.append(_case("tiny-values", 260, 3, True, values="tiny"))
    c.append(_case("nan-in-a-pooled-row", 260, 3, True, values="nan", anchor=[1, 3, 0], length=[5, 5, 5]))
    c.append(_case("columns-255", 8, 3, True, L=255))
    c.append(_case("columns-257", 5, 2, False, L=257))
    c.append(_case("strided-transform", 768, 12, True, strided=True))
    c.append(_case("out-of-range", 260, 3, True, anchor=[-7, 99, 2], length=[-1, 3, 1 << 40]))
    return tuple(c)


CASES = _cases()
CASE_IDS = tuple(c.name for c in CASES)
EMPTY_WORD = 1          # row of the transform without a non-zero, in every sentence (T > 1)


def build(case, dtype):
    """``(a, vals, anchor, length)`` of a case on the CPU, the same on every call: ``a`` [B, T, L] float32 (word ``EMPTY_WORD``
    without sub-words; ``strided``: the reference's slice of a padded buffer filled with junk), ``vals`` [n, B, L, Dl] in
    ``dtype``, ``anchor`` and ``length`` int64 [B]."""
    rng = np.random.default_rng(sum(case.name.encode()) * 7919 + case.Dl)
    B, T, L = case.B, case.T, case.L
    m = sc.dense_transform(B, T, L, 0.5, rng, scale=sc.value_scale(L), empty=(EMPTY_WORD,) if T > 1 else ())
    if case.strided:
        buf = torch.full((B, T + 3, L + 5), sc.JUNK)
        a = buf[:, :T, :L]
        a.copy_(torch.from_numpy(m))
    else:
        a = torch.from_numpy(m)
    x = rng.standard_normal((case.n, B, L, case.Dl)).astype(np.float32)
    if case.values == "negative":
        # every pooled value negative: positive weights only, negative features -- the 1.0f floor decides both sides
        a = a.abs() if not case.strided else a
        x = -np.abs(x) - np.float32(0.5)
    elif case.values == "tiny":
        x = x * np.float32(1e-9)                              # v + 1 rounds to 1: the sides come out as exact zeros
    elif case.values == "nan":
        x[:, :, 3, ::7] = np.nan                              # sub-word 3 of every sentence, every seventh feature
        a = a.clone()
        a[:, 2, 3] = 0.5                                      # ... pooled into word 2, and into no other word
        a[:, :2, 3] = 0.0
        a[:, 3:, 3] = 0.0
    vals = torch.from_numpy(x).to(dtype)
    anchor = torch.tensor(case.anchor if case.anchor is not None else [(b * 2 + 1) % T for b in range(B)], dtype=torch.int64)
    length = torch.tensor(case.length if case.length is not None else [max(1, T - b) for b in range(B)], dtype=torch.int64)
    return a, vals, anchor, length
