"""THE FLOAT64 STATEMENT OF THE FORWARD CSR AGGREGATION AND ITS ERROR BOUND (test infrastructure, NOT product code).

Written from the formula in ``include/ggcn.h`` (the comment above ``ggcn_aggregate``), not from the kernel.  numpy only.

For row i of graph g, over the entries e of the row (duplicates and unsorted columns included: the formula is a sum over e)::

    S    = sum_e w_e * h[col_e]            A    = sum_e |w_e| * |h[col_e]|
    den  = sum_e w_e + 1                   dabs = sum_e |w_e| + 1
    y    = S / den + bias                  out  = y * store_gate[g]
    pool_x[g] = max over the T rows of y * gate_x[g]

``vals = None`` is the 0/1 adjacency (w_e = 1); an absent bias is 0, an absent gate is 1.

THE BOUND.  What an fp32 evaluation of the above may differ by from the float64 one, whatever the order of its sums, to first
order in u = 2^-24 (round to nearest, a fused multiply-add rounds once).  n = the row's number of entries.

* The sum S: n products added in any order or grouping (one after the other, in pairs, in partial sums that are added at the
  end).  Every term passes through at most n roundings on its way into the result -- its own multiply-add and the later ones
  of its chain; a tree of partial sums is shallower than the chain -- and each rounding of a partial sum is relative to the
  terms that partial sum holds, so the roundings a term meets are charged to it: |S32 - S| <= n u A.
* The denominator, by the same count: at most n - 1 roundings for the weights and one for the + 1, charged to terms whose
  magnitudes add up to dabs: |den32 - den| <= n u dabs.  Its reciprocal rounds once more, so 1/den is off by
  (n + 1) u dabs / |den| of itself; the term below carries n + 3, two to spare.
* S32 * inv32 rounds once: with the reciprocal's own rounding that is (n + 2) u A / |den| on the side of the sum and
  (n + 3) u |S| / |den| * dabs / |den| on the side of the denominator.
* + bias rounds once, relative to |y|; the bound carries 2 u |y|: the second is what the gate multiply of a pool spends.

::

    bound_y   = u * ( (n + 2) * A / |den|  +  (n + 3) * |S| / |den| * dabs / |den|  +  2 * |y| )
    bound_out = bound_y * |store_gate| + u * |out|                    (the gate multiply rounds once)
    bound_pool_x[g] = max over the rows of bound_y * |gate_x[g]|      (max is 1-Lipschitz in the sup norm)

An output stored as IEEE half adds one round-to-nearest: ``2^-11 * |out| + 2^-25`` (half an ulp of a normal number, and half the
subnormal spacing 2^-24); the pools of the half entry are fp32 and get no such term.  The tests use these bounds with no extra
factor and no absolute floor.  With exact sums (small integers times powers of two) the n-terms vanish and what is left is the
reciprocal, the multiply, the bias add and the gate: ``exact_bound`` = 4 u |ref| (plus the half term).
"""
import numpy as np

U32 = 2.0 ** -24
U16 = 2.0 ** -11
HALF_SUBNORMAL = 2.0 ** -25


def row_sums(h, rowptr, colidx, vals):
    """float64 (S [N,F], A [N,F], den [N], dabs [N], n [N]) of the rows of a CSR over h [N,F]."""
    h = np.asarray(h, dtype=np.float64)
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colidx = np.asarray(colidx, dtype=np.int64)
    N, F = h.shape
    assert rowptr.shape == (N + 1,) and rowptr[0] == 0 and rowptr[-1] == len(colidx) and np.all(np.diff(rowptr) >= 0)
    n = np.diff(rowptr)
    w = np.ones(len(colidx)) if vals is None else np.asarray(vals, dtype=np.float64)
    assert w.shape == colidx.shape
    S, A = np.zeros((N, F)), np.zeros((N, F))
    wsum, wabs = np.zeros(N), np.zeros(N)
    rows = np.flatnonzero(n)
    if len(rows):
        # the entries of a row are contiguous and rows without entries own none: the segments that start at the first entry of
        # each non-empty row are exactly the rows
        starts = rowptr[rows]
        g = h[colidx]
        S[rows] = np.add.reduceat(w[:, None] * g, starts, axis=0)
        A[rows] = np.add.reduceat(np.abs(w)[:, None] * np.abs(g), starts, axis=0)
        wsum[rows] = np.add.reduceat(w, starts)
        wabs[rows] = np.add.reduceat(np.abs(w), starts)
    return S, A, wsum + 1.0, wabs + 1.0, n.astype(np.float64)


def aggregate_ref(h, rowptr, colidx, vals, bias, B, T, store_gate=None, gate_a=None, gate_b=None, half_out=False):
    """h [B*T,F]: the exact values the kernel is given (float32, or fp16 widened); rowptr [B*T+1], colidx global node ids;
    vals None or [nnz]; bias None or [F]; gates None or [B,F].  Returns a dict of float64 arrays: ``y``, ``out`` [B*T,F],
    ``pool_a``, ``pool_b`` [B,F] and the bounds ``bound_y``, ``bound_out``, ``bound_pool_a``, ``bound_pool_b`` of the module's
    docstring (``half_out``: ``bound_out`` with the half rounding of the stored value)."""
    S, A, den, dabs, n = row_sums(h, rowptr, colidx, vals)
    N, F = S.shape
    assert N == B * T
    assert np.all(den != 0.0), "a row whose weights sum to -1 has no value"
    ad = np.abs(den)[:, None]
    y = S / den[:, None] + (0.0 if bias is None else np.asarray(bias, dtype=np.float64)[None, :])
    bound_y = U32 * ((n[:, None] + 2.0) * A / ad + (n[:, None] + 3.0) * np.abs(S) / ad * dabs[:, None] / ad + 2.0 * np.abs(y))

    def per_row(g):
        return np.ones((N, F)) if g is None else np.repeat(np.asarray(g, dtype=np.float64).reshape(B, F), T, axis=0)

    sg = per_row(store_gate)
    out = y * sg
    bound_out = bound_y * np.abs(sg) + U32 * np.abs(out)
    if half_out:
        bound_out = bound_out + U16 * np.abs(out) + HALF_SUBNORMAL
    r = {"y": y, "bound_y": bound_y, "out": out, "bound_out": bound_out}
    for key, g in (("pool_a", gate_a), ("pool_b", gate_b)):
        gg = per_row(g)
        r[key] = (y * gg).reshape(B, T, F).max(axis=1)
        r["bound_" + key] = (bound_y * np.abs(gg)).reshape(B, T, F).max(axis=1)
    return r


def exact_bound(ref, half_out=False):
    """The gate of ``out`` in a case whose fp32 sums are exact and that has no bias (a bias that cancels S / den would leave the
    reciprocal's and the multiply's roundings above |y|): 4 u |ref| -- reciprocal, multiply, gate and one to spare -- plus the
    half rounding for a half output.  The pools of such a case take ``exact_pool_bound``."""
    b = 4.0 * U32 * np.abs(ref)
    return b + U16 * np.abs(ref) + HALF_SUBNORMAL if half_out else b


def exact_pool_bound(y, gate, B, T):
    """max over a graph's rows of 4 u |y * gate| (max is 1-Lipschitz): the pool's gate in an exact case."""
    N, F = y.shape
    g = np.ones((N, F)) if gate is None else np.repeat(np.asarray(gate, dtype=np.float64).reshape(B, F), T, axis=0)
    return (4.0 * U32 * np.abs(y * g)).reshape(B, T, F).max(axis=1)
