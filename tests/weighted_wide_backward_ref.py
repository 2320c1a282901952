"""WHAT THE TWO TEST FILES OF THE ONE-LAUNCH BACKWARD ON REAL-VALUED ADJACENCIES OF 33..128 NODES SHARE (test infrastructure, NOT
product code).

``tests/test_weighted_wide_backward_cpu.py`` (no GPU) and ``tests/test_gpu_weighted_wide_backward.py`` run the same cases: the case
lists and their CPU inputs, the numpy statement of the operand of ``ggcn_graph_operands_weighted_wide_t`` (bit for bit), a numpy
emulation of the arithmetic of ``csrc/gate_pool_backward_weighted_wide.hip`` and the elementwise bounds both files hold results
to.  The float64 reference is ``oracle/gates.gate_pool_backward_statement64``; nothing here comes from the code under test.

The bounds, with u = 2^-23 (one rounding is at most u/2 relative):

* ``dH[s,f]``:  (7 n_s + 8) u sum_t |A[t,s]| |inv_t| absdY[t,f],  n_s = the non-zero entries of column s,
  absdY = |d_out sg| + [t = ia] |d_pa ga| + [t = ib] |d_pb gb|.  Per term: dY carries at most three roundings (1.5 u), the product
  with inv one (0.5 u), the two split3 residuals 2^-25 each (0.25 u + 0.25 u), the three dropped plane products (n1.y2, n2.y1,
  n2.y2: each <= 2^-24 of the term) at most 1 u.  Summation: the 6 n_s kept bf16 products are exact in float32 and are added in
  float32 in any order: at most (6 n_s - 1) u (1 + 2^-8)^2 of the sum of their magnitudes, below (6.05 n_s - 1) u.  Together
  (6.05 n_s + 2.5) u; the rest of 7 n_s + 8 is slack.
* ``d_sg`` and ``d_bsum``:  (T + 4) u sum |terms|  (T additions in two partial sums, up to four roundings inside a term).
* ``d_ga`` and ``d_gb``:  4 u |ref|  (1/sg, y, d_p y: three roundings = 1.5 u).
* ``dY``:  4 u |ref|, elementwise.  Sums in float32 cannot promise that: at a pool's winner d_pa ga may cancel most of d_out sg,
  and the roundings of the two products (u/2 of EACH) are then several u of the result -- the float32 emulation of these cases
  was at 3.4 times the bound.  The kernel therefore forms dY in float64, where the three products are exact, and rounds once:
  (1/2 + 2^-29) u |ref|.  The same holds for the dH bound's "1.5 u (dY)", now 0.5 u.
* beside them dH and dY are held to the project's gate for this path, 2e-6 max|ref| (tests/test_gpu_weighted_backward.py).
"""
import numpy as np
import torch

import wide_backward_ref as wb
from oracle import backward_ref as br
from oracle import gates

U = 2.0 ** -23
B = 3
GATE = 2e-6
BLOCK_BYTES = 6144
KERNEL_T = (33, 64, 65, 96, 97, 100, 128)
KERNEL_F = (4, 36, 100, 260)
BUILDER_T = (33, 64, 65, 96, 97, 100, 128)
GRAPHS = ("sparse", "softmax", "corner-block", "hub", "isolated", "len1", "directed")
BUILDER_GRAPHS = ("sparse", "softmax", "corner-block", "hub")
STRUCTURES = wb.STRUCTURES
VARIANTS = wb.VARIANTS
GRAPH_T, GRAPH_F = (65, 100), 36
# (T, F, graph, variant): T x F on sparse / full, then every graph and variant at T = 65 and 100, F = 36
KERNEL_CASES = tuple((T, F, "sparse", "full") for T in KERNEL_T for F in KERNEL_F) + tuple(
    (T, GRAPH_F, g, v) for T in GRAPH_T for g in GRAPHS for v in VARIANTS if (g, v) != ("sparse", "full"))
# autograd cases: (B, T, K, F, seed) of br.case_inputs(..., graph="weighted"); the dense softmax adjacency is made from seed + 7
AUTOGRAD = {"t33": (3, 33, 40, 36, 9433), "t65": (3, 65, 64, 96, 9465), "t100": (3, 100, 64, 64, 9500), "t128": (2, 128, 72, 40, 9528)}
MIN_DENOMINATOR = 0.2


def _weights(shape, rng):
    """float32 of magnitude 2^U(-10, 10), either sign."""
    mag = np.exp2(rng.uniform(-10.0, 10.0, size=shape))
    return (mag * rng.choice((-1.0, 1.0), size=shape)).astype(np.float32)


def adjacency(T, graph, seed):
    """float32 [3,T,T], real-valued.  "softmax": dense softmax rows (positive).  Every other kind: the 0/1 pattern of the 0/1 tests
    (``wide_backward_ref.adjacency``; "sparse" is its "tree") times weights of magnitude within [2^-10, 2^10] and of both signs; a
    row whose |rowsum + 1| comes out below 0.2 takes the magnitudes of its weights, so that rowsum + 1 >= 1 there."""
    rng = np.random.default_rng(seed)
    if graph == "softmax":
        return torch.softmax(torch.from_numpy(rng.normal(0.0, 2.0, size=(B, T, T))), dim=2).float()
    pattern = wb.adjacency(T, "tree" if graph == "sparse" else graph, seed).numpy()
    a = np.where(pattern != 0, _weights(pattern.shape, rng), np.float32(0.0))      # (no -0.0: its bf16 planes would carry the sign)
    small = np.abs(a.astype(np.float64).sum(2) + 1.0) < 2 * MIN_DENOMINATOR      # (twice: float32 sums in any order stay above 0.2)
    a = np.where(small[:, :, None], np.abs(a), a).astype(np.float32)
    assert np.abs(a.astype(np.float64).sum(2) + 1.0).min() >= 2 * MIN_DENOMINATOR
    nz = np.abs(a[a != 0])
    assert nz.size == 0 or (nz.min() >= 2.0 ** -10 and nz.max() <= 2.0 ** 10)
    return torch.from_numpy(a)


def kernel_inputs(T, F, graph="sparse", variant="full"):
    """``wide_backward_ref.kernel_inputs`` with a real-valued adjacency: CPU float32 tensors of one C-ABI case."""
    seed = 2000 * T + F + 17 * GRAPHS.index(graph)
    c = wb.kernel_inputs(T, F, "tree", "full")
    c["adj"] = adjacency(T, graph, seed + 1)
    c["inv"] = (1.0 / (c["adj"].sum(2) + 1.0)).float()
    for k in {"no-store-gate": ("sg",), "no-pool-a": ("ga", "d_pa"), "no-pool-b": ("gb", "d_pb"), "no-d_out": ("d_out",), "full": ()}[variant]:
        c[k] = None
    return c


def softmax_adjacency(Bn, T, seed):
    """float32 [Bn,T,T]: dense softmax rows, the adjacency of a learned graph."""
    g = torch.Generator().manual_seed(seed)
    return torch.softmax(2.0 * torch.randn(Bn, T, T, generator=g), dim=2)


def autograd_inputs(name, bf16, dense):
    Bn, T, K, F, seed = AUTOGRAD[name]
    c = br.case_inputs(Bn, T, K, F, seed, bf16=bf16, graph="weighted")
    if dense:
        c["adj"] = softmax_adjacency(Bn, T, seed + 7)
    return c


# ---------------------------------------------------------------- the operand
def split3_np(x):
    """float32 -> three bf16 planes (as float32 values), each the nearest bfloat16 (ties to even) of what the planes before left."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    p0 = wb._bf16(x)
    r1 = x - p0
    p1 = wb._bf16(r1)
    return p0, p1, wb._bf16(r1 - p1)


def operand_bytes(Bn, T):
    W = (T + 31) // 32
    return Bn * (W * W * BLOCK_BYTES + 4)


def operand_np(adj):
    """The statement of ``ggcn_graph_operands_weighted_wide_t`` on a float32 [B,T,T] adjacency: ``(blocks, summary)``, uint8
    [B, W^2 * 6144] and uint32 [B].  N = A^T padded with zeros to 32 W; plane p, k-step k of block (s, t) at
    ((s W + t) * 6 + 2 p + k) * 1024; there lane l holds, as 8 bfloat16, row 32 s + l % 32 of N at the columns
    32 t + 16 k + 8 (j >> 2) + 4 (l / 32) + (j & 3), j = 0..7.  Bit 4 s + t of the summary: block (s, t) of N has a non-zero."""
    a = np.asarray(adj, dtype=np.float32)
    Bn, T, _ = a.shape
    W = (T + 31) // 32
    n = np.zeros((Bn, 32 * W, 32 * W), dtype=np.float32)
    n[:, :T, :T] = a.transpose(0, 2, 1)
    planes = np.stack([(p.view(np.uint32) >> 16).astype(np.uint16) for p in split3_np(n)])            # [3,B,32W,32W]
    lane, j, k = np.arange(64), np.arange(8), np.arange(2)
    rows = (32 * np.arange(W)[:, None] + (lane & 31)[None, :])[:, None, None, :, None]                   # [s,1,1,l,1]
    cols = (32 * np.arange(W)[:, None, None, None] + 16 * k[None, :, None, None] + 4 * (lane >> 5)[None, None, :, None]
            + (8 * (j >> 2) + (j & 3))[None, None, None, :])[None]                                        # [1,t,k,l,j]
    got = planes[:, :, rows, cols]                                                                         # [p,b,s,t,k,l,j]
    blocks = np.ascontiguousarray(got.transpose(1, 2, 3, 0, 4, 5, 6)).reshape(Bn, -1).view(np.uint8)
    assert blocks.shape == (Bn, W * W * BLOCK_BYTES)
    live = (n != 0).reshape(Bn, W, 32, W, 32).any(axis=(2, 4))                                             # [b,s,t]
    summary = (live.astype(np.uint32) << (4 * np.arange(W)[:, None] + np.arange(W)[None, :]).astype(np.uint32)).sum(axis=(1, 2)).astype(np.uint32)
    return blocks, summary


def operand_buffer_np(adj):
    """The whole buffer as the builder leaves it: the blocks of every graph, then the summary words."""
    blocks, summary = operand_np(adj)
    return np.concatenate([blocks.reshape(-1), summary.view(np.uint8)])


def planes_from_blocks(blocks, T):
    """The inverse of the layout: float32 [3,B,32W,32W] planes of N from uint8 [B, W^2 * 6144]."""
    Bn = blocks.shape[0]
    W = (T + 31) // 32
    v = blocks.view(np.uint16).reshape(Bn, W, W, 3, 2, 64, 8)
    out = np.zeros((3, Bn, 32 * W, 32 * W), dtype=np.float32)
    for s, t, k, l, j in np.ndindex(W, W, 2, 64, 8):
        col = 32 * t + 16 * k + 8 * (j >> 2) + 4 * (l >> 5) + (j & 3)
        out[:, :, 32 * s + (l & 31), col] = (v[:, s, t, :, k, l, j].astype(np.uint32) << 16).view(np.float32).T
    return out


# ---------------------------------------------------------------- the kernel's arithmetic in numpy
PRODUCTS = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))      # (plane of N, plane of D.dY), smallest first


def emulate(c):
    """float32 dH, dY [B,T,F], d_sg, d_ga, d_gb, d_bsum [B,F] of the case ``c`` (``kernel_inputs``) in the arithmetic of
    gate_pool_backward_weighted_wide_kernel: dY summed in float64 and rounded once to float32, fl(dY inv), split3 of it and of A^T into bf16 planes, float32 accumulation
    of the six exact plane products, smallest first, source blocks in ascending order, rows in ascending order inside a product;
    the column sums as two partial sums (rows with bit 2 clear / set).  The matrix cores' own order inside one MFMA is not public:
    the bound must hold for any."""
    f32 = np.float32
    n = lambda t: None if t is None else t.numpy().astype(f32)     # noqa: E731
    out, d_out, sg, ga, gb, d_pa, d_pb = (n(c[k]) for k in ("out", "d_out", "sg", "ga", "gb", "d_pa", "d_pb"))
    adj, inv = n(c["adj"]), n(c["inv"])
    Bn, T, F = out.shape
    one = np.ones((Bn, F), dtype=f32)
    sgv = one if sg is None else sg
    with np.errstate(divide="ignore"):
        inv_sg = one if sg is None else np.where(sg != 0, f32(1.0) / sg, f32(0.0)).astype(f32)
    gav, gbv = (one if ga is None else ga), (one if gb is None else gb)
    dpa, dpb = (np.zeros_like(one) if d_pa is None else d_pa), (np.zeros_like(one) if d_pb is None else d_pb)
    dv = np.zeros_like(out) if d_out is None else d_out
    y = out * inv_sg[:, None]
    ia, ib = (y * gav[:, None]).argmax(1), (y * gbv[:, None]).argmax(1)      # numpy's argmax: the first maximum
    take = lambda v, i: np.take_along_axis(v, i[:, None, :], 1)[:, 0]     # noqa: E731
    r = {"d_ga": dpa * take(y, ia), "d_gb": dpb * take(y, ib)}
    f64 = np.float64
    g = dv.astype(f64) * sgv.astype(f64)[:, None]                     # (float64: the products are exact, dY is rounded once)
    hot_a, hot_b = (np.arange(T)[None, :, None] == i[:, None, :] for i in (ia, ib))
    if d_pa is not None:
        g = np.where(hot_a, g + (dpa.astype(f64) * gav)[:, None], g)
    if d_pb is not None:
        g = np.where(hot_b, g + (dpb.astype(f64) * gbv)[:, None], g)
    g = g.astype(f32)
    half = (np.arange(T) >> 2) & 1
    acc_sg, bsum = np.zeros((2, Bn, F), dtype=f32), np.zeros((2, Bn, F), dtype=f32)
    for t in range(T):
        acc_sg[half[t]] = wb._fma(dv[:, t], y[:, t], acc_sg[half[t]])
        bsum[half[t]] = bsum[half[t]] + g[:, t]
    r["d_sg"], r["d_bsum"], r["dY"] = acc_sg[0] + acc_sg[1], bsum[0] + bsum[1], g
    yp = split3_np(g * inv[:, :, None])
    npl = split3_np(adj)                                              # planes of A: N[s][t] = A[t][s]
    acc = np.zeros((Bn, T, F), dtype=f32)
    for t0 in range(0, T, 32):
        for P, Q in PRODUCTS:
            for t in range(t0, min(t0 + 32, T)):
                acc = acc + npl[P][:, t, :, None] * yp[Q][:, t, None, :]      # (a product of two bf16 is exact in float32)
    r["dH"] = acc
    return r


def bounds(c, ref):
    """The elementwise bounds of the module docstring (float64 tensors) for the case ``c`` and its float64 statement ``ref``
    (``gates.gate_pool_backward_statement64`` on the same inputs, whose winners are the kernel's)."""
    d = lambda t: None if t is None else t.double()     # noqa: E731
    out, d_out, sg, ga, gb, d_pa, d_pb, adj, inv = (d(c[k]) for k in ("out", "d_out", "sg", "ga", "gb", "d_pa", "d_pb", "adj", "inv"))
    Bn, T, F = out.shape
    one = torch.ones(Bn, T, F, dtype=torch.float64, device=out.device)
    inv_sg = one[:, 0] if sg is None else torch.where(sg != 0, 1.0 / sg, torch.zeros_like(sg))
    y = out * inv_sg[:, None, :]
    absdy = torch.zeros_like(one)
    sg_terms = torch.zeros_like(one)
    if d_out is not None:
        absdy = absdy + (d_out * (1.0 if sg is None else sg[:, None, :])).abs()
        sg_terms = (d_out * y).abs()
    inv_sg32 = torch.ones_like(c["out"][:, 0]) if sg is None else torch.where(c["sg"] != 0, 1.0 / c["sg"], torch.zeros_like(c["sg"]))
    y32 = c["out"] * inv_sg32[:, None, :]
    for g, dp in ((ga, d_pa), (gb, d_pb)):
        if dp is None:
            continue
        gv = one[:, 0] if g is None else g
        hot = gates.first_argmax(y32 * gv.float()[:, None, :]).double()
        absdy = absdy + hot * (dp * gv)[:, None, :].abs()
    n_s = (adj != 0).double().sum(1)                                   # [B,S]: the non-zero entries of column s
    weight = torch.einsum("bts,btf->bsf", adj.abs(), inv.abs()[:, :, None] * absdy)
    return {"dH": (7.0 * n_s[:, :, None] + 8.0) * U * weight, "d_sg": (T + 4) * U * sg_terms.sum(1), "d_bsum": (T + 4) * U * absdy.sum(1),
            "d_ga": None if d_pa is None else 4 * U * ref["d_ga"].abs(), "d_gb": None if d_pb is None else 4 * U * ref["d_gb"].abs(),
            "dY": 4 * U * ref["dY"].abs()}


def statement(c, inv=None):
    return gates.gate_pool_backward_statement64(c["out"], c["sg"], c["ga"], c["gb"], c["d_out"], c["d_pa"], c["d_pb"], c["adj"],
                                                c["inv"] if inv is None else inv)
