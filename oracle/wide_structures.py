"""DIRECTED AND EXTREME GRAPHS OF 33..256 NODES (test infrastructure, NOT product code).

One batch that holds one graph per structure, so that one launch of the one-launch float32 layers (``fused_wide.hip``: 33..128
nodes, ``fused_wide8.hip``: 129..256) sees them all.  Every other graph that reaches those kernels comes from
``synth.dependency_batch``: symmetric, self loops, about 4 edges per row -- on which ``A^T = A``, no row is empty, no row is near
the 8 / 16 edge-list boundaries and no 32 x 32 adjacency block is empty.  ``tests/test_wide_structures_cpu.py`` holds the batch
to what the names claim (and to telling ``A`` from ``A^T`` by 100 gates); ``tests/test_gpu_wide_structures.py`` runs the kernels
on it.  Row i of an adjacency holds the SOURCES node i sums over (``gcn.py:41``: ``adj @ hidden``).

The float64 reference stays ``oracle/backward_ref.py`` (``gated_layer_ref``, ``block_ref``); here are only the graphs and the
input recipe the CPU and GPU tests share.
"""
import numpy as np
import torch

NAMES = ("tree", "upper", "lower", "random-directed", "complete", "empty", "hub", "ladder", "corner-block", "shift", "len1", "ragged")
SYMMETRIC = ("tree", "complete", "empty", "len1")
ASYMMETRIC = tuple(n for n in NAMES if n not in SYMMETRIC)
LADDER_DEGREES = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33)      # around the edge lists' 8 / 16 boundaries and a mask word's 32

# the lengths the GPU tests run: both slots of fused_wide.hip at and just past their edges, both row-group counts of
# fused_wide8.hip, the filler row (255) against the full slot (256); 100 and 231 are the product's own (LitBank, ACE cased)
LAYER_T = (33, 64, 65, 96, 97, 128, 129, 160, 161, 192, 193, 255, 256)
FAST_SHAPE, GENERAL_SHAPE = (64, 96), (72, 40)   # (K, F): the fast main loop + vector stores / K % 32 != 0, a dead-column tail
# (T, K, F) of every layer case: the two shapes alternate along LAYER_T; the product's lengths at (256, 256)
LAYER_CASES = tuple((T,) + (FAST_SHAPE if i % 2 == 0 else GENERAL_SHAPE) for i, T in enumerate(LAYER_T)) + ((100, 256, 256), (231, 256, 256))
BLOCK_T, BLOCK_H = (33, 100, 129, 231, 256), 128
DROP_CASES = ((100,) + GENERAL_SHAPE, (231,) + FAST_SHAPE)
HOSTILE_T, HOSTILE_SHAPE = (100, 231), (64, 72)   # F = 72: a column-tile guard; ldo = F + 3 / F + 4 are the two store forms


def structure_batch(T, seed):
    """(float32 [G,T,T] of 0 / 1, the graphs' names): one graph per structure of ``NAMES``, 33 <= T."""
    from ed_gated_gcn_amd import synth
    assert T >= 33
    rng = np.random.default_rng(seed)
    tree = synth.dependency_batch(1, T, 3.5, seed=seed)[0].astype(np.float32)
    g = {"tree": tree, "upper": np.triu(tree), "lower": np.tril(tree)}      # row i sees only j >= i / only j <= i
    rd = (rng.random((T, T)) < 0.05).astype(np.float32)
    rd[np.arange(T), np.arange(T)] = 0
    assert not np.array_equal(rd, rd.T)
    g["random-directed"] = rd
    g["complete"] = np.ones((T, T), dtype=np.float32)       # largest nnz: every row of a 129..256-node graph walks its mask words
    g["empty"] = np.zeros((T, T), dtype=np.float32)         # not even a self loop: y = bias, the denominator is 1
    hub = np.zeros((T, T), dtype=np.float32)
    hub[5, :] = 1               # one row sees every node
    hub[20:32, 7] = 1           # twelve rows share one source
    hub[0, T - 1] = 1           # a source in the last mask word
    g["hub"] = hub
    ladder = np.zeros((T, T), dtype=np.float32)
    for r in range(T):
        d = min(LADDER_DEGREES[r % len(LADDER_DEGREES)], T)
        ladder[r, rng.choice(T, size=d, replace=False)] = 1
    g["ladder"] = ladder
    corner = np.zeros((T, T), dtype=np.float32)
    corner[32 * ((T - 1) // 32):, :32] = 1                  # ONE off-diagonal 32 x 32 block; every other block is empty
    g["corner-block"] = corner
    shift = np.zeros((T, T), dtype=np.float32)
    shift[np.arange(T - 1), np.arange(1, T)] = 1            # row i sees node i + 1 only
    g["shift"] = shift
    len1 = np.zeros((T, T), dtype=np.float32)
    len1[0, 0] = 1
    g["len1"] = len1
    n = T - 1 - T // 3
    ragged = np.zeros((T, T), dtype=np.float32)
    ragged[:n, :n] = np.triu(synth.dependency_batch(1, n, 3.5, seed=seed + 1)[0])
    g["ragged"] = ragged
    assert tuple(g) == NAMES
    return np.stack([g[k] for k in NAMES]), NAMES


def case_seed(T, K, F):
    return 40000 + 1000 * T + 7 * K + F


def layer_inputs(T, K, F):
    """CPU tensors of the layer case (T, K, F) on ``structure_batch(T, seed)``: x = randn [G,T,K], (w, b) = synth.layer_params,
    store gate ``sg`` in U(0.1, 0.9), pool gate ``ga`` in U(-1, 1) (negative gates: the min side of the pools), ``gb`` = sg, and a
    second bias ``pre`` [F] (``ggcn_layer_fused_prebias``'s ``bias_pre``)."""
    from ed_gated_gcn_amd import synth
    seed = case_seed(T, K, F)
    adj, names = structure_batch(T, seed)
    G = len(names)
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(G, T, K, generator=gen)
    w, b = synth.layer_params(K, F, seed=seed + 1)
    sg = 0.1 + 0.8 * torch.rand(G, F, generator=gen)
    ga = 2.0 * torch.rand(G, F, generator=gen) - 1.0
    pre = torch.from_numpy(synth.layer_params(K, F, seed=seed + 2)[1])
    return {"names": names, "adj": torch.from_numpy(adj), "x": x, "w": torch.from_numpy(w), "b": torch.from_numpy(b),
            "sg": sg, "ga": ga, "gb": sg.clone(), "pre": pre}


def block_inputs(T, H=BLOCK_H):
    """CPU tensors of the block case: x = randn [G,T,H], two gates in U(0,1), two square layers."""
    from ed_gated_gcn_amd import synth
    seed = case_seed(T, H, H) + 500
    adj, names = structure_batch(T, seed)
    G = len(names)
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(G, T, H, generator=gen)
    (w1, b1), (w2, b2) = synth.layer_params(H, H, seed=seed + 1), synth.layer_params(H, H, seed=seed + 2)
    t = torch.from_numpy
    return {"names": names, "adj": t(adj), "x": x, "g1": torch.rand(G, H, generator=gen), "g2": torch.rand(G, H, generator=gen),
            "w1": t(w1), "b1": t(b1), "w2": t(w2), "b2": t(b2)}


def with_prebias(x, w, pre):
    """(x', w') with ``x'.w' = x.w + 1.pre^T``: a column of ones on x, the row ``pre`` under w -- so that the float64 reference of
    the folded evaluation's launch, ``D.A.(x.w + 1.pre^T) + b``, is ``gated_layer_ref`` itself on (x', w')."""
    ones = torch.ones(x.shape[:-1] + (1,), dtype=x.dtype, device=x.device)
    return torch.cat([x, ones], dim=-1), torch.cat([w, pre.to(w.dtype)[None, :]], dim=0)


def gate_of(ref, tol):
    """The project's parity gate on one graph's reference values: tol * max(1, max|ref|) (the bound of ``oracle/gates.py`` ``gate``)."""
    return tol * max(1.0, float(ref.abs().max())) if ref.numel() else 0.0
