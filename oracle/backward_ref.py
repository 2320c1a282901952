"""FLOAT64 REFERENCE OF THE GATED LAYER AND ITS GRADIENTS (test infrastructure, NOT product code).

``models/gcn.py:30-45`` + the gates and pools of ``models/bert_amir5.py:621-640`` in float64, on CPU or GPU tensors;
gradients come from torch autograd on it.  bfloat16 / float32 inputs enter as ``.double()``, which is exact.

Near-ties.  A max-pool sends its gradient to ONE row, and a forward error of TOL can move it to another row when the two
largest values are closer than that.  ``pool_tie_mask`` names those pools from the float64 values alone (nothing of the
code under test enters); a test zeroes the upstream gradient of the pools there for the GPU and the reference alike, so
the comparison does not depend on which of two (nearly) equal rows either side picked.  At most ``MAX_MASKED`` of a case's
pools may be masked: a condition on the inputs, asserted in every case.

``case_inputs`` is the input recipe the backward tests share (CPU: the 3 % condition, GPU: the kernels).
"""
import numpy as np
import torch

from oracle import ref_dense

MAX_MASKED = 0.03
# the forward parity gate per arithmetic, the one dict every test imports (bfloat16 features run the bf16x3 class)
TOL = {"fp32": 2e-5, "bf16x3": 1e-4, "f16mx8": 1e-4, "f16mx6": 1e-4}


def tie_delta(precision, p=0.0):
    """Two pooled candidates closer than this may swap under a forward error of TOL[precision] each (keep factors of gate
    dropout scale the values, and so the error, by 1/(1-p))."""
    return 2.0 * TOL[precision] / (1.0 - p)


def layer_output(x, adj, w, b):
    """y = D.A.(x.W) + b in float64 (``ref_dense.graph_convolution``)."""
    return ref_dense.graph_convolution(x.double(), adj.double(), w.double(), None if b is None else b.double(),
                                       dtype=torch.float64)


def gated(y, gate, keep=None):
    """y [B,T,F] * gate [B,F] (None: ones) * keep [B,T,F] (None: ones) -- ``bert_amir5.py:621-625`` without the repeat."""
    v = y if gate is None else y * gate.double()[:, None, :]
    return v if keep is None else v * keep.double()


def gated_layer_ref(x, adj, w, b, sg, ga, gb, keep=None):
    """``out, pa, pb`` in float64: out = y*sg*ks, pa = max_t y*ga*ka, pb = max_t y*gb*kb with y the plain layer output;
    ``keep = (ks, ka, kb)`` are the optional per-(token, feature) keep factors [B,T,F] of gate dropout (each may be None).
    A gate that is None counts as ones.  Leaves that require grad keep their graph (pass float64 leaves)."""
    ks, ka, kb = keep if keep is not None else (None, None, None)
    y = layer_output(x, adj, w, b)
    return gated(y, sg, ks), torch.max(gated(y, ga, ka), 1)[0], torch.max(gated(y, gb, kb), 1)[0]


def pool_tie_mask(v, delta):
    """[B,F] bool: pools of v [B,T,F] (float64, v = y*gate*keep) whose two largest values over t differ by less than
    delta.  A single row (T = 1) has no runner-up: nothing is masked."""
    if v.shape[1] < 2:
        return torch.zeros(v.shape[0], v.shape[2], dtype=torch.bool, device=v.device)
    top = torch.topk(v.detach(), 2, dim=1)[0]
    return (top[:, 0] - top[:, 1]) < delta


def layer_tie_masks(x, adj, w, b, ga, gb, delta, keep=None):
    """(mask_a, mask_b) of the two pools of ``gated_layer_ref`` on the same arguments."""
    _, ka, kb = keep if keep is not None else (None, None, None)
    with torch.no_grad():
        y = layer_output(x, adj, w, b)
        return pool_tie_mask(gated(y, ga, ka), delta), pool_tie_mask(gated(y, gb, kb), delta)


def masked_share(*masks):
    n = sum(int(m.numel()) for m in masks)
    return (sum(int(m.sum()) for m in masks) / n) if n else 0.0


# ---------------------------------------------------------------- the input recipe of the backward tests
GRAPHS = ("tree", "directed", "isolated", "complete", "len1", "weighted")


def case_adjacency(B, T, seed, graph="tree"):
    """float32 [B,T,T]: ``synth.dependency_batch(B, T, 3.5, lengths in [T//3, T])`` (graph 0 fills every row), and its variants:
    directed (upper triangle), isolated (every third node keeps its self loop only), complete (graph 0 has every edge),
    len1 (all lengths 1: self loops only), weighted (real-valued asymmetric edge weights in [0.25, 2))."""
    from ed_gated_gcn_amd import synth
    assert graph in GRAPHS
    rng = np.random.default_rng(seed)
    lengths = rng.integers(max(1, T // 3), T + 1, size=B)
    lengths[0] = T
    if graph == "len1":
        lengths[:] = 1
    a = synth.dependency_batch(B, T, 3.5, seed=seed, lengths=lengths).astype(np.float32)
    if graph == "directed":
        a = np.triu(a)
    if graph == "isolated":
        iso = np.arange(T) % 3 == 1
        a[:, iso, :] = 0
        a[:, :, iso] = 0
        a[:, np.arange(T), np.arange(T)] = 1
    if graph == "complete":
        a[0] = 1
    if graph == "weighted":
        a = a * rng.uniform(0.25, 2.0, size=a.shape).astype(np.float32)
    return torch.from_numpy(a)


def case_inputs(B, T, K, F, seed, bf16=False, gates="u01", graph="tree", bias=True):
    """CPU tensors of one case: x = randn [B,T,K] (rounded to bfloat16 when bf16), adj, (w, b) = synth.layer_params,
    three gates [B,F] in U(0,1) ("u01") or U(-0.5,0.5) ("sym"), upstream gradients R1 [B,T,F], R2, R3 [B,F] = randn."""
    from ed_gated_gcn_amd import synth
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, K, generator=g)
    if bf16:
        x = x.to(torch.bfloat16)
    w, b = synth.layer_params(K, F, seed=seed + 1)
    shift = 0.0 if gates == "u01" else 0.5
    sg, ga, gb = (torch.rand(B, F, generator=g) - shift for _ in range(3))
    r1, r2, r3 = torch.randn(B, T, F, generator=g), torch.randn(B, F, generator=g), torch.randn(B, F, generator=g)
    return {"x": x, "adj": case_adjacency(B, T, seed + 2, graph), "w": torch.from_numpy(w),
            "b": torch.from_numpy(b) if bias else None, "sg": sg, "ga": ga, "gb": gb, "r1": r1, "r2": r2, "r3": r3}


def block_ref(x, adj, g1, g2, w1, b1, w2, b2):
    """The block of ``bert_amir5.py:621-640`` in float64 (``ref_dense.gated_block``): gcn1, x1, y1, xy, x, out."""
    return ref_dense.gated_block(x.double(), adj.double(), g1.double(), g2.double(), w1.double(), b1.double(), w2.double(),
                                 b2.double(), dtype=torch.float64)


def block_tie_masks(x, adj, g1, g2, w1, b1, w2, b2, delta):
    """(m_x1, m_y1, m_out) of the block's three pools, from the float64 values."""
    with torch.no_grad():
        r = block_ref(x, adj, g1, g2, w1, b1, w2, b2)
        return (pool_tie_mask(gated(r["gcn1"], g1), delta), pool_tie_mask(gated(r["gcn1"], g2), delta),
                pool_tie_mask(r["x"], delta))


# (id, B, T, K, F, gates, graph, p): every input recipe of tests/test_gpu_backward.py's autograd cases; the seed of a case is
# derived from its id (case_seed).  tests/test_backward_ref_cpu.py holds each to the MAX_MASKED condition at a reduced batch.
RECIPES = [
    ("record", 4096, 32, 768, 768, "u01", "tree", 0.0),
    ("narrow", 64, 31, 256, 256, "u01", "tree", 0.0),
    ("f96", 16, 32, 128, 96, "sym", "tree", 0.0),
    ("ragged17", 5, 17, 34, 20, "u01", "tree", 0.0),
    ("ragged30", 7, 30, 300, 200, "u01", "tree", 0.0),
    ("f30", 6, 20, 64, 30, "u01", "tree", 0.0),
    ("square", 16, 32, 256, 256, "u01", "tree", 0.0),
    ("square-sym", 16, 32, 256, 256, "sym", "tree", 0.0),
    ("view", 16, 29, 256, 192, "u01", "tree", 0.0),
    ("drop32", 32, 32, 256, 256, "u01", "tree", 0.25),
    ("drop24", 16, 24, 128, 96, "u01", "tree", 0.25),
    ("drop100", 8, 100, 256, 256, "u01", "tree", 0.25),
    ("directed", 32, 32, 256, 256, "sym", "directed", 0.0),
    ("isolated", 32, 32, 256, 256, "u01", "isolated", 0.0),
    ("complete", 96, 32, 256, 256, "u01", "complete", 0.0),   # (every pool of the complete graph is an exact tie: 1 graph of 96)
    ("len1", 32, 32, 256, 256, "u01", "len1", 0.0),
    ("one", 1, 1, 8, 8, "u01", "tree", 0.0),
    ("weighted", 32, 24, 256, 256, "u01", "weighted", 0.0),
] + [("wide%d" % T, 5, T, 256, 256, "u01", "tree", 0.0) for T in (33, 40, 48, 49, 64, 65, 128, 129, 200, 231, 256)] + [
    ("wide768", 64, 231, 768, 768, "u01", "tree", 0.0),
] + [("long%d" % T, 4, T, 128, 128, "u01", "tree", 0.0) for T in (257, 300, 513)]
RECIPE = {r[0]: r for r in RECIPES}
BLOCK_RECIPES = [("block32", 256, 32, 768), ("block231", 64, 231, 768)]


def case_seed(name):
    return 1000 + 7 * sum(ord(c) * (i + 1) for i, c in enumerate(name)) % 100000


def recipe_inputs(name, bf16=False, batch=None, bias=True):
    """``case_inputs`` of the named recipe (``batch``: a reduced batch size for the CPU check)."""
    _, B, T, K, F, gates, graph, _ = RECIPE[name]
    return case_inputs(B if batch is None else min(B, batch), T, K, F, case_seed(name), bf16=bf16, gates=gates, graph=graph, bias=bias)


def block_inputs(name, bf16=False, batch=None):
    """x, adj, two gates in U(0,1), two square layers, R1 [B,H] and R2 [B,T,H] of the named block recipe."""
    from ed_gated_gcn_amd import synth
    _, B, T, H = [r for r in BLOCK_RECIPES if r[0] == name][0]
    B = B if batch is None else min(B, batch)
    seed = case_seed(name)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, H, generator=g)
    if bf16:
        x = x.to(torch.bfloat16)
    (w1, b1), (w2, b2) = synth.layer_params(H, H, seed=seed + 1), synth.layer_params(H, H, seed=seed + 2)
    t = torch.from_numpy
    return {"x": x, "adj": case_adjacency(B, T, seed + 3), "g1": torch.rand(B, H, generator=g), "g2": torch.rand(B, H, generator=g),
            "w1": t(w1), "b1": t(b1), "w2": t(w2), "b2": t(b2),
            "r1": torch.randn(B, H, generator=g), "r2": torch.randn(B, T, H, generator=g)}
