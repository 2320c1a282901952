"""The inputs of tests/test_gpu_wide_structures.py can tell a wrong kernel from a right one (no GPU needed).

``oracle/wide_structures.py`` builds one batch of directed and extreme graphs per length.  Here, for every length and shape the GPU
tests run:

1. each graph is what its name claims (asymmetric where claimed, the ladder's degrees around the 8 / 16 edge-list boundaries, the
   hub and the corner block zero elsewhere, the empty graph empty);
2. DISCRIMINATION: on every asymmetric graph the float64 reference of ``A`` and of ``A^T`` are at least 100 gates apart over ``out``
   -- a kernel, edge-list builder or aggregation that used sources for destinations cannot pass the GPU gate on any of them;
3. the gate is REACHABLE: the plain float32 layer on the CPU (``ref_dense.graph_convolution``) stays within a tenth of the gate of the
   float64 reference, so a GPU miss is the kernel's, not the reference's or the inputs'.

The gate is the project's own: ``br.TOL[precision] * max(1, max|ref|)`` per graph (both split precisions share 1e-4).
"""
import numpy as np
import pytest
import torch

from oracle import backward_ref as br
from oracle import ref_dense
from oracle import wide_structures as ws

TOL = br.TOL["f16mx8"]
assert TOL == br.TOL["bf16x3"]
ALL_T = tuple(sorted(set(ws.LAYER_T) | set(ws.BLOCK_T) | set(ws.HOSTILE_T) | {c[0] for c in ws.LAYER_CASES + ws.DROP_CASES}))
SHAPES = tuple(dict.fromkeys(ws.LAYER_CASES + ws.DROP_CASES + tuple((T,) + ws.HOSTILE_SHAPE for T in ws.HOSTILE_T)))


@pytest.mark.parametrize("T", ALL_T)
def test_each_graph_is_what_its_name_claims(T):
    adj, names = ws.structure_batch(T, seed=T)
    assert names == ws.NAMES and adj.shape == (len(names), T, T) and adj.dtype == np.float32
    assert set(np.unique(adj)) <= {0.0, 1.0}
    again, _ = ws.structure_batch(T, seed=T)
    assert np.array_equal(adj, again)
    g = dict(zip(names, adj))
    for n in ws.SYMMETRIC:
        assert np.array_equal(g[n], g[n].T), n
    for n in ws.ASYMMETRIC:
        assert not np.array_equal(g[n], g[n].T), n
    idx = np.arange(T)
    assert g["tree"][idx, idx].all() and 3.0 <= g["tree"].sum() / T <= 4.0          # self loops, the mean degree asked for
    assert not np.tril(g["upper"], -1).any() and not np.triu(g["lower"], 1).any()
    assert np.array_equal(g["upper"] + g["lower"] - np.eye(T, dtype=np.float32), g["tree"])
    assert not g["random-directed"][idx, idx].any() and g["random-directed"].sum() > T
    assert g["complete"].sum() == T * T and g["empty"].sum() == 0
    hub = g["hub"].copy()
    assert hub[5].all() and hub[20:32, 7].all() and hub[0, T - 1] == 1
    hub[5, :] = 0; hub[20:32, 7] = 0; hub[0, T - 1] = 0
    assert not hub.any()
    deg = g["ladder"].sum(1).astype(int)
    assert np.array_equal(deg, [min(ws.LADDER_DEGREES[r % len(ws.LADDER_DEGREES)], T) for r in range(T)])
    assert {0, 1, 8, 9, 16, 17} <= set(deg.tolist())
    r0 = 32 * ((T - 1) // 32)
    corner = g["corner-block"].copy()
    assert corner[r0:, :32].all() and r0 >= 32
    corner[r0:, :32] = 0
    assert not corner.any()
    assert np.array_equal(g["shift"], np.eye(T, k=1, dtype=np.float32))
    assert g["len1"].sum() == 1 and g["len1"][0, 0] == 1
    n = T - 1 - T // 3
    assert not g["ragged"][n:].any() and not g["ragged"][:, n:].any() and not np.tril(g["ragged"], -1).any()
    assert g["ragged"][np.arange(n), np.arange(n)].all()
    if T > 128:   # what the eight-wavefront layer's three degree branches and its filler row need
        for name in ("ladder", "hub", "complete", "empty"):
            d = g[name].sum(1)
            print("T=%d %s: rows with <= 8 / 9..16 / > 16 sources: %d / %d / %d" % (
                T, name, int((d <= 8).sum()), int(((d > 8) & (d <= 16)).sum()), int((d > 16).sum())))
        d = g["ladder"].sum(1)
        assert (d <= 8).any() and ((d > 8) & (d <= 16)).any() and (d > 16).any()


@pytest.mark.parametrize("T,K,F", SHAPES)
def test_layer_inputs_discriminate_and_the_gate_is_reachable(T, K, F):
    c = ws.layer_inputs(T, K, F)
    ref = br.gated_layer_ref(c["x"], c["adj"], c["w"], c["b"], c["sg"], c["ga"], c["gb"])
    swapped = br.gated_layer_ref(c["x"], c["adj"].transpose(1, 2), c["w"], c["b"], c["sg"], c["ga"], c["gb"])
    assert ref[0].dtype == torch.float64
    ratios = {}
    for g, name in enumerate(c["names"]):
        gate = ws.gate_of(ref[0][g], TOL)
        ratios[name] = float((ref[0][g] - swapped[0][g]).abs().max()) / gate
    print("T=%d K=%d F=%d: max|ref(A) - ref(A^T)| / gate: %s" % (T, K, F, ", ".join("%s %.0f" % kv for kv in ratios.items())))
    for name in ws.SYMMETRIC:
        assert ratios[name] == 0.0, name
    for name in ws.ASYMMETRIC:
        assert ratios[name] >= 100.0, "%s at T=%d: A and A^T are only %.1f gates apart" % (name, T, ratios[name])
    # the same for the folded evaluation's launch (bias_pre added before the aggregation)
    xp, wp = ws.with_prebias(c["x"], c["w"], c["pre"])
    pref = br.gated_layer_ref(xp, c["adj"], wp, c["b"], c["sg"], c["ga"], c["gb"])[0]
    pswap = br.gated_layer_ref(xp, c["adj"].transpose(1, 2), wp, c["b"], c["sg"], c["ga"], c["gb"])[0]
    for g, name in enumerate(c["names"]):
        if name in ws.ASYMMETRIC:
            assert float((pref[g] - pswap[g]).abs().max()) >= 100.0 * ws.gate_of(pref[g], TOL), name
    # with_prebias is the entry's formula: D.A.(x.w + 1.pre^T) + b
    hidden = c["x"].double() @ c["w"].double() + c["pre"].double()
    a = c["adj"].double()
    direct = (a @ hidden) / (a.sum(2, keepdim=True) + 1) + c["b"].double()
    assert float((direct * c["sg"].double()[:, None, :] - pref).abs().max()) <= 1e-12
    # the empty graph: y = bias, the denominator is 1
    e = c["names"].index("empty")
    assert float((ref[0][e] - (c["b"].double() * c["sg"][e].double()).expand(T, F)).abs().max()) <= 1e-15
    # reachability: float32 on the CPU against float64
    y32 = ref_dense.graph_convolution(c["x"], c["adj"], c["w"], c["b"])
    assert y32.dtype == torch.float32
    worst = 0.0
    for g, name in enumerate(c["names"]):
        out32 = y32[g] * c["sg"][g]
        worst = max(worst, float((out32.double() - ref[0][g]).abs().max()) / ws.gate_of(ref[0][g], TOL))
    print("  float32 on the CPU: at most %.2f %% of the gate; max|ref| %.3g" % (100 * worst, float(ref[0].abs().max())))
    assert worst <= 0.1


@pytest.mark.parametrize("T", ws.BLOCK_T)
def test_block_inputs_discriminate_and_the_gate_is_reachable(T):
    c = ws.block_inputs(T)
    args = (c["g1"], c["g2"], c["w1"], c["b1"], c["w2"], c["b2"])
    ref = br.block_ref(c["x"], c["adj"], *args)
    swapped = br.block_ref(c["x"], c["adj"].transpose(1, 2), *args)
    f32 = ref_dense.gated_block(c["x"], c["adj"], *args)
    assert ref["out"].dtype == torch.float64 and f32["out"].dtype == torch.float32
    # `out` = max_t x is all that want=("out",) returns, and a max over rows does not see WHICH rows hold the values: on `shift` (a
    # permutation) A and A^T pool to the same values but for the end rows, and on `corner-block` no path of two edges exists, so
    # that layer 2 sees the biases alone on either.  The GPU test therefore also asks the folded evaluation for x.
    for k, blind in (("x", ()), ("out", ("shift", "corner-block"))):
        ratios = {}
        for g, name in enumerate(c["names"]):
            gate = ws.gate_of(ref[k][g], TOL)
            ratios[name] = float((ref[k][g] - swapped[k][g]).abs().max()) / gate
            assert float((f32[k][g].double() - ref[k][g]).abs().max()) <= 0.1 * gate, (k, name)
        print("T=%d block %s: max|ref(A) - ref(A^T)| / gate: %s" % (T, k, ", ".join("%s %.0f" % kv for kv in ratios.items())))
        for name in (n for n in ws.ASYMMETRIC if n not in blind):
            assert ratios[name] >= 100.0, "%s at T=%d (%s): A and A^T are only %.1f gates apart" % (name, T, k, ratios[name])
