"""The float64 reference of the gated layer's backward (oracle/backward_ref.py) checked on its own, on the CPU: its autograd
gradients against central finite differences, pool_tie_mask on hand-made ties, and the condition every GPU backward case
asserts -- at most 3 % of a case's pools are near-ties -- for each input recipe at a reduced batch (the keep factors of gate
dropout are a Bernoulli stand-in here: the hash that draws the real ones lives on the device)."""
import pytest
import torch

from oracle import backward_ref as br


def _leaves(B, T, K, F, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    adj = (torch.rand(B, T, T, generator=g) < 0.4).double()
    adj[:, torch.arange(T), torch.arange(T)] = 1.0
    adj[1] = adj[1] * torch.rand(T, T, generator=g, dtype=torch.float64)      # a weighted, asymmetric graph too
    return [r(B, T, K), r(K, F), r(F), r(B, F), r(B, F), r(B, F)], adj, (r(B, T, F), r(B, F), r(B, F))


@pytest.mark.parametrize("with_keep", [False, True], ids=["plain", "keep-factors"])
def test_reference_gradients_match_finite_differences(with_keep):
    B, T, K, F = 2, 5, 4, 3
    leaves, adj, (r1, r2, r3) = _leaves(B, T, K, F, seed=3)
    keep = None
    if with_keep:
        g = torch.Generator().manual_seed(4)
        keep = tuple((torch.rand(B, T, F, generator=g) >= 0.5).double() * 2.0 for _ in range(3))

    def loss(vs):
        x, w, b, sg, ga, gb = vs
        out, pa, pb = br.gated_layer_ref(x, adj, w, b, sg, ga, gb, keep=keep)
        return (out * r1).sum() + (pa * r2).sum() + (pb * r3).sum()

    # finite differences need the arg-max rows to stay put: no pool of this case is a near-tie
    ma, mb = br.layer_tie_masks(leaves[0], adj, leaves[1], leaves[2], leaves[4], leaves[5], 1e-3,
                                keep=keep)
    if not with_keep:   # (dropped tokens tie exactly at zero: flat there, for autograd and for the differences alike)
        assert not bool(ma.any()) and not bool(mb.any())
    vs = [v.clone().requires_grad_() for v in leaves]
    loss(vs).backward()
    eps = 1e-6
    for i, v in enumerate(leaves):
        fd = torch.zeros_like(v)
        flat, fdf = v.reshape(-1), fd.reshape(-1)
        for j in range(flat.numel()):
            keep_v = float(flat[j])
            flat[j] = keep_v + eps
            up = float(loss(leaves))
            flat[j] = keep_v - eps
            dn = float(loss(leaves))
            flat[j] = keep_v
            fdf[j] = (up - dn) / (2 * eps)
        err = float((vs[i].grad - fd).abs().max())
        assert err <= 1e-7 * max(1.0, float(fd.abs().max())), (i, err)


def test_absent_gates_count_as_ones_and_bf16_enters_exactly():
    B, T, K, F = 2, 4, 8, 3
    leaves, adj, _ = _leaves(B, T, K, F, seed=5)
    x, w, b = leaves[0], leaves[1], leaves[2]
    out, pa, pb = br.gated_layer_ref(x, adj, w, None, None, None, None)
    y = torch.einsum("bts,bsf->btf", adj, x @ w) / (adj.sum(2, keepdim=True) + 1)
    assert torch.allclose(out, y, rtol=0, atol=1e-14) and torch.equal(pa, out.max(1)[0]) and torch.equal(pa, pb)
    xb = x.to(torch.bfloat16)
    o1, _, _ = br.gated_layer_ref(xb, adj.float(), w.float(), b.float(), None, None, None)
    o2, _, _ = br.gated_layer_ref(xb.double(), adj.float().double(), w.float().double(), b.float().double(), None, None, None)
    assert o1.dtype == torch.float64 and torch.equal(o1, o2)


def test_pool_tie_mask_on_hand_made_ties():
    v = torch.tensor([[[1.0, 5.0, 0.0, -1.0], [1.0, 5.0 - 1e-5, 0.0, -3.0], [0.5, 1.0, 0.0, -1.0 - 3e-4]]], dtype=torch.float64)
    # columns: exact tie / gap 1e-5 / all-zero exact tie / gap 3e-4
    assert br.pool_tie_mask(v, 2e-4).tolist() == [[True, True, True, False]]
    assert br.pool_tie_mask(v, 4e-4).tolist() == [[True, True, True, True]]
    assert br.pool_tie_mask(v, 1e-6).tolist() == [[True, False, True, False]]
    assert br.pool_tie_mask(v[:, :1], 1.0).tolist() == [[False] * 4]       # one row: no runner-up
    assert br.tie_delta("f16mx8") == 2e-4 and br.tie_delta("fp32") == 4e-5 and abs(br.tie_delta("bf16x3", 0.5) - 4e-4) < 1e-18
    assert br.masked_share(torch.tensor([[True, False]]), torch.tensor([[False, False]])) == 0.25


@pytest.mark.parametrize("bf16", [False, True], ids=["float32", "bf16"])
@pytest.mark.parametrize("name", [r[0] for r in br.RECIPES])
def test_every_recipe_keeps_its_near_ties_under_three_percent(name, bf16):
    _, B, T, K, F, gates, graph, p = br.RECIPE[name]
    c = br.recipe_inputs(name, bf16=bf16, batch=None if B * T * K * F <= 2 ** 28 else 8)   # (only the large cases are reduced)
    keep = None
    if p:
        g = torch.Generator().manual_seed(br.case_seed(name) + 9)
        keep = tuple((torch.rand(c["r1"].shape, generator=g) >= p).double() / (1.0 - p) for _ in range(3))
    ma, mb = br.layer_tie_masks(c["x"], c["adj"], c["w"], c["b"], c["ga"], c["gb"], br.tie_delta("bf16x3", p), keep=keep)
    share = br.masked_share(ma, mb)
    print("%s: %.2f %% of the pools masked" % (name, 100 * share))
    assert share <= br.MAX_MASKED


@pytest.mark.parametrize("name", [r[0] for r in br.BLOCK_RECIPES])
def test_block_recipes_keep_their_near_ties_under_three_percent(name):
    c = br.block_inputs(name, bf16=True, batch=4)
    masks = br.block_tie_masks(c["x"], c["adj"], c["g1"], c["g2"], c["w1"], c["b1"], c["w2"], c["b2"], br.tie_delta("bf16x3"))
    share = br.masked_share(*masks)
    print("%s: %.2f %% of the pools masked" % (name, 100 * share))
    assert share <= br.MAX_MASKED
