"""The gated block at the batch sizes the product runs it (run with ``-m gpu`` on an MI355X).

From 2048 graphs up (f16mx8, every output) ``ggcn_block_fused`` runs the eight-wavefront kernel of ``fused_block8.hip``: the
kernel behind the headline number.  Here every graph it computes is compared with a float64 restatement of the block
(``oracle/ref_dense.py`` with ``dtype=torch.float64``) at the project's tolerance, 1e-4 * max(1, max |ref|), and with the
four-wavefront kernel (``GGCN_BLOCK_FORM=4``) bit for bit -- at ragged and whole shapes, on the graph structures and
parameters where a kernel goes wrong, for inputs beyond 2 GiB -- and the sticky f16mx8 range flag is checked on both kernels
for every staging pass of a tile.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_dense  # noqa: E402  (tests may use the oracle)
from oracle.gpu_support import dev, make_layer, pkg  # noqa: E402,F401

TOL = 1e-4
OUTS = ("x1", "y1", "x", "out")


def _layer(pkg, dev, w, b):
    return make_layer(pkg, dev, w, b, precision="f16mx8").eval()


def _graphs(kind, B, T, rng):
    """uint8 [B,T,T] 0/1 adjacencies of one structure class."""
    from ed_gated_gcn_amd import synth
    if kind == "complete":                   # the largest nnz: every node sees every node
        return np.ones((B, T, T), dtype=np.uint8)
    if kind == "directed":                   # asymmetric: row i lists the sources of node i only
        adj = (rng.random((B, T, T)) < 0.2).astype(np.uint8)
        assert (adj != adj.transpose(0, 2, 1)).any()
        return adj
    lengths = rng.integers(1, T + 1, size=B)
    lengths[:3] = (1, T, 2)
    lengths[-2:] = (T, 1)                    # padded graphs, length 1 included, at both ends of the batch
    adj = synth.dependency_batch(B, T, min(4.0, T), seed=int(rng.integers(1 << 30)), lengths=lengths)
    if kind == "isolated":                   # degree 0: no edge, not even the self loop
        iso = rng.random((B, T)) < 0.2
        iso[:, -1] = True
        adj[iso] = 0
        adj.transpose(0, 2, 1)[iso] = 0
    return adj


def _ref64(x, adj, g1, g2, params, graphs, chunk=256):
    """float64 block on the listed graphs, a chunk at a time: (graph indices, dict of float64 CPU tensors)."""
    p64 = [None if a is None else torch.from_numpy(np.asarray(a, dtype=np.float64)) for a in params]
    for i in range(0, len(graphs), chunk):
        idx = np.asarray(graphs[i:i + chunk])
        it = torch.from_numpy(idx).to(x.device)
        yield idx, ref_dense.gated_block(x[it].cpu().double(), torch.from_numpy(adj[idx]), g1[it].cpu().double(),
                                         g2[it].cpu().double(), *p64, dtype=torch.float64)


def _run_both_forms(pkg, lib, x, csr, g1, g2, l1, l2, want):
    with torch.no_grad():
        r8 = pkg.gated_gcn_block(x, csr, g1, g2, l1, l2, want=want)
        os.environ["GGCN_BLOCK_FORM"] = "4"
        try:
            B, T, K = x.shape
            assert lib.ggcn_block_fused_form(B, T, K, l2.out_features) == 4
            r4 = pkg.gated_gcn_block(x, csr, g1, g2, l1, l2, want=want)
        finally:
            os.environ.pop("GGCN_BLOCK_FORM", None)
    torch.cuda.synchronize()
    return r8, r4


def _check_block(pkg, dev, x, adj, g1, g2, params, want=None, graphs=None):
    """The eight-wavefront form's shape rule holds; form 8 and form 4 give the same bits for every output; every output is
    finite; the listed graphs (all by default) match the float64 block; outputs not asked for are None."""
    lib = pkg.load_library()
    B, T, K = x.shape
    w1, b1, w2, b2 = params
    F = w2.shape[1]
    assert lib.ggcn_block_fused_form(B, T, K, F) == 8
    l1, l2 = _layer(pkg, dev, w1, b1), _layer(pkg, dev, w2, b2)
    csr = pkg.BatchedCSR.from_dense(torch.from_numpy(adj).to(dev))
    want = ("x1", "y1", "xy", "x", "out") if want is None else want
    r8, r4 = _run_both_forms(pkg, lib, x, csr, g1, g2, l1, l2, want)
    for k in ("x1", "y1", "xy", "x", "out"):
        if k not in want:
            assert r8[k] is None and r4[k] is None, k
            continue
        assert r8[k] is not None and torch.equal(r8[k], r4[k]), "%s: form 8 and form 4 differ" % k
        assert bool(torch.isfinite(r8[k]).all()), "%s: not finite" % k
    l1.check_range()                          # in-range data: no report
    full = graphs is None
    graphs = np.arange(B) if full else np.asarray(graphs)
    err = {k: 0.0 for k in OUTS}
    top = {k: 0.0 for k in OUTS}
    worst = {k: -1 for k in OUTS}
    xy_ref = 0.0
    for idx, ref in _ref64(x, adj, g1, g2, params, graphs):
        it = torch.from_numpy(idx).to(dev)
        for k in OUTS:
            if r8[k] is None:
                continue
            d = (r8[k][it].cpu().double() - ref[k]).abs().reshape(len(idx), -1).amax(1)
            if float(d.max()) > err[k]:
                err[k], worst[k] = float(d.max()), int(idx[int(d.argmax())])
            top[k] = max(top[k], float(ref[k].abs().max()))
        xy_ref += float((ref["x1"] * ref["y1"]).sum())
    for k in OUTS:
        if r8[k] is not None:
            assert err[k] <= TOL * max(1.0, top[k]), "%s: max|diff| %.3g (graph %d) > %.1g * max(1, %.3g)" % (k, err[k], worst[k], TOL, top[k])
    if full and r8["xy"] is not None:
        xy_ref /= B
        assert abs(float(r8["xy"]) - xy_ref) <= TOL * max(1.0, abs(xy_ref)), (float(r8["xy"]), xy_ref)
    return r8


def _case(dev, B, T, K, F, seed, kind="padded", bias=(True, True)):
    from ed_gated_gcn_amd import synth
    rng = np.random.default_rng(seed)
    adj = _graphs(kind, B, T, rng)
    gen = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(B, T, K, device=dev, generator=gen)
    g1 = torch.rand(B, F, device=dev, generator=gen)
    g2 = torch.rand(B, F, device=dev, generator=gen)
    (w1, b1), (w2, b2) = synth.layer_params(K, F, seed=seed + 1), synth.layer_params(F, F, seed=seed + 2)
    return x, adj, g1, g2, [w1, b1 if bias[0] else None, w2, b2 if bias[1] else None]


# ---------------------------------------------------------------- 1. every graph against float64, on the product's path
@pytest.mark.parametrize("B,T,K,F", [(4096, 32, 768, 768), (2048, 32, 768, 768), (2100, 29, 768, 768), (1024, 32, 768, 768),
                                     (2048, 16, 768, 768), (6144, 32, 256, 256), (1536, 32, 1024, 1024), (2048, 32, 1024, 768)],
                         ids=["headline", "2048", "ragged-T29", "whole-rounds-1024", "T16", "F256-one-slice", "F1024-four-slices",
                              "K1024-F768"])
def test_eight_wavefront_block_every_graph_vs_float64(pkg, dev, B, T, K, F):
    """The batch shapes that take form 8 -- the headline, the smallest 6-round and 3-whole-round batches, graph slots with
    T < 32 (rows >= T never read, stored or pooled), one and four column slices, K != F -- every graph vs float64."""
    _check_block(pkg, dev, *_case(dev, B, T, K, F, seed=B + T + K + F))


@pytest.mark.parametrize("kind", ["padded", "isolated", "complete", "directed"])
def test_eight_wavefront_block_graph_structures_vs_float64(pkg, dev, kind):
    """Padded graphs (length 1 included), nodes of degree 0, complete 32-node graphs (the largest nnz), directed 0/1
    adjacencies: every graph of a 2048-graph batch vs float64."""
    _check_block(pkg, dev, *_case(dev, 2048, 32, 768, 768, seed=11, kind=kind))


def test_eight_wavefront_block_zero_gates_and_negative_columns(pkg, dev):
    """Gates with exact zeros (the pool of a zero-gated column is a signed zero, never -inf) and columns whose gated values are
    negative on every node (the pool picks a negative value, not the 0 of a padding row): T = 29 and T = 32."""
    for T in (32, 29):
        x, adj, g1, g2, params = _case(dev, 2048 if T == 32 else 2100, T, 768, 768, seed=13 + T)
        B, F = g1.shape
        cols = torch.arange(0, F, 7, device=dev)
        g1[:, cols] = 0.0                               # x1 of these columns: max of zeros
        g2[::3, 5::11] = 0.0                            # y1, x and out of some graphs' columns: max of zeros
        params[1] = params[1].copy()
        params[3] = params[3].copy()
        params[1][1::5] -= 40.0                         # gcn1 < 0 on every node of these columns (|x.W1| is a few units)
        params[3][2::5] -= 40.0                         # and gc2's output
        r = _check_block(pkg, dev, x, adj, g1, g2, params)
        neg = r["y1"][:, 1::5][g2[:, 1::5] > 0]
        assert bool((neg < 0).all())                    # the pool kept a negative value
        assert bool((r["x1"][:, cols] == 0).all())      # zero gates pool to (signed) zero


@pytest.mark.parametrize("bias", [(False, True), (True, False), (False, False)], ids=["gc1-no-bias", "gc2-no-bias", "no-bias"])
def test_eight_wavefront_block_without_bias_vs_float64(pkg, dev, bias):
    """gc1 and / or gc2 built without bias: the launch gets NULL bias rows (and a zero `mid` row for gc1 without bias)."""
    _check_block(pkg, dev, *_case(dev, 2048, 32, 768, 768, seed=17, bias=bias))


@pytest.mark.parametrize("want", [("x1", "y1", "xy", "out"), ("x1", "y1", "x", "out"), ("x1", "y1", "out")],
                         ids=["no-x", "no-xy", "x1-y1-out"])
def test_eight_wavefront_block_output_subsets_vs_float64(pkg, dev, want):
    """want= without x (x_out = NULL), without xy (no regulariser partials) and both: the same kernel, the outputs not asked
    for come back as None, the others match float64 on every graph."""
    _check_block(pkg, dev, *_case(dev, 2048, 32, 768, 768, seed=19), want=want)


@pytest.mark.parametrize("pad", [4, 3], ids=["ldx%4==0", "ldx%4!=0"])
def test_eight_wavefront_block_strided_input_vs_float64(pkg, dev, pad):
    """x as a [:, :, :K] view of a wider tensor: ldx = K + 4 is read through the stride by form 8; ldx = K + 3 breaks the 16-byte
    rows and falls back to the four-wavefront kernel.  Both vs float64."""
    x, adj, g1, g2, params = _case(dev, 2048, 32, 768, 768, seed=23)
    wide = torch.randn(2048, 32, 768 + pad, device=dev)
    wide[:, :, :768] = x
    view = wide[:, :, :768]
    assert not view.is_contiguous() and view.reshape(-1, 768).stride(0) == 768 + pad
    _check_block(pkg, dev, view, adj, g1, g2, params)


def test_eight_wavefront_block_beyond_2gib(pkg, dev):
    """22 000 graphs x 32 x 768: X and x each exceed 2 GiB (rows whose byte offset from X passes 2^31).  Form 8 and form 4 the
    same bits over the whole batch; against float64 the first and last 8 graphs, every 1000th and 256 drawn with a seed."""
    B, T, H = 22000, 32, 768
    assert B * T * H * 4 > 2 ** 31
    x, adj, g1, g2, params = _case(dev, B, T, H, H, seed=29)
    rng = np.random.default_rng(29)
    graphs = np.unique(np.concatenate([np.arange(8), np.arange(B - 8, B), np.arange(0, B, 1000), rng.integers(0, B, size=256)]))
    assert (graphs.max() * T * H * 4) > 2 ** 31
    _check_block(pkg, dev, x, adj, g1, g2, params, graphs=graphs)


# ---------------------------------------------------------------- 2. the range flag on both block kernels at large batches
FORMS = ["8", "4"]


def _range_setup(pkg, dev, B, T, w1, b1, w2, b2, seed):
    rng = np.random.default_rng(seed)
    adj = _graphs("padded", B, T, rng)
    csr = pkg.BatchedCSR.from_dense(torch.from_numpy(adj).to(dev))
    gen = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(B, T, 768, device=dev, generator=gen).clamp_(-4.0, 4.0)
    g1, g2 = torch.rand(B, 768, device=dev, generator=gen), torch.rand(B, 768, device=dev, generator=gen)
    return x, csr, g1, g2, _layer(pkg, dev, w1, b1), _layer(pkg, dev, w2, b2)


def _forward(pkg, x, csr, g1, g2, l1, l2, form):
    if form == "4":
        os.environ["GGCN_BLOCK_FORM"] = "4"
    try:
        lib = pkg.load_library()
        B, T, K = x.shape
        assert lib.ggcn_block_fused_form(B, T, K, l2.out_features) == int(form)
        with torch.no_grad():
            pkg.gated_gcn_block(x, csr, g1, g2, l1, l2)
    finally:
        os.environ.pop("GGCN_BLOCK_FORM", None)


def _bad_graphs(B):
    g = 4 * (B // 8)
    return [g, g + 1, g + 2, g + 3, B - 1]       # every staging pass of a tile, and the last tile


@pytest.mark.parametrize("form", FORMS, ids=["form8", "form4"])
@pytest.mark.parametrize("B,T", [(2048, 32), (2100, 29)])
def test_range_flag_of_the_large_batch_block(pkg, dev, B, T, form):
    """Clean data raises nothing; one activation of 1000 (outside the window |x| <= 448), of 7e4 or of inf in graph g raises the
    matching report -- for g % 4 in {0, 1, 2, 3} (every staging pass of a tile: the two groups of the eight-wavefront
    workgroup stage two each) and g = B - 1."""
    from ed_gated_gcn_amd import synth
    (w1, b1), (w2, b2) = synth.layer_params(768, 768, seed=1), synth.layer_params(768, 768, seed=2)
    x, csr, g1, g2, l1, l2 = _range_setup(pkg, dev, B, T, w1, b1, w2, b2, seed=B + T)
    l1.check_range()                                    # clears whatever earlier tests left
    _forward(pkg, x, csr, g1, g2, l1, l2, form)
    l1.check_range()
    for v, match in ((1000.0, r"left \|x\| <= 448"), (7.0e4, "reached fp16's range"), (float("inf"), "reached fp16's range")):
        for g in _bad_graphs(B):
            bad = x.clone()
            bad[g, T - 1, 767] = v
            _forward(pkg, bad, csr, g1, g2, l1, l2, form)
            with pytest.raises(RuntimeError, match=match):
                l1.check_range()
            l1.check_range()                            # reported once, cleared


@pytest.mark.parametrize("form", FORMS, ids=["form8", "form4"])
@pytest.mark.parametrize("B,T", [(2048, 32), (2100, 29)])
@pytest.mark.parametrize("which", ["W1", "W12"])
def test_hidden_value_bound_of_both_weight_images_on_every_row(pkg, dev, B, T, which, form):
    """The one-launch block must bound the hidden values of BOTH weight images on every row: max|x| * colsum|W1| (the W1
    tiles) and max|x| * colsum|W12| + max|mid| (the W12 tiles).  In the eight-wavefront kernel each row is split by ONE of
    the two groups (group 0: graphs 4t, 4t + 1 of a tile; group 1: 4t + 2, 4t + 3), so each group must judge its rows against
    both bounds.  An activation of 400 (inside the window) with colsum|W1| ~ 200 in graphs of group 1, and with colsum|W12|
    ~ 200 in graphs of group 0, must raise the hidden-value report, as the four-wavefront kernel does."""
    from ed_gated_gcn_amd import synth
    (w1, b1), (w2, b2) = synth.layer_params(768, 768, seed=1), synth.layer_params(768, 768, seed=2)
    w1_64, w2_64 = w1.astype(np.float64), w2.astype(np.float64)
    c12 = np.abs(w1_64 @ w2_64).sum(0).max()
    if which == "W1":                                  # colsum|W1| ~ 200, W12 = W1.W2 unchanged (small)
        s = 200.0 / np.abs(w1_64).sum(0).max()
        w1, w2 = (w1 * s).astype(np.float32), (w2 / s).astype(np.float32)
        rows = (2, 3)
    else:                                              # colsum|W1| small, colsum|W12| ~ 200
        w2 = (w2 * (200.0 / c12)).astype(np.float32)
        rows = (0, 1)
    c1 = np.abs(w1.astype(np.float64)).sum(0).max()
    c12 = np.abs(w1.astype(np.float64) @ w2.astype(np.float64)).sum(0).max()
    big, small = (c1, c12) if which == "W1" else (c12, c1)
    assert 400.0 * big > 65504 and 400.0 * small + 100.0 < 65504 and 4.0 * max(c1, c12) + 100.0 < 65504
    x, csr, g1, g2, l1, l2 = _range_setup(pkg, dev, B, T, w1, b1, w2, b2, seed=B + T + 1)
    l1.check_range()
    _forward(pkg, x, csr, g1, g2, l1, l2, form)
    l1.check_range()                                    # |x| <= 4: both bounds below 65504
    tiles = (B // 8, (B - 1) // 4)                       # a tile in the middle and the last one
    for t in tiles:
        for p in rows:
            g = 4 * t + p
            if g >= B:
                continue
            bad = x.clone()
            bad[g, T - 1, 767] = 400.0
            _forward(pkg, bad, csr, g1, g2, l1, l2, form)
            with pytest.raises(RuntimeError, match="hidden values"):
                l1.check_range()
            l1.check_range()


# ---------------------------------------------------------------- 4. the automatic precision under autograd
def test_automatic_precision_under_autograd_keeps_the_full_range(pkg, dev, golden_dir):
    """GatedGCNEventDetector keeps f16mx8 for gcn1 beyond the window (m1 > 448) only where the block runs as ONE launch (gc2
    never splits gcn1).  With autograd the block runs two launches: a training step with those weights takes bf16x3 and
    raises no range report, and the proof itself says bf16x3 whenever a gradient is wanted."""
    import types
    from oracle.ref_amir55 import BertAmir55Oracle, EncoderStandIn
    g = np.load(os.path.join(golden_dir, "amir55_full.npz"))
    oracle = BertAmir55Oracle(EncoderStandIn(int(g["seed_encoder"])), int(g["n_class"]))
    oracle.seeded_init(torch.Generator().manual_seed(int(g["seed_params"])))
    inputs = {k[3:]: torch.from_numpy(g[k]).to(dev) for k in g.files if k.startswith("in_")}
    opt = types.SimpleNamespace(device=dev, dropout=0.25, polarities_dim=int(g["n_class"]), ggcn_eval_logits_only=False)
    m = pkg.GatedGCNEventDetector(EncoderStandIn(int(g["seed_encoder"])), opt)
    m.load_state_dict(oracle.state_dict())
    m = m.to(dev)
    with torch.no_grad():                               # the window: 448 < m1 = max(colsum|W1| + |b1|) < 32752
        c1 = float((m.gc1.weight.abs().sum(0) + m.gc1.bias.abs()).max())
        s = 2000.0 / c1
        m.gc1.weight.mul_(s); m.gc1.bias.mul_(s)
        m.gc2.weight.mul_(1.0 / s)
    adj31 = inputs["dependency_graph"][:, :31, :31].contiguous()
    B = adj31.shape[0]
    x31 = torch.rand(B, 31, 2 * m.hidden_dim, device=dev) * 2 - 1
    csr31 = m.gc1._as_csr(adj31, x31)
    m.gc1.check_range()
    with torch.no_grad():
        assert m._proved_precision(csr31, x31) == "f16mx8"          # one launch: gcn1 is never split
    assert torch.is_grad_enabled()
    assert m._proved_precision(csr31, x31) == "bf16x3"              # the parameters want gradients: two launches
    assert m._proved_precision(csr31, x31.requires_grad_()) == "bf16x3"
    m.eval()
    with torch.no_grad():
        m(inputs)
    assert m._auto_precision and m.gc1.precision == "f16mx8"
    m.train()
    m.dropout.p = 0.0
    logits, xy, kl, scores = m(inputs)
    assert m.gc1.precision == m.gc2.precision == "bf16x3"
    (logits.sum() + sum(t.sum() for t in (xy, kl, scores) if torch.is_tensor(t))).backward()
    torch.cuda.synchronize()
    assert m.gc1.weight.grad is not None and bool(torch.isfinite(m.gc1.weight.grad).all())
    m.gc1.check_range()                                 # nothing tripped
