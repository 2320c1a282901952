"""The inference block on a REAL-valued adjacency of graphs of <= 32 nodes as ONE launch (``ggcn_block_fused_weighted`` on
``ggcn_graph_operands_weighted`` / ``ggcn_graph_operands2_weighted`` blocks; opt-in ``GraphConvolution.weighted_block``).  Run with
``-m gpu -s`` on an MI355X to see the figures.

1. the builder against float64 ``M @ M`` / ``rowsum(M)`` of the float32 ``M = w * inv``, per entry within
   ``2^-18 * sum_j |M_rj M_jc| + eps_plane * |M2_rc|`` (the fp32 chain of <= 32 terms plus the two-part split: eps = 2^-21 in fp16
   planes, 2^-16 in bf16 planes).  The bound has no absolute term, and the lo part of an fp16 pair has one (2^-25 of the scaled
   entry, fp16's subnormal spacing): it holds for entries whose ``sum_j |M_rj M_jc|`` is at least 2^-17, which the inputs are
   asserted to be;
2. the builder's flag: an adjacency whose M fits fp16 planes and whose M^2 does not keeps today's launches and today's bits;
3. the block against the float64 oracle at the project's parity gate, ``1e-4 * max(1, max|ref|)`` per output, the C entry called
   with NaN-filled outputs between poisoned guard bands; the distance to the option-off result is printed, not gated;
4. the forms: ``want=``, ``want_gcn1``, ``dense_head=``, which entries ran, and what turns the option's launch off;
5. the C entry directly: absent outputs, leading dimensions above F, the eval form without layer 1's operands;
6. the f16mx8 range report on the new launch;
7. the classifier in ``eval()`` on a signed dependency graph.
"""
import types

import numpy as np
import pytest
import torch

from oracle import ref_dense
from oracle.gates import poisoned_rows
from oracle.gpu_support import clean_range_flag, count_calls, dev, make_layer, pkg, range_bits as _bits  # noqa: F401

pytestmark = pytest.mark.gpu

GATE = 1e-4                      # oracle/backward_ref.py TOL: the same for both precisions
OPS2_BYTES = 4224                # include/ggcn.h GGCN_GRAPH_OPS2_BYTES
BLOCK, LAYER_W, BUILD_M, BUILD_M2 = ("ggcn_block_fused_weighted", "ggcn_layer_fused_weighted", "ggcn_graph_operands_weighted",
                                     "ggcn_graph_operands2_weighted")
COUNTED = (BLOCK, LAYER_W, BUILD_M, BUILD_M2, "ggcn_gate_overlap", "ggcn_overlap_reduce", "ggcn_dense_head", "ggcn_block_fused",
           "ggcn_linear", "ggcn_aggregate")
OUTPUTS = ("x1", "y1", "xy", "x", "out")
GUARD = 4096                     # floats of poison on either side of every output of the direct calls


@pytest.fixture(autouse=True)
def clean_flag(pkg, dev):
    """Every test starts and ends with the range flag clear (some of the inputs below leave the fp16 window on purpose)."""
    yield from clean_range_flag(pkg, dev)


def _adjacency(B, T, kind, rng, lens):
    """The three kinds of tests/test_gpu_weighted_wide.py: float32 [B,T,T], zero outside each graph's length: sparse / signed =
    dependency trees x U(0.05, 2) weights (signed: 20 % of them x -0.25), dense = a row-softmax of standard normals."""
    from ed_gated_gcn_amd import synth
    if kind == "dense":
        a = np.zeros((B, T, T), dtype=np.float32)
        for g, n in enumerate(lens):
            z = rng.standard_normal((n, n))
            e = np.exp(z - z.max(1, keepdims=True))
            a[g, :n, :n] = (e / e.sum(1, keepdims=True)).astype(np.float32)
        return a
    a = synth.dependency_batch(B, T, 3.0, seed=B + T, lengths=lens).astype(np.float32)
    wts = rng.uniform(0.05, 2.0, size=a.shape).astype(np.float32)
    if kind == "signed":
        wts *= np.where(rng.random(a.shape) < 0.2, -0.25, 1.0).astype(np.float32)
    return a * wts


def _lengths(rng, B, T):
    lens = rng.integers(max(1, T // 3), T + 1, size=B)
    lens[0] = T
    return lens


def _layers(pkg, dev, params, precision, block=True):
    return [make_layer(pkg, dev, w, b, opt=types.SimpleNamespace(ggcn_precision=precision, ggcn_weighted_block=block)) for w, b in params]


# ================================================================ 1. the builder
def _decode(ops, B, plane):
    """``(M2 [B,32,32], rowsum [B,32])`` as float64 out of ``ggcn_graph_operands2`` blocks: (hi + lo) / 2^10 and the rowsum field."""
    raw = ops.cpu().numpy().reshape(B, OPS2_BYTES)
    frag = np.ascontiguousarray(raw[:, :4096]).view(np.uint16).reshape(B, 2, 2, 64, 8)          # [graph][hi / lo][k-step][lane][element]
    if plane == 1:
        val = frag.view(np.float16).astype(np.float64)
    else:
        val = (frag.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    s, lane, j = np.meshgrid(np.arange(2), np.arange(64), np.arange(8), indexing="ij")
    row, col = lane & 31, 16 * s + 8 * (j >> 2) + 4 * (lane >> 5) + (j & 3)
    m2 = np.full((B, 32, 32), np.nan)
    m2[:, row, col] = (val[:, 0] + val[:, 1]) / 1024.0
    field = np.ascontiguousarray(raw[:, 4096:]).view(np.float32).reshape(B, 32).astype(np.float64)
    idx = np.arange(32)
    rows = (idx & 3) + 8 * ((idx & 15) >> 2) + 4 * (idx >> 4)
    rowsum = np.full((B, 32), np.nan)
    rowsum[:, rows] = field
    return m2, rowsum


def _m_float32(adj):
    """M = w * inv as the builders compute it: a row's weights summed in CSR (column) order in float32, one IEEE division."""
    wsum = np.zeros(adj.shape[:2], dtype=np.float32)
    for j in range(adj.shape[2]):
        wsum = (wsum + adj[:, :, j]).astype(np.float32)
    inv = (np.float32(1.0) / (wsum + np.float32(1.0))).astype(np.float32)
    return (adj * inv[:, :, None]).astype(np.float32)


def _build(pkg, dev, csr, plane, vals=True, flag=None):
    """``ggcn_graph_operands2_weighted`` into a buffer of exactly ``ggcn_graph_operands2_bytes(B)`` bytes, every byte 0xFF (NaN in
    every format) beforehand, between two poisoned guard bands."""
    from ed_gated_gcn_amd import _capi
    lib = pkg.load_library()
    n = lib.ggcn_graph_operands2_bytes(csr.B)
    assert n == csr.B * OPS2_BYTES
    buf = torch.full((n + 2 * 4096,), 0xFF, dtype=torch.uint8, device=dev)
    ops = buf[4096:4096 + n]
    _capi.check(lib.ggcn_graph_operands2_weighted(_capi.ptr(csr.rowptr), _capi.ptr(csr.colidx), _capi.ptr(csr.vals if vals else None),
                                                  csr.B, csr.T, plane, _capi.ptr(ops), _capi.ptr(flag), _capi.stream_of(dev)), BUILD_M2)
    torch.cuda.synchronize()
    assert bool((buf[:4096] == 0xFF).all()) and bool((buf[4096 + n:] == 0xFF).all()), "the builder wrote outside its blocks"
    return ops


@pytest.mark.parametrize("plane", [0, 1])
@pytest.mark.parametrize("kind", ["sparse", "signed", "dense"])
@pytest.mark.parametrize("B,T", [(1, 1), (5, 32), (6, 17), (7, 9)])
def test_builder_vs_float64(pkg, dev, B, T, kind, plane):
    rng = np.random.default_rng(B * 1000 + T)
    adj = _adjacency(B, T, kind, rng, _lengths(rng, B, T))
    csr = pkg.BatchedCSR.from_dense(torch.from_numpy(adj).to(dev), binary=False)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ops = _build(pkg, dev, csr, plane, flag=flag)
    again = _build(pkg, dev, csr, plane)
    assert torch.equal(ops, again), "two calls differ: the summation order is not fixed"
    assert int(flag.item()) == 0
    m2, rowsum = _decode(ops, B, plane)
    assert not np.isnan(m2).any() and not np.isnan(rowsum).any(), "a byte of the blocks was not written"
    assert (m2[:, T:, :] == 0).all() and (m2[:, :, T:] == 0).all() and (rowsum[:, T:] == 0).all(), "rows / columns >= T are not zero"
    m = _m_float32(adj).astype(np.float64)
    ref, terms = m @ m, np.abs(m) @ np.abs(m)
    assert terms[terms > 0].min() >= 2.0 ** -17              # (the module docstring: where the bound applies to fp16 pairs)
    eps = 2.0 ** -21 if plane == 1 else 2.0 ** -16
    bound = 2.0 ** -18 * terms + eps * np.abs(ref)
    err = np.abs(m2[:, :T, :T] - ref)
    rs_ref, rs_bound = m.sum(2), 2.0 ** -18 * np.abs(m).sum(2)   # an fp32 chain of <= 32 terms, stored as float32
    rs_err = np.abs(rowsum[:, :T] - rs_ref)
    worst = float((err / np.where(bound > 0, bound, 1.0)).max())
    print("%dx%d %s plane %d: max err %.3g, worst err / bound %.3g; rowsum max err %.3g (bound %.3g)" % (
        B, T, kind, plane, err.max(), worst, rs_err.max(), rs_bound.max()))
    assert (err <= bound).all(), "M2: %d entries beyond the bound, worst err / bound %.3g" % (int((err > bound).sum()), worst)
    assert (rs_err <= rs_bound).all()


@pytest.mark.parametrize("plane", [0, 1])
def test_builder_without_values_means_ones(pkg, dev, plane):
    B, T = 6, 17
    rng = np.random.default_rng(5)
    adj = _adjacency(B, T, "sparse", rng, _lengths(rng, B, T))
    csr = pkg.BatchedCSR.from_dense(torch.from_numpy(adj).to(dev), binary=False)
    m2, rowsum = _decode(_build(pkg, dev, csr, plane, vals=False), B, plane)
    m = _m_float32((adj != 0).astype(np.float32)).astype(np.float64)
    ref, terms = m @ m, np.abs(m) @ np.abs(m)
    bound = 2.0 ** -18 * terms + (2.0 ** -21 if plane == 1 else 2.0 ** -16) * np.abs(ref)
    assert (np.abs(m2[:, :T, :T] - ref) <= bound).all() and (np.abs(rowsum[:, :T] - m.sum(2)) <= 2.0 ** -18 * np.abs(m).sum(2)).all()
    assert (m2[:, T:, :] == 0).all() and (m2[:, :, T:] == 0).all() and (rowsum[:, T:] == 0).all()


# ================================================================ 2. the builder's flag
def _block_inputs(rng, B, T, K, F, bias=True, seeds=(1, 2)):
    from ed_gated_gcn_amd import synth
    x = rng.standard_normal((B, T, K)).astype(np.float32)
    g1, g2 = (torch.sigmoid(torch.from_numpy(rng.standard_normal((B, F)).astype(np.float32))) for _ in range(2))
    (w1, b1), (w2, b2) = synth.layer_params(K, F, seed=seeds[0]), synth.layer_params(F, F, seed=seeds[1])
    if not bias:
        b1 = b2 = None
    return x, g1, g2, ((w1, b1), (w2, b2))


def _oracle(x, adj, g1, g2, params):
    (w1, b1), (w2, b2) = params
    t = lambda a: None if a is None else torch.as_tensor(a).double()   # noqa: E731
    ref = ref_dense.gated_block(t(x), t(adj), t(g1), t(g2), t(w1), t(b1), t(w2), t(b2), dtype=torch.float64)
    assert ref["out"].dtype == torch.float64
    return ref


def _check(got, ref, keys, what):
    """Every named output inside ``GATE * max(1, max|ref|)`` of the float64 reference; returns the printed figures."""
    figures = []
    for k in keys:
        g, r = got[k], ref[k]
        assert g is not None and g.dtype == torch.float32 and tuple(g.shape) == tuple(r.shape), (what, k)
        tol = GATE * max(1.0, float(r.abs().max()))
        err = float((g.double().cpu() - r).abs().max())
        figures.append("%s %.3g/%.3g" % (k, err, tol))
        assert err == err and err <= tol, "%s %s: max|diff| %.3g > %.3g" % (what, k, err, tol)
    return ", ".join(figures)


def _extreme(dev, rows):
    """Three 2-node graphs; graph 1 holds ``rows``, the others ordinary weights."""
    adj = np.zeros((3, 2, 2), dtype=np.float32)
    adj[0] = [[0.5, 0.25], [0.0, 1.5]]
    adj[1] = rows
    adj[2] = [[0.0, 0.75], [1.25, 0.5]]
    return adj


def test_m_fits_fp16_planes_and_its_square_does_not(pkg, dev, monkeypatch):
    """adj[0][1] = adj[1][0] = -31/32: rowsum + 1 = 1/32, M = -31 (times 2^10: inside fp16), M^2 = 961 (times 2^10: outside)."""
    adj = _extreme(dev, [[0.0, -31.0 / 32.0], [-31.0 / 32.0, 0.0]])
    B, T, K, F = 3, 2, 64, 64
    x, g1, g2, params = _block_inputs(np.random.default_rng(2), B, T, K, F)
    xd, ad, g1d, g2d = torch.from_numpy(x).to(dev), torch.from_numpy(adj).to(dev), g1.to(dev), g2.to(dev)
    ref = _oracle(x, adj, g1, g2, params)
    calls = count_calls(monkeypatch, COUNTED)
    # fp16 planes: M has its operand, M^2 has none -> today's two weighted layer launches, today's bits
    on, off = _layers(pkg, dev, params, "f16mx8"), _layers(pkg, dev, params, "f16mx8", block=False)
    csr = pkg.BatchedCSR.from_dense(ad)
    assert not csr.is_binary and csr.graph_ops_weighted(1) is not None and csr.graph_ops2_weighted(1) is None
    assert calls[BUILD_M2] == 1 and csr.graph_ops2_weighted(1) is None and calls[BUILD_M2] == 1      # the refusal is cached too
    assert not pkg.gated_block.takes_weighted_block_path(xd, csr, *on)
    for k in calls:
        calls[k] = 0
    with torch.no_grad():
        r_on = pkg.gated_gcn_block(xd, csr, g1d, g2d, *on, want_gcn1=True)
        assert calls[BLOCK] == 0 and calls[LAYER_W] == 2 and calls["ggcn_gate_overlap"] == 1, calls
        r_off = pkg.gated_gcn_block(xd, csr, g1d, g2d, *off, want_gcn1=True)
    torch.cuda.synchronize()
    for k in OUTPUTS + ("gcn1",):
        assert torch.equal(r_on[k], r_off[k]), k
    # bf16 planes hold 961 * 2^10: the flag stays clear and the new launch runs, inside the gate
    on = _layers(pkg, dev, params, "bf16x3")
    assert csr.graph_ops2_weighted(0) is not None and pkg.gated_block.takes_weighted_block_path(xd, csr, *on)
    for k in calls:
        calls[k] = 0
    with torch.no_grad():
        r = pkg.gated_gcn_block(xd, csr, g1d, g2d, *on, want_gcn1=True)
    torch.cuda.synchronize()
    assert calls[BLOCK] == 1 and calls[LAYER_W] == 0, calls
    print("M = -31, bf16x3:", _check(r, ref, OUTPUTS + ("gcn1",), "M = -31 bf16x3"))


def test_a_row_with_rowsum_minus_one_is_refused_in_both_planes(pkg, dev):
    adj = _extreme(dev, [[-0.5, -0.5], [0.25, 0.5]])          # rowsum + 1 == 0: 1 / 0
    csr = pkg.BatchedCSR.from_dense(torch.from_numpy(adj).to(dev))
    for plane in (0, 1):
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        _build(pkg, dev, csr, plane, flag=flag)
        assert int(flag.item()) == 1
        assert csr.graph_ops2_weighted(plane) is None
    params = _block_inputs(np.random.default_rng(2), 3, 2, 64, 64)[3]
    for precision in ("bf16x3", "f16mx8"):
        assert not pkg.gated_block.takes_weighted_block_path(torch.zeros(3, 2, 64, device=dev), csr, *_layers(pkg, dev, params, precision))


# ================================================================ 3. the block against float64
CASES = [(9, 32, 64, 256, "sparse"),     # whole tiles (LDS-DMA staged operands in f16mx8) and a one-graph tail tile
         (4, 32, 256, 256, "dense"),     # every row of every tile a real node: the unguarded form
         (5, 17, 34, 100, "signed"),     # general main loop, column guard, scalar row stores
         (3, 1, 32, 64, "sparse"),       # one-node graphs
         (6, 31, 768, 768, "dense"),     # three column tiles
         (2, 24, 33, 64, "signed")]      # K % 4 != 0
_CASE = {}     # case -> inputs and the float64 reference, computed once and left unchanged


def _case(B, T, K, F, kind, bias):
    key = (B, T, K, F, kind, bias)
    if key not in _CASE:
        rng = np.random.default_rng(B * 1000 + T)
        adj = _adjacency(B, T, kind, rng, _lengths(rng, B, T))
        x, g1, g2, params = _block_inputs(rng, B, T, K, F, bias)
        _CASE[key] = types.SimpleNamespace(B=B, T=T, K=K, F=F, x=x, adj=adj, g1=g1, g2=g2, params=params, ref=_oracle(x, adj, g1, g2, params))
    return _CASE[key]


def _direct(pkg, dev, c, layers, xd, csr, g1d, g2d, outputs=("x1", "y1", "xy", "x", "out", "gcn1"), ld1=None, ld2=None, eval_operands=True):
    """``ggcn_block_fused_weighted`` called directly on NaN-filled outputs between poisoned guard bands.  ``outputs`` names what is
    handed in (the rest is NULL); ``eval_operands=False`` (the eval form) passes NULL for graph_opsw, wpack1, gate1 and zero_mid.
    Returns the outputs as the public call shapes them; checks that no NaN survives where a result belongs and that nothing else
    was written."""
    from ed_gated_gcn_amd import _capi, gated_block
    lib, ptr = pkg.load_library(), _capi.ptr
    gc1, gc2 = layers
    B, T, K, F = c.B, c.T, c.K, c.F
    ld1, ld2 = ld1 or F, ld2 or F
    plane = 0 if gc1.precision == "bf16x3" else 1
    layer1 = any(k in outputs for k in ("x1", "y1", "xy", "gcn1"))
    shapes = {"gcn1": (B * T, ld1), "x": (B * T, ld2), "x1": (B, F), "y1": (B, F), "out": (B, F), "xy": (B, (F + 63) // 64)}
    bufs = {k: poisoned_rows(dev, rows, ld, GUARD) for k, (rows, ld) in shapes.items()}
    arg = {k: (bufs[k][1] if k in outputs else None) for k in bufs}
    x2d = xd.view(B * T, K)
    with torch.cuda.device(dev):
        st = _capi.stream_of(dev)
        pack1, pack12, mid = gated_block._block_operands(gc1, gc2, lib, st, precision=gc1.precision)
        keep1 = layer1 or eval_operands
        b1 = None if gc1.bias is None else gc1.bias.detach()
        b2 = None if gc2.bias is None else gc2.bias.detach()
        rc = lib.ggcn_block_fused_weighted(ptr(x2d), K, ptr(pack1 if keep1 else None), ptr(pack12),
                                           ptr(csr.graph_ops_weighted(plane) if keep1 else None), ptr(csr.graph_ops2_weighted(plane)),
                                           ptr(b1), ptr(mid), ptr(b2), ptr(gc1._zero_row(F, dev) if keep1 else None), B, T, K, F,
                                           ptr(g1d if keep1 else None), ptr(g2d), ptr(arg["gcn1"]), ld1, ptr(arg["x"]), ld2,
                                           ptr(arg["x1"]), ptr(arg["y1"]), ptr(arg["out"]), ptr(arg["xy"]), _capi.PREC[gc1.precision], st)
        _capi.check(rc, BLOCK)
        xy = None
        if "xy" in outputs:
            xy = torch.empty((), dtype=torch.float32, device=dev)
            _capi.check(lib.ggcn_overlap_reduce(ptr(arg["xy"]), B, F, ptr(xy), st), "ggcn_overlap_reduce")
    torch.cuda.synchronize()
    res = {"xy": xy}
    for k, (buf, view) in bufs.items():
        width = (F + 63) // 64 if k == "xy" else F
        nan = torch.isnan(buf)
        assert bool(nan[:GUARD].all()) and bool(nan[-GUARD:].all()), "%s: a guard band was written" % k
        if k not in outputs:
            assert bool(nan.all()), "%s was not asked for and was written" % k
            res.setdefault(k, None)
            continue
        assert not bool(torch.isnan(view[:, :width]).any()), "%s: a NaN survived where a result belongs" % k
        assert bool(torch.isnan(view[:, width:]).all()), "%s: columns beyond F were written" % k
        if k != "xy":
            val = view[:, :width].contiguous()
            res[k] = val.view(B, T, F) if k in ("gcn1", "x") else val
    return res


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("precision", ["bf16x3", "f16mx8"])
@pytest.mark.parametrize("B,T,K,F,kind", CASES)
def test_block_vs_float64_oracle(pkg, dev, monkeypatch, B, T, K, F, kind, precision, bias):
    c = _case(B, T, K, F, kind, bias)
    xd, ad, g1d, g2d = torch.from_numpy(c.x).to(dev), torch.from_numpy(c.adj).to(dev), c.g1.to(dev), c.g2.to(dev)
    on, off = _layers(pkg, dev, c.params, precision), _layers(pkg, dev, c.params, precision, block=False)
    csr = pkg.BatchedCSR.from_dense(ad)
    assert not csr.is_binary and pkg.gated_block.takes_weighted_block_path(xd, csr, *on)
    assert not pkg.gated_block.takes_weighted_block_path(xd, csr, *off)
    calls = count_calls(monkeypatch, COUNTED)
    with torch.no_grad():
        r = pkg.gated_gcn_block(xd, csr, g1d, g2d, *on, want_gcn1=True)
        assert calls[BLOCK] == 1 and calls[LAYER_W] == 0 and calls["ggcn_block_fused"] == 0, calls
        r_off = pkg.gated_gcn_block(xd, csr, g1d, g2d, *off, want_gcn1=True)
        assert calls[BLOCK] == 1 and calls[LAYER_W] == 2, calls
    torch.cuda.synchronize()
    what = "%dx%dx%dx%d %s %s %s" % (B, T, K, F, kind, precision, "bias" if bias else "no bias")
    keys = OUTPUTS + ("gcn1",)
    figures = _check(r, c.ref, keys, what)
    apart = max(float((r[k] - r_off[k]).abs().max()) for k in keys)
    print("%s | vs float64 (err/gate): %s | vs the option off: %.3g" % (what, figures, apart))
    # the C entry itself on NaN-filled outputs between guard bands: the public call's bits, nothing written outside
    d = _direct(pkg, dev, c, on, xd, csr, g1d, g2d)
    for k in keys:
        assert torch.equal(d[k], r[k]), "%s %s: the direct call differs from the public one" % (what, k)
    if precision == "f16mx8":
        assert _bits(pkg, dev) == 0, "clean data raised the range flag"


@pytest.mark.parametrize("B,T,K,F,form", [(2048, 32, 256, 256, None), (1024, 32, 64, 768, 8)])
def test_block_on_large_batches_never_takes_the_eight_wavefront_kernel(pkg, dev, monkeypatch, B, T, K, F, form):
    """Large batches, f16mx8, every output: where ``ggcn_block_fused`` runs its eight-wavefront kernel, which reads the 0/1 operand
    format, the weighted launch must not.  2048 x 32 x 256 x 256 is 512 workgroups per part, two per CU of an MI355X (the 0/1 block
    keeps four wavefronts there: ``ggcn_block_fused_form``); 1024 x 32 x 64 x 768 is the smallest batch that block does hand to the
    eight-wavefront kernel (three whole rounds of the 256 CUs).  Eight graphs spread over the batch against the oracle."""
    monkeypatch.delenv("GGCN_BLOCK_FORM", raising=False)
    if form is not None:
        assert pkg.load_library().ggcn_block_fused_form(B, T, K, F) == form
    rng = np.random.default_rng(B)
    adj = _adjacency(B, T, "sparse", rng, _lengths(rng, B, T))
    x, g1, g2, params = _block_inputs(rng, B, T, K, F)
    xd, ad, g1d, g2d = torch.from_numpy(x).to(dev), torch.from_numpy(adj).to(dev), g1.to(dev), g2.to(dev)
    on = _layers(pkg, dev, params, "f16mx8")
    calls = count_calls(monkeypatch, COUNTED)
    with torch.no_grad():
        r = pkg.gated_gcn_block(xd, ad, g1d, g2d, *on)
    torch.cuda.synchronize()
    assert calls[BLOCK] == 1 and calls["ggcn_block_fused"] == 0 and calls[LAYER_W] == 0, calls
    for k in ("x1", "y1", "x", "out"):
        assert bool(torch.isfinite(r[k]).all()), k
    pick = [0, 3, B // 4 - 1, B // 2, B // 2 + 1, B - 49, B - 2, B - 1]
    ref = _oracle(x[pick], adj[pick], g1[pick], g2[pick], params)
    got = {k: r[k][pick] for k in ("x1", "y1", "x", "out")}
    print("%dx%dx%dx%d sparse f16mx8, 8 graphs:" % (B, T, K, F), _check(got, ref, ("x1", "y1", "x", "out"), "%d graphs" % B))
    xy64 = float((r["x1"].double() * r["y1"].double()).sum(1).mean())
    assert abs(float(r["xy"]) - xy64) <= GATE * max(1.0, abs(xy64))      # the regulariser over the whole batch, from the kernel's own pools
    assert _bits(pkg, dev) == 0


# ================================================================ 4. the forms
@pytest.mark.parametrize("precision", ["bf16x3", "f16mx8"])
def test_forms_and_which_launches_ran(pkg, dev, monkeypatch, precision):
    c = _case(9, 32, 64, 256, "sparse", True)
    xd, ad, g1d, g2d = torch.from_numpy(c.x).to(dev), torch.from_numpy(c.adj).to(dev), c.g1.to(dev), c.g2.to(dev)
    on = _layers(pkg, dev, c.params, precision)
    calls = count_calls(monkeypatch, COUNTED)
    with torch.no_grad():
        full = pkg.gated_gcn_block(xd, ad, g1d, g2d, *on)
        assert calls[BLOCK] == 1 and calls[LAYER_W] == 0 and calls["ggcn_gate_overlap"] == 0 and calls["ggcn_overlap_reduce"] == 1, calls
        assert calls[BUILD_M] == 1 and calls[BUILD_M2] == 1, calls
        assert full["gcn1"] is None
        ev = pkg.gated_gcn_block(xd, ad, g1d, g2d, *on, want=("out",))          # the same adjacency tensor: the builders' blocks are cached
        assert calls[BLOCK] == 2 and calls[BUILD_M] == 1 and calls[BUILD_M2] == 1 and calls["ggcn_overlap_reduce"] == 1, calls
        ex = pkg.gated_gcn_block(xd, ad, g1d, g2d, *on, want=("x", "out"))
        wg = pkg.gated_gcn_block(xd, ad, g1d, g2d, *on, want_gcn1=True)
        assert calls[BLOCK] == 4 and calls[LAYER_W] == 0 and calls["ggcn_aggregate"] == 0, calls
    torch.cuda.synchronize()
    assert torch.equal(ev["out"], full["out"]) and all(ev[k] is None for k in ("x1", "y1", "xy", "x", "gcn1"))
    assert torch.equal(ex["out"], full["out"]) and torch.equal(ex["x"], full["x"]) and all(ex[k] is None for k in ("x1", "y1", "xy"))
    _check(full, c.ref, OUTPUTS, "all outputs")
    _check(wg, c.ref, OUTPUTS + ("gcn1",), "want_gcn1")
    # a fresh adjacency tensor, the eval form first
    ad2 = ad.clone()
    for k in calls:
        calls[k] = 0
    with torch.no_grad():
        ev2 = pkg.gated_gcn_block(xd, ad2, g1d, g2d, *on, want=("out",))
    assert torch.equal(ev2["out"], full["out"]) and calls[BLOCK] == 1 and calls[BUILD_M2] == 1, calls


@pytest.mark.parametrize("precision", ["bf16x3", "f16mx8"])
def test_dense_head_finishes_xy_two_launches_in_all(pkg, dev, monkeypatch, precision):
    c = _case(5, 17, 34, 100, "signed", True)
    xd, ad, g1d, g2d = torch.from_numpy(c.x).to(dev), torch.from_numpy(c.adj).to(dev), c.g1.to(dev), c.g2.to(dev)
    rng = np.random.default_rng(11)
    wt = torch.from_numpy((rng.standard_normal((c.F, 34)) / 10).astype(np.float32))
    hb = torch.from_numpy(rng.standard_normal(34).astype(np.float32))
    on = _layers(pkg, dev, c.params, precision)
    csr = pkg.BatchedCSR.from_dense(ad)
    head = (wt.to(dev), hb.to(dev))
    with torch.no_grad():
        pkg.gated_gcn_block(xd, csr, g1d, g2d, *on, dense_head=head)     # folds W12 and builds the graph's operands: once per weights / adjacency
    calls = count_calls(monkeypatch, COUNTED)
    with torch.no_grad():
        r = pkg.gated_gcn_block(xd, csr, g1d, g2d, *on, dense_head=head)
    torch.cuda.synchronize()
    assert {k: v for k, v in calls.items() if v} == {BLOCK: 1, "ggcn_dense_head": 1}, calls
    ref = dict(c.ref, logits=c.ref["out"] @ wt.double() + hb.double())
    print("dense_head %s:" % precision, _check(r, ref, OUTPUTS + ("logits",), "dense_head"))


@pytest.mark.parametrize("precision", ["bf16x3", "f16mx8"])
def test_what_keeps_todays_launches_and_todays_bits(pkg, dev, monkeypatch, precision):
    c = _case(5, 17, 34, 100, "signed", True)
    xd, ad, g1d, g2d = torch.from_numpy(c.x).to(dev), torch.from_numpy(c.adj).to(dev), c.g1.to(dev), c.g2.to(dev)
    on, off = _layers(pkg, dev, c.params, precision), _layers(pkg, dev, c.params, precision, block=False)
    calls = count_calls(monkeypatch, COUNTED)
    with torch.no_grad():
        base = pkg.gated_gcn_block(xd, ad, g1d, g2d, *off, want_gcn1=True)
        base_eval = pkg.gated_gcn_block(xd, ad, g1d, g2d, *off, want=("x", "out"))
        assert calls[BLOCK] == 0 and calls[BUILD_M2] == 0 and calls[LAYER_W] == 4 and calls["ggcn_gate_overlap"] == 1, calls
        two = pkg.gated_gcn_block(xd, ad, g1d, g2d, *on, want_gcn1=True, one_launch=False)
        two_eval = pkg.gated_gcn_block(xd, ad, g1d, g2d, *on, want=("x", "out"), one_launch=False)
        assert calls[BLOCK] == 0 and calls[BUILD_M2] == 0 and calls[LAYER_W] == 8, calls
    for k in OUTPUTS + ("gcn1",):
        assert torch.equal(two[k], base[k]), k
    assert torch.equal(two_eval["out"], base_eval["out"]) and torch.equal(two_eval["x"], base_eval["x"])
    # an adjacency that wants its gradient: under autograd, the layers
    for layers in (on, off):
        for m in layers:
            m.requires_grad_(False)
    ag = ad.clone().requires_grad_(True)
    r_on = pkg.gated_gcn_block(xd, ag, g1d, g2d, *on)
    assert calls[BLOCK] == 0 and calls[BUILD_M2] == 0, calls
    r_off = pkg.gated_gcn_block(xd, ag, g1d, g2d, *off)
    torch.cuda.synchronize()
    assert r_on["out"].requires_grad
    for k in OUTPUTS + ("gcn1",):
        assert torch.equal(r_on[k].detach(), r_off[k].detach()), k
    # ... and with autograd switched off the same tensor takes the one launch
    with torch.no_grad():
        pkg.gated_gcn_block(xd, ag, g1d, g2d, *on)
    assert calls[BLOCK] == 1, calls


# ================================================================ 5. the C entry directly
@pytest.mark.parametrize("precision", ["bf16x3", "f16mx8"])
def test_c_entry_forms(pkg, dev, precision):
    for B, T, K, F, kind in ((9, 32, 64, 256, "sparse"), (5, 17, 34, 100, "signed")):
        c = _case(B, T, K, F, kind, True)
        xd, ad, g1d, g2d = torch.from_numpy(c.x).to(dev), torch.from_numpy(c.adj).to(dev), c.g1.to(dev), c.g2.to(dev)
        on = _layers(pkg, dev, c.params, precision)
        csr = pkg.BatchedCSR.from_dense(ad)
        full = _direct(pkg, dev, c, on, xd, csr, g1d, g2d)
        what = "%dx%d %s" % (B, T, precision)
        _check(full, c.ref, OUTPUTS + ("gcn1",), what)
        no_x = _direct(pkg, dev, c, on, xd, csr, g1d, g2d, outputs=("x1", "y1", "xy", "out"))           # x_out = NULL with pool_out
        no_pool = _direct(pkg, dev, c, on, xd, csr, g1d, g2d, outputs=("x1", "y1", "xy", "x"))          # pool_out = NULL with x_out
        wide = _direct(pkg, dev, c, on, xd, csr, g1d, g2d, ld1=F + 12, ld2=F + 8)                      # leading dimensions above F
        odd = _direct(pkg, dev, c, on, xd, csr, g1d, g2d, ld1=F + 3, ld2=F + 1)                        # ... that rule out 16-byte row stores
        ev = _direct(pkg, dev, c, on, xd, csr, g1d, g2d, outputs=("x", "out"), eval_operands=False)    # the eval form, layer 1's operands NULL
        ev_pool = _direct(pkg, dev, c, on, xd, csr, g1d, g2d, outputs=("out",), eval_operands=False)
        for k in ("x1", "y1", "xy", "out"):
            assert torch.equal(no_x[k], full[k]), (what, k)
        for k in ("x1", "y1", "xy", "x"):
            assert torch.equal(no_pool[k], full[k]), (what, k)
        for k in OUTPUTS + ("gcn1",):
            assert torch.equal(wide[k], full[k]) and torch.equal(odd[k], full[k]), (what, k)
        assert torch.equal(ev["x"], full["x"]) and torch.equal(ev["out"], full["out"]) and torch.equal(ev_pool["out"], full["out"]), what


def test_c_entry_refuses_misaligned_blocks(pkg, dev):
    from ed_gated_gcn_amd import _capi
    c = _case(5, 17, 34, 100, "signed", True)
    xd, ad, g1d, g2d = torch.from_numpy(c.x).to(dev), torch.from_numpy(c.adj).to(dev), c.g1.to(dev), c.g2.to(dev)
    on = _layers(pkg, dev, c.params, "f16mx8")
    csr = pkg.BatchedCSR.from_dense(ad)
    good = {"w": csr.graph_ops_weighted(1), "w2": csr.graph_ops2_weighted(1)}
    lib = pkg.load_library()
    for which in ("w", "w2"):
        shifted = torch.empty(good[which].numel() + 16, dtype=torch.uint8, device=dev)[4:4 + good[which].numel()].copy_(good[which])
        assert shifted.data_ptr() % 16 == 4
        stand_in = types.SimpleNamespace(graph_ops_weighted=lambda p, w=which: shifted if w == "w" else good["w"],
                                         graph_ops2_weighted=lambda p, w=which: shifted if w == "w2" else good["w2"])
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            _direct(pkg, dev, c, on, xd, stand_in, g1d, g2d)
        assert lib.ggcn_last_error().decode().startswith(BLOCK + ":")
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.empty(csr.B * OPS2_BYTES + 16, dtype=torch.uint8, device=dev)[4:]
    rc = lib.ggcn_graph_operands2_weighted(_capi.ptr(csr.rowptr), _capi.ptr(csr.colidx), _capi.ptr(csr.vals), csr.B, csr.T, 1, _capi.ptr(out),
                                           _capi.ptr(flag), _capi.stream_of(dev))
    assert rc == 1 and lib.ggcn_last_error().decode().startswith(BUILD_M2 + ":")


# ================================================================ 6. the range report
def test_range_report_on_the_new_launch(pkg, dev, monkeypatch):
    B, T, K, F = 5, 17, 64, 64
    rng = np.random.default_rng(17)
    lens = _lengths(rng, B, T)
    lens[-1] = T                                             # the last row of the last graph is a real node
    adj = _adjacency(B, T, "sparse", rng, lens)
    x, g1, g2, params = _block_inputs(rng, B, T, K, F)
    ad, g1d, g2d = torch.from_numpy(adj).to(dev), g1.to(dev), g2.to(dev)
    calls = count_calls(monkeypatch, COUNTED)
    for precision in ("f16mx8", "bf16x3"):
        on = _layers(pkg, dev, params, precision)
        for value, word in ((None, None), (450.0, "window"), (65504.0, "65504 or infinite")):
            xd = torch.from_numpy(x).to(dev)
            if value is not None:
                xd[B - 1, T - 1, K - 1] = value
            before = calls[BLOCK]
            with torch.no_grad():
                pkg.gated_gcn_block(xd, ad, g1d, g2d, *on)
            assert calls[BLOCK] == before + 1
            if precision == "f16mx8" and value is not None:
                with pytest.raises(RuntimeError, match=word) as e:
                    on[0].check_range()
                assert "f16mx8" in str(e.value)
                if value == 450.0:
                    assert "65504 or infinite" not in str(e.value), "an element inside fp16's range reported an overflow"
            on[0].check_range()                              # clean data, bf16x3, or already reported: nothing is raised


# ================================================================ 7. the classifier
def test_classifier_in_eval_on_a_signed_graph(pkg, dev, monkeypatch):
    from ed_gated_gcn_amd import synth

    class _Bert(torch.nn.Module):
        def forward(self, ids, seg, output_all_encoded_layers=True):
            gen = torch.Generator(device=ids.device).manual_seed(1)
            return ([torch.randn(ids.shape[0], ids.shape[1], 768, device=ids.device, generator=gen) for _ in range(12)],
                    torch.zeros(ids.shape[0], 768, device=ids.device))
    B, ORI_ML, BERT_ML = 16, 31, 60
    rng = np.random.default_rng(0)
    sent_len = rng.integers(5, ORI_ML + 1, size=B)
    sent_len[0] = ORI_ML
    bert_len = np.minimum(sent_len + rng.integers(2, 10, size=B), BERT_ML)
    adj = synth.dependency_batch(B, ORI_ML, 3.5, seed=12, lengths=sent_len).astype(np.float32)
    adj = adj * rng.uniform(0.05, 2.0, size=adj.shape).astype(np.float32) * np.where(rng.random(adj.shape) < 0.2, -0.25, 1.0).astype(np.float32)
    transform = np.zeros((B, ORI_ML, BERT_ML), dtype=np.float32)
    for b in range(B):
        for tkn in range(int(sent_len[b])):
            transform[b, tkn, 1 + min(tkn, BERT_ML - 2)] = 1.0
    inputs = {"sentence_length": torch.from_numpy(sent_len), "cls_text_sep_length": torch.from_numpy(bert_len),
              "cls_text_sep_indices": torch.zeros(B, BERT_ML, dtype=torch.long),
              "cls_text_sep_segments_ids": torch.zeros(B, BERT_ML, dtype=torch.long), "transform": torch.from_numpy(transform),
              "anchor_index": torch.from_numpy(np.array([int(rng.integers(0, n)) for n in sent_len])),
              "dist_to_target": torch.from_numpy(rng.integers(0, 6, size=(B, ORI_ML))), "dependency_graph": torch.from_numpy(adj)}
    inputs = {k: v.to(dev) for k, v in inputs.items()}
    opt = types.SimpleNamespace(dropout=0.5, polarities_dim=34, device=dev, ggcn_weighted_block=True)
    m = pkg.GatedGCNEventDetector(_Bert(), opt)
    assert m.gc1.weighted_block and m.gc2.weighted_block
    gen = torch.Generator().manual_seed(0)
    for p in m.parameters():
        if p.dim() > 1:
            torch.nn.init.xavier_uniform_(p, generator=gen)
        else:
            torch.nn.init.uniform_(p, -0.05, 0.05, generator=gen)
    m = m.to(dev).eval()
    calls = count_calls(monkeypatch, COUNTED)
    with torch.no_grad():
        logits, xy, kl, scores = m(inputs)
        assert calls[BLOCK] == 1 and calls[LAYER_W] == 0, calls
        m.gc1.weighted_block = m.gc2.weighted_block = False
        logits0, xy0, kl0, scores0 = m(inputs)
        assert calls[BLOCK] == 1 and calls[LAYER_W] == 2, calls
    torch.cuda.synchronize()
    tol = 1e-3 * max(1.0, float(logits0.abs().max()))        # tests/test_gpu_parity.py: the classifier's logits gate
    err = float((logits - logits0).abs().max())
    print("classifier logits, option on against off: %.3g (gate %.3g); xy %.6g / %.6g" % (err, tol, float(xy), float(xy0)))
    assert bool(torch.isfinite(logits).all()) and err <= tol
    assert abs(float(xy) - float(xy0)) <= 1e-3 * max(1.0, abs(float(xy0)))
