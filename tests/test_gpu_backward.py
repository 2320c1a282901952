"""The backward pass against float64 on every dispatch branch (run with ``-m gpu -s`` on an MI355X to see the figures).

First half: the backward's GEMMs and the transposed aggregation through the C ABI -- outputs pre-filled with NaN, the pad
columns of every strided operand NaN, the workspace pre-filled with 0xFF bytes (NaN as float32 and as bfloat16), each call
made twice and compared bit for bit, then against a float64 product of the same operands on the device.

Second half: ``GraphConvolution.forward_gated`` and ``gated_gcn_block`` under autograd against ``oracle/backward_ref.py``
(float64, torch autograd), one case per branch of ``_GatedLayerFunction.backward`` -- the pass, dX and dW forms that
``dispatch.backward_plan`` names.  Every case counts the library calls its
backward makes and asserts the branch it is named after, so a silent fall-back fails.  Pools whose two largest float64 values
are closer than 2*TOL/(1-p) get a zero upstream gradient on both sides (``backward_ref.pool_tie_mask``: the reference never sees
the GPU's picks); at most 3 % of a case's pools may be masked, asserted in every case.

Gates, all the project's own: float32 gradients |got - ref| <= 2e-4 * max|ref| (5e-4 under gate dropout and for the block),
the bf16 dX |dx - ref| <= 2^-8 |ref| + 1e-4 max|ref|, float32 results of bf16 features 1e-4 * max(1, max|ref|); forward
values TOL[precision] * max(1, max|ref|) / (1 - p) (keep factors scale the values and their error by 1/(1-p)).
"""
import numpy as np
import pytest
import torch

from oracle import backward_ref as br
from oracle import gates
from oracle.gpu_support import count_calls, dev, drop_mask as _drop_mask, make_layer, pkg  # noqa: F401

pytestmark = pytest.mark.gpu

NAN = float("nan")
_poisoned, _close32, _gate, _gate_dx = gates.poisoned, gates.close32, gates.gate, gates.gate_dx


def _padded(t, pad):
    """t [M,C] as a view of a [M, C + pad] buffer whose spare columns are NaN (a kernel that reads them shows it)."""
    if not pad:
        return t.contiguous()
    buf = torch.full((t.shape[0], t.shape[1] + pad), NAN, dtype=t.dtype, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


def _untouched(buf, width):
    """The spare columns of an output buffer are still the NaN they were filled with."""
    return buf.shape[1] == width or bool(torch.isnan(buf[:, width:].float()).all())


def _randn(shape, dev, seed):
    return torch.randn(*shape, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))


# ================================================================ 1. kernel-level sweeps through the C ABI
DW_SHAPES = [(20000, 768, 768), (5000, 132, 260), (37, 8, 12), (513, 256, 34), (1, 4, 4), (301, 7, 9), (64, 33, 2), (70001, 256, 512)]
DW_BF16_SHAPES = DW_SHAPES + [(131072, 768, 768), (511, 64, 64), (512, 64, 64), (513, 64, 64), (1025, 300, 200), (4097, 768, 34)]


@pytest.mark.parametrize("N,K,F", DW_BF16_SHAPES)
def test_dweight_bf16_vs_float64(pkg, dev, N, K, F):
    """ggcn_dweight_bf16 (its own transpose kernel, plan and single-plane main loop): dW = X^T.dH with bf16 X against float64, for
    ldx = K, K + 3 (rows 2-byte aligned only), K + 8, ldg = F, F + 4, lddw = F, F + 5.  Gate: the fp32 ggcn_dweight's for
    bf16x3, 3e-5 * max(sqrt(N) * 1e-3, 1e-3) (dH keeps its hi/lo image: csrc/dweight_bx3.hip)."""
    from ed_gated_gcn_amd import _capi
    lib = pkg.load_library()
    x = _randn((N, K), dev, N + K).to(torch.bfloat16)
    g = _randn((N, F), dev, N + F + 1) * 1e-3
    ref = x.double().t() @ g.double()
    bound = 3e-5 * max(np.sqrt(N) * 1e-3, 1e-3)
    nbytes = lib.ggcn_dweight_bf16_workspace_bytes(N, K, F)
    worst = 0.0
    for px in (0, 3, 8):
        xv = _padded(x, px)
        for pg in (0, 4):
            gv = _padded(g, pg)
            for pw in (0, 5):
                outs = []
                for _ in range(2):
                    dw = torch.full((K, F + pw), NAN, device=dev)
                    ws = _poisoned(nbytes, dev)
                    _capi.check(lib.ggcn_dweight_bf16(_capi.ptr(xv), K + px, _capi.ptr(gv), F + pg, N, K, F, _capi.ptr(dw), F + pw,
                                                      _capi.ptr(ws), _capi.stream_of(dev)), "ggcn_dweight_bf16")
                    outs.append(dw)
                what = "ldx=K+%d ldg=F+%d lddw=F+%d" % (px, pg, pw)
                assert torch.equal(outs[0][:, :F], outs[1][:, :F]), what
                assert _untouched(outs[0], F), what
                err = float((outs[0][:, :F].double() - ref).abs().max())
                assert err == err and err <= bound, "%s: max|diff| %.3g > %.3g" % (what, err, bound)
                worst = max(worst, err)
    print("dW bf16 %dx%dx%d: max|diff| %.3g (gate %.3g)" % (N, K, F, worst, bound))


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
@pytest.mark.parametrize("N,K,F", DW_SHAPES)
def test_dweight_strided_with_poisoned_workspace(pkg, dev, precision, N, K, F):
    """ggcn_dweight with ldx = K + 4 (keeps the TN form / 16-byte row loads) and K + 3 (forces transpose + pack for bf16x3, element
    loads for fp32), lddw = F + 5, the workspace 0xFF: the gates and the operands of test_weight_gradient_vs_float64.  (The gate of
    the exact-fp32 form is tight at 20000 x 768 x 768: 2.79e-7 of 2.83e-7 on these operands, whatever the leading dimension, and
    3.03e-7 was measured on another draw of the same shape -- the bound follows the data there, not the form taken.)"""
    from ed_gated_gcn_amd import _capi
    lib = pkg.load_library()
    rng = np.random.default_rng(N + K)                                 # the operands of test_weight_gradient_vs_float64
    x = torch.from_numpy(rng.standard_normal((N, K)).astype(np.float32)).to(dev)
    g = torch.from_numpy((rng.standard_normal((N, F)) * 1e-3).astype(np.float32)).to(dev)
    ref = x.double().t() @ g.double()
    bound = {"fp32": 2e-6, "bf16x3": 3e-5}[precision] * max(np.sqrt(N) * 1e-3, 1e-3)
    if precision == "fp32" and N > 50000:
        bound *= 2.0     # (as in test_weight_gradient_vs_float64: fp32 chains three times as long)
    prec = _capi.PREC[precision]
    nbytes = lib.ggcn_dweight_workspace_bytes(N, K, F, prec)
    for px in (4, 3):
        xv = _padded(x, px)
        outs = []
        for _ in range(2):
            dw = torch.full((K, F + 5), NAN, device=dev)
            ws = _poisoned(nbytes, dev)
            _capi.check(lib.ggcn_dweight(_capi.ptr(xv), K + px, _capi.ptr(g), F, N, K, F, _capi.ptr(dw), F + 5, prec, _capi.ptr(ws),
                                         _capi.stream_of(dev)), "ggcn_dweight")
            outs.append(dw)
        assert torch.equal(outs[0][:, :F], outs[1][:, :F]) and _untouched(outs[0], F), px
        err = float((outs[0][:, :F].double() - ref).abs().max())
        print("dW %s %dx%dx%d ldx=K+%d: max|diff| %.3g (gate %.3g)" % (precision, N, K, F, px, err, bound))
        assert err == err and err <= bound, "ldx=K+%d: max|diff| %.3g > %.3g" % (px, err, bound)


LIN_SHAPES = [(256, 768, 768), (1000, 300, 300), (33, 17, 5), (513, 768, 34), (7, 9216, 256), (131072, 768, 768)]


def _packed(pkg, dev, K, F, transposed, seed=5):
    """(W [K,F] on the device, its bf16x3 image) -- packed from W itself, or from W^T stored [F,K] with transposed = 1 (what the
    backward's dX linear does with the forward's weight)."""
    from ed_gated_gcn_amd import _capi, synth
    lib = pkg.load_library()
    w = torch.from_numpy(synth.layer_params(K, F, seed=seed)[0]).to(dev)
    prec = _capi.PREC["bf16x3"]
    pack = torch.empty(lib.ggcn_weight_pack_bytes(K, F, prec), dtype=torch.uint8, device=dev)
    stored, ldw = (w.t().contiguous(), K) if transposed else (w, F)
    _capi.check(lib.ggcn_weight_pack(_capi.ptr(stored), ldw, K, F, prec, 1 if transposed else 0, _capi.ptr(pack), _capi.stream_of(dev)),
                "ggcn_weight_pack")
    return w, pack


@pytest.mark.parametrize("transposed", [False, True], ids=["W", "Wt"])
@pytest.mark.parametrize("M,K,F", LIN_SHAPES)
def test_linear_out_bf16_vs_float64(pkg, dev, M, K, F, transposed):
    """ggcn_linear_out_bf16 (the bf16 dX): float32 X . W with the result rounded to bfloat16 in the store, over the float32
    exponent range (scale 3e-9 ... 2e7: the reason dX stays on bf16x3), ldx = K, K + 1, ldy = F, F + 1 (bf16 rows at odd element
    offsets).  Gate: |y - ref| <= 2^-8 |ref| + 1e-4 max|ref| for every element."""
    from ed_gated_gcn_amd import _capi
    lib = pkg.load_library()
    w, pack = _packed(pkg, dev, K, F, transposed)
    x0 = _randn((M, K), dev, M + K)
    for scale in (1.0, 3e-9, 2e7):
        x = x0 * scale
        ref = x.double() @ w.double()
        top = float(ref.abs().max())
        bound = 2.0 ** -8 * ref.abs() + 1e-4 * top
        worst = -1.0
        for px in (0, 1):
            xv = _padded(x, px)
            for py in (0, 1):
                outs = []
                for _ in range(2):
                    y = torch.full((M, F + py), NAN, dtype=torch.bfloat16, device=dev)
                    _capi.check(lib.ggcn_linear_out_bf16(_capi.ptr(xv), K + px, _capi.ptr(pack), _capi.ptr(y), F + py, M, K, F,
                                                         _capi.stream_of(dev)), "ggcn_linear_out_bf16")
                    outs.append(y)
                what = "scale %g ldx=K+%d ldy=F+%d" % (scale, px, py)
                assert torch.equal(outs[0][:, :F], outs[1][:, :F]) and _untouched(outs[0], F), what
                excess = (outs[0][:, :F].double() - ref).abs() - bound
                assert not bool(torch.isnan(excess).any()), what
                assert float(excess.max()) <= 0.0, "%s: %d elements outside the gate, worst by %.3g of max|ref|" % (
                    what, int((excess > 0).sum()), float(excess.max()) / top)
                worst = max(worst, float(((outs[0][:, :F].double() - ref).abs() / bound).max()))
        print("Y bf16 %dx%dx%d scale %g: max |diff| / gate %.3f" % (M, K, F, scale, worst))


@pytest.mark.parametrize("M,K,F", LIN_SHAPES)
def test_linear_bf16_vs_float64(pkg, dev, M, K, F):
    """ggcn_linear_bf16 (bf16 X -> float32 Y) on the same shapes, ldx = K, K + 3 (element loads), ldy = F, F + 1; 1e-4 * max|ref|."""
    from ed_gated_gcn_amd import _capi
    lib = pkg.load_library()
    w, pack = _packed(pkg, dev, K, F, False)
    x = _randn((M, K), dev, M + K).to(torch.bfloat16)
    ref = x.double() @ w.double()
    gate = 1e-4 * float(ref.abs().max())
    worst = 0.0
    for px in (0, 3):
        xv = _padded(x, px)
        for py in (0, 1):
            outs = []
            for _ in range(2):
                y = torch.full((M, F + py), NAN, device=dev)
                _capi.check(lib.ggcn_linear_bf16(_capi.ptr(xv), K + px, _capi.ptr(pack), _capi.ptr(y), F + py, M, K, F,
                                                 _capi.stream_of(dev)), "ggcn_linear_bf16")
                outs.append(y)
            what = "ldx=K+%d ldy=F+%d" % (px, py)
            assert torch.equal(outs[0][:, :F], outs[1][:, :F]) and _untouched(outs[0], F), what
            err = float((outs[0][:, :F].double() - ref).abs().max())
            assert err == err and err <= gate, "%s: max|diff| %.3g > %.3g" % (what, err, gate)
            worst = max(worst, err)
    print("Y f32 of bf16 X %dx%dx%d: max|diff| %.3g (gate %.3g)" % (M, K, F, worst, gate))


def _aggregate_t_case(pkg, dev, adj, F, seed, unaligned=False):
    """ggcn_aggregate_t on the transposed CSR of adj against dH[s] = sum_t A[t,s] dY[t] / (rowsum_t + 1) in float64."""
    from ed_gated_gcn_amd import _capi
    lib = pkg.load_library()
    B, T, _ = adj.shape
    adj_d = adj.to(dev)
    csr = pkg.BatchedCSR.from_dense(adj_d)
    csr_t, inv = csr.transposed(), csr.inv_denominators()
    if unaligned:   # a contiguous view one float into its buffer: 4-byte aligned rows
        buf = _randn((B * T * F + 1,), dev, seed)
        dy = buf[1:].view(B * T, F)
        assert dy.data_ptr() % 16 == 4
    else:
        dy = _randn((B * T, F), dev, seed)
    outs = []
    for _ in range(2):
        dh = torch.full((B * T, F), NAN, device=dev)
        _capi.check(lib.ggcn_aggregate_t(_capi.ptr(dy), F, _capi.ptr(csr_t.rowptr), _capi.ptr(csr_t.colidx), _capi.ptr(csr_t.vals),
                                         _capi.ptr(inv), B, T, F, _capi.ptr(dh), F, _capi.stream_of(dev)), "ggcn_aggregate_t")
        outs.append(dh)
    assert torch.equal(outs[0], outs[1])
    a64 = adj_d.double()
    scale = 1.0 / (a64.sum(2) + 1.0)
    want = torch.einsum("bts,btf->bsf", a64 * scale[:, :, None], dy.view(B, T, F).double())
    gate = 2e-6 * float(want.abs().max())
    err = float((outs[0].view(B, T, F).double() - want).abs().max())
    print("dH %dx%dx%d: max|diff| %.3g (gate %.3g)" % (B, T, F, err, gate))
    assert err == err and err <= gate, "max|diff| %.3g > %.3g" % (err, gate)


@pytest.mark.parametrize("graph", ["tree", "directed", "weighted"])
@pytest.mark.parametrize("F", [256, 30, 1028])
@pytest.mark.parametrize("T", [1, 33, 40, 48, 49, 100, 256, 257, 513])
def test_aggregate_t_vs_float64(pkg, dev, T, F, graph):
    """The three forms of ggcn_aggregate_t (LDS-tiled for T <= 48, 16-row chunks beyond, one column per thread when F % 4 != 0)
    on symmetric, directed and real-valued asymmetric adjacencies; 2e-6 * max|ref| (the float64 statement's gate in
    test_gate_pool_backward_on_the_matrix_cores)."""
    _aggregate_t_case(pkg, dev, br.case_adjacency(3, T, 40 + T, graph), F, seed=T + F)


@pytest.mark.parametrize("T,F,how", [(100, 256, "complete"), (100, 30, "complete"), (40, 256, "unaligned"), (100, 256, "unaligned"),
                                     (300, 1028, "unaligned")])
def test_aggregate_t_long_rows_and_unaligned_gradient(pkg, dev, T, F, how):
    """A complete graph of 100 nodes (rows longer than a wavefront) and a dY that is only 4-byte aligned (one column per thread)."""
    if how == "complete":
        adj = torch.ones(2, T, T)
        adj[1] = br.case_adjacency(1, T, 7)[0]
        _aggregate_t_case(pkg, dev, adj, F, seed=T + F)
    else:
        _aggregate_t_case(pkg, dev, br.case_adjacency(3, T, 8), F, seed=T + F, unaligned=True)


# ================================================================ 2. the dispatch tree under autograd
MMA, AGG, GPB, GPB_DROP, AGG_T = ("ggcn_gate_pool_backward_mma", "ggcn_gate_pool_backward_agg", "ggcn_gate_pool_backward",
                                   "ggcn_gate_pool_backward_drop", "ggcn_aggregate_t")
BWD = (MMA, AGG, GPB, GPB_DROP, AGG_T, "ggcn_linear_scaled", "ggcn_linear", "ggcn_linear_out_bf16", "ggcn_dweight", "ggcn_dweight_bf16",
       "ggcn_colsum")
FWD = ("ggcn_layer_fused", "ggcn_layer_fused_drop", "ggcn_layer_fused_bf16", "ggcn_layer_fused_bf16_drop", "ggcn_layer_fused_bf16_wide",
       "ggcn_layer_fused_weighted", "ggcn_linear_bf16", "ggcn_aggregate")
PREC_ARG = {"ggcn_linear": 10, "ggcn_dweight": 9}     # where the two entries that serve several arithmetics take `precision`
PASSES = {"mma": (MMA,), "agg": (AGG,), "two": (GPB, AGG_T), "two-drop": (GPB_DROP, AGG_T)}
DX = {"scaled": ("ggcn_linear_scaled",), "bf16x3": ("ggcn_linear", "ggcn_linear/bf16x3"), "fp32": ("ggcn_linear", "ggcn_linear/fp32"),
      "bf16": ("ggcn_linear_out_bf16",), None: ()}
DW = {"bf16x3": ("ggcn_dweight", "ggcn_dweight/bf16x3"), "fp32": ("ggcn_dweight", "ggcn_dweight/fp32"), "bf16": ("ggcn_dweight_bf16",),
      None: ()}
KEYS = BWD + FWD + ("ggcn_linear/bf16x3", "ggcn_linear/fp32", "ggcn_linear/f16mx8", "ggcn_dweight/bf16x3", "ggcn_dweight/fp32")


def _expected(passes, dx, dw, db, times=1):
    e = {k: 0 for k in KEYS if k not in FWD}
    for k in PASSES[passes] + DX[dx] + DW[dw] + (("ggcn_colsum",) if db else ()):
        e[k] += times
    return e


def _assert_calls(calls, before, expect, what):
    got = {k: calls[k] - before[k] for k in expect}
    assert got == expect, "%s: the backward made %s, not %s" % (
        what, {k: v for k, v in got.items() if v}, {k: v for k, v in expect.items() if v})


def _layer(pkg, dev, w, b, precision, fused_max_t=None):
    return make_layer(pkg, dev, w, b, precision=precision, fused_max_t=fused_max_t)


def _offset_leaf(t):
    """(leaf buffer, contiguous view of it at storage offset 1 holding t): a [B,F] operand that is only 4-byte aligned."""
    buf = torch.cat([torch.full((1,), NAN, device=t.device), t.reshape(-1)]).requires_grad_()
    view = buf[1:].view(t.shape)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return buf, view


def _run_layer(pkg, dev, monkeypatch, name, precision, bf16, expect, fwd=None, env=None, fused_max_t=None, x_pad=0,
               offset_gates=False, streams=None, loss=("out", "pa", "pb"), gates=("sg", "ga", "gb"), gate_grad=True, w_grad=True,
               x_grad=True, bias=True):
    """One case: forward_gated under autograd with loss sum(out*R1) + sum(pa*R2) + sum(pb*R3) (R2, R3 tie-masked), the float64
    reference on the same device, the calls of the backward counted against `expect` = (pass, dX, dW).  Returns the gradients."""
    _, B, T, K, F, _, _, p = br.RECIPE[name]
    what = "%s/%s" % (name, "bf16" if bf16 else precision)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    c = {k: (v.to(dev) if v is not None else None) for k, v in br.recipe_inputs(name, bf16=bf16, bias=bias).items()}
    m = _layer(pkg, dev, c["w"], c["b"], precision, fused_max_t)
    m.weight.requires_grad_(w_grad)
    dropout = (p, 2 ** 40 + 99, streams) if p else None
    tol = br.TOL[precision] / (1.0 - p)
    # ---- the float64 reference and the near-tie masks (nothing of the GPU run enters)
    use = {k: (c[k] if k in gates else None) for k in ("sg", "ga", "gb")}
    keep = None
    if dropout is not None:
        keep = tuple(None if s == 0 else _drop_mask(pkg, dev, B * T, F, p, dropout[1], s).view(B, T, F).double() for s in streams)
    ma, mb = br.layer_tie_masks(c["x"], c["adj"], c["w"], c["b"], use["ga"], use["gb"], br.tie_delta(precision, p), keep=keep)
    share = br.masked_share(*[mk for mk, g in ((ma, "ga"), (mb, "gb")) if g in gates])
    print("%s: %.2f %% of the pools masked" % (what, 100 * share))
    assert share <= br.MAX_MASKED
    r1, r2, r3 = c["r1"], c["r2"] * (~ma), c["r3"] * (~mb)
    ref = {k: (None if v is None else v.double().requires_grad_()) for k, v in
           (("x", c["x"]), ("w", c["w"]), ("b", c["b"]), ("sg", use["sg"]), ("ga", use["ga"]), ("gb", use["gb"]))}
    o64, a64, b64 = br.gated_layer_ref(ref["x"], c["adj"], ref["w"], ref["b"], ref["sg"], ref["ga"], ref["gb"], keep=keep)
    terms = {"out": (o64 * r1).sum(), "pa": (a64 * r2).sum(), "pb": (b64 * r3).sum()}
    sum(terms[k] for k in loss).backward()
    # ---- the layer under autograd
    calls = count_calls(monkeypatch, BWD + FWD, PREC_ARG)
    if x_pad:   # x as a view with row stride K + x_pad of a leaf whose spare columns are NaN
        xbuf = torch.full((B, T, K + x_pad), NAN, dtype=c["x"].dtype, device=dev)
        with torch.no_grad():
            xbuf[..., :K] = c["x"]
        xbuf.requires_grad_(x_grad)
        xv = xbuf[..., :K]
        assert xv.reshape(B * T, K).stride(0) == K + x_pad
    else:
        xbuf = xv = c["x"].clone().requires_grad_(x_grad)
    leaf, view = {}, {}
    for k in ("sg", "ga", "gb"):
        if use[k] is None:
            leaf[k] = view[k] = None
        elif offset_gates:
            leaf[k], view[k] = _offset_leaf(use[k])
        else:
            leaf[k] = view[k] = use[k].clone().requires_grad_(gate_grad)
    out, pa, pb = m.forward_gated(xv, c["adj"], store_gate=view["sg"], pool_gate_a=view["ga"], pool_gate_b=view["gb"],
                                  want_pool_a="ga" in gates, want_pool_b="gb" in gates, dropout=dropout)
    if fwd is not None:
        got_fwd = {k: calls[k] for k in FWD + ("ggcn_linear",) if calls[k]}
        assert got_fwd == {k: 1 for k in fwd}, "%s: the forward made %s, not %s" % (what, got_fwd, fwd)
    got_terms = {"out": lambda: (out * r1).sum(), "pa": lambda: (pa * r2).sum(), "pb": lambda: (pb * r3).sum()}
    total = sum(got_terms[k]() for k in loss)
    before = dict(calls)
    total.backward()
    torch.cuda.synchronize()
    passes, dx_form, dw_form = expect
    _assert_calls(calls, before, _expected(passes, dx_form if x_grad else None, dw_form if w_grad else None, bias), what)
    # ---- forward values (the pools of masked entries too)
    assert out.dtype == torch.float32
    _gate(out.detach(), o64.detach(), "out", tol)
    if pa is not None:
        _gate(pa.detach(), a64.detach(), "pool a", tol)
    if pb is not None:
        _gate(pb.detach(), b64.detach(), "pool b", tol)
    # ---- gradients
    rel = 5e-4 if dropout is not None else 2e-4
    grads = {"x": None if xbuf.grad is None else xbuf.grad[..., :K], "w": m.weight.grad, "b": None if m.bias is None else m.bias.grad}
    for k in ("sg", "ga", "gb"):
        gk = None if leaf[k] is None else leaf[k].grad
        grads[k] = (None if gk is None else gk[1:].view(B, F)) if offset_gates else gk
    if x_pad and x_grad:
        assert bool((xbuf.grad[..., K:] == 0).all())
    if offset_gates:
        assert all(leaf[k] is None or float(leaf[k].grad[0]) == 0.0 for k in leaf)
    need = {"x": x_grad, "w": w_grad, "b": bias, "sg": gate_grad, "ga": gate_grad, "gb": gate_grad}
    for k, label in (("x", "dX"), ("w", "dW"), ("b", "db"), ("sg", "d store gate"), ("ga", "d gate a"), ("gb", "d gate b")):
        got, want = grads[k], (None if ref[k] is None else ref[k].grad)
        if ref[k] is None or not need[k]:
            assert got is None, "%s: %s must be None" % (what, label)
        elif want is None:      # a leaf the loss never reaches: no gradient, or zeros
            assert got is None or not bool(got.float().abs().any()), "%s: %s must vanish" % (what, label)
        else:
            assert got is not None, "%s: %s is missing" % (what, label)
            if k == "x" and bf16:
                _gate_dx(got, want)
            elif bf16:
                _gate(got, want, label)
            else:
                _close32(got, want, label, rel)
    return grads


F32 = [("f16mx8", False)]
BOTH = [("f16mx8", False), ("f16mx8", True)]      # bfloat16 features on the default layer precision (the bf16 pair form)
IDS = lambda v: "bf16" if v is True else ("f32" if v is False else v)   # noqa: E731


def _forms(bf16, dx, dw="bf16x3"):
    """bfloat16 features take ggcn_linear_out_bf16 / ggcn_dweight_bf16 whatever the float32 case takes."""
    return ("bf16", "bf16") if bf16 else (dx, dw)


@pytest.mark.parametrize("precision,bf16", BOTH, ids=IDS)
def test_record_shape(pkg, dev, monkeypatch, precision, bf16):
    """4096 x 32 x 768 x 768, N = 131072: the matrix-core gate / pool pass, dX on the scaled f16mx8 product, dW on the 256 x 256 TN
    tile; bfloat16 features: ggcn_dweight_bf16 / ggcn_linear_out_bf16 at training size."""
    _run_layer(pkg, dev, monkeypatch, "record", precision, bf16, ("mma",) + _forms(bf16, "scaled"),
               fwd=("ggcn_layer_fused_bf16",) if bf16 else ("ggcn_layer_fused",))


@pytest.mark.parametrize("precision,bf16,dx,dw", [("f16mx8", False, "scaled", "bf16x3"), ("bf16x3", False, "bf16x3", "bf16x3"),
                                                  ("fp32", False, "fp32", "fp32"), ("bf16x3", True, "bf16", "bf16")],
                         ids=["f16mx8", "bf16x3", "fp32", "bf16"])
def test_narrow_every_precision(pkg, dev, monkeypatch, precision, bf16, dx, dw):
    """64 x 31 x 256 x 256: dX on the scaled / bf16x3 / exact-fp32 linear, dW on the full TN tile / the exact fp32 form."""
    _run_layer(pkg, dev, monkeypatch, "narrow", precision, bf16, ("mma", dx, dw))


@pytest.mark.parametrize("scalar", [False, True], ids=["mma", "GGCN_BACKWARD_SCALAR"])
def test_f96_amax_handover(pkg, dev, monkeypatch, scalar):
    """F = 96: the matrix-core pass hands max|dH| over -> scaled dX; the scalar one-launch pass does so for whole wavefronts of
    columns only (F % 256 == 0) -> dX on bf16x3."""
    _run_layer(pkg, dev, monkeypatch, "f96", "f16mx8", False, ("agg", "bf16x3", "bf16x3") if scalar else ("mma", "scaled", "bf16x3"),
               env={"GGCN_BACKWARD_SCALAR": "1"} if scalar else None)


@pytest.mark.parametrize("precision,bf16", BOTH, ids=IDS)
@pytest.mark.parametrize("name", ["ragged17", "ragged30"])
def test_ragged_widths(pkg, dev, monkeypatch, name, precision, bf16):
    """F % 32 != 0 -> dX on bf16x3; K = 34: the transpose form of dW; K = 300, F = 200: the ragged 128 x 256 TN tile; bfloat16
    features with K % 8 != 0: element loads."""
    _run_layer(pkg, dev, monkeypatch, name, precision, bf16, ("mma",) + _forms(bf16, "bf16x3"))


def test_f30_one_column_kernels(pkg, dev, monkeypatch):
    """F % 4 != 0: ggcn_gate_pool_backward and ggcn_aggregate_t one column per thread, dW in the transpose form."""
    _run_layer(pkg, dev, monkeypatch, "f30", "f16mx8", False, ("two", "bf16x3", "bf16x3"))


@pytest.mark.parametrize("env,expect", [({"GGCN_BACKWARD_TWO_PASS": "1"}, ("two", "bf16x3", "bf16x3")),
                                        ({"GGCN_DX_PRECISION": "bf16x3"}, ("mma", "bf16x3", "bf16x3"))],
                         ids=["GGCN_BACKWARD_TWO_PASS", "GGCN_DX_PRECISION"])
def test_environment_switches(pkg, dev, monkeypatch, env, expect):
    _run_layer(pkg, dev, monkeypatch, "square", "f16mx8", False, expect, env=env)


@pytest.mark.parametrize("precision,bf16", BOTH, ids=IDS)
def test_unaligned_gates_take_the_two_calls(pkg, dev, monkeypatch, precision, bf16):
    """Each gate a contiguous [B,F] view at storage offset 1 of a larger leaf (4-byte aligned only): the backward leaves the
    one-launch forms (their 16-byte accesses) for ggcn_gate_pool_backward + ggcn_aggregate_t; forward and gradients stay inside
    the gates of the aligned run."""
    _run_layer(pkg, dev, monkeypatch, "square", precision, bf16, ("two",) + _forms(bf16, "bf16x3"), offset_gates=True)


@pytest.mark.parametrize("pad", [3, 4])
@pytest.mark.parametrize("precision,bf16,dx,dw", [("f16mx8", False, "scaled", "bf16x3"), ("fp32", False, "fp32", "fp32"),
                                                  ("bf16x3", True, "bf16", "bf16")], ids=["f16mx8", "fp32", "bf16"])
def test_strided_x_view(pkg, dev, monkeypatch, precision, bf16, dx, dw, pad):
    """x a view with row stride K + 3 / K + 4 (x2d.stride(0) != K goes straight into both dW kernels)."""
    _run_layer(pkg, dev, monkeypatch, "view", precision, bf16, ("mma", dx, dw), x_pad=pad)


@pytest.mark.parametrize("streams", [(0, 1, 2), (2, 2, 0)], ids=["layer1-streams", "layer2-streams"])
@pytest.mark.parametrize("precision,bf16", BOTH, ids=IDS)
@pytest.mark.parametrize("name,dx", [("drop32", "scaled"), ("drop24", "bf16x3")])
def test_gate_dropout(pkg, dev, monkeypatch, name, dx, precision, bf16, streams):
    """p = 0.25: the scalar one-launch pass with (F % 256 == 0) and without max|dH|; the reference multiplies the repeated gates
    by the keep factors of ggcn_dropout_mask.  Streams as in the block: layer 1 (0, 1, 2) with all three gates, layer 2 (2, 2, 0)
    with its store gate and one pool on the same stream (bert_amir5.py:639-640: no second pool)."""
    layer2 = dict(gates=("sg", "ga"), loss=("out", "pa")) if streams[0] else {}
    _run_layer(pkg, dev, monkeypatch, name, precision, bf16, ("agg",) + _forms(bf16, dx), streams=streams, **layer2)


@pytest.mark.parametrize("precision,bf16", BOTH, ids=IDS)
def test_gate_dropout_beyond_32_nodes(pkg, dev, monkeypatch, precision, bf16):
    """8 x 100 x 256 x 256, p = 0.25: ggcn_gate_pool_backward_drop + ggcn_aggregate_t."""
    _run_layer(pkg, dev, monkeypatch, "drop100", precision, bf16, ("two-drop",) + _forms(bf16, "bf16x3"), streams=(0, 1, 2),
               fused_max_t=256)


@pytest.mark.parametrize("bf16", [False, True], ids=IDS)
def test_dropped_store_gate_with_a_pool_on_another_stream_is_refused_under_autograd(pkg, dev, bf16):
    """The backward reads y back from the stored out = y * sg * k_store; where k_store = 0 nothing is left, which is exact only
    for pools that drop the same tokens.  A pool on another stream (or undropped) next to a dropped store gate used to get its
    gradient routed to wrong rows without a word (dX off by 11 % of its scale at 32 x 32 x 256 x 256, p = 0.25, streams
    (2, 2, 0) with a second pool): under autograd that combination is now refused; inference still runs it."""
    c = {k: (v.to(dev) if v is not None else None) for k, v in br.recipe_inputs("drop32", bf16=bf16).items()}
    m = _layer(pkg, dev, c["w"], c["b"], "f16mx8")
    kw = dict(store_gate=c["sg"], pool_gate_a=c["ga"], pool_gate_b=c["gb"], want_pool_a=True, want_pool_b=True)
    with torch.no_grad():
        out, pa, pb = m.forward_gated(c["x"], c["adj"], dropout=(0.25, 7, (2, 2, 0)), **kw)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(pb).all())
    x = c["x"].clone().requires_grad_()
    for streams in ((2, 2, 0), (1, 2, 1), (2, 0, 2)):
        with pytest.raises(RuntimeError, match="share the store gate's keep stream"):
            m.forward_gated(x, c["adj"], dropout=(0.25, 7, streams), **kw)
    m.forward_gated(x, c["adj"], dropout=(0.25, 7, (2, 2, 2)), **kw)[0].sum().backward()      # one stream for all three: fine
    assert x.grad is not None and bool(torch.isfinite(x.grad.float()).all())


@pytest.mark.parametrize("precision,bf16", BOTH, ids=IDS)
@pytest.mark.parametrize("name,dx", [("directed", "scaled"), ("isolated", "scaled"), ("complete", "scaled"), ("len1", "scaled"),
                                     ("one", "bf16x3")])
def test_graph_shapes(pkg, dev, monkeypatch, name, dx, precision, bf16):
    """Directed (A^T is not A), isolated nodes, one complete 32-node graph, all lengths 1, and one node in all."""
    _run_layer(pkg, dev, monkeypatch, name, precision, bf16, ("mma",) + _forms(bf16, dx))


@pytest.mark.parametrize("precision,bf16", BOTH, ids=IDS)
def test_weighted_adjacency(pkg, dev, monkeypatch, precision, bf16):
    """A real-valued asymmetric adjacency: the two calls, ggcn_aggregate_t with edge values."""
    _run_layer(pkg, dev, monkeypatch, "weighted", precision, bf16, ("two",) + _forms(bf16, "bf16x3"))


SUBSETS = {
    "pools-only": dict(loss=("pa", "pb")),                       # d_out arrives as None
    "out-only": dict(loss=("out",)),                             # d_pa, d_pb arrive as None
    "pb-only": dict(loss=("pb",)),
    "no-store-gate": dict(gates=("ga", "gb")),
    "one-pool": dict(gates=("sg", "ga"), loss=("out", "pa")),
    "gates-without-gradient": dict(gate_grad=False),
}


@pytest.mark.parametrize("precision,bf16", BOTH, ids=IDS)
@pytest.mark.parametrize("subset", list(SUBSETS))
def test_subsets_of_outputs_and_gates(pkg, dev, monkeypatch, subset, precision, bf16):
    """Outputs the loss never reads reach the backward as None (ctx.set_materialize_grads(False)); absent gates and pools; gates
    that need no gradient."""
    _run_layer(pkg, dev, monkeypatch, "square-sym" if subset in ("pools-only", "pb-only") else "square", precision, bf16,
               ("mma",) + _forms(bf16, "scaled"), **SUBSETS[subset])


@pytest.mark.parametrize("precision,bf16", BOTH, ids=IDS)
def test_no_bias_frozen_weight_and_x_without_gradient(pkg, dev, monkeypatch, precision, bf16):
    """bias=False (no db, no per-graph sums); a frozen weight (dW is None, everything else bit for bit what it was); an x that
    needs no gradient."""
    forms = ("mma",) + _forms(bf16, "scaled")
    full = _run_layer(pkg, dev, monkeypatch, "square", precision, bf16, forms)
    _run_layer(pkg, dev, monkeypatch, "square", precision, bf16, forms, bias=False)
    frozen = _run_layer(pkg, dev, monkeypatch, "square", precision, bf16, forms, w_grad=False)
    assert frozen["w"] is None
    for k in ("x", "b", "sg", "ga", "gb"):
        assert torch.equal(frozen[k], full[k]), k
    nox = _run_layer(pkg, dev, monkeypatch, "square", precision, bf16, forms, x_grad=False)
    assert nox["x"] is None


@pytest.mark.parametrize("precision,bf16", BOTH, ids=IDS)
@pytest.mark.parametrize("T", [33, 40, 48, 49, 64, 65, 128, 129, 200, 231, 256])
def test_wide_graphs(pkg, dev, monkeypatch, T, precision, bf16):
    """33..256 nodes (fused_max_t = 256): one-launch forward, two-call backward; ggcn_aggregate_t LDS-tiled up to 48 nodes, in
    16-row chunks beyond."""
    _run_layer(pkg, dev, monkeypatch, "wide%d" % T, precision, bf16, ("two",) + _forms(bf16, "bf16x3"), fused_max_t=256,
               fwd=("ggcn_layer_fused_bf16_wide",) if bf16 else ("ggcn_layer_fused",))


@pytest.mark.parametrize("precision,bf16", BOTH, ids=IDS)
def test_wide_graphs_at_the_models_width(pkg, dev, monkeypatch, precision, bf16):
    """64 x 231 x 768 x 768: the ACE-cased length at the model's width."""
    _run_layer(pkg, dev, monkeypatch, "wide768", precision, bf16, ("two",) + _forms(bf16, "bf16x3"), fused_max_t=256,
               fwd=("ggcn_layer_fused_bf16_wide",) if bf16 else ("ggcn_layer_fused",))


@pytest.mark.parametrize("precision,bf16", BOTH, ids=IDS)
@pytest.mark.parametrize("T", [257, 300, 513])
def test_long_graphs_past_the_row_masks(pkg, dev, monkeypatch, T, precision, bf16):
    """T > 256: linear + aggregate forward, CSR backward."""
    _run_layer(pkg, dev, monkeypatch, "long%d" % T, precision, bf16, ("two",) + _forms(bf16, "bf16x3"),
               fwd=("ggcn_linear_bf16", "ggcn_aggregate") if bf16 else ("ggcn_linear", "ggcn_aggregate"))


# ---------------------------------------------------------------- the whole block under autograd
@pytest.mark.parametrize("precision,bf16", BOTH, ids=IDS)
@pytest.mark.parametrize("name", [r[0] for r in br.BLOCK_RECIPES])
def test_gated_block_under_autograd(pkg, dev, monkeypatch, name, precision, bf16):
    """gated_gcn_block at the two training lengths at the model's width (256 x 32 x 768, 64 x 231 x 768): two layer launches, gc2
    sees d_pb = None and gc1 a d_out that is gc2's dX.  Loss on out, x and the regulariser as in
    test_gated_block_backward_vs_oracle_autograd; the tie mask covers x1, y1 and out, and the regulariser term is taken as
    sum(x1 * y1 * unmasked) / B from the returned pools on both sides (xy itself is checked as a forward value)."""
    _, B, T, H = [r for r in br.BLOCK_RECIPES if r[0] == name][0]
    c = {k: v.to(dev) for k, v in br.block_inputs(name, bf16=bf16).items()}
    m1, my, mo = br.block_tie_masks(c["x"], c["adj"], c["g1"], c["g2"], c["w1"], c["b1"], c["w2"], c["b2"], br.tie_delta(precision))
    share = br.masked_share(m1, my, mo)
    print("%s/%s: %.2f %% of the pools masked" % (name, "bf16" if bf16 else precision, 100 * share))
    assert share <= br.MAX_MASKED
    unmasked, r1, r2 = ~(m1 | my), c["r1"] * (~mo), c["r2"]

    def loss_of(r):
        return (r["out"] * r1).sum() + 0.1 * (r["x"] * r2).sum() + 0.01 * (r["x1"] * r["y1"] * unmasked).sum() / B

    names = ("x", "g1", "g2", "w1", "b1", "w2", "b2")
    ref = {k: c[k].double().requires_grad_() for k in names}
    rr = br.block_ref(ref["x"], c["adj"], *[ref[k] for k in names[1:]])
    loss_of(rr).backward()

    gc1, gc2 = _layer(pkg, dev, c["w1"], c["b1"], precision, 256), _layer(pkg, dev, c["w2"], c["b2"], precision, 256)
    xg, g1g, g2g = (c[k].clone().requires_grad_() for k in ("x", "g1", "g2"))
    calls = count_calls(monkeypatch, BWD + FWD, PREC_ARG)
    r = pkg.gated_gcn_block(xg, c["adj"], g1g, g2g, gc1, gc2)
    before = dict(calls)
    loss_of(r).backward()
    torch.cuda.synchronize()
    if T <= 32 and not bf16:
        expect = _expected("mma", "scaled", "bf16x3", True, times=2)
    elif T <= 32:      # gc1 reads the bf16 x, gc2 the float32 gcn1
        expect = _expected("mma", "scaled", "bf16x3", True)
        for k, v in _expected("mma", "bf16", "bf16", True).items():
            expect[k] += v
    elif not bf16:
        expect = _expected("two", "bf16x3", "bf16x3", True, times=2)
    else:
        expect = _expected("two", "bf16x3", "bf16x3", True)
        for k, v in _expected("two", "bf16", "bf16", True).items():
            expect[k] += v
    _assert_calls(calls, before, expect, name)
    tol = br.TOL[precision]
    for k in ("gcn1", "x1", "y1", "x", "out"):
        _gate(r[k].detach(), rr[k].detach(), k, tol)
    _gate(r["xy"].detach().reshape(1), rr["xy"].detach().reshape(1), "xy", 1e-4)
    got = {"x": xg.grad, "g1": g1g.grad, "g2": g2g.grad, "w1": gc1.weight.grad, "b1": gc1.bias.grad, "w2": gc2.weight.grad,
           "b2": gc2.bias.grad}
    for k in names:
        if k == "x" and bf16:
            _gate_dx(got[k], ref[k].grad)
        else:
            _close32(got[k], ref[k].grad, "d " + k, 5e-4)
