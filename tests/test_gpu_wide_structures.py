"""The one-launch float32 layers of 33..256-node graphs (``fused_wide.hip``: 64- / 128-row slots on ceil(T/32)^2 blocks of mask
bits; ``fused_wide8.hip``: eight wavefronts per graph, per-row edge lists with the branches deg <= 8, 9..16 and > 16, a filler row
for T < 256 and a full-slot form for T = 256) on DIRECTED AND EXTREME graphs.  Run with ``-m gpu -s`` on an MI355X to see the figures.

Every other test that reaches these kernels builds symmetric dependency trees, on which ``A^T = A``.  Here one batch holds one graph
per structure of ``oracle/wide_structures.py`` (triangles of a tree, a random directed graph, the complete and the empty graph, a hub,
a ladder of degrees around the list boundaries, one off-diagonal block, a shift, a single node, a ragged directed tree), so that one
launch sees them all; ``tests/test_wide_structures_cpu.py`` shows that on every asymmetric one ``A`` and ``A^T`` are >= 100 gates apart.

(a) ``ggcn_layer_fused`` at both slots of the first kernel and both row-group counts of the second, at and just past their edges, in a
    fast and a general shape: out and both pools against float64, pools-only, a host-collated CSR, edge lists built inside the
    workgroup (``GGCN_EDGE_LISTS=0``) -- bit for bit -- and linear + aggregate on the same batch against float64;
(b) the folded evaluation (``ggcn_aggregate`` + ``ggcn_layer_fused_prebias``: two applications of D.A) and the two-launch block;
(c) gate dropout inside the launch (``ggcn_layer_fused_drop``) on the exported keep masks;
(d) the C entries in a hostile state: NaN wherever they may not write, strided x and out, out = NULL, a pool NULL.

The float64 reference is ``oracle/backward_ref.py``; the gate is the project's own, ``br.TOL[precision] * max(1, max|ref|)``, taken
PER GRAPH (``/ (1 - p)`` under dropout), and a failure names the structure.  Each case asserts the entry calls it made.

Measured on one MI355X, largest error / gate per part: (a) 0.184 (`hub`, out, T = 231, 256 x 256, f16mx8; bf16x3 at most 0.088),
(b) 0.163 (`lower`, x of the two launches, T = 256, f16mx8), (c) 0.129 (`ladder`, out, T = 100, f16mx8), (d) 0.156 (`lower`, out,
``ggcn_layer_fused``, T = 100, f16mx8).  With ``_kernel_adj`` returning ``adj.transpose(1, 2)`` every case of (a) misses on each of
the eight asymmetric structures and on none of `tree`, `complete`, `empty`, `len1`.
"""
import pytest
import torch

from oracle import backward_ref as br
from oracle import wide_structures as ws
from oracle.gpu_support import call_log, count_calls, dev, drop_mask as _drop_mask, make_layer, pkg  # noqa: F401

pytestmark = pytest.mark.gpu

NAN = float("nan")
PRECISIONS = ["bf16x3", "f16mx8"]
FUSED, PREBIAS, DROP, LINEAR, AGGREGATE, LISTS = ("ggcn_layer_fused", "ggcn_layer_fused_prebias", "ggcn_layer_fused_drop", "ggcn_linear",
                                                   "ggcn_aggregate", "ggcn_graph_edge_lists")
COUNTED = (FUSED, PREBIAS, DROP, LINEAR, AGGREGATE, LISTS)


def _layer(pkg, dev, w, b, precision, fused=True):
    """fused_max_t = 256 sends every graph of <= 256 nodes to the one launch, whatever the batch (as tests/test_gpu_parity.py)."""
    return make_layer(pkg, dev, w, b, precision=precision, fused=bool(fused), fused_max_t=256).eval()


def _watch(monkeypatch):
    """``(calls, log)``: the counter and the recorder of ``oracle/gpu_support.py`` on the entries of COUNTED."""
    return count_calls(monkeypatch, COUNTED), call_log(monkeypatch, COUNTED)


def _since(calls, before):
    return {k: calls[k] - before[k] for k in COUNTED if calls[k] != before[k]}


def _last(log, entry):
    """The arguments of the last call of ``entry`` (pointers as integers, NULL: None)."""
    return [a for n, a in log if n == entry][-1]


def _kernel_adj(c):
    """The adjacency the code under test is given (the reference keeps c["adj"])."""
    return c["adj"]


class _Report:
    """Per-graph comparison at the gate: every miss is collected with its structure's name, the largest error / gate is kept."""
    def __init__(self, part, what, names, tol):
        self.part, self.what, self.names, self.tol = part, what, names, tol
        self.fails, self.worst = [], (0.0, "-", "-")

    def gate(self, label, got, ref):
        assert got.dtype == torch.float32 and got.shape == ref.shape, (label, got.dtype, tuple(got.shape), tuple(ref.shape))
        G = ref.shape[0]
        err = (got.double() - ref).abs().reshape(G, -1).amax(1).cpu().tolist()
        scale = ref.abs().reshape(G, -1).amax(1).clamp(min=1.0).cpu().tolist()
        for name, e, s in zip(self.names, err, scale):
            gate = self.tol * s
            ratio = e / gate if e == e else float("inf")
            if not e <= gate:
                self.fails.append("%s on `%s`: max|diff| %.3g > gate %.3g" % (label, name, e, gate))
            if ratio > self.worst[0]:
                self.worst = (ratio, name, label)

    def done(self):
        print("[part %s] %s: largest error / gate %.3f on `%s` (%s)" % ((self.part, self.what) + self.worst))
        assert not self.fails, "%s: %d misses: %s" % (self.what, len(self.fails), "; ".join(self.fails))


def _same_bits(fails, label, got, ref, names):
    """got == ref bit for bit, per graph."""
    G = ref.shape[0]
    bad = (got.reshape(G, -1) != ref.reshape(G, -1)).any(1).cpu().tolist()
    fails.extend("%s differs on `%s`" % (label, n) for n, b in zip(names, bad) if b)


_CASES = {}     # inputs on the device and the float64 reference, computed once per case and left unchanged


def _layer_case(dev, T, K, F):
    key = ("layer", T, K, F)
    if key not in _CASES:
        c = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in ws.layer_inputs(T, K, F).items()}
        with torch.no_grad():
            c["ref"] = br.gated_layer_ref(c["x"], c["adj"], c["w"], c["b"], c["sg"], c["ga"], c["gb"])
        assert c["ref"][0].dtype == torch.float64
        _CASES[key] = c
    return _CASES[key]


def _block_case(dev, T):
    key = ("block", T)
    if key not in _CASES:
        c = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in ws.block_inputs(T).items()}
        with torch.no_grad():
            c["ref"] = br.block_ref(c["x"], c["adj"], c["g1"], c["g2"], c["w1"], c["b1"], c["w2"], c["b2"])
        assert c["ref"]["out"].dtype == torch.float64
        _CASES[key] = c
    return _CASES[key]


# ================================================================ (a) the layer
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("T,K,F", ws.LAYER_CASES)
def test_layer_on_directed_and_extreme_graphs(pkg, dev, monkeypatch, T, K, F, precision):
    from ed_gated_gcn_amd import synth
    c = _layer_case(dev, T, K, F)
    names, G = c["names"], len(c["names"])
    what = "T=%d K=%d F=%d %s" % (T, K, F, precision)
    fused, unfused = _layer(pkg, dev, c["w"], c["b"], precision, True), _layer(pkg, dev, c["w"], c["b"], precision, False)
    ad = _kernel_adj(c).contiguous()
    csr = pkg.BatchedCSR.from_dense(ad)
    assert csr.is_binary and csr.rowmask is not None and fused.takes_fused_path(c["x"], csr) and not unfused.takes_fused_path(c["x"], csr)
    kw = dict(store_gate=c["sg"], pool_gate_a=c["ga"], pool_gate_b=c["gb"], want_pool_a=True, want_pool_b=True)
    calls, log = _watch(monkeypatch)
    with torch.no_grad():
        # ---- the one launch, on the edge lists made once per adjacency (129..256 nodes)
        before = dict(calls)
        got = fused.forward_gated(c["x"], csr, **kw)
        assert _since(calls, before) == ({FUSED: 1, LISTS: 1} if T > 128 else {FUSED: 1}), (what, _since(calls, before))
        assert (_last(log, FUSED)[4] is not None) == (T > 128), "%s: edge lists handed over: %r" % (what, _last(log, FUSED)[4])
        # ---- pools only
        before = dict(calls)
        pools_only = fused.forward_gated(c["x"], csr, pool_gate_a=c["ga"], pool_gate_b=c["gb"], want_out=False, want_pool_a=True, want_pool_b=True)
        assert _since(calls, before) == {FUSED: 1} and _last(log, FUSED)[13] is None, (what, _since(calls, before))
        # ---- a host-collated CSR of the same graphs
        rp, ci, _ = synth.csr_from_dense_host(ad.cpu().numpy())
        host = pkg.BatchedCSR.from_arrays(rp, ci, G, T, dev)
        before = dict(calls)
        via_host = fused.forward_gated(c["x"], host, **kw)
        assert _since(calls, before) == ({FUSED: 1, LISTS: 1} if T > 128 else {FUSED: 1}), (what, _since(calls, before))
        # ---- 129..256 nodes: the lists built inside the workgroup from the row masks
        inside = None
        if T > 128:
            monkeypatch.setenv("GGCN_EDGE_LISTS", "0")
            before = dict(calls)
            inside = fused.forward_gated(c["x"], csr, **kw)
            assert _since(calls, before) == {FUSED: 1} and _last(log, FUSED)[4] is None, (what, _since(calls, before))
            monkeypatch.delenv("GGCN_EDGE_LISTS")
        # ---- linear + aggregate (the general CSR kernel) on the same batch
        before = dict(calls)
        two = unfused.forward_gated(c["x"], csr, **kw)
        assert _since(calls, before) == {LINEAR: 1, AGGREGATE: 1}, (what, _since(calls, before))
    torch.cuda.synchronize()
    rep = _Report("a", what, names, br.TOL[precision])
    for label, gv, rv in zip(("out", "pool a", "pool b"), got, c["ref"]):
        rep.gate(label, gv, rv)
    one = rep.worst
    for label, gv, rv in zip(("out", "pool a", "pool b"), two, c["ref"]):
        rep.gate("linear + aggregate " + label, gv, rv)
    print("[part a] %s: the one launch alone: largest error / gate %.3f on `%s` (%s)" % ((what,) + one))
    assert pools_only[0] is None
    _same_bits(rep.fails, "pools-only pool a", pools_only[1], got[1], names)
    _same_bits(rep.fails, "pools-only pool b", pools_only[2], got[2], names)
    for label, gv, hv in zip(("out", "pool a", "pool b"), got, via_host):
        _same_bits(rep.fails, "host-collated CSR " + label, hv, gv, names)
    if inside is not None:
        for label, gv, iv in zip(("out", "pool a", "pool b"), got, inside):
            _same_bits(rep.fails, "lists built in the workgroup " + label, iv, gv, names)
    rep.done()


# ================================================================ (b) the folded evaluation and the two-launch block
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("T", ws.BLOCK_T)
def test_folded_evaluation_and_two_launch_block(pkg, dev, monkeypatch, T, precision):
    c = _block_case(dev, T)
    names, ref = c["names"], c["ref"]
    what = "block T=%d H=%d %s" % (T, ws.BLOCK_H, precision)
    l1, l2 = _layer(pkg, dev, c["w1"], c["b1"], precision), _layer(pkg, dev, c["w2"], c["b2"], precision)
    csr = pkg.BatchedCSR.from_dense(_kernel_adj(c).contiguous())
    calls, log = _watch(monkeypatch)
    with torch.no_grad():
        before = dict(calls)
        ev = pkg.gated_gcn_block(c["x"], csr, c["g1"], c["g2"], l1, l2, want=("out",))
        made = _since(calls, before)
        made.pop(LINEAR, None)      # (W12 = W1.W2 and mid = W2^T.b1 are folded once per weight, by the exact fp32 linear)
        assert made == {AGGREGATE: 1, PREBIAS: 1}, (what, made)
        assert _last(log, PREBIAS)[13] is None          # no [B,T,H] store was asked for
        before = dict(calls)
        evx = pkg.gated_gcn_block(c["x"], csr, c["g1"], c["g2"], l1, l2, want=("x", "out"))
        assert _since(calls, before) == {AGGREGATE: 1, PREBIAS: 1}, (what, _since(calls, before))
        before = dict(calls)
        full = pkg.gated_gcn_block(c["x"], csr, c["g1"], c["g2"], l1, l2, want_gcn1=True)
        assert _since(calls, before) == ({FUSED: 2, LISTS: 1} if T > 128 else {FUSED: 2}), (what, _since(calls, before))
    torch.cuda.synchronize()
    assert all(ev[k] is None for k in ("gcn1", "x1", "y1", "xy", "x"))
    rep = _Report("b", what, names, br.TOL[precision])
    rep.gate("folded out", ev["out"], ref["out"])
    rep.gate("folded x", evx["x"], ref["x"])
    _same_bits(rep.fails, "folded out with x", evx["out"], ev["out"], names)
    for k in ("gcn1", "x1", "y1", "x", "out"):
        rep.gate("two launches " + k, full[k], ref[k])
    xy, xy_ref = float(full["xy"]), float(ref["xy"])
    print("[part b] %s: xy %.6g against %.6g" % (what, xy, xy_ref))
    if not abs(xy - xy_ref) <= 1e-4 * max(1.0, abs(xy_ref)):
        rep.fails.append("xy %.6g against %.6g" % (xy, xy_ref))
    rep.done()


# ================================================================ (c) gate dropout inside the launch
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("T,K,F", ws.DROP_CASES)
def test_gate_dropout_inside_the_launch(pkg, dev, monkeypatch, T, K, F, precision):
    c = _layer_case(dev, T, K, F)
    names, G = c["names"], len(c["names"])
    p, seed, streams = 0.25, 2 ** 40 + 99, (0, 1, 2)
    what = "dropout T=%d K=%d F=%d %s" % (T, K, F, precision)
    m = _layer(pkg, dev, c["w"], c["b"], precision)
    csr = pkg.BatchedCSR.from_dense(_kernel_adj(c).contiguous())
    keep = tuple(None if s == 0 else _drop_mask(pkg, dev, G * T, F, p, seed, s).view(G, T, F).double() for s in streams)
    assert 0.2 < float((keep[1] == 0).double().mean()) < 0.3 and not torch.equal(keep[1], keep[2])
    with torch.no_grad():
        ref = br.gated_layer_ref(c["x"], c["adj"], c["w"], c["b"], c["sg"], c["ga"], c["gb"], keep=keep)
    calls, log = _watch(monkeypatch)
    with torch.no_grad():
        got = m.forward_gated(c["x"], csr, store_gate=c["sg"], pool_gate_a=c["ga"], pool_gate_b=c["gb"], want_pool_a=True, want_pool_b=True,
                              dropout=(p, seed, streams))
    assert _since(calls, {k: 0 for k in COUNTED}) == {DROP: 1}, (what, dict(calls))
    torch.cuda.synchronize()
    rep = _Report("c", what, names, br.TOL[precision] / (1.0 - p))
    for label, gv, rv in zip(("out", "pool a", "pool b"), got, ref):
        rep.gate(label, gv, rv)
    rep.done()


# ================================================================ (d) the C entries in a hostile state
@pytest.mark.parametrize("entry", [FUSED, PREBIAS])
@pytest.mark.parametrize("T", ws.HOSTILE_T)
def test_c_entries_in_a_hostile_state(pkg, dev, T, entry):
    """The Python layer always hands these entries contiguous outputs: the scalar-store form on an unaligned ldo and writes outside
    [B*T, F] are reached only here.  ldo = F + 3 with ldx = K + 3: rows at odd offsets, the general main loop and the scalar store
    form; F + 4 / K + 4: 16-byte rows, the fast main loop and the vector store form.  x's pad columns, out's pad columns and guard
    row and the pools' guard row are NaN before the call."""
    from ed_gated_gcn_amd import _capi
    lib = pkg.load_library()
    P, st = _capi.ptr, _capi.stream_of(dev)
    K, F = ws.HOSTILE_SHAPE
    c = _layer_case(dev, T, K, F)
    names, G = c["names"], len(c["names"])
    csr = pkg.BatchedCSR.from_dense(_kernel_adj(c).contiguous())
    lists = csr.edge_lists
    assert (lists is not None) == (T > 128)
    if entry == PREBIAS:
        xp, wp = ws.with_prebias(c["x"], c["w"], c["pre"])
        with torch.no_grad():
            ref = br.gated_layer_ref(xp, c["adj"], wp, c["b"], c["sg"], c["ga"], c["gb"])
    else:
        ref = c["ref"]
    m = _layer(pkg, dev, c["w"], c["b"], "f16mx8")
    bias = m.bias.detach()
    for precision in PRECISIONS:
        with torch.cuda.device(dev):
            pack = m._packed_weight(lib, st, precision=precision)
        for pad in (3, 4):
            ldx, ldo = K + pad, F + pad
            xbuf = torch.full((G * T, ldx), NAN, device=dev)
            xbuf[:, :K] = c["x"].reshape(G * T, K)
            xv = xbuf[:, :K]
            assert xv.data_ptr() == xbuf.data_ptr() and xv.stride(0) == ldx

            def call(with_out, with_a, with_b):
                out = torch.full((G * T + 1, ldo), NAN, device=dev)
                pa, pb = torch.full((G + 1, F), NAN, device=dev), torch.full((G + 1, F), NAN, device=dev)
                tail = (G, T, K, F, P(c["sg"]), P(c["ga"]), P(c["gb"]), P(out) if with_out else None, ldo, P(pa) if with_a else None,
                        P(pb) if with_b else None)
                if entry == PREBIAS:
                    rc = lib.ggcn_layer_fused_prebias(P(xv), ldx, P(pack), P(csr.rowmask), P(bias), P(c["pre"]), *tail, _capi.PREC[precision], st)
                else:
                    rc = lib.ggcn_layer_fused(P(xv), ldx, P(pack), P(csr.rowmask), P(lists), P(bias), *tail, None, None, None,
                                              _capi.PREC[precision], st)
                _capi.check(rc, entry)
                torch.cuda.synchronize()
                return out, pa, pb
            what = "%s T=%d %s ldx=K+%d ldo=F+%d" % (entry, T, precision, pad, pad)
            full = call(True, True, True)
            out, pa, pb = full
            inner = out[:G * T, :F].reshape(G, T, F)
            assert not bool(torch.isnan(inner).any()), what + ": NaN inside [B*T, F] of out"
            assert not bool(torch.isnan(pa[:G]).any()) and not bool(torch.isnan(pb[:G]).any()), what + ": NaN inside [B, F] of a pool"
            assert bool(torch.isnan(out[G * T]).all()) and bool(torch.isnan(out[:, F:]).all()), what + ": wrote outside [B*T, F]"
            assert bool(torch.isnan(pa[G]).all()) and bool(torch.isnan(pb[G]).all()), what + ": wrote past B pool rows"
            assert bool(torch.isnan(xbuf[:, K:]).all())
            rep = _Report("d", what, names, br.TOL[precision])
            for label, gv, rv in zip(("out", "pool a", "pool b"), (inner, pa[:G], pb[:G]), ref):
                rep.gate(label, gv, rv)
            for asked in ((False, True, True), (True, False, True), (True, True, False)):
                part = call(*asked)
                for label, want, pv, fv in zip(("out", "pool a", "pool b"), asked, part, full):
                    if want:     # (NaN == NaN is false: the guard rows and pad columns are compared as bits)
                        if not torch.equal(pv.view(torch.int32), fv.view(torch.int32)):
                            rep.fails.append("%s with (out, pool a, pool b) = %s is not the full call's" % (label, asked))
                    elif not bool(torch.isnan(pv).all()):
                        rep.fails.append("%s = NULL was written" % label)
            rep.done()
