"""The f16mx8 range report on every launch path, probed with lone elements: "no silent wrong answer".

``precision="f16mx8"`` (the default) matches the reference's fp32 matmul only for activations of |x| <= 448 and hidden values below
65504.  What stands between out-of-window data and a silently degraded result is the sticky device flag the kernels raise themselves
(``f16mx8_core.h``: ``range_verdict``), one copy per translation unit, collected by ``ggcn_range_flag``.  The contract checked here,
for every launch of the table in ``CASES``: after the launch the raw bits are read (and cleared) with ``ggcn_range_flag``;

* a probe that violates a limit sets EXACTLY the expected bits, and a second read returns 0;
* when no bit is set, every output is finite and within ``1e-4 * max(1, max|ref|)`` of a float64 reference computed here on the CPU.

Every case asserts the C entry that ran (a call recorder on the loaded library), its shape arguments, its row stride and, for graphs
of 33..256 nodes, the row slot the launcher picks for that T.  B = 9 = two whole four-graph tiles and a partial one; K = F = 64 is
the fast shape (buffer loads); the other shapes select the other instantiations (``AVEC`` / ``KFULL`` / ``FULLT`` / ``BUF``):
B = 8 with T = 32 is ``FULLT``; a row stride of K + 3 floats is ``AVEC`` false (element loads); K = 80 is ``KFULL`` false (the launchers
ask ``K % 32``, the depth of a stage: the last stage's columns 80..95 are masked); K = 96 keeps ``KFULL`` and runs an odd number of
stages, the tail of the double-buffered loop.

The expected bits are ``range_verdict``'s three comparisons, written out in ``_verdict``: ``> 448`` WINDOW, ``>= 65504`` OVERFLOW,
and -- on the launches that bound their fp16 hidden planes -- ``amax * c (+ max|mid|) >= 65504`` HIDDEN, c = max_f sum_k |w[k,f]|.
The value table runs with c = 0.5, so that no finite probe reaches the hidden bound; an INFINITE activation has an infinite bound
(inf * c), so on those launches ``inf`` sets HIDDEN next to OVERFLOW and WINDOW -- "NaN outputs are possible" is true of it."""
import types

import numpy as np
import pytest
import torch

from oracle.gpu_support import call_log, clean_range_flag, dev, make_layer, pkg, range_bits as _bits  # noqa: F401

pytestmark = pytest.mark.gpu

SEED = 2 ** 40 + 99
DROPOUT = (0.25, SEED, (0, 1, 2))         # the store gate undropped, the two pools on the two keep streams
POISON = 7.0e4                            # finite (v_max3 ignores NaN: NaN would prove nothing)
INF = float("inf")
UP448 = float(np.nextafter(np.float32(448.0), np.float32(np.inf)))
BELOW_HALF_MAX = float(np.nextafter(np.float32(65504.0), np.float32(0.0)))
OVERFLOW, WINDOW, HIDDEN = 1, 2, 4        # include/ggcn.h GGCN_RANGE_* (test_the_bits_are_the_bindings pins them to _capi)
TABLE = [(448.0, 0), (UP448, WINDOW), (BELOW_HALF_MAX, WINDOW), (65504.0, OVERFLOW | WINDOW), (POISON, OVERFLOW | WINDOW),
         (INF, OVERFLOW | WINDOW)]
ENTRIES = ("ggcn_layer_fused", "ggcn_layer_fused_drop", "ggcn_layer_fused_prebias", "ggcn_layer_fused_weighted",
           "ggcn_layer_fused_weighted_wide", "ggcn_layer_fused_weighted_drop", "ggcn_layer_fused_weighted_wide_drop", "ggcn_block_fused",
           "ggcn_layer_fused_bf16", "ggcn_layer_fused_bf16_drop", "ggcn_layer_fused_bf16_wide", "ggcn_block_fused_bf16", "ggcn_layer_fused_h",
           "ggcn_linear", "ggcn_linear_h", "ggcn_linear_bf16", "ggcn_aggregate", "ggcn_aggregate_h", "ggcn_aggregate_bf16")
# where (B, T, K, F) sit in an entry's arguments (include/ggcn.h); ggcn_linear takes (M, K, F) instead
SHAPE_AT = {"ggcn_layer_fused": 6, "ggcn_layer_fused_drop": 6, "ggcn_layer_fused_prebias": 6, "ggcn_layer_fused_weighted": 6,
            "ggcn_layer_fused_weighted_drop": 6, "ggcn_layer_fused_weighted_wide": 5, "ggcn_layer_fused_weighted_wide_drop": 5,
            "ggcn_block_fused": 9}


def _verdict(amax, bounds=()):
    """``range_verdict`` (f16mx8_core.h) of a launch whose largest |x| is ``amax``; ``bounds``: the (c, add) of its hidden bounds."""
    bits = 0
    if amax > 448.0:
        bits |= WINDOW
    if amax >= 65504.0:
        bits |= OVERFLOW
    if any(amax * c + add >= 65504.0 for c, add in bounds):
        bits |= HIDDEN
    return bits


def _slot_rows(T):
    """Rows of the graph slot launch_fused / layer_fused_weighted_wide pick: ``sb = T <= 64 ? 2 : T <= 128 ? 4 : 8`` blocks of 32."""
    return 32 if T <= 32 else 64 if T <= 64 else 128 if T <= 128 else 256


# ---------------------------------------------------------------- fixtures
@pytest.fixture(autouse=True)
def clean_flag(pkg, dev):
    """Every test starts and ends with the flag clear, whatever ran before: the order does not matter."""
    yield from clean_range_flag(pkg, dev)


@pytest.fixture
def guard(monkeypatch):
    """The lazy half out of the way: ``range_guard.after`` would read AND CLEAR the flag behind a forward of its choosing.  Returns the
    list of devices it was called with."""
    from ed_gated_gcn_amd import range_guard
    calls = []
    monkeypatch.setattr(range_guard, "after", calls.append)
    monkeypatch.setattr(range_guard, "before", lambda d: None)
    return calls


@pytest.fixture
def log(monkeypatch, pkg):
    """``[(entry, [arguments])]`` of every layer, block, linear and aggregate entry called from here on."""
    return call_log(monkeypatch, ENTRIES)


# ---------------------------------------------------------------- the cases
def _spec(id, path, T, entries, B=9, K=64, F=64, layout="contig", slot=32, **options):
    """slot: the rows of the graph slot the case is meant for (32: one of a tile's four; 64: two graphs per workgroup; 128; 256)."""
    return pytest.param(types.SimpleNamespace(id=id, path=path, T=T, entries=entries, B=B, K=K, F=F, layout=layout, slot=slot,
                                              options=options), id=id)


L, LD, PRE, BLK, LIN, AGG = ("ggcn_layer_fused", "ggcn_layer_fused_drop", "ggcn_layer_fused_prebias", "ggcn_block_fused", "ggcn_linear",
                             "ggcn_aggregate")
CASES = [
    _spec("fused-T20", "fused", 20, [L]),
    _spec("fused-T32", "fused", 32, [L]),
    _spec("fused-T32-B8-whole-tiles", "fused", 32, [L], B=8),                      # FULLT
    _spec("fused-T20-F256-both-verdict-forms", "fused", 20, [L], F=256),           # tiles 0, 1: dma_range_verdict; tile 2: fused_range_verdict
    _spec("fused-T32-F256-both-verdict-forms", "fused", 32, [L], F=256),
    _spec("fused-T20-K96-three-stages", "fused", 20, [L], K=96),                   # an odd number of 32-deep stages (KFULL stays true)
    _spec("fused-T20-K80-tail", "fused", 20, [L], K=80),                           # KFULL false: the K-tail mask
    _spec("fused-T20-stride-K+3", "fused", 20, [L], layout="pad3"),                # AVEC false: element loads
    _spec("fused_drop-T20", "fused_drop", 20, [LD]),
    _spec("fused-wide64-T33", "fused", 33, [L], slot=64),
    _spec("fused-wide64-T64", "fused", 64, [L], slot=64),
    _spec("fused-wide64-T33-K96-three-stages", "fused", 33, [L], K=96, slot=64),
    _spec("fused-wide64-T33-K80-tail", "fused", 33, [L], K=80, slot=64),
    _spec("fused-wide64-T33-stride-K+3", "fused", 33, [L], layout="pad3", slot=64),
    _spec("fused-wide128-T65", "fused", 65, [L], slot=128),
    _spec("fused-wide128-T128", "fused", 128, [L], slot=128),
    _spec("fused-wide8-T129", "fused", 129, [L], fused_max_t=256, slot=256),
    _spec("fused-wide8-T256", "fused", 256, [L], fused_max_t=256, slot=256),
    _spec("prebias-T33", "folded_eval", 33, [AGG, PRE], slot=64),
    _spec("prebias-T129", "folded_eval", 129, [AGG, PRE], fused_max_t=256, slot=256),
    _spec("block-full-T20", "block", 20, [BLK]),
    _spec("block-full-T32", "block", 32, [BLK]),
    _spec("block-full-T32-B8-whole-tiles", "block", 32, [BLK], B=8),
    _spec("block-w12only-T20", "block_eval", 20, [BLK]),
    _spec("block-w12only-T32", "block_eval", 32, [BLK]),
    _spec("two_fused-T20", "two_fused", 20, [L, L]),
    _spec("weighted-T20", "weighted", 20, ["ggcn_layer_fused_weighted"]),
    _spec("weighted-T32", "weighted", 32, ["ggcn_layer_fused_weighted"]),
    _spec("weighted_wide-T33", "weighted_wide", 33, ["ggcn_layer_fused_weighted_wide"], weighted_max_t=128, slot=64),
    _spec("weighted_wide-T100", "weighted_wide", 100, ["ggcn_layer_fused_weighted_wide"], weighted_max_t=128, slot=128),
    _spec("weighted_drop-T20", "weighted_drop", 20, ["ggcn_layer_fused_weighted_drop"], weighted_dropout=True),
    _spec("weighted_wide_drop-T100", "weighted_wide_drop", 100, ["ggcn_layer_fused_weighted_wide_drop"], weighted_max_t=128,
          weighted_dropout=True, slot=128),
    _spec("two_launch-T20", "two_launch", 20, [LIN, AGG], fused=False),
]
# the block paths: path -> (want= of gated_gcn_block, one_launch=, the name dispatch.block_path gives it); every other path is one layer
ALL_OUTPUTS = ("x1", "y1", "xy", "x", "out")
BLOCK_CALLS = {"block": (ALL_OUTPUTS, True, "block"), "block_eval": (("out",), True, "block"), "two_fused": (ALL_OUTPUTS, False, "two_fused"),
               "folded_eval": (("out",), True, "folded_eval")}
BLOCKS = tuple(BLOCK_CALLS)
DROPS = ("fused_drop", "weighted_drop", "weighted_wide_drop")


def _adjacency(B, T, weighted, isolate, gen):
    a = (torch.rand(B, T, T, generator=gen) < 3.0 / T).double()
    a = ((a + a.transpose(1, 2) + torch.eye(T, dtype=torch.float64)) > 0).double()
    if weighted:
        a = a * (0.25 + 0.5 * torch.rand(B, T, T, generator=gen)).float().double()
    for n in isolate:          # a node with its self loop alone: D.A.x of that row is x / 2, exactly
        a[:, n, :] = 0.0
        a[:, :, n] = 0.0
        a[:, n, n] = 1.0
    return a


def _colsum(w):
    return float(w.double().abs().sum(0).max())


def _scaled(w, c):
    """``w`` (float32) rescaled so that max_f sum_k |w[k,f]| is about ``c``."""
    return (w.double() * (c / _colsum(w))).float()


def _gc(x, a, w, b):
    """models/gcn.py:30-45 in float64: (adj @ (x @ W)) / (rowsum(adj) + 1) + b."""
    return (a @ (x @ w)) / (a.sum(2, keepdim=True) + 1.0) + b


class Case:
    """One launch path at one shape: the layers on the device, the float64 operands on the CPU, ``run`` and ``ref``.
    ``c``: the column-sum scale of W (W1); ``c12`` / ``mid``: of the block's folded W12 = W1.W2 and of max|W2^T.b1|; ``w1_std``: W1 =
    w1_std * randn instead."""

    def __init__(self, pkg, dev, s, c=0.5, c12=None, mid=None, w1_std=None, precision="f16mx8"):
        from ed_gated_gcn_amd import _capi
        self.pkg, self.dev, self.s, self.path = pkg, dev, s, s.path
        B, T, K, F = s.B, s.T, s.K, s.F
        self.block = s.path in BLOCKS
        assert not self.block or K == F
        gen = torch.Generator().manual_seed(1000 * T + 10 * B + K + F)
        self.weighted = s.path.startswith("weighted")
        # the folded eval hands the layer Z = D.A.X, not X: its probe nodes keep their self loop alone and the probes are doubled
        self.nodes = [0, T - 1]
        self.scale = 2.0 if s.path == "folded_eval" else 1.0
        self.adj = _adjacency(B, T, self.weighted, self.nodes if s.path == "folded_eval" else [], gen)
        w1 = torch.randn(K, F, generator=gen)
        w1 = w1_std * w1 if w1_std else _scaled(w1, c)
        b1 = 0.1 * torch.randn(F, generator=gen)
        self.x0 = torch.randn(B, T, K, generator=gen).clamp_(-4.0, 4.0)
        self.gates = [torch.rand(B, F, generator=gen) for _ in range(3)]
        self.layers = [self._layer(w1, b1, precision)]
        self.w, self.b = [w1.double()], [b1.double()]
        if self.block:
            w2 = _scaled(torch.randn(F, F, generator=gen), 0.5)
            if c12 is not None:
                w2 = (w2.double() * (c12 / _colsum((w1.double() @ w2.double())))).float()
            if mid is not None:
                b1 = (b1.double() * (mid / float((w2.double().t() @ b1.double()).abs().max()))).float()
                self.layers = [self._layer(w1, b1, precision)]
                self.b = [b1.double()]
            b2 = 0.1 * torch.randn(F, generator=gen)
            self.layers.append(self._layer(w2, b2, precision))
            self.w.append(w2.double())
            self.b.append(b2.double())
        self.c1 = _colsum(w1)
        self.c12 = _colsum(self.w[0] @ self.w[1]) if self.block else None
        self.mid = float((self.w[1].t() @ self.b[0]).abs().max()) if self.block else None
        # the hidden bounds range_verdict is handed on this path
        self.bounds = []
        if s.path in ("fused", "fused_drop", "weighted", "weighted_drop") and T <= 32:
            self.bounds = [(self.c1, 0.0)]
        elif s.path in ("block", "two_fused"):
            self.bounds = [(self.c1, 0.0)] + ([(self.c12, self.mid)] if s.path == "block" else [])
        elif s.path == "block_eval":
            self.bounds = [(self.c12, self.mid)]
        self.dropout = DROPOUT if s.path in DROPS else None
        self.keep = [torch.ones(B, T, F, dtype=torch.float64)] * 3
        if self.dropout:
            lib = pkg.load_library()
            self.keep = [torch.ones(B, T, F, dtype=torch.float64)]
            for stream in (1, 2):
                m = torch.empty(B * T, F, dtype=torch.float32, device=dev)
                _capi.check(lib.ggcn_dropout_mask(B * T, F, DROPOUT[0], SEED, stream, _capi.ptr(m), _capi.stream_of(dev)), "ggcn_dropout_mask")
                self.keep.append(m.view(B, T, F).double().cpu())
        self.csr = pkg.BatchedCSR.from_dense(self.adj.float().to(dev))
        assert self.csr.is_binary == (not self.weighted)
        self.gates_d = [g.to(dev) for g in self.gates]

    def _layer(self, w, b, precision):
        m = make_layer(self.pkg, self.dev, w, b, precision=precision, **self.s.options)
        if self.s.path not in DROPS:
            m.requires_grad_(False)
        return m

    def on_device(self, x, layout=None):
        """``x`` [B,T,K] on the device in the case's (or the given) layout, everything AROUND it filled with POISON: "pad4" / "pad3" are
        ``[:, :, :K]`` views of rows of K + 4 / K + 3 floats, "slice" is ``big[1:B+1]`` of a (B+2)-graph tensor."""
        layout = layout or self.s.layout
        B, T, K = x.shape
        if layout == "contig":
            return x.to(self.dev)
        if layout == "slice":
            big = torch.full((B + 2, T, K), POISON)
            big[1:B + 1] = x
            return big.to(self.dev)[1:B + 1]
        pad = {"pad4": 4, "pad3": 3}[layout]
        big = torch.full((B, T, K + pad), POISON)
        big[:, :, :K] = x
        return big.to(self.dev)[:, :, :K]

    def ldx(self, layout=None):
        return self.s.K + {"contig": 0, "slice": 0, "pad4": 4, "pad3": 3}[layout or self.s.layout]

    def check_dispatch(self, xd):
        """The rules name the intended launch for these operands (a case that falls back to linear + aggregate tests nothing)."""
        from ed_gated_gcn_amd import dispatch
        from ed_gated_gcn_amd.gcn import _rows2d
        if self.block:
            want, one, name = BLOCK_CALLS[self.path]
            got = dispatch.block_path(xd, self.csr, self.layers[0], self.layers[1], want, False, one, False)
            assert got == name, got
            if self.path in ("block", "block_eval"):   # B below the eight-wavefront threshold: the four-wavefront kernel (fused_layer.hip)
                assert self.pkg.load_library().ggcn_block_fused_form(self.s.B, self.s.T, self.s.K, self.s.F) == 4
        else:
            rows = None if self.dropout else _rows2d(xd)
            assert dispatch.layer_launch(self.layers[0], xd, self.csr, self.dropout is not None, rows) == self.path

    def run(self, xd):
        """The launch(es); every output as a device tensor."""
        sg, ga, gb = self.gates_d
        if self.block:
            want, one, _ = BLOCK_CALLS[self.path]
            with torch.no_grad():
                r = self.pkg.gated_gcn_block(xd, self.csr, ga, gb, self.layers[0], self.layers[1], want=want, one_launch=one)
            return {k: v for k, v in r.items() if v is not None}
        m = self.layers[0]
        if self.dropout:   # training: the layer under autograd, the keep factors drawn inside the launch
            out, pa, pb = m.forward_gated(xd, self.csr, store_gate=sg, pool_gate_a=ga, pool_gate_b=gb, want_out=True, want_pool_a=True,
                                          want_pool_b=True, dropout=self.dropout)
        else:
            with torch.no_grad():
                out, pa, pb = m.forward_gated(xd, self.csr, store_gate=sg, pool_gate_a=ga, pool_gate_b=gb, want_out=True, want_pool_a=True,
                                              want_pool_b=True)
        return {"out": out.detach(), "pool_a": pa.detach(), "pool_b": pb.detach()}

    def ref(self, x):
        """The same operation in float64 on the CPU (models/gcn.py:30-45, bert_amir5.py:621-640), on the exported keep factors."""
        x, a = x.double(), self.adj
        sg, ga, gb = (g.double()[:, None, :] for g in self.gates)
        if not self.block:
            y = _gc(x, a, self.w[0], self.b[0])
            return {"out": y * sg * self.keep[0], "pool_a": (y * ga * self.keep[1]).max(1)[0], "pool_b": (y * gb * self.keep[2]).max(1)[0]}
        gcn1 = _gc(x, a, self.w[0], self.b[0])
        x1, y1 = (gcn1 * ga).max(1)[0], (gcn1 * gb).max(1)[0]
        xo = gb * _gc(gcn1, a, self.w[1], self.b[1])
        r = {"x1": x1, "y1": y1, "xy": (x1 * y1).sum(1).mean(), "x": xo, "out": xo.max(1)[0]}
        return r if self.path in ("block", "two_fused") else {"out": r["out"]}

    def positions(self):
        """First and last column (K = 80, 96: one of the last 32-deep stage too) x first and last node x a graph in each of a tile's four slots
        (graph 1: the second graph of a 64-row slot's workgroup) and the last graph (B = 9: the partial tile's only one)."""
        B, K = self.s.B, self.s.K
        cols = [0, K - 1] + ([70] if K in (80, 96) else [])
        return [(g, n, k) for g in sorted({0, 1, 2, 3, B - 1}) for n in self.nodes for k in cols]


def _check_calls(case, log, layout=None):
    """The recorded entries are the case's, with its shape, its row stride and f16mx8 where the entry takes a precision."""
    s = case.s
    assert [c[0] for c in log] == s.entries, [c[0] for c in log]
    assert log[0][1][1] == case.ldx(layout), "%s: row stride %r, meant %d" % (log[0][0], log[0][1][1], case.ldx(layout))
    for name, a in log:
        if name in SHAPE_AT:
            i = SHAPE_AT[name]
            assert a[i:i + 4] == [s.B, s.T, s.K, s.F], (name, a[i:i + 4])
            assert _slot_rows(a[i + 1]) == s.slot, "%s: T = %d takes the %d-row slot, the case is meant for %d" % (name, a[i + 1], _slot_rows(a[i + 1]), s.slot)
        if name == "ggcn_layer_fused_prebias":   # its input is Z = D.A.X, made contiguous inside the call whatever X's layout: the layouts
            assert a[1] == s.K                   # of the false-alarm test reach ggcn_aggregate alone on this path (log[0], above)
        if name == "ggcn_linear":
            assert a[7:11] == [s.B * s.T, s.K, s.F, 2], a[7:11]
        if name in ("ggcn_layer_fused", "ggcn_layer_fused_prebias", "ggcn_block_fused", "ggcn_layer_fused_weighted", "ggcn_layer_fused_weighted_wide"):
            assert a[-2] == 2, "%s: precision code %r" % (name, a[-2])           # GGCN_PREC_F16MX8
        if name in ("ggcn_layer_fused_drop", "ggcn_layer_fused_weighted_drop", "ggcn_layer_fused_weighted_wide_drop"):
            assert a[-7] == 2 and a[-6:-1] == [DROPOUT[0], SEED, 0, 1, 2], a[-7:-1]


def _in_gate(got, want, what):
    """Finite and within the project's parity gate, 1e-4 * max(1, max|ref|), output by output."""
    assert set(want) <= set(got), (what, sorted(got))
    for k, r in want.items():
        g = got[k].detach().double().cpu().reshape(r.shape)
        assert bool(torch.isfinite(g).all()), "%s: %s is not finite" % (what, k)
        err, gate = float((g - r).abs().max()), 1e-4 * max(1.0, float(r.abs().max()))
        assert err <= gate, "%s: %s max|diff| %.3g > gate %.3g and no bit set: a silent wrong answer" % (what, k, err, gate)


def _probe(case, xd, x0, pos, value, expected, what):
    """One lone element: launch, exact bits, reported once; silent means in gate.  The element is restored."""
    g, n, k = pos
    xd[g, n, k] = value
    try:
        got = case.run(xd)
        bits = _bits(case.pkg, case.dev)
        assert bits == expected, "%s: x[%d,%d,%d] = %r set bits %d, expected %d" % (what, g, n, k, value, bits, expected)
        assert _bits(case.pkg, case.dev) == 0, "%s: the second read is not 0 (reported once, then cleared)" % what
        if expected == 0:
            x = x0.clone()
            x[g, n, k] = value
            _in_gate(got, case.ref(x), "%s x[%d,%d,%d] = %r" % (what, g, n, k, value))
    finally:
        xd[g, n, k] = float(x0[g, n, k])


def test_the_bits_are_the_bindings(pkg):
    from ed_gated_gcn_amd import _capi
    assert (_capi.RANGE_OVERFLOW, _capi.RANGE_WINDOW, _capi.RANGE_HIDDEN) == (OVERFLOW, WINDOW, HIDDEN)
    assert all(_verdict(v) == b for v, b in TABLE)          # the table is range_verdict's first two comparisons


# ---------------------------------------------------------------- 1. lone elements at the limits, on every path
@pytest.mark.parametrize("s", CASES)
def test_lone_elements_at_the_limits_set_exactly_their_bits(pkg, dev, guard, log, s):
    """Clean data (randn clipped to |x| <= 4): the intended entry ran, silent, in gate.  Then every value of the table, in both signs,
    at every position of ``Case.positions``: exactly the expected bits, a second read 0, and where no bit is expected the output in
    gate.  (Folded eval: the layer splits Z = D.A.X; the probed nodes keep their self loop alone, so Z there is x / 2 exactly and the
    probes are the table's values doubled.)"""
    case = Case(pkg, dev, s)
    xd = case.on_device(case.x0)
    case.check_dispatch(xd)
    case.run(xd)                       # builds the cached operands (weight images, the block's fold)
    del log[:], guard[:]
    got = case.run(xd)
    _check_calls(case, log)
    assert _bits(pkg, dev) == 0, "clean data raised the flag"
    _in_gate(got, case.ref(case.x0), s.id + " clean")
    for pos in case.positions():
        for value, bits in TABLE:
            for sign in (1.0, -1.0):
                expected = _verdict(value, case.bounds)
                assert (expected & ~HIDDEN) == bits and (expected == bits or value == INF)    # the table; inf: an infinite hidden bound
                _probe(case, xd, case.x0, pos, sign * value * case.scale, expected, s.id)


# ---------------------------------------------------------------- 2. false alarms: poison the layer was never given
@pytest.mark.parametrize("s", CASES)
def test_poison_around_the_data_raises_nothing(pkg, dev, guard, log, monkeypatch, s):
    """7e4 in the pad columns of a strided view (row stride K + 4: still the vector / buffer form; K + 3: element loads), in the
    graphs before and after a batch slice, and in every float32 buffer the call allocates for its outputs: the flag stays 0 and the
    output stays in gate.  A report here would make ``forward`` raise on clean production data.

    What this guards is the ADDRESSING: a launch that reads a column past K, a row past the batch slice (a buffer descriptor that is
    too long, a padding lane that is not clamped) or its own output buffer meets the poison.  It does NOT guard the ``in ? x : 0``
    select in front of ``split4``: the loads of a K tail and of padding rows are clamped first (``gk < K ? gk : 0``, ``avalid ? node :
    0``), so without the select a lane splits ``x[row][0]`` or node 0 of the batch again -- data the launch was given, finite here --
    the zero tail of the weight image and the zero columns of the graph operands multiply it away, and the buffer-load forms compile
    no select at all.  Flag and outputs are the same with and without it on finite data, and non-finite data is reported either way:
    no test that only calls the launches can tell (tried: the library built without the select passes this whole file).  On the
    folded eval the layouts reach ``ggcn_aggregate``; the prebias launch itself always reads the contiguous Z."""
    case = Case(pkg, dev, s)
    want = case.ref(case.x0)
    case.run(case.on_device(case.x0, "contig"))
    real_empty = torch.empty

    def poisoned_empty(*a, **kw):
        t = real_empty(*a, **kw)
        return t.fill_(POISON) if t.dtype == torch.float32 and t.is_cuda else t
    for layout in ("pad4", "pad3", "slice"):
        xd = case.on_device(case.x0, layout)
        assert xd.stride(1) == case.ldx(layout) and not (layout != "slice" and xd.is_contiguous())
        del log[:]
        with monkeypatch.context() as mp:
            mp.setattr(torch, "empty", poisoned_empty)
            got = case.run(xd)
        _check_calls(case, log, layout)
        assert _bits(pkg, dev) == 0, "%s %s: a report raised by data the layer was never given" % (s.id, layout)
        _in_gate(got, want, "%s %s" % (s.id, layout))


# ---------------------------------------------------------------- 3. the hidden-value bound
HIDDEN_CASES = [
    (_spec("fused-T20", "fused", 20, [L]), {"c": 200.0}, "c1"),
    (_spec("fused-T32-F256-both-verdict-forms", "fused", 32, [L], F=256), {"c": 200.0}, "c1"),
    (_spec("fused_drop-T20", "fused_drop", 20, [LD]), {"c": 200.0}, "c1"),
    (_spec("weighted-T20", "weighted", 20, ["ggcn_layer_fused_weighted"]), {"c": 200.0}, "c1"),
    (_spec("weighted_drop-T20", "weighted_drop", 20, ["ggcn_layer_fused_weighted_drop"], weighted_dropout=True), {"c": 200.0}, "c1"),
    (_spec("block-full-T20-against-W1", "block", 20, [BLK]), {"c": 200.0, "c12": 20.0}, "c1"),
    (_spec("block-full-T20-against-W12-and-mid", "block", 20, [BLK]), {"c": 20.0, "c12": 200.0, "mid": 2000.0}, "c12"),
    (_spec("block-w12only-T32-against-W12-and-mid", "block_eval", 32, [BLK]), {"c": 20.0, "c12": 200.0, "mid": 2000.0}, "c12"),
]


@pytest.mark.parametrize("s,scales,which", [pytest.param(p.values[0], sc, w, id=p.id) for p, sc, w in HIDDEN_CASES])
def test_hidden_value_bound_within_one_percent(pkg, dev, guard, log, s, scales, which):
    """c = max_f sum_k |w[k,f]| about 200 and one in-window activation a: ``a * c (+ max|mid|) = 0.99 * 65504`` stays silent (and in
    gate), ``1.01 * 65504`` sets HIDDEN alone.  The bound's only slack is the fp16 rounding of the packed weights, 2^-11 relative: 1 %
    clears it and keeps the test sharp.  The block's W12 case has max|mid| = 2000 > 1 % of 65504: a verdict without it stays silent."""
    case = Case(pkg, dev, s, **scales)
    c, add = (case.c1, 0.0) if which == "c1" else (case.c12, case.mid)
    other = [b for b in case.bounds if b != (c, add)]
    assert (c, add) in case.bounds and 190.0 < c < 210.0
    lo, hi = (0.99 * 65504.0 - add) / c, (1.01 * 65504.0 - add) / c
    assert 4.0 < lo < hi < 448.0 and all(hi * oc + oa < 0.5 * 65504.0 for oc, oa in other) and 4.0 * c + add < 0.5 * 65504.0
    assert which == "c1" or hi * c < 0.99 * 65504.0          # the W12 case bites on max|mid|
    xd = case.on_device(case.x0)
    case.check_dispatch(xd)
    case.run(xd)
    del log[:]
    got = case.run(xd)
    _check_calls(case, log)
    assert _bits(pkg, dev) == 0
    _in_gate(got, case.ref(case.x0), s.id + " clean")
    K, T, B = s.K, s.T, s.B
    for g in (0, 2, B - 1):            # a whole tile (F = 256: dma_range_verdict) and the partial one (fused_range_verdict)
        for sign in (1.0, -1.0):
            pos = (g, T - 1, K - 1) if sign > 0 else (g, 0, 0)
            _probe(case, xd, case.x0, pos, sign * lo, 0, s.id + " 0.99")
            _probe(case, xd, case.x0, pos, sign * hi, HIDDEN, s.id + " 1.01")


UNBOUNDED = [
    _spec("fused-wide64-T33", "fused", 33, [L], slot=64),
    _spec("fused-wide8-T129", "fused", 129, [L], fused_max_t=256, slot=256),
    _spec("weighted_wide-T33", "weighted_wide", 33, ["ggcn_layer_fused_weighted_wide"], weighted_max_t=128, slot=64),
    _spec("two_launch-T20", "two_launch", 20, [LIN, AGG], fused=False),
]


@pytest.mark.parametrize("s", UNBOUNDED)
def test_launches_without_a_hidden_bound_stay_silent_and_in_gate(pkg, dev, guard, log, s):
    """The same data on the launches that make no hidden bound.  What they promise instead, read from the kernels: the layers of
    33..256 nodes (fused_wide.hip, fused_wide8.hip; the weighted and prebias forms included) split the fp32 accumulators into bf16
    planes, which have fp32's exponent range, and the plain linear stores its fp32 accumulators -- no fp16 value of `hidden`
    exists, so nothing can overflow and nothing is reported: silent AND in gate, for a * c on both sides of 65504."""
    case = Case(pkg, dev, s, c=200.0)
    assert case.bounds == []
    xd = case.on_device(case.x0)
    case.check_dispatch(xd)
    case.run(xd)
    del log[:]
    case.run(xd)
    _check_calls(case, log)
    assert _bits(pkg, dev) == 0
    for a in (0.99 * 65504.0 / case.c1, 1.01 * 65504.0 / case.c1):
        assert 4.0 < a < 448.0
        for g in (0, 1, s.B - 1):
            _probe(case, xd, case.x0, (g, s.T - 1, s.K - 1), a, 0, s.id)


# ---------------------------------------------------------------- 4. the second layer's input
@pytest.mark.parametrize("path,entries,expected", [("two_fused", [L, L], WINDOW), ("block", [BLK], 0)], ids=["two_fused", "block"])
def test_second_layer_input_beyond_the_window(pkg, dev, guard, log, path, entries, expected):
    """W1 = 100 * randn: |x| <= 4 and every hidden bound below 65504, but gcn1 leaves the window.  The second of two layer launches
    SPLITS gcn1 and must say WINDOW; the one-launch block never splits gcn1 (gc2(gc1(x)) = a product of x with W12) and must be
    silent and in gate on the same data."""
    s = _spec(path, path, 20, entries).values[0]
    case = Case(pkg, dev, s, w1_std=100.0)
    want = case.ref(case.x0)
    gcn1 = _gc(case.x0.double(), case.adj, case.w[0], case.b[0])
    m1, c2 = float(gcn1.abs().max()), _colsum(case.w[1])
    assert 1.05 * 448.0 < m1 < 0.5 * 65504.0
    assert 4.0 * case.c1 < 0.99 * 65504.0 and m1 * c2 < 0.99 * 65504.0 and 4.0 * case.c12 + case.mid < 0.99 * 65504.0
    xd = case.on_device(case.x0)
    case.check_dispatch(xd)
    case.run(xd)
    _bits(pkg, dev)
    del log[:]
    got = case.run(xd)
    _check_calls(case, log)
    bits = _bits(pkg, dev)
    assert bits == expected, "%s: bits %d, expected %d (max|gcn1| = %.0f)" % (path, bits, expected, m1)
    assert _bits(pkg, dev) == 0
    if expected == 0:
        _in_gate(got, want, path)


# ---------------------------------------------------------------- 5. the weight image's own report (linear_split.hip's copy)
@pytest.mark.parametrize("transposed", [0, 1])
def test_weight_pack_reports_a_weight_beyond_fp16(pkg, dev, transposed):
    from ed_gated_gcn_amd import _capi
    lib, K, F = pkg.load_library(), 96, 64
    prec = _capi.PREC["f16mx8"]
    w = 0.05 * torch.randn(K, F, generator=torch.Generator().manual_seed(3))
    rows, cols = (F, K) if transposed else (K, F)          # the image of W, or of W^T (the backward's dX)
    pack = torch.empty(lib.ggcn_weight_pack_bytes(rows, cols, prec), dtype=torch.uint8, device=dev)
    for value, expected in ((BELOW_HALF_MAX, 0), (65504.0, OVERFLOW), (POISON, OVERFLOW), (-POISON, OVERFLOW), (INF, OVERFLOW)):
        for k, f in ((K - 1, F - 1), (0, 0)):
            bad = w.clone()
            bad[k, f] = value
            wd = bad.to(dev)
            _capi.check(lib.ggcn_weight_pack(_capi.ptr(wd), F, rows, cols, prec, transposed, _capi.ptr(pack), _capi.stream_of(dev)), "ggcn_weight_pack")
            bits = _bits(pkg, dev)
            assert bits == expected, "w[%d,%d] = %r: bits %d, expected %d" % (k, f, value, bits, expected)
            assert _bits(pkg, dev) == 0


# ---------------------------------------------------------------- 6. collection and the lazy half
@pytest.mark.parametrize("s", CASES)
def test_check_range_raises_once_and_every_forward_polls_once(pkg, dev, monkeypatch, s):
    """With the real ``range_guard``: every forward that ran f16mx8 kernels calls ``range_guard.after`` exactly once (the block paths:
    once per call of ``gated_gcn_block``; "two_fused" is two layer forwards, each of which polls), and after a violating launch
    ``check_range()`` raises, a second call does not."""
    from ed_gated_gcn_amd import range_guard
    case = Case(pkg, dev, s)
    calls, real_after = [], range_guard.after

    def after(d):
        calls.append(d)
        return real_after(d)
    monkeypatch.setattr(range_guard, "after", after)
    xd = case.on_device(case.x0)
    case.run(xd)
    assert len(calls) == (2 if s.path == "two_fused" else 1), "%s: range_guard.after ran %d times in one forward" % (s.id, len(calls))
    case.layers[0].check_range()                     # clean data: nothing to report
    g, n, k = case.positions()[-1]
    xd[g, n, k] = POISON * case.scale
    case.run(xd)
    with pytest.raises(RuntimeError, match="f16mx8"):
        case.layers[0].check_range()
    case.layers[0].check_range()                     # reported once, cleared
    assert _bits(pkg, dev) == 0


def test_replay_of_a_captured_forward_reports(pkg, dev, monkeypatch):
    """A forward on clean data captured into a hipGraph (one stream): the capture enqueues no snapshot of the flag
    (``range_guard.after`` returns early under capture); an out-of-window element copied into the static input and a replay later,
    ``check_range()`` raises -- the kernels raise the flag wherever they run."""
    from ed_gated_gcn_amd import range_guard
    s = _spec("block-full-T20", "block", 20, [BLK]).values[0]
    case = Case(pkg, dev, s)
    static_x = case.on_device(case.x0)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(2):             # packs the weights, folds W12, fills the allocator before the capture
            case.run(static_x)
    torch.cuda.current_stream(dev).wait_stream(side)
    case.layers[0].check_range()       # nothing pending when the capture begins
    snapshots, real_snapshot = [], range_guard._snapshot

    def snapshot(st, d):
        snapshots.append(d)
        return real_snapshot(st, d)
    monkeypatch.setattr(range_guard, "_snapshot", snapshot)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = case.run(static_x)
    assert snapshots == [], "the capture enqueued a snapshot of the flag"
    graph.replay()
    torch.cuda.synchronize()
    case.layers[0].check_range()       # clean data
    _in_gate(out, case.ref(case.x0), "replay, clean")
    bad = case.x0.clone()
    bad[s.B - 1, s.T - 1, s.K - 1] = 1000.0
    static_x.copy_(bad.to(dev))
    graph.replay()
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match=r"left \|x\| <= 448"):
        case.layers[0].check_range()
    case.layers[0].check_range()


@pytest.mark.parametrize("T", [20, 33])
def test_bf16x3_and_bfloat16_features_report_nothing(pkg, dev, guard, log, T):
    """The same violating data where no fp16 arithmetic runs: precision bf16x3 (in gate: it has fp32's range) and bfloat16 features
    under the default precision (the bf16 pair form on the bf16x3 image) leave the flag 0."""
    s = _spec("fused-T%d" % T, "fused", T, [L]).values[0]
    case = Case(pkg, dev, s, precision="bf16x3")
    bad = case.x0.clone()
    bad[s.B - 1, T - 1, s.K - 1] = POISON
    bad[0, 0, 0] = -1000.0
    got = case.run(case.on_device(bad))
    assert [c[0] for c in log] == [L] and log[0][1][-2] == 0          # GGCN_PREC_BF16X3
    assert _bits(pkg, dev) == 0
    _in_gate(got, case.ref(bad), "bf16x3")
    case16 = Case(pkg, dev, s)
    del log[:]
    got = case16.run(case16.on_device(bad).to(torch.bfloat16))
    assert log and log[0][0] in ("ggcn_layer_fused_bf16", "ggcn_layer_fused_bf16_wide", "ggcn_linear_bf16"), log[0][0]
    assert _bits(pkg, dev) == 0
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    assert guard == [], "range_guard.after ran for bfloat16 features or bf16x3"
