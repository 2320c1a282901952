"""Host side of the one-launch backward for real-valued adjacencies of 33..128 nodes (``ggcn_graph_operands_weighted_wide_t`` +
``ggcn_gate_pool_backward_weighted_wide``, include/ggcn.h; opt-in ``GraphConvolution.weighted_wide_backward``), on a machine
without a GPU:

* the option and its environment switch; header, ``_capi`` and library agree on the three entries and on ABI 14; the kernel's
  prototype is ``ggcn_gate_pool_backward_weighted``'s; ``_bytes``;
* every refusal of the builder and the kernel, exact texts (each check comes before a launch: the pointers handed in are never
  dereferenced);
* ``dispatch.takes_weighted_wide_backward`` on stand-in graphs that log what they are asked, and ``dispatch.backward_launch``
  against ``backward_plan`` on the grid of ``test_wide_backward_cpu._grid`` with the options off and on;
* the numpy statement of the operand (``weighted_wide_backward_ref.operand_np``): layout, split3, zero padding, summary word,
  reconstruction bound;
* the numpy emulation of the kernel's arithmetic against the float64 statement on every C-ABI case of
  ``tests/test_gpu_weighted_wide_backward.py``: inside a quarter of the dH / d_sg / d_bsum bounds, inside the d_ga / d_gb / dY
  bounds, and inside half of the 2e-6 max|ref| gate for dH and dY.  Measured here: dH 0.123, d_sg 0.009, d_bsum 0.011, d_ga
  0.273, d_gb 0.260, dY 0.125 of their bounds at the worst element; dH 0.301 (dense softmax rows) and dY 0.025 of the gate;
* the tie condition (``br.MAX_MASKED``) of the autograd inputs of the GPU file, on the float64 reference alone.
"""
import ctypes
import itertools
import types

import numpy as np
import pytest
import torch

import ed_gated_gcn_amd as pkg
import weighted_wide_backward_ref as ww
from ed_gated_gcn_amd import _capi, dispatch
from ed_gated_gcn_amd.gcn import GraphConvolution
from oracle import backward_ref as br
from oracle.host_support import header as _header, msg as _msg
from test_wide_backward_cpu import _grid, _operands

EINVAL, EUNSUPPORTED = 1, 3
P = ctypes.c_void_p(1 << 20)   # non-null, 16-byte aligned, never dereferenced
ODD = ctypes.c_void_p((1 << 20) + 4)
H = 64
SIZE, BUILD, KERNEL = ("ggcn_graph_operands_weighted_wide_t_bytes", "ggcn_graph_operands_weighted_wide_t",
                       "ggcn_gate_pool_backward_weighted_wide")
DROP = (0.25, 7, (0, 1, 2))
ENV = "GGCN_WEIGHTED_WIDE_BACKWARD"


@pytest.fixture(autouse=True)
def _no_env(monkeypatch):
    for k in (ENV, "GGCN_WIDE_BACKWARD", "GGCN_WEIGHTED_BACKWARD", "GGCN_BACKWARD_TWO_PASS", "GGCN_BACKWARD_SCALAR", "GGCN_DX_PRECISION"):
        monkeypatch.delenv(k, raising=False)


# ---------------------------------------------------------------- the option and the surface
def _layer(on=True, precision="f16mx8", **more):
    opt = types.SimpleNamespace(ggcn_precision=precision, **more)
    if on is not None:
        opt.ggcn_weighted_wide_backward = on
    return GraphConvolution(H, H, opt=opt)


def test_option_is_off_by_default(monkeypatch):
    assert GraphConvolution(H, H).weighted_wide_backward is False and _layer(None).weighted_wide_backward is False
    assert _layer(True).weighted_wide_backward is True and _layer(False).weighted_wide_backward is False
    # separate from the options beside it
    assert _layer(True).weighted_backward is False and _layer(True).wide_backward is False
    assert _layer(None, ggcn_weighted_backward=True, ggcn_wide_backward=True).weighted_wide_backward is False
    monkeypatch.setenv(ENV, "1")
    assert GraphConvolution(H, H).weighted_wide_backward is True
    monkeypatch.setenv(ENV, "0")
    assert GraphConvolution(H, H).weighted_wide_backward is False


def test_declared_bound_exported_and_abi_stays_14():
    lib = ctypes.CDLL(pkg.lib_path())
    header = _header()
    for name in (SIZE, BUILD, KERNEL):
        assert name + "(" in header and name in _capi.PROTOTYPES and hasattr(lib, name), name
    assert "#define GGCN_ABI_VERSION 14" in header and _capi.ABI_VERSION == 14 and pkg.load_library().ggcn_abi_version() == 14
    proto = lambda n: _capi.PROTOTYPES[n]     # noqa: E731
    assert proto(KERNEL) == proto("ggcn_gate_pool_backward_weighted")
    assert proto(BUILD) == proto("ggcn_graph_operands_weighted_wide") and proto(SIZE) == proto("ggcn_graph_operands_weighted_wide_bytes")
    assert not any(n.startswith(KERNEL + "_") for n in _capi.PROTOTYPES)            # no form under gate dropout
    assert "weighted_wide" in dispatch.BACKWARD_LAUNCHES and "weighted_wide" not in dispatch.BACKWARD_PASSES
    from ed_gated_gcn_amd import gcn
    assert set(gcn._BACKWARD_LAUNCHES) == set(dispatch.BACKWARD_LAUNCHES)
    row = gcn._BACKWARD_LAUNCHES["weighted_wide"]
    assert row[0] == KERNEL and row[2:] == ("both", ())
    assert "_graph_ops_wwt" in pkg.BatchedCSR.__slots__


def test_bytes():
    lib = pkg.load_library()
    for T, W in ((33, 2), (64, 2), (65, 3), (96, 3), (97, 4), (128, 4)):
        for Bn in (1, 3, 512):
            assert lib.ggcn_graph_operands_weighted_wide_t_bytes(Bn, T) == Bn * W * W * 6144 + 4 * Bn == ww.operand_bytes(Bn, T)
    assert {T: lib.ggcn_graph_operands_weighted_wide_t_bytes(1, T) - 4 for T in (64, 96, 128)} == {64: 24 << 10, 96: 54 << 10, 128: 96 << 10}
    for Bn, T in ((0, 64), (-1, 64), (4, 32), (4, 1), (4, 129)):
        assert lib.ggcn_graph_operands_weighted_wide_t_bytes(Bn, T) == 0


def test_builder_refusals():
    lib = pkg.load_library()

    def build(rowptr=P, colidx=P, vals=P, B=4, T=100, ops=P, flag=P):
        return lib.ggcn_graph_operands_weighted_wide_t(rowptr, colidx, vals, B, T, ops, flag, None)
    for kw in (dict(rowptr=None), dict(colidx=None), dict(ops=None)):
        assert _msg(lib, build(**kw), EINVAL) == BUILD + ": null pointer", kw
    assert _msg(lib, build(B=0), EINVAL) == BUILD + ": B=0 T=100 must be positive"
    assert _msg(lib, build(T=-1), EINVAL) == BUILD + ": B=4 T=-1 must be positive"
    for T in (1, 32):
        assert _msg(lib, build(T=T), EUNSUPPORTED) == BUILD + ": T=%d <= 32; use ggcn_graph_operands_weighted_t" % T
    for T in (129, 256):
        assert _msg(lib, build(T=T), EUNSUPPORTED) == BUILD + ": T=%d > 128 (four blocks per row of blocks)" % T
    assert _msg(lib, build(ops=ODD), EINVAL) == BUILD + ": the blocks must be 16-byte aligned"
    assert _msg(lib, build(B=(1 << 31) // 100 + 1), EUNSUPPORTED) == BUILD + ": B*T does not fit int32 node ids"


def test_kernel_refusals():
    lib, who = pkg.load_library(), KERNEL

    def run(out=P, ldo=H, d_out=P, ldd=H, ops=P, inv=P, B=4, T=100, F=H, dh=P, ldh=H, dy=P, ldy=H):
        return getattr(lib, who)(out, ldo, P, P, P, d_out, ldd, P, P, ops, inv, B, T, F, dh, ldh, dy, ldy, P, P, P, P, None)
    for kw in (dict(out=None), dict(dh=None), dict(ops=None), dict(inv=None)):
        assert _msg(lib, run(**kw), EINVAL) == who + ": null pointer", kw
    assert _msg(lib, run(B=0), EINVAL) == who + ": B=0 T=100 F=64 must be positive"
    assert _msg(lib, run(T=0), EINVAL) == who + ": B=4 T=0 F=64 must be positive"
    assert _msg(lib, run(F=-4), EINVAL) == who + ": B=4 T=100 F=-4 must be positive"
    for T in (1, 32):
        assert _msg(lib, run(T=T), EUNSUPPORTED) == who + ": T=%d <= 32; use ggcn_gate_pool_backward_weighted" % T
    for T in (129, 231):
        assert _msg(lib, run(T=T), EUNSUPPORTED) == who + ": T=%d > 128; use ggcn_gate_pool_backward + ggcn_aggregate_t" % T
    for kw in (dict(ldo=H - 4), dict(ldh=H - 4), dict(ldd=H - 4), dict(ldy=H - 4)):
        assert _msg(lib, run(**kw), EINVAL) == who + ": leading dimension smaller than F=64", kw
    # an absent d_out / dY takes ldd / ldy out of the checks: the call is refused by a later one
    assert _msg(lib, run(d_out=None, ldd=0, dh=ODD), EUNSUPPORTED).startswith(who + ": needs F % 4 == 0")
    assert _msg(lib, run(dy=None, ldy=0, dh=ODD), EUNSUPPORTED).startswith(who + ": needs F % 4 == 0")
    big = (1 << 31) // (4 * 128)                        # T = 100 is four blocks = 128 rows: 128 * ld * 4 >= 2 GiB
    for kw in (dict(ldo=big), dict(ldh=big), dict(ldd=big), dict(ldy=big), dict(ldo=(1 << 31) // 400 + 1)):
        assert _msg(lib, run(**kw), EUNSUPPORTED) == who + ": a graph's rows exceed 2 GiB", kw
    assert _msg(lib, run(dy=None, ldy=big, dh=ODD), EUNSUPPORTED).startswith(who + ": needs F % 4 == 0")
    align = who + ": needs F % 4 == 0, ldh % 4 == 0 and 16-byte aligned dH / graph_ops_wwt; use ggcn_gate_pool_backward + ggcn_aggregate_t"
    for kw in (dict(F=30, ldo=30, ldd=30, ldh=32, ldy=30), dict(ldh=H + 2), dict(dh=ODD), dict(ops=ODD)):
        assert _msg(lib, run(**kw), EUNSUPPORTED) == align, kw


def test_kernel_refusals_are_the_0_1_entry_s_word_for_word():
    """The refusals the two 33..128-node backward entries share are two copies of one text (each unit checks at the head of its
    own launcher): the same arguments draw the same code and the same words from both, the entry's name apart."""
    lib, other = pkg.load_library(), "ggcn_gate_pool_backward_wide"
    big = (1 << 31) // (4 * 128)
    for kw in (dict(out=None), dict(dh=None), dict(ops=None), dict(inv=None), dict(B=0), dict(T=0), dict(F=-4), dict(T=129), dict(T=231),
               dict(ldo=H - 4), dict(ldh=H - 4), dict(ldd=H - 4), dict(ldo=big), dict(ldh=big), dict(ldd=big)):
        a = dict(out=P, ldo=H, d_out=P, ldd=H, ops=P, inv=P, B=4, T=100, F=H, dh=P, ldh=H)
        a.update(kw)
        head = (a["out"], a["ldo"], P, P, P, a["d_out"], a["ldd"], P, P, a["ops"], a["inv"], a["B"], a["T"], a["F"], a["dh"], a["ldh"])
        texts = []
        for who, mid in ((KERNEL, (P, H)), (other, ())):
            rc = getattr(lib, who)(*head, *mid, P, P, P, P, None)
            assert rc in (EINVAL, EUNSUPPORTED)
            texts.append((rc, _msg(lib, rc, rc).replace(who, "<entry>")))
        assert texts[0] == texts[1], kw


# ---------------------------------------------------------------- the predicate
def _graph(T=100, binary=False, operand=True, B=4):
    """A stand-in for a BatchedCSR that logs every attribute the predicate reads."""
    asked = []

    class Graph:
        def __getattr__(self, name):
            asked.append(name)
            values = {"T": T, "B": B, "is_binary": binary,
                      "graph_ops_weighted_wide_t": lambda: types.SimpleNamespace(is_cuda=True) if operand else None}
            if name not in values:
                raise AttributeError(name)
            return values[name]
    g = Graph()
    g.__dict__["asked"] = asked
    return g


def _takes(layer=None, csr=None, F=H, dropout=None, operands=None):
    return dispatch.takes_weighted_wide_backward(layer or _layer(), csr, F, dropout, operands or _operands())


def test_option_off_asks_nothing():
    for layer in (_layer(False), _layer(None), types.SimpleNamespace(precision="f16mx8"),      # (the third: a layer that predates the option)
                  types.SimpleNamespace(precision="f16mx8", weighted_backward=True, wide_backward=True)):
        g = _graph()
        log = []
        ops = (types.SimpleNamespace(data_ptr=lambda: (log.append("ptr"), 1 << 20)[1]),)
        assert dispatch.takes_weighted_wide_backward(layer, g, H, None, ops) is False
        assert g.asked == [] and log == []


def test_predicate_holds_and_each_condition_alone_turns_it_off(monkeypatch):
    name = "graph_ops_weighted_wide_t"
    for T in (33, 64, 65, 100, 128):
        g = _graph(T)
        assert _takes(csr=g) is True
        assert g.asked.count(name) == 1 and g.asked[-1] == name, g.asked      # asked once, last
    cases = {
        "a 0/1 adjacency": dict(csr=_graph(binary=True)),
        "T = 32": dict(csr=_graph(32)),
        "T = 1": dict(csr=_graph(1)),
        "T = 129": dict(csr=_graph(129)),
        "F = 30": dict(F=30),
        "a 4-byte aligned operand": dict(operands=_operands(4)),
        "gate dropout": dict(dropout=DROP),
    }
    for what, kw in cases.items():
        g = kw.pop("csr", None) or _graph()
        assert _takes(csr=g, **kw) is False, what
        assert name not in g.asked, "%s: the graph was asked for its operand" % what
    g = _graph(operand=False)                                        # a non-finite entry: asked, and the answer is None
    assert _takes(csr=g) is False and g.asked[-1] == name and g.asked.count(name) == 1
    monkeypatch.setenv("GGCN_BACKWARD_TWO_PASS", "1")
    g = _graph()
    assert _takes(csr=g) is False and name not in g.asked
    monkeypatch.setenv("GGCN_BACKWARD_TWO_PASS", "0")
    assert _takes(csr=_graph()) is True


# ---------------------------------------------------------------- backward_launch against backward_plan
def _plan_graph(T, binary, masks, new=True):
    on_gpu = types.SimpleNamespace(is_cuda=True)
    g = types.SimpleNamespace(T=T, B=4, is_binary=binary, rowmask=on_gpu if masks else None, graph_ops=on_gpu, graph_ops_t=on_gpu,
                              graph_ops_weighted_t=lambda: None, rowmask_t_wide=on_gpu if (binary and masks and 32 < T <= 128) else None)
    if new:      # (without: a stand-in of the existing tests, which has no such attribute)
        g.graph_ops_weighted_wide_t = lambda: on_gpu if (not binary and 32 < T <= 128) else None
    return g


def test_backward_launch_is_backward_plan_with_every_option_off(monkeypatch):
    n = 0
    for T, binary, masks, F, dropout, need_adj, offset, two_pass, dtype, precision in _grid():
        monkeypatch.setenv("GGCN_BACKWARD_TWO_PASS", "1" if two_pass else "0")
        for layer in (_layer(False, precision), _layer(None, precision)):
            g = _plan_graph(T, binary, masks, new=False)
            args = (True, need_adj, dropout, _operands(offset))
            assert dispatch.backward_launch(layer, g, dtype, 4, H, F, *args) == dispatch.backward_plan(layer, g, dtype, H, F, *args)
            n += 1
    assert n == 2 * 8 * 2 * 2 * 3 * 2 * 2 * 2 * 2 * 2 * 2


@pytest.mark.parametrize("wide_too", [False, True], ids=["alone", "with-wide_backward"])
def test_backward_launch_with_the_option_on_differs_only_where_the_rule_says(monkeypatch, wide_too):
    seen = set()
    for T, binary, masks, F, dropout, need_adj, offset, two_pass, dtype, precision in _grid():
        monkeypatch.setenv("GGCN_BACKWARD_TWO_PASS", "1" if two_pass else "0")
        layer, g = _layer(True, precision, ggcn_wide_backward=wide_too), _plan_graph(T, binary, masks)
        assert layer.wide_backward is wide_too
        args = (True, need_adj, dropout, _operands(offset))
        plan = dispatch.backward_plan(layer, g, dtype, H, F, *args)
        got = dispatch.backward_launch(layer, g, dtype, 4, H, F, *args)
        common = 32 < T <= 128 and F % 4 == 0 and not offset and not two_pass and dropout is None
        rule = common and not binary                                             # (with and without an adjacency gradient)
        wide_rule = wide_too and common and binary and masks and not need_adj
        what = (T, binary, masks, F, dropout, need_adj, offset, two_pass, dtype, precision)
        assert got[1:] == plan[1:], what
        if rule:
            assert plan[0] == "two_pass" and got[0] == "weighted_wide", what
        elif wide_rule:
            assert plan[0] == "two_pass" and got[0] == "wide", what
        else:
            assert got[0] == plan[0] and got[0] in dispatch.BACKWARD_PASSES, what
        seen.add(got[0])
    assert seen == set(dispatch.BACKWARD_PASSES) | {"weighted_wide"} | ({"wide"} if wide_too else set())


# ---------------------------------------------------------------- the numpy statement of the operand
@pytest.mark.parametrize("T", ww.BUILDER_T)
def test_operand_statement(T):
    W = (T + 31) // 32
    for graph in ww.BUILDER_GRAPHS:
        adj = ww.adjacency(T, graph, 400 + T).numpy()
        blocks, summary = ww.operand_np(adj)
        assert blocks.dtype == np.uint8 and blocks.shape == (ww.B, W * W * 6144) and summary.dtype == np.uint32 and summary.shape == (ww.B,)
        assert ww.operand_buffer_np(adj).size == ww.operand_bytes(ww.B, T)
        planes = ww.planes_from_blocks(blocks, T)                              # the layout, read back by its own description
        n = np.zeros((ww.B, 32 * W, 32 * W), dtype=np.float32)
        n[:, :T, :T] = adj.transpose(0, 2, 1)
        for p, want in enumerate(ww.split3_np(n)):
            assert np.array_equal(planes[p], want), (graph, p)
        assert not planes[:, :, T:, :].any() and not planes[:, :, :, T:].any()        # rows and columns >= T: zero
        assert not ((planes.view(np.uint32)) & 0xFFFF).any()                           # every plane is a bfloat16
        total = planes.astype(np.float64).sum(0)
        assert (np.abs(total - n) <= 2.0 ** -25 * np.abs(n)).all(), graph              # |p0 + p1 + p2 - A| <= 2^-25 |A|
        for b, s, t in itertools.product(range(ww.B), range(W), range(W)):
            assert (int(summary[b]) >> (4 * s + t)) & 1 == int(n[b, 32 * s:32 * s + 32, 32 * t:32 * t + 32].any()), (graph, b, s, t)
        assert not (summary >> np.uint32(16)).any()
        if graph in ww.STRUCTURES:
            full = sum(1 << (4 * s + t) for s in range(W) for t in range(W))
            assert any(0 < int(w) < full for w in summary), "%s: no graph with empty and non-empty blocks" % graph
    # one entry, by hand: A[t=40, s=3] = 1 + 2^-9 + 2^-18 sits in block (0, 1), row 3, column 8 -> k-step 0, lane 3, element 4
    a = np.zeros((1, T, T), dtype=np.float32)
    a[0, 40 % T, 3] = 1.0 + 2.0 ** -9 + 2.0 ** -18
    if T > 40:
        blocks, summary = ww.operand_np(a)
        v = blocks.view(np.uint16).reshape(W, W, 3, 2, 64, 8)
        assert [int(v[0, 1, p, 0, 3, 4]) for p in range(3)] == [0x3F80, 0x3B00, 0x3680] and int(summary[0]) == 1 << 1
        assert int((v != 0).sum()) == 3


# ---------------------------------------------------------------- the emulation of the kernel
def _ratios(c):
    ref = ww.statement(c)
    em, bd = ww.emulate(c), ww.bounds(c, ref)
    out = {}
    for k, bound in bd.items():
        if bound is None or (k == "d_sg" and c["sg"] is None):
            continue
        err = (torch.from_numpy(em[k]).double() - ref[k]).abs()
        assert bool((err <= bound).all()), (k, float((err / (bound + 1e-300)).max()))
        out[k] = float((err / (bound + 1e-300)).max())
    for k in ("dH", "dY"):
        err = float((torch.from_numpy(em[k]).double() - ref[k]).abs().max())
        out[k + " gate"] = err / (ww.GATE * float(ref[k].abs().max()) + 1e-300)
    return out


SPARE = {"dH": 0.25, "d_sg": 0.25, "d_bsum": 0.25, "d_ga": 1.0, "d_gb": 1.0, "dY": 1.0, "dH gate": 0.5, "dY gate": 0.5}


@pytest.mark.parametrize("T", ww.KERNEL_T)
def test_emulation_inside_the_bounds_with_a_factor_to_spare(T):
    for case in [k for k in ww.KERNEL_CASES if k[0] == T]:
        c = ww.kernel_inputs(*case)
        assert float((c["adj"].double().sum(2) + 1.0).abs().min()) >= ww.MIN_DENOMINATOR
        r = _ratios(c)
        print(case, {k: "%.3f" % v for k, v in r.items()})
        assert "dH" in r and "d_bsum" in r
        for k, v in r.items():
            assert v <= SPARE[k], (case, k, v)


def test_the_bound_notices_a_lost_plane_of_the_adjacency():
    """Two bf16 planes of A_w instead of three (2^-17 of a term) is outside the dH bound: the bound is no blanket."""
    c = ww.kernel_inputs(100, 36)
    ref = ww.statement(c)
    bound = ww.bounds(c, ref)["dH"]
    p0, p1, _ = ww.split3_np(c["adj"].numpy())
    two = torch.from_numpy(p0.astype(np.float64) + p1.astype(np.float64))
    dh2 = torch.einsum("bts,btf->bsf", two, c["inv"].double()[:, :, None] * ref["dY"])
    assert bool(((dh2 - ref["dH"]).abs() > bound).any())


# ---------------------------------------------------------------- the tie condition of the autograd inputs of the GPU file
@pytest.mark.parametrize("dense", [False, True], ids=["sparse", "softmax"])
@pytest.mark.parametrize("name", sorted(ww.AUTOGRAD))
def test_tie_condition_of_the_autograd_cases(name, dense):
    for bf16 in (False, True):
        c = ww.autograd_inputs(name, bf16, dense)
        ma, mb = br.layer_tie_masks(c["x"], c["adj"], c["w"], c["b"], c["ga"], c["gb"], br.tie_delta("f16mx8"))
        share = br.masked_share(ma, mb)
        print("%s %s%s: %.2f %% of the pools masked" % (name, "softmax" if dense else "sparse", " bf16" if bf16 else "", 100 * share))
        assert share <= br.MAX_MASKED
