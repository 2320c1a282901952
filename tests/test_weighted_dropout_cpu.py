"""Host side of gate dropout inside the launches on a real-valued adjacency (``ggcn_layer_fused_weighted_drop``,
``ggcn_layer_fused_weighted_wide_drop``, ``ggcn_gate_pool_backward_weighted_drop``; include/ggcn.h): the three entries on all three
sides of the ABI, every refusal (each check comes before a launch: the pointers handed in are never dereferenced, so no GPU is
needed), the opt-in ``GraphConvolution.weighted_dropout`` and the two predicates ``dispatch.takes_weighted_dropout`` /
``dispatch.takes_weighted_backward_drop`` on stand-ins for graphs and tensors -- and that everything the dispatch table pins
answers as before with the option on."""
import ctypes
import os
import types

import pytest
import torch

import ed_gated_gcn_amd as pkg
from ed_gated_gcn_amd import _capi, dispatch
from ed_gated_gcn_amd.gcn import GraphConvolution
from oracle.host_support import msg as _msg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = 1, 3
P = ctypes.c_void_p(1 << 20)   # non-null, 16-byte aligned, never dereferenced
H = 64
FWD, WIDE, BWD = "ggcn_layer_fused_weighted_drop", "ggcn_layer_fused_weighted_wide_drop", "ggcn_gate_pool_backward_weighted_drop"
BF16X3, F16MX8, F16MX6 = 0, 2, 4
DROP = (0.25, 7, 0, 1, 2)
ENV = ("GGCN_WEIGHTED_DROPOUT", "GGCN_WEIGHTED_BACKWARD", "GGCN_WEIGHTED_MAX_T", "GGCN_BACKWARD_TWO_PASS", "GGCN_FUSED",
       "GGCN_FUSED_MAX_T", "GGCN_PRECISION")


@pytest.fixture(autouse=True)
def _no_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


# ---------------------------------------------------------------- the ABI
def test_declared_bound_exported_and_abi_stays_14():
    lib = ctypes.CDLL(pkg.lib_path())
    header = open(os.path.join(ROOT, "include", "ggcn.h")).read()
    for name in (FWD, WIDE, BWD):
        assert name + "(" in header and name in _capi.PROTOTYPES and hasattr(lib, name), name
    assert "#define GGCN_ABI_VERSION 14" in header and _capi.ABI_VERSION == 14 and pkg.load_library().ggcn_abi_version() == 14
    proto = {k: v[1] for k, v in _capi.PROTOTYPES.items()}
    tail = [ctypes.c_float, ctypes.c_uint64, _capi.c_i32, _capi.c_i32, _capi.c_i32, _capi.c_vp]   # p, seed, three streams, stream
    # the entries without dropout, minus the overlap arguments (<= 32 nodes), with ggcn_layer_fused_drop's tail
    assert proto["ggcn_layer_fused_drop"][-6:] == tail
    w = proto["ggcn_layer_fused_weighted"]
    assert proto[FWD] == w[:17] + w[20:21] + tail
    assert proto[WIDE] == proto["ggcn_layer_fused_weighted_wide"][:-1] + tail
    assert proto[BWD] == proto["ggcn_gate_pool_backward_weighted"][:-1] + tail


# ---------------------------------------------------------------- refusals, all before a launch
def _fwd(lib, ops=P, zero=P, B=4, T=24, K=H, F=H, prec=F16MX8, drop=DROP):
    return lib.ggcn_layer_fused_weighted_drop(P, K, P, ops, P, zero, B, T, K, F, P, P, P, P, F, P, P, prec, *drop, None)


def _wide(lib, ops=P, B=4, T=100, K=H, F=H, prec=F16MX8, drop=DROP):
    return lib.ggcn_layer_fused_weighted_wide_drop(P, K, P, ops, P, B, T, K, F, P, P, P, P, F, P, P, prec, *drop, None)


def _bwd(lib, B=4, T=24, F=H, drop=DROP, **kw):
    a = dict(out=P, ops=P, inv=P, dh=P)
    a.update(kw)
    return lib.ggcn_gate_pool_backward_weighted_drop(a["out"], F, P, P, P, P, F, P, P, a["ops"], a["inv"], B, T, F, a["dh"], F, P, F,
                                                     P, P, P, P, *drop, None)


BAD_DROPS = [(1.0, 7, 0, 1, 2), (-0.1, 7, 0, 1, 2), (float("nan"), 7, 0, 1, 2), (0.25, 7, 3, 1, 2), (0.25, 7, 0, -1, 2), (0.25, 7, 0, 1, 3)]


def test_forward_refusals_up_to_32_nodes():
    lib = pkg.load_library()
    assert "T=33" in _msg(lib, _fwd(lib, T=33), EUNSUPPORTED)
    _msg(lib, _fwd(lib, prec=F16MX6), EUNSUPPORTED)
    assert "32 bits" in _msg(lib, _fwd(lib, B=1 << 19, T=32, F=256), EUNSUPPORTED)          # B*T*F = 2^32
    assert "32 bits" in _msg(lib, _fwd(lib, B=1 << 19, T=32, F=256, drop=(0.0, 7, 0, 0, 0)), EUNSUPPORTED)
    assert "blocks" in _msg(lib, _fwd(lib, ops=None), EINVAL)
    assert "zero row" in _msg(lib, _fwd(lib, zero=None), EINVAL)
    for drop in BAD_DROPS:
        assert "streams" in _msg(lib, _fwd(lib, drop=drop), EINVAL), drop


def test_forward_refusals_33_to_128_nodes():
    lib = pkg.load_library()
    for T in (32, 129):
        assert "T=%d" % T in _msg(lib, _wide(lib, T=T), EUNSUPPORTED)
    _msg(lib, _wide(lib, prec=F16MX6), EUNSUPPORTED)
    assert "32 bits" in _msg(lib, _wide(lib, B=1 << 17, T=128, F=256), EUNSUPPORTED)        # B*T*F = 2^32
    assert "blocks" in _msg(lib, _wide(lib, ops=None), EINVAL)
    for drop in BAD_DROPS:
        assert "streams" in _msg(lib, _wide(lib, drop=drop), EINVAL), drop
    # the entry without dropout takes the same shape as far as its launch (and still names itself)
    assert "ggcn_layer_fused_weighted_wide:" in _msg(lib, lib.ggcn_layer_fused_weighted_wide(P, H, P, None, P, 4, 100, H, H, P, P, P, P, H, P, P,
                                                                                            F16MX8, None), EINVAL)


def test_backward_refusals():
    lib = pkg.load_library()
    assert "32 bits" in _msg(lib, _bwd(lib, B=1 << 19, T=32, F=256), EUNSUPPORTED)          # B*T*F = 2^32
    msg = _msg(lib, _bwd(lib, T=33), EUNSUPPORTED)                                          # the entry's own refusals, under its name
    assert BWD in msg and "ggcn_aggregate_t" in msg
    assert "16-byte" in _msg(lib, _bwd(lib, F=30), EUNSUPPORTED)
    for k, word in (("out", "out"), ("dh", "dH"), ("inv", "inv"), ("ops", "graph_ops_wt")):
        assert word in _msg(lib, _bwd(lib, **{k: None}), EINVAL)
    for drop in BAD_DROPS:
        assert "streams" in _msg(lib, _bwd(lib, drop=drop), EINVAL), drop
    assert _bwd(lib, B=0) == 0                                                              # nothing to do: no launch


# ---------------------------------------------------------------- the option
def _layer(dropout=True, backward=True, max_t=None, precision="f16mx8"):
    opt = types.SimpleNamespace(ggcn_precision=precision)
    if dropout is not None:
        opt.ggcn_weighted_dropout = dropout
    if backward is not None:
        opt.ggcn_weighted_backward = backward
    if max_t is not None:
        opt.ggcn_weighted_max_t = max_t
    return GraphConvolution(H, H, opt=opt)


def test_option_is_off_by_default(monkeypatch):
    assert GraphConvolution(H, H).weighted_dropout is False and _layer(None).weighted_dropout is False
    assert _layer(True).weighted_dropout is True and _layer(False).weighted_dropout is False
    monkeypatch.setenv("GGCN_WEIGHTED_DROPOUT", "1")
    assert GraphConvolution(H, H).weighted_dropout is True
    monkeypatch.setenv("GGCN_WEIGHTED_DROPOUT", "0")
    assert GraphConvolution(H, H).weighted_dropout is False


# ---------------------------------------------------------------- the forward predicate
def _graph(T=24, binary=False, ops=True):
    asked = []
    blk = types.SimpleNamespace(is_cuda=True)
    g = types.SimpleNamespace(T=T, B=4, is_binary=binary, asked=asked, rowmask=None)
    g.graph_ops_weighted = lambda plane: (asked.append("w%d" % plane), blk if ops else None)[1]
    g.graph_ops_weighted_wide = lambda: (asked.append("ww"), blk if ops else None)[1]
    g.graph_ops_weighted_t = lambda: (asked.append("wt"), blk if ops else None)[1]
    return g


def _inp(B=4, T=24, dtype=torch.float32, gpu="cuda:0"):
    return dispatch.Input(dtype, B, T, gpu)


def test_forward_predicate_holds_and_each_condition_alone_turns_it_off():
    g = _graph()
    assert dispatch.takes_weighted_dropout(_layer(), g, _inp()) is True and g.asked == ["w1"]
    g = _graph()
    assert dispatch.takes_weighted_dropout(_layer(precision="bf16x3"), g, _inp()) is True and g.asked == ["w0"]
    g = _graph(100)
    assert dispatch.takes_weighted_dropout(_layer(max_t=128), g, _inp(T=100)) is True and g.asked == ["ww"]
    cases = {
        "option off": (dict(layer=_layer(False)), False),
        "index past 32 bits": (dict(inp=_inp(B=1 << 22, T=24)), False),               # 2^22 * 24 * 64 >= 2^32
        "binary adjacency": (dict(csr=_graph(binary=True)), False),
        "bfloat16 features": (dict(inp=_inp(dtype=torch.bfloat16)), False),
        "not on a GPU": (dict(inp=_inp(gpu=None)), False),
        "precision fp32": (dict(layer=_layer(precision="fp32")), False),
        "T = 33 with weighted_max_t = 32": (dict(csr=_graph(33), inp=_inp(T=33)), False),
        "T = 129 with weighted_max_t = 128": (dict(layer=_layer(max_t=128), csr=_graph(129), inp=_inp(T=129)), False),
        "no operand block": (dict(csr=_graph(ops=False)), True),
    }
    for what, (kw, asks) in cases.items():
        a = dict(layer=_layer(), csr=_graph(), inp=_inp())
        a.update(kw)
        assert dispatch.takes_weighted_dropout(a["layer"], a["csr"], a["inp"]) is False, what
        assert bool(a["csr"].asked) == asks, "%s: the graph's builders were asked %s" % (what, a["csr"].asked)
    fused_off = _layer()
    fused_off.fused = False
    g = _graph()
    assert dispatch.takes_weighted_dropout(fused_off, g, _inp()) is False and g.asked == []


def test_a_layer_that_predates_the_option_is_off():
    old = _layer()
    del old.weighted_dropout
    g = _graph()
    assert dispatch.takes_weighted_dropout(old, g, _inp()) is False and g.asked == []


def test_public_predicate_is_the_dispatch_one():
    m, g = _layer(), _graph()
    text = types.SimpleNamespace(dtype=torch.float32, shape=(4, 24, H), is_cuda=True, device="cuda:0")
    assert m.takes_weighted_dropout_path(text, g) is True and g.asked == ["w1"]
    m.weighted_dropout = False
    g = _graph()
    assert m.takes_weighted_dropout_path(text, g) is False and g.asked == []


# ---------------------------------------------------------------- the backward predicate
def _operands(offset=0):
    t = types.SimpleNamespace(data_ptr=lambda: (1 << 20) + offset)
    return (types.SimpleNamespace(data_ptr=lambda: 1 << 20), None, t, None)


DROPOUT = (0.25, 7, (0, 1, 2))


def test_backward_predicate_holds_and_each_condition_alone_turns_it_off(monkeypatch):
    g = _graph()
    assert dispatch.takes_weighted_backward_drop(_layer(), g, 4, H, DROPOUT, _operands()) is True and g.asked == ["wt"]
    for T in (1, 5, 31, 32):
        assert dispatch.takes_weighted_backward_drop(_layer(), _graph(T), 4, 4, DROPOUT, _operands()) is True
    # the forward option is not this predicate's business: the two-call forward of another build of the layer ends here too
    assert dispatch.takes_weighted_backward_drop(_layer(dropout=False), _graph(), 4, H, DROPOUT, _operands()) is True
    cases = {
        "weighted_backward off": dict(layer=_layer(backward=False)),
        "no dropout": dict(dropout=None),
        "index past 32 bits": dict(B=1 << 22),
        "binary adjacency": dict(csr=_graph(binary=True)),
        "T = 33": dict(csr=_graph(33)),
        "F = 30": dict(F=30),
        "a 4-byte aligned operand": dict(operands=_operands(4)),
        "no operand block": dict(csr=_graph(ops=False)),
    }
    for what, kw in cases.items():
        a = dict(layer=_layer(), csr=_graph(), B=4, F=H, dropout=DROPOUT, operands=_operands())
        a.update(kw)
        assert dispatch.takes_weighted_backward_drop(a["layer"], a["csr"], a["B"], a["F"], a["dropout"], a["operands"]) is False, what
        if what != "no operand block":
            assert a["csr"].asked == [], "%s: the graph was asked for its operand" % what      # asked last: nothing is built
    monkeypatch.setenv("GGCN_BACKWARD_TWO_PASS", "1")
    g = _graph()
    assert dispatch.takes_weighted_backward_drop(_layer(), g, 4, H, DROPOUT, _operands()) is False and g.asked == []


# ---------------------------------------------------------------- what is pinned stays
def test_the_pinned_answers_stay_with_the_option_on():
    assert dispatch.LAYER_PATHS == ("fused", "fused_drop", "bf16", "bf16_drop", "bf16_wide", "bf16_wide_drop", "weighted", "long", "two_launch")
    assert dispatch.DROPOUT_PATHS == ("fused_drop", "bf16_drop", "bf16_wide_drop")
    assert dispatch.BACKWARD_PASSES == ("mma", "one_pass", "two_pass", "two_pass_drop")
    m = _layer()
    text = types.SimpleNamespace(dtype=torch.float32, shape=(4, 24, H), is_cuda=True, device="cuda:0")
    g = _graph()
    assert dispatch.layer_path(m, text, g, dropout=False) == "weighted"
    g = _graph()
    assert dispatch.layer_path(m, text, g, dropout=True) == "two_launch" and g.asked == []     # layer_path has no name for the new launches
    g = _graph()
    assert dispatch.takes_weighted_backward(m, g, H, DROPOUT, _operands()) is False and g.asked == []
    assert dispatch.takes_weighted_backward(m, _graph(), H, None, _operands()) is True
    g = _graph()
    assert dispatch.backward_plan(m, g, torch.float32, H, H, True, False, DROPOUT, _operands()) == ("two_pass_drop", "bf16x3", "bf16x3")
    assert dispatch.backward_plan(m, g, torch.float32, H, H, True, False, None, _operands()) == ("two_pass", "bf16x3", "bf16x3")
    assert g.asked == []
