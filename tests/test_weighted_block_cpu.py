"""Host side of the one-launch inference block on a real-valued adjacency (``ggcn_graph_operands2_weighted``,
``ggcn_block_fused_weighted``; include/ggcn.h): the two entries on all three sides of the ABI, every refusal (each check comes
before a launch: the pointers handed in are never dereferenced, so no GPU is needed), the opt-in
``GraphConvolution.weighted_block``, ``dispatch.takes_weighted_block_path`` on stand-ins for graphs and tensors, and
``dispatch.block_launch``, which answers as ``dispatch.block_path`` on the whole grid of ``tests/golden/dispatch_table.json``."""
import ctypes
import importlib.util
import itertools
import os
import types

import pytest
import torch

import ed_gated_gcn_amd as pkg
from ed_gated_gcn_amd import _capi, dispatch, gated_block
from ed_gated_gcn_amd.gcn import GraphConvolution
from oracle.host_support import msg as _msg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = 1, 3
P = ctypes.c_void_p(1 << 20)   # non-null, 16-byte aligned, never dereferenced
ODD = ctypes.c_void_p((1 << 20) + 4)
H = 64
BUILDER, BLOCK = "ggcn_graph_operands2_weighted", "ggcn_block_fused_weighted"
BF16X3, F16MX8, F16MX6 = 0, 2, 4
ENV = ("GGCN_WEIGHTED_BLOCK", "GGCN_WEIGHTED_MAX_T", "GGCN_FUSED", "GGCN_FUSED_MAX_T", "GGCN_PRECISION", "GGCN_BF16_BLOCK")


@pytest.fixture(autouse=True)
def _no_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


# ---------------------------------------------------------------- the ABI
def test_declared_bound_exported_and_abi_stays_14():
    lib = ctypes.CDLL(pkg.lib_path())
    header = open(os.path.join(ROOT, "include", "ggcn.h")).read()
    for name in (BUILDER, BLOCK):
        assert "int %s(" % name in header and name in _capi.PROTOTYPES and hasattr(lib, name), name
    assert "#define GGCN_ABI_VERSION 14" in header and _capi.ABI_VERSION == 14 and pkg.load_library().ggcn_abi_version() == 14
    proto = {k: v[1] for k, v in _capi.PROTOTYPES.items()}
    assert proto[BUILDER] == proto["ggcn_graph_operands_weighted"]
    b = proto["ggcn_block_fused"]
    assert proto[BLOCK] == b[:9] + [_capi.c_vp] + b[9:]          # ggcn_block_fused's list with zero_mid after bias2


# ---------------------------------------------------------------- refusals, all before a launch
def _builder(lib, rowptr=P, colidx=P, ops=P, B=4, T=24, plane=1):
    return lib.ggcn_graph_operands2_weighted(rowptr, colidx, P, B, T, plane, ops, None, None)


def _block(lib, **kw):
    a = dict(x=P, w1=P, w12=P, opsw=P, ops2w=P, mid=P, zero=P, B=4, T=24, K=H, F=H, gate1=P, gate2=P, gcn1=None, ld1=H, xo=P, ld2=H,
             x1=P, y1=P, out=P, part=P, prec=F16MX8)
    a.update(kw)
    return lib.ggcn_block_fused_weighted(a["x"], a["K"], a["w1"], a["w12"], a["opsw"], a["ops2w"], P, a["mid"], P, a["zero"], a["B"],
                                         a["T"], a["K"], a["F"], a["gate1"], a["gate2"], a["gcn1"], a["ld1"], a["xo"], a["ld2"],
                                         a["x1"], a["y1"], a["out"], a["part"], a["prec"], None)


def test_builder_refusals():
    lib = pkg.load_library()
    for kw in (dict(rowptr=None), dict(colidx=None), dict(ops=None)):
        assert "null" in _msg(lib, _builder(lib, **kw), EINVAL, BUILDER)
    assert "T=33" in _msg(lib, _builder(lib, T=33), EUNSUPPORTED, BUILDER)
    _msg(lib, _builder(lib, T=0), EINVAL, BUILDER)
    _msg(lib, _builder(lib, B=0), EINVAL, BUILDER)
    for plane in (2, -1):
        assert "plane" in _msg(lib, _builder(lib, plane=plane), EINVAL, BUILDER)
    assert "aligned" in _msg(lib, _builder(lib, ops=ODD), EINVAL, BUILDER)


def test_block_refusals():
    lib = pkg.load_library()
    assert "graph_ops2w" in _msg(lib, _block(lib, ops2w=None), EINVAL, BLOCK)            # null blocks
    assert "graph_opsw" in _msg(lib, _block(lib, opsw=None), EINVAL, BLOCK)
    assert "graph_ops2w" in _msg(lib, _block(lib, ops2w=ODD), EINVAL, BLOCK)             # misaligned blocks
    assert "graph_opsw" in _msg(lib, _block(lib, opsw=ODD), EINVAL, BLOCK)
    assert "T=33" in _msg(lib, _block(lib, T=33), EUNSUPPORTED, BLOCK)
    _msg(lib, _block(lib, prec=F16MX6), EUNSUPPORTED, BLOCK)
    _msg(lib, _block(lib, prec=1), EUNSUPPORTED, BLOCK)                                  # fp32: no one-launch form
    assert "zero_mid" in _msg(lib, _block(lib, zero=None), EINVAL, BLOCK)
    assert "zero_mid" in _msg(lib, _block(lib, zero=ODD), EINVAL, BLOCK)
    for kw in (dict(x1=None), dict(y1=None), dict(gate1=None), dict(x1=None, y1=None), dict(x1=None, y1=None, part=None, gcn1=P)):
        assert "go together" in _msg(lib, _block(lib, **kw), EINVAL, BLOCK), kw          # layer 1's outputs given only in part
    assert "gate2" in _msg(lib, _block(lib, gate2=None), EINVAL, BLOCK)
    assert "bias_mid" in _msg(lib, _block(lib, mid=None), EINVAL, BLOCK)
    _msg(lib, _block(lib, xo=None, out=None), EINVAL, BLOCK)
    _msg(lib, _block(lib, x=None), EINVAL, BLOCK)
    _msg(lib, _block(lib, w12=None), EINVAL, BLOCK)
    _msg(lib, _block(lib, w1=None), EINVAL, BLOCK)
    _msg(lib, _block(lib, B=0), EINVAL, BLOCK)
    _msg(lib, _block(lib, T=0), EINVAL, BLOCK)
    _msg(lib, _block(lib, ld2=H - 4), EINVAL, BLOCK)                                     # leading dimension below F
    _msg(lib, _block(lib, ld2=1 << 31), EUNSUPPORTED, BLOCK)
    # the eval form takes no graph_opsw, wpack1, gate1 or zero_mid, and is refused for what it does need
    eval_form = dict(x1=None, y1=None, part=None, gcn1=None, opsw=None, w1=None, gate1=None, zero=None)
    assert "graph_ops2w" in _msg(lib, _block(lib, ops2w=None, **eval_form), EINVAL, BLOCK)
    assert "T=33" in _msg(lib, _block(lib, T=33, **eval_form), EUNSUPPORTED, BLOCK)


# ---------------------------------------------------------------- the option
def _layer(block=True, precision="f16mx8", fout=H):
    opt = types.SimpleNamespace(ggcn_precision=precision)
    if block is not None:
        opt.ggcn_weighted_block = block
    return GraphConvolution(H, fout, opt=opt)


def test_option_is_off_by_default(monkeypatch):
    assert GraphConvolution(H, H).weighted_block is False and _layer(None).weighted_block is False
    assert _layer(True).weighted_block is True and _layer(False).weighted_block is False
    monkeypatch.setenv("GGCN_WEIGHTED_BLOCK", "1")
    assert GraphConvolution(H, H).weighted_block is True
    monkeypatch.setenv("GGCN_WEIGHTED_BLOCK", "0")
    assert GraphConvolution(H, H).weighted_block is False


# ---------------------------------------------------------------- the predicate
def _graph(T=24, binary=False, ops=True, ops2=True):
    asked = []
    blk = types.SimpleNamespace(is_cuda=True)
    g = types.SimpleNamespace(T=T, B=4, is_binary=binary, asked=asked, rowmask=None)
    g.graph_ops_weighted = lambda plane: (asked.append("w%d" % plane), blk if ops else None)[1]
    g.graph_ops2_weighted = lambda plane: (asked.append("w2_%d" % plane), blk if ops2 else None)[1]
    g.graph_ops_weighted_wide = lambda: (asked.append("ww"), None)[1]
    return g


def _text(T=24, dtype=torch.float32, gpu=True):
    return types.SimpleNamespace(dtype=dtype, shape=(4, T, H), is_cuda=gpu, device="cuda:0" if gpu else "cpu")


def test_predicate_holds_and_each_condition_alone_turns_it_off():
    g = _graph()
    assert dispatch.takes_weighted_block_path(_text(), g, _layer(), _layer()) is True and g.asked == ["w1", "w1", "w2_1"]   # M2 asked last
    g = _graph()
    assert dispatch.takes_weighted_block_path(_text(), g, _layer(precision="bf16x3"), _layer(precision="bf16x3")) is True
    assert g.asked == ["w0", "w0", "w2_0"]
    for T in (1, 17, 32):
        assert dispatch.takes_weighted_block_path(_text(T), _graph(T), _layer(), _layer()) is True
    fused_off = _layer()
    fused_off.fused = False
    cases = {
        "CPU tensors": (dict(x=_text(gpu=False)), []),
        "the option off": (dict(gc1=_layer(False)), []),
        "a binary CSR": (dict(csr=_graph(binary=True)), []),
        "bfloat16 x": (dict(x=_text(dtype=torch.bfloat16)), []),
        "float16 x": (dict(x=_text(dtype=torch.float16)), []),
        "T = 33": (dict(x=_text(33), csr=_graph(33)), []),
        "unequal precisions": (dict(gc2=_layer(precision="bf16x3")), []),
        "f16mx6": (dict(gc1=_layer(precision="f16mx6"), gc2=_layer(precision="f16mx6")), []),
        "fp32": (dict(gc1=_layer(precision="fp32"), gc2=_layer(precision="fp32")), []),
        "non-square widths": (dict(gc2=_layer(fout=2 * H)), []),
        "gc2 without fused": (dict(gc2=fused_off), []),
        "no M operand": (dict(csr=_graph(ops=False)), ["w1"]),
        "no M2 operand": (dict(csr=_graph(ops2=False)), ["w1", "w1", "w2_1"]),
    }
    for what, (kw, asked) in cases.items():
        a = dict(x=_text(), csr=_graph(), gc1=_layer(), gc2=_layer())
        a.update(kw)
        assert dispatch.takes_weighted_block_path(a["x"], a["csr"], a["gc1"], a["gc2"]) is False, what
        assert a["csr"].asked == asked, "%s: the graph's builders were asked %s" % (what, a["csr"].asked)
    assert dispatch.takes_weighted_block_path(torch.zeros(4, 24, H), _graph(), _layer(), _layer()) is False      # a real CPU tensor


def test_option_off_never_asks_for_the_operand():
    def boom(plane):
        raise AssertionError("graph_ops2_weighted was called with the option off")
    g = _graph()
    g.graph_ops2_weighted = boom
    off = _layer(False)
    assert dispatch.takes_weighted_block_path(_text(), g, off, _layer()) is False
    for want, gcn1, one, training in itertools.product((gated_block.BLOCK_OUTPUTS, ("out",)), (False, True), (False, True), (False, True)):
        assert dispatch.block_launch(_text(), g, off, _layer(), want, gcn1, one, training) in ("layers", "layers_eval")
    old = _layer()
    del old.weighted_block                      # a layer that predates the option
    assert dispatch.takes_weighted_block_path(_text(), g, old, _layer()) is False


def test_public_predicate_is_the_dispatch_one():
    assert gated_block.takes_weighted_block_path is dispatch.takes_weighted_block_path
    assert pkg.gated_block.takes_weighted_block_path is dispatch.takes_weighted_block_path


# ---------------------------------------------------------------- block_launch
def test_block_launches_are_the_paths_plus_one():
    assert dispatch.BLOCK_PATHS == ("block", "bf16_block", "folded_eval", "bf16_folded_eval", "two_fused", "layers_eval", "layers")
    assert dispatch.BLOCK_LAUNCHES == dispatch.BLOCK_PATHS + ("weighted_block",)


def test_block_launch_replaces_layers_only_in_inference_with_one_launch():
    everything = gated_block.BLOCK_OUTPUTS
    on = dict(x=_text(), gc1=_layer(), gc2=_layer())
    for want, path in ((everything, "layers"), (("out",), "layers_eval"), (("x", "out"), "layers_eval"), (("xy", "out"), "layers")):
        for gcn1 in (False, True):
            g = _graph()
            assert dispatch.block_path(on["x"], g, on["gc1"], on["gc2"], want, gcn1, True, False) == path
            assert dispatch.block_launch(on["x"], g, on["gc1"], on["gc2"], want, gcn1, True, False) == "weighted_block"
            g = _graph()
            assert dispatch.block_launch(on["x"], g, on["gc1"], on["gc2"], want, gcn1, False, False) == path      # one_launch=False
            assert "w2_1" not in g.asked
    g = _graph()
    assert dispatch.block_launch(on["x"], g, on["gc1"], on["gc2"], everything, False, True, True) == "layers"      # under autograd
    assert "w2_1" not in g.asked
    g = _graph(ops2=False)
    assert dispatch.block_launch(on["x"], g, on["gc1"], on["gc2"], everything, False, True, False) == "layers"     # the builder refused


def test_block_launch_is_block_path_on_the_whole_pinned_grid():
    spec = importlib.util.spec_from_file_location("dispatch_table_tool_wb", os.path.join(ROOT, "tools", "dispatch_table.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    everything = ("x1", "y1", "xy", "x", "out")
    flags = [f + (False,) for f in itertools.product((everything, ("out",), ("xy", "out")), (False, True), (False, True))]
    flags += [(everything, g, o, True) for g, o in itertools.product((False, True), (False, True))]
    n, seen = 0, set()
    with tool.pretend_device():
        for label, x, csr, gc1, gc2 in tool.block_cases():
            assert gc1.weighted_block is False
            for want, want_gcn1, one_launch, training in flags:
                path = dispatch.block_path(x, csr, gc1, gc2, want, want_gcn1, one_launch, training)
                assert dispatch.block_launch(x, csr, gc1, gc2, want, want_gcn1, one_launch, training) == path, (label, want, want_gcn1, one_launch, training)
                seen.add(path)
            n += 1
    assert n == 25920 and seen == set(dispatch.BLOCK_PATHS)
