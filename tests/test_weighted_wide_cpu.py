"""Host side of the one-launch layer for a real-valued adjacency of graphs of 33..128 nodes (``ggcn_layer_fused_weighted_wide``,
include/ggcn.h): the opt-in ``GraphConvolution.weighted_max_t`` (``opt.ggcn_weighted_max_t`` / ``GGCN_WEIGHTED_MAX_T``, 32 by
default) in ``dispatch.takes_weighted`` / ``layer_path`` on stand-ins for tensors and graphs like ``tools/dispatch_table.py``'s,
the size of the operand blocks, and the refusals of the two new entries (every check comes before a launch: the pointers handed
in are never dereferenced)."""
import ctypes
import importlib.util
import os
import types

import pytest
import torch

import ed_gated_gcn_amd as pkg
from ed_gated_gcn_amd import _capi, dispatch
from ed_gated_gcn_amd.gcn import GraphConvolution
from oracle.host_support import msg as _msg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("dispatch_table_tool", os.path.join(ROOT, "tools", "dispatch_table.py"))
dt = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dt)

EINVAL, EUNSUPPORTED = 1, 3
P = ctypes.c_void_p(1 << 20)   # non-null, 16-byte aligned, never dereferenced
ODD = ctypes.c_void_p((1 << 20) + 4)
H = 64


def _graph(T, ops=True, method=True, B=4):
    """A weighted graph as the predicates see it; ``method=False``: a stand-in that predates ``graph_ops_weighted_wide``."""
    g = dt.graph(B, T, False, True, True)
    if method:
        asked = []
        g.asked = asked
        g.graph_ops_weighted_wide = lambda: (asked.append(1), types.SimpleNamespace(is_cuda=True) if ops else None)[1]
    return g


def _layer(max_t=None, precision="f16mx8", fused=True):
    opt = types.SimpleNamespace(ggcn_precision=precision, ggcn_fused=fused)
    if max_t is not None:
        opt.ggcn_weighted_max_t = max_t
    return GraphConvolution(H, H, opt=opt)


@pytest.fixture(autouse=True)
def _no_env(monkeypatch):
    monkeypatch.delenv("GGCN_WEIGHTED_MAX_T", raising=False)


@pytest.mark.parametrize("T", [33, 64, 128])
def test_off_by_default_and_on_with_the_option(T):
    x = dt.features(4, T, H, torch.float32)
    off, on = _layer(), _layer(128)
    assert off.weighted_max_t == 32 and on.weighted_max_t == 128
    g = _graph(T)
    assert dispatch.takes_weighted(off, g, dispatch.Input.of(x)) is False and g.asked == []      # the option first: never asked
    assert dispatch.layer_path(off, x, g) == "two_launch"
    assert dispatch.takes_weighted(on, g, dispatch.Input.of(x)) is True and on.takes_weighted_path(x, g)
    assert dispatch.layer_path(on, x, g) == "weighted"
    assert dispatch.layer_path(on, x, g, dropout=True) == "two_launch"                           # no dropout epilogue in this launch
    for precision in ("bf16x3", "f16mx6"):
        assert dispatch.layer_path(_layer(128, precision), x, g) == "weighted"


def test_where_the_option_does_not_reach():
    on = _layer(128)
    x = dt.features(4, 129, H, torch.float32)
    assert not dispatch.takes_weighted(on, _graph(129), dispatch.Input.of(x))
    assert not dispatch.takes_weighted(_layer(1000), _graph(129), dispatch.Input.of(x))          # larger values mean 128
    x = dt.features(4, 64, H, torch.float32)
    assert not dispatch.takes_weighted(_layer(63), _graph(64), dispatch.Input.of(x))
    assert dispatch.takes_weighted(_layer(64), _graph(64), dispatch.Input.of(x))
    for dtype in (torch.float16, torch.bfloat16):
        assert not dispatch.takes_weighted(on, _graph(64), dispatch.Input.of(dt.features(4, 64, H, dtype)))
    assert not dispatch.takes_weighted(_layer(128, "fp32"), _graph(64), dispatch.Input.of(x))
    assert not dispatch.takes_weighted(_layer(128, fused=False), _graph(64), dispatch.Input.of(x))
    assert not dispatch.takes_weighted(on, _graph(64, ops=False), dispatch.Input.of(x))          # the builder's flag came back set
    assert dispatch.layer_path(on, x, _graph(64, ops=False)) == "two_launch"
    assert not dispatch.takes_weighted(on, _graph(64), dispatch.Input.of(torch.empty(4, 64, H)))  # CPU features
    binary = dt.graph(4, 64, True, True, True)
    assert not dispatch.takes_weighted(on, binary, dispatch.Input.of(x)) and dispatch.layer_path(on, x, binary) == "fused"
    # graphs of <= 32 nodes: what it was, whatever the option says
    x32 = dt.features(4, 32, H, torch.float32)
    for layer in (_layer(), on, _layer(16)):
        assert dispatch.takes_weighted(layer, _graph(32), dispatch.Input.of(x32))


@pytest.mark.parametrize("T", [33, 100, 128, 231])
def test_a_graph_without_the_method_is_never_asked_by_default(T):
    x = dt.features(4, T, H, torch.float32)
    g = _graph(T, method=False)
    assert not hasattr(g, "graph_ops_weighted_wide")
    for precision in ("f16mx8", "bf16x3", "fp32"):
        layer = _layer(None, precision)
        assert dispatch.takes_weighted(layer, g, dispatch.Input.of(x)) is False
        assert dispatch.layer_path(layer, x, g) == "two_launch"
    old = _layer()
    del old.weighted_max_t                                      # a layer object that predates the option
    assert dispatch.takes_weighted(old, g, dispatch.Input.of(x)) is False


def test_environment_variable(monkeypatch):
    assert GraphConvolution(H, H).weighted_max_t == 32
    monkeypatch.setenv("GGCN_WEIGHTED_MAX_T", "128")
    assert GraphConvolution(H, H).weighted_max_t == 128
    assert GraphConvolution(H, H, opt=types.SimpleNamespace(ggcn_weighted_max_t=64)).weighted_max_t == 64


@pytest.mark.parametrize("T", [33, 64, 65, 96, 97, 128])
def test_bytes_is_the_documented_layout(T):
    """W x W blocks per graph, W = ceil(T/32); a block = (hi, lo) x 2 k-steps x 64 lanes x 16 bytes."""
    lib = pkg.load_library()
    W = -(-T // 32)
    block = 2 * 2 * 64 * 16
    assert block == 4096
    for B in (1, 7):
        assert lib.ggcn_graph_operands_weighted_wide_bytes(B, T) == B * W * W * block
    assert W == {33: 2, 64: 2, 65: 3, 96: 3, 97: 4, 128: 4}[T]


def test_bytes_outside_the_range():
    lib = pkg.load_library()
    for B, T in ((4, 32), (4, 129), (0, 64), (-1, 64), (4, 0)):
        assert lib.ggcn_graph_operands_weighted_wide_bytes(B, T) == 0


def test_builder_refusals():
    lib = pkg.load_library()

    def build(rp=P, ci=P, va=P, B=4, T=64, ops=P, flag=None):
        return lib.ggcn_graph_operands_weighted_wide(rp, ci, va, B, T, ops, flag, None)
    assert "ggcn_graph_operands_weighted" in _msg(lib, build(T=32), EUNSUPPORTED)     # points at the one-block builder
    assert "<= 32" in _msg(lib, build(T=17), EUNSUPPORTED)
    assert "128" in _msg(lib, build(T=129), EUNSUPPORTED)
    for kw in (dict(rp=None), dict(ci=None), dict(ops=None)):
        assert "null" in _msg(lib, build(**kw), EINVAL)
    _msg(lib, build(B=0), EINVAL)
    _msg(lib, build(T=0), EINVAL)
    assert "aligned" in _msg(lib, build(ops=ODD), EINVAL)


def test_layer_refusals():
    lib = pkg.load_library()

    def layer(x=P, ldx=64, w=P, ops=P, B=4, T=64, K=64, F=64, out=P, ldo=64, pa=P, pb=P, prec=_capi.PREC["f16mx8"]):
        return lib.ggcn_layer_fused_weighted_wide(x, ldx, w, ops, None, B, T, K, F, None, None, None, out, ldo, pa, pb, prec, None)
    for T in (1, 32):
        assert "ggcn_layer_fused_weighted" in _msg(lib, layer(T=T), EUNSUPPORTED)
    assert "128" in _msg(lib, layer(T=129), EUNSUPPORTED)
    for prec in ("fp32", "f16", "f16mx6"):
        assert "precision" in _msg(lib, layer(prec=_capi.PREC[prec]), EUNSUPPORTED)
    assert "ldx" in _msg(lib, layer(ldx=63), EINVAL)
    assert "leading dimension" in _msg(lib, layer(ldo=63), EINVAL)
    assert "wpack" in _msg(lib, layer(w=ODD), EINVAL)
    assert "aligned" in _msg(lib, layer(ops=ODD), EINVAL)
    for kw in (dict(x=None), dict(w=None), dict(ops=None)):
        _msg(lib, layer(**kw), EINVAL)
    assert "no output" in _msg(lib, layer(out=None, pa=None, pb=None), EINVAL)
    _msg(lib, layer(B=0), EINVAL)


def test_declared_bound_exported_and_abi_stays_14():
    lib = ctypes.CDLL(pkg.lib_path())
    header = open(os.path.join(ROOT, "include", "ggcn.h")).read()
    for name in ("ggcn_graph_operands_weighted_wide_bytes", "ggcn_graph_operands_weighted_wide", "ggcn_layer_fused_weighted_wide"):
        assert name + "(" in header and name in _capi.PROTOTYPES and hasattr(lib, name), name
    assert "#define GGCN_ABI_VERSION 14" in header and _capi.ABI_VERSION == 14 and pkg.load_library().ggcn_abi_version() == 14
    # the argument list of ggcn_layer_fused without the row masks and the three regulariser pointers
    full, ww = _capi.PROTOTYPES["ggcn_layer_fused"][1], _capi.PROTOTYPES["ggcn_layer_fused_weighted_wide"][1]
    assert ww == full[:3] + full[4:17] + full[20:]

