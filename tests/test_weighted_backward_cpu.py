"""Host side of the one-launch backward for a real-valued adjacency of graphs of <= 32 nodes (``ggcn_graph_operands_weighted_t`` +
``ggcn_gate_pool_backward_weighted``, include/ggcn.h): the three entries on all three sides of the ABI, the size of the operand
blocks, every refusal (each check comes before a launch: the pointers handed in are never dereferenced, so no GPU is needed),
the opt-in ``GraphConvolution.weighted_backward`` and ``dispatch.takes_weighted_backward`` on stand-ins for graphs and tensors."""
import ctypes
import os
import types

import pytest

import ed_gated_gcn_amd as pkg
from ed_gated_gcn_amd import _capi, dispatch
from ed_gated_gcn_amd.gcn import GraphConvolution
from oracle.host_support import msg as _msg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = 1, 3
P = ctypes.c_void_p(1 << 20)   # non-null, 16-byte aligned, never dereferenced
ODD = ctypes.c_void_p((1 << 20) + 4)
H = 64
NAMES = ("ggcn_graph_operands_weighted_t_bytes", "ggcn_graph_operands_weighted_t", "ggcn_gate_pool_backward_weighted")


@pytest.fixture(autouse=True)
def _no_env(monkeypatch):
    monkeypatch.delenv("GGCN_WEIGHTED_BACKWARD", raising=False)
    monkeypatch.delenv("GGCN_BACKWARD_TWO_PASS", raising=False)


def test_declared_bound_exported_and_abi_stays_14():
    lib = ctypes.CDLL(pkg.lib_path())
    header = open(os.path.join(ROOT, "include", "ggcn.h")).read()
    for name in NAMES:
        assert name + "(" in header and name in _capi.PROTOTYPES and hasattr(lib, name), name
    assert "#define GGCN_ABI_VERSION 14" in header and _capi.ABI_VERSION == 14 and pkg.load_library().ggcn_abi_version() == 14
    assert "#define GGCN_GRAPH_OPSWT_BYTES 6144" in header
    # the argument list of ggcn_gate_pool_backward_mma with (graph_ops_wt, inv) for its two operand blocks, (dY, ldy) after
    # (dH, ldh) and without max |dH|
    mma, w = _capi.PROTOTYPES["ggcn_gate_pool_backward_mma"][1], _capi.PROTOTYPES["ggcn_gate_pool_backward_weighted"][1]
    assert w == mma[:16] + [_capi.c_vp, _capi.c_i64] + mma[16:20] + mma[21:]


def test_bytes():
    """One block per graph: 3 planes x 2 k-steps x 64 lanes x 16 bytes."""
    lib = pkg.load_library()
    assert 3 * 2 * 64 * 16 == 6144
    for B in (1, 3, 7, 4096):
        assert lib.ggcn_graph_operands_weighted_t_bytes(B) == 6144 * B
    for B in (0, -1, -4096):
        assert lib.ggcn_graph_operands_weighted_t_bytes(B) == 0


def test_builder_refusals():
    lib = pkg.load_library()

    def build(rp=P, ci=P, va=P, B=4, T=24, ops=P, flag=None):
        return lib.ggcn_graph_operands_weighted_t(rp, ci, va, B, T, ops, flag, None)
    for T in (33, 100):
        assert "T=%d" % T in _msg(lib, build(T=T), EUNSUPPORTED)
    assert "rowptr" in _msg(lib, build(rp=None), EINVAL)
    assert "colidx" in _msg(lib, build(ci=None), EINVAL)
    assert "graph_ops_wt" in _msg(lib, build(ops=None), EINVAL)
    for T in (0, -3):
        assert "T=%d" % T in _msg(lib, build(T=T), EINVAL)
    assert "B=-1" in _msg(lib, build(B=-1), EINVAL)
    msg = _msg(lib, build(ops=ODD), EINVAL)
    assert "graph_ops_wt" in msg and "aligned" in msg
    assert build(B=0) == 0                                       # nothing to do: no launch (there is no GPU to refuse one here)
    assert build(B=0, va=None) == 0


def test_kernel_refusals():
    lib = pkg.load_library()

    def run(out=P, ldo=H, d_out=P, ldd=H, ops=P, inv=P, B=4, T=24, F=H, dh=P, ldh=H, dy=P, ldy=H):
        return lib.ggcn_gate_pool_backward_weighted(out, ldo, P, P, P, d_out, ldd, P, P, ops, inv, B, T, F, dh, ldh, dy, ldy,
                                                    P, P, P, P, None)
    msg = _msg(lib, run(T=33), EUNSUPPORTED)
    assert "ggcn_gate_pool_backward" in msg and "ggcn_aggregate_t" in msg
    for kw in (dict(F=30, ldo=30, ldd=30, ldh=30, ldy=30), dict(ldh=H + 2), dict(ldo=H + 1), dict(ldd=H + 3), dict(ldy=H + 2),
               dict(dh=ODD), dict(dy=ODD), dict(ops=ODD)):
        msg = _msg(lib, run(**kw), EUNSUPPORTED)
        assert "16-byte" in msg and "ggcn_aggregate_t" in msg, kw
    assert "out" in _msg(lib, run(out=None), EINVAL)
    assert "dH" in _msg(lib, run(dh=None), EINVAL)
    assert "inv" in _msg(lib, run(inv=None), EINVAL)
    assert "graph_ops_wt" in _msg(lib, run(ops=None), EINVAL)
    for kw in (dict(ldo=H - 4), dict(ldh=H - 4), dict(ldd=H - 4), dict(ldy=H - 4)):
        assert "leading dimension" in _msg(lib, run(**kw), EINVAL), kw
    for kw in (dict(T=0), dict(F=0), dict(B=-1)):
        _msg(lib, run(**kw), EINVAL)
    assert run(B=0) == 0                                         # no launch
    # optional operands: an absent d_out / dY takes its leading dimension out of the checks
    assert run(B=0, d_out=None, ldd=0) == 0 and run(B=0, dy=None, ldy=0) == 0


# ---------------------------------------------------------------- the option and the predicate
def _layer(on=True):
    opt = types.SimpleNamespace(ggcn_precision="f16mx8")
    if on is not None:
        opt.ggcn_weighted_backward = on
    return GraphConvolution(H, H, opt=opt)


def _graph(T=24, binary=False, ops=True):
    asked = []
    g = types.SimpleNamespace(T=T, B=4, is_binary=binary, asked=asked)
    g.graph_ops_weighted_t = lambda: (asked.append(1), types.SimpleNamespace(is_cuda=True) if ops else None)[1]
    return g


def _operands(offset=0):
    t = types.SimpleNamespace(data_ptr=lambda: (1 << 20) + offset)
    return (types.SimpleNamespace(data_ptr=lambda: 1 << 20), None, t, None)


def test_option_is_off_by_default(monkeypatch):
    assert GraphConvolution(H, H).weighted_backward is False and _layer(None).weighted_backward is False
    assert _layer(True).weighted_backward is True
    monkeypatch.setenv("GGCN_WEIGHTED_BACKWARD", "1")
    assert GraphConvolution(H, H).weighted_backward is True
    monkeypatch.setenv("GGCN_WEIGHTED_BACKWARD", "0")
    assert GraphConvolution(H, H).weighted_backward is False


def test_predicate_holds_and_each_condition_alone_turns_it_off(monkeypatch):
    g = _graph()
    assert dispatch.takes_weighted_backward(_layer(), g, H, None, _operands()) is True and g.asked == [1]
    for T in (1, 5, 31, 32):
        assert dispatch.takes_weighted_backward(_layer(), _graph(T), 4, None, _operands()) is True
    cases = {
        "option off": dict(layer=_layer(False)),
        "binary adjacency": dict(csr=_graph(binary=True)),
        "T = 33": dict(csr=_graph(33)),
        "F = 30": dict(F=30),
        "dropout": dict(dropout=(0.25, 7, (0, 1, 2))),
        "a 4-byte aligned operand": dict(operands=_operands(4)),
        "no operand block": dict(csr=_graph(ops=False)),
    }
    for what, kw in cases.items():
        a = dict(layer=_layer(), csr=_graph(), F=H, dropout=None, operands=_operands())
        a.update(kw)
        assert dispatch.takes_weighted_backward(a["layer"], a["csr"], a["F"], a["dropout"], a["operands"]) is False, what
        if what != "no operand block":
            assert a["csr"].asked == [], "%s: the graph was asked for its operand" % what      # asked last: nothing is built
    monkeypatch.setenv("GGCN_BACKWARD_TWO_PASS", "1")
    g = _graph()
    assert dispatch.takes_weighted_backward(_layer(), g, H, None, _operands()) is False and g.asked == []
    monkeypatch.setenv("GGCN_BACKWARD_TWO_PASS", "0")
    assert dispatch.takes_weighted_backward(_layer(), _graph(), H, None, _operands()) is True


def test_a_layer_that_predates_the_option_is_off():
    old = _layer()
    del old.weighted_backward
    g = _graph()
    assert dispatch.takes_weighted_backward(old, g, H, None, _operands()) is False and g.asked == []


def test_the_plan_and_its_names_stay():
    """The new launch is decided AFTER backward_plan, which still says "two_pass" for a real-valued adjacency."""
    assert dispatch.BACKWARD_PASSES == ("mma", "one_pass", "two_pass", "two_pass_drop")
    import torch
    g = _graph()
    g.rowmask = None
    assert dispatch.backward_plan(_layer(), g, torch.float32, H, H, True, False, None, _operands()) == ("two_pass", "bf16x3", "bf16x3")
    assert g.asked == []
