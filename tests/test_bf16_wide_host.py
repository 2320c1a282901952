"""CPU checks of the bfloat16 one-launch entries for graphs of 33..256 nodes and for gate dropout (include/ggcn.h "bfloat16
features": ggcn_layer_fused_bf16_drop, ggcn_layer_fused_bf16_wide): declared, bound and exported with the ABI still 14 (functions
were added, nothing changed), every refusal returning its code and a message that names the argument BEFORE any launch (the
pointers handed in are never dereferenced), and the new predicates of GraphConvolution saying no to CPU and float32 text."""
import ctypes
import re
import types

import torch

import ed_gated_gcn_amd as pkg
from ed_gated_gcn_amd import _capi
from ed_gated_gcn_amd.gcn import GraphConvolution
from oracle.host_support import header as _header, msg as _msg

EINVAL, EUNSUPPORTED = 1, 3
NEW = ("ggcn_layer_fused_bf16_drop", "ggcn_layer_fused_bf16_wide")
P = ctypes.c_void_p(1 << 20)   # a non-null, 16-byte aligned address: never dereferenced (the checks come first)
ODD = ctypes.c_void_p((1 << 20) + 1)
OFF8 = ctypes.c_void_p((1 << 20) + 8)


def test_new_symbols_declared_bound_and_exported():
    src = _header()
    lib = ctypes.CDLL(pkg.lib_path())
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _capi.PROTOTYPES, name
        assert hasattr(lib, name), name


def test_abi_version_stays_14_on_all_three_sides():
    m = re.search(r"#define\s+GGCN_ABI_VERSION\s+(\d+)", _header())
    assert int(m.group(1)) == 14
    assert _capi.ABI_VERSION == 14
    assert pkg.load_library().ggcn_abi_version() == 14


def _drop(lib, x=P, ldx=64, wpack=P, ops=P, out=P, ldo=64, B=4, T=31, F=64, ov_in=None, ov_out=None, p=0.25, streams=(0, 1, 2)):
    return lib.ggcn_layer_fused_bf16_drop(x, ldx, wpack, ops, None, B, T, 64, F, None, None, None, out, ldo, None, None, None,
                                          ov_in, ov_out, p, 7, *streams, None)


def _wide(lib, x=P, ldx=64, wpack=P, masks=P, lists=None, out=P, ldo=64, B=4, T=100, F=64, ov_in=None, ov_out=None, p=0.0,
          streams=(0, 0, 0)):
    return lib.ggcn_layer_fused_bf16_wide(x, ldx, wpack, masks, lists, None, B, T, 64, F, None, None, None, out, ldo, None, None,
                                          None, ov_in, ov_out, p, 7, *streams, None)


def test_layer_fused_bf16_drop_refuses_bad_arguments():
    lib = pkg.load_library()
    assert "null input" in _msg(lib, _drop(lib, x=None), EINVAL)
    assert "weight image" in _msg(lib, _drop(lib, wpack=None), EINVAL)
    assert "operand blocks" in _msg(lib, _drop(lib, ops=None), EINVAL)
    assert "ldx < K" in _msg(lib, _drop(lib, ldx=63), EINVAL)
    assert "leading dimension of the output" in _msg(lib, _drop(lib, ldo=63), EINVAL)
    assert "X not 2-byte aligned" in _msg(lib, _drop(lib, x=ODD), EINVAL)
    assert "wpack must be 16-byte aligned" in _msg(lib, _drop(lib, wpack=OFF8), EINVAL)
    assert "graph_ops must be 16-byte aligned" in _msg(lib, _drop(lib, ops=OFF8), EINVAL)
    assert "overlap_in and overlap_out" in _msg(lib, _drop(lib, ov_in=P), EINVAL)
    assert "overlap_in and overlap_out" in _msg(lib, _drop(lib, ov_out=P), EINVAL)
    assert "p=1" in _msg(lib, _drop(lib, p=1.0), EINVAL)
    assert "streams" in _msg(lib, _drop(lib, streams=(0, 3, 1)), EINVAL)
    m = _msg(lib, _drop(lib, T=33), EUNSUPPORTED)
    assert "T=33" in m and "ggcn_layer_fused_bf16_wide" in m
    # B*T*F = 2^32 exactly: the 32-bit element index of the keep factors does not cover it
    m = _msg(lib, _drop(lib, B=1 << 15, T=32, F=4096, ldo=4096), EUNSUPPORTED)
    assert "B*T*F" in m


def test_layer_fused_bf16_wide_refuses_bad_arguments():
    lib = pkg.load_library()
    assert "null input" in _msg(lib, _wide(lib, x=None), EINVAL)
    assert "weight image" in _msg(lib, _wide(lib, wpack=None), EINVAL)
    assert "row masks" in _msg(lib, _wide(lib, masks=None), EINVAL)
    assert "ldx < K" in _msg(lib, _wide(lib, ldx=63), EINVAL)
    assert "leading dimension of the output" in _msg(lib, _wide(lib, ldo=63), EINVAL)
    assert "X not 2-byte aligned" in _msg(lib, _wide(lib, x=ODD), EINVAL)
    assert "wpack must be 16-byte aligned" in _msg(lib, _wide(lib, wpack=OFF8), EINVAL)
    assert "edge-list blocks must be 16-byte aligned" in _msg(lib, _wide(lib, T=200, lists=OFF8), EINVAL)
    assert "overlap_in and overlap_out" in _msg(lib, _wide(lib, ov_in=P), EINVAL)
    assert "overlap_in and overlap_out" in _msg(lib, _wide(lib, ov_out=P), EINVAL)
    assert "streams" in _msg(lib, _wide(lib, p=0.5, streams=(1, 2, 5)), EINVAL)
    m = _msg(lib, _wide(lib, T=32), EUNSUPPORTED)
    assert "T=32" in m and "ggcn_layer_fused_bf16" in m
    m = _msg(lib, _wide(lib, T=257), EUNSUPPORTED)
    assert "T=257" in m and "ggcn_linear_bf16" in m and "ggcn_aggregate" in m
    # dropout only: B*T*F = 2^32 is refused
    m = _msg(lib, _wide(lib, B=1 << 14, T=64, F=4096, ldo=4096, p=0.25, streams=(0, 1, 2)), EUNSUPPORTED)
    assert "B*T*F" in m


def test_layer_fused_bf16_keeps_its_range():
    """The <= 32-node entry still refuses longer graphs (GGCN_EUNSUPPORTED) and now names the entry that takes them."""
    lib = pkg.load_library()
    rc = lib.ggcn_layer_fused_bf16(P, 64, P, P, None, 4, 33, 64, 64, None, None, None, P, 64, None, None, None, None, None, None)
    m = _msg(lib, rc, EUNSUPPORTED)
    assert "T=33" in m and "ggcn_layer_fused_bf16_wide" in m


def test_new_predicates_say_no_to_cpu_and_float32_text():
    m = GraphConvolution(16, 16)
    assert m.precision in ("bf16x3", "f16mx8", "f16mx6") and m.fused
    for T in (8, 100):
        csr = types.SimpleNamespace(T=T, B=2, is_binary=True, rowmask=torch.zeros(2 * T, (T + 31) // 32, dtype=torch.int32))
        for x in (torch.zeros(2, T, 16, dtype=torch.bfloat16), torch.zeros(2, T, 16, dtype=torch.float32)):
            assert m.takes_bf16_wide_path(x, csr) is False      # CPU row masks / float32 text
            assert m.takes_bf16_dropout_path(x, csr) is False
