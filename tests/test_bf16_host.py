"""CPU checks of the bfloat16-feature entry points (include/ggcn.h "bfloat16 features"): declared, bound and exported,
the ABI version bumped on both sides, every new entry refusing bad arguments with GGCN_EINVAL before any launch, and
the Python layer's dtype contract for bf16 features (no GPU needed: the checks run before anything touches a device)."""
import ctypes
import re

import pytest
import torch

import ed_gated_gcn_amd as pkg
from ed_gated_gcn_amd import _capi
from ed_gated_gcn_amd.gcn import BF16_PRECISIONS, GraphConvolution
from oracle.host_support import header as _header

EINVAL = 1
NEW = ("ggcn_linear_bf16", "ggcn_linear_out_bf16", "ggcn_layer_fused_bf16", "ggcn_dweight_bf16",
       "ggcn_dweight_bf16_workspace_bytes", "ggcn_subword_pool_bf16")
P = ctypes.c_void_p(1 << 20)   # a non-null, 16-byte aligned address: never dereferenced (the checks come first)


def test_new_symbols_declared_bound_and_exported():
    src = _header()
    lib = ctypes.CDLL(pkg.lib_path())
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _capi.PROTOTYPES, name
        assert hasattr(lib, name), name


def test_abi_version_is_14_on_both_sides():
    m = re.search(r"#define\s+GGCN_ABI_VERSION\s+(\d+)", _header())
    assert int(m.group(1)) == _capi.ABI_VERSION == 14
    assert pkg.load_library().ggcn_abi_version() == 14


def _err(lib, rc):
    assert rc == EINVAL, rc
    return lib.ggcn_last_error().decode()


def test_linear_bf16_rejects_bad_arguments():
    lib = pkg.load_library()
    for fn in (lib.ggcn_linear_bf16, lib.ggcn_linear_out_bf16):
        assert "null" in _err(lib, fn(None, 64, P, P, 64, 8, 64, 64, None))
        assert "null" in _err(lib, fn(P, 64, None, P, 64, 8, 64, 64, None))
        assert "null" in _err(lib, fn(P, 64, P, None, 64, 8, 64, 64, None))
        assert "leading" in _err(lib, fn(P, 63, P, P, 64, 8, 64, 64, None))    # ldx < K
        assert "leading" in _err(lib, fn(P, 64, P, P, 63, 8, 64, 64, None))    # ldy < F
    assert "aligned" in _err(lib, lib.ggcn_linear_bf16(ctypes.c_void_p((1 << 20) + 1), 64, P, P, 64, 8, 64, 64, None))
    assert "aligned" in _err(lib, lib.ggcn_linear_out_bf16(ctypes.c_void_p((1 << 20) + 2), 64, P, P, 64, 8, 64, 64, None))


def test_layer_fused_bf16_rejects_bad_arguments():
    lib = pkg.load_library()
    f = lib.ggcn_layer_fused_bf16

    def call(x=P, ldx=64, wpack=P, ops=P, out=P, ldo=64):
        return f(x, ldx, wpack, ops, None, 4, 31, 64, 64, None, None, None, out, ldo, None, None, None, None, None, None)
    assert "null" in _err(lib, call(x=None))
    assert "graph" in _err(lib, call(ops=None))
    assert "ldx < K" in _err(lib, call(ldx=63))
    assert "weight image" in _err(lib, call(wpack=None))
    assert "leading" in _err(lib, call(ldo=63))
    assert "aligned" in _err(lib, call(x=ctypes.c_void_p((1 << 20) + 1)))
    assert "16-byte" in _err(lib, call(wpack=ctypes.c_void_p((1 << 20) + 8)))


def test_dweight_bf16_rejects_bad_arguments():
    lib = pkg.load_library()
    f = lib.ggcn_dweight_bf16
    assert lib.ggcn_dweight_bf16_workspace_bytes(0, 64, 64) == 0
    assert lib.ggcn_dweight_bf16_workspace_bytes(4096, 256, 256) > 0
    assert "null" in _err(lib, f(None, 64, P, 64, 128, 64, 64, P, 64, P, None))
    assert "null" in _err(lib, f(P, 64, P, 64, 128, 64, 64, P, 64, None, None))
    assert "leading" in _err(lib, f(P, 63, P, 64, 128, 64, 64, P, 64, P, None))    # ldx < K
    assert "leading" in _err(lib, f(P, 64, P, 63, 128, 64, 64, P, 64, P, None))    # ldg < F
    assert "aligned" in _err(lib, f(P, 64, P, 64, 128, 64, 64, P, 64, ctypes.c_void_p((1 << 20) + 8), None))


def test_subword_pool_bf16_rejects_bad_arguments():
    lib = pkg.load_library()
    f = lib.ggcn_subword_pool_bf16
    assert "null" in _err(lib, f(None, 64, 8, 1, P, 64, 64, P, 64, 64, 1, 8, 8, 64, None))
    assert "null" in _err(lib, f(P, 64, 8, 1, None, 64, 64, P, 64, 64, 1, 8, 8, 64, None))
    assert "leading" in _err(lib, f(P, 64, 8, 1, P, 64, 63, P, 64, 64, 1, 8, 8, 64, None))    # ldx < D


def test_bf16_precisions_and_cpu_refusal():
    assert set(BF16_PRECISIONS) == {"bf16x3", "f16mx8", "f16mx6"}
    m = GraphConvolution(16, 16)
    x = torch.zeros(2, 4, 16, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="GPU"):   # no CPU fallback for bf16 either
        m(x, torch.zeros(2, 4, 4))
