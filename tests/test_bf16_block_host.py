"""CPU checks of the bfloat16 block entries (include/ggcn.h "bfloat16 features": ggcn_block_fused_bf16, ggcn_aggregate_bf16):
declared, bound and exported with the ABI still 14 (functions were added, nothing changed), every refusal returning its code and
a message that names the argument BEFORE any launch (the pointers handed in are never dereferenced), and the new predicates of
gated_block saying no to CPU tensors, to float32 text and to layers whose ``bf16_block`` option is off (the default)."""
import ctypes
import re
import types

import torch

import ed_gated_gcn_amd as pkg
from ed_gated_gcn_amd import _capi, gated_block
from ed_gated_gcn_amd.gcn import GraphConvolution
from oracle.host_support import header as _header, msg as _msg

EINVAL, EUNSUPPORTED = 1, 3
NEW = ("ggcn_block_fused_bf16", "ggcn_aggregate_bf16")
P = ctypes.c_void_p(1 << 20)   # a non-null, 16-byte aligned address: never dereferenced (the checks come first)
ODD = ctypes.c_void_p((1 << 20) + 1)
OFF2 = ctypes.c_void_p((1 << 20) + 2)
OFF8 = ctypes.c_void_p((1 << 20) + 8)


def test_new_symbols_declared_bound_and_exported():
    src = _header()
    lib = ctypes.CDLL(pkg.lib_path())
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _capi.PROTOTYPES, name
        assert hasattr(lib, name), name
    # the argument list of ggcn_block_fused without `precision`
    full, bf = _capi.PROTOTYPES["ggcn_block_fused"][1], _capi.PROTOTYPES["ggcn_block_fused_bf16"][1]
    assert bf == full[:-2] + full[-1:]


def test_abi_version_stays_14_on_all_three_sides():
    m = re.search(r"#define\s+GGCN_ABI_VERSION\s+(\d+)", _header())
    assert int(m.group(1)) == 14
    assert _capi.ABI_VERSION == 14
    assert pkg.load_library().ggcn_abi_version() == 14


def _block(lib, x=P, ldx=64, w1=P, w12=P, ops=P, ops2=P, mid=P, T=31, gate1=P, gate2=P, gcn1=None, ld1=64, xo=P, ld2=64, x1=P, y1=P,
           out=P, part=None, B=4, F=64):
    return lib.ggcn_block_fused_bf16(x, ldx, w1, w12, ops, ops2, None, mid, None, B, T, 64, F, gate1, gate2, gcn1, ld1, xo, ld2,
                                     x1, y1, out, part, None)


def test_block_fused_bf16_refuses_bad_arguments():
    lib = pkg.load_library()
    assert "null input" in _msg(lib, _block(lib, x=None), EINVAL)
    assert "X not 2-byte aligned" in _msg(lib, _block(lib, x=ODD), EINVAL)
    assert "weight image" in _msg(lib, _block(lib, w1=None), EINVAL)
    assert "weight image" in _msg(lib, _block(lib, w12=None), EINVAL)
    assert "wpack must be 16-byte aligned" in _msg(lib, _block(lib, w1=OFF8), EINVAL)
    assert "wpack must be 16-byte aligned" in _msg(lib, _block(lib, w12=OFF8), EINVAL)
    assert "operand blocks" in _msg(lib, _block(lib, ops=None), EINVAL)
    assert "graph_ops must be 16-byte aligned" in _msg(lib, _block(lib, ops=OFF8), EINVAL)
    assert "graph_ops2" in _msg(lib, _block(lib, ops2=None), EINVAL)
    assert "graph_ops2 must be 16-byte aligned" in _msg(lib, _block(lib, ops2=OFF8), EINVAL)
    assert "bias_mid" in _msg(lib, _block(lib, mid=None), EINVAL)
    assert "gate2" in _msg(lib, _block(lib, gate2=None), EINVAL)
    assert "ldx < K" in _msg(lib, _block(lib, ldx=63), EINVAL)
    assert "leading dimension of the output" in _msg(lib, _block(lib, ld2=63), EINVAL)
    assert "leading dimension of the output" in _msg(lib, _block(lib, gcn1=P, ld1=63), EINVAL)
    assert "neither x nor its pool" in _msg(lib, _block(lib, xo=None, out=None), EINVAL)
    # layer 1's outputs in part
    for kw in (dict(x1=None), dict(y1=None), dict(gate1=None), dict(x1=None, y1=None, gcn1=P), dict(x1=None, y1=None, part=P)):
        assert "layer 1's outputs go together" in _msg(lib, _block(lib, **kw), EINVAL), kw
    m = _msg(lib, _block(lib, T=33), EUNSUPPORTED)
    assert "T=33" in m and "ggcn_layer_fused_bf16_wide" in m
    # the eval form (nothing of layer 1) keeps the checks of what it reads
    ev = dict(x1=None, y1=None, gate1=None, w1=None, ops=None)
    assert "weight image" in _msg(lib, _block(lib, w12=None, **ev), EINVAL)
    assert "graph_ops2 must be 16-byte aligned" in _msg(lib, _block(lib, ops2=OFF8, **ev), EINVAL)
    assert "T=40" in _msg(lib, _block(lib, T=40, **ev), EUNSUPPORTED)


def _agg(lib, x=P, ldx=64, rowptr=P, colidx=P, z=P, ldz=64, B=4, T=100, K=64):
    return lib.ggcn_aggregate_bf16(x, ldx, rowptr, colidx, None, B, T, K, z, ldz, None)


def test_aggregate_bf16_refuses_bad_arguments():
    lib = pkg.load_library()
    assert "null input" in _msg(lib, _agg(lib, x=None), EINVAL)
    assert "null input" in _msg(lib, _agg(lib, rowptr=None), EINVAL)
    assert "null input" in _msg(lib, _agg(lib, colidx=None), EINVAL)
    assert "null output" in _msg(lib, _agg(lib, z=None), EINVAL)
    assert "ldx < K" in _msg(lib, _agg(lib, ldx=63), EINVAL)
    assert "ldz < K" in _msg(lib, _agg(lib, ldz=63), EINVAL)
    assert "X not 2-byte aligned" in _msg(lib, _agg(lib, x=ODD), EINVAL)
    assert "Z not 4-byte aligned" in _msg(lib, _agg(lib, z=OFF2), EINVAL)
    assert "must be positive" in _msg(lib, _agg(lib, B=0), EINVAL)
    assert "B*T" in _msg(lib, _agg(lib, B=1 << 24, T=128), EUNSUPPORTED)


def test_layer_fused_bf16_keeps_its_range():
    """The <= 32-node layer entry still refuses longer graphs (GGCN_EUNSUPPORTED) and names the entry that takes them."""
    lib = pkg.load_library()
    rc = lib.ggcn_layer_fused_bf16(P, 64, P, P, None, 4, 33, 64, 64, None, None, None, P, 64, None, None, None, None, None, None)
    m = _msg(lib, rc, EUNSUPPORTED)
    assert "T=33" in m and "ggcn_layer_fused_bf16_wide" in m


def test_option_is_off_by_default_and_read_from_opt_and_env(monkeypatch):
    monkeypatch.delenv("GGCN_BF16_BLOCK", raising=False)
    assert GraphConvolution(16, 16).bf16_block is False
    assert GraphConvolution(16, 16, opt=types.SimpleNamespace(ggcn_bf16_block=True)).bf16_block is True
    monkeypatch.setenv("GGCN_BF16_BLOCK", "1")
    assert GraphConvolution(16, 16).bf16_block is True


def test_new_predicates_say_no_to_cpu_float32_and_the_default(monkeypatch):
    monkeypatch.delenv("GGCN_BF16_BLOCK", raising=False)
    on = types.SimpleNamespace(ggcn_bf16_block=True)
    for T in (8, 100):
        csr = types.SimpleNamespace(T=T, B=2, is_binary=True, rowmask=torch.zeros(2 * T, (T + 31) // 32, dtype=torch.int32))
        for opt in (None, on):
            gc1, gc2 = GraphConvolution(16, 16, opt=opt), GraphConvolution(16, 16, opt=opt)
            for x in (torch.zeros(2, T, 16, dtype=torch.bfloat16), torch.zeros(2, T, 16, dtype=torch.float32)):
                assert gated_block.takes_bf16_block_path(x, csr, gc1, gc2) is False          # CPU tensors / float32 text / option off
                assert gated_block.takes_bf16_folded_eval_path(x, csr, gc1, gc2) is False
