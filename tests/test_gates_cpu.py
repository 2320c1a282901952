"""The gates of the GPU tests (``oracle/gates.py``) and the call recorders of ``oracle/gpu_support.py``, pinned on hand-made CPU
tensors: an error exactly at the bound passes, one float64 ulp above it fails, a single NaN fails, the wrong dtype fails.

Every GPU test that compares against float64 goes through these few functions, so what they accept is stated here once.  The
bounds are recomputed below from their definitions, not taken from the functions under test."""
import ctypes
import math
import types

import pytest
import torch

from oracle import gates
from oracle.gpu_support import call_log, count_calls

SHAPE = (2, 3, 4)
AT = (1, 2, 3)          # the element that carries the error
TOP = (0, 0, 0)         # the element that carries max|ref| = 1


def _pair(dtype, bound_of):
    """``(got, ref, ref_above)``: got == ref exactly (ref[TOP] = 1, small values elsewhere) but for got[AT] = 0 against
    ref[AT] = b, the float64 fixed point of b = bound_of(b): the error there IS the bound.  ``ref_above`` has the next float64
    above b in that place."""
    got = (torch.arange(24, dtype=torch.float64).reshape(SHAPE) / 64.0).to(dtype)          # k / 64, k < 24: exact in bfloat16
    got[TOP], got[AT] = 1.0, 0.0
    ref = got.double()
    b = 0.0
    for _ in range(8):          # the bounds depend on ref[AT] through a factor <= 2^-8: the iteration settles in two steps
        b = bound_of(b)
    assert b == bound_of(b) and 0.0 < b < 1.0
    ref[AT] = b
    above = ref.clone()
    above[AT] = math.nextafter(b, 1.0)
    return got, ref, above


CASES = {
    "gate": (torch.float32, lambda b: 1e-4 * max(1.0, 1.0), lambda got, ref: gates.gate(got, ref, "t")),
    "gate-tol": (torch.float32, lambda b: 2e-5 * max(1.0, 1.0), lambda got, ref: gates.gate(got, ref, "t", 2e-5)),
    "gate_dx": (torch.bfloat16, lambda b: 2.0 ** -8 * b + 1e-4 * 1.0, lambda got, ref: gates.gate_dx(got, ref)),
    "close32": (torch.float32, lambda b: 2e-4 * (1.0 + 1e-12), lambda got, ref: gates.close32(got, ref, "t", 2e-4)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_at_the_bound_passes_and_one_ulp_above_fails(name):
    dtype, bound_of, check = CASES[name]
    got, ref, above = _pair(dtype, bound_of)
    check(got, ref)
    with pytest.raises(AssertionError):
        check(got, above)
    if name == "gate":
        assert gates.gate(got, ref, "t") == 1.0          # err / gate
    # a reference of the largest magnitude elsewhere widens the bound: the same error passes again
    wider = above.clone()
    wider[TOP] = 2.0
    got2 = got.clone()
    got2[TOP] = 2.0
    check(got2, wider)


@pytest.mark.parametrize("name", list(CASES))
def test_a_single_nan_fails_with_every_other_element_exact(name):
    dtype, _, check = CASES[name]
    got = (torch.arange(24, dtype=torch.float64).reshape(SHAPE) / 64.0).to(dtype)
    ref = got.double()
    check(got, ref)
    bad = got.clone()
    bad[AT] = float("nan")
    with pytest.raises(AssertionError):
        check(bad, ref)
    nan_ref = ref.clone()
    nan_ref[AT] = float("nan")
    with pytest.raises(AssertionError):
        check(got, nan_ref)


@pytest.mark.parametrize("name", list(CASES))
def test_the_wrong_dtype_fails(name):
    dtype, _, check = CASES[name]
    got = (torch.arange(24, dtype=torch.float64).reshape(SHAPE) / 64.0).to(dtype)
    for other in (torch.float32, torch.bfloat16, torch.float64, torch.float16):
        if other != dtype:
            with pytest.raises(AssertionError):
                check(got.to(other), got.double())


def test_gate_dtype_argument_and_the_empty_tensor():
    got = torch.zeros(SHAPE, dtype=torch.bfloat16)
    gates.gate(got, got.double(), "t", dtype=torch.bfloat16)
    gates.close32(got, got.double(), "t", 2e-4, dtype=torch.bfloat16)
    with pytest.raises(AssertionError):
        gates.gate(got.float(), got.double(), "t", dtype=torch.bfloat16)
    empty = torch.zeros(0, 3, 4)
    assert gates.gate(empty, empty.double(), "empty") == 0.0
    with pytest.raises(AssertionError):
        gates.gate(empty.double(), empty.double(), "empty")          # the dtype is asked of an empty result too


def test_gate_dx_bounds_every_element_by_its_own_reference():
    """An error that the largest reference entry would allow fails at an element whose own reference is small."""
    ref = torch.zeros(SHAPE, dtype=torch.float64)
    ref[TOP], ref[0, 0, 1] = 64.0, 32.125
    dx = ref.to(torch.bfloat16)
    assert float(dx[0, 0, 1]) == 32.0                    # off by 0.125 <= 2^-8 * 32.125 + 1e-4 * 64: inside
    gates.gate_dx(dx, ref)
    dx[AT] = 0.125                                       # the same error where ref = 0: the bound is 1e-4 * 64
    with pytest.raises(AssertionError):
        gates.gate_dx(dx, ref)


def test_first_argmax_resolves_a_tie_to_the_smaller_row():
    v = torch.tensor([[[1.0, 5.0], [3.0, 5.0], [3.0, 2.0], [3.0, 5.0]]])                 # [1, 4, 2]
    hot = gates.first_argmax(v)
    assert hot.dtype == torch.bool and hot.tolist() == [[[False, True], [True, False], [False, False], [False, False]]]
    assert bool((hot.sum(1) == 1).all())


def test_hostile_leaves_t_in_place_and_only_fill_elsewhere():
    t = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    buf = gates.hostile(t, 2)
    assert buf.shape == (4, 6) and buf.dtype == t.dtype and torch.equal(buf[:3, :4], t)
    assert bool(torch.isnan(buf[3]).all()) and bool(torch.isnan(buf[:, 4:]).all())
    buf = gates.hostile(t, 0, fill=7.0)
    assert buf.shape == (4, 4) and torch.equal(buf[:3], t) and bool((buf[3] == 7.0).all())
    ws = gates.poisoned(10, "cpu")
    assert ws.dtype == torch.uint8 and ws.numel() == 256 and bool((ws == 0xFF).all()) and gates.poisoned(1000, "cpu").numel() == 1000
    whole, view = gates.poisoned_rows("cpu", 3, 5, 8)
    assert whole.numel() == 31 and view.shape == (3, 5) and view.data_ptr() == whole[8:].data_ptr() and bool(torch.isnan(whole).all())
    assert whole.dtype == torch.float32
    whole, view = gates.poisoned_rows("cpu", 3, 5, 8, dtype=torch.float16)           # the half outputs of ggcn_aggregate_h
    assert whole.dtype == view.dtype == torch.float16 and whole.numel() == 31 and view.data_ptr() == whole[8:].data_ptr()
    assert bool(torch.isnan(whole).all())


def test_statement64_without_keep_factors_is_the_same_statement_bit_for_bit():
    B, T, F = 2, 5, 8
    g = torch.Generator().manual_seed(11)
    out, d_out = torch.randn(B, T, F, generator=g), torch.randn(B, T, F, generator=g)
    sg = torch.randn(B, F, generator=g)
    sg[0, 0] = 0.0                                       # a store gate of 0: y is taken as 0 there
    gb, d_pa = torch.rand(B, F, generator=g), torch.randn(B, F, generator=g)
    adj = torch.rand(B, T, T, generator=g)
    inv = 1.0 / (adj.sum(2) + 1.0)
    args = (out, sg, None, gb, d_out, d_pa, None, adj, inv)                              # gate a absent, d_pb absent
    ones = torch.ones(B, T, F, dtype=torch.float64)
    results = [gates.gate_pool_backward_statement64(*args), gates.gate_pool_backward_statement64(*args, keep=None),
               gates.gate_pool_backward_statement64(*args, keep=(None, None, None)),
               gates.gate_pool_backward_statement64(*args, keep=(ones, ones.clone(), ones.clone()))]
    assert set(results[0]) == {"d_sg", "d_ga", "dY", "d_bsum", "dH"}
    for r in results[1:]:
        assert set(r) == set(results[0])
        for k, v in results[0].items():
            assert v.dtype == torch.float64 and torch.equal(v.view(torch.int64), r[k].view(torch.int64)), k
    half = gates.gate_pool_backward_statement64(*args, keep=(ones, 0.5 * ones, ones))
    assert not torch.equal(half["d_ga"], results[0]["d_ga"])                             # the keep factors do enter


def _stub():
    """Two callables in the shape of library entries."""
    return types.SimpleNamespace(first=lambda a, b: a + b, second=lambda *a: len(a))


def test_count_calls_and_call_log_on_a_stub(monkeypatch):
    stub = _stub()
    first, second = stub.first, stub.second
    with monkeypatch.context() as mp:
        calls = count_calls(mp, ("first", "second"), lib=stub)
        log = call_log(mp, ("second",), lib=stub)
        assert calls == {"first": 0, "second": 0} and log == []
        assert stub.first(2, 3) == 5 and stub.first(4, 5) == 9                         # the return value comes through
        assert stub.second(ctypes.c_void_p(4096), ctypes.c_void_p(None), None, 7, 0.5) == 5
        assert stub.second() == 0
        assert calls == {"first": 2, "second": 2}
        assert log == [("second", [4096, None, None, 7, 0.5]), ("second", [])]
    assert stub.first is first and stub.second is second                               # nothing is left patched
    assert stub.first(1, 1) == 2 and calls == {"first": 2, "second": 2}


def test_count_calls_counts_the_precision_argument_under_its_own_key(monkeypatch):
    from ed_gated_gcn_amd import _capi
    stub = _stub()
    with monkeypatch.context() as mp:
        calls = count_calls(mp, ("first", "second"), prec_arg={"second": 1}, lib=stub)
        assert all(calls["second/" + p] == 0 for p in _capi.PREC)
        stub.second(0, _capi.PREC["fp32"])
        stub.second(0, _capi.PREC["bf16x3"], 9)
        stub.second(0, _capi.PREC["bf16x3"])
        stub.second(0, -123)
        stub.first(1, 2)
    assert calls["second"] == 4 and calls["second/fp32"] == 1 and calls["second/bf16x3"] == 2 and calls["second/?"] == 1
    assert calls["first"] == 1 and not any(k.startswith("first/") for k in calls)
