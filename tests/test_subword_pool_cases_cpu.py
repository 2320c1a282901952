"""The cases of the sub-word pooling tests (oracle/subword_pool_cases.py) held to what they claim, their bound held to a float32
evaluation, and the refusals of the two C entries -- all without a GPU.

A case names the launch form it must take and the rows it forces; the GPU tests (tests/test_gpu_subword_pool.py) rely on both, so
both are checked here on the very inputs they use.  The bound is derived, not measured: it has to be tight enough to see an error
(below 1e-5 of the result's scale) and loose enough that an honest float32 evaluation in the kernel's order passes it.
"""
import ctypes

import numpy as np
import pytest
import torch

import ed_gated_gcn_amd as pkg
from oracle import subword_pool_cases as sc
from oracle.host_support import msg as _msg

EINVAL, EUNSUPPORTED = 1, 3
P = ctypes.c_void_p(1 << 20)   # a non-null, 16-byte aligned address: never dereferenced (the checks come first)


@pytest.fixture(scope="module")
def built():
    """name -> (a, x, launch matrix): every case built once."""
    out = {}
    for c in sc.CASES:
        a, x = sc.build(c)
        out[c.name] = (a, x, sc.launch_matrix(c, a))
    return out


# ------------------------------------------------------------------------------------------------------------------ the list
def test_the_list_holds_what_the_tests_are_about():
    names = set(sc.CASE_IDS)
    assert len(names) == len(sc.CASES)
    for D in sc.VECTOR_D:
        assert {"slab-vector-D%d" % D, "swap-slab-vector-D%d" % D} <= names
    for D in sc.SCALAR_D:
        assert {"slab-scalar-D%d" % D, "swap-slab-scalar-D%d" % D} <= names
    for C in sc.ROUND_C:
        assert {"rounds-C%d" % C, "swap-rounds-C%d" % C} <= names
    assert sc.VECTOR_D == (4, 1020, 1024, 1028, 2052) and sc.SCALAR_D == (1, 3, 255, 257, 1023, 1025, 2049)
    assert sc.ROUND_C == (1, 255, 256, 257, 512, 513)
    for c in sc.CASES:
        assert c.form in ("vector", "scalar") and 1 <= c.B <= 3 and 1 <= c.C <= sc.MAX_COLS, c.name
        assert c.B * (c.R + c.C) * c.D <= 1 << 18, c.name                  # small: a megabyte of x and y at the most
        if c.name != "swap-capacity-R2048":                                 # blockIdx.x / R is no shift
            assert c.R & (c.R - 1), "%s: R = %d is a power of two" % (c.name, c.R)
    assert sc.CASE["capacity-C2048"].C == sc.MAX_COLS and sc.CASE["swap-capacity-R2048"].R == 2048
    assert {sc.CASE["swap-rows-R257"].R, sc.CASE["swap-rows-R513"].R} == {257, 513}
    assert any(c.x_off for c in sc.CASES) and any(c.ldx == c.D + 1 for c in sc.CASES) and any(c.x_gap == 2 for c in sc.CASES)
    assert {c.a_layout for c in sc.CASES} == {"contig", "slice", "step2", "perm"}


def test_cases_are_built_by_seed():
    for name in ("rounds-C513", "swap-reference-D37", "scalar-by-base-D1028"):
        (a0, x0), (a1, x1) = sc.build(sc.CASE[name]), sc.build(sc.CASE[name])
        assert torch.equal(a0, a1) and torch.equal(x0, x1) and a0.stride() == a1.stride()


# ---------------------------------------------------------------------------------------------------------------- the claims
@pytest.mark.parametrize("name", sc.CASE_IDS)
def test_case_claims(built, name):
    c = sc.CASE[name]
    a, x, m = built[name]
    B, R, C, D = c.B, c.R, c.C, c.D
    assert tuple(m.shape) == (B, R, C) and tuple(x.shape) == (B, C, D)
    assert tuple(a.shape) == ((B, C, R) if c.swap else (B, R, C))
    assert not bool(torch.isnan(x).any()) and bool(torch.isfinite(a).all())
    assert x.stride() == (C * c.ldx + c.x_gap, c.ldx, 1) and x.storage_offset() == c.x_off
    # the layouts are what they are named after
    if c.a_layout == "contig":
        assert a.is_contiguous()
    elif c.a_layout == "slice":
        assert a.stride() == ((a.shape[1] + 3) * (a.shape[2] + 5), a.shape[2] + 5, 1)
    elif c.a_layout == "step2":
        assert a.stride(2) == 2
    else:
        assert a.stride(1) == 1 and a.stride(2) == a.shape[1]
    if c.a_layout != "contig":      # junk, not zeros, wherever the view does not reach
        whole = torch.as_strided(a, (a.untyped_storage().nbytes() // 4,), (1,), 0)
        assert int((whole == sc.JUNK).sum()) == whole.numel() - a.numel()
    # the rows
    nnz = (m != 0).sum(dim=2)
    rounds = -(-C // sc.ROUND)
    assert c.rounds == rounds and c.nnz[0] <= int(nnz.max()) <= c.nnz[1], (rounds, int(nnz.max()))
    rows = c.rows
    if "empty" in rows:
        assert int(nnz[:, rows["empty"]].max()) == 0
    if "full" in rows:
        assert int(nnz[:, rows["full"]].min()) == C
    if "last_round" in rows:
        r, first = rows["last_round"], sc.ROUND * (rounds - 1)
        assert int((m[:, r, :first] != 0).sum()) == 0 and bool((m[:, r, first:] != 0).all())
    if "ends" in rows:
        cols = sorted({0, C - 1})
        for b in range(B):
            assert torch.nonzero(m[b, rows["ends"]]).ravel().tolist() == cols
    if name.endswith(("rounds-C512", "rounds-C513")):
        assert rounds == 3 - (C == 512) and int(nnz.max()) > sc.ROUND       # more non-zeros than one round brings
    if name.endswith("rounds-C257"):
        assert rounds == 2
    if name.endswith(("rounds-C1", "rounds-C255", "rounds-C256")):
        assert rounds == 1
    if "capacity-C2048" in name:
        assert rounds == 8 and int(nnz.max()) == sc.MAX_COLS
        free = nnz[:, 2]
        assert 0 < int(free.min()) and int(free.max()) < C                  # the third row is neither
    if c.kind == "reference":       # 1/l on l <= 4 consecutive positions from offset 1; a word per row, each position in one word
        t = m.transpose(1, 2) if c.swap else m
        assert int((t != 0).sum(dim=2).max()) <= 4 and int((t != 0).sum(dim=1).max()) == 1 and not bool(t[:, :, 0].any())
        sums = t.sum(dim=2)
        assert bool(((sums - 1).abs() < 1e-6)[(t != 0).any(dim=2)].all())
    # the form: the arguments the Python wrapper passes, x where the case puts it
    for bf16 in (False, True):
        args = sc.wrapper_args(a, x, c.swap, bf16)
        assert dict(zip(sc.ARGS, args))["X"] % 16 == (c.x_off * (2 if bf16 else 4)) % 16
        assert args[10:14] == [B, R, C, D]
        assert sc.takes_vector_form(args, bf16) == (c.form == "vector"), (name, bf16)


def test_vector_rule_term_by_term():
    """Every term of the rule alone turns the vector form off, at the alignment of its type."""
    good = [sc.A_BASE, 72, 9, 1, sc.X_BASE, 9 * 1028, 1028, sc.Y_BASE, 3 * 1028, 1028, 2, 3, 9, 1028, None]
    at = {k: i for i, k in enumerate(sc.ARGS)}
    assert sc.takes_vector_form(good, False) and sc.takes_vector_form(good, True)
    for k in ("D", "ldx", "ldy", "x_batch", "y_batch"):
        for d in (1, 2, 3):
            bad = list(good)
            bad[at[k]] += d
            assert not sc.takes_vector_form(bad, False) and not sc.takes_vector_form(bad, True), (k, d)
    for k in ("X", "Y"):
        for d, f32, bf16 in ((2, False, False), (4, False, False), (8, False, True), (16, True, True)):
            bad = list(good)
            bad[at[k]] += d
            assert sc.takes_vector_form(bad, False) == f32 and sc.takes_vector_form(bad, True) == bf16, (k, d)
    for k in ("A", "sa_b", "sa_r", "sa_c"):     # A is read one element at a time: it has no say
        bad = list(good)
        bad[at[k]] += 1
        assert sc.takes_vector_form(bad, False)


# ----------------------------------------------------------------------------------------------------------------- the bound
def test_reference_and_bound_by_hand():
    a = torch.tensor([[[0.5, 0.0, -2.0], [0.0, 0.0, 0.0]]])
    x = torch.tensor([[[1.0, 2.0], [100.0, 100.0], [3.0, -1.0]]])
    assert sc.ref64(a, x).tolist() == [[[-5.5, 3.0], [0.0, 0.0]]]
    assert sc.ref64(a.transpose(1, 2).contiguous(), x, swap=True).tolist() == [[[-5.5, 3.0], [0.0, 0.0]]]
    s = torch.tensor([[[6.5, 3.0], [0.0, 0.0]]], dtype=torch.float64)
    want = 3 * sc.U32 * s + torch.tensor([[[2.0], [0.0]]], dtype=torch.float64) * sc.TINY32
    assert torch.equal(sc.bound(a, x), want)
    assert torch.equal(sc.bound(a.transpose(1, 2).contiguous(), x, swap=True), want)
    want16 = 2.0 ** -8 * sc.ref64(a, x).abs() + 2 * 3 * sc.U32 * s + torch.tensor([[[2.0], [0.0]]], dtype=torch.float64) * sc.TINY32
    assert torch.equal(sc.bound(a, x, bf16=True), want16)
    assert sc.ascending_float32(a, x).tolist() == [[[-5.5, 3.0], [0.0, 0.0]]]


@pytest.mark.parametrize("name", sc.CASE_IDS)
def test_bound_is_neither_vacuous_nor_impossible(built, name):
    c = sc.CASE[name]
    a, x, m = built[name]
    ref = sc.ref64(a, x, c.swap)
    b32 = sc.bound(a, x, c.swap)
    assert tuple(ref.shape) == tuple(b32.shape) == (c.B, c.R, c.D)
    # not vacuous: an error of 1e-5 of the result's scale does not fit in it
    assert float(b32.max()) < 1e-5 * max(1.0, float(ref.abs().max())), (float(b32.max()), float(ref.abs().max()))
    empty = (m != 0).sum(dim=2) == 0
    assert float(b32[empty].max() if bool(empty.any()) else 0.0) == 0.0
    # not impossible: float32 in the kernel's order fits in it, and so does its bfloat16 rounding on bfloat16 inputs
    got = torch.from_numpy(sc.ascending_float32(a, x, c.swap))
    err = (got.double() - ref).abs()
    assert bool((err <= b32).all()), float((err / b32.clamp_min(1e-300)).max())
    xb = x.bfloat16()
    ref16, b16 = sc.ref64(a, xb, c.swap), sc.bound(a, xb, c.swap, bf16=True)
    got16 = torch.from_numpy(sc.ascending_float32(a, xb, c.swap)).bfloat16()
    err16 = (got16.double() - ref16).abs()
    assert bool((err16 <= b16).all()), float((err16 / b16.clamp_min(1e-300)).max())
    assert float((b16 - 2.0 ** -8 * ref16.abs()).max()) < 2e-5 * max(1.0, float(ref16.abs().max()))


# -------------------------------------------------------------------------------------------------------------- the refusals
# Fake pointers: never where a launch could reach a card (a check that stopped refusing would launch on them).
no_card = pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: never where a launch could reach a card")
ENTRIES = ("ggcn_subword_pool", "ggcn_subword_pool_bf16")


def _call(lib, entry, A=P, X=P, Y=P, ldx=64, ldy=64, B=2, R=8, C=8, D=64):
    return getattr(lib, entry)(A, R * C, C, 1, X, C * ldx, ldx, Y, R * ldy, ldy, B, R, C, D, None)


@no_card
@pytest.mark.parametrize("entry", ENTRIES)
def test_entries_refuse_bad_arguments(entry):
    lib = pkg.load_library()
    for k in ("A", "X", "Y"):
        assert "null" in _msg(lib, _call(lib, entry, **{k: None}), EINVAL, entry), k
    for k in ("B", "R", "C", "D"):
        for v in (0, -1):
            text = _msg(lib, _call(lib, entry, **{k: v}), EINVAL, entry)
            assert "must be positive" in text and "%s=%d" % (k, v) in text, text
    text = _msg(lib, _call(lib, entry, C=sc.MAX_COLS + 1), EUNSUPPORTED, entry)
    assert "C=2049" in text and "2048" in text.replace("C=2049", ""), text
    assert "leading" in _msg(lib, _call(lib, entry, ldx=63), EINVAL, entry)
    assert "leading" in _msg(lib, _call(lib, entry, ldy=63), EINVAL, entry)
    # the order of the list: a null pointer is named before a size, a size before the capacity, the capacity before a stride
    assert "null" in _msg(lib, _call(lib, entry, A=None, B=0, C=4096, ldx=1), EINVAL, entry)
    assert "positive" in _msg(lib, _call(lib, entry, B=0, C=4096, ldx=1), EINVAL, entry)
    assert "columns" in _msg(lib, _call(lib, entry, C=4096, ldx=1), EUNSUPPORTED, entry)
    # C = 2048 passes the capacity check: the next fault in the list is the one reported (no launch is needed to see that)
    assert "leading" in _msg(lib, _call(lib, entry, C=sc.MAX_COLS, ldx=63), EINVAL, entry)


def test_wrapper_checks_come_before_any_device():
    from ed_gated_gcn_amd.pooling import subword_pool
    a, x = torch.zeros(2, 3, 4), torch.zeros(2, 4, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        subword_pool(a, x)
    with pytest.raises(TypeError):
        subword_pool(a[0], x)
