"""Sub-word pooling (csrc/subword_pool.hip, pooling.py) on every launch form against float64 and ITS derived bound.

The cases, the reference and the bound are those of oracle/subword_pool_cases.py (tests/test_subword_pool_cases_cpu.py holds them
to their claims without a GPU).  Which form a call takes is read from the logged arguments of the C entry with the kernel's own
rule (``takes_vector_form``), never assumed from the shape.

(a) every case through the Python layer, float32 and bfloat16, per element inside the bound, twice with the same bits.  A case
    with ``swap`` is the launch of the backward pass: it goes through ``pooling._launch(a, x, True)``, the call ``backward`` makes,
    so that it too can take ``x`` where the case puts it.
(b) the vector and the scalar form, and the swapped and the plain call, agree bit for bit: both add the same products in the same
    order (one fmaf per kept entry, ascending c).
(c) the C entries with Y inside NaN, X between NaN, and NaN in every row of X that A does not select.
(d) autograd; (e) empty operands like ``torch.bmm``.
"""
import numpy as np
import pytest
import torch

from oracle import subword_pool_cases as sc
from oracle.gpu_support import call_log, count_calls, dev, pkg  # noqa: F401

pytestmark = pytest.mark.gpu

ENTRIES = ("ggcn_subword_pool", "ggcn_subword_pool_bf16")
DTYPES = (torch.float32, torch.bfloat16)
DTYPE_IDS = ("f32", "bf16")
GUARD = 8          # elements of NaN on either side of Y: 32 bytes of float, 16 of bfloat16 -- the view keeps its alignment
WORST = {}         # part -> (worst err / bound seen, where)


@pytest.fixture(scope="module", autouse=True)
def worst_ratios():
    yield
    for k in sorted(WORST):
        print("\n  worst err / bound over the module, %s: %.3f (%s)" % (k, WORST[k][0], WORST[k][1]))


def _entry(dtype):
    return ENTRIES[dtype == torch.bfloat16]


def _within(got, ref, bound, part, what):
    """|got - ref| <= bound for every element (0 where the bound is 0), no NaN; records err / bound."""
    err = (got.double().cpu() - ref).abs()
    assert not bool(torch.isnan(err).any()), "%s: NaN" % what
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print("  %s %s: max err / bound %.3f (max err %.3g, max bound %.3g)" % (part, what, ratio, float(err.max()), float(bound.max())))
    if ratio > WORST.get(part, (-1.0, ""))[0]:
        WORST[part] = (ratio, what)
    bad = err > bound
    assert not bool(bad.any()), "%s: %d elements outside the bound, the worst %.3f times it" % (what, int(bad.sum()), ratio)


def _operands(case, dev, dtype):
    """(a, x on the device in the case's layout, float64 reference, bound): x rounded to ``dtype`` first, the reference and the bound
    taken on the rounded values."""
    a, x = sc.build(case)
    bf16 = dtype == torch.bfloat16
    xq = x.bfloat16() if bf16 else x
    return (sc.on_device(a, dev), sc.on_device(x, dev, dtype), sc.ref64(a, xq, case.swap), sc.bound(a, xq, case.swap, bf16))


def _pool(pkg, case, a, x):
    from ed_gated_gcn_amd import pooling
    return pooling._launch(a, x, True) if case.swap else pkg.subword_pool(a, x)


# ------------------------------------------------------------------------------------------------------- (a) every case
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("name", sc.CASE_IDS)
def test_case_against_float64(pkg, dev, monkeypatch, name, dtype):
    case = sc.CASE[name]
    bf16 = dtype == torch.bfloat16
    a, x, ref, bound = _operands(case, dev, dtype)
    assert x.stride() == (case.C * case.ldx + case.x_gap, case.ldx, 1) and x.dtype == dtype
    log = call_log(monkeypatch, ENTRIES)
    y = _pool(pkg, case, a, x)
    y2 = _pool(pkg, case, a, x)
    torch.cuda.synchronize()
    assert [n for n, _ in log] == [_entry(dtype)] * 2, [n for n, _ in log]
    args = log[0][1]
    assert args[:14] == [a.data_ptr()] + sc.wrapper_args(a, x, case.swap, bf16)[1:4] + [x.data_ptr()] + list(x.stride()[:2]) \
        + [y.data_ptr(), case.R * case.D, case.D, case.B, case.R, case.C, case.D]
    assert sc.takes_vector_form(args, bf16) == (case.form == "vector"), args
    assert y.dtype == dtype and tuple(y.shape) == (case.B, case.R, case.D) and y.is_contiguous()
    _within(y, ref, bound, "(a) " + DTYPE_IDS[bf16], name)
    assert torch.equal(y, y2), "%s: two calls, different bits" % name


# ---------------------------------------------------------------------------------------------------- (b) the forms agree
VECTOR_CASES = tuple(c.name for c in sc.CASES if c.form == "vector")


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("name", VECTOR_CASES)
def test_scalar_form_equals_vector_form_bit_for_bit(pkg, dev, monkeypatch, name, dtype):
    """The same values once aligned and once one element further into a buffer: the second call takes the scalar form (read from
    its arguments) and gives the same bits -- both forms make one fmaf per kept entry in ascending c."""
    case = sc.CASE[name]
    bf16 = dtype == torch.bfloat16
    a, x, _, _ = _operands(case, dev, dtype)
    x1 = sc.shifted(x)
    assert torch.equal(x1, x) and x1.stride() == x.stride() and x1.data_ptr() % 16 == x1.element_size()
    log = call_log(monkeypatch, ENTRIES)
    y, y1 = _pool(pkg, case, a, x), _pool(pkg, case, a, x1)
    torch.cuda.synchronize()
    assert [n for n, _ in log] == [_entry(dtype)] * 2
    assert sc.takes_vector_form(log[0][1], bf16) and not sc.takes_vector_form(log[1][1], bf16)
    assert torch.equal(y, y1), "%s: %d elements differ between the forms" % (name, int((y != y1).sum()))


SWAP_CASES = tuple(c.name for c in sc.CASES if c.swap)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("name", SWAP_CASES)
def test_swapped_call_equals_plain_call_on_the_transpose(pkg, dev, monkeypatch, name, dtype):
    case = sc.CASE[name]
    a, x, _, _ = _operands(case, dev, dtype)
    at = a.transpose(1, 2).contiguous()
    log = call_log(monkeypatch, ENTRIES)
    y, yt = _pool(pkg, case, a, x), pkg.subword_pool(at, x)
    torch.cuda.synchronize()
    (_, swapped), (_, plain) = log
    assert swapped[10:14] == plain[10:14] and swapped[2:4] == [a.stride(2), a.stride(1)] and plain[2:4] == [case.C, 1]
    assert torch.equal(y, yt), "%s: %d elements differ" % (name, int((y != yt).sum()))


# ------------------------------------------------------------------------------------------- (c) the C entries, hostile
# (id, D, ldx - D, x_batch - C * ldx, ldy - D, the form the launch must take)
HOSTILE = (("vector", 1028, 4, 8, 4, True),
           ("vector-shape-ldy3", 1028, 4, 8, 3, False),        # a row stride of Y alone takes the vector form away
           ("scalar-by-xbatch", 1028, 4, 2, 4, False),         # x_batch = C * ldx + 2: only the C entry can be handed this
           ("scalar-by-xbatch-ldy3", 1028, 4, 2, 3, False),
           ("scalar-by-width", 37, 3, 5, 4, False),
           ("scalar-by-width-ldy3", 37, 3, 5, 3, False))


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("form", HOSTILE, ids=[h[0] for h in HOSTILE])
def test_c_entries_in_a_hostile_state(pkg, dev, form, dtype):
    """Y [B, R, D] lies in a NaN buffer with rows ``ldy`` > D and batches R * ldy + 8 apart; X has NaN behind every row, between
    the batches, and in EVERY row that no non-zero of A selects.  Y[:, :, :D] matches float64 inside the bound, every other byte of
    the buffer of Y is unchanged, and nothing in the result is NaN: only the non-zeros of A are multiplied.  Where A is 0 and X is
    not finite the result is finite -- unlike the dense ``torch.bmm``, which makes 0 * NaN = NaN there.  That is the documented
    behaviour (csrc/subword_pool.hip, pooling.py: "multiplies only the non-zeros"), and it is what makes padding rows of x harmless."""
    from ed_gated_gcn_amd import _capi
    _, D, xpad, xgap, ypad, vector = form
    bf16 = dtype == torch.bfloat16
    B, R, C = 2, 5, 12
    rng = np.random.default_rng(7 + D + xgap + ypad)
    m = sc.dense_transform(B, R, C, 0.4, rng, scale=0.25, empty=(3,))
    m[:, :, [0, 5, C - 1]] = 0.0                                  # rows of X nothing selects
    m[0, :, 7] = 0.0                                              # ... and one in the first batch only
    a = torch.from_numpy(m)
    dead = torch.from_numpy((m != 0).sum(axis=1) == 0)            # [B, C]
    assert int(dead.sum()) >= 3 * B + 1 and int((~dead).sum()) > 0
    xv = torch.from_numpy(rng.standard_normal((B, C, D)).astype(np.float32)).to(dtype)
    ldx, ldy = D + xpad, D + ypad
    x_batch, y_batch = C * ldx + xgap, R * ldy + 8
    xbuf = torch.full((B * x_batch,), float("nan"), dtype=dtype, device=dev)
    x = xbuf.as_strided((B, C, D), (x_batch, ldx, 1), 0)
    x.copy_(torch.where(dead[:, :, None], torch.full_like(xv, float("nan")), xv))
    assert int(torch.isnan(xbuf).sum()) == xbuf.numel() - int((~dead).sum()) * D
    ybuf = torch.full((GUARD + B * y_batch + GUARD,), float("nan"), dtype=dtype, device=dev)
    y = ybuf.as_strided((B, R, D), (y_batch, ldy, 1), GUARD)
    inside = torch.zeros_like(ybuf, dtype=torch.bool)
    inside.as_strided((B, R, D), (y_batch, ldy, 1), GUARD).fill_(True)
    assert int(inside.sum()) == B * R * D
    bits = torch.int16 if bf16 else torch.int32
    snap = ybuf.clone()
    ad = a.to(dev)
    args = [_capi.ptr(ad), R * C, C, 1, _capi.ptr(x), x_batch, ldx, _capi.ptr(y), y_batch, ldy, B, R, C, D, _capi.stream_of(dev)]
    assert sc.takes_vector_form([v.value if hasattr(v, "value") else v for v in args], bf16) == vector
    lib = pkg.load_library()
    with torch.cuda.device(dev):
        _capi.check(getattr(lib, _entry(dtype))(*args), _entry(dtype))
    torch.cuda.synchronize()
    assert torch.equal(ybuf.view(bits)[~inside], snap.view(bits)[~inside]), "a byte outside Y[:, :, :D] changed"
    assert not bool(torch.isnan(y).any()), "NaN in the result: a row of X that A does not select was read into it"
    x0 = torch.where(dead[:, :, None], torch.zeros_like(xv), xv)  # the reference never sees the NaN: their factors are 0
    _within(y, sc.ref64(a, x0), sc.bound(a, x0, bf16=bf16), "(c) " + DTYPE_IDS[bf16], form[0])
    assert float(y[:, 3].abs().max()) == 0.0                      # the empty row: exact zeros


def test_c_entries_take_the_full_capacity(pkg, dev):
    """C = 2048 is accepted (C = 2049 is refused: tests/test_subword_pool_cases_cpu.py) -- through the C entry with an all-ones row
    on ones: 2048 exact additions."""
    from ed_gated_gcn_amd import _capi
    a = torch.zeros(1, 3, sc.MAX_COLS, device=dev)
    a[0, 1] = 1.0
    a[0, 2, -1] = 3.0
    x = torch.ones(1, sc.MAX_COLS, 4, device=dev)
    x[0, -1] = 2.0
    y = torch.full((1, 3, 4), float("nan"), device=dev)
    with torch.cuda.device(dev):
        _capi.check(pkg.load_library().ggcn_subword_pool(_capi.ptr(a), a.stride(0), a.stride(1), 1, _capi.ptr(x), x.stride(0), 4,
                                                         _capi.ptr(y), 12, 4, 1, 3, sc.MAX_COLS, 4, _capi.stream_of(dev)),
                    "ggcn_subword_pool")
    assert y.cpu().tolist() == [[[0.0] * 4, [2049.0] * 4, [6.0] * 4]]


# ---------------------------------------------------------------------------------------------------------- (d) autograd
GRAD_CASES = ("slab-vector-D1028", "slab-scalar-D1025", "a-step2")


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("name", GRAD_CASES)
def test_autograd_against_float64(pkg, dev, monkeypatch, name, dtype):
    """dX = a^T dY against float64 autograd through ``torch.bmm``, at the bound of the transposed product; the incoming gradient
    is a non-contiguous view (the first D columns of wider rows)."""
    case = sc.CASE[name]
    bf16 = dtype == torch.bfloat16
    a, x, ref, bound = _operands(case, dev, dtype)
    a_cpu, _ = sc.build(case)
    rng = np.random.default_rng(11)
    dy_cpu = torch.from_numpy(rng.standard_normal((case.B, case.R, case.D + 3)).astype(np.float32)).to(dtype)
    dy = dy_cpu.to(dev)[..., :case.D]
    assert not dy.is_contiguous()
    x64 = x.detach().cpu().double().requires_grad_(True)
    torch.bmm(a_cpu.double(), x64).backward(dy_cpu[..., :case.D].double())
    xg = x.detach().clone().requires_grad_(True)
    calls = count_calls(monkeypatch, ENTRIES)
    y = pkg.subword_pool(a, xg)
    assert y.requires_grad and calls[_entry(dtype)] == 1
    y.backward(dy)
    torch.cuda.synchronize()
    assert calls[_entry(dtype)] == 2 and calls[_entry(DTYPES[not bf16])] == 0
    assert a.grad is None and xg.grad.dtype == dtype and xg.grad.shape == xg.shape
    _within(y.detach(), ref, bound, "(d) forward " + DTYPE_IDS[bf16], name)
    _within(xg.grad, x64.grad, sc.bound(a_cpu, dy_cpu[..., :case.D], swap=True, bf16=bf16), "(d) dX " + DTYPE_IDS[bf16], name)


def test_autograd_launches_only_what_is_needed(pkg, dev, monkeypatch):
    from ed_gated_gcn_amd.pooling import _SubwordPool
    case = sc.CASE["slab-scalar-D3"]
    a, x, _, _ = _operands(case, dev, torch.float32)
    calls = count_calls(monkeypatch, ENTRIES)
    w = torch.ones((), device=dev, requires_grad=True)
    y = pkg.subword_pool(a, x)                      # x does not require a gradient: nothing to go back through
    assert not y.requires_grad
    (y * w).sum().backward()
    torch.cuda.synchronize()
    assert calls == {ENTRIES[0]: 1, ENTRIES[1]: 0} and w.grad is not None

    class Ctx:
        saved_tensors = (a,)
        needs_input_grad = (False, False)
    assert _SubwordPool.backward(Ctx, torch.ones_like(y)) == (None, None) and calls[ENTRIES[0]] == 1
    Ctx.needs_input_grad = (False, True)
    d_a, d_x = _SubwordPool.backward(Ctx, torch.ones_like(y))
    assert d_a is None and d_x.shape == x.shape and calls[ENTRIES[0]] == 2      # the transform gets None
    with pytest.raises(RuntimeError, match="does not differentiate"):
        pkg.subword_pool(a.clone().requires_grad_(True), x)
    assert calls[ENTRIES[0]] == 2


# ---------------------------------------------------------------------------------------------------- (e) empty operands
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("B,T,L,D", [(0, 3, 5, 8), (2, 0, 5, 8), (2, 3, 0, 8), (2, 3, 5, 0), (0, 0, 0, 0)],
                         ids=["B0", "T0", "L0", "D0", "all0"])
def test_empty_operands_like_bmm(pkg, dev, monkeypatch, B, T, L, D, dtype):
    """What ``torch.bmm`` returns: an empty [B, T, D], or zeros for L = 0 (the empty sum); x's dtype and device, no library call,
    and differentiable with a zero or empty gradient."""
    a = torch.ones(B, T, L, device=dev)
    x = torch.ones(B, L, D, device=dev, dtype=dtype, requires_grad=True)
    want = torch.bmm(torch.ones(B, T, L, dtype=dtype), torch.ones(B, L, D, dtype=dtype))
    calls = count_calls(monkeypatch, ENTRIES)
    y = pkg.subword_pool(a, x)
    assert tuple(y.shape) == tuple(want.shape) == (B, T, D) and y.dtype == dtype and y.device == x.device
    assert torch.equal(y.detach().cpu(), want)
    assert y.requires_grad
    y.sum().backward()
    torch.cuda.synchronize()
    assert x.grad is not None and x.grad.shape == x.shape and x.grad.dtype == dtype
    want_grad = torch.zeros(B, L, D, dtype=dtype) if T == 0 else torch.full((B, L, D), float(T), dtype=dtype)
    assert torch.equal(x.grad.cpu(), want_grad)
    assert calls == {ENTRIES[0]: 0, ENTRIES[1]: 0}
    with pytest.raises(RuntimeError, match="does not match"):
        pkg.subword_pool(torch.ones(B, T, L + 1, device=dev), x)
