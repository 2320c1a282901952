"""The forward linear's case table (``linear_ref.py``) checked without a GPU: the form every case expects is the form
``ggcn_linear_form`` -- the function the launchers themselves dispatch on -- names for such operands, the table reaches every form a
launcher can pick, the query refuses what the entries refuse, and the derived gates hold for an emulation of the arithmetic with
room to spare.  The library loads without a GPU (``ggcn_linear_form`` launches nothing and dereferences nothing): device buffers
are imitated by integer pointer values, 16-byte aligned plus the case's offset."""
import ctypes

import pytest
import torch

import linear_ref as lr
from ed_gated_gcn_amd import _capi

BASE_X, BASE_W, BASE_Y = 1 << 32, 3 << 32, 5 << 32     # 16-byte aligned stand-ins for device allocations


def _form(lib, c, x=None, y=None, w=BASE_W, M=None, K=None, ldx=None, ldy=None, ldw=None, precision=None, entry=None):
    ox, oy = lr.pointer_offsets(c)
    P = ctypes.c_void_p
    return lib.ggcn_linear_form(_capi.LINEAR_ENTRY[c.entry] if entry is None else entry, P(BASE_X + ox if x is None else x),
                                c.K + c.pad_x if ldx is None else ldx, P(w), c.F + c.pad_w if ldw is None else ldw,
                                P(BASE_Y + oy if y is None else y), c.F + c.pad_y if ldy is None else ldy,
                                c.M if M is None else M, c.K if K is None else K, c.F,
                                _capi.PREC[c.precision] if precision is None else precision)


def test_form_bits_are_the_headers():
    assert (lr.XVEC, lr.KFULL, lr.VST, lr.WVEC) == (_capi.FORM_XVEC, _capi.FORM_KFULL, _capi.FORM_VST, _capi.FORM_WVEC) == (1, 2, 4, 8)
    from oracle import host_support
    h = host_support.header()
    for name, v in list(_capi.LINEAR_ENTRY.items()) + [("FORM_XVEC", 1), ("FORM_KFULL", 2), ("FORM_VST", 4), ("FORM_WVEC", 8)]:
        enum = "GGCN_ENTRY_" + name[5:].upper() if name.startswith("ggcn_") else "GGCN_" + name
        assert "%s = %d" % (enum, v) in h, enum
    assert "#define GGCN_ABI_VERSION 14" in h and _capi.ABI_VERSION == 14        # a function was added, no prototype changed


@pytest.mark.parametrize("c", lr.CASES, ids=lr.case_id)
def test_every_case_takes_the_form_it_names(c):
    lib = _capi.load_library()
    got = _form(lib, c)
    assert got == c.form, "%s: ggcn_linear_form says %d, the table %d (%s)" % (lr.case_id(c), got, c.form, lib.ggcn_last_error().decode())


def test_the_table_reaches_every_form_of_every_launcher():
    reached = {}
    for c in lr.CASES:
        reached.setdefault((c.entry, c.precision), set()).add(c.form)
    assert reached == lr.FORMS, {k: (sorted(reached.get(k, ())), sorted(v)) for k, v in lr.FORMS.items() if reached.get(k) != v}
    # four forms per float entry of launch_linear, three per half entry, three of launch_linear_f16, four of linear_fp32
    assert [len(lr.FORMS[k]) for k in sorted(lr.FORMS)] == [4, 4, 4, 3, 3, 3, 1]
    ids = [lr.case_id(c) for c in lr.CASES]
    assert len(set(ids)) == len(ids)


def test_the_two_boundaries_the_launchers_draw():
    """ldx * sizeof * 257 < 2^31 for the 16-byte loads of the split kernels, exactly; any M for the fp32 kernel (it walks the rows
    in slices of 65535 tiles) while the split kernels' grid has a limit the query reports."""
    lib = _capi.load_library()
    c = next(c for c in lr.CASES if c.precision == "bf16x3" and c.pad_x == lr.LDX_LAST_FAST - 64)
    assert _form(lib, c, ldx=lr.LDX_LAST_FAST) == lr.FAST and _form(lib, c, ldx=lr.LDX_FIRST_SLOW) == lr.ELEM
    assert all(_form(lib, c, ldx=v) == lr.ELEM for v in lr.LDX_BEYOND)
    h = next(c for c in lr.CASES if c.entry == lr.LINEAR_H and c.precision == "bf16x3" and c.form == lr.STAGED)
    last = (2 ** 31 - 1) // (2 * 257) // 8 * 8
    assert last * 2 * 257 < 2 ** 31 <= (last + 8) * 2 * 257
    assert _form(lib, h, ldx=last) == lr.STAGED and _form(lib, h, ldx=last + 8) == lr.ELEM
    f = next(c for c in lr.CASES if c.precision == "fp32" and c.M > lr.ROW_TILES_MAX * 128)
    assert _form(lib, f, M=2 ** 40) == f.form
    s = next(c for c in lr.CASES if c.precision == "bf16x3" and c.form == lr.FAST)
    assert _form(lib, s, M=2 ** 31 * 128 // 8) == lr.FAST and _form(lib, s, M=2 ** 40) == -3       # GGCN_EUNSUPPORTED: M too large


def test_the_query_refuses_what_the_entries_refuse():
    lib = _capi.load_library()
    c = lr.CASES[0]
    e = _capi.LINEAR_ENTRY
    assert _form(lib, c) == lr.FAST
    assert _form(lib, c, x=0) == -1 and _form(lib, c, y=0) == -1                                     # GGCN_EINVAL: null pointer
    assert _form(lib, c, M=0) == -1 and _form(lib, c, ldx=c.K - 1) == -1 and _form(lib, c, ldy=c.F - 1) == -1
    assert _form(lib, c, precision=_capi.PREC["f16"]) == -1 and _form(lib, c, precision=77) == -1   # ggcn_linear has no such precision
    assert _form(lib, c, entry=9) == -1 and "unknown entry" in lib.ggcn_last_error().decode()
    assert _form(lib, c, precision=_capi.PREC["fp32"], w=0) == -1 and _form(lib, c, precision=_capi.PREC["fp32"], ldw=c.F - 1) == -1
    assert _form(lib, c, entry=e["ggcn_linear_h"], precision=_capi.PREC["fp32"]) == -3               # GGCN_EUNSUPPORTED
    assert _form(lib, c, entry=e["ggcn_linear_h"], precision=_capi.PREC["f16"]) == lr.VEC             # K = 32: half a 64-k stage
    # bf16 entries: operands aligned to their element size, and the staged stores for float32 Y alone
    assert _form(lib, c, entry=e["ggcn_linear_bf16"]) == lr.FAST and _form(lib, c, entry=e["ggcn_linear_out_bf16"]) == lr.STAGED
    assert _form(lib, c, entry=e["ggcn_linear_bf16"], x=BASE_X + 1) == -1 and _form(lib, c, entry=e["ggcn_linear_bf16"], y=BASE_Y + 2) == -1
    assert _form(lib, c, entry=e["ggcn_linear_bf16"], x=BASE_X + 2) == lr.ELEM
    assert _form(lib, c, entry=e["ggcn_linear_out_bf16"], x=BASE_X + 2) == -1 and _form(lib, c, entry=e["ggcn_linear_out_bf16"], y=BASE_Y + 2) == lr.STAGED
    # ggcn_linear_scaled: the fast form or nothing
    s = e["ggcn_linear_scaled"]
    assert _form(lib, c, entry=s) == lr.FAST
    for kw in ({"ldx": c.K + 1}, {"ldy": c.F + 1}, {"x": BASE_X + 4}, {"y": BASE_Y + 4}, {"K": 16, "ldx": 32}, {"ldx": lr.LDX_FIRST_SLOW}):
        assert _form(lib, c, entry=s, **kw) == -3, kw
    assert _form(lib, lr.CASES[5], entry=s) == -3                                                    # F = 34


# ---------------------------------------------------------------- the derived gates against the emulated arithmetic
def _emulated():
    seen, out = set(), []
    for c in lr.CASES:
        kind = "fp32" if c.precision == "fp32" else "bx3-half" if lr.half_features(c) else "bx3"
        if c.precision in ("fp32", "bf16x3") and (kind, c.M, c.K, c.F) not in seen:
            seen.add((kind, c.M, c.K, c.F))
            out.append(pytest.param(kind, c, id="%s-%dx%dx%d" % (kind, c.M, c.K, c.F)))
    return out


@pytest.mark.parametrize("kind,c", _emulated())
def test_the_emulated_arithmetic_stays_below_half_the_derived_gate(kind, c):
    """float32 products and sums in k order (fp32), the three bf16 products with float32 sums (bf16x3), rows scaled by 2^-20 ..
    2^20 (2^-3 .. 2^5 for half features: fp16's range): every element below HALF of its gate -- the gates have room for another
    summation order, none to hide a wrong term (test_a_wrong_term_breaks_the_gates)."""
    gen = torch.Generator().manual_seed(c.M % 9973 + c.K + c.F)
    w = lr.weight(c.K, c.F)
    lo, hi = (-3, 5) if kind == "bx3-half" else (-20, 20)
    x = torch.randn(c.M, c.K, generator=gen) * lr.pow2(lr.row_exponents(c.M, lo, hi, "cpu", c.K))[:, None]
    if kind == "bx3-half":
        x = x.half()
    ref, S = lr.statement64(x, w)
    if kind == "fp32":
        r = lr.worst_ratio(lr.emulate_fp32(x, w), ref, lr.gate_fp32(S, c.K) + 1e-300)
    elif kind == "bx3":
        r = lr.worst_ratio(lr.emulate_bx3(x, w), ref, lr.gate_bx3(S, c.K) + 1e-300)
    else:
        # the fp16 store's share of the gate, 2^-11 |ref| + 2^-25, is no estimate with slack: round-to-nearest attains half an
        # ulp, and half an ulp is 2^-11 |ref| just above a power of two.  So the half applies to the float32 sum before the store
        # against the sum's share of the gate, and the stored value has to meet the whole gate.
        acc = lr.emulate_bx3(x, w)
        r = lr.worst_ratio(acc, ref, (2.1 * 2.0 ** -16 + 3 * c.K * lr.U) * S + 1e-300)
        stored = lr.worst_ratio(acc.half(), ref, lr.gate_bx3_half(S, c.K, ref))
        assert stored == stored and stored <= 1.0, stored
    print("%s %dx%dx%d: emulation at %.3f of the gate" % (kind, c.M, c.K, c.F, r))
    # fp32 with K < 8 (the 1 x 1 x 1 and the 8.4 M x 4 x 4 case): K u S is a theorem there and nothing more -- one rounded product
    # attains u |x w| (K = 1), and four roundings over 33 M elements come within a fifth of 4 u S -- so correct arithmetic has to
    # meet the gate, not half of it.  The half is a statement about cancellation in longer sums (sqrt(K) against K).
    assert r == r and r <= (1.0 if kind == "fp32" and c.K < 8 else 0.5), r


def test_a_wrong_term_breaks_the_gates():
    """The gates are not so wide that dropping the lo.hi product, or one k of a sum, passes."""
    c = lr.CASES[0]
    x, w = torch.randn(c.M, c.K, generator=torch.Generator().manual_seed(1)), lr.weight(c.K, c.F)
    ref, S = lr.statement64(x, w)
    (xh, xl), (wh, wl) = lr.split_bf16(x), lr.split_bf16(w)
    no_lo = (xh.double() @ wh.double() + xh.double() @ wl.double()).float()
    assert lr.worst_ratio(no_lo, ref, lr.gate_bx3(S, c.K)) > 10.0
    short = lr.emulate_fp32(x[:, :-1], w[:-1])
    assert lr.worst_ratio(short, ref, lr.gate_fp32(S, c.K)) > 1000.0
