"""The dense head on every staging path against float64, and the other fixed-order tail launches (run with ``-m gpu -s`` on an
MI355X to see the figures; the module prints the worst |logits - ref| / gate per class of width when it finishes).

``ggcn_dense_head`` / ``ggcn_dense_head_signal`` (``csrc/heads.hip``, ``dense_head_kernel``): the cases, the two branch conditions,
the operands and the gates are in ``tests/dense_head_ref.py`` (checked without a GPU by ``tests/test_dense_head_cases_cpu.py``,
which also shows that the gates refuse a lost staging race and a dropped k-slice).  Every case:

* ``pooled`` is a view of a buffer whose pad columns and the row after the last one are NaN (for ``offset`` one element into it);
  ``Wt`` likewise with ``ldw = C + pad_w``; bias and partials are followed directly by NaN; the logits are NaN between two NaN
  guard bands, ``ldl = C + pad_l``;
* the call runs twice: the same bits; every pad column and both guard bands of the logits still NaN; no NaN in the live part;
* both gates, per element, against a float64 product of the same operands taken on the device:
  ``|logits - ref| <= (H + 17) u / (1 - (H + 17) u) * (|p| . |Wt| + |bias|)`` (derived: H FMAs in 16 slices, the slice additions,
  the bias) and the project's ``2e-5 * max(1, max|ref|)``.

Then what staging must not change: the same bits across layouts, a row's bits alone / in any sub-batch / in the full batch (also
for an element-staged and an 8m - 1 width), ``pkg.dense_head`` on ``buf[:, :H]`` views for H = 8m - 1 repeatedly, the final sum
``xy`` at n_part around the 1024-thread stride, the signal words, the refusals with their messages.

``ggcn_colsum``, ``ggcn_transpose`` and ``ggcn_gate_overlap`` follow with padded operands, poisoned workspaces and guarded outputs;
their gates are derived in ``dense_head_ref.py`` too.
"""
import pytest
import torch

import dense_head_ref as dr
from oracle import gates
from oracle.gpu_support import dev, pkg  # noqa: F401

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 64                      # elements of each guard band of an output
CASES = [pytest.param(name, c, id="%s-%s" % (name, dr.case_id(c))) for name, c in dr.CASES]


@pytest.fixture(scope="module")
def report():
    worst = {}
    yield worst
    print("\nworst |logits - ref| / gate per class of width (xy: the final sum's own gate)")
    for key in sorted(worst):
        print("  %-14s %s" % (key, "  ".join("%s: %.3f" % kv for kv in sorted(worst[key].items()))))


def _note(report, name, r):
    slot = report.setdefault(name, {})
    for k, v in r.items():
        slot[k] = max(slot.get(k, 0.0), v)


# ---------------------------------------------------------------- hostile operands
def _rows_view(t, pad, offset=0):
    """t [N,F] (on the device) as a view with row stride F + pad of a NaN buffer with one more row, starting ``offset`` elements
    into the 16-byte aligned buffer."""
    N, F = t.shape
    ld = F + pad
    buf = torch.full(((N + 1) * ld + offset,), NAN, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[offset:].view(-1, ld)[:N, :F]
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * offset
    return v


def _tailed(t):
    """t [n] at the start of a buffer that goes on with NaN, after 8 NaN."""
    buf = torch.full((t.numel() + 72,), NAN, dtype=t.dtype, device=t.device)
    buf[8:8 + t.numel()] = t
    return buf[8:8 + t.numel()]


def _operands(c, dev):
    """((p, wt, bias, part) plain on the device, (pooled view, Wt view, bias, partials) as the case lays them out)."""
    plain = tuple(None if t is None else t.to(dev) for t in dr.operands(c))
    p, wt, bias, part = plain
    return plain, (_rows_view(p, c.pad_p, c.offset), _rows_view(wt, c.pad_w),
                   None if bias is None else _tailed(bias), None if part is None else _tailed(part))


def _launch(pkg, dev, pv, wv, bias, pad_l=0, part=None, f_block=0, signal=None, what=""):
    """One call of the C entry on the views ``pv`` [B,H], ``wv`` [H,C]: (logits [B,C], xy or None).  The logits lie between guard
    bands with ldl = C + pad_l, everything NaN before the call; pads and guards must still be NaN after it, the live part not."""
    from ed_gated_gcn_amd import _capi
    lib, P, st = pkg.load_library(), _capi.ptr, _capi.stream_of(dev)
    (B, H), C = pv.shape, wv.shape[1]
    buf, lv = gates.poisoned_rows(dev, B, C + pad_l, GUARD)
    xyb = torch.full((3,), NAN, device=dev)
    args = (P(pv), pv.stride(0), P(wv), wv.stride(0), P(bias), B, H, C, P(lv), C + pad_l, P(part), f_block,
            P(xyb[1:2]) if part is not None else None)
    if signal is None:
        _capi.check(lib.ggcn_dense_head(*args, st), "ggcn_dense_head")
    else:
        _capi.check(lib.ggcn_dense_head_signal(*args, P(signal), st), "ggcn_dense_head_signal")
    logits = lv[:, :C].clone()
    lv[:, :C] = NAN
    assert bool(torch.isnan(buf).all()), "%s: a pad column or a guard band of the logits was written" % what
    assert not bool(torch.isnan(logits).any()), "%s: NaN in the logits" % what
    xy = None
    if part is not None:
        assert bool(torch.isnan(xyb[0])) and bool(torch.isnan(xyb[2])), "%s: a neighbour of xy was written" % what
        xy = xyb[1].clone()
    return logits, xy


def _run(pkg, dev, c, views, partials=True, signal=None):
    pv, wv, bias, part = views
    part = part if partials else None
    return _launch(pkg, dev, pv, wv, bias, c.pad_l, part, c.n_part_spec if part is not None else 0, signal, dr.case_id(c))


# ---------------------------------------------------------------- the dense head
@pytest.mark.parametrize("name,c", CASES)
def test_dense_head_case_vs_float64_twice(pkg, dev, report, name, c):
    (p, wt, bias, part), views = _operands(c, dev)
    first, xy1 = _run(pkg, dev, c, views)
    second, xy2 = _run(pkg, dev, c, views)
    r = dr.ratios(c, p, wt, bias, first)
    if part is not None:
        r["xy"] = dr.xy_ratio(part, c.B, xy1)
    print("  %s [%s]: %s" % (dr.case_id(c), name, "  ".join("%s %.3f" % kv for kv in sorted(r.items()))))
    _note(report, name, r)
    dr.assert_gates(c, r)
    assert torch.equal(first, second), "%s: two calls, two results" % dr.case_id(c)
    if part is not None:
        assert float(xy1) == float(xy2)


@pytest.mark.parametrize("name", sorted(dr.REQUIRED))
def test_the_same_bits_in_every_layout_of_pooled(pkg, dev, name):
    """Staging only copies: contiguous, padded by 1 / 3 / 4 NaN columns, one element into the buffer."""
    H = dr.REQUIRED[name][-1]
    base = dr.Case(17, H, 34, 0, 0, 0, 0, True, None)
    want = _run(pkg, dev, base, _operands(base, dev)[1])[0]
    seen = set()
    for pad_p, offset in ((1, 0), (3, 0), (4, 0), (0, 1), (3, 1)):
        c = base._replace(pad_p=pad_p, offset=offset)
        seen.add(dr.staging16(c))
        got = _run(pkg, dev, c, _operands(c, dev)[1])[0]
        assert torch.equal(got, want), "%s differs from the contiguous layout" % dr.case_id(c)
    assert seen == ({True, False} if H % 8 == 0 else {False})


@pytest.mark.parametrize("H,pad_p", [(768, 0), (52, 0), (767, 1), (767, 0)])
def test_a_rows_logits_do_not_depend_on_its_batch(pkg, dev, H, pad_p):
    """Alone, in a sub-batch that starts at every offset of an 8-row group, and in the full batch: the same bits (what the sharded
    run compares); 52 stages by elements, 767 with one pad column is the width the 16-byte staging overran."""
    c = dr.Case(24, H, 34, pad_p, 0, 0, 0, True, None)
    _, (pv, wv, bias, _) = _operands(c, dev)
    full = _launch(pkg, dev, pv, wv, bias)[0]
    for r in range(c.B):
        alone = _launch(pkg, dev, pv[r:r + 1], wv, bias)[0]
        assert torch.equal(alone[0], full[r]), "row %d alone" % r
    for s in range(8):
        sub = _launch(pkg, dev, pv[s:s + 11], wv, bias)[0]
        assert torch.equal(sub, full[s:s + 11]), "rows %d..%d as a batch of their own" % (s, s + 10)


@pytest.mark.parametrize("H", [7, 39, 767])
def test_pkg_dense_head_on_views_of_a_padded_buffer(pkg, dev, report, H):
    """``pkg.dense_head(buf[:, :H], wt)`` with ``buf`` [B, H + 1], the pad column NaN: ten calls, each finite and within the gates."""
    c = dr.Case(dr.MANY, H, 34, 1, 0, 0, 0, True, None)
    assert dr.defect_class(c)
    p, wt, bias, _ = (None if t is None else t.to(dev) for t in dr.operands(c))
    buf = torch.full((c.B, H + 1), NAN, device=dev)
    buf[:, :H] = p
    assert buf.data_ptr() % 16 == 0
    for i in range(10):
        logits = pkg.dense_head(buf[:, :H], wt, bias)
        assert bool(torch.isfinite(logits).all()), "call %d: %d elements not finite" % (i, int((~torch.isfinite(logits)).sum()))
        r = dr.ratios(c, p, wt, bias, logits)
        _note(report, "8m-1", r)
        dr.assert_gates(c, r, "call %d" % i)
    print("  %s through pkg.dense_head x10: %s" % (dr.case_id(c), "  ".join("%s %.3f" % kv for kv in sorted(r.items()))))


@pytest.mark.parametrize("c", [c for _, c in dr.CASES if c.n_part_spec], ids=dr.case_id)
def test_the_final_sum_rides_along(pkg, dev, report, c):
    """n_part = 1, 63, 1024, 1025, 6240 floats followed directly by NaN: xy within its derived gate of float64, the same bits
    twice, and logits that are the bits of the call without partials."""
    (p, wt, bias, part), views = _operands(c, dev)
    assert part.numel() == dr.n_part(c)
    logits, xy = _run(pkg, dev, c, views)
    again, xy2 = _run(pkg, dev, c, views)
    r = dr.xy_ratio(part, c.B, xy)
    print("  %s: n_part %d, xy at %.3f of its gate" % (dr.case_id(c), dr.n_part(c), r))
    _note(report, "xy n_part=%d" % dr.n_part(c), {"xy": r})
    assert r == r and r <= 1.0, "xy is %.3f of its gate" % r
    assert float(xy) == float(xy2) and torch.equal(logits, again)
    assert torch.equal(logits, _run(pkg, dev, c, views, partials=False)[0])


@pytest.mark.parametrize("B,f_block", [(5, None), (5, 768), (dr.MANY, 768)], ids=["one-workgroup", "two-workgroups", "many"])
def test_the_signal_words_count_finished_launches(pkg, dev, B, f_block):
    c = dr.Case(B, 96, 34, 0, 0, 0, 0, True, f_block)
    _, views = _operands(c, dev)
    want, want_xy = _run(pkg, dev, c, views)
    signal = torch.zeros(2, dtype=torch.int32, device=dev)
    for n in (1, 2, 3):
        got, xy = _run(pkg, dev, c, views, signal=signal)
        torch.cuda.synchronize()
        assert signal.tolist() == [0, n]
        assert torch.equal(got, want) and (xy is None) == (want_xy is None) and (xy is None or float(xy) == float(want_xy))


def test_refusals_and_their_messages(pkg, dev):
    from ed_gated_gcn_amd import _capi
    lib, P, st = pkg.load_library(), _capi.ptr, _capi.stream_of(dev)
    p, wt, out = torch.zeros(8, 1025, device=dev), torch.zeros(1025, 65, device=dev), torch.full((8, 65), NAN, device=dev)
    part, xy = torch.zeros(64, device=dev), torch.full((1,), NAN, device=dev)

    def refused(msg, B=8, H=64, C=34, ldp=1025, ldw=65, ldl=65, partials=None, f_block=0, xy_=None):
        rc = lib.ggcn_dense_head(P(p), ldp, P(wt), ldw, None, B, H, C, P(out), ldl, P(partials), f_block, P(xy_), st)
        err = lib.ggcn_last_error().decode()
        assert rc != 0 and msg in err, (rc, err)

    refused("at most 64", C=65)
    refused("needs more than 64 KiB of LDS", H=1025)
    for kw in ({"ldp": 63}, {"ldw": 33}, {"ldl": 33}):
        refused("leading dimension too small", **kw)
    refused("overlap_partials and xy go together", partials=part, f_block=64)
    refused("overlap_partials and xy go together", xy_=xy)
    assert lib.ggcn_dense_head_signal(P(p), 1025, P(wt), 65, None, 8, 64, 34, P(out), 65, None, 0, None, None, st) != 0
    assert "null signal words" in lib.ggcn_last_error().decode()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(xy).all())          # nothing was launched
    with pytest.raises(RuntimeError, match="at most 64"):
        pkg.dense_head(p[:, :64], wt[:64])
    with pytest.raises(RuntimeError, match="64 KiB of LDS"):
        pkg.dense_head(p, wt[:, :34])
    # the widest width that fits, for comparison, is accepted
    assert lib.ggcn_dense_head(P(p), 1025, P(wt), 65, None, 8, 1024, 64, P(out), 65, None, 0, None, st) == 0
    torch.cuda.synchronize()
    assert bool((out[:, :64] == 0).all()) and bool(torch.isnan(out[:, 64]).all())


# ---------------------------------------------------------------- the other fixed-order tail launches
def _guarded(dev, n):
    buf = torch.full((n + 2 * GUARD,), NAN, device=dev)
    return buf, buf[GUARD:GUARD + n]


@pytest.mark.parametrize("M", dr.COLSUM_M)
def test_colsum_vs_float64(pkg, dev, M):
    """ld = F + 3 with NaN pads, a poisoned workspace, an output of NaN between guard bands; M = 65 and 129 leave trailing slabs of
    the 64-slab plan empty.  ``M u / (1 - M u) * sum_r |x_rf|``; the same bits twice."""
    from ed_gated_gcn_amd import _capi
    lib, P, st = pkg.load_library(), _capi.ptr, _capi.stream_of(dev)
    for F in dr.COLSUM_F:
        x = torch.randn(M, F, generator=torch.Generator().manual_seed(31 * M + F)).to(dev)
        xv = _rows_view(x, 3)
        outs = []
        for _ in range(2):
            ws = gates.poisoned(lib.ggcn_colsum_workspace_bytes(F), dev)
            buf, out = _guarded(dev, F)
            _capi.check(lib.ggcn_colsum(P(xv), F + 3, M, F, P(out), P(ws), st), "ggcn_colsum")
            outs.append(out.clone())
            out.fill_(NAN)
            assert bool(torch.isnan(buf).all()), "M=%d F=%d: a guard band was written" % (M, F)
        r = dr.colsum_ratio(x, outs[0])
        print("  colsum %d x %d: %.3f of the gate" % (M, F, r))
        assert r == r and r <= 1.0, "colsum %d x %d: %.3f of the gate" % (M, F, r)
        assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("rows", dr.TRANSPOSE_N)
def test_transpose_is_bit_exact(pkg, dev, rows):
    from ed_gated_gcn_amd import _capi
    lib, P, st = pkg.load_library(), _capi.ptr, _capi.stream_of(dev)
    for cols in dr.TRANSPOSE_N:
        w = torch.randn(rows, cols, generator=torch.Generator().manual_seed(rows + 7 * cols)).to(dev)
        wv = _rows_view(w, 3)
        buf, out = gates.poisoned_rows(dev, cols, rows, GUARD)
        _capi.check(lib.ggcn_transpose(P(wv), rows, cols, cols + 3, P(out), st), "ggcn_transpose")
        assert torch.equal(out, w.t()), "%d x %d" % (rows, cols)
        out.fill_(NAN)
        assert bool(torch.isnan(buf).all()), "%d x %d: a guard band was written" % (rows, cols)


@pytest.mark.parametrize("B", dr.OVERLAP_B)
def test_gate_overlap_vs_float64(pkg, dev, B):
    """A length-F FMA dot product per row plus the length-B sum and the division: ``(F + B) u / (1 - (F + B) u) * sum|x1 y1| / B``;
    a poisoned workspace, NaN after the operands' last row and around xy; the same bits twice."""
    from ed_gated_gcn_amd import _capi
    lib, P, st = pkg.load_library(), _capi.ptr, _capi.stream_of(dev)
    for F in dr.OVERLAP_F:
        gen = torch.Generator().manual_seed(B + 3 * F)
        x1, y1 = torch.randn(B, F, generator=gen).to(dev), torch.randn(B, F, generator=gen).to(dev)
        xv, yv = _rows_view(x1, 0), _rows_view(y1, 0)
        got = []
        for _ in range(2):
            ws = gates.poisoned(lib.ggcn_overlap_workspace_bytes(B), dev)
            xyb = torch.full((3,), NAN, device=dev)
            _capi.check(lib.ggcn_gate_overlap(P(xv), P(yv), B, F, P(xyb[1:2]), P(ws), st), "ggcn_gate_overlap")
            assert bool(torch.isnan(xyb[0])) and bool(torch.isnan(xyb[2]))
            got.append(float(xyb[1]))
        r = dr.overlap_ratio(x1, y1, got[0])
        print("  gate_overlap %d x %d: %.3f of the gate" % (B, F, r))
        assert r == r and r <= 1.0, "gate_overlap %d x %d: %.3f of the gate" % (B, F, r)
        assert got[0] == got[1]
