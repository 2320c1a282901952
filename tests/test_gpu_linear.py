"""The forward linear on every kernel form against float64 (run with ``-m gpu -s`` on an MI355X to see the figures; the module
prints the worst |y - ref| / gate per (entry, precision, form) when it finishes: ``profiles/linear_gates.txt`` is that table).

Entries: ``ggcn_linear`` at fp32 / bf16x3 / f16mx8, ``ggcn_linear_h`` at bf16x3 / f16mx8 / f16, ``ggcn_linear_scaled``.  The cases,
the form each must take and the gates are in ``tests/linear_ref.py`` (checked without a GPU by ``tests/test_linear_cases_cpu.py``).
Every case, as ``tests/test_gpu_backward.py`` does for the backward's GEMMs:

* X is a view of a buffer whose pad columns and the row after the last one are NaN; W (fp32, and what ``ggcn_weight_pack`` reads)
  likewise with ``ldw = width + pad``; Y is NaN between two NaN guard bands;
* ``ggcn_linear_form`` must name the case's form for the real pointers -- the launchers dispatch on the same function, so a
  fall-back to the element-load form fails here;
* the call runs twice: same bits; every pad column and both guard bands of Y still NaN; no NaN in the live part;
* every gate that applies, per element, against a float64 product of the same operands taken on the device.

Gates, and where each comes from (``linear_ref.py`` has the derivations):

* fp32: ``|y - ref| <= K u / (1 - K u) * S`` with ``S = |X| . |W|``, ``u = 2^-24`` -- the bound of a K-long fp32 dot product.
* bf16x3: ``(3.1 * 2^-16 + 3 K * 2^-24) * S``; half features ``(2.1 * 2^-16 + 3 K * 2^-24) * S + 2^-11 |ref| + 2^-25`` (the fp16
  store).  Derived from the two-term bf16 split and three fp32 accumulations.
* the project's own: ``test_linear_vs_float64``'s matrix gate 1e-5 / 3e-5 / 6e-5 * max(1, sqrt(K) rms(x) rms(w)) (float features),
  ``test_f16_linear_for_half_features``' 6e-4 / 2e-3 * max(1, max|ref|) (half features), ggcn_linear_scaled's 6e-5 * max|ref|.
  f16mx8 and f16 have only these, on rows scaled by 2^-3 .. 2^5 and taken per class of rows of one scale; f16mx8's
  ``err / (2^-15 S)`` is printed, not asserted (the header's 2^-15 is relative to a 32-k block's largest weight).
* f16mx8: ``ggcn_range_flag`` reads 0 after the pack and after the call, and the case runs once more with +inf for NaN in the
  pads of X and W: a pad element taken into the running maximum raises GGCN_RANGE_OVERFLOW even where the product hides it.  The
  +inf run must give the NaN run's bits.
* fp32 and bf16x3 (float features): ``Y(diag(2^k) X) == diag(2^k) Y(X)`` bit for bit, k in -20 .. 20 per row -- every step is an
  IEEE rounding and a power of two shifts all exponents of a row alike, nothing near underflow: the matrix gate holds for rows of
  every magnitude.
* weight images: ``ggcn_weight_pack`` of W and of W^T stored [F,K] with ``transposed = 1`` give the same bytes (both NaN-padded,
  ldw = width + 3), the f16mx8 trailers' float[0] (two reduction orders) agree to 1e-6 relative and are finite.
"""
import pytest
import torch

import linear_ref as lr
from oracle import gates
from oracle.gpu_support import clean_range_flag, dev, pkg, range_bits  # noqa: F401

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
GUARD = 64                      # elements of each guard band of Y (a multiple of 8: the view stays 16-byte aligned)
WIDE_PAD = 4096                 # beyond this pad X is allocated empty and only the columns next to the live ones are filled
_PACKS = {}


@pytest.fixture(autouse=True)
def clean_flag(pkg, dev):
    yield from clean_range_flag(pkg, dev)


@pytest.fixture(scope="module")
def report():
    worst = {}
    yield worst
    print("\nworst |y - ref| / gate per (entry, precision, form); 'vs 2^-15 S' is a figure, not a gate")
    for key in sorted(worst):
        print("  %-18s %-7s %-15s %s" % (key + ("  ".join("%s: %.3f" % kv for kv in sorted(worst[key].items())),)))


def _note(report, c, r):
    slot = report.setdefault((c.entry, c.precision, lr.form_name(c)), {})
    for k, v in r.items():
        slot[k] = max(slot.get(k, 0.0), v)


def _x_view(c, x, fill):
    """x [M,K] as a [M,K] view with row stride K + pad_x of a buffer with one more row, everything outside the view ``fill``."""
    M, K, ld = c.M, c.K, c.K + c.pad_x
    off = 1 if c.offset == lr.OFF_X else 0
    if c.pad_x > WIDE_PAD:      # the 1 GB stride: only the live columns, the eight behind them and the spare row's start are written
        buf = torch.empty((M + 1) * ld, dtype=x.dtype, device=x.device)
        v = buf.view(M + 1, ld)
        v[:, K:K + 8] = fill
        v[M, :K] = fill
    else:
        buf = torch.full(((M + 1) * ld + off,), fill, dtype=x.dtype, device=x.device)
        v = buf[off:].view(M + 1, ld)
    v[:M, :K] = x
    assert buf.data_ptr() % 16 == 0
    return v[:M, :K]


def _weights(pkg, dev, c, fill=NAN, transposed=False):
    """(W [K,F] on the device, the fp32 operand view or None, its ldw, the packed image or None): fp32 reads W as a view of a
    ``fill``-padded buffer with ldw = F + pad_w; the other precisions read an image packed from a ``fill``-padded W with
    ldw = width + 3 (from W^T stored [F,K] with ``transposed``), made once per (K, F, precision, fill, transposed)."""
    from ed_gated_gcn_amd import _capi
    w = lr.weight(c.K, c.F).to(dev)
    if c.precision == "fp32":
        return w, gates.hostile(w, c.pad_w, fill)[:c.K, :c.F], c.F + c.pad_w, None
    key = (c.K, c.F, c.precision, fill != fill, transposed)
    if key not in _PACKS:
        lib, prec = pkg.load_library(), _capi.PREC[c.precision]
        stored = gates.hostile(w.t().contiguous() if transposed else w, 3, fill)
        pack = gates.poisoned(lib.ggcn_weight_pack_bytes(c.K, c.F, prec), dev)
        _capi.check(lib.ggcn_weight_pack(_capi.ptr(stored), stored.shape[1], c.K, c.F, prec, 1 if transposed else 0, _capi.ptr(pack),
                                         _capi.stream_of(dev)), "ggcn_weight_pack")
        if c.precision == "f16mx8":
            assert range_bits(pkg, dev) == 0, "ggcn_weight_pack raised the range flag on %s-padded weights" % fill
        _PACKS[key] = pack
    return w, None, 0, _PACKS[key]


def _run(pkg, dev, c, x, fill=NAN, transposed=False, amax=None):
    """The case's call on x, twice, in hostile buffers: the form, same bits, pads and guard bands untouched, no NaN.  Returns
    (w, y [M,F])."""
    from ed_gated_gcn_amd import _capi
    lib, P, st = pkg.load_library(), _capi.ptr, _capi.stream_of(dev)
    w, wv, ldw, pack = _weights(pkg, dev, c, fill, transposed)
    xv = _x_view(c, x, fill)
    ldx, ldy, prec = c.K + c.pad_x, c.F + c.pad_y, _capi.PREC[c.precision]
    guard = GUARD + (1 if c.offset == lr.OFF_Y else 0)
    what = "%s (pads %s)" % (lr.case_id(c), fill)
    outs = []
    for _ in range(2):
        buf, yv = gates.poisoned_rows(dev, c.M, ldy, guard, dtype=x.dtype)
        assert buf.data_ptr() % 16 == 0
        form = lib.ggcn_linear_form(_capi.LINEAR_ENTRY[c.entry], P(xv), ldx, P(wv), ldw, P(yv), ldy, c.M, c.K, c.F, prec)
        assert form == c.form, "%s: ggcn_linear_form says %d, the case %d" % (what, form, c.form)
        if c.entry == lr.LINEAR:
            rc = lib.ggcn_linear(P(xv), ldx, P(wv), ldw, P(pack), P(yv), ldy, c.M, c.K, c.F, prec, st)
        elif c.entry == lr.LINEAR_H:
            rc = lib.ggcn_linear_h(P(xv), ldx, P(pack), P(yv), ldy, c.M, c.K, c.F, prec, st)
        else:
            rc = lib.ggcn_linear_scaled(P(xv), ldx, P(pack), P(yv), ldy, c.M, c.K, c.F, P(amax), st)
        _capi.check(rc, c.entry)
        y = yv[:, :c.F].clone()
        yv[:, :c.F] = NAN
        assert bool(torch.isnan(buf).all()), "%s: a pad column or a guard band of Y was written" % what
        assert not bool(torch.isnan(y).any()), "%s: NaN in the result" % what
        outs.append(y)
    assert torch.equal(outs[0], outs[1]), "%s: two calls, two results" % what
    if c.precision == "f16mx8":
        bits = range_bits(pkg, dev)
        assert bits == 0, "%s: range flag %d" % (what, bits)
    return w, outs[0]


def _judge(report, c, x, w, y, classes, what=""):
    r = lr.ratios(c, x, w, y, classes)
    print("  %s [%s]%s: %s" % (lr.case_id(c), lr.form_name(c), what, "  ".join("%s %.3f" % kv for kv in sorted(r.items()))))
    _note(report, c, r)
    lr.assert_gates(c, r, what)


@pytest.mark.parametrize("c", [c for c in lr.CASES if c.entry != lr.SCALED], ids=lr.case_id)
def test_linear_case_vs_float64(pkg, dev, report, c):
    x, classes = lr.features(c, dev)
    w, y = _run(pkg, dev, c, x)
    _judge(report, c, x, w, y, classes)
    if c.precision == "f16mx8":
        _, y_inf = _run(pkg, dev, c, x, fill=INF)
        assert torch.equal(y, y_inf), "%s: +inf pads change the result" % lr.case_id(c)


@pytest.mark.parametrize("scale", lr.SCALED_SCALES)
@pytest.mark.parametrize("c", [c for c in lr.CASES if c.entry == lr.SCALED], ids=lr.case_id)
def test_scaled_linear_case_vs_float64(pkg, dev, report, c, scale):
    x = lr.features(c, dev)[0] * scale
    amax = x.abs().max().reshape(1).contiguous()
    w, y = _run(pkg, dev, c, x, amax=amax)
    _judge(report, c, x, w, y, None, " scale %g" % scale)
    _, y_inf = _run(pkg, dev, c, x, fill=INF, amax=amax)
    assert torch.equal(y, y_inf), "%s: +inf pads change the result" % lr.case_id(c)


@pytest.mark.parametrize("c", [c for c in lr.CASES if c.entry == lr.LINEAR and c.precision in ("fp32", "bf16x3")], ids=lr.case_id)
def test_rows_scaled_by_powers_of_two_scale_their_results_exactly(pkg, dev, c):
    x, _ = lr.features(c, dev)
    k = lr.row_exponents(c.M, -20, 20, dev, c.M + c.F)
    _, y = _run(pkg, dev, c, x)
    two_k = lr.pow2(k)[:, None]                      # exact powers of two: both products below are exact
    _, y_scaled = _run(pkg, dev, c, x * two_k)
    want = y * two_k
    differ = y_scaled != want
    assert not bool(differ.any()), "%s: %d elements of Y(2^k X) are not 2^k Y(X), first in row %d" % (
        lr.case_id(c), int(differ.sum()), int(torch.nonzero(differ)[0, 0]))


KF_PAIRS = sorted({(c.K, c.F) for c in lr.CASES if c.precision in ("bf16x3", "f16mx8")})


@pytest.mark.parametrize("precision", ["bf16x3", "f16mx8"])
def test_weight_images_of_w_and_of_its_stored_transpose(pkg, dev, precision):
    from ed_gated_gcn_amd import _capi
    lib = pkg.load_library()
    trailer = 16 if precision == "f16mx8" else 0        # bf16x3's image has none
    for K, F in KF_PAIRS:
        c = lr.Case(lr.LINEAR, precision, 1, K, F, 0, 0, 0, 0, 0)
        plain, turned = _weights(pkg, dev, c)[3], _weights(pkg, dev, c, transposed=True)[3]
        n = lib.ggcn_weight_pack_bytes(K, F, _capi.PREC[precision])
        assert torch.equal(plain[:n - trailer], turned[:n - trailer]), "%s %dx%d: the two images differ" % (precision, K, F)
        if trailer:
            a, b = (float(p[n - 16:n - 12].view(torch.float32)) for p in (plain, turned))
            w = lr.weight(K, F).double()
            assert a == a and b == b and abs(a) != INF and abs(b) != INF, (K, F, a, b)
            assert abs(a - b) <= 1e-6 * abs(a), "%dx%d: trailers %.9g and %.9g" % (K, F, a, b)
            assert abs(a - float(w.abs().sum(0).max())) <= 1e-5 * abs(a), (K, F, a)      # what it states: max_f sum_k |w[k,f]|


@pytest.mark.parametrize("c", [c for c in lr.CASES if c.entry == lr.LINEAR and c.precision in ("bf16x3", "f16mx8")
                               and (c.M, c.K, c.F) in ((129, 32, 36), (129, 33, 36)) and not (c.pad_x or c.pad_y or c.offset)],
                         ids=lr.case_id)
def test_linear_case_through_the_transposed_image(pkg, dev, report, c):
    x, classes = lr.features(c, dev)
    w, y = _run(pkg, dev, c, x, transposed=True)
    _judge(report, c, x, w, y, classes, " W^T image")
    assert torch.equal(y, _run(pkg, dev, c, x)[1])
