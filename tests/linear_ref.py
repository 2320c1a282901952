"""THE CASES AND GATES OF THE FORWARD LINEAR'S SWEEP (test infrastructure, NOT product code; no GPU needed to import).

``tests/test_linear_cases_cpu.py`` checks the table against ``ggcn_linear_form`` and the derived gates against an emulation of the
arithmetic; ``tests/test_gpu_linear.py`` runs every case on the device.  Pure torch: every function here takes CPU and device
tensors alike.

A case is ``Case(entry, precision, M, K, F, pad_x, pad_y, pad_w, offset, form)``: ``Y [M,F] = X [M,K] . W [K,F]`` through ``entry``
with ``ldx = K + pad_x``, ``ldy = F + pad_y`` and (fp32 alone: the other precisions read a packed image) ``ldw = F + pad_w``;
``offset`` is ``OFF_X`` / ``OFF_Y`` when that view starts ONE element into its buffer (rows aligned to the element size only);
``form`` is the set of ``ggcn_linear_form_bits`` the launcher must take for 16-byte aligned buffers.

Tile geometry the shapes are chosen against: split kernels 128 rows x 256 columns per workgroup (four wavefronts of 64 columns),
32 k per stage, 16-byte X loads for K, ldx multiples of 4 (float) / 8 (half); fp16 kernel 64 k per stage; fp32 kernel 128 x 128,
16 k per stage.

Gates (``S_ij = sum_k |x_ik| |w_kj|`` and ``ref`` in float64; every element must meet every gate that applies):

* fp32: ``|y - ref| <= K u / (1 - K u) * S``, ``u = 2^-24`` -- the standard bound of a length-K fp32 dot product (K rounded
  products, K - 1 rounded sums) in any order.
* bf16x3, float features: ``(3.1 * 2^-16 + 3 K * 2^-24) * S``.  A bf16 keeps 8 significant bits, so hi + lo leaves at most 2^-16 of
  each operand (x and w: 2 * 2^-16, their product 2^-32), the dropped lo.lo term at most 2^-16 of the product (together
  < 3.1 * 2^-16); products of two bf16 are exact in fp32, and three K-long fp32 accumulations add 3 K u.
* bf16x3, half features: an fp16 value splits into hi + lo exactly, so the operand term is w's alone: ``2.1 * 2^-16`` for
  3.1 * 2^-16; the fp16 store adds ``2^-11 |ref| + 2^-25`` (half an ulp of a normal / of a subnormal fp16; the rounding of the
  float32 sum itself, <= 2^-11 of an error already counted, disappears in the .1).
* the project's own: the matrix gate of ``test_linear_vs_float64`` (1e-5 / 3e-5 / 6e-5 * max(1, sqrt(K) rms(x) rms(w))) for float
  features, the 6e-4 / 2e-3 * max(1, max|ref|) gates of ``test_f16_linear_for_half_features`` for half features (6e-4 against the
  product with the weights the kernel multiplies -- fp16-rounded for precision f16 -- and 2e-3 against the float32 weights), and
  ggcn_linear_scaled's 6e-5 * max|ref|.  f16mx8 and f16 have only these: the header's "~2^-15 per product" is relative to a 32-k
  block's largest weight, not to each product (the figure ``vs 2^-15 S`` of ``ratios`` is printed, never asserted).

Operands: ``W`` xavier-uniform (``synth.layer_params``), ``X ~ N(0,1)``.  f16mx8 and f16 run on X whose rows are additionally scaled
by powers of two in 2^-3 .. 2^5 (inside the 2^-9 .. 448 window of the fixed-scale fp8 correction); their max-abs gates are then
taken per CLASS of rows of one scale -- the sub-matrix of those rows times W is a linear call of its own (rows never mix), and the
project's gate is a statement about such a call -- so the small rows are not judged by the large rows' magnitude.
"""
import collections
import math

import torch

Case = collections.namedtuple("Case", "entry precision M K F pad_x pad_y pad_w offset form")
OFF_X, OFF_Y = 1, 2
XVEC, KFULL, VST, WVEC = 1, 2, 4, 8           # include/ggcn.h ggcn_linear_form_bits
FAST, STAGED, VEC, ELEM = XVEC | KFULL | VST, XVEC | KFULL, XVEC, 0
LINEAR, LINEAR_H, SCALED = "ggcn_linear", "ggcn_linear_h", "ggcn_linear_scaled"
U = 2.0 ** -24
ROW_TILES_MAX = 65535                          # linear_fp32 walks the rows in slices of this many 128-row tiles
# ldx * sizeof(float) * 257 < 2^31 keeps the 16-byte X loads: 2088988 is the largest multiple of 4 that does, 2088992 the first that
# does not.  (2089004 / 2089008, the pair the issue behind this sweep named as the boundary, both lie beyond it:
# 2089004 * 4 * 257 = 2^31 + 12464.  They stay in the table as element-load cases.)
LDX_LAST_FAST, LDX_FIRST_SLOW, LDX_BEYOND = 2088988, 2088992, (2089004, 2089008)
assert LDX_LAST_FAST * 4 * 257 < 2 ** 31 <= LDX_FIRST_SLOW * 4 * 257


def _c(entry, precision, M, K, F, form, pad_x=0, pad_y=0, pad_w=0, offset=0):
    return Case(entry, precision, M, K, F, pad_x, pad_y, pad_w, offset, form)


def _split_float(p):
    big = (129, 64, 64)
    return [
        # 16-byte loads, whole stages, staged stores: a second row tile of one row, a second 32-column tile of 4 live columns,
        # wavefronts 1..3 past F; one row; ten row tiles (tile_of_block returns early for six block ids) and two column
        # workgroups, the second with 4 live columns
        _c(LINEAR, p, 129, 32, 36, FAST), _c(LINEAR, p, 1, 64, 4, FAST), _c(LINEAR, p, 1153, 96, 260, FAST),
        _c(LINEAR, p, 129, 32, 36, FAST, pad_x=4, pad_y=4), _c(LINEAR, p, 1153, 96, 260, FAST, pad_x=4, pad_y=4),
        # ... guarded element stores
        _c(LINEAR, p, 129, 32, 34, STAGED), _c(LINEAR, p, 128, 64, 33, STAGED), _c(LINEAR, p, 129, 32, 36, STAGED, pad_y=1),
        _c(LINEAR, p, 129, 32, 36, STAGED, offset=OFF_Y),
        # ... a partial last stage
        _c(LINEAR, p, 130, 36, 68, VEC), _c(LINEAR, p, 127, 100, 31, VEC),
        # element loads
        _c(LINEAR, p, 129, 33, 36, ELEM), _c(LINEAR, p, 7, 1, 1, ELEM), _c(LINEAR, p, 33, 17, 5, ELEM), _c(LINEAR, p, 128, 31, 256, ELEM),
        _c(LINEAR, p, 129, 32, 36, ELEM, pad_x=3), _c(LINEAR, p, 129, 32, 36, ELEM, offset=OFF_X),
        # the 32-bit row-offset limit of the fast forms: row 128 about 1.07e9 bytes from row 0
        _c(LINEAR, p, *big, FAST, pad_x=LDX_LAST_FAST - 64), _c(LINEAR, p, *big, ELEM, pad_x=LDX_FIRST_SLOW - 64),
        _c(LINEAR, p, *big, ELEM, pad_x=LDX_BEYOND[0] - 64), _c(LINEAR, p, *big, ELEM, pad_x=LDX_BEYOND[1] - 64),
    ]


def _split_half(p):
    return [_c(LINEAR_H, p, 129, 32, 36, STAGED), _c(LINEAR_H, p, 130, 40, 68, VEC), _c(LINEAR_H, p, 33, 36, 5, ELEM),
            _c(LINEAR_H, p, 129, 32, 36, ELEM, pad_x=4), _c(LINEAR_H, p, 129, 32, 36, STAGED, pad_x=8, pad_y=1)]


CASES = (
    _split_float("bf16x3") + _split_float("f16mx8") + _split_half("bf16x3") + _split_half("f16mx8")
    + [_c(LINEAR_H, "f16", 129, 64, 36, STAGED), _c(LINEAR_H, "f16", 129, 96, 36, VEC), _c(LINEAR_H, "f16", 33, 36, 5, ELEM),
       _c(LINEAR_H, "f16", 129, 64, 36, ELEM, pad_x=4)]
    + [_c(LINEAR, "fp32", 129, 16, 132, XVEC | WVEC), _c(LINEAR, "fp32", 129, 20, 130, XVEC), _c(LINEAR, "fp32", 130, 17, 132, WVEC),
       _c(LINEAR, "fp32", 33, 17, 5, ELEM), _c(LINEAR, "fp32", 1, 1, 1, ELEM),
       _c(LINEAR, "fp32", 5, 15, 8, WVEC), _c(LINEAR, "fp32", 5, 16, 8, XVEC | WVEC), _c(LINEAR, "fp32", 5, 17, 8, WVEC),
       _c(LINEAR, "fp32", 129, 16, 132, XVEC | WVEC, pad_w=4), _c(LINEAR, "fp32", 129, 16, 132, XVEC, pad_w=3),
       _c(LINEAR, "fp32", 1, 768, 768, XVEC | WVEC),                           # b1.W2 of the folded block
       _c(LINEAR, "fp32", ROW_TILES_MAX * 128 + 5, 4, 4, XVEC | WVEC)]          # the launcher's second slice: five rows
    + [_c(SCALED, "f16mx8", 129, 32, 36, FAST, pad_x=4, pad_y=4), _c(SCALED, "f16mx8", 1153, 96, 260, FAST, pad_x=4, pad_y=4)]
)
SCALED_SCALES = (1.0, 3e-9)

# every form each launcher can pick: {(entry, precision): the forms the table must reach}
FORMS = {(LINEAR, "bf16x3"): {FAST, STAGED, VEC, ELEM}, (LINEAR, "f16mx8"): {FAST, STAGED, VEC, ELEM},
         (LINEAR_H, "bf16x3"): {STAGED, VEC, ELEM}, (LINEAR_H, "f16mx8"): {STAGED, VEC, ELEM}, (LINEAR_H, "f16"): {STAGED, VEC, ELEM},
         (LINEAR, "fp32"): {XVEC | WVEC, XVEC, WVEC, ELEM}, (SCALED, "f16mx8"): {FAST}}
FORM_NAMES = {FAST: "xvec+kfull+vst", STAGED: "xvec+kfull", VEC: "xvec", ELEM: "elem", XVEC | WVEC: "xvec+wvec", WVEC: "wvec"}


def case_id(c):
    s = "%s-%s-%dx%dx%d" % (c.entry[5:], c.precision, c.M, c.K, c.F)
    for name, v in (("px", c.pad_x), ("py", c.pad_y), ("pw", c.pad_w)):
        s += "-%s%d" % (name, v) if v else ""
    return s + {0: "", OFF_X: "-xoff", OFF_Y: "-yoff"}[c.offset]


def form_name(c):
    return FORM_NAMES[c.form]


def half_features(c):
    return c.entry == LINEAR_H


def row_scaled(c):
    """The precisions whose operands carry per-row powers of two (module docstring)."""
    return c.precision in ("f16mx8", "f16") and c.entry != SCALED


def pointer_offsets(c):
    """Byte offsets (X, Y) of the two views from a 16-byte boundary."""
    size = 2 if half_features(c) else 4
    return (size if c.offset == OFF_X else 0), (size if c.offset == OFF_Y else 0)


# ---------------------------------------------------------------- operands
def weight(K, F, seed=3):
    """W [K,F] float32 on the CPU: xavier-uniform, the operand of test_linear_vs_float64."""
    from ed_gated_gcn_amd import synth
    return torch.from_numpy(synth.layer_params(K, F, seed=seed)[0])


def row_exponents(M, lo, hi, device, seed):
    """One integer in lo .. hi per row, the extremes present from two rows up."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    k = torch.randint(lo, hi + 1, (M,), generator=gen)
    if M >= 2:
        k[0], k[-1] = hi, lo
    return k.to(device)


def pow2(k):
    """2^k as float32, exactly (from the bit pattern: a device's pow may be an ulp off), k integers in -126 .. 127."""
    return ((k.to(torch.int32) + 127) << 23).view(torch.float32)


def features(c, device):
    """(X [M,K] float32 or float16, the row classes {exponent: row indices} or None)."""
    gen = torch.Generator(device=device).manual_seed(c.M % 9973 + 7 * c.K + 13 * c.F)
    x = torch.randn(c.M, c.K, device=device, generator=gen)
    classes = None
    if row_scaled(c):
        k = row_exponents(c.M, -3, 5, device, c.M + c.K)
        x = x * pow2(k)[:, None]
        classes = {int(e): torch.nonzero(k == e)[:, 0] for e in torch.unique(k).tolist()}
    return (x.half() if half_features(c) else x), classes


# ---------------------------------------------------------------- the float64 statement and the gates
def statement64(x, w):
    """(ref, S) = (X . W, |X| . |W|) in float64 on x's device."""
    x64, w64 = x.double(), w.double().to(x.device)
    return x64 @ w64, x64.abs() @ w64.abs()


def gate_fp32(S, K):
    return K * U / (1.0 - K * U) * S


def gate_bx3(S, K):
    return (3.1 * 2.0 ** -16 + 3 * K * U) * S


def gate_bx3_half(S, K, ref):
    return (2.1 * 2.0 ** -16 + 3 * K * U) * S + 2.0 ** -11 * ref.abs() + 2.0 ** -25


MATRIX_TOL = {"fp32": 1e-5, "bf16x3": 3e-5, "f16mx8": 6e-5}


def matrix_gate(x, w, precision):
    """test_linear_vs_float64's: tol * max(1, sqrt(K) * rms(x) * rms(w)), one number for the matrix."""
    K = x.shape[1]
    scale = math.sqrt(K) * math.sqrt(float((x.double() ** 2).mean()) * float((w.double() ** 2).mean()))
    return MATRIX_TOL[precision] * max(1.0, scale)


def worst_ratio(y, ref, bound):
    """max |y - ref| / bound over the elements (bound: a tensor or a number, > 0); NaN if y holds one."""
    r = (y.double() - ref).abs() / bound
    return float("nan") if bool(torch.isnan(r).any()) else float(r.max())


def ratios(c, x, w, y, classes=None):
    """{gate name: worst |y - ref| / gate} of every gate that applies to case ``c`` (module docstring), plus the figure
    ``vs 2^-15 S`` (f16mx8 alone; reported, not a gate).  x, y on one device; w anywhere."""
    ref, S = statement64(x, w)
    out = {}
    if c.entry == SCALED:
        out["6e-5 max|ref|"] = worst_ratio(y, ref, 6e-5 * float(ref.abs().max()))
    elif c.precision == "fp32":
        out["K u S"] = worst_ratio(y, ref, gate_fp32(S, c.K) + 1e-300)
    elif c.precision == "bf16x3":
        out["2^-16 S"] = worst_ratio(y, ref, gate_bx3_half(S, c.K, ref) if half_features(c) else gate_bx3(S, c.K) + 1e-300)
    groups = [torch.arange(c.M, device=x.device)] if classes is None else list(classes.values())
    if c.entry == LINEAR:
        out["matrix"] = max(worst_ratio(y[g], ref[g], matrix_gate(x[g], w, c.precision)) for g in groups)
    elif c.entry == LINEAR_H:
        if c.precision == "f16":
            tight = x.double() @ w.half().double().to(x.device)
            out["6e-4"] = max(worst_ratio(y[g], tight[g], 6e-4 * max(1.0, float(ref[g].abs().max()))) for g in groups)
            out["2e-3"] = max(worst_ratio(y[g], ref[g], 2e-3 * max(1.0, float(ref[g].abs().max()))) for g in groups)
        else:
            out["6e-4"] = max(worst_ratio(y[g], ref[g], 6e-4 * max(1.0, float(ref[g].abs().max()))) for g in groups)
    if c.precision == "f16mx8" and c.entry == LINEAR:
        out["vs 2^-15 S"] = worst_ratio(y, ref, 2.0 ** -15 * S + 1e-300)
    return out


REPORTED_ONLY = ("vs 2^-15 S",)


def assert_gates(c, r, what=""):
    for name, v in r.items():
        if name not in REPORTED_ONLY:
            assert v == v and v <= 1.0, "%s %s: |y - ref| is %.3f of the gate '%s'" % (case_id(c), what, v, name)


# ---------------------------------------------------------------- the arithmetic, emulated (tests/test_linear_cases_cpu.py)
def emulate_fp32(x, w):
    """A k-ordered float32 chain: every product and every sum rounded to float32."""
    acc = torch.zeros(x.shape[0], w.shape[1], dtype=torch.float32)
    for k in range(x.shape[1]):
        acc = acc + x[:, k, None] * w[None, k, :]
    return acc


def split_bf16(v):
    hi = v.float().bfloat16().float()
    return hi, (v.float() - hi).bfloat16().float()


def emulate_bx3(x, w, half=False):
    """hi.hi + lo.hi + hi.lo on the bf16 hi/lo parts (bf16 x bf16 is exact in float32), every sum in float32; half features: x is
    float16 and the result is rounded to float16."""
    (xh, xl), (wh, wl) = split_bf16(x), split_bf16(w)
    acc = torch.zeros(x.shape[0], w.shape[1], dtype=torch.float32)
    for k in range(x.shape[1]):
        acc = acc + xl[:, k, None] * wh[None, k, :]
        acc = acc + xh[:, k, None] * wl[None, k, :]
        acc = acc + xh[:, k, None] * wh[None, k, :]
    return acc.half() if half else acc
