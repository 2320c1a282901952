"""THE CASES AND GATES OF THE DENSE HEAD'S SWEEP AND OF THE OTHER FIXED-ORDER TAIL LAUNCHES (test infrastructure, NOT product code;
no GPU needed to import).

``tests/test_dense_head_cases_cpu.py`` checks the table against the kernel's two branch conditions and the gates against float32
products, right and wrong; ``tests/test_gpu_dense_head.py`` runs every case on the device.  Pure torch: every function here takes
CPU and device tensors alike.

A case is ``Case(B, H, C, pad_p, pad_w, pad_l, offset, bias, n_part_spec)``: ``logits [B,C] = pooled [B,H] . Wt [H,C] (+ bias)``
through ``ggcn_dense_head`` with ``ldp = H + pad_p``, ``ldw = C + pad_w``, ``ldl = C + pad_l``; ``offset`` = 1 when ``pooled`` starts ONE
element into its 16-byte aligned buffer; ``n_part_spec`` is None or the ``F_block`` of the regulariser's partials the launch also
adds (``n_part = B * ceil(F_block / 64)`` floats).

``dense_head_kernel`` (``csrc/heads.hip``): one workgroup of 16 wavefronts per 8 sentences.  Two wavefronts stage a pooled row in
LDS, each ``hb = (H + 1) >> 1`` columns of it; wavefront w then takes k-slice w of ``kq = ceil(H / 16)`` columns for the 8 rows,
lane = class; the 16 slices meet in LDS and are added in ascending order, then the bias.  Two branch conditions, pure functions of
the case (``staging16``, ``product16``):

* 16-byte staging: ``H % 8 == 0``, ``ldp % 4 == 0`` and a 16-byte aligned ``pooled``.  Before the fix this sweep came with, the
  condition on H was ``hb % 4 == 0`` (``staging16_parent``), which also holds for H = 8m - 1: there the second wavefront of row r
  loaded ``pooled[r][H-3 .. H]`` -- the pad column with it -- and stored it to ``rows[r*H + H-3 .. r*H + H]``, the last float being
  row r + 1's first element, which row r + 1's first wavefront writes in the same phase.  The race's loser leaves the pad value
  as ``pooled[r+1][0]`` (``defect_signature``).
* 16-byte product loop (four k per step): ``H % 4 == 0`` and ``kq % 4 == 0``.

Classes of width (``width_class``; the table must hold every one: ``REQUIRED``):

* ``8m-1``           H % 8 == 7: 7, 15, 39, 767, 1023.  With ``pad_p = 1`` and an aligned base the parent's condition took the
                     16-byte staging (the defect class); every other layout of these widths staged by elements then as now.
* ``mult8-prod16``   H % 8 == 0, 16-byte product: 64, 128, 768, 1024 (the LDS bound: 32 KiB of rows + 32 KiB of slices).
* ``mult8-prod1``    H % 8 == 0, scalar product: 8, 16, 96.
* ``scalar-prod16``  H % 8 == 4 with kq % 4 == 0: element staging with the 16-byte product, and k-slices that are empty
                     (52: slices 13..15; 116, 180: slice 15, 116's slice 14 half full).
* ``narrow``         fewer columns than wavefronts: 1, 2, 5 (kq = 1, slices H..15 empty).
* ``ordinary``       odd, nothing else: 37, 301.

Operands (seeded, made on the CPU): ``pooled ~ N(0,1)`` with ``1 <= |pooled[:, 0]| <= 2``, ``Wt ~ N(0,1) / sqrt(H)`` with
``|Wt[0, :]| >= 1 / sqrt(H)``, ``bias ~ 0.1 N(0,1)``, ``partials ~ 0.5 + U(0,1)`` (one sign: nothing cancels, so a share of them
left out shows).  The clamps on column 0 / row 0 make the defect's
signature (pad value 3.0 for ``pooled[b][0]``) an error of at least ``1 / sqrt(H)`` in EVERY element of every row it touches, far
outside both gates -- the GPU sweep cannot pass on a kernel that loses the race, whichever rows lose it.

Gates (``S_bc = sum_k |p_bk| |Wt_kc| + |bias_c|`` and ``ref`` in float64, ``u = 2^-24``; every element meets both):

* derived: ``|logits - ref| <= n u / (1 - n u) * S`` with ``n = H + 17`` -- the arithmetic the header states: a length-H fp32 FMA dot
  product (H roundings at most along a path, in 16 slices), 15 slice additions (16 counted: the first adds to 0.0f), one bias
  addition.
* the project's own, from ``test_dense_head_rides_with_the_regularisers_final_sum``: ``gates.gate(..., tol=2e-5)``, i.e.
  ``2e-5 * max(1, max|ref|)``.
* ``xy``: ``|xy - ref| <= n u / (1 - n u) * sum|part| / B + u |ref|`` with ``n = n_part`` and ``ref = sum(part) / B``: a sum of
  n_part floats in any order has at most n_part - 1 rounded additions along a path (an addition to an exact zero rounds nothing),
  the division by B rounds once more.

The other tail launches (``tests/test_gpu_dense_head.py`` runs them; same reasoning -- a sum's path has at most as many roundings
as it has non-zero leaves, whatever its tree):

* ``ggcn_colsum`` (rows in at most 64 slabs, four wavefronts per slab pairwise, slabs ascending): ``M u / (1 - M u) * sum_r |x_rf|``.
* ``ggcn_transpose``: copies; bit-exact.
* ``ggcn_gate_overlap`` (per row a 256-thread-strided FMA dot product of length F and a fixed tree, then the B row sums in a
  256-strided chain and the same tree, then / B): at most F roundings along a row's path, B - 1 along the sum's, one for the
  division: ``n u / (1 - n u) * sum_bf |x1 y1| / B`` with ``n = F + B``.
"""
import collections
import math

import torch

Case = collections.namedtuple("Case", "B H C pad_p pad_w pad_l offset bias n_part_spec")
U = 2.0 ** -24
ROWS, WAVES = 8, 16                      # kHeadRows, kHeadWaves of csrc/heads.hip
PROJECT_TOL = 2e-5                       # test_dense_head_rides_with_the_regularisers_final_sum's
PAD_VALUE = 3.0                          # the finite stand-in for the pad column in defect_signature
MANY = 520                               # rows of the many-workgroup case of every class (65 workgroups)


def _c(B, H, C, bias=True, pad_p=0, pad_w=0, pad_l=0, offset=0, f_block=None):
    return Case(B, H, C, pad_p, pad_w, pad_l, offset, bias, f_block)


# ---------------------------------------------------------------- the kernel's branch conditions
def pointer_offset(c):
    """Bytes of ``pooled`` past a 16-byte boundary."""
    return 4 * c.offset


def staging16(c):
    """The 16-byte staging loop is taken (csrc/heads.hip after the fix)."""
    return c.H % 8 == 0 and (c.H + c.pad_p) % 4 == 0 and pointer_offset(c) % 16 == 0


def staging16_parent(c):
    """What took the 16-byte staging before the fix: hb % 4 == 0, which H = 8m - 1 also meets."""
    return ((c.H + 1) >> 1) % 4 == 0 and (c.H + c.pad_p) % 4 == 0 and pointer_offset(c) % 16 == 0


def product16(c):
    """The 16-byte LDS reads of the product loop are taken."""
    return c.H % 4 == 0 and (-(-c.H // WAVES)) % 4 == 0


def empty_slices(H):
    """How many of the 16 k-slices hold no column."""
    kq = -(-H // WAVES)
    return sum(1 for w in range(WAVES) if w * kq >= H)


def width_class(c):
    if c.H % 8 == 7:
        return "8m-1"
    if c.H % 8 == 0:
        return "mult8-prod16" if product16(c) else "mult8-prod1"
    if product16(c):
        return "scalar-prod16"
    return "narrow" if c.H < WAVES else "ordinary"


def defect_class(c):
    """The layout of an 8m - 1 width that the parent's condition sent through the 16-byte staging."""
    return c.H % 8 == 7 and staging16_parent(c)


# class -> the widths the table must hold for it
REQUIRED = {"8m-1": (7, 15, 39, 767, 1023), "mult8-prod16": (64, 128, 768, 1024), "mult8-prod1": (8, 16, 96),
            "scalar-prod16": (52, 116, 180), "narrow": (1, 2, 5), "ordinary": (37, 301)}
BATCHES, CLASSES_C = (1, 7, 8, 9, 17), (1, 5, 34, 63, 64)
PADS_P = (1, 3, 4)
# (B, F_block) of the final-sum cases: n_part = 1, 63, 1024, 1025, 6240
FINAL_SUMS = ((1, 1), (7, 576), (16, 4096), (41, 1600), (MANY, 768))
N_PARTS = (1, 63, 1024, 1025, 6240)


def _table():
    """{class: [cases]}.  Per width: the five batches, each with another C, bias on and off in turn, contiguous; the widest and the
    narrowest width of a class also in every layout (pads 1, 3, 4 of pooled; offset; Wt and logits padded) at B = 9; the class's
    MANY-row case on its widest width that keeps the class's staging (pad_p = 1 for 8m - 1: the defect's own layout)."""
    table = {}
    n = 0
    for name, widths in REQUIRED.items():
        cases = []
        for H in widths:
            own = 1 if name == "8m-1" else 0          # 8m - 1: every batch in the defect's layout
            for i, B in enumerate(BATCHES):
                cases.append(_c(B, H, CLASSES_C[(i + n) % 5], bias=(i + n) % 2 == 0, pad_p=own))
            n += 1
        for H in (widths[0], widths[-1]):
            cases += [_c(9, H, 34, pad_p=p) for p in PADS_P if not (name == "8m-1" and p == 1)]
            cases += [_c(9, H, 34, pad_p=0)] if name == "8m-1" else []
            cases += [_c(9, H, 34, offset=1), _c(9, H, 34, offset=1, pad_p=3), _c(9, H, 5, bias=False, pad_w=3),
                      _c(9, H, 63, pad_l=3), _c(17, H, 64, bias=False, pad_p=4 + own, pad_w=3, pad_l=3)]
        cases.append(_c(MANY, widths[-1], 34, pad_p=1 if name == "8m-1" else 0, pad_w=3, pad_l=3))
        cases.append(_c(MANY, widths[0], 64, bias=False, pad_p=1 if name == "8m-1" else 0))
        table[name] = cases
    # the final sum rides along: partials of B * ceil(F_block / 64) floats
    for i, (B, F_block) in enumerate(FINAL_SUMS):
        H = (768, 7, 52, 37, 767)[i]
        c = _c(B, H, 34, pad_p=1 if H % 8 == 7 else 0, f_block=F_block)
        table[width_class(c)].append(c)
    return table


TABLE = _table()
CASES = [(name, c) for name, cases in TABLE.items() for c in cases]


def case_id(c):
    s = "%dx%dx%d" % (c.B, c.H, c.C)
    for name, v in (("pp", c.pad_p), ("pw", c.pad_w), ("pl", c.pad_l)):
        s += "-%s%d" % (name, v) if v else ""
    return s + ("-off" if c.offset else "") + ("" if c.bias else "-nobias") + ("-xy%d" % c.n_part_spec if c.n_part_spec else "")


def n_part(c):
    return c.B * ((c.n_part_spec + 63) // 64) if c.n_part_spec else 0


# ---------------------------------------------------------------- operands
def operands(c):
    """(pooled [B,H], Wt [H,C], bias [C] or None, partials [n_part] or None): float32 on the CPU, seeded by the shape."""
    gen = torch.Generator().manual_seed(1000003 * c.B + 1009 * c.H + c.C)
    p = torch.randn(c.B, c.H, generator=gen)
    wt = torch.randn(c.H, c.C, generator=gen) / math.sqrt(c.H)
    bias = 0.1 * torch.randn(c.C, generator=gen)
    part = 0.5 + torch.rand(max(n_part(c), 1), generator=gen)
    sign = lambda t: torch.where(t < 0, -torch.ones_like(t), torch.ones_like(t))
    p[:, 0] = sign(p[:, 0]) * p[:, 0].abs().clamp(1.0, 2.0)
    wt[0] = sign(wt[0]) * wt[0].abs().clamp_min(1.0 / math.sqrt(c.H))
    return p, wt, (bias if c.bias else None), (part[:n_part(c)] if c.n_part_spec else None)


# ---------------------------------------------------------------- the float64 statement and the gates
def statement64(p, wt, bias):
    """(ref, S) = (p . Wt + bias, |p| . |Wt| + |bias|) in float64 on p's device."""
    p64, w64 = p.double(), wt.double().to(p.device)
    ref, S = p64 @ w64, p64.abs() @ w64.abs()
    if bias is not None:
        b64 = bias.double().to(p.device)
        ref, S = ref + b64, S + b64.abs()
    return ref, S


def gamma(n):
    return n * U / (1.0 - n * U)


def derived_gate(S, H):
    return gamma(H + 17) * S


def project_gate(ref):
    return PROJECT_TOL * max(1.0, float(ref.abs().max()))


def worst_ratio(y, ref, bound):
    """max |y - ref| / bound over the elements (bound: a tensor or a number, > 0); NaN if y holds one."""
    r = (y.double() - ref.to(y.device)).abs() / bound
    return float("nan") if bool(torch.isnan(r).any()) else float(r.max())


def ratios(c, p, wt, bias, logits):
    """{gate name: worst |logits - ref| / gate}."""
    ref, S = statement64(p, wt, bias)
    return {"derived": worst_ratio(logits, ref, derived_gate(S, c.H) + 1e-300), "project": worst_ratio(logits, ref, project_gate(ref))}


def assert_gates(c, r, what=""):
    for name, v in r.items():
        assert v == v and v <= 1.0, "%s %s: |logits - ref| is %.3f of the %s gate" % (case_id(c), what, v, name)


def xy_ratio(part, B, xy):
    """|xy - ref| / (n u / (1 - n u) * sum|part| / B + u |ref|), n = len(part)."""
    p64 = part.double()
    ref = float(p64.sum()) / B
    bound = gamma(part.numel()) * float(p64.abs().sum()) / B + U * abs(ref)
    err = abs(float(xy) - ref)
    return float("nan") if err != err else err / (bound + 1e-300)


# ---------------------------------------------------------------- wrong kernels (tests/test_dense_head_cases_cpu.py)
def defect_signature(p):
    """The pooled rows as the workgroups saw them where every race was lost: row r + 1's first element is the pad value, for
    every row but the first of each 8-row group (row 7's stray store lands on the slices' area, which is written later)."""
    q = p.clone()
    rows = torch.arange(p.shape[0])
    q[rows % ROWS != 0, 0] = PAD_VALUE
    return q


def slice_dropped(p, w):
    """The pooled rows with k-slice ``w`` of 16 zeroed: what a product that skips the slice computes."""
    H = p.shape[1]
    kq = -(-H // WAVES)
    q = p.clone()
    q[:, w * kq:min(H, (w + 1) * kq)] = 0.0
    return q


# ---------------------------------------------------------------- the other tail launches
COLSUM_M, COLSUM_F = (1, 63, 64, 65, 129), (1, 63, 64, 65, 300)
TRANSPOSE_N = (1, 31, 32, 33, 300)
OVERLAP_F, OVERLAP_B = (1, 255, 256, 257, 768), (1, 256, 257)


def colsum_ratio(x, out):
    """|out - ref| / (M u / (1 - M u) * sum_r |x_rf|), worst column."""
    x64 = x.double()
    return worst_ratio(out, x64.sum(0), gamma(x.shape[0]) * x64.abs().sum(0) + 1e-300)


def overlap_ratio(x1, y1, xy):
    """|xy - ref| / (n u / (1 - n u) * sum |x1 y1| / B), n = F + B."""
    B, F = x1.shape
    prod = x1.double() * y1.double()
    ref = float(prod.sum()) / B
    err = abs(float(xy) - ref)
    return float("nan") if err != err else err / (gamma(F + B) * float(prod.abs().sum()) / B + 1e-300)
