"""CASES, FLOAT64 REFERENCE AND DERIVED BOUND OF THE SUB-WORD POOLING TESTS (test infrastructure, NOT product code).

``ggcn_subword_pool`` / ``ggcn_subword_pool_bf16`` (csrc/subword_pool.hip) compute ``Y[b, r, :] = sum_c A[b, r, c] * X[b, c, :]`` on
the non-zeros of ``A`` only; the backward pass is the same launch with the two strides of ``A`` swapped.  Here: the transforms
(``transform_like_reference``, ``dense_transform``), the float64 statement ``ref64``, the per-element ``bound``, the vector / scalar
rule of the two C entries restated on an argument list (``takes_vector_form``), and ``CASES``: named inputs built by seed, each with
the launch form it must take and what it claims about its rows.  ``tests/test_subword_pool_cases_cpu.py`` holds every case to its
claims and the bound to a float32 evaluation; ``tests/test_gpu_subword_pool.py`` runs the kernels on the same cases.  numpy and
torch on CPU tensors only: nothing here calls the library.

A case is stated at the level of the launch: ``R`` rows of ``Y``, ``C`` rows of ``X``, ``D`` features.  ``swap=False``: the caller's
``a`` is [B, R, C] and the product is ``a @ x``; ``swap=True``: ``a`` is [B, C, R] and the product is ``a^T @ x`` (what the backward
pass launches).  ``a`` and ``x`` are views into larger buffers whose other elements are junk (7 in ``a``, NaN in ``x``), so a wrong
stride or offset shows in the values.
"""
import math
import zlib
from collections import namedtuple

import numpy as np
import torch

MAX_COLS = 2048      # kMaxCols of csrc/subword_pool.hip: columns of A per row
ROUND = 256          # columns the compaction loop takes per round
SLAB = 1024          # features per workgroup
U32 = 2.0 ** -24     # unit roundoff of float32
TINY32 = 2.0 ** -149  # the smallest float32 subnormal
JUNK = 7.0           # what the buffers of ``a`` hold outside the view

# fake, 512-byte aligned addresses for ``wrapper_args`` without a device (what a fresh device allocation is aligned to)
A_BASE, X_BASE, Y_BASE = 1 << 20, 1 << 24, 1 << 28


# ------------------------------------------------------------------------------------------------------------ the transforms
def transform_like_reference(B, T, L, rng, ori_ml=None, bert_ml=None):
    """data_utils.py:749-766: word i covers l_i consecutive sub-word positions starting at offset 1
    ([CLS] first), each with weight 1/l_i; padded to [ORI_ML, BERT_ML]."""
    ori_ml, bert_ml = ori_ml or T, bert_ml or L
    tr = np.zeros((B, ori_ml, bert_ml), dtype=np.float32)
    for b in range(B):
        n_words = int(rng.integers(1, T + 1))
        off = 1
        for i in range(n_words):
            l = int(rng.integers(1, 5))
            if off + l >= L:
                break
            tr[b, i, off:off + l] = 1.0 / l
            off += l
    return tr


def dense_transform(B, R, C, density, rng, scale=1.0, empty=(), full=()):
    """float32 [B, R, C]: an entry is non-zero with probability ``density``, its value a random sign times ``scale`` times a draw
    from [0.5, 1).  The rows ``empty`` hold no non-zero and the rows ``full`` hold C of them, in every batch."""
    v = rng.uniform(0.5, 1.0, size=(B, R, C)) * rng.choice([-1.0, 1.0], size=(B, R, C)) * scale
    a = np.where(rng.random((B, R, C)) < density, v, 0.0)
    for r in full:
        a[:, r, :] = v[:, r, :]
    for r in empty:
        a[:, r, :] = 0.0
    return a.astype(np.float32)


# ------------------------------------------------------------------------------------------------- the reference and its bound
def _launch_matrix(a, swap):
    return a.transpose(1, 2) if swap else a


def ref64(a, x, swap=False):
    """``a @ x`` (``swap``: ``a^T @ x``) in float64, on the values the tensors hold (a bfloat16 ``x`` converts exactly)."""
    return _launch_matrix(a.double(), swap) @ x.double()


def bound(a, x, swap=False, bf16=False):
    """The per-element bound on ``|kernel - ref64|``, [B, R, D] float64, derived from the kernel and not measured.

    One thread owns one element of Y.  It starts from 0 and makes one ``fmaf(a_c, x_c, acc)`` per kept entry of its row of A, in
    ascending c, where "kept" is ``a_c != 0``: n fused multiply-adds for a row of n non-zeros, each with one rounding of relative
    size u = 2^-24 (the product inside an fmaf is exact).  The term of entry e goes through at most n roundings, so by the
    standard forward analysis of a recursive sum

        |got - ref| <= gamma_n * S,    gamma_n = n u / (1 - n u),    S = sum_c |a_c| |x_c|  (= |A| @ |X|).

    ``gamma_n <= (n + 1) u`` as long as n (n + 1) <= 2^24, which n <= 2048 satisfies, so the bound is ``(n + 1) u S``; a float32
    evaluation that rounds the products too (numpy has no fmaf) spends the same n roundings per term and stays inside it.  Where an
    intermediate sum is subnormal a rounding is absolute, at most 2^-149: ``n * 2^-149`` is added.  A row without non-zeros has
    S = 0 and the bound is 0: the kernel must write exact zeros.

    bfloat16 (``X`` and ``Y`` in bf16, sums in float32): the inputs convert exactly, the float32 sum carries the error E above, and
    the store rounds it to nearest even once: bfloat16 keeps 8 significant bits, so |got - sum| <= 2^-8 |sum| <= 2^-8 (|ref| + E)
    and |got - ref| <= 2^-8 |ref| + (1 + 2^-8) E.  Stated as the tests use it: ``2^-8 |ref| + 2 (n + 1) u S`` (+ the subnormal
    term).  The first term is reached: a sum that lies half-way between two bfloat16 values.
    """
    m = _launch_matrix(a, swap).double()
    xd = x.double()
    n = (m != 0).sum(dim=2, keepdim=True).double()
    s = m.abs() @ xd.abs()
    b32 = (n + 1.0) * U32 * s + n * TINY32
    if not bf16:
        return b32
    return 2.0 ** -8 * (m @ xd).abs() + 2.0 * (n + 1.0) * U32 * s + n * TINY32


def ascending_float32(a, x, swap=False):
    """The sum as a float32 machine makes it in ascending c with zeros skipped: products and sums rounded to float32 (a zero of
    ``a`` contributes an exact zero, so skipping it changes nothing).  numpy [B, R, D] float32."""
    m = _launch_matrix(a, swap).numpy().astype(np.float32)
    xv = x.float().numpy()
    acc = np.zeros((m.shape[0], m.shape[1], xv.shape[2]), dtype=np.float32)
    for c in range(m.shape[2]):
        col = m[:, :, c]
        if not col.any():
            continue
        with np.errstate(invalid="ignore"):
            term = (col[:, :, None] * xv[:, c, None, :]).astype(np.float32)
        acc = np.where(col[:, :, None] != 0, (acc + term).astype(np.float32), acc)
    return acc


# ------------------------------------------------------------------------------------------------------------- the vec rule
ARGS = ("A", "sa_b", "sa_r", "sa_c", "X", "x_batch", "ldx", "Y", "y_batch", "ldy", "B", "R", "C", "D", "stream")


def takes_vector_form(args, bf16):
    """The ``vec`` rule of ``subword_pool`` / ``subword_pool_bf16`` on an entry's argument list (``ARGS``; pointers as integers):
    D, ldx, ldy, x_batch and y_batch multiples of 4, X and Y aligned to 16 bytes (float32) or 8 bytes (four bf16)."""
    v = dict(zip(ARGS, args))
    align = 8 if bf16 else 16
    return (all(int(v[k]) % 4 == 0 for k in ("D", "ldx", "ldy", "x_batch", "y_batch"))
            and int(v["X"]) % align == 0 and int(v["Y"]) % align == 0)


def wrapper_args(a, x, swap, bf16, x_base=X_BASE):
    """The argument list ``pooling._launch`` passes for ``a`` and ``x`` (``x`` with unit stride along D): the strides of ``a``
    (swapped under ``swap``), ``x`` where it lies in its buffer, a fresh contiguous ``y``.  ``x_base`` is the address of the
    buffer of ``x``; a device allocation is 512-byte aligned, so only the offset of ``x`` in it decides the alignment."""
    assert x.stride(2) == 1
    B, R, C = a.shape
    sb, sr, sc = a.stride()
    if swap:
        R, C, sr, sc = C, R, sc, sr
    D = x.shape[2]
    size = 2 if bf16 else 4
    return [A_BASE + a.storage_offset() * 4, sb, sr, sc, x_base + x.storage_offset() * size, x.stride(0), x.stride(1),
            Y_BASE, R * D, D, B, R, C, D, None]


# ----------------------------------------------------------------------------------------------------------------- the cases
# name; form "vector" | "scalar"; swap; B, R, C, D of the launch; kind "dense" | "reference"; density; a_layout "contig" |
# "slice" ([:, :d1, :d2] of a buffer padded by 3 rows and 5 columns) | "step2" (buf[:, :, ::2]) | "perm" (a [B, d2, d1] buffer
# permuted); x_off (elements between the start of the buffer of x and x), ldx, x_gap (x_batch - C * ldx); rows {"empty" |
# "last_round" | "ends" | "full": row of the launch matrix, in every batch}, rounds (of the compaction loop) and nnz (lo, hi: where
# the largest number of non-zeros in a row of the launch matrix lies): what the case claims.
Case = namedtuple("Case", "name form swap B R C D kind density a_layout x_off ldx x_gap rows rounds nnz")


def _case(name, form, B, R, C, D, swap=False, kind="dense", density=0.5, a_layout="contig", x_off=0, ldx=None, x_gap=0,
          rows=None, rounds=1, nnz=(2, 9)):
    return Case(name, form, swap, B, R, C, D, kind, density, a_layout, x_off, D if ldx is None else ldx, x_gap, dict(rows or {}),
                rounds, nnz)


VECTOR_D = (4, 1020, 1024, 1028, 2052)             # one lane, a slab less one lane, a slab, a slab and a lane, two and a lane
SCALAR_D = (1, 3, 255, 257, 1023, 1025, 2049)      # q = 0 alone; q = 0, 1; all four q; a second and a third slab of one column
ROUND_C = (1, 255, 256, 257, 512, 513)
ROUND_ROWS = {"empty": 0, "last_round": 1, "ends": 2}
# C -> (rounds, where the largest row lies): up to 256 columns the row that fills the last round is the largest; beyond, a row
# drawn at density 0.6 holds more than one round brings
ROUND_CLAIMS = {1: (1, (1, 1)), 255: (1, (255, 255)), 256: (1, (256, 256)), 257: (2, (120, 200)), 512: (2, (257, 360)),
                513: (3, (257, 360))}
CAP_ROWS = {"full": 0, "empty": 1}


def _cases():
    c = []
    for D in VECTOR_D:
        c.append(_case("slab-vector-D%d" % D, "vector", 2, 3, 9, D))
    for D in SCALAR_D:
        c.append(_case("slab-scalar-D%d" % D, "scalar", 2, 3, 9, D))
    c.append(_case("scalar-by-base-D1028", "scalar", 2, 3, 9, 1028, x_off=1, ldx=1032))
    c.append(_case("scalar-by-ldx-D1028", "scalar", 2, 3, 9, 1028, ldx=1029))
    c.append(_case("scalar-by-xbatch-D1028", "scalar", 2, 3, 9, 1028, x_gap=2))
    for C in ROUND_C:
        c.append(_case("rounds-C%d" % C, "vector", 2, 5, C, 8, density=0.6, rows=ROUND_ROWS, rounds=ROUND_CLAIMS[C][0],
                       nnz=ROUND_CLAIMS[C][1]))
    c.append(_case("capacity-C2048", "vector", 1, 3, 2048, 8, density=0.6, rows=CAP_ROWS, rounds=8, nnz=(2048, 2048)))
    for D, form in ((1028, "vector"), (37, "scalar")):      # a word of up to four sub-words
        c.append(_case("reference-D%d" % D, form, 3, 7, 40, D, kind="reference", a_layout="slice", nnz=(2, 4)))
    # ---- the transposed twins: a is [B, C, R], the row of the launch is a column of a
    for D in VECTOR_D:
        c.append(_case("swap-slab-vector-D%d" % D, "vector", 2, 3, 9, D, swap=True))
    for D in SCALAR_D:
        c.append(_case("swap-slab-scalar-D%d" % D, "scalar", 2, 3, 9, D, swap=True))
    for C in ROUND_C:
        c.append(_case("swap-rounds-C%d" % C, "vector", 2, 5, C, 8, swap=True, density=0.6, rows=ROUND_ROWS,
                       rounds=ROUND_CLAIMS[C][0], nnz=ROUND_CLAIMS[C][1]))
    for R in (257, 513):                            # the forward's R becomes the twin's C: here its C (5) became R
        c.append(_case("swap-rows-R%d" % R, "vector", 2, R, 5, 8, swap=True, density=0.6, rows={"empty": 0}, nnz=(5, 5)))
    c.append(_case("swap-capacity-R2048", "vector", 1, 2048, 3, 8, swap=True, density=0.6, rows={"empty": 1}, nnz=(3, 3)))
    c.append(_case("swap-capacity-C2048", "vector", 1, 3, 2048, 8, swap=True, density=0.6, rows=CAP_ROWS, rounds=8,
                   nnz=(2048, 2048)))
    for D, form in ((1028, "vector"), (37, "scalar")):      # a sub-word belongs to one word
        c.append(_case("swap-reference-D%d" % D, form, 3, 40, 7, D, swap=True, kind="reference", a_layout="slice", nnz=(1, 1)))
    # ---- a with other strides
    c.append(_case("a-step2", "vector", 2, 5, 300, 12, density=0.3, a_layout="step2", rows={"empty": 3}, rounds=2, nnz=(70, 130)))
    c.append(_case("a-permuted", "vector", 3, 5, 300, 12, density=0.3, a_layout="perm", rows={"empty": 3}, rounds=2,
                   nnz=(70, 130)))
    c.append(_case("swap-a-step2", "scalar", 2, 6, 270, 9, swap=True, density=0.3, a_layout="step2", rows={"empty": 3}, rounds=2,
                   nnz=(60, 120)))
    return tuple(c)


CASES = _cases()
CASE = {c.name: c for c in CASES}
CASE_IDS = tuple(c.name for c in CASES)


def value_scale(C):
    """The power of two the entries of a dense transform of C columns are scaled by, so that the float32 bound, which grows like
    n^2 (n roundings on a sum of n terms), stays below 1e-5: ``C (C + 1) scale <= 25`` (1 for C = 4, 2^-18 at C = 2048)."""
    return 2.0 ** -max(0, math.ceil(math.log2(C * (C + 1) / 25.0)))


def _launch_level(case, rng):
    """The matrix of the launch, numpy float32 [B, R, C]."""
    B, R, C = case.B, case.R, case.C
    if case.kind == "reference":                     # the reference's transform is the caller's a: [B, T, L], words by sub-words
        tr = transform_like_reference(B, C, R, rng) if case.swap else transform_like_reference(B, R, C, rng)
        return tr.transpose(0, 2, 1) if case.swap else tr
    rows = case.rows
    m = dense_transform(B, R, C, case.density, rng, scale=value_scale(C),
                        empty=[rows[k] for k in ("empty",) if k in rows], full=[rows[k] for k in ("full",) if k in rows])
    if "last_round" in rows:                         # non-zeros only in the last round of 256 columns (all of them kept)
        first = ROUND * ((C - 1) // ROUND)
        m[:, rows["last_round"], :first] = 0.0
        m[:, rows["last_round"], first:] = np.where(m[:, rows["last_round"], first:] != 0, m[:, rows["last_round"], first:],
                                                    np.float32(value_scale(C)))
    if "ends" in rows:                               # columns 0 and C - 1 alone
        keep = np.float32(0.75 * value_scale(C))
        m[:, rows["ends"], :] = 0.0
        m[:, rows["ends"], 0], m[:, rows["ends"], C - 1] = keep, -keep if C > 1 else keep
    return m


def _lay_out(u, layout):
    """numpy [B, d1, d2] -> a torch view of that shape and those values in a junk-filled buffer."""
    B, d1, d2 = u.shape
    t = torch.from_numpy(np.ascontiguousarray(u))
    if layout == "contig":
        return t.clone()
    if layout == "slice":
        buf = torch.full((B, d1 + 3, d2 + 5), JUNK)
        v = buf[:, :d1, :d2]
    elif layout == "step2":
        buf = torch.full((B, d1, 2 * d2), JUNK)
        v = buf[:, :, ::2]
    else:
        assert layout == "perm", layout
        buf = torch.full((B, d2, d1), JUNK)
        v = buf.permute(0, 2, 1)
    v.copy_(t)
    return v


def build(case):
    """``(a, x)`` of a case as CPU float32 views, the same on every call: ``a`` [B, R, C] (``swap``: [B, C, R]) in its layout,
    ``x`` [B, C, D] standard normal at ``x_off`` elements into a NaN buffer, rows ``ldx`` and batches ``C * ldx + x_gap`` apart."""
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    m = _launch_level(case, rng)
    a = _lay_out(m.transpose(0, 2, 1) if case.swap else m, case.a_layout)
    B, C, D = case.B, case.C, case.D
    x_batch = C * case.ldx + case.x_gap
    buf = torch.full((case.x_off + B * x_batch,), float("nan"))
    x = buf.as_strided((B, C, D), (x_batch, case.ldx, 1), case.x_off)
    x.copy_(torch.from_numpy(rng.standard_normal((B, C, D)).astype(np.float32)))
    return a, x


def on_device(t, dev, dtype=None):
    """The whole buffer behind the view ``t`` copied to ``dev`` (as ``dtype``), and the same view of the copy: shape, strides and
    offset survive, unlike with ``t.to(dev)``."""
    n = t.untyped_storage().nbytes() // t.element_size()
    flat = torch.as_strided(t, (n,), (1,), 0).to(dev)
    flat = flat if dtype is None else flat.to(dtype)
    assert flat.data_ptr() % 16 == 0
    return flat.as_strided(tuple(t.shape), tuple(t.stride()), t.storage_offset())


def shifted(t, by=1):
    """The view ``t`` copied to a new buffer, same strides, ``by`` elements further from its start."""
    n = t.untyped_storage().nbytes() // t.element_size()
    flat = torch.full((n + by,), float("nan"), dtype=t.dtype, device=t.device)
    v = flat.as_strided(tuple(t.shape), tuple(t.stride()), t.storage_offset() + by)
    v.copy_(t)
    return v


def launch_matrix(case, a):
    """The matrix of the launch [B, R, C] behind the caller's ``a``."""
    return _launch_matrix(a, case.swap)
