"""CASE GENERATORS OF THE FORWARD AGGREGATION TESTS (test infrastructure, NOT product code).

Batched CSRs built in numpy, row by row, so that a test owns the structure: duplicate and unsorted columns stay as they are
drawn.  ``tests/test_aggregate_ref_cpu.py`` runs every generator through a float32 evaluation in three summation orders and
holds it to the bound of ``oracle/aggregate_ref.py``; ``tests/test_gpu_aggregate.py`` runs the kernels on the same cases.
"""
import numpy as np

STRUCTURES = ("degrees", "hub", "empty", "self", "ragged", "dup")
WEIGHTS = ("ones", "positive", "signed")
DEGREES = (0, 1, 2, 3, 4, 5, 7, 8, 9)   # consecutive rows: the paired rows t, t + 4 differ in their number of four-edge trips
MIN_DEN = 0.5
IDX_CAP = 4096                          # edges per graph whose column ids the narrow form stages (kIdxCap of csrc/aggregate.hip)


def _sparse_rows(T, rng, mean=3):
    return [rng.choice(T, size=min(T, int(k)), replace=False) for k in rng.poisson(mean, size=T)]


def graph_rows(kind, T, rng, g=0):
    """The T rows of one graph as arrays of local column ids."""
    if kind == "degrees":     # degree 0, 1, 2, 3, 4, 5, 7, 8, 9, 0, 1, ...; a degree above T repeats columns
        return [rng.choice(T, size=d, replace=d > T) for d in (DEGREES[(t + g) % len(DEGREES)] for t in range(T))]
    if kind == "hub":         # one row with all T columns, one column in every row
        rows = _sparse_rows(T, rng, 2)
        hub_row, hub_col = int(rng.integers(0, T)), int(rng.integers(0, T))
        rows = [np.union1d(r, [hub_col]) for r in rows]
        rows[hub_row] = rng.permutation(T)
        return rows
    if kind == "empty":
        return [np.zeros(0, dtype=np.int64) for _ in range(T)]
    if kind == "self":        # a self loop in every row, first, last or alone
        rows = []
        for t in range(T):
            others = np.setdiff1d(rng.choice(T, size=min(T, int(rng.integers(0, 4))), replace=False), [t])
            rows.append(np.concatenate(([t], others) if t % 2 else (others, [t])).astype(np.int64))
        return rows
    if kind == "ragged":      # a graph of L <= T nodes: the padding rows have no edges and no one points at them
        L = int(rng.integers(1, T + 1))
        return [rng.choice(L, size=min(L, int(k)), replace=False) if t < L else np.zeros(0, dtype=np.int64)
                for t, k in enumerate(rng.poisson(3, size=T))]
    if kind == "dup":         # columns drawn with replacement, left in the order drawn; row 0 holds c, d, c whatever was drawn
        rows = [rng.integers(0, T, size=int(k)) for k in rng.poisson(4, size=T)]
        c, d = int(rng.integers(0, T)), int(rng.integers(0, T))
        rows[0] = np.array([c, d, c] + list(rows[0]), dtype=np.int64)
        return rows
    raise ValueError(kind)


def edges_exactly(T, want, rng):
    """A graph of T nodes with exactly ``want`` distinct edges (the staging capacity of the narrow form and one more)."""
    assert want <= T * T
    flat = rng.choice(T * T, size=want, replace=False)
    r, c = np.divmod(np.sort(flat), T)
    return [c[r == t] for t in range(T)]


def batch_rows(kind, B, T, rng):
    """B graphs: ``kind`` in STRUCTURES for every graph ("empty": graph 1 of a batch of two or more, graph 0 of one, among
    sparse graphs), "mixed" (graph g takes STRUCTURES[g % 6]) or "cap" (T * T >= 4097: graph 0 holds 4096 edges, graph 1
    4097, the rest are sparse)."""
    out = []
    for g in range(B):
        if kind == "mixed":
            out.append(graph_rows(STRUCTURES[g % len(STRUCTURES)], T, rng, g))
        elif kind == "empty":
            out.append(graph_rows("empty", T, rng) if g == min(1, B - 1) else _sparse_rows(T, rng))
        elif kind == "cap":
            out.append(edges_exactly(T, IDX_CAP + g, rng) if g < 2 else _sparse_rows(T, rng))
        else:
            out.append(graph_rows(kind, T, rng, g))
    return out


def build_csr(graphs, T):
    """``graphs`` [B][T] arrays of local column ids -> (rowptr int32 [B*T+1], colidx int32 [nnz], global node ids)."""
    counts = np.array([len(r) for rows in graphs for r in rows], dtype=np.int64)
    assert len(counts) == len(graphs) * T
    rowptr = np.zeros(len(counts) + 1, dtype=np.int64)
    np.cumsum(counts, out=rowptr[1:])
    cols = [np.asarray(r, dtype=np.int64) + g * T for g, rows in enumerate(graphs) for r in rows]
    colidx = np.concatenate(cols) if cols else np.zeros(0, dtype=np.int64)
    for g in range(len(graphs)):
        seg = colidx[rowptr[g * T]:rowptr[(g + 1) * T]]
        assert seg.size == 0 or (seg.min() >= g * T and seg.max() < (g + 1) * T), "an edge leaves its graph"
    assert rowptr[-1] < 2 ** 31
    return rowptr.astype(np.int32), colidx.astype(np.int32)


def draw_weights(mode, rowptr, rng, stats=None):
    """float32 edge values of a CSR: "ones" -> None (the 0/1 adjacency), "positive" -> [0.25, 2), "signed" -> [-0.25, 2) with
    every row's den = sum + 1 >= MIN_DEN: a row below it is drawn again, and fewer than 5 % of the rows that hold an edge may
    need that (asserted; ``stats``, a dict, receives ``rows`` and ``rejected``).  "exact" -> {0.5, 1, 2}."""
    nnz = int(rowptr[-1])
    if mode == "ones":
        return None
    if mode == "positive":
        return rng.uniform(0.25, 2.0, size=nnz).astype(np.float32)
    if mode == "exact":
        return rng.choice(np.array([0.5, 1.0, 2.0], dtype=np.float32), size=nnz)
    assert mode == "signed", mode
    w = rng.uniform(-0.25, 2.0, size=nnz).astype(np.float32)
    rows = rejected = 0
    for i in np.flatnonzero(np.diff(rowptr)):
        a, b = int(rowptr[i]), int(rowptr[i + 1])
        rows += 1
        first = True
        while float(w[a:b].astype(np.float64).sum()) + 1.0 < MIN_DEN:
            rejected += first
            first = False
            w[a:b] = rng.uniform(-0.25, 2.0, size=b - a).astype(np.float32)
    assert rejected * 20 < max(rows, 1), "%d of %d rows fell below den = %.1f" % (rejected, rows, MIN_DEN)
    if stats is not None:
        stats["rows"], stats["rejected"] = stats.get("rows", 0) + rows, stats.get("rejected", 0) + rejected
    return w


def make_case(kind, weights, B, T, F, seed, half=False, exact=False, negative=False):
    """One whole case as numpy arrays: ``h`` [B*T,F] float32 (``half``: values a half holds exactly), the CSR, ``vals``, ``bias``
    [F], the three gates [B,F] (store gate in (0, 1), gate_a in [-1, 1], gate_b in (0, 1)).  ``exact``: integer features in
    [-8, 8] and weights in {0.5, 1, 2} (``weights`` "ones" stays 0/1), so that every fp32 sum is exact.  ``negative``: features
    below -0.5 and a negative bias -- with non-negative weights y is negative everywhere."""
    rng = np.random.default_rng(seed)
    rowptr, colidx = build_csr(batch_rows(kind, B, T, rng), T)
    vals = draw_weights("exact" if exact and weights != "ones" else weights, rowptr, rng)
    N = B * T
    if exact:
        h = rng.integers(-8, 9, size=(N, F)).astype(np.float32)
    elif negative:
        assert weights != "signed"
        h = (-0.5 - np.abs(rng.standard_normal((N, F)))).astype(np.float32)
    else:
        h = rng.standard_normal((N, F)).astype(np.float32)
    if half:
        h = h.astype(np.float16).astype(np.float32)
    bias = rng.uniform(-1.0, -0.25, size=F) if negative else rng.uniform(-0.5, 0.5, size=F)
    sg = 1.0 / (1.0 + np.exp(-rng.standard_normal((B, F))))
    ga = rng.uniform(-1.0, 1.0, size=(B, F))
    gb = 1.0 / (1.0 + np.exp(-rng.standard_normal((B, F))))
    f32 = np.float32
    return {"h": h, "rowptr": rowptr, "colidx": colidx, "vals": vals, "bias": bias.astype(f32), "sg": sg.astype(f32),
            "ga": ga.astype(f32), "gb": gb.astype(f32), "B": B, "T": T, "F": F}
