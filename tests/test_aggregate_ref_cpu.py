"""The float64 statement of the forward aggregation (oracle/aggregate_ref.py) and the case generators of its GPU tests
(oracle/aggregate_cases.py), pinned on the CPU: against the dense oracle, on hand-made numbers, and -- the statement that the
reference alone passes its own gate -- a float32 evaluation in three summation orders inside the derived bound on every
generator."""
import numpy as np
import pytest
import torch

from oracle import aggregate_cases as ac
from oracle import ref_dense
from oracle.aggregate_ref import HALF_SUBNORMAL, U16, U32, aggregate_ref, exact_bound, exact_pool_bound, row_sums

KINDS = ac.STRUCTURES + ("mixed",)


def _ref(c, **kw):
    return aggregate_ref(c["h"], c["rowptr"], c["colidx"], c["vals"], c["bias"], c["B"], c["T"], c["sg"], c["ga"], c["gb"], **kw)


def _dense(c):
    B, T = c["B"], c["T"]
    adj = np.zeros((B * T, T))
    rows = np.repeat(np.arange(B * T), np.diff(c["rowptr"]))
    w = np.ones(len(c["colidx"])) if c["vals"] is None else c["vals"].astype(np.float64)
    np.add.at(adj, (rows, c["colidx"].astype(np.int64) % T), w)       # duplicates add
    return torch.from_numpy(adj.reshape(B, T, T))


@pytest.mark.parametrize("weights", ac.WEIGHTS)
@pytest.mark.parametrize("kind", KINDS)
def test_equals_the_dense_oracle_in_float64(kind, weights):
    """ref_dense.graph_convolution in float64 with W = identity (the hidden fed directly), then the gates and the max."""
    c = ac.make_case(kind, weights, 6, 19, 5, seed=11)
    B, T, F = c["B"], c["T"], c["F"]
    h = torch.from_numpy(c["h"]).double().view(B, T, F)
    y = ref_dense.graph_convolution(h, _dense(c), torch.eye(F, dtype=torch.float64), torch.from_numpy(c["bias"]).double(),
                                    dtype=torch.float64)
    sg, ga, gb = (torch.from_numpy(c[k]).double()[:, None, :] for k in ("sg", "ga", "gb"))
    r = _ref(c)
    for key, want in (("y", y), ("out", y * sg), ("pool_a", (y * ga).max(dim=1)[0]), ("pool_b", (y * gb).max(dim=1)[0])):
        np.testing.assert_allclose(r[key].reshape(want.shape), want.numpy(), rtol=1e-13, atol=1e-14, err_msg=key)


def test_two_nodes_by_hand():
    h = np.array([[2.0], [4.0]], dtype=np.float32)
    # 0/1: row 0 <- {0, 1}, row 1 <- {0}
    r = aggregate_ref(h, [0, 2, 3], [0, 1, 0], None, np.array([0.5]), 1, 2)
    assert r["y"].ravel().tolist() == [6.0 / 3.0 + 0.5, 2.0 / 2.0 + 0.5]
    assert r["out"].ravel().tolist() == [2.5, 1.5] and r["pool_a"].tolist() == [[2.5]] and r["pool_b"].tolist() == [[2.5]]
    # weighted: row 0 <- 3 * h[1]; row 1 <- -0.5 * h[0] + 0.5 * h[1]
    r = aggregate_ref(h, [0, 1, 3], [1, 0, 1], np.array([3.0, -0.5, 0.5], dtype=np.float32), np.array([0.25]), 1, 2,
                      store_gate=np.array([[2.0]]), gate_a=np.array([[-1.0]]))
    assert r["y"].ravel().tolist() == [12.0 / 4.0 + 0.25, 1.0 / 1.0 + 0.25]
    assert r["out"].ravel().tolist() == [6.5, 2.5]
    assert r["pool_a"].tolist() == [[-1.25]] and r["pool_b"].tolist() == [[3.25]]      # a negative gate picks the other end
    # row 0: n = 1, A = 12, S = 12, den = dabs = 4;  row 1: n = 2, A = 3, S = 1, den = 1, dabs = 2
    by = [U32 * (3 * 12 / 4 + 4 * (12 / 4) * (4 / 4) + 2 * 3.25), U32 * (4 * 3 / 1 + 5 * (1 / 1) * (2 / 1) + 2 * 1.25)]
    assert r["bound_y"].ravel().tolist() == by == [27.5 * U32, 24.5 * U32]
    assert r["bound_out"].ravel().tolist() == [by[0] * 2 + U32 * 6.5, by[1] * 2 + U32 * 2.5]
    assert r["bound_pool_a"].tolist() == [[by[0]]] and r["bound_pool_b"].tolist() == [[by[0]]]
    rh = aggregate_ref(h, [0, 1, 3], [1, 0, 1], np.array([3.0, -0.5, 0.5], dtype=np.float32), np.array([0.25]), 1, 2,
                       store_gate=np.array([[2.0]]), half_out=True)
    assert rh["bound_out"].ravel().tolist() == [by[0] * 2 + U32 * 6.5 + U16 * 6.5 + HALF_SUBNORMAL,
                                                by[1] * 2 + U32 * 2.5 + U16 * 2.5 + HALF_SUBNORMAL]
    assert np.array_equal(rh["bound_pool_b"], r["bound_pool_b"])                        # the pools stay fp32


def test_an_edgeless_graph_gives_bias_times_gate():
    c = ac.make_case("empty", "positive", 3, 7, 4, seed=2)
    assert c["rowptr"][7] == c["rowptr"][14] and c["rowptr"][7] > 0 and c["rowptr"][-1] > c["rowptr"][14]
    r = _ref(c)
    b64 = c["bias"].astype(np.float64)
    assert np.array_equal(r["out"][7:14], np.tile(b64 * c["sg"][1].astype(np.float64), (7, 1)))
    assert np.array_equal(r["pool_a"][1], b64 * c["ga"][1].astype(np.float64))
    assert np.array_equal(r["bound_y"][7:14], np.tile(2 * U32 * np.abs(b64), (7, 1)))   # n = 0, S = A = 0: only the bias term
    r0 = aggregate_ref(c["h"], c["rowptr"], c["colidx"], c["vals"], None, 3, 7)
    assert not r0["out"][7:14].any() and not r0["bound_out"][7:14].any()


def test_duplicates_add_and_order_does_not_matter():
    h = np.array([[1.0, -2.0], [3.0, 5.0], [7.0, 11.0]], dtype=np.float32)
    w = np.array([0.5, 2.0, 0.25], dtype=np.float32)
    dup = aggregate_ref(h, [0, 3, 3, 3], [2, 0, 2], w, None, 1, 3)                    # row 0 <- 0.5 h[2] + 2 h[0] + 0.25 h[2]
    one = aggregate_ref(h, [0, 2, 2, 2], [0, 2], np.array([2.0, 0.75], dtype=np.float32), None, 1, 3)
    assert np.array_equal(dup["out"], one["out"])
    assert dup["out"][0].tolist() == [(2.0 + 0.75 * 7.0) / 3.75, (-4.0 + 0.75 * 11.0) / 3.75]
    assert dup["bound_y"][0, 0] > one["bound_y"][0, 0]                                 # three entries round more than two
    c = ac.make_case("dup", "ones", 2, 9, 3, seed=5)
    row0 = c["colidx"][c["rowptr"][0]:c["rowptr"][1]]
    assert row0[0] == row0[2] and len(row0) >= 3
    assert any(np.any(np.diff(c["colidx"][a:b]) < 0) for a, b in zip(c["rowptr"][:-1], c["rowptr"][1:]))   # unsorted rows


def test_the_generators_make_what_they_say():
    rng = np.random.default_rng(0)
    deg = [len(r) for r in ac.graph_rows("degrees", 30, rng)]
    assert deg[:9] == list(ac.DEGREES) and deg[9:18] == list(ac.DEGREES)
    rows = ac.graph_rows("hub", 21, rng)
    assert any(sorted(r.tolist()) == list(range(21)) for r in rows)
    assert any(all(c in r for r in rows) for c in range(21))
    assert all(t in r for t, r in enumerate(ac.graph_rows("self", 13, rng)))
    rag = ac.graph_rows("ragged", 40, np.random.default_rng(4))
    L = 1 + max(int(r.max()) for r in rag if len(r))
    assert L < 40 and all(len(r) == 0 for r in rag[L:])                                # padding rows: no edges, never a source
    for want in (ac.IDX_CAP, ac.IDX_CAP + 1):
        g = ac.edges_exactly(333, want, rng)
        assert sum(len(r) for r in g) == want and all(len(np.unique(r)) == len(r) for r in g)
    rp, ci = ac.build_csr(ac.batch_rows("cap", 3, 333, rng), 333)
    assert rp[333] == 4096 and rp[666] - rp[333] == 4097 and rp.dtype == np.int32 and ci.dtype == np.int32
    kinds = ac.batch_rows("mixed", 9, 12, rng)
    assert all(len(r) == 0 for r in kinds[2]) and all(len(r) == 0 for r in kinds[8])  # the edgeless graphs of a mixed batch


def test_signed_weights_keep_the_denominator_and_reject_few_rows():
    """den = sum w + 1 >= 0.5 on every row, negative weights present, fewer than 5 % of the rows drawn again (the generator's own
    assert, here over every structure at once)."""
    stats = {}
    for kind in KINDS:
        rng = np.random.default_rng(31)
        rp, _ = ac.build_csr(ac.batch_rows(kind, 9, 48, rng), 48)
        w = ac.draw_weights("signed", rp, rng, stats)
        den = np.array([w[a:b].astype(np.float64).sum() + 1.0 for a, b in zip(rp[:-1], rp[1:])])
        assert den.min() >= ac.MIN_DEN and w.dtype == np.float32 and (w < 0).mean() > 0.05
    print("signed rows drawn again: %d of %d" % (stats["rejected"], stats["rows"]))
    assert stats["rejected"] * 20 < stats["rows"]
    w = ac.draw_weights("positive", rp, np.random.default_rng(1))
    assert w.min() >= 0.25 and w.max() < 2.0 and ac.draw_weights("ones", rp, rng) is None
    assert set(np.unique(ac.draw_weights("exact", rp, rng)).tolist()) == {0.5, 1.0, 2.0}


def _fma32(w, x, acc):
    """fp32 fused multiply-add: the product of two floats is exact in float64; the sum's double rounding is beyond 2^-29."""
    return (np.float64(w) * x.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)


def _eval32(c, order, gates=True):
    """The formula in float32, row by row: ``order`` "forward" (CSR order), "reversed", or "four" (four partial sums over the
    entries e = 0, 1, 2, 3 mod 4, then (s0 + s1) + (s2 + s3)); the reciprocal, the multiply, the bias add and each gate
    multiply round once."""
    f32 = np.float32
    h, rp, ci, vals, T = c["h"], c["rowptr"], c["colidx"], c["vals"], c["T"]
    N, F = h.shape
    y = np.zeros((N, F), dtype=f32)
    for i in range(N):
        es = list(range(rp[i], rp[i + 1]))
        if order == "reversed":
            es = es[::-1]
        lanes = [es[k::4] for k in range(4)] if order == "four" else [es]
        accs, dens = [], []
        for lane in lanes:
            acc, d = np.zeros(F, dtype=f32), f32(0.0)
            for e in lane:
                w = f32(1.0) if vals is None else vals[e]
                acc = _fma32(w, h[ci[e]], acc)
                d = f32(d + w)
            accs.append(acc)
            dens.append(d)
        if order == "four":
            acc = ((accs[0] + accs[1]).astype(f32) + (accs[2] + accs[3]).astype(f32)).astype(f32)
            d = f32(f32(dens[0] + dens[1]) + f32(dens[2] + dens[3]))
        else:
            acc, d = accs[0], dens[0]
        inv = f32(f32(1.0) / f32(d + f32(1.0)))
        y[i] = ((acc * inv).astype(f32) + (c["bias"] if c["bias"] is not None else f32(0.0))).astype(f32)
    B = c["B"]
    per_row = lambda g: np.repeat(g, T, axis=0)                                          # noqa: E731
    out = (y * per_row(c["sg"])).astype(f32)
    pa = (y * per_row(c["ga"])).astype(f32).reshape(B, T, F).max(axis=1)
    pb = (y * per_row(c["gb"])).astype(f32).reshape(B, T, F).max(axis=1)
    return out, pa, pb


def _worst(got, ref, bound):
    err = np.abs(got.astype(np.float64) - ref)
    assert not np.isnan(err).any()
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / bound, 0.0)
    return float(ratio.max())


@pytest.mark.parametrize("weights", ac.WEIGHTS)
@pytest.mark.parametrize("kind", KINDS + ("cap",))
def test_float32_in_three_orders_stays_inside_the_bound(kind, weights):
    """Every generator of the GPU tests: a float32 evaluation in CSR order, reversed and in four partial sums is inside the derived
    bound on every element of out (float32 and rounded to half) and of both pools -- no factor, no floor."""
    if kind == "cap":
        B, T, F = 2, 333, 2
    else:
        B, T, F = (9, 21, 6) if kind == "mixed" else (3, 37, 6)
    c = ac.make_case(kind, weights, B, T, F, seed=17, half=True)
    r, rh = _ref(c), _ref(c, half_out=True)
    worst32 = worst16 = 0.0
    for order in ("forward", "reversed", "four"):
        out, pa, pb = _eval32(c, order)
        worst32 = max(worst32, _worst(out, r["out"], r["bound_out"]), _worst(pa, r["pool_a"], r["bound_pool_a"]),
                      _worst(pb, r["pool_b"], r["bound_pool_b"]))
        worst16 = max(worst16, _worst(out.astype(np.float16), rh["out"], rh["bound_out"]))
    print("  %s/%s: worst err / bound  fp32 %.3f  half %.3f" % (kind, weights, worst32, worst16))
    assert worst32 <= 1.0 and worst16 <= 1.0


@pytest.mark.parametrize("weights", ["ones", "exact"])
def test_exact_sums_leave_four_roundings(weights):
    """Integer features in [-8, 8] and weights in {0.5, 1, 2}: the fp32 sums are exact in every order (the three orders agree bit
    for bit before the division), and without a bias the result is within 4 u |ref|."""
    c = ac.make_case("mixed", "positive" if weights == "exact" else "ones", 9, 21, 6, seed=23, exact=True)
    c["bias"] = None
    S, A, den, dabs, n = row_sums(c["h"], c["rowptr"], c["colidx"], c["vals"])
    assert np.array_equal(S, S.astype(np.float32)) and np.array_equal(den, den.astype(np.float32)) and np.abs(S).max() > 8
    r = aggregate_ref(c["h"], c["rowptr"], c["colidx"], c["vals"], None, 9, 21, c["sg"], c["ga"], c["gb"])
    outs = [_eval32(c, order) for order in ("forward", "reversed", "four")]
    for o in outs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(o, outs[0]))
    out, pa, pb = outs[0]
    assert _worst(out, r["out"], exact_bound(r["out"])) <= 1.0
    assert _worst(out.astype(np.float16), r["out"], exact_bound(r["out"], half_out=True)) <= 1.0
    assert _worst(pa, r["pool_a"], exact_pool_bound(r["y"], c["ga"], 9, 21)) <= 1.0
    assert _worst(pb, r["pool_b"], exact_pool_bound(r["y"], c["gb"], 9, 21)) <= 1.0
