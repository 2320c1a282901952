"""ggcn_aggregate and ggcn_aggregate_h called at the C ABI, on every launch form, against the float64 statement of
oracle/aggregate_ref.py and ITS derived bound (no factor, no floor) -- the fallback of the whole forward pass, which the layer
tests only reach behind a linear whose gate is a thousand times wider than the neighbour sums' error.

The CSR is built in numpy by oracle/aggregate_cases.py, so duplicate and unsorted columns reach the kernel as drawn.  Every case
runs twice into fresh hostile buffers (NaN pad columns and a NaN row in Hd, out with ldo > F between guard bands, pools between
guard bands): the two runs are bit-equal, every byte outside [N,F] / [B,F] is bit-unchanged and nothing inside is NaN.

Which form a shape takes follows csrc/aggregate.hip: ``aggregate`` / ``aggregate_h`` (16- / 8-byte accesses when F, the leading
dimensions and every pointer allow, else one column per thread), ``launch`` (LDS-tiled for T <= 48 with vector accesses, else
chunks of 16 rows: more than one chunk combines the pools through integer atomics), ``launch_narrow`` (half, 48 < T <= 768,
F % 8 == 0, everything 16-byte aligned: 4 wavefronts x 8 steps below 256 rows, 8 x 8 up to 512, 8 x 12 up to 768).
"""
import numpy as np
import pytest
import torch

from oracle import aggregate_cases as ac
from oracle import gates
from oracle.aggregate_ref import aggregate_ref, exact_bound, exact_pool_bound
from oracle.gpu_support import dev, pkg  # noqa: F401

pytestmark = pytest.mark.gpu

GUARD = 8          # elements of NaN on either side of an output: 16 bytes of half, 32 of float -- the views stay 16-byte aligned
WORST = {}         # entry -> worst err / bound seen (printed when the module is done)


@pytest.fixture(scope="module", autouse=True)
def worst_ratios():
    yield
    for k in sorted(WORST):
        print("\n  worst err / bound over the module, %s: %.3f" % (k, WORST[k]))


# ---------------------------------------------------------------------------------------------------------------- the forms
# (id, entry, T, F, B, layout).  entry "f": ggcn_aggregate, "h": ggcn_aggregate_h.  layout: hd_pad (columns of NaN behind a row
# of Hd; default 8, which keeps 16-byte rows of either type), hd_off (Hd starts that many elements into its buffer), bias_off /
# gate_off (bias / the three gates sliced at that element of a larger buffer).
def _forms():
    f = []
    for T in (1, 5, 47, 48):                                  # tiled, 16-byte; F = 260: the second slab has one live lane
        f.append(("f32-tiled-T%d" % T, "f", T, 260, 3, {}))
    for T in (9, 16):                                         # one column per thread, one chunk: pools written directly
        f.append(("f32-scalar-F7-T%d" % T, "f", T, 7, 3, {}))
        f.append(("f32-scalar-ldh9-T%d" % T, "f", T, 8, 3, {"hd_pad": 1}))
        f.append(("f32-scalar-hdoff-T%d" % T, "f", T, 8, 3, {"hd_off": 1}))
        f.append(("f32-scalar-biasoff-T%d" % T, "f", T, 8, 3, {"bias_off": 1}))
    for T in (17, 48):                                        # one column per thread is never tiled: 2 / 3 chunks, pools by atomics
        f.append(("f32-scalar-chunked-T%d" % T, "f", T, 70, 3, {}))
    for T in (49, 64, 100):                                   # 16-byte chunks: a last chunk of 1 / 16 / 4 rows
        for B in (1, 8, 9):                                   # B % 8 != 0: ghost workgroups
            f.append(("f32-chunked-T%d-B%d" % (T, B), "f", T, 260, B, {}))
    for T in (513, 769):                                      # 33 / 49 chunks
        f.append(("f32-chunked-T%d" % T, "f", T, 8, 2, {}))
    for T in (5, 48):                                         # tiled, 8-byte half
        f.append(("f16-tiled-T%d" % T, "h", T, 264, 3, {}))
    for T in (49, 255):                                       # narrow, 4 wavefronts x 8 steps; F = 72: the second slab has one live piece
        for F in (8, 72, 136):
            for B in (3, 9):
                f.append(("f16-narrow4x8-T%d-F%d-B%d" % (T, F, B), "h", T, F, B, {}))
    for T in (256, 512):
        f.append(("f16-narrow8x8-T%d" % T, "h", T, 72, 3, {}))
    for T in (513, 768):
        for B in (2, 9):
            f.append(("f16-narrow8x12-T%d-B%d" % (T, B), "h", T, 72, B, {}))
    f.append(("f16-chunked-T769", "h", 769, 72, 3, {}))       # beyond the narrow window
    f.append(("f16-chunked8B-T300-F12", "h", 300, 12, 3, {"hd_pad": 4}))      # F % 8 != 0 falls out of narrow: 8-byte chunks
    f.append(("f16-scalar-T300-F13", "h", 300, 13, 3, {"hd_pad": 3}))
    f.append(("f16-scalar-gateoff-T300-F72", "h", 300, 72, 3, {"gate_off": 1}))
    return f


FORMS = _forms()
FORM = {f[0]: f for f in FORMS}
FORM_IDS = [f[0] for f in FORMS]
# one tiled, one chunked with atomics in each access width, one narrow, one chunked half: what the structures and epilogues go through
THROUGH = ("f32-tiled-T47", "f32-scalar-chunked-T17", "f32-chunked-T100-B9", "f16-narrow4x8-T255-F72-B3", "f16-chunked-T769")
ALL = ("bias", "sg", "ga", "gb")


# ------------------------------------------------------------------------------------------------------------- the launcher
def _at(t, off, dev):
    """t as a contiguous view ``off`` elements into a NaN buffer of its own."""
    buf = torch.full((t.numel() + off,), gates.NAN, dtype=t.dtype, device=dev)
    v = buf[off:].view(t.shape)
    v.copy_(t)
    return v


def _features(c, half, lay, dev):
    """(view [N,F] handed to the library, ldh): NaN pad columns and a NaN row behind the last."""
    h = torch.from_numpy(c["h"]).to(dev)
    h = h.half() if half else h
    assert torch.equal(h.float().cpu(), torch.from_numpy(c["h"]))
    pad, off = lay.get("hd_pad", 8), lay.get("hd_off", 0)
    if off:
        N, F = h.shape
        buf = torch.full((off + (N + 1) * F,), gates.NAN, dtype=h.dtype, device=dev)
        v = buf[off:].view(N + 1, F)
        v[:N] = h
        assert v.data_ptr() % 16 == off * h.element_size()
        return v, F
    v = gates.hostile(h, pad)
    return v, v.shape[1]


def _untouched_and_clean(buf, snap, view_rows, ld, F, what):
    """Every element of ``buf`` outside the first F columns of the rows x ld view behind the guard band is bit-unchanged, every
    element inside is no NaN."""
    bits = torch.int16 if buf.dtype == torch.float16 else torch.int32
    inside = torch.zeros(buf.numel(), dtype=torch.bool, device=buf.device)
    inside[GUARD:GUARD + view_rows * ld].view(view_rows, ld)[:, :F] = True
    assert torch.equal(buf.view(bits)[~inside], snap.view(bits)[~inside]), "%s: a byte outside the result changed" % what
    assert not bool(torch.isnan(buf[inside]).any()), "%s: NaN inside the result" % what


def _run(pkg, dev, entry, c, lay=None, use=ALL, want=("out", "pa", "pb")):
    """Two launches into fresh hostile buffers -> {"out" [N,F], "pa", "pb" [B,F]} as numpy (float32 / float16), after the
    bit-equality, the guard bands and the NaN check."""
    from ed_gated_gcn_amd import _capi
    lib = pkg.load_library()
    lay = lay or {}
    half = entry == "h"
    fn, name = (lib.ggcn_aggregate_h, "ggcn_aggregate_h") if half else (lib.ggcn_aggregate, "ggcn_aggregate")
    B, T, F = c["B"], c["T"], c["F"]
    N = B * T
    hd, ldh = _features(c, half, lay, dev)
    rowptr, colidx = torch.from_numpy(c["rowptr"]).to(dev), torch.from_numpy(c["colidx"]).to(dev)
    if colidx.numel() == 0:
        colidx = torch.zeros(1, dtype=torch.int32, device=dev)        # a pointer, never read
    vals = None if c["vals"] is None else torch.from_numpy(c["vals"]).to(dev)
    side = {}
    for k in ALL:
        off = lay.get("bias_off" if k == "bias" else "gate_off", 0)
        side[k] = _at(torch.from_numpy(c[k]), off, dev) if k in use else None
        assert side[k] is None or side[k].data_ptr() % 16 == 4 * off
    ldo = F + 8
    runs = []
    for _ in range(2):
        o = gates.poisoned_rows(dev, N, ldo, GUARD, dtype=torch.float16 if half else torch.float32) if "out" in want else None
        pa = gates.poisoned_rows(dev, B, F, GUARD) if "pa" in want else None
        pb = gates.poisoned_rows(dev, B, F, GUARD) if "pb" in want else None
        snaps = [None if x is None else x[0].clone() for x in (o, pa, pb)]
        hd_snap = hd.clone()
        _capi.check(fn(_capi.ptr(hd), ldh, _capi.ptr(rowptr), _capi.ptr(colidx), _capi.ptr(vals), _capi.ptr(side["bias"]), B, T, F,
                       _capi.ptr(side["sg"]), _capi.ptr(side["ga"]), _capi.ptr(side["gb"]), None if o is None else _capi.ptr(o[1]),
                       ldo, None if pa is None else _capi.ptr(pa[1]), None if pb is None else _capi.ptr(pb[1]),
                       _capi.stream_of(dev)), name)
        torch.cuda.synchronize(dev)
        bits = torch.int16 if half else torch.int32
        assert torch.equal(hd.view(bits), hd_snap.view(bits)), "Hd was written"
        for x, snap, rows, ld, what in ((o, snaps[0], N, ldo, "out"), (pa, snaps[1], B, F, "pool_a"), (pb, snaps[2], B, F, "pool_b")):
            if x is not None:
                _untouched_and_clean(x[0], snap, rows, ld, F, what)
        runs.append({"out": None if o is None else o[1][:, :F], "pa": None if pa is None else pa[1], "pb": None if pb is None else pb[1]})
    got = {}
    for k in ("out", "pa", "pb"):
        a, b = runs[0][k], runs[1][k]
        if a is not None:
            assert torch.equal(a.view(torch.int16 if a.dtype == torch.float16 else torch.int32),
                               b.view(torch.int16 if b.dtype == torch.float16 else torch.int32)), "%s differs between two runs" % k
            got[k] = a.cpu().numpy()
    return got


def _hold(entry, got, ref, bound, what):
    """|got - ref| <= bound on every element; prints and records the worst err / bound."""
    err = np.abs(got.astype(np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / bound, 0.0)
    worst = float(ratio.max()) if ratio.size else 0.0
    print("  %s: worst err / bound %.3f" % (what, worst))
    bad = ~(err <= bound)
    if bad.any():
        i = np.unravel_index(int(np.argmax(np.where(bad, ratio, -1.0))), err.shape)
        raise AssertionError("%s: %d elements outside the bound, worst at %s: got %r, ref %r, |diff| %.3g > %.3g" % (
            what, int(bad.sum()), i, float(got[i]), float(ref[i]), float(err[i]), float(bound[i])))
    key = {"f": "ggcn_aggregate", "h": "ggcn_aggregate_h"}[entry] + (" pools" if what.split()[-1] != "out" else " out")
    WORST[key] = max(WORST.get(key, 0.0), worst)


def _check(entry, c, got, use=ALL, tag=""):
    """Every result that was asked for against the statement and its bound."""
    p = {k: (c[k] if k in use else None) for k in ALL}
    r = aggregate_ref(c["h"], c["rowptr"], c["colidx"], c["vals"], p["bias"], c["B"], c["T"], p["sg"], p["ga"], p["gb"],
                      half_out=entry == "h")
    for k, name in (("out", "out"), ("pa", "pool_a"), ("pb", "pool_b")):
        if k in got:
            assert got[k].dtype == (np.float16 if entry == "h" and k == "out" else np.float32)
            _hold(entry, got[k], r[name], r["bound_" + name], "%s %s" % (tag, name))
    return r


def _seed(*parts):
    return sum((i + 1) * sum(map(ord, str(p))) for i, p in enumerate(parts)) % (2 ** 31)


# ------------------------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("weights", ac.WEIGHTS)
@pytest.mark.parametrize("form", FORM_IDS)
def test_every_form_vs_float64(pkg, dev, form, weights):
    """Each row of the table of forms, on a batch whose graph g has structure g % 6 (consecutive degrees 0..9, hub row and hub
    column, no edge at all, self loops, padding rows, duplicate and unsorted columns), 0/1, weighted and signed, with the bias,
    the three gates (gate_a in [-1, 1]) and both pools."""
    _, entry, T, F, B, lay = FORM[form]
    c = ac.make_case("mixed", weights, B, T, F, _seed(form, weights), half=entry == "h")
    _check(entry, c, _run(pkg, dev, entry, c, lay), tag=form)


@pytest.mark.parametrize("weights", ac.WEIGHTS)
@pytest.mark.parametrize("form", THROUGH)
@pytest.mark.parametrize("kind", ac.STRUCTURES)
def test_every_structure_through_tiled_chunked_and_narrow(pkg, dev, kind, form, weights):
    """Each structure in every graph of the batch (the edgeless graph: one among graphs that have edges)."""
    _, entry, T, F, B, lay = FORM[form]
    c = ac.make_case(kind, weights, B, T, F, _seed(kind, form, weights), half=entry == "h")
    _check(entry, c, _run(pkg, dev, entry, c, lay), tag="%s %s" % (kind, form))


@pytest.mark.parametrize("weights", ac.WEIGHTS)
def test_narrow_form_at_its_staging_capacity(pkg, dev, weights):
    """333 nodes: a graph with exactly the 4096 edges whose column ids the narrow form stages in LDS, one with 4097 (ids read
    from global memory) and a sparse one, in one launch."""
    c = ac.make_case("cap", weights, 3, 333, 72, _seed("cap", weights), half=True)
    rp = c["rowptr"]
    assert rp[333] == ac.IDX_CAP and rp[666] - rp[333] == ac.IDX_CAP + 1
    _check("h", c, _run(pkg, dev, "h", c), tag="cap")


def _epilogue(variant, c):
    """(use, want) of an epilogue variant; may edit the case."""
    if variant == "zero-gate-columns":
        c["sg"][:, 1], c["ga"][:, 2], c["gb"][:, 0] = 0.0, 0.0, 0.0
        return ALL, ("out", "pa", "pb")
    if variant == "negative-y":       # a max that starts from, or loses to, -inf shows; the zero column makes every candidate -0.0
        c["gb"][:, 0] = 0.0
        c["ga"] = np.abs(c["ga"]) + np.float32(0.125)
        return ALL, ("out", "pa", "pb")
    return {
        "all-gates": (ALL, ("out", "pa", "pb")),
        "pool-gates-null": (("bias", "sg"), ("out", "pa", "pb")),        # pool_gate_x = NULL with the pool wanted: a gate of ones
        "only-pool-b": (("bias", "gb"), ("pb",)),
        "pools-only": (("bias", "ga", "gb"), ("pa", "pb")),              # out = NULL
        "no-bias": (("sg", "ga", "gb"), ("out", "pa", "pb")),
        "out-only": (("bias", "sg"), ("out",)),
    }[variant]


@pytest.mark.parametrize("form", THROUGH)
@pytest.mark.parametrize("variant", ["all-gates", "zero-gate-columns", "pool-gates-null", "only-pool-b", "pools-only", "no-bias",
                                     "out-only", "negative-y"])
def test_epilogue_vs_float64(pkg, dev, variant, form):
    """Gates present and absent, exact zeros in a gate, pools without out and out without pools, no bias, and a y that is
    negative everywhere (so that -inf, the preset of the atomics and the initial value of the others, is what a wrong max
    returns; with a zero gate column every candidate of that column is -0.0)."""
    _, entry, T, F, B, lay = FORM[form]
    c = ac.make_case("mixed", "positive", B, T, F, _seed(variant, form), half=entry == "h", negative=variant == "negative-y")
    use, want = _epilogue(variant, c)
    got = _run(pkg, dev, entry, c, lay, use=use, want=want)
    assert set(got) == set(want)
    r = _check(entry, c, got, use=use, tag="%s %s" % (variant, form))
    if variant == "negative-y":
        assert r["y"].max() < 0 and r["pool_a"].max() < 0 and not r["pool_b"][:, 0].any()
        assert np.isfinite(got["pa"]).all() and np.isfinite(got["pb"]).all() and not got["pb"][:, 0].any()


@pytest.mark.parametrize("form", FORM_IDS)
def test_exact_sums_on_every_form(pkg, dev, form):
    """Integer features in [-8, 8], weights in {0.5, 1, 2} (every third form 0/1), no bias: the fp32 sums are exact in any order,
    so the gate is 4 u |ref| (plus the half rounding of a half out) -- a dropped, doubled or misplaced edge that carries a
    feature other than 0 moves a row by at least 0.5 / (2 T + 1) of a unit, thousands of times that."""
    i = FORM_IDS.index(form)
    _, entry, T, F, B, lay = FORM[form]
    c = ac.make_case("mixed", "ones" if i % 3 == 2 else "positive", B, T, F, _seed("exact", form), half=entry == "h", exact=True)
    use = ("sg", "ga", "gb")
    got = _run(pkg, dev, entry, c, lay, use=use)
    r = aggregate_ref(c["h"], c["rowptr"], c["colidx"], c["vals"], None, B, T, c["sg"], c["ga"], c["gb"])
    _hold(entry, got["out"], r["out"], exact_bound(r["out"], half_out=entry == "h"), "exact %s out" % form)
    _hold(entry, got["pa"], r["pool_a"], exact_pool_bound(r["y"], c["ga"], B, T), "exact %s pool_a" % form)
    _hold(entry, got["pb"], r["pool_b"], exact_pool_bound(r["y"], c["gb"], B, T), "exact %s pool_b" % form)


REFUSALS = {
    "null-Hd": (dict(hd=None), "ggcn_aggregate: null input pointer"),
    "null-rowptr": (dict(rowptr=None), "ggcn_aggregate: null input pointer"),
    "B0": (dict(B=0), "ggcn_aggregate: B=0 T=5 F=8 must be positive"),
    "T0": (dict(T=0), "ggcn_aggregate: B=2 T=0 F=8 must be positive"),
    "F0": (dict(F=0), "ggcn_aggregate: B=2 T=5 F=0 must be positive"),
    "no-output": (dict(out=None, pa=None, pb=None), "ggcn_aggregate: no output requested"),
    "ldh-below-F": (dict(ldh=7), "ggcn_aggregate: leading dimension smaller than F=8"),
    "ldo-below-F": (dict(ldo=7), "ggcn_aggregate: leading dimension smaller than F=8"),
}


@pytest.mark.parametrize("entry", ["f", "h"])
@pytest.mark.parametrize("what", list(REFUSALS))
def test_refusals_say_why_and_write_nothing(pkg, dev, what, entry):
    """Both entries share one argument check: the return code is not 0, ggcn_last_error() holds the text, no output changes."""
    from ed_gated_gcn_amd import _capi
    lib = pkg.load_library()
    change, text = REFUSALS[what]
    c = ac.make_case("self", "ones", 2, 5, 8, 3, half=entry == "h")
    h = torch.from_numpy(c["h"]).to(dev)
    dt = torch.float16 if entry == "h" else torch.float32
    a = dict(hd=h.to(dt), ldh=8, rowptr=torch.from_numpy(c["rowptr"]).to(dev), colidx=torch.from_numpy(c["colidx"]).to(dev),
             B=2, T=5, F=8, out=torch.full((10, 8), gates.NAN, dtype=dt, device=dev), ldo=8,
             pa=torch.full((2, 8), gates.NAN, device=dev), pb=torch.full((2, 8), gates.NAN, device=dev))
    a.update(change)
    fn = lib.ggcn_aggregate_h if entry == "h" else lib.ggcn_aggregate
    p = _capi.ptr
    rc = fn(p(a["hd"]), a["ldh"], p(a["rowptr"]), p(a["colidx"]), None, None, a["B"], a["T"], a["F"], None, None, None,
            p(a["out"]), a["ldo"], p(a["pa"]), p(a["pb"]), _capi.stream_of(dev))
    assert rc != 0
    assert lib.ggcn_last_error().decode() == text
    with pytest.raises(RuntimeError, match="ggcn_aggregate"):
        _capi.check(rc, "ggcn_aggregate")
    torch.cuda.synchronize(dev)
    for k in ("out", "pa", "pb"):
        assert a[k] is None or bool(torch.isnan(a[k]).all()), k
