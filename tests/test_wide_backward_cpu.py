"""Host side of the one-launch backward for 0/1 graphs of 33..128 nodes (``ggcn_rowmask_transpose_wide`` +
``ggcn_gate_pool_backward_wide``, include/ggcn.h; opt-in ``GraphConvolution.wide_backward``), on a machine without a GPU:

* the option and its environment switch; header, ``_capi`` and library agree on the two entries and on ABI 14;
* every refusal of the two entries, exact texts (each check comes before a launch: the pointers handed in are never
  dereferenced);
* ``dispatch.takes_wide_backward`` on stand-in graphs that log what they are asked, and ``dispatch.backward_launch`` against
  ``backward_plan`` on a grid with the option off and on;
* the numpy statement of the transposed masks the GPU test compares the builder with;
* the numpy emulation of the kernel's arithmetic (``wide_backward_ref.emulate``) against the float64 statement on every C-ABI case
  of ``tests/test_gpu_wide_backward.py``: inside the derived bounds of ``wide_backward_ref`` with a factor of at least 4 to spare
  for dH, d_sg and d_bsum.  Measured here: dH 0.092, d_sg 0.024, d_bsum 0.021 of their bounds at the worst element.  d_ga and d_gb
  are single products whose bound 4 u |ref| is a count of their three roundings (1.5 u at worst): no factor of 4 can be there, the
  emulation is at 0.275 of it, and they are held to the bound itself -- the one the GPU file applies;
* the tie condition (``br.MAX_MASKED``) of the autograd inputs the GPU file adds, on the float64 reference alone.
"""
import ctypes
import itertools
import types

import numpy as np
import pytest
import torch

import ed_gated_gcn_amd as pkg
import wide_backward_ref as wb
from ed_gated_gcn_amd import _capi, dispatch
from ed_gated_gcn_amd.gcn import GraphConvolution
from oracle import backward_ref as br
from oracle import gates
from oracle.host_support import header as _header, msg as _msg

EINVAL, EUNSUPPORTED = 1, 3
P = ctypes.c_void_p(1 << 20)   # non-null, 16-byte aligned, never dereferenced
ODD = ctypes.c_void_p((1 << 20) + 4)
H = 64
BUILD, WIDE = "ggcn_rowmask_transpose_wide", "ggcn_gate_pool_backward_wide"
DROP = (0.25, 7, (0, 1, 2))


@pytest.fixture(autouse=True)
def _no_env(monkeypatch):
    for k in ("GGCN_WIDE_BACKWARD", "GGCN_WEIGHTED_BACKWARD", "GGCN_BACKWARD_TWO_PASS", "GGCN_BACKWARD_SCALAR", "GGCN_DX_PRECISION"):
        monkeypatch.delenv(k, raising=False)


# ---------------------------------------------------------------- the option and the surface
def _layer(on=True, precision="f16mx8"):
    opt = types.SimpleNamespace(ggcn_precision=precision)
    if on is not None:
        opt.ggcn_wide_backward = on
    return GraphConvolution(H, H, opt=opt)


def test_option_is_off_by_default(monkeypatch):
    assert GraphConvolution(H, H).wide_backward is False and _layer(None).wide_backward is False
    assert _layer(True).wide_backward is True and _layer(False).wide_backward is False
    monkeypatch.setenv("GGCN_WIDE_BACKWARD", "1")
    assert GraphConvolution(H, H).wide_backward is True
    monkeypatch.setenv("GGCN_WIDE_BACKWARD", "0")
    assert GraphConvolution(H, H).wide_backward is False


def test_declared_bound_exported_and_abi_stays_14():
    lib = ctypes.CDLL(pkg.lib_path())
    header = _header()
    for name in (BUILD, WIDE):
        assert name + "(" in header and name in _capi.PROTOTYPES and hasattr(lib, name), name
    assert "#define GGCN_ABI_VERSION 14" in header and _capi.ABI_VERSION == 14 and pkg.load_library().ggcn_abi_version() == 14
    # the builder's arguments are ggcn_rowmask_transpose's; the kernel's are ggcn_gate_pool_backward_weighted's without (dY, ldy)
    proto = lambda n: _capi.PROTOTYPES[n][1]     # noqa: E731
    assert proto(BUILD) == proto("ggcn_rowmask_transpose")
    weighted = proto("ggcn_gate_pool_backward_weighted")
    assert proto(WIDE) == weighted[:16] + weighted[18:]
    assert not any(n.startswith(WIDE + "_") for n in _capi.PROTOTYPES)            # no form under gate dropout
    assert "wide" in dispatch.BACKWARD_LAUNCHES and "wide" not in dispatch.BACKWARD_PASSES
    from ed_gated_gcn_amd import gcn
    assert gcn._BACKWARD_LAUNCHES["wide"][0] == WIDE and gcn._BACKWARD_LAUNCHES["wide"][2:] == ("dH", ())
    assert set(gcn._BACKWARD_LAUNCHES) == set(dispatch.BACKWARD_LAUNCHES)


def test_builder_refusals():
    lib = pkg.load_library()

    def build(src=P, B=4, T=100, dst=P):
        return lib.ggcn_rowmask_transpose_wide(src, B, T, dst, None)
    assert _msg(lib, build(src=None), EINVAL) == BUILD + ": null pointer"
    assert _msg(lib, build(dst=None), EINVAL) == BUILD + ": null pointer"
    assert _msg(lib, build(B=0), EINVAL) == BUILD + ": B=0 T=100 must be positive"
    assert _msg(lib, build(T=-1), EINVAL) == BUILD + ": B=4 T=-1 must be positive"
    for T in (1, 32):
        assert _msg(lib, build(T=T), EUNSUPPORTED) == BUILD + ": T=%d <= 32; use ggcn_rowmask_transpose" % T
    for T in (129, 256):
        assert _msg(lib, build(T=T), EUNSUPPORTED) == BUILD + ": T=%d > 128 (four words per node)" % T


def test_kernel_refusals():
    lib, who = pkg.load_library(), WIDE

    def run(out=P, ldo=H, d_out=P, ldd=H, mt=P, inv=P, B=4, T=100, F=H, dh=P, ldh=H):
        return getattr(lib, who)(out, ldo, P, P, P, d_out, ldd, P, P, mt, inv, B, T, F, dh, ldh, P, P, P, P, None)
    for kw in (dict(out=None), dict(dh=None), dict(mt=None), dict(inv=None)):
        assert _msg(lib, run(**kw), EINVAL) == who + ": null pointer", kw
    assert _msg(lib, run(B=0), EINVAL) == who + ": B=0 T=100 F=64 must be positive"
    assert _msg(lib, run(T=0), EINVAL) == who + ": B=4 T=0 F=64 must be positive"
    assert _msg(lib, run(F=-4), EINVAL) == who + ": B=4 T=100 F=-4 must be positive"
    for T in (1, 32):
        assert _msg(lib, run(T=T), EUNSUPPORTED) == who + ": T=%d <= 32; use ggcn_gate_pool_backward_mma" % T
    for T in (129, 231):
        assert _msg(lib, run(T=T), EUNSUPPORTED) == who + ": T=%d > 128; use ggcn_gate_pool_backward + ggcn_aggregate_t" % T
    for kw in (dict(ldo=H - 4), dict(ldh=H - 4), dict(ldd=H - 4)):
        assert _msg(lib, run(**kw), EINVAL) == who + ": leading dimension smaller than F=64", kw
    # an absent d_out takes ldd out of the checks: the call is refused by a later one
    assert _msg(lib, run(d_out=None, ldd=0, dh=ODD), EUNSUPPORTED).startswith(who + ": needs F % 4 == 0")
    big = (1 << 31) // (4 * 128)                        # T = 100 is four blocks = 128 rows: 128 * ld * 4 >= 2 GiB
    for kw in (dict(ldo=big), dict(ldh=big), dict(ldd=big), dict(ldo=(1 << 31) // 400 + 1)):
        assert _msg(lib, run(**kw), EUNSUPPORTED) == who + ": a graph's rows exceed 2 GiB", kw
    align = who + ": needs F % 4 == 0, ldh % 4 == 0 and 16-byte aligned dH / rowmask_t; use ggcn_gate_pool_backward + ggcn_aggregate_t"
    for kw in (dict(F=30, ldo=30, ldd=30, ldh=32), dict(ldh=H + 2), dict(dh=ODD), dict(mt=ODD)):
        assert _msg(lib, run(**kw), EUNSUPPORTED) == align, kw


# ---------------------------------------------------------------- the predicate
def _graph(T=100, binary=True, masks=True, B=4):
    """A stand-in for a BatchedCSR that logs every attribute the predicate reads."""
    asked = []

    class Graph:
        def __getattr__(self, name):
            asked.append(name)
            values = {"T": T, "B": B, "is_binary": binary, "rowmask_t_wide": types.SimpleNamespace(is_cuda=True) if masks else None}
            if name not in values:
                raise AttributeError(name)
            return values[name]
    g = Graph()
    g.__dict__["asked"] = asked
    return g


def _operands(offset=0):
    t = types.SimpleNamespace(data_ptr=lambda: (1 << 20) + offset)
    return (types.SimpleNamespace(data_ptr=lambda: 1 << 20), None, t, None)


def _takes(layer=None, csr=None, B=4, F=H, dropout=None, operands=None):
    return dispatch.takes_wide_backward(layer or _layer(), csr, B, F, dropout, operands or _operands())


def test_option_off_asks_nothing():
    for layer in (_layer(False), _layer(None), types.SimpleNamespace(precision="f16mx8")):      # (the last: a layer that predates the option)
        g = _graph()
        log = []
        ops = (types.SimpleNamespace(data_ptr=lambda: (log.append("ptr"), 1 << 20)[1]),)
        assert dispatch.takes_wide_backward(layer, g, 4, H, None, ops) is False
        assert g.asked == [] and log == []


def test_predicate_holds_and_each_condition_alone_turns_it_off(monkeypatch):
    for T in (33, 64, 65, 100, 128):
        g = _graph(T)
        assert _takes(csr=g) is True
        assert g.asked.count("rowmask_t_wide") == 1 and g.asked[-1] == "rowmask_t_wide", g.asked      # asked once, last
    cases = {
        "a real-valued adjacency": dict(csr=_graph(binary=False)),
        "T = 32": dict(csr=_graph(32)),
        "T = 1": dict(csr=_graph(1)),
        "T = 129": dict(csr=_graph(129)),
        "F = 30": dict(F=30),
        "a 4-byte aligned operand": dict(operands=_operands(4)),
        "gate dropout": dict(dropout=DROP),
    }
    for what, kw in cases.items():
        g = kw.pop("csr", None) or _graph()
        assert _takes(csr=g, **kw) is False, what
        assert "rowmask_t_wide" not in g.asked, "%s: the graph was asked for its masks" % what
    assert _takes(csr=_graph(128), B=2 ** 32 // (128 * H)) is True          # (no element index without dropout: any batch size)
    g = _graph(masks=False)                                        # no row masks on the GPU: asked, and the answer is None
    assert _takes(csr=g) is False and g.asked[-1] == "rowmask_t_wide"
    monkeypatch.setenv("GGCN_BACKWARD_TWO_PASS", "1")
    g = _graph()
    assert _takes(csr=g) is False and "rowmask_t_wide" not in g.asked
    monkeypatch.setenv("GGCN_BACKWARD_TWO_PASS", "0")
    assert _takes(csr=_graph()) is True


# ---------------------------------------------------------------- backward_launch against backward_plan
def _plan_graph(T, binary, masks, wide=True):
    on_gpu = types.SimpleNamespace(is_cuda=True)
    g = types.SimpleNamespace(T=T, B=4, is_binary=binary, rowmask=on_gpu if masks else None, graph_ops=on_gpu, graph_ops_t=on_gpu,
                              graph_ops_weighted_t=lambda: None)
    if wide:      # (without: a stand-in of the existing tests, which has no such attribute)
        g.rowmask_t_wide = on_gpu if (binary and masks and 32 < T <= 128) else None
    return g


def _grid():
    for T, binary, masks, F, dropout, need_adj, offset, two_pass, dtype, precision in itertools.product(
            (24, 32, 33, 64, 100, 128, 129, 231), (True, False), (True, False), (64, 30, 256), (None, DROP), (False, True), (0, 4),
            (False, True), (torch.float32, torch.bfloat16), ("f16mx8", "fp32")):
        yield T, binary, masks, F, dropout, need_adj, offset, two_pass, dtype, precision


def test_backward_launch_is_backward_plan_with_the_option_off(monkeypatch):
    n = 0
    for T, binary, masks, F, dropout, need_adj, offset, two_pass, dtype, precision in _grid():
        monkeypatch.setenv("GGCN_BACKWARD_TWO_PASS", "1" if two_pass else "0")
        for layer in (_layer(False, precision), _layer(None, precision)):
            g = _plan_graph(T, binary, masks, wide=False)
            args = (True, need_adj, dropout, _operands(offset))
            assert dispatch.backward_launch(layer, g, dtype, 4, H, F, *args) == dispatch.backward_plan(layer, g, dtype, H, F, *args)
            n += 1
    assert n == 2 * 8 * 2 * 2 * 3 * 2 * 2 * 2 * 2 * 2 * 2


def test_backward_launch_with_the_option_on_differs_only_where_the_rule_says(monkeypatch):
    seen = set()
    for T, binary, masks, F, dropout, need_adj, offset, two_pass, dtype, precision in _grid():
        monkeypatch.setenv("GGCN_BACKWARD_TWO_PASS", "1" if two_pass else "0")
        layer, g = _layer(True, precision), _plan_graph(T, binary, masks)
        args = (True, need_adj, dropout, _operands(offset))
        plan = dispatch.backward_plan(layer, g, dtype, H, F, *args)
        got = dispatch.backward_launch(layer, g, dtype, 4, H, F, *args)
        rule = (binary and masks and 32 < T <= 128 and F % 4 == 0 and not offset and not two_pass and not need_adj and dropout is None)
        what = (T, binary, masks, F, dropout, need_adj, offset, two_pass, dtype, precision)
        assert got[1:] == plan[1:], what
        if rule:
            assert plan[0] == "two_pass" and got[0] == "wide", what
        else:
            assert got[0] == plan[0] and got[0] in dispatch.BACKWARD_PASSES, what
        seen.add(got[0])
    assert seen == set(dispatch.BACKWARD_PASSES) | {"wide"}


def test_the_pinned_plan_cases(monkeypatch):
    """The cases of tests/test_launch_names_cpu.py (those of ``test_backward_plan_names_every_form``): with the option off the
    launch is the plan on stand-ins that have no ``rowmask_t_wide`` at all; with it on, the one case of 33 nodes becomes "wide"."""
    from test_launch_names_cpu import _plan_cases
    changed = []
    for env, a in _plan_cases():
        for k in ("GGCN_BACKWARD_SCALAR", "GGCN_DX_PRECISION", "GGCN_BACKWARD_TWO_PASS"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        rest = (a["need_x"], a["need_adj"], a["dropout"], a["operands"])
        off = types.SimpleNamespace(precision=a["precision"])
        plan = dispatch.backward_plan(off, a["csr"], a["dtype"], a["K"], a["F"], *rest)
        assert not hasattr(a["csr"], "rowmask_t_wide")
        assert dispatch.backward_launch(off, a["csr"], a["dtype"], 4, a["K"], a["F"], *rest) == plan, (env, a)
        on = types.SimpleNamespace(precision=a["precision"], wide_backward=True)
        g = types.SimpleNamespace(**vars(a["csr"]), graph_ops_weighted_t=lambda: None, rowmask_t_wide=a["csr"].rowmask)
        got = dispatch.backward_launch(on, g, a["dtype"], 4, a["K"], a["F"], *rest)
        assert got[1:] == plan[1:]
        if got != plan:
            changed.append((g.T, plan[0], got[0]))
    assert changed == [(33, "two_pass", "wide")]


# ---------------------------------------------------------------- the numpy statements
@pytest.mark.parametrize("T", [33, 64, 65, 96, 97, 128])
def test_transposed_masks_statement(T):
    adj, _ = wb.ws.structure_batch(T, 300 + T)
    m = wb.rowmask_np(adj)
    W = (T + 31) // 32
    assert m.shape == (len(adj), T, W) and m.dtype == np.uint32
    mt = wb.transposed_masks_np(m, T)
    for b, s, t in itertools.product(range(len(adj)), (0, 1, 31, 32, T - 2, T - 1), range(T)):
        assert (int(mt[b, s, t // 32]) >> (t % 32)) & 1 == (int(m[b, t, s // 32]) >> (s % 32)) & 1 == int(adj[b, t, s] != 0)
    if T % 32:
        assert not (mt[:, :, W - 1] >> np.uint32(T % 32)).any()              # bits at or beyond T: exactly 0
    assert np.array_equal(wb.transposed_masks_np(mt, T), m)
    sym = [i for i, n in enumerate(wb.ws.NAMES) if n in wb.ws.SYMMETRIC]
    assert np.array_equal(mt[sym], m[sym]) and not np.array_equal(mt, m)


def _ratios(c):
    ref = gates.gate_pool_backward_statement64(c["out"], c["sg"], c["ga"], c["gb"], c["d_out"], c["d_pa"], c["d_pb"], c["adj"], c["inv"])
    em, bd = wb.emulate(c), wb.bounds(c, ref)
    out = {}
    for k, bound in bd.items():
        if bound is None or (k == "d_sg" and c["sg"] is None):
            continue
        err = (torch.from_numpy(em[k]).double() - ref[k]).abs()
        assert bool((err <= bound).all()), k
        out[k] = float((err / (bound + 1e-300)).max())
    return out


SPARE = {"dH": 0.25, "d_sg": 0.25, "d_bsum": 0.25, "d_ga": 1.0, "d_gb": 1.0}      # (the module docstring on d_ga / d_gb)


@pytest.mark.parametrize("T", wb.KERNEL_T)
def test_emulation_inside_the_bounds_with_a_factor_to_spare(T):
    for case in [k for k in wb.KERNEL_CASES if k[0] == T]:
        r = _ratios(wb.kernel_inputs(*case))
        print(case, {k: "%.3f" % v for k, v in r.items()})
        assert "dH" in r and "d_bsum" in r
        for k, v in r.items():
            assert v <= SPARE[k], (case, k, v)


def test_the_bound_notices_a_lost_plane():
    """Two bf16 planes instead of three (2^-17 of a term) is outside the dH bound: the bound is no blanket."""
    c = wb.kernel_inputs(100, 36)
    ref = gates.gate_pool_backward_statement64(c["out"], c["sg"], c["ga"], c["gb"], c["d_out"], c["d_pa"], c["d_pb"], c["adj"], c["inv"])
    bound = wb.bounds(c, ref)["dH"]
    gw = (c["inv"].double()[:, :, None] * ref["dY"]).float()
    hi = gw.to(torch.bfloat16).float()
    two = (hi + (gw - hi).to(torch.bfloat16).float()).double()
    dh2 = torch.einsum("bts,btf->bsf", c["adj"].double(), two)
    assert bool(((dh2 - ref["dH"]).abs() > bound).any())


# ---------------------------------------------------------------- the tie condition of the autograd inputs the GPU file adds
@pytest.mark.parametrize("name", sorted(wb.EXTRA))
def test_tie_condition_of_the_added_cases(name):
    Bn, T, K, F, seed = wb.EXTRA[name]
    for bf16 in (False, True):
        c = br.case_inputs(Bn, T, K, F, seed, bf16=bf16)
        ma, mb = br.layer_tie_masks(c["x"], c["adj"], c["w"], c["b"], c["ga"], c["gb"], br.tie_delta("f16mx8"))
        share = br.masked_share(ma, mb)
        print("%s%s: %.2f %% of the pools masked" % (name, " bf16" if bf16 else "", 100 * share))
        assert share <= br.MAX_MASKED
