"""The one name per launch (``dispatch.layer_launch`` / ``dispatch.backward_launch``) against the composition of calls it replaced,
and the entry checks of ``capi.hip`` that moved into shared helpers -- on a machine without a GPU.

The old compositions (``layer_path``, then ``takes_weighted_dropout``, then the ``T > 32`` split inside the branch chain of
``_forward_gated``; ``backward_plan``, then one of the two weighted-backward predicates) are written out here, independently of
``dispatch.py``, and so are the bodies the two weighted-backward predicates had before they became statements over one private
predicate.  Graphs are stand-ins that log which operand block they were asked for: the new functions must ask for the same blocks,
in the same order, as the old sequence of calls.  Section 4 does the same for ``backward_launch`` as a loop over one table of the
four opt-in one-launch backwards: against the four-armed chain over the four predicates' bodies that it replaced, on a joint grid
of the three options.  The refusals are asked of the loaded library with NULL pointers: every check
tested here comes before anything is dereferenced or launched."""
import ctypes
import importlib.util
import itertools
import os
import types

import pytest
import torch

import ed_gated_gcn_amd as pkg
from ed_gated_gcn_amd import _capi, dispatch
from ed_gated_gcn_amd.gcn import GraphConvolution

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("dispatch_table_tool", os.path.join(ROOT, "tools", "dispatch_table.py"))
tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tool)

H = 64
ENV = ("GGCN_WEIGHTED_DROPOUT", "GGCN_WEIGHTED_BACKWARD", "GGCN_WEIGHTED_MAX_T", "GGCN_BACKWARD_TWO_PASS", "GGCN_BACKWARD_SCALAR",
       "GGCN_DX_PRECISION", "GGCN_FUSED", "GGCN_FUSED_MAX_T", "GGCN_PRECISION", "GGCN_EDGE_LISTS")
NEW_LAYER_NAMES = ("weighted_wide", "weighted_drop", "weighted_wide_drop")


@pytest.fixture(autouse=True)
def _no_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def test_the_tuples():
    assert dispatch.LAYER_LAUNCHES == dispatch.LAYER_PATHS + NEW_LAYER_NAMES
    assert dispatch.DROPOUT_LAUNCHES == dispatch.DROPOUT_PATHS + ("weighted_drop", "weighted_wide_drop")
    assert dispatch.OVERLAP_LAUNCHES == dispatch.OVERLAP_PATHS
    assert dispatch.BACKWARD_LAUNCHES == ("mma", "one_pass", "two_pass", "two_pass_drop", "weighted", "weighted_drop", "wide", "weighted_wide")
    assert dispatch.BACKWARD_LAUNCHES[:4] == dispatch.BACKWARD_PASSES


# ---------------------------------------------------------------- 1. layer_launch
def _old_layer_launch(layer, text, csr, dropout, rows=None):
    """What ``_forward_gated`` decided before ``layer_launch``: ``layer_path``, then -- dropout handed in and no ``DROPOUT_PATHS`` name --
    ``takes_weighted_dropout``; the branch chain took the weighted dropout launches first and split both weighted forms at T > 32."""
    path = dispatch.layer_path(layer, text, csr, dropout, rows)
    weighted_drop = dropout and path not in dispatch.DROPOUT_PATHS and dispatch.takes_weighted_dropout(layer, csr, dispatch.Input.of(text))
    if weighted_drop:
        return "weighted_wide_drop" if csr.T > 32 else "weighted_drop"
    if path == "weighted" and csr.T > 32:
        return "weighted_wide"
    return path


def test_layer_launch_is_layer_path_on_the_pinned_grid():
    seen, n = set(), 0
    with tool.pretend_device():
        for label, layer, text, csr in tool.layer_cases():
            for dropout in (False, True):
                path = dispatch.layer_path(layer, text, csr, dropout)
                want = "weighted_wide" if path == "weighted" and csr.T > 32 else path   # every opt-in is off on this grid
                assert dispatch.layer_launch(layer, text, csr, dropout) == want, (label, dropout)
                seen.add(want)
            n += 1
    assert n == 75600
    assert seen == set(dispatch.LAYER_PATHS)       # weighted_max_t is 32 here: no graph of > 32 nodes is "weighted"


def _graph(T, B=4, binary=False, ops=True, log=None):
    """A ``BatchedCSR`` stand-in that logs the operand blocks it is asked for."""
    asked = [] if log is None else log
    blk = types.SimpleNamespace(is_cuda=True)
    g = types.SimpleNamespace(T=T, B=B, is_binary=binary, asked=asked, rowmask=blk if binary else None,
                              graph_ops=blk if binary else None, graph_ops_t=blk if binary else None)
    g.graph_ops_weighted = lambda plane: (asked.append("w%d" % plane), blk if ops else None)[1]
    g.graph_ops_weighted_wide = lambda: (asked.append("ww"), blk if ops else None)[1]
    g.graph_ops_weighted_t = lambda: (asked.append("wt"), blk if ops else None)[1]
    return g


def _layer(precision="f16mx8", dropout=False, backward=False, max_t=32, fused=True):
    return GraphConvolution(H, H, opt=types.SimpleNamespace(ggcn_precision=precision, ggcn_weighted_dropout=dropout, ggcn_fused=fused,
                                                            ggcn_weighted_backward=backward, ggcn_weighted_max_t=max_t))


def _from_the_rules(option, max_t, T, precision, ops, fits, fused, dtype, dropout):
    """``(name, asked)`` on a real-valued adjacency from the rules as the documents state them, without ``dispatch.py``: one launch for
    ``fused``, float32 features, a split precision and graphs of <= 32 nodes or 33..min(weighted_max_t, 128); under dropout only
    with the option and an element index below 2^32; the graph is asked for its block only once all of that holds."""
    eligible = fused and dtype == torch.float32 and precision in ("bf16x3", "f16mx8") and (T <= 32 or T <= min(max_t, 128))
    if dropout:
        eligible = eligible and option and fits
    if not eligible:
        return "two_launch", []
    block = "ww" if T > 32 else "w0" if precision == "bf16x3" else "w1"
    name = "weighted" + ("_wide" if T > 32 else "") + ("_drop" if dropout else "")
    return (name if ops else "two_launch"), [block]


def test_layer_launch_with_the_options_on():
    seen, n = set(), 0
    layers = {k: _layer(k[0], k[1], max_t=k[2], fused=k[3])
              for k in itertools.product(("bf16x3", "f16mx8", "fp32"), (False, True), (32, 128), (True, False))}
    for T, ops, fits, dtype, dropout in itertools.product((1, 32, 33, 128, 129), (True, False), (True, False),
                                                          (torch.float32, torch.bfloat16), (False, True)):
        B = -(-2 ** 32 // (T * H)) - (1 if fits else 0)      # B*T*F on both sides of 2^32 (F = H)
        assert (B * T * H < 2 ** 32) == fits and (B + 1) * T * H >= 2 ** 32
        text = types.SimpleNamespace(dtype=dtype, shape=(B, T, H), is_cuda=True, device="cuda:0")
        for (precision, option, max_t, fused), layer in layers.items():
            if dtype == torch.bfloat16 and precision == "fp32":
                continue                                      # _check refuses it before any launch is chosen
            old_g, new_g = _graph(T, B, ops=ops), _graph(T, B, ops=ops)
            want = _old_layer_launch(layer, text, old_g, dropout)
            got = dispatch.layer_launch(layer, text, new_g, dropout)
            what = (T, ops, fits, dtype, dropout, precision, option, max_t, fused)
            assert got == want and got in dispatch.LAYER_LAUNCHES, what
            assert new_g.asked == old_g.asked, what
            assert (got, new_g.asked) == _from_the_rules(option, max_t, T, precision, ops, fits, fused, dtype, dropout), what
            seen.add(got)
            n += 1
    assert n == 5 * 2 * 2 * 2 * 2 * 24 - 5 * 2 * 2 * 2 * 8
    assert seen == {"weighted", "two_launch"} | set(NEW_LAYER_NAMES)   # with the pinned grid above: every name of LAYER_LAUNCHES


# ---------------------------------------------------------------- 2. / 3. backward_launch and the two predicates
def _old_takes_weighted_backward(layer, csr, F, dropout, operands):
    """The body at the parent commit."""
    return bool(getattr(layer, "weighted_backward", False) and not csr.is_binary and csr.T <= 32 and F % 4 == 0 and dropout is None
                and all(t is None or t.data_ptr() % 16 == 0 for t in operands)
                and os.environ.get("GGCN_BACKWARD_TWO_PASS", "0") != "1" and csr.graph_ops_weighted_t() is not None)


def _old_takes_weighted_backward_drop(layer, csr, B, F, dropout, operands):
    """The body at the parent commit."""
    return bool(getattr(layer, "weighted_backward", False) and dropout is not None and B * csr.T * F < 2 ** 32
                and not csr.is_binary and csr.T <= 32 and F % 4 == 0
                and all(t is None or t.data_ptr() % 16 == 0 for t in operands)
                and os.environ.get("GGCN_BACKWARD_TWO_PASS", "0") != "1" and csr.graph_ops_weighted_t() is not None)


def _old_backward_launch(layer, csr, dtype, B, K, F, need_x, need_adj, dropout, operands):
    """``_GatedLayerFunction.backward`` before ``backward_launch``: the plan, then one predicate where the plan says two passes."""
    passes, dx, dw = dispatch.backward_plan(layer, csr, dtype, K, F, need_x, need_adj, dropout, operands)
    weighted = ((passes == "two_pass" and _old_takes_weighted_backward(layer, csr, F, dropout, operands))
                or (passes == "two_pass_drop" and _old_takes_weighted_backward_drop(layer, csr, B, F, dropout, operands)))
    return ("weighted" + ("_drop" if dropout is not None else "") if weighted else passes), dx, dw


def _at(address, log=None):
    return types.SimpleNamespace(data_ptr=lambda: (log.append("ptr") if log is not None else None, address)[1])


def _plan_cases():
    """The cases of ``test_backward_plan_names_every_form`` as ``(environment, arguments)``."""
    on_gpu = types.SimpleNamespace(is_cuda=True)
    csr = types.SimpleNamespace(T=24, is_binary=True, rowmask=on_gpu, graph_ops=on_gpu, graph_ops_t=on_gpu)
    drop = (0.5, 1, (0, 1, 2))
    base = dict(precision="f16mx8", csr=csr, dtype=torch.float32, K=64, F=64, need_x=True, need_adj=False, dropout=None,
                operands=(_at(4096), None))
    edits = [{}, dict(need_x=False), dict(precision="bf16x3"), dict(precision="fp32"), dict(dtype=torch.bfloat16), dict(F=48),
             dict(dropout=drop), dict(F=256, dropout=drop), dict(F=30), dict(need_adj=True), dict(operands=(_at(4096), _at(4100))),
             dict(dropout=drop, operands=(_at(4100),))]
    edits += [dict(csr=types.SimpleNamespace(**{**vars(csr), **g})) for g in (dict(T=33), dict(is_binary=False), dict(rowmask=None),
                                                                              dict(graph_ops_t=None))]
    cases = [({}, {**base, **e}) for e in edits]
    cases.append((dict(GGCN_BACKWARD_SCALAR="1"), {**base, "F": 256}))
    cases.append((dict(GGCN_BACKWARD_SCALAR="1", GGCN_DX_PRECISION="bf16x3"), {**base, "F": 256}))
    cases.append((dict(GGCN_BACKWARD_SCALAR="1", GGCN_DX_PRECISION="bf16x3", GGCN_BACKWARD_TWO_PASS="1"), dict(base)))
    return cases


def test_backward_launch_is_backward_plan_where_no_weighted_launch_applies(monkeypatch):
    seen = set()
    for env, a in _plan_cases():
        for k in ("GGCN_BACKWARD_SCALAR", "GGCN_DX_PRECISION", "GGCN_BACKWARD_TWO_PASS"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        layer = types.SimpleNamespace(precision=a["precision"])
        rest = (a["need_x"], a["need_adj"], a["dropout"], a["operands"])
        plan = dispatch.backward_plan(layer, a["csr"], a["dtype"], a["K"], a["F"], *rest)
        assert dispatch.backward_launch(layer, a["csr"], a["dtype"], 4, a["K"], a["F"], *rest) == plan, (env, a)
        assert _old_backward_launch(layer, a["csr"], a["dtype"], 4, a["K"], a["F"], *rest) == plan
        seen.add(plan[0])
    assert seen == set(dispatch.BACKWARD_PASSES)


def _weighted_backward_cases():
    """``(what, environment, make)``; ``make()`` gives fresh ``(log, layer, csr, B, F, dropout, operands)``: the graph and the operands log
    into ``log`` what they are asked, in order."""
    for option, binary, T, F, drop, offset, two_pass, ops, big in itertools.product(
            (True, False), (False, True), (32, 33), (4, 30), (None, (0.25, 7, (0, 1, 2))), (0, 4), (False, True), (True, False), (False, True)):
        B = -(-2 ** 32 // (T * F)) if big else 4              # B*T*F >= 2^32 (== 2^32 for T = 32, F = 4): matters under dropout only

        def make(option=option, binary=binary, T=T, B=B, F=F, drop=drop, offset=offset, ops=ops):
            log = []
            operands = (_at(1 << 20, log), None, _at((1 << 20) + offset, log), None)
            return log, _layer(backward=option), _graph(T, B, binary=binary, ops=ops, log=log), B, F, drop, operands
        yield (option, binary, T, F, drop, offset, two_pass, ops, big), ({"GGCN_BACKWARD_TWO_PASS": "1"} if two_pass else {}), make


def test_backward_launch_matches_the_old_composition(monkeypatch):
    seen, n = set(), 0
    for what, env, make in _weighted_backward_cases():
        monkeypatch.delenv("GGCN_BACKWARD_TWO_PASS", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for need_adj in (False, True):
            old_log, layer, csr, B, F, drop, operands = make()
            want = _old_backward_launch(layer, csr, torch.float32, B, H, F, True, need_adj, drop, operands)
            new_log, layer, csr, B, F, drop, operands = make()
            got = dispatch.backward_launch(layer, csr, torch.float32, B, H, F, True, need_adj, drop, operands)
            assert got == want and got[0] in dispatch.BACKWARD_LAUNCHES, (what, need_adj)
            assert new_log == old_log, (what, need_adj)
            assert new_log.count("wt") <= 1 and "wt" not in new_log[:-1], (what, need_adj)      # asked last, or not at all
            assert got[1:] == dispatch.backward_plan(layer, csr, torch.float32, H, F, True, need_adj, drop, operands)[1:]
            if got[0] in ("weighted", "weighted_drop"):
                option, binary, T, F_, drop_, offset, two_pass, ops, big = what
                assert option and not binary and T == 32 and F_ == 4 and not offset and not two_pass and ops and not (big and drop_), what
                assert (got[0] == "weighted_drop") == (drop_ is not None)
            seen.add(got[0])
            n += 1
    assert n == 2 ** 10
    assert seen == set(dispatch.BACKWARD_PASSES) | {"weighted", "weighted_drop"}


def test_the_weighted_backward_predicates_answer_as_their_parent_commit_bodies(monkeypatch):
    answers = set()
    for what, env, make in _weighted_backward_cases():
        monkeypatch.delenv("GGCN_BACKWARD_TWO_PASS", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for old, new, with_b in ((_old_takes_weighted_backward, dispatch.takes_weighted_backward, False),
                                 (_old_takes_weighted_backward_drop, dispatch.takes_weighted_backward_drop, True)):
            old_log, layer, csr, B, F, drop, operands = make()
            want = old(layer, csr, *((B,) if with_b else ()), F, drop, operands)
            new_log, layer, csr, B, F, drop, operands = make()
            got = new(layer, csr, *((B,) if with_b else ()), F, drop, operands)
            assert got is want, (what, new.__name__)
            assert [a for a in new_log if a != "ptr"] == [a for a in old_log if a != "ptr"], (what, new.__name__)
            assert "wt" not in new_log[:-1], (what, new.__name__)
            answers.add((new.__name__, got))
    assert len(answers) == 4                                   # both predicates answer True and False


# ---------------------------------------------------------------- 4. backward_launch with all three options: the parent's elif chain
def _old_takes_wide_backward(layer, csr, B, F, dropout, operands):
    """The body at the parent commit."""
    if not getattr(layer, "wide_backward", False):
        return False
    if not (dropout is None and csr.is_binary and 32 < csr.T <= 128 and F % 4 == 0
            and all(t is None or t.data_ptr() % 16 == 0 for t in operands) and os.environ.get("GGCN_BACKWARD_TWO_PASS", "0") != "1"):
        return False
    return csr.rowmask_t_wide is not None


def _old_takes_weighted_wide_backward(layer, csr, F, dropout, operands):
    """The body at the parent commit."""
    if not getattr(layer, "weighted_wide_backward", False):
        return False
    if not (dropout is None and not csr.is_binary and 32 < csr.T <= 128 and F % 4 == 0
            and all(t is None or t.data_ptr() % 16 == 0 for t in operands) and os.environ.get("GGCN_BACKWARD_TWO_PASS", "0") != "1"):
        return False
    return csr.graph_ops_weighted_wide_t() is not None


def _parent_backward_launch(layer, csr, dtype, B, K, F, need_x, need_adj, dropout, operands):
    """``dispatch.backward_launch`` at the parent commit: the plan, then a four-armed chain over the four predicates."""
    passes, dx, dw = dispatch.backward_plan(layer, csr, dtype, K, F, need_x, need_adj, dropout, operands)
    if passes == "two_pass" and _old_takes_weighted_backward(layer, csr, F, dropout, operands):
        passes = "weighted"
    elif passes == "two_pass_drop" and _old_takes_weighted_backward_drop(layer, csr, B, F, dropout, operands):
        passes = "weighted_drop"
    elif passes == "two_pass" and not need_adj and _old_takes_wide_backward(layer, csr, B, F, dropout, operands):
        passes = "wide"
    elif passes == "two_pass" and _old_takes_weighted_wide_backward(layer, csr, F, dropout, operands):
        passes = "weighted_wide"
    return passes, dx, dw


OPERAND_BLOCKS = ("wt", "mtw", "wwt")


def _joint_graph(T, B, binary, masks, ops, log):
    """A ``BatchedCSR`` stand-in for all three options: the three transposed operands log into ``log`` that they were asked for
    (``rowmask_t_wide`` is a property, like the real one, and exists only with row masks)."""
    blk = types.SimpleNamespace(is_cuda=True)

    class Graph:
        rowmask_t_wide = property(lambda self: (log.append("mtw"), blk if ops and masks else None)[1])
    g = Graph()
    g.T, g.B, g.is_binary = T, B, binary
    g.rowmask = g.graph_ops = g.graph_ops_t = blk if masks else None
    g.graph_ops_weighted_t = lambda: (log.append("wt"), blk if ops else None)[1]
    g.graph_ops_weighted_wide_t = lambda: (log.append("wwt"), blk if ops else None)[1]
    return g


def test_backward_launch_with_all_three_options_matches_the_parent_chain(monkeypatch):
    options = list(itertools.product((False, True), repeat=3))
    layers = {o: GraphConvolution(H, H, opt=types.SimpleNamespace(ggcn_weighted_backward=o[0], ggcn_wide_backward=o[1],
                                                                  ggcn_weighted_wide_backward=o[2])) for o in options}
    for o, layer in layers.items():
        assert (layer.weighted_backward, layer.wide_backward, layer.weighted_wide_backward) == o
    seen, n = set(), 0
    for two_pass in (False, True):
        monkeypatch.setenv("GGCN_BACKWARD_TWO_PASS", "1" if two_pass else "0")
        for T, binary, masks, ops, F, drop, offset, need_adj, fits in itertools.product(
                (1, 32, 33, 128, 129), (False, True), (True, False), (True, False), (4, 30), (None, (0.25, 7, (0, 1, 2))), (0, 4),
                (False, True), (True, False)):
            B = -(-2 ** 32 // (T * F)) - (1 if fits else 0)      # B*T*F on both sides of 2^32
            assert (B * T * F < 2 ** 32) == fits and (B + 1) * T * F >= 2 ** 32
            for o, layer in layers.items():
                logs, answers = [], []
                for launch in (_parent_backward_launch, dispatch.backward_launch):
                    log = []
                    operands = (_at(1 << 20, log), None, _at((1 << 20) + offset, log), None)
                    csr = _joint_graph(T, B, binary, masks, ops, log)
                    answers.append(launch(layer, csr, torch.float32, B, H, F, True, need_adj, drop, operands))
                    logs.append(log)
                what = (o, T, binary, masks, ops, F, drop, offset, two_pass, need_adj, fits)
                assert answers[1] == answers[0] and answers[1][0] in dispatch.BACKWARD_LAUNCHES, what
                assert logs[1] == logs[0], what
                blocks = [a for a in logs[1] if a in OPERAND_BLOCKS]
                assert len(blocks) <= 1 and not any(a in OPERAND_BLOCKS for a in logs[1][:-1]), what      # asked last, or not at all
                seen.add(answers[1][0])
                n += 1
    assert n == 2 * 5 * 2 ** 8 * 8
    assert seen == set(dispatch.BACKWARD_LAUNCHES)


# ---------------------------------------------------------------- 5. the refusals that moved into helpers
EINVAL = 1
P = ctypes.c_void_p(1 << 20)   # non-null, 16-byte aligned, never dereferenced
DROP_ENTRIES = sorted(n for n, (_, args) in _capi.PROTOTYPES.items() if ctypes.c_float in args and n != "ggcn_dropout_mask")
BAD_DROPS = ((1.0, (0, 0, 0), "p=1 streams 0 0 0"), (0.25, (0, 1, 3), "p=0.25 streams 0 1 3"), (-0.5, (2, 1, 0), "p=-0.5 streams 2 1 0"),
             (float("nan"), (0, 0, 0), "p=nan streams 0 0 0"))


def test_there_are_eight_entries_with_dropout_arguments():
    assert DROP_ENTRIES == sorted(("ggcn_layer_fused_drop", "ggcn_layer_fused_bf16_drop", "ggcn_layer_fused_bf16_wide",
                                   "ggcn_layer_fused_weighted_drop", "ggcn_layer_fused_weighted_wide_drop", "ggcn_gate_pool_backward_drop",
                                   "ggcn_gate_pool_backward_agg", "ggcn_gate_pool_backward_weighted_drop"))


@pytest.mark.parametrize("entry", DROP_ENTRIES)
def test_dropout_arguments_are_refused_in_the_entrys_name(entry):
    lib = pkg.load_library()
    types_ = _capi.PROTOTYPES[entry][1]
    at = types_.index(ctypes.c_float)
    assert types_[at + 1] is ctypes.c_uint64 and types_[at + 2:at + 5] == [_capi.c_i32] * 3
    for p, sels, text in BAD_DROPS:
        args = [None if t is _capi.c_vp else 7 for t in types_]          # NULL pointers, any positive integers
        args[at:at + 5] = [p, 5, *sels]
        assert getattr(lib, entry)(*args) == EINVAL, (entry, p, sels)
        assert lib.ggcn_last_error().decode() == "%s: %s" % (entry, text)


LINEARS = {   # entry -> its arguments by name, in order (include/ggcn.h)
    "ggcn_linear": ("X", "ldx", "W", "ldw", "wpack", "Y", "ldy", "M", "K", "F", "precision", "stream"),
    "ggcn_linear_bf16": ("X", "ldx", "wpack", "Y", "ldy", "M", "K", "F", "stream"),
    "ggcn_linear_out_bf16": ("X", "ldx", "wpack", "Y", "ldy", "M", "K", "F", "stream"),
    "ggcn_linear_h": ("X", "ldx", "wpack", "Y", "ldy", "M", "K", "F", "precision", "stream"),
}


@pytest.mark.parametrize("entry", sorted(LINEARS))
@pytest.mark.parametrize("edit,text", [(dict(X=None), "null pointer"), (dict(Y=None), "null pointer"),
                                       (dict(M=0), "M=0 K=64 F=48 must be positive"), (dict(K=-1, ldx=64), "M=8 K=-1 F=48 must be positive"),
                                       (dict(ldx=63), "leading dimension too small"), (dict(ldy=47), "leading dimension too small")])
def test_linear_preamble_refusals(entry, edit, text):
    lib = pkg.load_library()
    a = dict(X=P, W=P, wpack=P, Y=P, ldx=64, ldw=48, ldy=48, M=8, K=64, F=48, precision=_capi.PREC["bf16x3"], stream=None)
    a.update(edit)
    assert len(LINEARS[entry]) == len(_capi.PROTOTYPES[entry][1])
    assert getattr(lib, entry)(*(a[k] for k in LINEARS[entry])) == EINVAL
    assert lib.ggcn_last_error().decode() == "%s: %s" % (entry, text)
