"""The launch-path rules, pinned on a machine without a GPU.

``tests/golden/dispatch_table.json`` holds what every public ``takes_*`` predicate answered, over the grid of
``tools/dispatch_table.py``, at the commit before the rules moved into ``dispatch.py`` (the tool's docstring names it).  The
first test regenerates the table from the checked-out code and compares entry by entry; the others assert that
``dispatch.layer_path`` / ``dispatch.block_path`` return, for every case of the grid, the name that the precedence of the
old ``if`` chains implies from those recorded answers -- the chains are written out below, independently of ``dispatch.py``."""
import importlib.util
import itertools
import json
import os
import types

import pytest
import torch

from ed_gated_gcn_amd import dispatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("dispatch_table_tool", os.path.join(ROOT, "tools", "dispatch_table.py"))
tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tool)

LAYER_CASES = (len(tool.TS) * len(tool.BS) + len(tool.EXTRA_SHAPES)) * len(tool.DTYPES) * 8 * len(tool.PRECISIONS) * len(tool.FUSED_MAX_TS) * 2
BLOCK_CASES = (len(tool.BLOCK_TS) * len(tool.BLOCK_BS) * len(tool.DTYPES) * len(tool.BLOCK_GRAPHS)
               * len(tool.PRECISIONS) * 2 * len(tool.BLOCK_OPTIONS) * 2 * 2)


@pytest.fixture(scope="module")
def golden():
    with open(tool.GOLDEN) as f:
        table = json.load(f)
    return {"layer": tool.decode(table["layer"], table["layer_digits"]), "block": tool.decode(table["block"], table["block_digits"]),
            "table": table}


def test_table_matches_the_recorded_answers(golden):
    new = tool.build_table()
    assert LAYER_CASES == 75600 and BLOCK_CASES == 25920     # the grid itself is part of the record
    compared = 0
    for key, cases, columns, n in (("layer", tool.layer_cases, tool.LAYER_COLUMNS, LAYER_CASES),
                                   ("block", tool.block_cases, tool.BLOCK_COLUMNS, BLOCK_CASES)):
        assert new[key + "_columns"] == golden["table"][key + "_columns"] == list(columns)
        got, want = tool.decode(new[key], new[key + "_digits"]), golden[key]
        assert len(got) == len(want) == new[key + "_cases"] == golden["table"][key + "_cases"] == n
        for i, column in enumerate(columns):   # no column is trivial: both answers occur
            answers = {v >> i & 1 for v in want}
            assert answers == {0, 1}, "%s never answers %s" % (column, "True" if 0 in answers else "False")
        for i, (g, w) in enumerate(zip(got, want)):
            if g != w:
                label = next(itertools.islice(cases(), i, None))[0]
                names = [c for j, c in enumerate(columns) if (g ^ w) >> j & 1] or ["kernel_precision"]
                pytest.fail("%s case %d [%s]: %s differ(s) from the recorded answer (bits now %#x, recorded %#x)"
                            % (key, i, label, ", ".join(names), g, w))
            compared += 1
    assert compared == LAYER_CASES + BLOCK_CASES   # nothing skipped
    assert tool.dumps(new) == open(tool.GOLDEN).read()   # and the file the tool would write is the committed one, byte for byte


def _expected_layer_path(answer, dropout, aligned):
    """The old ``_forward_gated``: fused before bf16 before weighted before long before two launches; the ``_drop`` names exactly
    when the matching dropout predicate holds (any other name under ``dropout`` is a refusal)."""
    if answer["takes_fused_path"]:
        return "fused_drop" if dropout and answer["takes_dropout_path"] else "fused"
    if answer["takes_bf16_fused_path"] or answer["takes_bf16_wide_path"]:
        name = "bf16_wide" if answer["takes_bf16_wide_path"] else "bf16"
        return name + "_drop" if dropout and answer["takes_bf16_dropout_path"] else name
    if not dropout and answer["takes_weighted_path"]:
        return "weighted"
    if answer["takes_long_path"] and aligned:
        return "long"
    return "two_launch"


def test_layer_path_follows_the_precedence_of_the_predicates(golden):
    aligned = types.SimpleNamespace(data_ptr=lambda: 4096, stride=lambda d: 768)
    odd_address = types.SimpleNamespace(data_ptr=lambda: 4098, stride=lambda d: 768)
    odd_stride = types.SimpleNamespace(data_ptr=lambda: 4096, stride=lambda d: 772)
    seen, n = set(), 0
    with tool.pretend_device():
        for (label, layer, text, csr), bits in zip(tool.layer_cases(), golden["layer"]):
            answer = {c: bool(bits >> i & 1) for i, c in enumerate(tool.LAYER_COLUMNS)}
            for dropout, (rows, ok) in itertools.product((False, True), ((None, True), (aligned, True), (odd_address, False), (odd_stride, False))):
                if rows is not None and not answer["takes_long_path"]:
                    continue   # the rows are looked at on the long path alone: one call without them covers the case
                got = dispatch.layer_path(layer, text, csr, dropout, rows)
                assert got == _expected_layer_path(answer, dropout, ok), (label, dropout, ok)
                seen.add(got)
            n += 1
    assert n == LAYER_CASES
    assert seen == set(dispatch.LAYER_PATHS)   # every name is reached


def _expected_block_path(answer, layer1_one_launch, layer2_one_launch, equal_widths, want, want_gcn1, one_launch, training):
    """The old ``_gated_gcn_block``, statement by statement."""
    w_l1 = any(k in want for k in ("x1", "y1", "xy"))
    if not training and one_launch and answer["takes_block_path"]:
        return "block"
    if not training and one_launch and answer["takes_bf16_block_path"]:
        return "bf16_block"
    if not training and one_launch and not w_l1 and not want_gcn1 and answer["takes_bf16_folded_eval_path"]:
        return "bf16_folded_eval"
    if not training and layer1_one_launch and layer2_one_launch and equal_widths:
        if not w_l1 and not want_gcn1 and one_launch and answer["takes_folded_eval_path"]:
            return "folded_eval"
        if not w_l1:
            return "layers_eval"
        return "two_fused"
    if not training and not w_l1:
        return "layers_eval"
    return "layers"


def test_block_path_follows_the_precedence_of_the_predicates(golden):
    everything = ("x1", "y1", "xy", "x", "out")
    # (want, want_gcn1, one_launch, training): every combination in inference; under autograd want= is everything
    flags = [f + (False,) for f in itertools.product((everything, ("out",), ("xy", "out")), (False, True), (False, True))]
    flags += [(everything, g, o, True) for g, o in itertools.product((False, True), (False, True))]
    seen, n = set(), 0
    with tool.pretend_device():
        for (label, x, csr, gc1, gc2), bits in zip(tool.block_cases(), golden["block"]):
            answer = {c: bool(bits >> i & 1) for i, c in enumerate(tool.BLOCK_COLUMNS)}
            gcn1 = tool.features(x.shape[0], x.shape[1], gc1.out_features, torch.float32)   # what gc2 reads, whatever x is
            one1 = gc1.takes_fused_path(x, csr) or gc1.takes_bf16_fused_path(x, csr) or gc1.takes_bf16_wide_path(x, csr)
            one2 = gc2.takes_fused_path(gcn1, csr)
            for want, want_gcn1, one_launch, training in flags:
                got = dispatch.block_path(x, csr, gc1, gc2, want, want_gcn1, one_launch, training)
                assert got == _expected_block_path(answer, one1, one2, gc1.out_features == gc2.out_features, want, want_gcn1,
                                                   one_launch, training), (label, want, want_gcn1, one_launch, training)
                seen.add(got)
            n += 1
    assert n == BLOCK_CASES
    assert seen == set(dispatch.BLOCK_PATHS)


def test_backward_plan_names_every_form(monkeypatch):
    for name in ("GGCN_BACKWARD_TWO_PASS", "GGCN_BACKWARD_SCALAR", "GGCN_DX_PRECISION"):
        monkeypatch.delenv(name, raising=False)
    on_gpu = types.SimpleNamespace(is_cuda=True)
    at = lambda address: types.SimpleNamespace(data_ptr=lambda: address)   # noqa: E731
    csr = types.SimpleNamespace(T=24, is_binary=True, rowmask=on_gpu, graph_ops=on_gpu, graph_ops_t=on_gpu)
    layer = lambda precision: types.SimpleNamespace(precision=precision)   # noqa: E731
    f32, bf16 = torch.float32, torch.bfloat16

    def plan(precision="f16mx8", csr=csr, dtype=f32, K=64, F=64, need_x=True, need_adj=False, dropout=None, operands=(at(4096), None)):
        return dispatch.backward_plan(layer(precision), csr, dtype, K, F, need_x, need_adj, dropout, operands)

    assert plan() == ("mma", "scaled", "bf16x3")
    assert plan(need_x=False) == ("mma", None, "bf16x3")
    assert plan("bf16x3") == ("mma", "bf16x3", "bf16x3")
    assert plan("fp32") == ("mma", "fp32", "fp32")
    assert plan(dtype=bf16) == ("mma", "bf16", "bf16")
    assert plan(F=48) == ("mma", "bf16x3", "bf16x3")                                   # the scaled linear wants F % 32 == 0
    assert plan(dropout=(0.5, 1, (0, 1, 2))) == ("one_pass", "bf16x3", "bf16x3")      # the scalar launch: F % 256 == 0 for max |dH|
    assert plan(F=256, dropout=(0.5, 1, (0, 1, 2))) == ("one_pass", "scaled", "bf16x3")
    assert plan(F=30) == ("two_pass", "bf16x3", "bf16x3")
    assert plan(need_adj=True) == ("two_pass", "bf16x3", "bf16x3")
    assert plan(operands=(at(4096), at(4100))) == ("two_pass", "bf16x3", "bf16x3")
    assert plan(dropout=(0.5, 1, (0, 1, 2)), operands=(at(4100),)) == ("two_pass_drop", "bf16x3", "bf16x3")
    for graph in (dict(T=33), dict(is_binary=False), dict(rowmask=None)):
        assert plan(csr=types.SimpleNamespace(**{**vars(csr), **graph}))[0] == "two_pass", graph
    assert plan(csr=types.SimpleNamespace(**{**vars(csr), "graph_ops_t": None})) == ("one_pass", "bf16x3", "bf16x3")
    monkeypatch.setenv("GGCN_BACKWARD_SCALAR", "1")
    assert plan(F=256) == ("one_pass", "scaled", "bf16x3")
    monkeypatch.setenv("GGCN_DX_PRECISION", "bf16x3")
    assert plan(F=256) == ("one_pass", "bf16x3", "bf16x3")
    monkeypatch.setenv("GGCN_BACKWARD_TWO_PASS", "1")
    assert plan() == ("two_pass", "bf16x3", "bf16x3")
    assert set(dispatch.BACKWARD_PASSES) == {"mma", "one_pass", "two_pass", "two_pass_drop"}
    assert set(dispatch.DX_FORMS) == {"bf16", "scaled", "bf16x3", "fp32"}
