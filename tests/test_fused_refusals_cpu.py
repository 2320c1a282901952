"""The fifteen one-launch entries refuse what they refused, with the same code and the same message (no GPU).

``tests/golden/fused_refusals.json`` holds what ``ggcn_layer_fused*``, ``ggcn_block_fused*``, ``ggcn_lab_block_fused8`` and
``ggcn_debug_block_fused_stamped`` answered to every single-fault variant of ``tools/fused_refusals.py`` at the commit before their
host code was folded into one check list (the tool's docstring names it).  This test makes the same calls against the checked-out
library and compares code and message byte for byte: the entries share ``launch_fused``, ``fused_part_checks``, ``launch_block`` and
``block_fused8``, and a check moved, reworded or dropped in one of them shows up here as the entry and variant it changed.

The calls pass fake pointers, so the whole module is skipped where a GPU is visible: a regression that stopped refusing would
launch on them.  The host code is the same on both machines, so the check is complete without one."""
import importlib.util
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("fused_refusals_tool", os.path.join(ROOT, "tools", "fused_refusals.py"))
tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tool)

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: never where a launch could reach a card")

with open(tool.GOLDEN) as _f:
    GOLDEN = json.load(_f)


def test_the_table_covers_the_fifteen_entries():
    assert sorted(GOLDEN) == sorted(tool.ENTRIES) and len(GOLDEN) == 15
    assert all(GOLDEN[e] for e in GOLDEN), "an entry without a recorded refusal"
    assert all(rc in (tool.EINVAL, tool.EUNSUPPORTED) for per in GOLDEN.values() for rc, _ in per.values())


@pytest.mark.parametrize("entry", sorted(tool.ENTRIES))
def test_every_recorded_refusal_is_refused_alike(entry):
    lib, params = tool.load(), tool.prototypes()[entry]
    calls = dict(tool.cases(entry, params))
    recorded = GOLDEN[entry]
    assert set(recorded) <= set(calls), "recorded variants the tool no longer makes: %s" % sorted(set(recorded) - set(calls))
    wrong = []
    for label, (rc, msg) in recorded.items():
        got = tool.call(lib, entry, params, calls[label])
        if got != (rc, msg):
            wrong.append((label, (rc, msg), got))
    assert not wrong, "%d of %d refusals of %s changed; the first: %r" % (len(wrong), len(recorded), entry, wrong[:3])
