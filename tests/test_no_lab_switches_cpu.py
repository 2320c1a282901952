"""The kernels carry no compile-time lab switch, and the Makefile's header list names only files that exist (text only, no GPU).

``csrc/`` once held a family of ``GGCN_LAB_*`` macros that the product build never set: constants and discarded branches between the
real statements of the hot loops.  They are gone; a variant is now built from an older revision's sources (``tools/lab.py build
name@<rev>:-D...``).  What remains under that prefix are the four RUN-TIME switches of the experiment entry ``ggcn_lab_block_fused8``,
read with ``getenv`` in ``capi.hip``.  Comments may still speak of them."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ed-gated-gcn_amd", "csrc")
RUN_TIME = {"GGCN_LAB_BLOCK8_ROWMAJOR", "GGCN_LAB_BLOCK8_NODMA", "GGCN_LAB_BLOCK8_SAMESLOTS", "GGCN_LAB_BLOCK8_PRIO"}


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return _strip_comments(f.read())


def test_no_compile_time_lab_switch_outside_comments():
    sources = sorted(n for n in os.listdir(CSRC) if n.endswith((".hip", ".h")))
    assert "capi.hip" in sources and "f16mx8_core.h" in sources
    read_at_run_time = set()
    for name in sources:
        text = _read(name)
        if name == "capi.hip":   # the experiment's switches, and only as the argument of a getenv
            read_at_run_time = set(re.findall(r'\bgetenv\(\s*"(GGCN_LAB_\w+)"\s*\)', text))
            text = re.sub(r'\bgetenv\(\s*"GGCN_LAB_\w+"\s*\)', "getenv()", text)
        left = sorted(set(re.findall(r"GGCN_LAB_\w+", text)))
        assert not left, "%s still uses %s" % (name, ", ".join(left))
    assert read_at_run_time == RUN_TIME


def test_every_header_the_makefile_names_exists():
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = re.sub(r"#[^\n]*", "", f.read())
    m = re.search(r"^HDRS\s*:?=\s*(.*)$", mk, flags=re.M)
    assert m, "the Makefile no longer defines HDRS"
    headers = m.group(1).split()
    assert headers and all(h.endswith(".h") for h in headers)
    missing = [h for h in headers if not os.path.isfile(os.path.join(CSRC, h))]
    assert not missing, "HDRS names %s, which do not exist" % ", ".join(missing)
