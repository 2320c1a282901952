"""Every translation unit that can raise the f16mx8 range flag has a reader that registers itself with ``ggcn_range_flag`` (text
only, no GPU).

``static __device__ unsigned int g_range_flag`` (``f16mx8_core.h``) is ONE COPY PER TRANSLATION UNIT: a ``.hip`` file's reports reach
``ggcn_range_flag`` only if the file expands ``GGCN_RANGE_FLAG_TU(name)``, which defines the copy's reader and registers it when the
library is loaded.  A new ``.hip`` that instantiates ``mx8::mainloop`` and forgets the macro compiles, runs and never reports.  This
test reads ``csrc/*.hip`` with the project's own ``#include "..."`` lines resolved transitively, comments stripped.  That the reports
arrive is ``test_gpu_range_report.py``'s to prove, at run time.

What counts as "makes a verdict": an instantiation ``mx8::mainloop<`` / ``mx6::mainloop<``, a call ``range_verdict(`` or the word
``g_range_flag`` -- looked for in the ``.hip`` itself and in every header it includes EXCEPT the headers that define the flag or a
main loop (``f16mx8_core.h``, ``f16mx6_core.h``): what those define are inline templates that emit nothing until a ``.hip`` names
them, so including them alone makes no verdict (``fused_long.hip``)."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ed-gated-gcn_amd", "csrc")
MX6_GUARD = "GGCN_WITH_F16MX6"
VERDICT = re.compile(r"\bmx[68]::mainloop\s*<|\brange_verdict\s*\(|\bg_range_flag\b")
READER = re.compile(r"^\s*GGCN_RANGE_FLAG_TU\(\s*(\w+)\s*\)", re.M)


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return _strip_comments(f.read())


def _includes(name, seen=None):
    """The project's own headers ``name`` includes, transitively (those that live in csrc/)."""
    seen = set() if seen is None else seen
    for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', _read(name), flags=re.M):
        if inc not in seen and os.path.exists(os.path.join(CSRC, inc)):
            seen.add(inc)
            _includes(inc, seen)
    return seen


def _hips():
    return sorted(n for n in os.listdir(CSRC) if n.endswith(".hip"))


def _definers():
    """Headers that define the flag word or a split-precision main loop."""
    return sorted(n for n in os.listdir(CSRC) if n.endswith(".h")
                  and re.search(r"static\s+__device__\s+unsigned\s+int\s+g_range_flag|\bvoid\s+mainloop\s*\(", _read(n))
                  and re.search(r"namespace\s+mx[68]\b", _read(n)))


def _makes_verdict(hip):
    own = [hip] + sorted(h for h in _includes(hip) if h not in _definers())
    return any(VERDICT.search(_read(n)) for n in own)


def _range_flag_body():
    text = _read("capi.hip")
    m = re.search(r"\bint\s+ggcn_range_flag\s*\([^)]*\)\s*\{", text)
    assert m, "capi.hip no longer defines ggcn_range_flag"
    depth, i = 1, m.end()
    while depth:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        i += 1
    return text[m.end():i - 1]


def _macro_definition():
    """The ``#define GGCN_RANGE_FLAG_TU`` of ``f16mx8_core.h`` with its continuation lines."""
    m = re.search(r"^\s*#\s*define\s+GGCN_RANGE_FLAG_TU\b(?:[^\n]*\\\n)*[^\n]*", _read("f16mx8_core.h"), flags=re.M)
    assert m, "f16mx8_core.h no longer defines GGCN_RANGE_FLAG_TU"
    return m.group(0)


def _optional_sources():
    """``.hip`` files the Makefile compiles under ``F16MX6=1`` only, the build that defines ``GGCN_WITH_F16MX6``: the file names
    between the Makefile's ``F16MX6`` conditional and its ``endif``, however they are laid out.  The two source lists partition
    ``csrc/*.hip``, and every object is linked by name, so no reader's registration can be left out of the library."""
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = re.sub(r"#[^\n]*", "", f.read())
    m = re.search(r"^ifn?eq[^\n]*F16MX6[^\n]*\n(.*?)^endif", mk, flags=re.S | re.M)
    assert m and MX6_GUARD in m.group(1), "the Makefile no longer has an F16MX6 block that defines " + MX6_GUARD
    extra = set(re.findall(r"\b(\w+\.hip)\b", m.group(1)))
    always = set(re.findall(r"\b(\w+\.hip)\b", mk[:m.start()] + mk[m.end():]))
    assert not (extra & always) and sorted(extra | always) == _hips(), "a .hip file is in neither source list of the Makefile, or in both"
    return extra


def test_the_headers_that_define_the_flag_and_the_main_loops():
    assert _definers() == ["f16mx6_core.h", "f16mx8_core.h"]
    assert READER.search(_read("f16mx8_core.h")) is None      # the macro's definition is a #define line, not an expansion


def test_every_file_that_makes_a_verdict_has_one_reader_that_ggcn_range_flag_calls():
    assert _optional_sources() == {"fused6.hip"}
    reporters = [h for h in _hips() if _makes_verdict(h)]
    # today's list, so that a change of it shows up here
    assert reporters == ["fused6.hip", "fused_block8.hip", "fused_layer.hip", "fused_weighted_drop.hip", "fused_wide.hip",
                         "fused_wide8.hip", "linear_split.hip"]
    names = {}
    for hip in reporters:
        found = READER.findall(_read(hip))
        assert len(found) == 1, "%s makes range verdicts and expands GGCN_RANGE_FLAG_TU %d times (exactly once is needed)" % (hip, len(found))
        name = found[0]
        assert name not in names, "%s and %s define the same reader %s" % (hip, names.get(name), name)
        names[name] = hip
    # the converse: every reader defined anywhere is one of the above
    everywhere = {n: h for h in _hips() for n in READER.findall(_read(h))}
    assert everywhere == names, "a file without verdicts expands GGCN_RANGE_FLAG_TU: %s" % sorted(set(everywhere) - set(names))


def test_the_macro_registers_its_reader_and_ggcn_range_flag_names_none():
    """What replaced the declarations in ``common.h`` and the call list in ``capi.hip``: expanding the macro is all a file has to do."""
    assert re.search(r"\bregister_range_flag_reader\s*\(\s*fn\s*\)", _macro_definition()), \
        "GGCN_RANGE_FLAG_TU no longer registers the reader it defines"
    body = _range_flag_body()
    assert not re.search(r"\brange_flag_\w+", body), "ggcn_range_flag names a reader"
    assert not re.search(r"^\s*#", body, flags=re.M), "ggcn_range_flag has a preprocessor line (the F16MX6 build needs none)"
    assert not re.search(r"\brange_flag_\w+", _read("common.h")), "common.h declares a reader"


def test_files_that_include_the_flag_header_without_making_a_verdict():
    """Allowed (nothing to report), but listed: a file moving onto or off this list is a change someone should look at."""
    idle = [h for h in _hips() if set(_definers()) & _includes(h) and not _makes_verdict(h)]
    assert idle == ["fused_long.hip"]
    for hip in idle:
        assert not READER.findall(_read(hip))
