"""WHAT THE CPU-SIDE TESTS OF THE C ABI SHARE (test infrastructure, NOT product code)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    """include/ggcn.h without its comments."""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ggcn.h")).read(), flags=re.S)


def msg(lib, rc, code, who=None):
    """The library's last error text, after asserting that the call returned ``code`` (and, with ``who``, that the text names the
    entry that refused)."""
    text = lib.ggcn_last_error().decode()
    assert rc == code, (rc, text)
    assert who is None or text.startswith(who + ":"), text
    return text
