"""What the fifteen one-launch entries of libggcn_hip.so REFUSE, call by call, on a machine without a GPU.

    python tools/fused_refusals.py                # writes tests/golden/fused_refusals.json
    python tools/fused_refusals.py --out FILE
    GGCN_LIB=/path/to/libggcn_hip.so python tools/fused_refusals.py --out FILE     # another build of the library

The entries are the ten ``ggcn_layer_fused*`` (without ``ggcn_layer_fused_h``, which shares none of their host code), the three
``ggcn_block_fused*``, ``ggcn_lab_block_fused8`` and ``ggcn_debug_block_fused_stamped``.  Each gets one or more BASE calls -- valid
calls on distinct fake 16-byte aligned pointers, as ``tests/test_host_cpu.py`` makes them -- and from every base every SINGLE-FAULT
variant (``variants`` below).  What the library answers with ``GGCN_EINVAL`` or ``GGCN_EUNSUPPORTED`` is recorded as
``entry -> variant -> [code, message]``; what it accepts is counted only.

The pointers are fake, so this tool exits at once where ``torch.cuda.is_available()``: an accepted call launches, and nothing of
this may run where a launch could reach a card.  Without a device an accepted call ends in ``GGCN_ELAUNCH``.

The committed ``tests/golden/fused_refusals.json`` was written by this tool from a build of commit c5b58e5 ("Test ggcn_aggregate /
ggcn_aggregate_h against float64 on every form"), the parent of the change that made the C entries fill ``FusedArgs`` themselves;
``tests/test_fused_refusals_cpu.py`` replays it against the checked-out library.

It also reads the ``fail(...)`` format strings of the host functions behind these entries out of the sources and prints the ones
no recorded message matches: a refusal a fake-pointer call can reach and no variant reaches is a hole in the table."""
import argparse
import json
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "fused_refusals.json")
HEADER = os.path.join(ROOT, "include", "ggcn.h")
CSRC = os.path.join(ROOT, "ed-gated-gcn_amd", "csrc")
EINVAL, EUNSUPPORTED = 1, 3
F16MX8 = 2
BIG = dict(B=2048, T=32, K=768, F=768)   # 512 row blocks x 3 column slices = 6 rounds of 256 CUs (no device: 256): the eight-wavefront side

# entry -> the shapes of its base calls (the entry's range of T; B = 8, K = 64, F = 256 unless given)
ENTRIES = {
    "ggcn_layer_fused": [dict(T=20)],
    "ggcn_layer_fused_prebias": [dict(T=40), dict(T=200)],          # 33..256 nodes
    "ggcn_layer_fused_drop": [dict(T=20)],
    "ggcn_layer_fused_weighted": [dict(T=20)],
    "ggcn_layer_fused_weighted_drop": [dict(T=20)],
    "ggcn_layer_fused_weighted_wide": [dict(T=40), dict(T=100)],    # 33..128 nodes: the 64- and the 128-row slot
    "ggcn_layer_fused_weighted_wide_drop": [dict(T=40), dict(T=100)],
    "ggcn_layer_fused_bf16": [dict(T=20)],
    "ggcn_layer_fused_bf16_drop": [dict(T=20)],
    "ggcn_layer_fused_bf16_wide": [dict(T=40), dict(T=200)],        # 33..256 nodes: the row masks alone, and with edge lists
    "ggcn_block_fused": [dict(T=20), BIG],
    "ggcn_block_fused_weighted": [dict(T=20)],
    "ggcn_block_fused_bf16": [dict(T=20)],
    "ggcn_lab_block_fused8": [dict(T=20), BIG],
    "ggcn_debug_block_fused_stamped": [dict(T=20)],
}
T_RANGE = {"ggcn_layer_fused": (1, 256), "ggcn_layer_fused_drop": (1, 256), "ggcn_layer_fused_prebias": (33, 256),
           "ggcn_layer_fused_weighted_wide": (33, 128), "ggcn_layer_fused_weighted_wide_drop": (33, 128),
           "ggcn_layer_fused_bf16_wide": (33, 256)}   # every other entry: 1..32
LAYER1_OUTPUTS = ("x1", "y1", "gcn1", "overlap_partial")
LAYER1_INPUTS = ("wpack1", "gate1", "graph_ops", "graph_opsw", "zero_mid")   # what the eval form does not read


def prototypes():
    """entry -> [(type, name)] from include/ggcn.h."""
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    out = {}
    for name in ENTRIES:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        params = []
        for p in m.group(1).split(","):
            t, n = re.match(r"\s*(.*?)(\w+)\s*$", p, flags=re.S).groups()
            params.append((" ".join(t.split()), n))
        out[name] = params
    return out


def base_call(params, shape):
    """A valid call: every pointer its own fake address (NULL stream), leading dimensions at their minimum."""
    s = dict(dict(B=8, K=64, F=256), **shape)
    a, n_ptr = {}, 0
    for t, n in params:
        if n == "stream":
            a[n] = None
        elif "*" in t:
            a[n] = 0x10000000 + 0x100000 * n_ptr
            n_ptr += 1
        elif n in s:
            a[n] = s[n]
        elif n.startswith("ld"):
            a[n] = s["K"] if n == "ldx" else s["F"]
        else:
            a[n] = {"precision": F16MX8, "p": 0.25, "seed": 12345, "stream_store": 1, "stream_a": 2, "stream_b": 0}[n]
    if shape is BIG and "gcn1" in a:
        a["gcn1"] = None   # the eight-wavefront kernel writes every output but gcn1
    return a


def variants(entry, params, base):
    """(label, arguments) of every single-fault variant of `base`; the label is the key of the table."""
    names = [n for _, n in params]
    ptrs = [n for t, n in params if "*" in t and n != "stream"]
    lds = [n for n in names if n.startswith("ld")]

    def var(**kw):
        return dict(base, **kw)

    def faults(a, tag=""):
        for n in ptrs:
            if a[n] is not None:
                yield "%s%s=NULL" % (tag, n), dict(a, **{n: None})
                yield "%s%s+8" % (tag, n), dict(a, **{n: a[n] + 8})
        if "bf16" in entry and a["X"] is not None:
            yield tag + "X+1", dict(a, X=a["X"] + 1)
        for n in "BTKF":
            yield "%s%s=0" % (tag, n), dict(a, **{n: 0})
        lo, hi = T_RANGE.get(entry, (1, 32))
        if lo > 1:
            yield "%sT=%d" % (tag, lo - 1), dict(a, T=lo - 1)
        yield "%sT=%d" % (tag, hi + 1), dict(a, T=hi + 1)

    yield "base", dict(base)
    yield from faults(base)
    for n in lds:
        yield "%s-1" % n, var(**{n: base[n] - 1})
        yield "%s=2^31" % n, var(**{n: 1 << 31})
    if "precision" in base:
        for prec in range(6):
            yield "precision=%d" % prec, var(precision=prec)
    if "p" in base:
        for p in (-0.25, 1.0):
            yield "p=%g" % p, var(p=p)
        for n in ("stream_store", "stream_a", "stream_b"):
            yield "%s=3" % n, var(**{n: 3})
        b = -(-(1 << 32) // (base["T"] * base["F"]))
        yield "B*T*F=2^32", var(B=b)
        yield "B*T*F=2^32,p=0", var(B=b, p=0.0)
    # a grid beyond 2^31 workgroups: 2^29 row blocks (2^31 - 1 graphs) x 8 column tiles
    yield "grid>2^31", var(B=(1 << 31) - 1, F=2048, **{n: 2048 for n in lds if n != "ldx"})
    if "pool_a" in base:   # the layers: nothing to write
        yield "out=NULL,pool_a=NULL,pool_b=NULL", var(out=None, pool_a=None, pool_b=None)
    if "x1" in base:   # the blocks: layer 1 in part, and the eval form
        have = [n for n in LAYER1_OUTPUTS if n in base]
        for gone in (("x1", "y1"), ("x1", "y1", "overlap_partial"), ("x1", "y1", "gcn1")):
            yield "NULL:" + "+".join(gone), var(**{n: None for n in gone if n in base})
        yield "x_out=NULL,pool_out=NULL", var(x_out=None, pool_out=None)
        ev = var(**{n: None for n in have})
        yield "eval", ev
        ev = dict(ev, **{n: None for n in LAYER1_INPUTS if n in base})
        yield "eval,no layer 1 inputs", ev
        yield from faults(ev, "eval:")


def call(lib, entry, params, a):
    rc = getattr(lib, entry)(*[a[n] for _, n in params])
    return rc, lib.ggcn_last_error().decode()


def cases(entry, params):
    """Every (label, arguments) of `entry`, over all of its bases."""
    for shape in ENTRIES[entry]:
        tag = "B=%d,T=%d" % (shape.get("B", 8), shape["T"])
        for label, a in variants(entry, params, base_call(params, shape)):
            yield "%s/%s" % (tag, label), a


def load():
    if torch.cuda.is_available():
        sys.exit("fused_refusals: a GPU is visible -- these are fake pointers, and an accepted call would launch on them")
    from ed_gated_gcn_amd import _capi
    return _capi.load_library()


def record(lib):
    protos, table, counts = prototypes(), {}, dict(enumerated=0, refused=0, accepted=0)
    for entry in ENTRIES:
        table[entry] = {}
        for label, a in cases(entry, protos[entry]):
            rc, msg = call(lib, entry, protos[entry], a)
            counts["enumerated"] += 1
            if rc in (EINVAL, EUNSUPPORTED):
                table[entry][label] = [rc, msg]
                counts["refused"] += 1
            else:
                counts["accepted"] += 1
    return table, counts


# ---- the refusal sites of the sources ---------------------------------------------------------------------------------------------
# the host functions behind the fifteen entries, before and after the C entries filled FusedArgs themselves (absent names are skipped)
SOURCES = {
    "capi.hip": list(ENTRIES) + ["drop_entry_checks", "entry_drop_spec", "layer_entry_checks", "block_entry_checks"],
    "fused_layer.hip": ["fused_part_checks", "launch_fused", "launch_block", "layer_fused", "layer_fused_weighted",
                        "layer_fused_weighted_drop", "layer_fused_bf16", "block_fused", "block_fused_weighted", "block_fused_bf16"],
    "fused_wide.hip": ["launch_fused_weighted_wide", "layer_fused_weighted_wide"],
    "fused_block8.hip": ["block_fused8", "lab_block_fused8"],
}
FAIL = re.compile(r'\bfail\(\s*GGCN_E\w+\s*,\s*"((?:[^"\\]|\\.)*)"')
SPEC = {"%s": ".*", "%d": r"-?\d+", "%lld": r"-?\d+", "%g": r"[-+.\de]+", "%%": "%"}


def _body(text, name):
    """(offset, text) of the body of the host function `name`, or None."""
    m = re.search(r"^(?:int|bool)\s+%s\s*\([^)]*\)\s*\{" % name, text, flags=re.M)
    if not m:
        return None
    depth, i = 1, m.end()
    while depth:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        i += 1
    return m.end(), text[m.end():i]


def _under_mx6(before):
    """Whether the text after `before` stands between an #if(n)def GGCN_WITH_F16MX6 and its #endif."""
    stack = []
    for line in before.splitlines():
        if re.match(r"\s*#\s*if", line):
            stack.append("GGCN_WITH_F16MX6" in line)
        elif re.match(r"\s*#\s*endif", line) and stack:
            stack.pop()
    return any(stack)


def refusal_sites():
    """[(file, line, function, format string, under an #if of GGCN_WITH_F16MX6)] of the functions of SOURCES."""
    sites = []
    for fname, funcs in SOURCES.items():
        with open(os.path.join(CSRC, fname)) as f:
            text = f.read()
        for func in funcs:
            found = _body(text, func)
            if not found:
                continue
            for m in FAIL.finditer(found[1]):
                before = text[:found[0] + m.start()]
                sites.append((fname, before.count("\n") + 1, func, m.group(1), _under_mx6(before)))
    return sites


def unmatched_sites(table):
    messages = [msg for per in table.values() for _, msg in per.values()]
    out = []
    for fname, line, func, fmt, guarded in refusal_sites():
        pattern = "".join(SPEC.get(tok, re.escape(tok)) for tok in re.split(r"(%lld|%[sdg%])", fmt.replace('\\"', '"')))
        if not any(re.fullmatch(pattern, msg, flags=re.S) for msg in messages):
            out.append("%s:%d %s%s: %s" % (fname, line, func, " [#if GGCN_WITH_F16MX6]" if guarded else "", fmt))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    table, counts = record(load())
    with open(args.out, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write("\n")
    print("enumerated %(enumerated)d, refused %(refused)d, accepted %(accepted)d" % counts)
    missing = unmatched_sites(table)
    print("%d refusal sites no recorded message matches:" % len(missing))
    for line in missing:
        print("  " + line)


if __name__ == "__main__":
    main()
