"""Characterisation table of the launch-path predicates: what every public ``takes_*`` answers over a grid of shapes,
dtypes, precisions and options, on a machine without a GPU, in seconds.

    python tools/dispatch_table.py                # writes tests/golden/dispatch_table.json
    python tools/dispatch_table.py --out FILE

The committed ``tests/golden/dispatch_table.json`` was written by this tool at commit a515e3d ("Gradient with respect to a
real-valued adjacency"), the parent of the change that moved the dispatch rules into ``dispatch.py``;
``tests/test_dispatch_table_cpu.py`` regenerates it from the checked-out code and compares entry by entry.  Only the public
predicates are called, so the tool runs unchanged on both sides of that change.

How the predicates are driven without a device: ``text`` is a ``device="meta"`` tensor (nothing is allocated, so
``B*T*F >= 2**32`` costs nothing) viewed as a ``torch.Tensor`` subclass whose ``is_cuda`` is True; the CSR is a namespace with
the attributes the predicates read; ``torch.cuda.get_device_properties`` answers 256 compute units (the MI355X's) while the
table is built, and ``torch.zeros`` hands out the same subclass (stand-ins a predicate may build for layer 2's input).

Layer cases hold one bit per predicate of ``LAYER_COLUMNS`` (bit i = column i) plus, from bit ``len(LAYER_COLUMNS)`` up, the
index in ``PRECISIONS`` of ``kernel_precision(rows, csr)``; block cases one bit per predicate of ``BLOCK_COLUMNS``.  The file
stores each case as ``LAYER_DIGITS`` / ``BLOCK_DIGITS`` hexadecimal digits, cases in grid order."""
import argparse
import contextlib
import itertools
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from ed_gated_gcn_amd import gated_block  # noqa: E402
from ed_gated_gcn_amd.gcn import GraphConvolution  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "dispatch_table.json")
CUS = 256   # the MI355X's compute units
PRECISIONS = ("bf16x3", "f16mx8", "f16mx6", "fp32", "f16")
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
TS = (1, 32, 33, 47, 48, 64, 65, 95, 96, 128, 129, 160, 161, 192, 193, 256, 257, 512, 513)   # every edge of every rule
BS = (5, 128, 230, 256, 512)   # x 3 column tiles of 256: 15, 384, 690 workgroups miss whole rounds of 256 CUs, 768 and 1536 fill them
H = 768
FUSED_MAX_TS = (32, 128, 256)
LAYER_COLUMNS = ("takes_fused_path", "takes_bf16_fused_path", "takes_bf16_wide_path", "takes_bf16_dropout_path",
                 "takes_weighted_path", "takes_long_path", "takes_dropout_path")
BLOCK_COLUMNS = ("takes_block_path", "takes_folded_eval_path", "takes_bf16_block_path", "takes_bf16_folded_eval_path")
LAYER_DIGITS, BLOCK_DIGITS = 3, 1
# shapes beside the cross: widths off the long path's K % 64 / F % 8 and the fp6 kernel's K % 32, one column tile, and element
# indices B*T*F on both sides of 2**32 (the limit of the dropout paths) -- (B, T, K, F)
EXTRA_SHAPES = ((128, 200, 96, 768), (128, 200, 768, 12), (128, 200, 768, 100), (512, 160, 768, 256), (2, 24, 48, 64),
                (8192, 512, 768, 1024), (8191, 512, 768, 1024), (65536, 32, 768, 2048), (65536, 256, 768, 256), (65535, 256, 768, 256))
BLOCK_TS = (1, 32, 33, 47, 48, 128, 129, 161, 193, 256, 257, 513)
BLOCK_BS = (128, 512)
BLOCK_GRAPHS = (("binary", True), ("binary", False), ("weighted", True))             # (adjacency, row masks)
BLOCK_OPTIONS = ((128, True, True), (256, True, True), (128, True, False))           # (fused_max_t, gc1.fused, gc2.fused)


def _read_once(name):
    """A tensor attribute read through torch once per tensor: the predicates read these a million times, and every read of a
    subclass's attribute goes through ``__torch_function__``."""
    read = getattr(torch.Tensor, name).__get__

    def get(self):
        if name not in self.__dict__:
            self.__dict__[name] = read(self)
        return self.__dict__[name]
    return property(get)


class GpuMeta(torch.Tensor):
    """A meta tensor that says it lives on the GPU."""
    is_cuda = property(lambda self: True)
    dtype, shape, device = _read_once("dtype"), _read_once("shape"), _read_once("device")


def features(B, T, K, dtype):
    return torch.empty(B, T, K, dtype=dtype, device="meta").as_subclass(GpuMeta)


def graph(B, T, binary, masks, operands):
    """What the predicates read of a ``BatchedCSR``."""
    on_gpu = types.SimpleNamespace(is_cuda=True)
    return types.SimpleNamespace(B=B, T=T, is_binary=binary, rowmask=on_gpu if masks else None,
                                 graph_ops_weighted=lambda plane: on_gpu if operands else None)


def layer(K, F, precision, fused=True, fused_max_t=128, bf16_block=False):
    return GraphConvolution(K, F, opt=types.SimpleNamespace(ggcn_precision=precision, ggcn_fused=fused, ggcn_fused_max_t=fused_max_t,
                                                            ggcn_bf16_block=bf16_block))


@contextlib.contextmanager
def pretend_device():
    props, zeros = torch.cuda.get_device_properties, torch.zeros
    torch.cuda.get_device_properties = lambda device=None: types.SimpleNamespace(multi_processor_count=CUS)
    torch.zeros = lambda *a, **k: zeros(*a, **k).as_subclass(GpuMeta)
    saved = {k: os.environ.pop(k) for k in ("GGCN_PRECISION", "GGCN_FUSED", "GGCN_FUSED_MAX_T", "GGCN_BF16_BLOCK", "GGCN_WEIGHTED_MAX_T") if k in os.environ}
    try:
        yield
    finally:
        torch.cuda.get_device_properties, torch.zeros = props, zeros
        os.environ.update(saved)


def layer_cases():
    """``(label, layer, text, csr)`` of every layer case, in file order."""
    shapes = [(B, T, H, H) for T in TS for B in BS] + list(EXTRA_SHAPES)
    layers = {}
    for precision, fmt, fused in itertools.product(PRECISIONS, FUSED_MAX_TS, (True, False)):
        for K, F in sorted({s[2:] for s in shapes}):
            layers[precision, fmt, fused, K, F] = layer(K, F, precision, fused, fmt)
    for (B, T, K, F), dtype in itertools.product(shapes, DTYPES):
        text = features(B, T, K, dtype)
        for binary, masks, operands in itertools.product((True, False), (True, False), (True, False)):
            csr = graph(B, T, binary, masks, operands)
            for precision, fmt, fused in itertools.product(PRECISIONS, FUSED_MAX_TS, (True, False)):
                label = "B=%d T=%d K=%d F=%d %s %s masks=%s operands=%s precision=%s fused_max_t=%d fused=%s" % (
                    B, T, K, F, str(dtype)[6:], "binary" if binary else "weighted", masks, operands, precision, fmt, fused)
                yield label, layers[precision, fmt, fused, K, F], text, csr


def block_cases():
    """``(label, x, csr, gc1, gc2)`` of every block case, in file order."""
    pairs = {}
    for precision, equal, (fmt, fused1, fused2), on, square in itertools.product(PRECISIONS, (True, False), BLOCK_OPTIONS,
                                                                                  (True, False), (True, False)):
        other = precision if equal else ("bf16x3" if precision != "bf16x3" else "f16mx8")
        pairs[precision, equal, fmt, fused2, on, square] = (layer(H, H, precision, fused1, fmt, on),
                                                            layer(H, H if square else 512, other, fused2, fmt, on))
    for T, B, dtype in itertools.product(BLOCK_TS, BLOCK_BS, DTYPES):
        x = features(B, T, H, dtype)
        for adjacency, masks in BLOCK_GRAPHS:
            csr = graph(B, T, adjacency == "binary", masks, True)
            for (precision, equal, fmt, fused2, on, square), (gc1, gc2) in pairs.items():
                label = "B=%d T=%d %s %s masks=%s precision=%s/%s fused_max_t=%d gc2.fused=%s bf16_block=%s %s" % (
                    B, T, str(dtype)[6:], adjacency, masks, precision, gc2.precision, fmt, fused2, on, "square" if square else "H->512")
                yield label, x, csr, gc1, gc2


def layer_entry(m, text, csr):
    v = 0
    for i, name in enumerate(LAYER_COLUMNS):
        answer = getattr(m, name)(text, csr)
        assert answer is True or answer is False, (name, answer)
        v |= int(answer) << i
    rows = text.reshape(text.shape[0] * text.shape[1], text.shape[2])
    return v | PRECISIONS.index(m.kernel_precision(rows, csr)) << len(LAYER_COLUMNS)


def block_entry(x, csr, gc1, gc2):
    v = 0
    for i, name in enumerate(BLOCK_COLUMNS):
        answer = getattr(gated_block, name)(x, csr, gc1, gc2)
        assert answer is True or answer is False, (name, answer)
        v |= int(answer) << i
    return v


def build_table():
    with pretend_device():
        lay = [layer_entry(*c[1:]) for c in layer_cases()]
        blk = [block_entry(*c[1:]) for c in block_cases()]
    return {"cus": CUS, "layer_columns": list(LAYER_COLUMNS), "block_columns": list(BLOCK_COLUMNS), "precisions": list(PRECISIONS),
            "layer_digits": LAYER_DIGITS, "block_digits": BLOCK_DIGITS, "layer_cases": len(lay), "block_cases": len(blk),
            "layer": "".join("%0*x" % (LAYER_DIGITS, v) for v in lay), "block": "".join("%0*x" % (BLOCK_DIGITS, v) for v in blk)}


def decode(text, digits):
    return [int(text[i:i + digits], 16) for i in range(0, len(text), digits)]


def dumps(table):
    return json.dumps(table, indent=0, sort_keys=True) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    table = build_table()
    with open(args.out, "w") as f:
        f.write(dumps(table))
    for key, columns in (("layer", LAYER_COLUMNS), ("block", BLOCK_COLUMNS)):
        vals = decode(table[key], table[key + "_digits"])
        print("%s: %d cases; True answers per column: %s" % (key, len(vals), {c: sum(v >> i & 1 for v in vals) for i, c in enumerate(columns)}))


if __name__ == "__main__":
    main()
