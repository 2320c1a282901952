"""Which launch a layer call, its backward and a block call take: every rule in one place, decided once per call.

Host logic only -- nothing here loads libggcn_hip.so or launches.  ``layer_launch``, ``backward_launch`` and ``block_launch`` return
names out of fixed tuples; ``_forward_gated``, ``_GatedLayerFunction.backward`` and ``_gated_gcn_block`` call them once and look
the answer up.  ``layer_launch`` / ``backward_launch`` / ``block_launch`` are ``layer_path`` / ``backward_plan`` / ``block_path`` (whose
answers ``tests/golden/dispatch_table.json`` pins) plus the names of the opt-in weighted launches.  The public ``takes_*`` predicates are
one-line statements over the functions below (their docstrings keep the measurements behind the thresholds).  DESIGN.md "Dispatch"."""
import collections
import os

import torch

from . import _capi

# precisions that mean "the bf16 pair form" for bfloat16 features: x is exact in bf16, so every product is hi.Whi + hi.Wlo,
# two bf16 MFMAs on the bf16x3 image of W (include/ggcn.h ggcn_linear_bf16)
BF16_PRECISIONS = ("bf16x3", "f16mx8", "f16mx6")

LAYER_PATHS = ("fused", "fused_drop", "bf16", "bf16_drop", "bf16_wide", "bf16_wide_drop", "weighted", "long", "two_launch")
DROPOUT_PATHS = ("fused_drop", "bf16_drop", "bf16_wide_drop")           # the gates' dropout is drawn inside these launches
OVERLAP_PATHS = LAYER_PATHS[:6]                                         # launches that take overlap_partial / overlap_reduce
BACKWARD_PASSES = ("mma", "one_pass", "two_pass", "two_pass_drop")
# what is launched: the pinned names above plus the opt-in launches on a real-valued adjacency
LAYER_LAUNCHES = LAYER_PATHS + ("weighted_wide", "weighted_drop", "weighted_wide_drop")
DROPOUT_LAUNCHES = DROPOUT_PATHS + ("weighted_drop", "weighted_wide_drop")
OVERLAP_LAUNCHES = OVERLAP_PATHS
BACKWARD_LAUNCHES = BACKWARD_PASSES + ("weighted", "weighted_drop", "wide", "weighted_wide")   # ... plus the opt-in one-launch backwards
DX_FORMS = ("bf16", "scaled", "bf16x3", "fp32")                         # the dW forms are these without "scaled"
BLOCK_PATHS = ("block", "bf16_block", "folded_eval", "bf16_folded_eval", "two_fused", "layers_eval", "layers")
BLOCK_LAUNCHES = BLOCK_PATHS + ("weighted_block",)                    # the pinned names plus the opt-in block on a real-valued adjacency
WEIGHTED_BLOCK_PRECISIONS = ("bf16x3", "f16mx8")


class Input(collections.namedtuple("Input", "dtype B T gpu")):
    """What the rules read of a layer's features: dtype, batch size, graph length and the GPU they are on (None: not on one).
    gc2 of a block is judged by ``of(x, torch.float32)``: it reads gcn1, float32 whatever x is, with x's B, T and device."""
    @classmethod
    def of(cls, text, dtype=None):
        return cls(dtype or text.dtype, text.shape[0], text.shape[1], text.device if text.is_cuda else None)


def edge_lists(csr):
    """The graphs' edge lists for the row-mask kernels of > 32 (float32) / > 128 (bfloat16) nodes; GGCN_EDGE_LISTS=0: the masks alone."""
    return csr.edge_lists if os.environ.get("GGCN_EDGE_LISTS", "1") != "0" else None


# ---- one layer --------------------------------------------------------------------------------------------------------------
def _one_launch_base(layer, csr, precisions):
    """What every row-mask launch needs: the ``fused`` option, a split precision, a 0/1 adjacency and its row masks."""
    return bool(layer.fused and layer.precision in precisions and csr.rowmask is not None and csr.is_binary)


def _fills_whole_rounds(layer, B, device):
    """One workgroup per graph x 256 columns: at least two rounds of the GPU's CUs, the last one ``WIDE_AUTO_FILL`` full."""
    if device is None:
        return False
    wgs = B * ((layer.out_features + 255) // 256)
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    rounds = -(-wgs // cus)
    return rounds >= 2 and wgs >= layer.WIDE_AUTO_FILL * rounds * cus


def _index_fits(layer, inp):
    return inp.B * inp.T * layer.out_features < 2 ** 32   # the dropout hash takes a 32-bit element index


def takes_fused(layer, csr, inp):
    if not (_one_launch_base(layer, csr, _capi.PACKED) and inp.dtype == torch.float32):
        return False
    if csr.T <= layer.fused_max_t:
        return True
    if layer.fused_max_t < 128 or csr.T > 256:
        return False
    if csr.T >= layer.WIDE_AUTO_MIN_T:
        return True
    return csr.T >= layer.WIDE_AUTO_MIN_T_FULL.get(layer.precision, 161) and _fills_whole_rounds(layer, inp.B, inp.gpu)


def _bf16_base(layer, csr, inp):
    return _one_launch_base(layer, csr, BF16_PRECISIONS) and inp.dtype == torch.bfloat16 and bool(csr.rowmask.is_cuda)


def takes_bf16_fused(layer, csr, inp):
    return _bf16_base(layer, csr, inp) and csr.T <= 32 and csr.T <= layer.fused_max_t


def takes_bf16_wide(layer, csr, inp):
    if not (_bf16_base(layer, csr, inp) and 32 < csr.T <= 256):
        return False
    if layer.fused_max_t >= 256:
        return True
    if csr.T <= 128:
        slot = 64 if csr.T <= 64 else 128
        return csr.T <= layer.fused_max_t and csr.T >= layer.BF16_WIDE_MIN_FILL * slot
    return layer.fused_max_t >= 128 and _fills_whole_rounds(layer, inp.B, inp.gpu)


def takes_dropout(layer, csr, inp):
    return takes_fused(layer, csr, inp) and _index_fits(layer, inp)


def takes_bf16_dropout(layer, csr, inp):
    return (takes_bf16_fused(layer, csr, inp) or takes_bf16_wide(layer, csr, inp)) and _index_fits(layer, inp)


def takes_weighted(layer, csr, inp):
    if not (layer.fused and layer.precision in _capi.PACKED and not csr.is_binary and inp.dtype == torch.float32 and inp.gpu is not None):
        return False
    if csr.T <= 32:
        return bool(layer.fused_max_t >= 32 and csr.graph_ops_weighted(0 if layer.precision == "bf16x3" else 1) is not None)
    # 33..128 nodes: the opt-in ``weighted_max_t`` (32 by default) -- looked at BEFORE the graph is asked for its operand blocks
    return bool(csr.T <= min(getattr(layer, "weighted_max_t", 32), 128) and csr.graph_ops_weighted_wide() is not None)


def takes_weighted_dropout(layer, csr, inp):
    """True when the gates' training-mode dropout (``bert_amir5.py:621-625``) on a REAL-valued adjacency is drawn inside the
    weighted layer launch (``ggcn_layer_fused_weighted_drop`` for graphs of <= 32 nodes, ``ggcn_layer_fused_weighted_wide_drop``
    for 33..``weighted_max_t``): the option ``layer.weighted_dropout`` (``opt.ggcn_weighted_dropout`` /
    ``GGCN_WEIGHTED_DROPOUT=1``; OFF by default) -- looked at first, so that a refused call builds no operand block -- an element
    index below 2^32, and ``takes_weighted``.  ``layer_path`` does not know this path (its answers are pinned):
    ``_forward_gated`` asks here once where dropout is handed in and ``layer_path`` named no ``DROPOUT_PATHS`` launch.
    float32 features only; bfloat16 features on a weighted adjacency under dropout keep raising.
    Measured (``tools/weighted_dropout_timing.py``, one MI355X, one process, H = 768, f16mx8, p = 0.25, us per training step of
    one gated layer, per-adjacency builders inside; off = the plain weighted launch + the reference's [B,T,H] gate ops under PyTorch
    autograd, on = these launches, wb = with ``weighted_backward``): 4096 x 32 sparse 5346 / on 2322 / wb 2091 (with adj.grad
    5898 / 2855 / 2665), dense softmax rows 5754 / 2705 / 2080 (6310 / 3263 / 2697); 512 x 100 sparse 2200 / 1073 (2528 / 1405),
    dense 2974 / 1864 (3327 / 2221).  It stays opt-in, like the launches it builds on.  Not measured: the
    one-wavefront form of the 128-row slot (general f16mx8 main loop).
    The compiler's report: no scratch in any of the 22 new forward kernels."""
    return bool(getattr(layer, "weighted_dropout", False)) and _index_fits(layer, inp) and takes_weighted(layer, csr, inp)


def takes_long(layer, csr, inp):
    return bool(layer.fused and layer.precision == "f16" and inp.dtype == torch.float16
                and 128 < csr.T <= layer.LONG_MAX_T and layer.in_features % 64 == 0 and layer.out_features % 8 == 0)


def layer_path(layer, text, csr, dropout=False, rows=None):
    """The launch ``forward_gated`` takes, one of ``LAYER_PATHS``.  Precedence: fused, bf16 (33..256 nodes: bf16_wide), weighted,
    long, two launches (linear + aggregate).  ``dropout``: the caller hands gate dropout in -- a ``DROPOUT_PATHS`` name comes back
    exactly where ``takes_dropout_path`` / ``takes_bf16_dropout_path`` hold, and any other name means the request is refused;
    the weighted launch has no dropout epilogue.  ``rows``: the features as [B*T,K] rows (``ggcn_layer_fused_h`` wants them
    16-byte aligned; other views take linear_h + aggregate_h); None: not looked at."""
    inp = Input.of(text)
    drop = "_drop" if dropout and _index_fits(layer, inp) else ""
    if takes_fused(layer, csr, inp):
        return "fused" + drop
    if takes_bf16_wide(layer, csr, inp):
        return "bf16_wide" + drop
    if takes_bf16_fused(layer, csr, inp):
        return "bf16" + drop
    if not dropout and takes_weighted(layer, csr, inp):
        return "weighted"
    if takes_long(layer, csr, inp) and (rows is None or (rows.data_ptr() % 16 == 0 and rows.stride(0) % 8 == 0)):
        return "long"
    return "two_launch"


def layer_launch(layer, text, csr, dropout=False, rows=None):
    """The launch ``_forward_gated`` runs, one of ``LAYER_LAUNCHES``: ``layer_path``'s name, "weighted" told apart by graph size and,
    where dropout is handed in and ``layer_path`` named no ``DROPOUT_PATHS`` launch, ``takes_weighted_dropout`` asked once.  Under
    ``dropout`` any name outside ``DROPOUT_LAUNCHES`` means the request is refused."""
    path = layer_path(layer, text, csr, dropout, rows)
    if path == "weighted":
        return "weighted" if csr.T <= 32 else "weighted_wide"
    if dropout and path not in DROPOUT_PATHS and takes_weighted_dropout(layer, csr, Input.of(text)):
        return "weighted_drop" if csr.T <= 32 else "weighted_wide_drop"
    return path


def _aligned16(operands):
    return all(t is None or t.data_ptr() % 16 == 0 for t in operands)


def _two_pass_forced():
    return os.environ.get("GGCN_BACKWARD_TWO_PASS", "0") == "1"   # (read at call time)


def backward_plan(layer, csr, dtype, K, F, need_x, need_adj, dropout, operands):
    """``(passes, dx, dw)`` of the layer's backward: ``passes`` out of ``BACKWARD_PASSES``, ``dx`` out of ``DX_FORMS`` (None: no dX
    wanted), ``dw`` likewise.  The three environment switches are read here, at call time.
    * one pass -- gate / pool backward AND the transposed aggregation in one launch, dY never reaches memory: graphs of up to 32
      nodes, 0/1 adjacency, row masks, F % 4 == 0, every operand 16-byte aligned (a contiguous view at an odd storage offset takes
      the two calls), no adjacency gradient (it reads dY); "mma": that pass on the matrix cores, dH_g = A_g^T . (D.dY_g) as an MFMA
      chain, without gate dropout; two passes under gate dropout draw the forward's keep factors again ("two_pass_drop");
    * dX "scaled": the two-unit f16mx8 product (ggcn_linear_scaled) -- the launch that makes dH also leaves max |dH|, from which
      the linear derives a power-of-two scale on the device.  It wants F % 32 == 0 and 16-byte rows, and the scalar launch hands
      max |dH| over for whole wavefronts of columns only.  Otherwise split precisions take bf16x3 (gradients can be far below
      fp16's range), precision "fp32" the exact form, bfloat16 features the bf16 forms."""
    env = os.environ.get
    one_pass = (not need_adj and csr.T <= 32 and F % 4 == 0 and csr.is_binary and csr.rowmask is not None and csr.rowmask.is_cuda
                and not _two_pass_forced() and _aligned16(operands))
    mma = (one_pass and dropout is None and env("GGCN_BACKWARD_SCALAR", "0") != "1"
           and csr.graph_ops is not None and csr.graph_ops_t is not None)
    passes = "mma" if mma else "one_pass" if one_pass else "two_pass" if dropout is None else "two_pass_drop"
    if dtype == torch.bfloat16:
        return passes, ("bf16" if need_x else None), "bf16"
    dw = "bf16x3" if layer.precision in _capi.PACKED else "fp32"
    scaled = (one_pass and need_x and layer.precision == "f16mx8" and K % 4 == 0 and F % 32 == 0 and (mma or F % 256 == 0)
              and env("GGCN_DX_PRECISION", "f16mx8") == "f16mx8")
    return passes, ("scaled" if scaled else dw if need_x else None), dw


# The opt-in one-launch gate / pool backwards, in the order ``backward_launch`` asks them.  replaces: the plan's pass; option: the
# layer's attribute; binary: a 0/1 (True) or real-valued adjacency; wide: graphs of 33..128 nodes (False: <= 32); drop: taken under gate
# dropout, and only there (it then needs B*T*F < 2^32: the hash takes a 32-bit element index); with_adj: taken where an adjacency
# gradient is wanted too (the launch stores dY); operand: how the graph is asked for its A^T operand (None: refused)
_OneLaunchBackward = collections.namedtuple("_OneLaunchBackward", "replaces option binary wide drop with_adj operand")
_ONE_LAUNCH_BACKWARDS = {
    "weighted": _OneLaunchBackward("two_pass", "weighted_backward", False, False, False, True, lambda c: c.graph_ops_weighted_t()),
    "weighted_drop": _OneLaunchBackward("two_pass_drop", "weighted_backward", False, False, True, True, lambda c: c.graph_ops_weighted_t()),
    "wide": _OneLaunchBackward("two_pass", "wide_backward", True, True, False, False, lambda c: c.rowmask_t_wide),
    "weighted_wide": _OneLaunchBackward("two_pass", "weighted_wide_backward", False, True, False, True,
                                        lambda c: c.graph_ops_weighted_wide_t()),
}


def _takes_one_launch_backward(row, layer, csr, B, F, dropout, operands):
    """The one rule of the four ``takes_*_backward`` predicates on a row of the table above, in one order: the option (a layer that predates
    it is a plain namespace without the attribute) -- FIRST, so that a layer without it reads nothing of the graph or the operands --
    the dropout side, the adjacency kind, the node range, F % 4 == 0, every operand 16-byte aligned, ``GGCN_BACKWARD_TWO_PASS`` not
    set, and -- asked once and LAST, so that a refused call builds nothing -- the graph's operand."""
    if not getattr(layer, row.option, False):
        return False
    if (dropout is not None) != row.drop or (row.drop and B * csr.T * F >= 2 ** 32):
        return False
    if bool(csr.is_binary) != row.binary or not (32 < csr.T <= 128 if row.wide else csr.T <= 32):
        return False
    return F % 4 == 0 and _aligned16(operands) and not _two_pass_forced() and row.operand(csr) is not None


def takes_weighted_backward(layer, csr, F, dropout, operands):
    """True when the backward of a layer on a REAL-valued adjacency runs its gate / pool pass AND ``dH = A_w^T . D . dY`` as ONE
    launch on the matrix cores (``ggcn_gate_pool_backward_weighted``) where ``backward_plan`` says "two_pass": the option
    ``layer.weighted_backward`` (``opt.ggcn_weighted_backward`` / ``GGCN_WEIGHTED_BACKWARD=1``; OFF by default), a real-valued
    adjacency of graphs of <= 32 nodes, F % 4 == 0, no gate dropout, every operand 16-byte aligned, ``GGCN_BACKWARD_TWO_PASS``
    not set, and -- asked last, so that a refused call builds nothing -- the graph's A_w^T operand
    (``BatchedCSR.graph_ops_weighted_t``: None when an entry is not finite).  It replaces ``ggcn_gate_pool_backward`` +
    ``BatchedCSR.transposed()`` + ``ggcn_aggregate_t``; dY is written only for an adjacency gradient; the dX / dW forms stay the
    plan's.  float32 and bfloat16 features alike (``out``, dY and dH are float32 in both).
    Measured (``tools/weighted_backward_timing.py``, one MI355X, one process, option off against on, H = 768, f16mx8, us, the
    per-adjacency builders inside): the replaced stage 552 -> 306 (4096 x 32 sparse; 383 with the dY store), 899 -> 337 (dense
    softmax rows; 416), 68 -> 62 (512 x 24); the whole layer backward 1521 -> 1271, 1881 -> 1295, 230 -> 226, with an adjacency
    gradient 2016 -> 1859, 2407 -> 1914, 300 -> 300.  It stays opt-in: dH differs in the last bits.
    The compiler's report: 165 VGPRs, no scratch, three workgroups per CU."""
    return _takes_one_launch_backward(_ONE_LAUNCH_BACKWARDS["weighted"], layer, csr, None, F, dropout, operands)


def takes_weighted_backward_drop(layer, csr, B, F, dropout, operands):
    """``takes_weighted_backward`` under gate dropout: True when the backward of a layer on a REAL-valued adjacency runs
    ``ggcn_gate_pool_backward_weighted_drop`` -- gate / pool pass with the forward's keep factors drawn again AND
    ``dH = A_w^T . D . dY`` in one launch -- where ``backward_plan`` says "two_pass_drop": the option ``layer.weighted_backward``,
    ``dropout`` handed in, B*T*F < 2^32 (the hash takes a 32-bit element index), and then ``takes_weighted_backward``'s
    conditions: a real-valued adjacency of graphs of <= 32 nodes, F % 4 == 0, every operand 16-byte aligned,
    ``GGCN_BACKWARD_TWO_PASS`` not set, and -- asked last, so that a refused call builds nothing -- the graph's A_w^T operand.
    It replaces ``ggcn_gate_pool_backward_drop`` + ``BatchedCSR.transposed()`` + ``ggcn_aggregate_t``; dY is written only for an
    adjacency gradient.  The compiler's report: 219 VGPRs, no scratch, TWO workgroups per CU (under the three-workgroup bound the
    keep factors spill 84 bytes per lane; the form without dropout keeps 165 VGPRs and three workgroups).
    Timings: ``takes_weighted_dropout``."""
    return _takes_one_launch_backward(_ONE_LAUNCH_BACKWARDS["weighted_drop"], layer, csr, B, F, dropout, operands)


def takes_wide_backward(layer, csr, B, F, dropout, operands):
    """True when the backward of a layer on a 0/1 adjacency of graphs of 33..128 nodes runs its gate / pool pass AND
    ``dH = A^T . D . dY`` as ONE launch on the matrix cores (``ggcn_gate_pool_backward_wide``) where ``backward_plan`` says
    "two_pass": the option ``layer.wide_backward`` (``opt.ggcn_wide_backward`` / ``GGCN_WIDE_BACKWARD=1``; OFF by default) --
    looked at FIRST, so that a refused call builds nothing -- no gate dropout (the launch has no form under it: "two_pass_drop"
    stays), a 0/1 adjacency, 32 < T <= 128, F % 4 == 0, every operand 16-byte aligned, ``GGCN_BACKWARD_TWO_PASS`` not set, and --
    asked last -- the graph's transposed row masks (``BatchedCSR.rowmask_t_wide``: None without row masks on the GPU).  It
    replaces ``ggcn_gate_pool_backward`` + ``BatchedCSR.transposed()`` + ``ggcn_aggregate_t``; ``backward_launch`` does not ask
    where an adjacency gradient is wanted (it reads dY from memory); the dX / dW forms stay the plan's.  float32 and bfloat16
    features alike (``out``, dY and dH are float32 in both).  ``B`` is not looked at (no element index without dropout).  It stays
    opt-in: dH differs in the last bits.
    Measured (``tools/wide_backward_timing.py``, one MI355X, one process, each form alone in steady state, H = 768, f16mx8, us,
    option off -> on; the box's calibration is not known, ``bench.py --full`` was not run beside it).  The replaced stage with the
    graph's transposed CSR / masks cached: 512 x 100: 238 -> 133, 1024 x 64: 284 -> 144, 512 x 128: 296 -> 149, 2048 x 40: 340 -> 226, 64 x 100: 78 -> 75;
    built inside every call: 313 -> 138, 351 -> 150, 423 -> 155, 392 -> 233, 95 -> 81; the builders alone: transposed CSR
    58-128, transposed masks 10.  The whole layer backward, cached: 679 -> 549, 773 -> 650, 811 -> 658, 960 -> 854, 188 -> 178.
    No shape lost; WEAK: the small batch (3-5 %).
    The compiler's report: 222 VGPRs, no scratch, 21 KiB of LDS, two workgroups per CU."""
    return _takes_one_launch_backward(_ONE_LAUNCH_BACKWARDS["wide"], layer, csr, B, F, dropout, operands)


def takes_weighted_wide_backward(layer, csr, F, dropout, operands):
    """True when the backward of a layer on a REAL-valued adjacency of graphs of 33..128 nodes runs its gate / pool pass AND
    ``dH = A_w^T . D . dY`` as ONE launch on the matrix cores (``ggcn_gate_pool_backward_weighted_wide``) where ``backward_plan``
    says "two_pass": the option ``layer.weighted_wide_backward`` (``opt.ggcn_weighted_wide_backward`` /
    ``GGCN_WEIGHTED_WIDE_BACKWARD=1``; OFF by default, and separate from ``weighted_backward``) -- looked at FIRST, so that a layer
    without it asks the graph nothing -- no gate dropout (the launch has no form under it: "two_pass_drop" stays), a real-valued
    adjacency, 32 < T <= 128, F % 4 == 0, every operand 16-byte aligned, ``GGCN_BACKWARD_TWO_PASS`` not set, and -- asked last,
    so that a refused call builds nothing -- the graph's A_w^T operand (``BatchedCSR.graph_ops_weighted_wide_t``: None when an
    entry is not finite).  It replaces ``ggcn_gate_pool_backward`` + ``BatchedCSR.transposed()`` + ``ggcn_aggregate_t``; unlike
    "wide" it is taken with an adjacency gradient too: the launch stores dY for ``ggcn_adjacency_grad``.  The dX / dW forms stay
    the plan's.  float32 and bfloat16 features alike (``out``, dY and dH are float32 in both).  It stays opt-in: dH differs in the
    last bits.
    Measured (``tools/weighted_wide_backward_timing.py``, one MI355X, one process, each form alone in steady state, H = 768,
    f16mx8, us, option off -> on, the per-adjacency builders inside every call; sparse / dense softmax rows).  The replaced
    stage: 512 x 100: 324 -> 210 / 1081 -> 236, 1024 x 64: 362 -> 203 / 921 -> 217, 512 x 128: 451 -> 237 / 1664 -> 272; with the dY
    store 239 / 266, 248 / 262, 282 / 314.  The whole layer backward: 758 -> 654 / 1569 -> 688, 879 -> 736 / 1478 -> 757,
    968 -> 753 / 2241 -> 799; with ``d adj`` 1116 -> 1034 / 1957 -> 1091 at 512 x 100.  The builders alone: transposed CSR 73-144,
    the operand 34-38 (sparse), 53-71 (dense).  NEGATIVE: 64 x 100 on a sparse graph LOSES (stage 98 -> 129, backward 214 -> 241);
    on dense rows it wins there too (222 -> 142).
    The compiler's report: 214 VGPRs, no scratch, 19 KiB of LDS, two workgroups per CU."""
    return _takes_one_launch_backward(_ONE_LAUNCH_BACKWARDS["weighted_wide"], layer, csr, None, F, dropout, operands)


def backward_launch(layer, csr, dtype, B, K, F, need_x, need_adj, dropout, operands):
    """``backward_plan`` with its pass replaced by the first opt-in one-launch backward ("weighted", "weighted_drop", "wide",
    "weighted_wide": ``BACKWARD_LAUNCHES``) that replaces that pass, admits the adjacency gradient where one is wanted (the wide
    launch does not: it stores no dY) and whose predicate above holds: asked after the plan and only where it says "two_pass" /
    "two_pass_drop", so the plan's answers stay as pinned."""
    passes, dx, dw = backward_plan(layer, csr, dtype, K, F, need_x, need_adj, dropout, operands)
    for name, row in _ONE_LAUNCH_BACKWARDS.items():
        if row.replaces == passes and (row.with_adj or not need_adj) and _takes_one_launch_backward(row, layer, csr, B, F, dropout, operands):
            return name, dx, dw
    return passes, dx, dw


# ---- the block of two layers (the four predicates are gated_block's public ones) -------------------------------------------------
def bf16_block_on(x, gc1):
    """The opt-in of the bf16 block forms (``GraphConvolution.bf16_block``) on bfloat16 GPU features."""
    return bool(getattr(gc1, "bf16_block", False)) and isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.bfloat16


def _square(gc1, gc2):
    return gc1.out_features == gc2.in_features and gc1.out_features == gc2.out_features


def takes_block_path(x, csr, gc1, gc2):
    """True when the inference block runs as ONE launch: both layers on the one-launch layer path with the
    same arithmetic, and gc1's output width = gc2's (the reference's blocks are square, bert_amir5.py:559-560)."""
    inp = Input.of(x)
    return (csr.T <= 32 and takes_fused(gc1, csr, inp) and takes_fused(gc2, csr, inp) and gc1.precision == gc2.precision
            and _square(gc1, gc2))


def takes_folded_eval_path(x, csr, gc1, gc2):
    """True when an evaluation that needs only ``out`` / ``x`` of graphs of 33..256 nodes runs WITHOUT the W1 product:
    ``Z = D.A.X`` (the aggregation kernel on the features), then ONE one-launch layer on Z with the folded weight
    ``W12 = W1.W2`` and ``mid = W2^T.b1`` added before its aggregation (``ggcn_layer_fused_prebias``):
    ``gc2(gc1(X)) = D.A.(Z.W12 + 1.mid^T) + b2`` (``bert_amir5.py:626,639``: no non-linearity between the layers)."""
    inp = Input.of(x)
    return (32 < csr.T <= 256 and takes_fused(gc1, csr, inp) and takes_fused(gc2, csr, inp) and gc1.precision == gc2.precision
            and gc1.precision in ("f16mx8", "bf16x3") and _square(gc1, gc2) and gc1.in_features == gc1.out_features)


def takes_bf16_block_path(x, csr, gc1, gc2):
    """True when inference on bfloat16 features runs the block as ONE launch (``ggcn_block_fused_bf16``): the option
    ``gc1.bf16_block`` (``opt.ggcn_bf16_block`` / ``GGCN_BF16_BLOCK=1``; off by default), graphs of <= 32 nodes that gc1 would run
    as one bf16 layer launch, gc2 on the one-launch path, split precisions on both layers (all of them mean the bf16 pair form on
    the ``bf16x3`` images) and square widths."""
    return (bf16_block_on(x, gc1) and csr.T <= 32 and takes_bf16_fused(gc1, csr, Input.of(x)) and bool(gc2.fused)
            and gc1.precision in BF16_PRECISIONS and gc2.precision in BF16_PRECISIONS and _square(gc1, gc2))


def takes_bf16_folded_eval_path(x, csr, gc1, gc2):
    """``takes_folded_eval_path`` for bfloat16 features (same option as ``takes_bf16_block_path``): graphs of 33..256 nodes with a
    0/1 adjacency and row masks on the device, gc2 on the float32 one-launch path for its float32 input, square widths.
    ``Z = D.A.X`` by ``ggcn_aggregate_bf16``, then one ``ggcn_layer_fused_prebias`` launch in ``bf16x3``."""
    return (bf16_block_on(x, gc1) and 32 < csr.T <= 256 and bool(csr.is_binary) and csr.rowmask is not None
            and bool(csr.rowmask.is_cuda) and gc1.precision in BF16_PRECISIONS and takes_fused(gc2, csr, Input.of(x, torch.float32))
            and _square(gc1, gc2) and gc1.in_features == gc1.out_features)


def block_path(x, csr, gc1, gc2, want, want_gcn1, one_launch, training):
    """What ``gated_gcn_block`` runs, one of ``BLOCK_PATHS``.  Under autograd "layers" (each layer through its own
    ``forward_gated``).  Inference, in this order: with ``one_launch``, "block" / "bf16_block" (<= 32 nodes, the whole block as one
    launch), then -- nothing of layer 1 wanted (no x1, y1, xy, gcn1) -- "bf16_folded_eval" / "folded_eval" (33..256 nodes, no
    product with W1); no x1, y1, xy wanted: "layers_eval" (gc1 plain, gc2 with its gate and pool); both layers one launch each
    and equal widths: "two_fused" (the regulariser's sums ride in the two launches); else "layers"."""
    if training:
        return "layers"
    layer1 = any(k in want for k in ("x1", "y1", "xy"))   # anything of bert_amir5.py:627-638
    eval_only = not layer1 and not want_gcn1
    for name, takes, allowed in (("block", takes_block_path, True), ("bf16_block", takes_bf16_block_path, True),
                                 ("bf16_folded_eval", takes_bf16_folded_eval_path, eval_only), ("folded_eval", takes_folded_eval_path, eval_only)):
        if one_launch and allowed and takes(x, csr, gc1, gc2):
            return name
    if not layer1:
        return "layers_eval"
    inp = Input.of(x)
    if ((takes_fused(gc1, csr, inp) or takes_bf16_fused(gc1, csr, inp) or takes_bf16_wide(gc1, csr, inp))
            and takes_fused(gc2, csr, Input.of(x, torch.float32)) and gc1.out_features == gc2.out_features):
        return "two_fused"
    return "layers"


def takes_weighted_block_path(x, csr, gc1, gc2):
    """True when the inference block on a REAL-valued adjacency runs as ONE launch (``ggcn_block_fused_weighted``) where
    ``block_path`` says "layers" / "layers_eval": the option ``gc1.weighted_block`` (``opt.ggcn_weighted_block`` /
    ``GGCN_WEIGHTED_BLOCK=1``; OFF by default) -- looked at first, so that a refused call builds nothing -- float32 features on a
    GPU, a real-valued adjacency of graphs of <= 32 nodes, both layers with ``fused`` and the same precision out of "bf16x3" /
    "f16mx8", square widths, ``takes_weighted`` for gc1 on ``x`` and for gc2 on float32 input (so M = D.A_w fits the plane type)
    and -- asked last -- the graph's (D.A_w)^2 operand (``BatchedCSR.graph_ops2_weighted``: None when an entry does not fit the
    plane type or is not finite; one read-back per adjacency and plane type).
    ``gc2(gc1(X)) = M^2.(X.W12) + rowsum(M).mid + b2`` with M = D.A_w: the W1 column tiles apply M with a zero ``mid`` row, the W12
    tiles M^2 with ``mid = W2^T.b1``, both through the hi / lo operand epilogue (one split of ``hidden``, 6 MFMAs).  It replaces two
    ``ggcn_layer_fused_weighted`` launches, the write and re-read of gcn1 and ``ggcn_gate_overlap``; ``want=("out",)`` launches the
    W12 tiles only.  It stays opt-in: its sums differ from the two layer launches' in the last bits (both inside the parity gate).
    Measured (``tools/weighted_block_timing.py``, one MI355X, one process, each form alone in steady state, H = 768, us per call,
    option off / on; "cached" = the graph's operand blocks exist, "built" = the per-adjacency builders and their flag read-backs
    inside every call).  f16mx8, every output: 4096 x 32 sparse cached 691 / 614, built 723 / 686; dense softmax rows cached
    696 / 618, built 753 / 753; 512 x 24 cached 110 / 88, built 151 / 171.  f16mx8, ``want=("out",)``: sparse cached 626 / 293, built
    652 / 374; dense cached 632 / 297, built 684 / 429; 512 x 24 cached 97 / 49, built 133 / 127.  bf16x3, every output: sparse cached
    963 / 856, built 989 / 913; dense cached 965 / 865, built 1022 / 979; 512 x 24 cached 132 / 109, built 170 / 191; ``want=("out",)``:
    sparse cached 893 / 432, built 925 / 488; dense cached 916 / 434, built 943 / 545; 512 x 24 cached 122 / 62, built 157 / 137.
    NEGATIVE: with the builders inside and every output wanted the option does not win on dense rows at 4096 x 32 in f16mx8 (a tie)
    and LOSES on the small batch (171 vs 151, 191 vs 170 us): the second builder and its read-back cost 40-80 us per adjacency
    (DESIGN.md 4.12).
    The compiler's report: ``block_fused_weighted_kernel`` 225-253 VGPRs (f16mx8) / 233-248 (bf16x3) over its twelve forms, no
    scratch, two workgroups per CU; ``graph_operands2_w_kernel`` 58 VGPRs, no scratch, 18 KiB of LDS."""
    if not getattr(gc1, "weighted_block", False):
        return False
    inp = Input.of(x)
    if not (inp.gpu is not None and inp.dtype == torch.float32 and not csr.is_binary and csr.T <= 32):
        return False
    if not (gc1.fused and gc2.fused and gc1.precision == gc2.precision and gc1.precision in WEIGHTED_BLOCK_PRECISIONS and _square(gc1, gc2)):
        return False
    if not (takes_weighted(gc1, csr, inp) and takes_weighted(gc2, csr, Input.of(x, torch.float32))):
        return False
    return csr.graph_ops2_weighted(0 if gc1.precision == "bf16x3" else 1) is not None


def block_launch(x, csr, gc1, gc2, want, want_gcn1, one_launch, training):
    """What ``_gated_gcn_block`` runs, one of ``BLOCK_LAUNCHES``: ``block_path``'s name, replaced by "weighted_block" where that name
    is "layers" / "layers_eval", the call is an inference call (``training`` is False: an ``adj`` that requires grad makes it
    True), ``one_launch`` is set and ``takes_weighted_block_path`` holds -- asked after ``block_path``, whose answers stay as pinned."""
    path = block_path(x, csr, gc1, gc2, want, want_gcn1, one_launch, training)
    if path in ("layers", "layers_eval") and not training and one_launch and takes_weighted_block_path(x, csr, gc1, gc2):
        return "weighted_block"
    return path
