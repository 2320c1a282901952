"""Host side of the differentiable gate MLPs (``ggcn_gate_mlp_save``, ``ggcn_gate_mlp_backward``; include/ggcn.h): the float64
statement of their formulas against float64 autograd through the ``nn.Sequential`` ops, the new entries on all three sides of the
ABI, their refusals with the exact ``ggcn_last_error`` text (every check comes before a launch: the pointers handed in are never
dereferenced, so no GPU is needed) and the classifier's opt-in ``gate_backward``."""
import ctypes
import types

import pytest
import torch

import ed_gated_gcn_amd as pkg
from ed_gated_gcn_amd import _capi
from oracle.host_support import header as _header, msg as _msg

import gate_mlp_ref as gm

EINVAL, EUNSUPPORTED = 1, 3
P = ctypes.c_void_p(1 << 20)   # non-null, 16-byte aligned, never dereferenced
SAVE, BACKWARD = "ggcn_gate_mlp_save", "ggcn_gate_mlp_backward"
ids = lambda s: "x".join(map(str, s))        # noqa: E731


# ---------------------------------------------------------------- the formulas
def _same(got, ref, what):
    """1e-12 relative to max|ref|; a gradient that is identically zero must be below 1e-13 outright."""
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    if scale < 1e-13:
        assert float(got.abs().max()) < 1e-13, "%s: %.3g where the reference is zero" % (what, float(got.abs().max()))
    else:
        assert err <= 1e-12 * scale, "%s: %.3g vs scale %.3g" % (what, err, scale)


@pytest.mark.parametrize("which", gm.LOSSES)
@pytest.mark.parametrize("shape", gm.SHAPES, ids=ids)
def test_statement_equals_float64_autograd_through_the_sequential_ops(shape, which):
    t = gm.make_inputs(shape, seed=sum(shape))
    ref = gm.autograd64(t, which)
    st = gm.statement64(t, *gm.incoming(t["r1"], t["r2"], which))
    _same(st["g1"], ref["g1"], "g1")
    _same(st["g2"], ref["g2"], "g2")
    for name in gm.NAMES:
        assert st["d" + name].shape == ref["d" + name].shape, name
        _same(st["d" + name], ref["d" + name], "d " + name)
    # Z is what the library's products are run on: [dz1_A | dz1_B]^T . s, dz2^T . h is inside statement64; the column sums
    B, H = shape
    Z = st["Z"]
    assert Z.shape == (B, 5 * H)
    _same(Z[:, :2 * H].t() @ Z[:, 4 * H:], torch.cat([ref["dw1_a"], ref["dw1_b"]]), "[dz1_A | dz1_B]^T . s")
    _same(Z[:, :4 * H].sum(0), torch.cat([ref["db1_a"], ref["db1_b"], ref["db2_a"], ref["db2_b"]]), "column sums of Z")


def test_literal_ops_in_float32_are_the_sequential():
    t = gm.make_inputs((3, 64), seed=1)
    seq = torch.nn.Sequential(torch.nn.Sigmoid(), torch.nn.Linear(64, 64), torch.nn.Sigmoid(), torch.nn.Linear(64, 64), torch.nn.Sigmoid())
    with torch.no_grad():
        for lin, w, b in ((seq[1], "w1_a", "b1_a"), (seq[3], "w2_a", "b2_a")):
            lin.weight.copy_(t[w])
            lin.bias.copy_(t[b])
        assert torch.equal(seq(t["aspect"]), gm.literal(t["aspect"], t["w1_a"], t["b1_a"], t["w2_a"], t["b2_a"]))


# ---------------------------------------------------------------- the ABI
def test_declared_bound_exported_and_without_a_float_argument():
    lib = ctypes.CDLL(pkg.lib_path())
    header = _header()
    for name in (SAVE, BACKWARD):
        assert "int %s(" % name in header and name in _capi.PROTOTYPES and hasattr(lib, name), name
        res, args = _capi.PROTOTYPES[name]
        assert res is _capi.c_i32 and ctypes.c_float not in args and ctypes.c_double not in args, name
        decl = header[header.index("int %s(" % name):]
        decl = decl[:decl.index(";")]
        assert "float " not in decl.replace("float *", ""), "%s takes a float by value" % name
        assert decl.count(",") + 1 == len(args), name
    assert _capi.ABI_VERSION == 14 and pkg.load_library().ggcn_abi_version() == 14
    vp, i64, i32 = _capi.c_vp, _capi.c_i64, _capi.c_i32
    plain = _capi.PROTOTYPES["ggcn_gate_mlp"][1]
    assert _capi.PROTOTYPES[SAVE][1] == plain[:-1] + [vp, vp] + plain[-1:]          # ggcn_gate_mlp's, then hid_a, hid_b, the stream
    assert _capi.PROTOTYPES[BACKWARD][1] == [vp, i64, i32, i32] + [vp] * 10 + [vp, i64, vp, i64, vp]


# ---------------------------------------------------------------- the refusals
def _save(lib, entry=SAVE, **kw):
    a = dict(aspect=P, lda=64, B=3, H=64, w1a=P, b1a=P, w2a=P, b2a=P, ga=P, w1b=P, b1b=P, w2b=P, b2b=P, gb=P, ha=P, hb=P)
    a.update(kw)
    args = [a[k] for k in ("aspect", "lda", "B", "H", "w1a", "b1a", "w2a", "b2a", "ga", "w1b", "b1b", "w2b", "b2b", "gb")]
    if entry == SAVE:
        args += [a["ha"], a["hb"]]
    return getattr(lib, entry)(*args, None)


SECOND = "the second gate needs both of its weights and its output (or none)"
SAVE_REFUSALS = [
    (dict(aspect=None), EINVAL, "null pointer"), (dict(w1a=None), EINVAL, "null pointer"), (dict(w2a=None), EINVAL, "null pointer"),
    (dict(ga=None), EINVAL, "null pointer"),
    (dict(w1b=None), EINVAL, SECOND), (dict(w2b=None), EINVAL, SECOND), (dict(gb=None), EINVAL, SECOND),
    (dict(B=0), EINVAL, "B=0 H=64 lda=64"), (dict(H=0), EINVAL, "B=3 H=0 lda=64"), (dict(lda=63), EINVAL, "B=3 H=64 lda=63"),
    (dict(H=1025, lda=1025), EUNSUPPORTED, "H=1025 needs more than 64 KiB of LDS"),
    (dict(H=4096, lda=4096), EUNSUPPORTED, "H=4096 needs more than 64 KiB of LDS"),
]


@pytest.mark.parametrize("kw, code, text", SAVE_REFUSALS + [
    (dict(ha=None), EINVAL, "null pointer"), (dict(hb=None), EINVAL, "hid_b goes with the second gate"),
    (dict(w1b=None, w2b=None, gb=None), EINVAL, "hid_b goes with the second gate"),
])
def test_save_refuses_before_it_launches(kw, code, text):
    lib = pkg.load_library()
    assert _msg(lib, _save(lib, **kw), code, SAVE) == "%s: %s" % (SAVE, text)


@pytest.mark.parametrize("kw, code, text", SAVE_REFUSALS)
def test_the_plain_forward_keeps_its_refusals(kw, code, text):
    lib = pkg.load_library()
    assert _msg(lib, _save(lib, entry="ggcn_gate_mlp", **kw), code, "ggcn_gate_mlp") == "ggcn_gate_mlp: %s" % text


def _backward(lib, **kw):
    a = dict(aspect=P, lda=64, B=3, H=64, w1a=P, w2a=P, ha=P, ga=P, dga=P, w1b=P, w2b=P, hb=P, gb=P, dgb=P, da=P, ldda=64, Z=P, ldz=320)
    a.update(kw)
    return lib.ggcn_gate_mlp_backward(*[a[k] for k in ("aspect", "lda", "B", "H", "w1a", "w2a", "ha", "ga", "dga", "w1b", "w2b", "hb", "gb",
                                                       "dgb", "da", "ldda", "Z", "ldz")], None)


NEEDS = "a gate with a gradient needs its weights, hid and gate"
LEADING = "leading dimension too small"


@pytest.mark.parametrize("kw, code, text", [
    (dict(aspect=None), EINVAL, "null pointer"),
    (dict(dga=None, dgb=None), EINVAL, "no incoming gradient (both d_gate are NULL)"),
    (dict(da=None, Z=None), EINVAL, "nothing to compute (d_aspect and Z are NULL)"),
    (dict(w1a=None), EINVAL, NEEDS), (dict(w2a=None), EINVAL, NEEDS), (dict(ha=None), EINVAL, NEEDS), (dict(ga=None), EINVAL, NEEDS),
    (dict(w1b=None), EINVAL, NEEDS), (dict(w2b=None), EINVAL, NEEDS), (dict(hb=None), EINVAL, NEEDS), (dict(gb=None), EINVAL, NEEDS),
    (dict(B=0), EINVAL, "B=0 H=64"), (dict(H=0), EINVAL, "B=3 H=0"),
    (dict(lda=63), EINVAL, LEADING), (dict(ldda=63), EINVAL, LEADING), (dict(ldz=319), EINVAL, LEADING),
    (dict(H=30, lda=30, ldda=30, ldz=159), EINVAL, LEADING),                       # Hp = 32: five groups need 160 columns
    (dict(H=1025, lda=1025, ldda=1025, ldz=5140), EUNSUPPORTED, "H=1025 needs more than 64 KiB of LDS"),
    (dict(H=4096, lda=4096, ldda=4096, ldz=20480), EUNSUPPORTED, "H=4096 needs more than 64 KiB of LDS"),
])
def test_backward_refuses_before_it_launches(kw, code, text):
    lib = pkg.load_library()
    assert _msg(lib, _backward(lib, **kw), code, BACKWARD) == "%s: %s" % (BACKWARD, text)


# ---------------------------------------------------------------- the classifier's option
def _classifier(cls=None, **opt):
    o = types.SimpleNamespace(dropout=0.0, polarities_dim=5, **opt)
    return (cls or pkg.GatedGCNEventDetector)(torch.nn.Identity(), o)


@pytest.mark.parametrize("cls_name", ["GatedGCNEventDetector", "GatedGCNEventDetector54", "GCNEventDetectorNoGate"])
def test_option_is_off_by_default_and_read_from_opt_and_environment(monkeypatch, cls_name):
    cls = getattr(pkg, cls_name)
    monkeypatch.delenv("GGCN_GATE_BACKWARD", raising=False)
    monkeypatch.delenv("GGCN_HEAD_BACKWARD", raising=False)
    assert _classifier(cls).gate_backward is False
    assert _classifier(cls, ggcn_gate_backward=True).gate_backward is True
    assert _classifier(cls, ggcn_gate_backward=False).gate_backward is False
    assert _classifier(cls, ggcn_gate_backward=True).head_backward is False, "the two options are independent"
    assert _classifier(cls, ggcn_head_backward=True).gate_backward is False
    monkeypatch.setenv("GGCN_GATE_BACKWARD", "1")
    assert _classifier(cls).gate_backward is True and _classifier(cls).head_backward is False
    monkeypatch.setenv("GGCN_GATE_BACKWARD", "0")
    assert _classifier(cls).gate_backward is False


def test_gate_mlps_still_refuses_cpu_tensors():
    t = gm.make_inputs((3, 64), seed=2)
    seq = lambda: torch.nn.Sequential(torch.nn.Sigmoid(), torch.nn.Linear(64, 64), torch.nn.Sigmoid(), torch.nn.Linear(64, 64),   # noqa: E731
                                      torch.nn.Sigmoid())
    with pytest.raises(RuntimeError, match="no CPU path"):
        pkg.gate_mlps(t["aspect"].requires_grad_(), seq(), seq())
