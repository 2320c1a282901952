"""Host side of the differentiable scores / kl head (``ggcn_scores_head_backward``, ``ggcn_scores_head_dweight``;
include/ggcn.h): the float64 statement of its formulas against float64 autograd through the reference's literal ops, the new
entries on all three sides of the ABI (which stays 14), their refusals (every check comes before a launch: the pointers handed
in are never dereferenced, so no GPU is needed) and the classifier's opt-in ``head_backward``."""
import ctypes
import os
import types

import pytest
import torch

import ed_gated_gcn_amd as pkg
from ed_gated_gcn_amd import _capi
from oracle.host_support import header as _header, msg as _msg

import head_backward_ref as hb

EINVAL, EUNSUPPORTED = 1, 3
P = ctypes.c_void_p(1 << 20)   # non-null, 16-byte aligned, never dereferenced
BACKWARD, WORKSPACE, DWEIGHT = "ggcn_scores_head_backward", "ggcn_scores_head_dweight_workspace_bytes", "ggcn_scores_head_dweight"


# ---------------------------------------------------------------- the formulas
def _same(got, ref, what):
    """1e-12 relative to max|ref|; a gradient that is identically zero (float64 autograd leaves ~1e-17 of noise there) must be
    below 1e-13 outright."""
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    if scale < 1e-13:
        assert float(got.abs().max()) < 1e-13, "%s: %.3g where the reference is zero" % (what, float(got.abs().max()))
    else:
        assert err <= 1e-12 * scale, "%s: %.3g vs scale %.3g" % (what, err, scale)


@pytest.mark.parametrize("which", hb.LOSSES)
@pytest.mark.parametrize("shape", hb.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_statement_equals_float64_autograd_through_the_literal_ops(shape, which):
    t = hb.make_inputs(shape, seed=sum(shape))
    ref = hb.autograd64(t, which)
    g_s, g_k = hb.incoming(t["r"], which)
    st = hb.statement64(t["x"], t["aspect"], t["logits"], t["weight"], t["bias"], t["dist"], g_s, g_k)
    _same(st["scores"], ref["scores"], "scores")
    _same(st["kl"], ref["kl"], "kl")
    for name in ("x", "aspect", "logits", "weight", "bias"):
        assert st["d" + name].shape == ref["d" + name].shape, name
        _same(st["d" + name], ref["d" + name], "d " + name)
    # the workspace the kernel hands to the weight product, and the kl term's share of dc0 (identically zero)
    _same(t["logits"].double().t() @ st["G"], ref["dweight"], "logits^T . G")
    if which == "kl":
        assert float(st["dc0"].abs().max()) < 1e-13


def test_literal_ops_in_float32_are_the_classifiers_lines():
    t = hb.make_inputs((3, 7, 64, 5), seed=1)
    fc = torch.nn.Linear(128, 5)
    with torch.no_grad():
        fc.weight.copy_(t["weight"])
        fc.bias.copy_(t["bias"])
        x, aspect, logits, T = t["x"], t["aspect"], t["logits"], 7
        output_w = fc(torch.cat([x, aspect[:, None, :].expand(-1, T, -1)], dim=2))                     # classifier.py, :645
        scores = (logits[:, None, :] * output_w).sum(2)                                                # :646
        kl = (torch.softmax(scores, 1) * torch.softmax(t["dist"].float(), 1)).sum(1).mean()            # :648
        got = hb.literal(x, aspect, logits, t["weight"], t["bias"], t["dist"])
    assert torch.equal(got[0], scores) and torch.equal(got[1], kl)


# ---------------------------------------------------------------- the ABI
def test_declared_bound_exported_and_abi_stays_14():
    lib = ctypes.CDLL(pkg.lib_path())
    header = _header()
    for name in (BACKWARD, WORKSPACE, DWEIGHT):
        assert name + "(" in header and name in _capi.PROTOTYPES and hasattr(lib, name), name
    raw = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ggcn.h")).read()
    assert "#define GGCN_ABI_VERSION 14" in raw and _capi.ABI_VERSION == 14 and pkg.load_library().ggcn_abi_version() == 14
    proto = {k: v[1] for k, v in _capi.PROTOTYPES.items()}
    fwd = proto["ggcn_scores_head"]
    vp, i64, i32 = _capi.c_vp, _capi.c_i64, _capi.c_i32
    # the forward's operands, then what it saved, the incoming gradients, the sizes, and the outputs with their strides
    assert proto[BACKWARD] == fwd[:11] + [vp, i64, vp, vp, i64, vp] + [i32] * 4 + [vp, i64] * 4 + [vp, vp]
    assert _capi.PROTOTYPES[WORKSPACE] == (_capi.c_sz, [i32, i32, i32])
    assert len(proto[DWEIGHT]) == 13


def test_workspace_is_one_slab_per_128_sentences():
    lib = pkg.load_library()
    per = 34 * (2 * 768 + 1) * 4
    assert lib.ggcn_scores_head_dweight_workspace_bytes(1, 768, 34) == per
    assert lib.ggcn_scores_head_dweight_workspace_bytes(128, 768, 34) == per
    assert lib.ggcn_scores_head_dweight_workspace_bytes(129, 768, 34) == 2 * per
    assert lib.ggcn_scores_head_dweight_workspace_bytes(4096, 768, 34) == 32 * per
    assert lib.ggcn_scores_head_dweight_workspace_bytes(0, 768, 34) > 0


def _backward(lib, **kw):
    a = dict(x=P, ldx=64, aspect=P, lda=64, logits=P, ldl=5, w=P, ldw=128, fb=P, dist=P, ldd=7, scores=P, lds=7, part=P, gs=P, ldgs=7,
             gk=P, B=3, T=7, H=64, C=5, dx=P, lddx=64, da=P, ldda=64, dlg=P, lddl=5, G=P, ldg=128, dc0=P)
    a.update(kw)
    return lib.ggcn_scores_head_backward(a["x"], a["ldx"], a["aspect"], a["lda"], a["logits"], a["ldl"], a["w"], a["ldw"], a["fb"],
                                         a["dist"], a["ldd"], a["scores"], a["lds"], a["part"], a["gs"], a["ldgs"], a["gk"], a["B"],
                                         a["T"], a["H"], a["C"], a["dx"], a["lddx"], a["da"], a["ldda"], a["dlg"], a["lddl"], a["G"],
                                         a["ldg"], a["dc0"], None)


@pytest.mark.parametrize("kw, code, word", [
    (dict(x=None), EINVAL, "null"), (dict(aspect=None), EINVAL, "null"), (dict(logits=None), EINVAL, "null"), (dict(w=None), EINVAL, "null"),
    (dict(dist=None), EINVAL, "gradient of kl"), (dict(scores=None), EINVAL, "gradient of kl"), (dict(part=None), EINVAL, "gradient of kl"),
    (dict(G=None), EINVAL, "go together"), (dict(dc0=None), EINVAL, "go together"),
    (dict(B=0), EINVAL, "B=0"), (dict(T=0), EINVAL, "T=0"), (dict(H=0), EINVAL, "H=0"), (dict(C=0), EINVAL, "C=0"),
    (dict(ldx=63), EINVAL, "leading"), (dict(lda=63), EINVAL, "leading"), (dict(ldl=4), EINVAL, "leading"), (dict(ldw=127), EINVAL, "leading"),
    (dict(ldd=6), EINVAL, "leading"), (dict(lds=6), EINVAL, "leading"), (dict(ldgs=6), EINVAL, "leading"), (dict(lddx=63), EINVAL, "leading"),
    (dict(ldda=63), EINVAL, "leading"), (dict(lddl=4), EINVAL, "leading"), (dict(ldg=127), EINVAL, "leading"),
    (dict(H=3280, ldx=3280, lda=3280, ldw=6560, lddx=3280, ldda=3280, ldg=6560), EUNSUPPORTED, "64 KiB"),
])
def test_backward_refuses_before_it_launches(kw, code, word):
    lib = pkg.load_library()
    assert word in _msg(lib, _backward(lib, **kw), code, BACKWARD)


@pytest.mark.parametrize("kw, code, word", [
    (dict(lg=None), EINVAL, "null"), (dict(G=None), EINVAL, "null"), (dict(dc0=None), EINVAL, "null"), (dict(dw=None), EINVAL, "null"),
    (dict(ws=None), EINVAL, "null"), (dict(B=0), EINVAL, "B=0"), (dict(ldl=4), EINVAL, "leading"), (dict(ldg=127), EINVAL, "leading"),
    (dict(lddw=127), EINVAL, "leading"), (dict(B=65536 * 128), EUNSUPPORTED, "sentences"),
])
def test_dweight_refuses_before_it_launches(kw, code, word):
    lib = pkg.load_library()
    a = dict(lg=P, ldl=5, G=P, ldg=128, dc0=P, B=3, H=64, C=5, dw=P, lddw=128, db=P, ws=P)
    a.update(kw)
    rc = lib.ggcn_scores_head_dweight(a["lg"], a["ldl"], a["G"], a["ldg"], a["dc0"], a["B"], a["H"], a["C"], a["dw"], a["lddw"], a["db"],
                                      a["ws"], None)
    assert word in _msg(lib, rc, code, DWEIGHT)


# ---------------------------------------------------------------- the classifier's option
def _classifier(monkeypatch, cls=None, **opt):
    o = types.SimpleNamespace(dropout=0.0, polarities_dim=5, **opt)
    return (cls or pkg.GatedGCNEventDetector)(torch.nn.Identity(), o)


def test_option_is_off_by_default_and_read_from_opt_and_environment(monkeypatch):
    monkeypatch.delenv("GGCN_HEAD_BACKWARD", raising=False)
    assert _classifier(monkeypatch).head_backward is False
    assert _classifier(monkeypatch, ggcn_head_backward=True).head_backward is True
    assert _classifier(monkeypatch, ggcn_head_backward=False).head_backward is False
    for cls in (pkg.GatedGCNEventDetector54, pkg.GCNEventDetectorNoGate):
        assert _classifier(monkeypatch, cls).head_backward is False and _classifier(monkeypatch, cls, ggcn_head_backward=True).head_backward is True
    monkeypatch.setenv("GGCN_HEAD_BACKWARD", "1")
    assert _classifier(monkeypatch).head_backward is True
    monkeypatch.setenv("GGCN_HEAD_BACKWARD", "0")
    assert _classifier(monkeypatch).head_backward is False


def test_scores_and_kl_still_refuses_cpu_tensors():
    t = hb.make_inputs((3, 7, 64, 5), seed=2)
    fc = torch.nn.Linear(128, 5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pkg.heads.scores_and_kl(t["x"].requires_grad_(), t["aspect"], t["logits"], fc, t["dist"])
