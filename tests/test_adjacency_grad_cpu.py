"""CPU checks of the adjacency gradient (include/ggcn.h ggcn_adjacency_grad; DESIGN.md "Gradient with respect to the adjacency").

The float64 oracle for the new argument: torch autograd of ``backward_ref.gated_layer_ref`` with respect to a float64 ``adj`` leaf
against central finite differences and against the closed form the kernel evaluates,

    G_ij = inv_i (dY_i . H_j),   c_i = inv_i sum_k A_ik G_ik,   dA_ij = G_ij - c_i   for every (i, j),

then the entry itself: declared, bound and exported with the ABI still 14, every refusal returning its code and a message that
names the argument BEFORE any launch (the pointers handed in are never dereferenced), and the predicate that sends a
differentiable ``adj`` to the autograd path.
"""
import ctypes
import re

import pytest
import torch

import ed_gated_gcn_amd as pkg
from ed_gated_gcn_amd import _capi
from ed_gated_gcn_amd.gcn import GraphConvolution
from oracle import backward_ref as br
from oracle.host_support import header as _header, msg as _msg

EINVAL, EUNSUPPORTED = 1, 3
NAME = "ggcn_adjacency_grad"
P = ctypes.c_void_p(1 << 20)   # a non-null, 16-byte aligned address: never dereferenced (the checks come first)
OFF2 = ctypes.c_void_p((1 << 20) + 2)


def closed_form(dy, hidden, adj):
    """dA [B,T,T] from dY, H [B,T,F] and A [B,T,T], in the dtype of the arguments."""
    inv = 1.0 / (adj.sum(2) + 1.0)
    g = inv[:, :, None] * torch.einsum("bif,bjf->bij", dy, hidden)
    c = inv * (adj * g).sum(2)
    return g - c[:, :, None]


def _loss(c, adj64, x64=None):
    """(loss, y) of the backward tests' loss sum(out*R1) + sum(pa*R2) + sum(pb*R3), built on backward_ref's own pieces so that
    y (and with it dY) can be named."""
    y = br.layer_output(c["x"] if x64 is None else x64, adj64, c["w"], c["b"])
    out, pa, pb = br.gated(y, c["sg"]), torch.max(br.gated(y, c["ga"]), 1)[0], torch.max(br.gated(y, c["gb"]), 1)[0]
    return (out * c["r1"]).sum() + (pa * c["r2"]).sum() + (pb * c["r3"]).sum(), y


@pytest.mark.parametrize("graph", ["tree", "directed", "weighted", "len1"])
@pytest.mark.parametrize("T", [3, 5])
def test_oracle_differentiates_through_adj(T, graph):
    """Autograd of gated_layer_ref w.r.t. a float64 adj leaf = central differences = the closed form.

    Bounds: the closed form is the same mathematics in another order, 1e-9 * max(1, max|ref|) (float64 rounding is ~1e-15).
    Central differences with h = 1e-5 carry a truncation term h^2 |f'''| / 6 ~ 1e-10 and a rounding term 2^-52 |loss| / h ~ 1e-10;
    the bound 1e-6 * max(1, max|ref|) is four orders above both and four below a missing term (the entries are O(1e-2..1))."""
    B, K, F = 2, 6, 4
    c = br.case_inputs(B, T, K, F, seed=300 + T, graph=graph)
    # nodes with the same neighbourhood have the same y: an exact tie in a max-pool, where the function has one-sided derivatives
    # only.  Pools whose two largest values are closer than 1e-3 (>> h * slope) get no upstream gradient (backward_ref's rule).
    ma, mb = br.layer_tie_masks(c["x"], c["adj"], c["w"], c["b"], c["ga"], c["gb"], 1e-3)
    c["r2"], c["r3"] = c["r2"] * (~ma), c["r3"] * (~mb)
    if graph == "directed":
        assert br.masked_share(ma, mb) < 0.5     # the pools do take part
    adj = c["adj"].double().requires_grad_()
    out, pa, pb = br.gated_layer_ref(c["x"], adj, c["w"], c["b"], c["sg"], c["ga"], c["gb"])
    ((out * c["r1"]).sum() + (pa * c["r2"]).sum() + (pb * c["r3"]).sum()).backward()
    ref = adj.grad
    scale = max(1.0, float(ref.abs().max()))
    assert float(ref.abs().max()) > 1e-3     # a gradient that vanishes checks nothing
    # the closed form, from dY of the same loss
    adj2 = c["adj"].double().requires_grad_()
    loss, y = _loss(c, adj2)
    dy, via_y = torch.autograd.grad(loss, [y, adj2])
    assert float((via_y - ref).abs().max()) <= 1e-12 * scale
    hidden = c["x"].double() @ c["w"].double()
    got = closed_form(dy, hidden, c["adj"].double())
    assert float((got - ref).abs().max()) <= 1e-9 * scale
    # zero entries receive gradients too: the gradient is dense (three nodes of a tree may leave no zero entry)
    zeros = c["adj"] == 0
    assert bool(zeros.any()) or graph in ("tree", "weighted")
    assert not bool(zeros.any()) or bool((ref[zeros] != 0).any())
    # central finite differences, entry by entry
    h = 1e-5
    base = c["adj"].double()
    fd = torch.zeros_like(base)
    with torch.no_grad():
        for b in range(B):
            for i in range(T):
                for j in range(T):
                    up, dn = base.clone(), base.clone()
                    up[b, i, j] += h
                    dn[b, i, j] -= h
                    fd[b, i, j] = (_loss(c, up)[0] - _loss(c, dn)[0]) / (2 * h)
    assert float((fd - ref).abs().max()) <= 1e-6 * scale


def test_closed_form_in_float32_is_close_to_float64():
    """What the kernel's arithmetic can reach: the same form in float32 against float64 stays far inside the GPU gate (2e-4)."""
    c = br.case_inputs(3, 33, 16, 24, seed=9, graph="weighted")
    g = torch.Generator().manual_seed(4)
    dy = torch.randn(3, 33, 24, generator=g)
    hidden = c["x"] @ c["w"]
    ref = closed_form(dy.double(), hidden.double(), c["adj"].double())
    got = closed_form(dy, hidden, c["adj"])
    assert float((got.double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


def test_symbol_declared_bound_and_exported():
    assert re.search(r"\b%s\s*\(" % NAME, _header())
    assert NAME in _capi.PROTOTYPES
    assert hasattr(ctypes.CDLL(pkg.lib_path()), NAME)
    res, args = _capi.PROTOTYPES[NAME]
    assert res is ctypes.c_int and len(args) == 13
    assert hasattr(pkg.load_library(), NAME)


def test_abi_version_stays_14_on_all_three_sides():
    m = re.search(r"#define\s+GGCN_ABI_VERSION\s+(\d+)", _header())
    assert int(m.group(1)) == 14
    assert _capi.ABI_VERSION == 14
    assert pkg.load_library().ggcn_abi_version() == 14


def _call(lib, dy=P, ldy=64, hidden=P, ldh=64, inv=P, rowptr=P, colidx=P, vals=None, B=4, T=40, F=64, d_adj=P):
    return lib.ggcn_adjacency_grad(dy, ldy, hidden, ldh, inv, rowptr, colidx, vals, B, T, F, d_adj, None)


def test_refuses_bad_arguments_before_any_launch():
    lib = pkg.load_library()
    for arg in ("dy", "hidden", "inv", "rowptr", "colidx", "d_adj"):
        m = _msg(lib, _call(lib, **{arg: None}), EINVAL)
        assert {"dy": "dY"}.get(arg, arg) + " is NULL" in m, m
    assert "ldy=63 < F=64" in _msg(lib, _call(lib, ldy=63), EINVAL)
    assert "ldh=63 < F=64" in _msg(lib, _call(lib, ldh=63), EINVAL)
    for arg in ("dy", "hidden", "inv", "rowptr", "colidx", "vals", "d_adj"):
        m = _msg(lib, _call(lib, **{arg: OFF2}), EINVAL)
        assert {"dy": "dY"}.get(arg, arg) + " not 4-byte aligned" in m, m
    assert "B=-1" in _msg(lib, _call(lib, B=-1), EINVAL)
    assert "T=-3" in _msg(lib, _call(lib, T=-3), EINVAL)
    assert "T=0" in _msg(lib, _call(lib, T=0), EINVAL)
    assert "F=-2" in _msg(lib, _call(lib, F=-2, ldy=0, ldh=0), EINVAL)
    assert "F=0" in _msg(lib, _call(lib, F=0), EINVAL)
    m = _msg(lib, _call(lib, T=513), EUNSUPPORTED)
    assert "T=513" in m and "512" in m
    # a bad argument is named even where the length is out of range too, and B = 0 launches nothing
    assert "ldy" in _msg(lib, _call(lib, T=513, ldy=1), EINVAL)
    assert _call(lib, B=0) == 0
    assert _call(lib, B=0, T=512, vals=P) == 0


def test_needs_grad_sees_a_differentiable_adjacency():
    m = GraphConvolution(8, 8)
    m.weight.requires_grad_(False)
    m.bias.requires_grad_(False)
    x = torch.zeros(2, 5, 8)
    adj = torch.ones(2, 5, 5)
    assert m._needs_grad(x) is False and m._needs_grad(x, adj=adj) is False
    soft = torch.rand(2, 5, 5, requires_grad=True)
    assert m._needs_grad(x, adj=soft) is True
    assert m._needs_grad(x, None, None, adj=soft.double()) is True      # a non-leaf that requires grad
    assert m._differentiable_adj(soft) is soft
    with torch.no_grad():
        assert m._needs_grad(x, adj=soft) is False and m._differentiable_adj(soft) is None
    assert m._needs_grad(x, adj=soft.detach()) is False
    assert m._needs_grad(x, adj=torch.ones(2, 5, 5, dtype=torch.int32)) is False
    assert m._needs_grad(x, adj=object()) is False                      # a BatchedCSR has no tensor to differentiate
    m.weight.requires_grad_(True)
    assert m._needs_grad(x, adj=adj) is True
