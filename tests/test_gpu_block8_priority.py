"""The priority bit of the eight-wavefront block kernel (run with ``-m gpu`` on an MI355X).

``ggcn_block_fused`` launches ``block_fused8_kernel`` (``fused_block8.hip``) with ``kBlock8Prio``: the W12 group of every workgroup
runs at ``s_setprio 1``.  Issue priority changes which wavefront of a SIMD goes first, never what it computes, so every output
must stay the bits of the four-wavefront kernel (``GGCN_BLOCK_FORM=4``), and the lab entry ``ggcn_lab_block_fused8`` must give the
same bits with ``GGCN_LAB_BLOCK8_PRIO`` on and off -- at the smallest shape the product hands to this kernel, 1024 x 32 x 64 x 768
(three whole rounds of one workgroup per CU; ``tests/test_gpu_weighted_block.py`` names the same shape), with mixed-sign gates
(the ``vmin`` branch of the pools), a graph with an isolated node and a complete graph; a 64-graph slice must match the float64 block
at the project's bound, 1e-4 * max(1, max |ref|).  The ragged instantiations get the bit too: 1022 graphs (a ragged last row
block), T = 31, and 2048 x 31 (``FULLT = false`` at six rounds) against the four-wavefront kernel.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_dense  # noqa: E402  (tests may use the oracle)
from oracle.gpu_support import dev, make_layer, pkg  # noqa: E402,F401

TOL = 1e-4
K, F = 64, 768
OUTS = ("xo", "x1", "y1", "out", "part")


def _env(**kv):
    class _Env:
        def __enter__(self):
            for k, v in kv.items():
                os.environ[k] = v

        def __exit__(self, *exc):
            for k in kv:
                os.environ.pop(k, None)
    return _Env()


class _Case:
    """One seeded block: mixed-sign gates (the vmin branch of the pools), graph 0 with an isolated node, graph 1 complete."""

    def __init__(self, pkg, dev, B, T):
        from ed_gated_gcn_amd import _capi, synth
        from ed_gated_gcn_amd.gated_block import _block_operands
        self.pkg, self.dev, self.B, self.T = pkg, dev, B, T
        self.lib = pkg.load_library()
        rng = np.random.default_rng(1000 * B + T)
        adj = synth.dependency_batch(B, T, min(4.0, T), seed=5, lengths=rng.integers(1, T + 1, size=B))
        adj[0] = synth.dependency_batch(1, T, min(4.0, T), seed=6)[0]
        adj[0, T // 2, :] = 0
        adj[0, :, T // 2] = 0                      # node T/2 of graph 0: no edge, not even the self loop
        adj[1] = 1                                 # graph 1: every node sees every node
        self.adj = adj
        gen = torch.Generator(device=dev).manual_seed(B + T)
        self.x = torch.randn(B, T, K, device=dev, generator=gen)
        self.g1 = torch.rand(B, F, device=dev, generator=gen) * 2 - 1
        self.g2 = torch.rand(B, F, device=dev, generator=gen) * 2 - 1
        assert bool((self.g1 < 0).any()) and bool((self.g2 < 0).any()) and bool((self.g1 > 0).any())
        (w1, b1), (w2, b2) = synth.layer_params(K, F, seed=1), synth.layer_params(F, F, seed=2)
        self.params = [w1, b1, w2, b2]
        self.l1 = make_layer(pkg, dev, w1, b1, precision="f16mx8").eval()
        self.l2 = make_layer(pkg, dev, w2, b2, precision="f16mx8").eval()
        self.csr = pkg.BatchedCSR.from_dense(torch.from_numpy(adj).to(dev))
        self.st = _capi.stream_of(dev)
        self.pack1, self.pack12, self.mid = _block_operands(self.l1, self.l2, self.lib, self.st, precision="f16mx8")
        self.bb1, self.bb2 = self.l1.bias.detach(), self.l2.bias.detach()
        self.ref4 = self.product(form4=True)       # the four-wavefront kernel: computed once, never written again

    def _bufs(self):
        e = lambda *s: torch.full(s, float("nan"), device=self.dev)   # noqa: E731
        return dict(xo=e(self.B * self.T, F), x1=e(self.B, F), y1=e(self.B, F), out=e(self.B, F), part=e(self.B, F // 64))

    def product(self, form4=False):
        """ggcn_block_fused through the C ABI (the regulariser's partials are an output there) + xy through the package."""
        from ed_gated_gcn_amd import _capi
        P, r = _capi.ptr, self._bufs()
        with _env(**({"GGCN_BLOCK_FORM": "4"} if form4 else {})):
            _capi.check(self.lib.ggcn_block_fused(P(self.x), K, P(self.pack1), P(self.pack12), P(self.csr.graph_ops), P(self.csr.graph_ops2(1)),
                                                  P(self.bb1), P(self.mid), P(self.bb2), self.B, self.T, K, F, P(self.g1), P(self.g2), None, F,
                                                  P(r["xo"]), F, P(r["x1"]), P(r["y1"]), P(r["out"]), P(r["part"]), _capi.PREC["f16mx8"],
                                                  self.st), "ggcn_block_fused")
            with torch.no_grad():
                r["xy"] = self.pkg.gated_gcn_block(self.x, self.csr, self.g1, self.g2, self.l1, self.l2)["xy"]
        torch.cuda.synchronize()
        return r

    def lab(self, **switches):
        """ggcn_lab_block_fused8 on the product's XCD map with the given GGCN_LAB_BLOCK8_* switches."""
        from ed_gated_gcn_amd import _capi
        P, r = _capi.ptr, self._bufs()
        with _env(GGCN_LAB_BLOCK8_ROWMAJOR="1", **{"GGCN_LAB_BLOCK8_" + k: "1" for k in switches}):
            _capi.check(self.lib.ggcn_lab_block_fused8(P(self.x), K, P(self.pack1), P(self.pack12), P(self.csr.graph_ops), P(self.csr.graph_ops2(1)),
                                                       P(self.bb1), P(self.mid), P(self.bb2), self.B, self.T, K, F, P(self.g1), P(self.g2),
                                                       P(r["xo"]), F, P(r["x1"]), P(r["y1"]), P(r["out"]), P(r["part"]), None, self.st),
                        "ggcn_lab_block_fused8")
        torch.cuda.synchronize()
        return r

    def same_bits(self, got, ref, what):
        for k in OUTS + (("xy",) if "xy" in got else ()):
            a, b = got[k], ref[k]
            assert not bool(torch.isnan(a).any()), "%s/%s: an element was not written" % (what, k)
            assert torch.equal(a, b), "%s: %s differs" % (what, k)


@pytest.fixture(scope="module")
def whole(pkg, dev):
    return _Case(pkg, dev, 1024, 32)


def test_block_with_the_priority_bit_is_the_four_wavefront_kernels_bits(whole):
    """1024 x 32 x 64 x 768 takes form 8; x, x1, y1, out, the xy partials and xy are form 4's bits."""
    assert whole.lib.ggcn_block_fused_form(1024, 32, K, F) == 8
    whole.same_bits(whole.product(), whole.ref4, "form 8")


def test_block_with_the_priority_bit_slice_vs_float64(whole):
    """Graphs 0..63 (the isolated node and the complete graph among them) against the float64 block."""
    got = whole.product()
    sl = slice(0, 64)
    p64 = [torch.from_numpy(np.asarray(a, dtype=np.float64)) for a in whole.params]
    ref = ref_dense.gated_block(whole.x[sl].cpu().double(), torch.from_numpy(whole.adj[sl]), whole.g1[sl].cpu().double(),
                                whole.g2[sl].cpu().double(), *p64, dtype=torch.float64)
    T = whole.T
    for k, kr in (("x1", "x1"), ("y1", "y1"), ("xo", "x"), ("out", "out")):
        g = got[k][:64 * T].reshape(64, T, F) if k == "xo" else got[k][sl]
        err, top = float((g.cpu().double() - ref[kr]).abs().max()), float(ref[kr].abs().max())
        print("%s: max|diff| %.3g, bound %.3g" % (k, err, TOL * max(1.0, top)))
        assert err <= TOL * max(1.0, top), "%s: max|diff| %.3g > %.1g * max(1, %.3g)" % (k, err, TOL, top)


def test_lab_priority_switch_changes_no_bit(whole):
    """ggcn_lab_block_fused8 with the priority bit off and on: identical bits, and form 4's."""
    plain = whole.lab()
    whole.same_bits(plain, whole.ref4, "lab entry")
    whole.same_bits(whole.lab(PRIO=True), plain, "GGCN_LAB_BLOCK8_PRIO")


@pytest.mark.parametrize("B,T,form", [(1022, 32, None), (1024, 31, None), (2048, 31, 8)], ids=["ragged-1022", "T31", "2048xT31-form8"])
def test_ragged_shapes_with_the_priority_bit(pkg, dev, B, T, form):
    """A ragged last row block, T = 31, and 2048 x 31 x 64 x 768 on the FULLT = false eight-wavefront instantiations: every
    output is form 4's bits."""
    lib = pkg.load_library()
    if form is not None:
        assert lib.ggcn_block_fused_form(B, T, K, F) == form
    c = _Case(pkg, dev, B, T)
    c.same_bits(c.product(), c.ref4, "%d x %d" % (B, T))
