"""What the four autograd Functions hand to the library's small products -- ``ggcn_weight_pack``, ``ggcn_linear`` on an image,
``ggcn_dweight`` / ``ggcn_dweight_bf16``, ``ggcn_colsum``, ``ggcn_transpose`` -- argument by argument over one training step each,
and when the operand caches of ``hostops.cached`` launch again.

A recorder (``call_log`` of oracle/gpu_support.py) logs ``(name, arguments)``, pointers as integers (NULL: None).  The expected lists
are written out from the prototypes of ``include/ggcn.h``, not taken from the helpers.  An integer or None is compared by value and
type; a tensor of the test by its ``data_ptr()``; a string names a buffer the Function made itself (``(name, byte offset)``: a
place inside it): it must be non-NULL and 16-byte aligned -- every workspace among them -- and the same wherever the name
comes again.  Shapes are those of ``tools/host_digest.py``, plus one layer with K != F, so that a swap of the two shows.  Every
call runs on a side stream, so that the stream argument is not NULL either."""
import ctypes

import pytest
import torch

from oracle.gpu_support import call_log, dev, make_layer, pkg  # noqa: F401

pytestmark = pytest.mark.gpu

B = 3
BF16X3, FP32 = 0, 1                       # include/ggcn.h GGCN_PREC_*
PRODUCTS = ("ggcn_dweight", "ggcn_dweight_bf16", "ggcn_colsum", "ggcn_weight_pack", "ggcn_linear", "ggcn_transpose")
HD = 128                                  # the BiLSTM's hidden size


@pytest.fixture
def side_stream(dev):
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        yield ctypes.c_void_p(s.cuda_stream).value
        s.synchronize()


@pytest.fixture
def log(monkeypatch, pkg):
    return call_log(monkeypatch, PRODUCTS + ("ggcn_linear_out_bf16", "ggcn_scores_head_backward"))


def _p(t):
    return None if t is None else t.data_ptr()


def _check(log, want):
    """Compare the log with ``want`` (module docstring); returns {buffer name: address}."""
    assert [c[0] for c in log] == [w[0] for w in want]
    made = {}
    for (name, got), (_, exp) in zip(log, want):
        assert len(got) == len(exp), (name, len(got), len(exp))
        for i, (g, e) in enumerate(zip(got, exp)):
            if isinstance(e, (str, tuple)):
                buf, off = (e, 0) if isinstance(e, str) else e
                assert type(g) is int and g != 0 and g % 16 == 0, "%s argument %d (%s): %r is not an aligned pointer" % (name, i, buf, g)
                assert made.setdefault(buf, g - off) == g - off, "%s argument %d: %s moved" % (name, i, buf)
            else:
                assert g == e and type(g) is type(e), "%s argument %d: got %r, expected %r" % (name, i, g, e)
    return made


# ---------------------------------------------------------------- the gated layer
@pytest.mark.parametrize("K,F,precision,dtype", [(64, 64, "bf16x3", torch.float32), (32, 64, "bf16x3", torch.float32),
                                                 (64, 64, "fp32", torch.float32), (64, 64, "bf16x3", torch.bfloat16)],
                         ids=["bf16x3", "bf16x3-K32", "fp32", "bfloat16-features"])
def test_gated_layer_step(pkg, dev, log, side_stream, K, F, precision, dtype):
    T, st = 5, side_stream
    g = torch.Generator().manual_seed(11)
    m = make_layer(pkg, dev, 0.05 * torch.randn(K, F, generator=g), 0.1 * torch.randn(F, generator=g), precision=precision)
    x = torch.randn(B, T, K, generator=g).to(dev).to(dtype).requires_grad_()
    gates = [torch.rand(B, F, generator=g).to(dev).requires_grad_() for _ in range(3)]
    a = (torch.rand(B, T, T, generator=g) < 0.6).float()
    csr = pkg.BatchedCSR.from_dense(((a + a.transpose(1, 2) + torch.eye(T)) > 0).float().to(dev), binary=True)
    out, pa, pb = m.forward_gated(x, csr, store_gate=gates[0], pool_gate_a=gates[1], pool_gate_b=gates[2], want_out=True,
                                  want_pool_a=True, want_pool_b=True)
    torch.autograd.backward([out, pa, pb], [torch.ones_like(out), torch.ones_like(pa), torch.ones_like(pb)])
    W, N = _p(m.weight), B * T
    # ggcn_weight_pack(W, ldw, K, F, precision, transposed, wpack, stream): the transposed image is that of the [F,K] matrix W^T
    pack = ("ggcn_weight_pack", [W, F, K, F, BF16X3, 0, "image", st])
    pack_t = ("ggcn_weight_pack", [W, F, F, K, BF16X3, 1, "image of W^T", st])
    # ggcn_dweight(X, ldx, dH, ldg, n_rows, K, F, dW, lddw, precision, workspace, stream)
    dweight = ("ggcn_dweight", [_p(x), K, "dH", F, N, K, F, "dW", F, FP32 if precision == "fp32" else BF16X3, "dW workspace", st])
    # ggcn_colsum(X, ld, M, F, out, workspace, stream) on the per-graph sums [B,F]
    colsum = ("ggcn_colsum", ["d_bsum", F, B, F, "db", "db workspace", st])
    if dtype == torch.bfloat16:
        # ggcn_linear_out_bf16(X, ldx, wpack, Y, ldy, M, K, F, stream); ggcn_dweight_bf16: ggcn_dweight without the precision
        want = [pack, pack_t, ("ggcn_linear_out_bf16", ["dH", F, "image of W^T", "dX", K, N, F, K, st]),
                ("ggcn_dweight_bf16", [_p(x), K, "dH", F, N, K, F, "dW", F, "dW workspace", st]), colsum]
    elif precision == "fp32":
        # ggcn_linear(X, ldx, W, ldw, wpack, Y, ldy, M, K, F, precision, stream): the forward on W itself, dX on a plain W^T [F,K]
        want = [("ggcn_linear", [_p(x), K, W, F, None, "hidden", F, N, K, F, FP32, st]),
                ("ggcn_linear", ["dH", F, "W^T", K, None, "dX", K, N, F, K, FP32, st]), dweight, colsum]
    else:
        want = [pack, pack_t, ("ggcn_linear", ["dH", F, None, 0, "image of W^T", "dX", K, N, F, K, BF16X3, st]), dweight, colsum]
    _check(log, want)
    assert x.grad.shape == x.shape and x.grad.dtype == dtype and m.weight.grad.shape == (K, F) and m.bias.grad.shape == (F,)


# ---------------------------------------------------------------- the gate MLPs
@pytest.mark.parametrize("H", [8, 6], ids=["H=8-fused-dW1", "H=6-separate"])
def test_gate_mlps_step(pkg, dev, log, side_stream, H):
    st, Hp = side_stream, (H + 3) & ~3
    torch.manual_seed(20 + H)
    seqs = [torch.nn.Sequential(torch.nn.Sigmoid(), torch.nn.Linear(H, H), torch.nn.Sigmoid(), torch.nn.Linear(H, H),
                                torch.nn.Sigmoid()).to(dev) for _ in range(2)]
    aspect = torch.randn(B, H).to(dev).requires_grad_()
    g1, g2 = pkg.gate_mlps(aspect, *seqs)
    torch.autograd.backward([g1, g2], [torch.ones_like(g1), torch.ones_like(g2)])
    linears = [s[i] for s in seqs for i in (1, 3)]
    # ggcn_transpose(W, rows, cols, ldw, Wt, stream)
    want = [("ggcn_transpose", [_p(l.weight), H, H, H, "Wt %d" % i, st]) for i, l in enumerate(linears)]
    ldz, f = 5 * Hp, 4      # Z [B, 5 Hp] floats: dz1_A | dz1_B | dz2_A | dz2_B | s

    def dweight(name, x_col, K, other, ld_other):   # ggcn_dweight(X, ldx, dH, ldg, n_rows, K, F, dW, lddw, precision, workspace, stream)
        return ("ggcn_dweight", [("Z", f * x_col), ldz, other, ld_other, B, K, H, name, H, FP32, name + " workspace", st])
    if Hp == H:
        want.append(dweight("dW1 of both gates", 0, 2 * H, ("Z", f * 4 * Hp), ldz))
    else:
        want += [dweight("dW1 of gate %d" % g, g * Hp, H, ("Z", f * 4 * Hp), ldz) for g in (0, 1)]
    want += [dweight("dW2 of gate %d" % g, (2 + g) * Hp, H, "hidden of gate %d" % g, H) for g in (0, 1)]
    want.append(("ggcn_colsum", [("Z", 0), ldz, B, 4 * Hp, "db", "db workspace", st]))    # ggcn_colsum(X, ld, M, F, out, workspace, stream)
    _check(log, want)
    assert all(p.grad is not None and p.grad.shape == p.shape for s in seqs for p in s.parameters())


# ---------------------------------------------------------------- the scores / kl head
@pytest.mark.parametrize("strided", [False, True], ids=["contiguous-g_scores", "strided-g_scores"])
def test_scores_and_kl_step(pkg, dev, log, side_stream, strided):
    """None of the products: the head has its own weight product.  Its two gradients go through ``f32_rows``: a contiguous float32
    one is handed to the launch as it lies, a strided one as a copy (g_scores, ld_gs, g_kl are arguments 14..16 of
    ``ggcn_scores_head_backward``)."""
    T, H, C = 5, 8, 3
    torch.manual_seed(30)
    fc = torch.nn.Linear(2 * H, C).to(dev)
    x, aspect, logits = (torch.randn(*s).to(dev).requires_grad_() for s in ((B, T, H), (B, H), (B, C)))
    dist = torch.randint(0, 6, (B, T)).to(dev)
    scores, kl = pkg.scores_and_kl(x, aspect, logits, fc, dist)
    g_scores = torch.randn(B, 2 * T).to(dev)[:, ::2] if strided else torch.randn(B, T).to(dev)
    g_kl = torch.ones((), device=dev)
    torch.autograd.backward([scores, kl], [g_scores, g_kl])
    assert [c[0] for c in log] == ["ggcn_scores_head_backward"]
    args = log[0][1]
    assert args[15] == T and args[16] == _p(g_kl) and args[-1] == side_stream
    assert (args[14] != _p(g_scores)) if strided else (args[14] == _p(g_scores))
    assert type(args[14]) is int and args[14] % 16 == 0


# ---------------------------------------------------------------- the BiLSTM
def test_bilstm_train_step(pkg, dev, log, side_stream):
    st, T, I, W = side_stream, 3, 64, 8 * HD
    torch.manual_seed(40)
    lstm = torch.nn.LSTM(I, HD, bidirectional=True, batch_first=True, num_layers=1).to(dev)
    x = torch.randn(2, T, I).to(dev).requires_grad_()
    y = pkg.bilstm_train(x, lstm)
    y.backward(torch.ones_like(y))
    N, f = 2 * T, 4
    want = [
        # ggcn_weight_pack(W, ldw, K, F, precision, transposed, wpack, stream): [W_ih_f ; W_ih_r] is stored [F = 8 hd, K = I]
        ("ggcn_weight_pack", ["W_ih stack", I, I, W, BF16X3, 1, "image", st]),
        # ggcn_linear(X, ldx, W, ldw, wpack, Y, ldy, M, K, F, precision, stream)
        ("ggcn_linear", [_p(x), I, None, 0, "image", "G", W, N, I, W, BF16X3, st]),
        # ggcn_dweight(X, ldx, dH, ldg, n_rows, K, F, dW, lddw, precision, workspace, stream)
        ("ggcn_dweight", [("dG", 0), W, _p(x), I, N, W, I, "dW_ih", I, BF16X3, "dW_ih workspace", st]),
        ("ggcn_dweight", [("dG", 0), W, ("Hprev", 0), 2 * HD, N, 4 * HD, HD, "dW_hh_f", HD, BF16X3, "dW_hh_f workspace", st]),
        ("ggcn_dweight", [("dG", f * 4 * HD), W, ("Hprev", f * HD), 2 * HD, N, 4 * HD, HD, "dW_hh_r", HD, BF16X3, "dW_hh_r workspace", st]),
        # ggcn_colsum(X, ld, M, F, out, workspace, stream)
        ("ggcn_colsum", [("dG", 0), W, N, W, "db", "db workspace", st]),
        ("ggcn_weight_pack", ["W_ih stack again", I, W, I, BF16X3, 0, "image for dX", st]),
        ("ggcn_linear", [("dG", 0), W, None, 0, "image for dX", "dX", I, N, W, I, BF16X3, st]),
    ]
    made = _check(log, want)
    assert made["image"] != made["image for dX"]
    assert x.grad.shape == x.shape and all(p.grad is not None and p.grad.shape == p.shape for p in lstm.parameters())


# ---------------------------------------------------------------- hostops.cached on the device
def test_cached_image_launches_only_for_a_new_key(pkg, dev, log):
    from ed_gated_gcn_amd import _capi
    m = make_layer(pkg, dev, 0.05 * torch.randn(64, 64), None)
    lib, st = pkg.load_library(), _capi.stream_of(dev)

    def packs():
        n = len(log)
        del log[:]
        return n
    a = m._packed_weight(lib, st, precision="bf16x3")
    assert packs() == 1
    assert m._packed_weight(lib, st, precision="bf16x3") is a and packs() == 0          # a second call does not launch
    b = m._packed_weight(lib, st, precision="f16mx8")                                   # another slot, side by side with the first
    assert packs() == 1 and b is not a
    assert m._packed_weight(lib, st, precision="bf16x3") is a and m._packed_weight(lib, st, precision="f16mx8") is b and packs() == 0
    with torch.no_grad():
        m.weight.mul_(0.5)                                                              # in place: the version moves
    a2 = m._packed_weight(lib, st, precision="bf16x3")
    assert packs() == 1 and a2 is not a
    assert m._packed_weight(lib, st, precision="f16mx8") is not b and packs() == 1      # ... for every slot, each when it is asked for
    m.weight.data = m.weight.data.clone()                                               # a new data_ptr at the same version or not
    assert m._packed_weight(lib, st, precision="bf16x3") is not a2 and packs() == 1
    assert m._packed_weight(lib, st, precision="bf16x3") is m._packed_weight(lib, st, precision="bf16x3") and packs() == 0


def test_cached_transpose_launches_only_for_a_new_key(pkg, dev, log):
    from ed_gated_gcn_amd import _capi, heads
    lin = torch.nn.Linear(8, 8).to(dev)
    lib, st = pkg.load_library(), _capi.stream_of(dev)
    wt = heads._transposed(lin, lib, st)
    assert heads._transposed(lin, lib, st) is wt and [c[0] for c in log] == ["ggcn_transpose"]
    assert torch.equal(wt, lin.weight.detach().t())
    with torch.no_grad():
        lin.weight.add_(1.0)
    wt2 = heads._transposed(lin, lib, st)
    assert wt2 is not wt and len(log) == 2 and torch.equal(wt2, lin.weight.detach().t())
    lin.weight.data = lin.weight.data.clone()
    assert heads._transposed(lin, lib, st) is not wt2 and len(log) == 3
    assert heads._transposed(lin, lib, st) is heads._transposed(lin, lib, st) and len(log) == 3
