"""THE GATES OF THE GPU TESTS, DEFINED ONCE (test infrastructure, NOT product code).

What "within the gate" means for a float32 result, a bfloat16 dX and a float32 gradient, the hostile buffers the kernels are
run in, and the float64 statement of the gate / pool backward.  Pure torch: everything here runs on CPU tensors too
(``tests/test_gates_cpu.py`` pins the bounds, the NaN and dtype rejections on hand-made tensors).  A reference on another device
than the result is moved to the result's.
"""
import torch

NAN = float("nan")


def gate(got, ref, what, tol=1e-4, dtype=torch.float32):
    """Forward value / float32 result of bf16 features: |got - ref| <= tol * max(1, max|ref|), ``got`` of ``dtype``, no NaN; an
    empty tensor passes with gate 0.  Prints error and gate (``-s``); returns err / gate."""
    ref = ref.double().to(got.device)
    bound = tol * max(1.0, float(ref.abs().max())) if ref.numel() else 0.0
    err = float((got.double() - ref).abs().max()) if ref.numel() else 0.0
    print("  %s: max|diff| %.3g (gate %.3g)" % (what, err, bound))
    assert got.dtype == dtype, "%s: %s, not %s" % (what, got.dtype, dtype)
    assert err == err and err <= bound, "%s: max|diff| %.3g > %.3g" % (what, err, bound)
    return err / bound if bound else 0.0


def gate_dx(dx, ref, what="dX"):
    """bfloat16 dX: |dx - ref| <= 2^-8 |ref| + 1e-4 max|ref| for every element (one bf16 rounding of the stored value on top of
    the bf16x3 error), no NaN."""
    assert dx.dtype == torch.bfloat16, "%s: %s, not bfloat16" % (what, dx.dtype)
    ref = ref.double().to(dx.device)
    bound = 2.0 ** -8 * ref.abs() + 1e-4 * float(ref.abs().max())
    diff = (dx.double() - ref).abs()
    print("  %s (bf16): max |diff| / gate %.3f" % (what, float((diff / (bound + 1e-300)).max())))
    assert not bool(torch.isnan(diff).any()), "%s: NaN" % what
    assert not bool((diff > bound).any()), "%s: %d elements outside 2^-8|ref| + 1e-4 max|ref|" % (what, int((diff > bound).sum()))


def close32(got, ref, what, rel, dtype=torch.float32):
    """Gradient, relative form: |got - ref| <= rel * max|ref| (+ 1e-12), ``got`` of ``dtype``, no NaN.  Returns err / scale."""
    ref = ref.double().to(got.device)
    scale = float(ref.abs().max()) + 1e-12
    err = float((got.double() - ref).abs().max())
    print("  %s: max|diff| %.3g vs scale %.3g (gate %.3g)" % (what, err, scale, rel * scale))
    assert got.dtype == dtype, "%s: %s, not %s" % (what, got.dtype, dtype)
    assert err == err and err <= rel * scale, "%s: max|diff| %.3g vs scale %.3g" % (what, err, scale)
    return err / scale


def hostile(t, pad, fill=NAN):
    """t [N,F] as the first N rows of a [N + 1, F + pad] buffer: pad columns and the row after the last one are ``fill``."""
    buf = torch.full((t.shape[0] + 1, t.shape[1] + pad), fill, dtype=t.dtype, device=t.device)
    buf[:t.shape[0], :t.shape[1]] = t
    return buf


def poisoned(nbytes, dev):
    """A workspace of at least ``nbytes`` bytes of 0xFF (NaN as float32 and as bfloat16)."""
    return torch.full((max(256, int(nbytes)),), 0xFF, dtype=torch.uint8, device=dev)


def poisoned_rows(dev, rows, ld, guard, dtype=torch.float32):
    """``rows`` x ``ld`` floats (or ``dtype``) of NaN between two guard bands of ``guard`` NaN: ``(whole buffer, the view handed to
    the library)``."""
    buf = torch.full((rows * ld + 2 * guard,), NAN, dtype=dtype, device=dev)
    return buf, buf[guard:guard + rows * ld].view(rows, ld)


def first_argmax(v):
    """[B,T,F] -> one-hot [B,T,F] bool of the first maximum over t (ties: the smaller row)."""
    m = v == v.max(dim=1, keepdim=True)[0]
    return m & (m.cumsum(1) == 1)


def gate_pool_backward_statement64(out, sg, ga, gb, d_out, d_pa, d_pb, adj, inv, keep=None):
    """float64 statement of the formulas in the headers of csrc/gate_pool_backward_mma.hip and (with keep factors)
    csrc/gate_pool_backward_weighted.hip, on float32 inputs ([B,T,F] / [B,F]; None = absent; keep = (ks, ka, kb), each float64
    [B,T,F] or None; keep=None is (None, None, None), which multiplies and divides by exact ones only).  The pools' winners are
    taken from the float32 values the kernel itself compares: y32 = out * inv_sg / ks (0 where ks = 0), candidates y32 * g * k."""
    B, T, F = out.shape
    ks, ka, kb = keep if keep is not None else (None, None, None)
    one32, one64 = torch.ones(B, T, F, device=out.device), torch.ones(B, T, F, dtype=torch.float64, device=out.device)
    ks32, ks64 = (one32, one64) if ks is None else (ks.float(), ks)
    inv_sg32 = torch.ones(B, F, device=out.device) if sg is None else torch.where(sg != 0, 1.0 / sg, torch.zeros_like(sg))
    inv_sg64 = one64[:, 0] if sg is None else torch.where(sg != 0, 1.0 / sg.double(), torch.zeros_like(sg).double())
    y32 = torch.where(ks32 != 0, out * inv_sg32[:, None, :] / ks32, torch.zeros_like(out))
    y = torch.where(ks64 != 0, out.double() * inv_sg64[:, None, :] / ks64, torch.zeros_like(one64))
    dy = torch.zeros(B, T, F, dtype=torch.float64, device=out.device)
    r = {}
    if d_out is not None:
        dy = dy + d_out.double() * (1.0 if sg is None else sg.double()[:, None, :]) * ks64
        r["d_sg"] = (d_out.double() * y * ks64).sum(1)
    else:
        r["d_sg"] = torch.zeros(B, F, dtype=torch.float64, device=out.device)
    for key, g, dp, k in (("d_ga", ga, d_pa, ka), ("d_gb", gb, d_pb, kb)):
        if dp is None:
            continue
        g32 = torch.ones(B, F, device=out.device) if g is None else g
        k32, k64 = (one32, one64) if k is None else (k.float(), k)
        hot = first_argmax(y32 * g32[:, None, :] * k32).double()
        dy = dy + hot * (dp.double() * g32.double())[:, None, :] * k64
        r[key] = dp.double() * (hot * y * k64).sum(1)
    r["dY"], r["d_bsum"] = dy, dy.sum(1)
    r["dH"] = torch.einsum("bts,btf->bsf", adj.double(), inv.double().view(B, T, 1) * dy)
    return r
