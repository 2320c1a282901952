#!/usr/bin/env python3
"""sha256 of everything the one-launch gate / pool backward entries of libggcn_hip.so write, at the smallest shapes at which
their kernels can go wrong: one line per case and output.  Two builds of the library that compute the same thing print the
same listing, line for line (the kernels have a fixed summation order; max |dH| is an order-free atomicMax):

    GGCN_LIB=/path/to/other/libggcn_hip.so python tools/backward_digest.py > other.txt
    python tools/backward_digest.py > this.txt && cmp other.txt this.txt

Entries, through the C ABI: ggcn_gate_pool_backward_mma, _weighted, _weighted_drop (graphs of 1, 5, 32 nodes), _wide,
_weighted_wide (33, 64, 100, 128 nodes) and the builders ggcn_graph_operands_weighted_t / _weighted_wide_t.  B = 3; F = 4 (a
lone 16-byte store), 36 (a partial second tile), 132 (a second trip of wavefront 0 in the wide kernels), 260 (a second trip in
the 64-column-group kernels); operands: all there, no d_out, no pools, no gates; dY stored and not; leading dimensions = F, and
once F + 12.  `out` takes a few distinct values, so the pools tie within a lane and across the two lane halves.  Outputs are
pre-filled, so a store outside a tile shows as well."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ed_gated_gcn_amd as pkg  # noqa: E402
from ed_gated_gcn_amd import _capi  # noqa: E402

B = 3
NARROW_T, WIDE_T = (1, 5, 32), (33, 64, 100, 128)
FS = (4, 36, 132, 260)
PRESENCE = ("all", "no d_out", "no pools", "no gates")
FILL = -7.0   # what a byte no kernel wrote still holds
DROP = (0.25, 12345, 1, 2, 0)   # p, seed, the keep streams of the store gate and the two pool gates


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def inputs(T, F, ld, presence, rng, dev):
    """The operands of one call: [B*T, ld] matrices of which F columns are used, [B, F] gates and pool gradients."""
    def mat(a):
        full = np.full((B * T, ld), 0.5, np.float32)
        full[:, :F] = a
        return torch.from_numpy(full).to(dev)
    sg = rng.uniform(0.25, 1.0, (B, F)).astype(np.float32)
    sg[0, 0] = 0.0   # a closed store gate: y = 0 for the whole column
    v = dict(out=mat(np.round(rng.standard_normal((B * T, F)) * 2.0) / 2.0), d_out=mat(rng.standard_normal((B * T, F))))
    for name in ("ga", "gb", "d_pa", "d_pb"):
        v[name] = torch.from_numpy(rng.uniform(-1.0, 1.0, (B, F)).astype(np.float32)).to(dev)
    v["sg"] = torch.from_numpy(sg).to(dev)
    for name in {"no d_out": ("d_out",), "no pools": ("d_pa", "d_pb"), "no gates": ("sg", "ga", "gb")}.get(presence, ()):
        v[name] = None
    return v


def adjacency(T, rng, real):
    a = (rng.random((B, T, T)) < min(1.0, 3.0 / T)).astype(np.float32)
    a[:, np.arange(T), np.arange(T)] = 1.0
    return a * rng.uniform(0.1, 2.0, a.shape).astype(np.float32) if real else a


def main():
    dev = torch.device("cuda:0")
    lib = pkg.load_library()
    p, st = _capi.ptr, _capi.stream_of(dev)

    def run(case, entry, v, T, F, ld, operands, with_dy, has_dy, tail=(), amax=False):
        """One call of `entry`; prints the sha256 of every output."""
        o = {n: torch.full((B * T, ld), FILL, device=dev) for n in ("dH",) + (("dY",) if with_dy else ())}
        o.update({n: torch.full((B, F), FILL, device=dev) for n in ("d_sg", "d_ga", "d_gb", "d_bsum")})
        if amax:
            o["dh_amax"] = torch.zeros(1, device=dev)
        args = [p(v["out"]), ld, p(v["sg"]), p(v["ga"]), p(v["gb"]), p(v["d_out"]), ld, p(v["d_pa"]), p(v["d_pb"])]
        args += [p(x) for x in operands] + [B, T, F, p(o["dH"]), ld]
        args += [p(o.get("dY")), ld] if has_dy else []
        args += [p(o[n]) for n in ("d_sg", "d_ga", "d_gb", "d_bsum")] + ([p(o["dh_amax"])] if amax else [])
        _capi.check(getattr(lib, entry)(*args, *tail, st), entry)
        torch.cuda.synchronize()
        for name, t in o.items():
            print("%s %s %s %s" % (entry, case, name, sha(t)), flush=True)

    def build(entry, sizer, csr, T, by_length):
        ops = torch.full((getattr(lib, sizer)(*((B, T) if by_length else (B,))),), 0xA5, dtype=torch.uint8, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        _capi.check(getattr(lib, entry)(p(csr.rowptr), p(csr.colidx), p(csr.vals), B, T, p(ops), p(flag), st), entry)
        torch.cuda.synchronize()
        print("%s T=%d operand %s" % (entry, T, sha(ops)), flush=True)
        print("%s T=%d flag %s" % (entry, T, sha(flag)), flush=True)
        return ops

    for T in NARROW_T + WIDE_T:
        rng = np.random.default_rng(1000 + T)
        wide = T > 32
        c01 = pkg.BatchedCSR.from_dense(torch.from_numpy(adjacency(T, rng, False)).to(dev), binary=True)
        cw = pkg.BatchedCSR.from_dense(torch.from_numpy(adjacency(T, rng, True)).to(dev), binary=False)
        inv01, invw = c01.inv_denominators(), cw.inv_denominators()
        if wide:
            opsw = build("ggcn_graph_operands_weighted_wide_t", "ggcn_graph_operands_weighted_wide_t_bytes", cw, T, True)
            forms = (("ggcn_gate_pool_backward_wide", (c01.rowmask_t_wide, inv01), False, {}),
                     ("ggcn_gate_pool_backward_weighted_wide", (opsw, invw), True, {}))
        else:
            opsw = build("ggcn_graph_operands_weighted_t", "ggcn_graph_operands_weighted_t_bytes", cw, T, False)
            forms = (("ggcn_gate_pool_backward_mma", (c01.graph_ops, c01.graph_ops_t), False, dict(amax=True)),
                     ("ggcn_gate_pool_backward_weighted", (opsw, invw), True, {}),
                     ("ggcn_gate_pool_backward_weighted_drop", (opsw, invw), True, dict(tail=DROP)))
        shapes = [(F, F, pr) for F in FS for pr in PRESENCE] + [(36, 48, "all")]   # the last: every leading dimension > F
        for F, ld, presence in shapes:
            v = inputs(T, F, ld, presence, rng, dev)
            for entry, operands, has_dy, kw in forms:
                for with_dy in ((True, False) if has_dy and presence == "all" else (has_dy,)):
                    case = "T=%d F=%d ld=%d %s%s" % (T, F, ld, presence, "" if with_dy or not has_dy else ", no dY")
                    run(case, entry, v, T, F, ld, operands, with_dy, has_dy, **kw)


if __name__ == "__main__":
    main()
