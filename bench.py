#!/usr/bin/env python3
"""Headline benchmark: gated-GCN forward throughput (edges/s) on MI355X.

One "step" = one pass of the hot path (models/bert_amir5.py:621-640: gate -> gc1 -> gate ->
gc2 -> gate -> max-pool, 2 GraphConvolution layers, models/gcn.py:30-45) over one batch of
synthetic dependency graphs already resident in HBM.  Workload = BASELINE.json configs[1]:
4096 graphs x 32 tokens, avg degree 4 (nnz = 524288 incl. self loops), hidden = 768, fp32.

    python bench.py --gpus 1 --steps 50 --warmup 10
    python bench.py --gpus 1 --steps 50 --warmup 10 --full          # + box, other precisions, CPU baseline, appendices
    python bench.py --gpus 1 --steps 50 --warmup 10 --dump-outputs DIR   # + the last timed step's outputs as .npy
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W
    python bench.py --config 4          # BASELINE.json configs[3]: 256 x 512-token graphs, hidden 1024, fp16 features

N > 1 (BASELINE.json configs[2]): the SAME 4096-graph batch is sharded over the ranks -- contiguous graph
ranges balanced by nnz, weights replicated; graphs are independent, so the data path has no exchange -- and
the per-shard pooled outputs out[B_r, H] are all-gathered over RCCL/xGMI each step, the path's only
collective; "scaling": "strong".  `--scaling weak` gives every rank its own 4096-graph batch.
Rank 0 prints ONE JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8.0 TB/s (spec)
MFMA_BF16_PEAK_TF = 2500.0   # dense bf16 MFMA peak (spec, no sparsity)
MFMA_F32_PEAK_TF = 157.3     # f32-input MFMA peak
SURVEY_8D_BYTES_PER_LAYER = 822873092   # 2*4*N*H + 4(N+1) + 4E + 4*B*H + 4H^2 + 4H
DUMP_BUDGET_BYTES = 60 << 20            # --dump-outputs: all files together (under 64 MB with the .npy headers)
DUMP_SAMPLE_SEED = 20251016             # --dump-outputs: which rows of an output too large to write whole

ISSUE_NOTE = {
    "f16mx6": "the f16mx6 linear spends 96 matrix-pipe cycles per 32x32x32 block (64 fp16 + 32 block-scaled fp6) where plain "
              "bf16 spends 64, so its ceiling on this peak is 2/3 (1667 TFLOP/s)",
    "bf16x3": "the bf16x3 linear issues 3 bf16 MFMA flops per algorithmic flop, so its ceiling on this peak is 1/3 "
              "(833 TFLOP/s)",
    "f16mx8": "the f16mx8 linear spends 128 matrix-pipe cycles per 32x32x32 block (64 fp16 + 64 block-scaled fp8) "
              "where plain bf16 spends 64, so its ceiling on this peak is 1/2 (1250 TFLOP/s)",
    "fp32": "exact fp32 MFMA (v_mfma_f32_32x32x2_f32)",
    "f16": "plain fp16 MFMA: one matrix-pipe flop per algorithmic flop",
}
DTYPE_NOTE = {"f16mx6": "f32 (fp16 MFMA + block-scaled fp6 correction MFMA, fp32 accumulate)", "fp32": "f32", "bf16x3": "f32 (bf16x3 MFMA split, fp32 accumulate)", "f16": "f16 (fp16 MFMA, fp32 accumulate)",
              "f16mx8": "f32 (fp16 MFMA + block-scaled fp8 correction MFMA, fp32 accumulate)"}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--config", type=int, default=2, choices=[2, 4],
                    help="2: BASELINE.json configs[1]/[2] (4096 x 32 tokens, hidden 768, fp32, 2 layers; the headline); "
                         "4: configs[3] (256 x 512 tokens, degree 6, hidden 1024, fp16 features, 1 gated layer)")
    ap.add_argument("--precondition", type=int, default=-1,
                    help="untimed steps run before the warm-up: the chip needs ~0.1 s of load to settle (measured: "
                         "the first ~60 steps after an idle period run 4.5 %% slower, DESIGN.md 5); the W warm-up "
                         "steps and the K timed steps follow as the contract says.  -1 (default): adaptive -- "
                         "windows of 50 steps until two consecutive windows agree within 1 %% (at least 150, at most "
                         "2000 steps)")
    ap.add_argument("--graphs", type=int, default=None, help="graphs in the batch (config 2: 4096, config 4: 256)")
    ap.add_argument("--tokens", type=int, default=None)
    ap.add_argument("--hidden", type=int, default=None)
    ap.add_argument("--degree", type=float, default=None)
    ap.add_argument("--precision", default=os.environ.get("GGCN_PRECISION"),
                    choices=["f16mx8", "f16mx6", "bf16x3", "fp32", "f16"],
                    help="arithmetic of the dense linear of the TIMED run; all three meet the 1e-4 parity gate "
                         "(tests/test_gpu_parity.py) and the other two are timed beside it (alt_precisions)")
    ap.add_argument("--scaling", default="strong", choices=["weak", "strong"],
                    help="strong (default, BASELINE configs[2]): --graphs in total, sharded over the GPUs; "
                         "weak: --graphs per GPU")
    ap.add_argument("--path", default="block", choices=["block", "layers", "unfused"],
                    help="block: the whole gated block as one launch (default); layers: one launch per layer; "
                         "unfused: linear + aggregate (2 launches per layer)")
    ap.add_argument("--capture", default="auto", choices=["auto", "on", "off"],
                    help="replay the step from a hipGraph (auto: when N > 1, where a shard's kernels are short enough "
                         "for the host launch path to show)")
    ap.add_argument("--gather", default="logits", choices=["logits", "pooled"],
                    help="N > 1: what every rank all-gathers per step -- per-shard logits [B_r, 34] = out . Wd (north_star; the "
                         "out-dependent share of bert_amir5.py:643's dense, 70 KB per rank at 8 GPUs) or the pooled out [B_r, H] itself "
                         "(1.5 MB per rank)")
    ap.add_argument("--gather-mode", default="async", choices=["async", "flag", "graph"],
                    help="N > 1: async (default) = all_gather_into_tensor(async_op=True) on RCCL's own stream behind every replay, so that step "
                         "i's gather overlaps step i+1's kernels; flag = the same eager collective issued from a side stream that "
                         "hipStreamWaitValue32 holds until the step's head launch has counted itself done in memory (ggcn_dense_head_signal): "
                         "no event record and no wait on the replay stream (logits payload, two-layer block, backend nccl; otherwise async); "
                         "graph = the all-gather captured INSIDE the step's hipGraph (one graph launch "
                         "per step and no cross-stream events: 95 vs 109 us per step at a 512-graph shard with a process group of one, "
                         "DESIGN.md 6; on 8 GPUs the RCCL kernel then runs serially behind the step -- unmeasured, hence opt-in; equal shards only)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-alt", action="store_true", help="skip the alt_precisions / accuracy legs")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL); 'gloo' only to "
                    "rehearse the N>1 code path on a one-GPU box together with --same-device")
    ap.add_argument("--same-device", action="store_true", help="rehearsal: every rank uses cuda:0")
    ap.add_argument("--force-dist", action="store_true",
                    help="run the N > 1 step loop (process group, hipGraph replay, logits head, asynchronous all-gather per "
                         "step) at ANY world size -- with --gpus 1 this is RCCL's whole code path on a one-GPU box "
                         "(tests/test_gpu_parity.py drives it with --backend nccl)")
    ap.add_argument("--cpu-graphs", type=int, default=None, help="sample size of the CPU baseline")
    ap.add_argument("--check-gather", action="store_true",
                    help="N > 1: after the timed region rank 0 recomputes the UNSHARDED batch on its own GPU and compares "
                         "the last gathered payload with it bit for bit (tests/test_gpu_parity.py drives this)")
    ap.add_argument("--no-config4", action="store_true",
                    help="N = 1, config 2: skip the compact configs[3] block (a child run of this script with --config 4)")
    ap.add_argument("--no-box", action="store_true", help="N = 1: skip the `box` block (power / clock under load / MFMA calibration after the timed region)")
    ap.add_argument("--master-port", type=int, default=0, help="self-launch (N > 1 without torch.distributed.run): rendezvous port, 0 = pick a free one")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beyond the headline after the timed region: the `box` block, other precisions "
                         "and their accuracy (alt_precisions, max_abs_err, product_default), the CPU baseline and, at N = 1 with "
                         "config 2, the eval / ACE-cased / config 4 / 512-graph-shard appendices (the --no-* options still drop "
                         "single legs).  Without it the run sets up, warms up, times the K steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed region, write what the last timed step computed (rank 0's outputs of the path, and at "
                         "N > 1 the last gathered payload) as DIR/<name>.npy in float32; an output larger than its share of "
                         "%d MiB is written as a fixed, seeded sample of its rows (the `dump` block of the line says which)"
                         % (DUMP_BUDGET_BYTES >> 20))
    a = ap.parse_args()
    if a.steps < 1:
        raise SystemExit("--steps must be at least 1")
    if not a.full:   # a plain run: the headline figure alone
        a.no_box = a.no_alt = a.no_cpu_baseline = a.no_config4 = True
    d = {2: (4096, 32, 768, 4.0, 4096), 4: (256, 512, 1024, 6.0, 16)}[a.config]
    a.graphs = a.graphs or d[0]
    a.tokens = a.tokens or d[1]
    a.hidden = a.hidden or d[2]
    a.degree = a.degree or d[3]
    a.cpu_graphs = a.cpu_graphs or d[4]
    # config 2: fp32 features at fp32-level accuracy (1e-4 gate) -> f16mx8; config 4: fp16 features and a 2e-3 gate ->
    # plain fp16 MFMA ("f16": half of f16mx8's matrix-pipe time, error below the rounding of the fp16 output)
    a.precision = a.precision or {2: "f16mx8", 4: "f16"}[a.config]
    if a.precision == "f16" and a.config != 4:
        raise SystemExit("--precision f16 is for the fp16 features of --config 4")
    return a


def cpu_baseline(x, adj, g1, g2, w1, b1, w2, b2, n_graphs, one_layer):
    """The reference's dense algorithm (oracle/ref_dense.py, bit-equal to the imported reference in
    the build container) on this host's cores: 1 warm-up + median of 5 forwards."""
    import torch
    from oracle import ref_dense
    avail = len(os.sched_getaffinity(0))
    n = min(n_graphs, x.shape[0])
    xs, adjs, g1s, g2s = x[:n].float(), adj[:n].float(), g1[:n], g2[:n]
    nnz = int((adj[:n] != 0).sum())

    def once():
        t0 = time.perf_counter()
        with torch.no_grad():
            if one_layer:   # config 4: gcn.py:30-45 + both gates and pools of bert_amir5.py:627-636
                y = ref_dense.graph_convolution(xs, adjs, w1, b1)
                torch.max(y * g1s[:, None, :], 1)
                torch.max(y * g2s[:, None, :], 1)
            else:
                ref_dense.gated_block(xs, adjs, g1s, g2s, w1, b1, w2, b2)
        return time.perf_counter() - t0

    # torch-CPU slows down when oversubscribed on many-core hosts: probe a few thread counts
    # (one forward each after a warm-up) and time the fastest -- the baseline gets its best shot.
    best, cores = None, avail
    for c in sorted({min(avail, k) for k in (16, 32, 64, avail)}):
        torch.set_num_threads(c)
        once()
        t = once()
        if best is None or t < best:
            best, cores = t, c
    torch.set_num_threads(cores)
    times = [once() for _ in range(5)]
    t = statistics.median(times)
    return {"value": nnz / t, "unit": "edges/s", "cores": cores, "kind": "port",
            "sample": "%d of the %d graphs (T=%d, H=%d, %s, dense adj, torch-CPU fp32), "
                      "threads chosen from {16,32,64,all=%d} by a probe, median of 5, %.3f s per forward"
                      % (n, x.shape[0], x.shape[1], x.shape[2], "1 gated layer" if one_layer else "2 layers", avail, t)}


def block_float64(x, adj, g1, g2, w1, b1, w2, b2, one_layer):
    """float64 evaluation of models/gcn.py:30-45 + models/bert_amir5.py:621-640 on a small slice: the yardstick of
    `max_abs_err` (plain torch-CPU double arithmetic written out here; nothing is imported for it)."""
    import torch
    a = adj.double()
    den = a.sum(2, keepdim=True) + 1
    x, g1, g2, w1, b1, w2, b2 = (t.double() for t in (x, g1, g2, w1, b1, w2, b2))
    gcn1 = (a @ (x @ w1)) / den + b1
    r = {"x1": (gcn1 * g1[:, None, :]).max(1)[0], "y1": (gcn1 * g2[:, None, :]).max(1)[0]}
    if not one_layer:
        x2 = g2[:, None, :] * ((a @ (gcn1 @ w2)) / den + b2)
        r.update({"x": x2, "out": x2.max(1)[0]})
    return r


def capture_steps(torch, dev, forward, gather_in_graph=None):
    """Two hipGraph copies of one step with their own output buffers: step i's all-gather may still be reading
    copy i % 2 while step i+1 replays the other one.  gather_in_graph(r, k) (--gather-mode graph): called inside the capture
    right after the step's kernels -- the collective becomes a node of the graph."""
    graphs = []
    for k in range(2):
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(2):
                forward()
        torch.cuda.current_stream(dev).wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(g):
            r = forward()
            if gather_in_graph is not None:
                gather_in_graph(r, k)
        graphs.append((g, r))
    return graphs


def percentiles(v):
    v = sorted(v)
    pick = lambda q: v[min(len(v) - 1, int(round(q * (len(v) - 1))))]
    return {"median": statistics.median(v), "p10": pick(0.10), "p90": pick(0.90), "min": v[0], "max": v[-1]}


def dump_outputs(out_dir, arrays):
    """--dump-outputs: {name: tensor} -> out_dir/<name>.npy in float32 (float64 stays float64).  Smallest first, every array
    gets an equal share of what is left of DUMP_BUDGET_BYTES; one larger than its share is written as the rows (first axis)
    that a fixed seed picks, in ascending order, so that two builds given the same arguments write the same sample.
    Returns what was written."""
    import numpy as np
    import torch
    arrays = {k: v.detach() for k, v in arrays.items() if isinstance(v, torch.Tensor)}
    arrays = {k: v.double() if v.dtype == torch.float64 else v.float() for k, v in arrays.items()}
    os.makedirs(out_dir, exist_ok=True)
    left = DUMP_BUDGET_BYTES
    written = {}
    for i, name in enumerate(sorted(arrays, key=lambda k: (arrays[k].numel() * arrays[k].element_size(), k))):
        t = arrays[name]
        share = left // (len(arrays) - i)
        row_bytes = t[0].numel() * t.element_size() if t.dim() and t.shape[0] else 0
        entry = {"shape": list(t.shape), "dtype": str(t.dtype).replace("torch.", "")}
        if t.dim() and row_bytes and t.numel() * t.element_size() > share:
            n = max(1, share // row_bytes)
            rows = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(t.shape[0], size=n, replace=False))
            t = t[torch.from_numpy(rows).to(t.device)]
            entry.update({"rows_written": int(n), "rows_seed": DUMP_SAMPLE_SEED})
        np.save(os.path.join(out_dir, name + ".npy"), t.cpu().numpy())
        left -= t.numel() * t.element_size()
        written[name] = entry
    return dict(sorted(written.items()))


def self_launch(args):
    """`python bench.py --gpus N` typed as is, N > 1: this process has not touched the GPU yet (torch is not even
    imported), so it starts N fresh rank processes through torch.distributed.run -- as a CHILD, never an exec -- relays
    their output (rank 0 prints the JSON line) and exits with their code."""
    import socket
    import subprocess
    port = args.master_port
    if not port:
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: RCCL needs it on this driver
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def config4_block(timeout_s=600):
    """BASELINE.json configs[3] measured by a child run of this script (`--config 4`) AFTER this process's own timed
    region: a compact block of the --full line, so that one command records it."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--config", "4", "--steps", "60", "--warmup", "20",
           "--no-cpu-baseline", "--full"]
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout_s)
        line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
        r = json.loads(line)
    except Exception as e:   # noqa: BLE001 -- the headline must not die with its appendix
        return {"error": "%s: %s" % (type(e).__name__, str(e)[:200])}
    roof = r.get("roofline") or {}
    return {"workload": r["config"]["workload"], "precision": r["config"]["precision"], "path": r["config"]["path"],
            "ms_per_step": r["ms_per_step"], "edges_per_sec": r["value"], "steps": r["steps"], "warmup": r["warmup"],
            "step_us_median": r["step_us"]["median"],
            "roofline": {k: roof.get(k) for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "avg_launch_us",
                                                  "hbm_GBps", "hbm_frac", "algorithmic_bytes_per_launch", "traffic")},
            "forward_hbm_frac": r["forward_hbm_frac"],
            "max_abs_err": (r.get("max_abs_err") or {}).get("value"),
            "max_abs_err_gate": "2e-3 (fp16 features, SURVEY 8d)",
            "measured_by": "child process `bench.py --config 4 --steps 60 --warmup 20 --full` after the headline's timed region"}


def shard512_block(ms_full, timeout_s=300):
    """The scaling ceiling one GPU can measure: the step of a 512-graph shard exactly as rank 0 of 8 would
    run it -- hipGraph replay of the block, the logits head, one asynchronous all-gather per step over RCCL with a process
    group of one -- by a child run of this script after the headline's timed region.  t4096/t512 is what 8 GPUs could reach
    if the collective and the ranks' skew cost nothing; NO scaling curve is measured here."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--gpus", "1", "--force-dist", "--graphs", "512", "--steps", "400",
           "--warmup", "100", "--no-cpu-baseline", "--no-alt", "--no-config4", "--no-box"]
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout_s)
        line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
        r = json.loads(line)
    except Exception as e:   # noqa: BLE001 -- the headline must not die with its appendix
        return {"error": "%s: %s" % (type(e).__name__, str(e)[:200])}
    us = r["ms_per_step"] * 1e3
    return {"shard512_us": us, "step_us_median": r["step_us"]["median"], "t4096_over_t512": ms_full * 1e3 / us,
            "hipgraph_replay": r["config"]["hipgraph_replay"], "backend": (r.get("rccl") or {}).get("backend"),
            "measured_by": "child process `bench.py --gpus 1 --force-dist --graphs 512 --steps 400 --warmup 100`: 512 of the 4096 graphs on ONE GPU, "
                           "hipGraph replay + logits head + all_gather_into_tensor on RCCL at world size 1",
            "note": "an upper bound of the 1 -> 8 GPU speed-up from one GPU's view (8 ranks of 512 graphs, free collective); no run on more than "
                    "one MI355X was made by the builder and no scaling curve exists"}


def eval_block(pkg, torch, dev, x, csr, g1, g2, gc1, gc2):
    """The eval form beside the full block (NOT the headline): train.py:227 keeps the logits only and those need `out` alone
    (bert_amir5.py:640,643) -- gated_gcn_block(..., want=("out",)) launches only the W12 column tiles.  Same inputs, same
    process, HIP events, after the timed region."""
    try:
        res = {}
        with torch.no_grad():
            for name, want in (("full_block_us", None), ("eval_logits_only_us", ("out",))):
                f = lambda: pkg.gated_gcn_block(x, csr, g1, g2, gc1, gc2, want=want)   # noqa: E731
                for _ in range(120):
                    f()
                ts = []
                for _ in range(8):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(10):
                        f()
                    e1.record()
                    torch.cuda.synchronize()
                    ts.append(e0.elapsed_time(e1) / 10 * 1e3)
                res[name] = statistics.median(ts)
            same = torch.equal(pkg.gated_gcn_block(x, csr, g1, g2, gc1, gc2, want=("out",))["out"],
                               pkg.gated_gcn_block(x, csr, g1, g2, gc1, gc2)["out"])
        res.update({"out_bitwise_equal_to_full_block": bool(same),
                    "note": "want=(\"out\",): only the W12 tiles of ggcn_block_fused, no x1 / y1 / xy, no [B,T,H] store of x; an appendix -- the "
                            "headline keeps all five outputs of SURVEY 8(d); median of 8 x 10 forwards behind 120 untimed ones"})
        return res
    except Exception as e:   # noqa: BLE001
        return {"error": "%s: %s" % (type(e).__name__, str(e)[:200])}


def ace_block(pkg, synth, torch, dev, precision):
    """One gated layer on an ACE-cased-shaped batch (512 graphs x 231 tokens -- ORI_ML of constant.py:267 -- degree 4, hidden
    768, fp32): the one-launch layer (eight wavefronts per graph) against linear + aggregate, timed with HIP events in this
    process AFTER the headline's timed region; a compact appendix of the default line."""
    import statistics
    try:
        B, T, H = 512, 231, 768
        adj = synth.dependency_batch(B, T, 4.0)
        rp, ci, _ = synth.csr_from_dense_host(adj)
        csr = pkg.BatchedCSR.from_arrays(rp, ci, B, T, dev)
        nnz = int(rp[-1])
        x = torch.randn(B, T, H, device=dev)
        g1, g2 = torch.rand(B, H, device=dev), torch.rand(B, H, device=dev)
        w, b = synth.layer_params(H, H, seed=1)
        res = {}
        for name, fused in (("one_launch", True), ("linear_plus_aggregate", False)):
            m = pkg.GraphConvolution(H, H, None).to(dev)
            m.precision, m.fused = precision, fused
            with torch.no_grad():
                m.weight.copy_(torch.from_numpy(w)); m.bias.copy_(torch.from_numpy(b))
                assert m.takes_fused_path(x, csr) == fused
                f = lambda: m.forward_gated(x, csr, store_gate=g2, pool_gate_a=g1, pool_gate_b=g2, want_pool_a=True, want_pool_b=True)  # noqa: E731
                for _ in range(120):     # ~50 ms of load: the chip's clocks settle; fewer and the timed launches ride the ramp
                    f()
                ts = []
                for _ in range(8):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(10):
                        f()
                    e1.record()
                    torch.cuda.synchronize()
                    ts.append(e0.elapsed_time(e1) / 10 * 1e3)
            res[name] = statistics.median(ts)
        # the two-layer block at this length (bert_amir5.py:626-640): all five outputs (two one-launch layers), and the eval form
        # (train.py:227 keeps the logits: only `out`; Z = D.A.X + one layer launch through W12, no product with W1)
        ls = []
        for seed in (1, 2):
            ww, bb = synth.layer_params(H, H, seed=seed)
            m = pkg.GraphConvolution(H, H, None).to(dev)
            m.precision = precision
            with torch.no_grad():
                m.weight.copy_(torch.from_numpy(ww)); m.bias.copy_(torch.from_numpy(bb))
            ls.append(m.eval())
        with torch.no_grad():
            for name, want in (("block_all_outputs_us", None), ("block_eval_out_only_us", ("out",))):
                f = lambda: pkg.gated_gcn_block(x, csr, g1, g2, ls[0], ls[1], want=want)   # noqa: E731
                for _ in range(60):
                    f()
                ts = []
                for _ in range(6):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(10):
                        f()
                    e1.record()
                    torch.cuda.synchronize()
                    ts.append(e0.elapsed_time(e1) / 10 * 1e3)
                res[name] = statistics.median(ts)
        t = res["one_launch"]
        layer_bytes = 2 * B * T * H * 4 + H * H * 4 + nnz * 4 + (B * T + 1) * 4 + 5 * B * H * 4
        return {"workload": "512 graphs x 231 tokens (ACE cased, constant.py:267), degree 4, hidden 768, fp32, 1 gated layer with both gates and pools",
                "precision": precision, "one_launch_us": t, "linear_plus_aggregate_us": res["linear_plus_aggregate"],
                "block_all_outputs_us": res["block_all_outputs_us"], "block_eval_out_only_us": res["block_eval_out_only_us"],
                "block_note": "the two-layer block at this length: two one-launch layers (all five outputs) / the eval form (only `out`: ggcn_aggregate on the "
                              "features + one layer launch through W12 = W1.W2, ggcn_layer_fused_prebias)",
                "edges_per_sec": nnz / (t * 1e-6), "hbm_frac": layer_bytes / (t * 1e-6) / 1e9 / HBM_PEAK_GBS,
                "kernel": "layer_fused_wide8_kernel (eight wavefronts per graph x 256 columns, edge-list neighbour sums from an fp32 LDS tile)",
                "timed": "median of 8 x 10 launches behind 120 untimed ones, HIP events, after the headline's timed region"}
    except Exception as e:   # noqa: BLE001 -- the headline must not die with its appendix
        return {"error": "%s: %s" % (type(e).__name__, str(e)[:200])}


# ---- the state of the box: what makes a figure taken on one MI355X readable on another -------------
# The block kernel sits at the board's power cap, so its time follows the clock each device holds under an MFMA-dense load.
# Everything below runs AFTER the timed region; nothing here touches the product kernels or the timed steps.
MFMA_CALIB_REF_US = 341.0   # ggcn_debug_mfma_calibrate(6144, 24) on the boxes of profiles/r05_box_calibration.json (their median)


def _read(path):
    try:
        with open(path) as f:
            return f.read().strip()
    except OSError:
        return None


def _amd_cards():
    """sysfs directories of the AMD GPUs with a power sensor: [(card dir, hwmon dir)]."""
    import glob
    out = []
    for hw in sorted(glob.glob("/sys/class/drm/card[0-9]*/device/hwmon/hwmon*")):
        if _read(os.path.join(hw, "power1_average")) is not None or _read(os.path.join(hw, "power1_input")) is not None:
            out.append((os.path.dirname(os.path.dirname(hw)), hw))
    return out


class PowerSampler:
    """Reads board power, power cap and the shader-clock DPM state from sysfs every ~20 ms on a helper thread (plain file
    reads: no GPU call, no child process) while the caller keeps the GPU busy."""

    def __init__(self):
        import threading
        self.cards = _amd_cards()
        self.samples = {c: [] for c, _ in self.cards}
        self.sclk = {c: [] for c, _ in self.cards}
        self._stop = threading.Event()
        self._thread = threading.Thread(target=self._run, daemon=True)

    def _run(self):
        while not self._stop.is_set():
            for card, hw in self.cards:
                v = _read(os.path.join(hw, "power1_average")) or _read(os.path.join(hw, "power1_input"))
                if v and v.isdigit():
                    self.samples[card].append(int(v) / 1e6)
                cur = [l for l in (_read(os.path.join(card, "pp_dpm_sclk")) or "").splitlines() if l.rstrip().endswith("*")]
                if cur:
                    try:
                        self.sclk[card].append(float(cur[0].split(":")[1].lower().replace("mhz", "").replace("*", "").strip()))
                    except (IndexError, ValueError):
                        pass
            self._stop.wait(0.02)

    def __enter__(self):
        self._thread.start()
        return self

    def __exit__(self, *exc):
        self._stop.set()
        self._thread.join(timeout=2)

    def summary(self):
        """The busiest card's figures (on a one-GPU box there is one; on a shared node the loaded card is this process's)."""
        best = None
        for card, hw in self.cards:
            v = self.samples[card]
            if len(v) >= 3 and (best is None or statistics.mean(v) > statistics.mean(self.samples[best[0]])):
                best = (card, hw)
        if best is None:
            return {"power_w": None, "power_cap_w": None, "sclk_dpm_mhz": None, "note": "no readable power sensor under /sys/class/drm"}
        card, hw = best
        v, c = self.samples[card], self.sclk[card]
        cap = _read(os.path.join(hw, "power1_cap"))
        return {"power_w": statistics.median(v), "power_w_max": max(v), "power_samples": len(v),
                "power_cap_w": int(cap) / 1e6 if cap and cap.isdigit() else None,
                "sclk_dpm_mhz": statistics.median(c) if c else None,
                "device_unique_id": _read(os.path.join(card, "unique_id")), "card": os.path.basename(os.path.dirname(card))}


def clock_from_stamps(stamps):
    """uint64 [n_wg, 2] = (d s_memtime, d s_memrealtime) per workgroup -> (median clock in MHz, median loop time in us)."""
    c, w = stamps[:, 0].double(), stamps[:, 1].double()
    ok = (w > 0) & (c > 0)
    if int(ok.sum()) == 0:
        return None, None
    return float((c[ok] / w[ok]).median()) * 100.0, float(w[ok].median()) * 0.01


def box_block(pkg, torch, dev, lib, step, sync_all, ms_per_step, block_args_ok):
    """`box`: (1) board power / cap / DPM clock sampled from sysfs while the SAME step loop keeps running for ~1 s right after
    the timed region; (2) the clock the chip holds inside the block kernel's main loop (a diagnostic instantiation that stamps
    s_memtime / s_memrealtime around it: MI355X_MICROARCH.md 'DVFS give-back' (6)); (3) a fixed MFMA-only calibration launch
    (csrc/calib.hip: exactly the main-loop matrix-pipe work of the block at config 2, no memory traffic), timed and stamped."""
    from ed_gated_gcn_amd import _capi
    box = {}
    try:
        with PowerSampler() as ps:
            t_end = time.perf_counter() + 1.0
            n_load = 0
            while time.perf_counter() < t_end:
                for _ in range(50):
                    step()
                n_load += 50
                sync_all()
        box.update(ps.summary())
        box["power_sampled"] = "sysfs, every ~20 ms for ~1 s while %d more untimed steps of the same loop ran, right after the timed region" % n_load
    except Exception as e:   # noqa: BLE001 -- diagnostics must not cost the headline
        box["power_error"] = "%s: %s" % (type(e).__name__, str(e)[:160])
    st = _capi.stream_of(dev)
    # (2) the block kernel's own main loop, stamped
    if block_args_ok:
        try:
            n_wg_max = 1 << 16
            stamps = torch.zeros(n_wg_max, 2, dtype=torch.int64, device=dev)
            plain = lib.ggcn_block_fused

            def stamped(*a):
                return lib.ggcn_debug_block_fused_stamped(*a[:-1], _capi.ptr(stamps), a[-1])
            lib.ggcn_block_fused = stamped
            try:
                ev = []
                for i in range(60):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(); step(); e1.record()
                    ev.append((e0, e1))
                torch.cuda.synchronize(dev)
            finally:
                lib.ggcn_block_fused = plain
            live = stamps[stamps[:, 1] > 0]
            mhz, loop_us = clock_from_stamps(live)
            box.update({"clock_under_load_mhz": mhz, "block_mainloop_us_per_workgroup": loop_us,
                        "block_workgroups_stamped": int(live.shape[0]),
                        "stamped_step_us": statistics.median(a.elapsed_time(b) * 1e3 for a, b in ev[20:]),
                        "clock_note": "median over the workgroups of the LAST of 60 stamped block launches of d(s_memtime)/d(s_memrealtime) x 100 MHz "
                                      "around the main loop (diagnostic instantiation; the timed steps execute no stamp)"})
        except Exception as e:   # noqa: BLE001
            box["clock_error"] = "%s: %s" % (type(e).__name__, str(e)[:160])
    # (3) MFMA-only calibration: ~0.4 s of back-to-back launches, the last 100 timed by events
    try:
        n_wg, stages = 6144, 24
        cst = torch.zeros(n_wg, 2, dtype=torch.int64, device=dev)
        sink = torch.zeros(256, device=dev)
        call = lambda: _capi.check(lib.ggcn_debug_mfma_calibrate(n_wg, stages, _capi.ptr(cst), _capi.ptr(sink), st), "mfma_calibrate")  # noqa: E731
        with PowerSampler() as ps2:   # what the matrix pipes alone draw: ~0.35 s of back-to-back calibration launches
            for _ in range(1000):
                call()
            torch.cuda.synchronize(dev)
        pw = ps2.summary()
        ev = []
        for _ in range(100):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); call(); e1.record()
            ev.append((e0, e1))
        torch.cuda.synchronize(dev)
        us = statistics.median(a.elapsed_time(b) * 1e3 for a, b in ev)
        mhz, loop_us = clock_from_stamps(cst)
        # 6144 workgroups x 4 wavefronts x 24 stages x (16 fp16 + 8 fp8-MX MFMAs of 32x32) = the block's main-loop MFMAs:
        # 2 parts x 2*N*K*F algorithmic flops at 128 matrix-pipe cycles per 32^3 block
        box.update({"mfma_calib_us": us, "mfma_calib_clock_mhz": mhz, "mfma_calib_loop_us_per_workgroup": loop_us,
                    "mfma_calib_power_w": pw.get("power_w"),
                    "mfma_calib_ref_us": MFMA_CALIB_REF_US,
                    "mfma_calib_note": "ggcn_debug_mfma_calibrate(6144 workgroups, 24 stages): the block kernel's main-loop MFMAs at config 2 on random "
                                       "register operands, no memory / LDS traffic, two workgroups per CU; median of 100 launches by HIP events behind 1000 "
                                       "untimed ones; at the nominal 2.4 GHz it would take %.0f us" % (6144 * 4 * 24 * 1024 / 1024 / 2.4e3 / 1.0)})
        box["headline_at_calib_ms"] = ms_per_step * MFMA_CALIB_REF_US / us
        box["headline_at_calib_note"] = ("ms_per_step x mfma_calib_ref_us / mfma_calib_us: the raw figure rescaled to a box whose MFMA calibration "
                                         "equals the reference of profiles/r05_box_calibration.json; a reading aid, never `value`")
    except Exception as e:   # noqa: BLE001
        box["calib_error"] = "%s: %s" % (type(e).__name__, str(e)[:160])
    return box


def main():
    args = parse()
    if args.gpus > 1 and int(os.environ.get("WORLD_SIZE", "1")) == 1 and "RANK" not in os.environ:
        sys.exit(self_launch(args))
    # dmabuf IPC (RCCL needs it on this driver): read by the HSA runtime when it initialises, so it is set before torch is even
    # imported -- a rank started by an outer torch.distributed.run inherits the launcher's environment or gets it here
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import numpy as np
    import torch
    import torch.distributed as dist

    import ed_gated_gcn_amd as pkg
    from ed_gated_gcn_amd import _capi, shard, synth

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d: start this script plainly (it launches its own ranks) or through "
                         "torch.distributed.run with --nproc-per-node %d" % (args.gpus, world, args.gpus))
    assert torch.cuda.is_available(), "bench.py needs an MI355X (no CPU fallback exists)"
    dev = torch.device("cuda", 0 if args.same_device else local)
    torch.cuda.set_device(dev)
    # the distributed branch: every N > 1 run, and N = 1 on request (--force-dist: the same loop with a process group of one)
    dist_on = world > 1 or args.force_dist
    if dist_on:
        if "MASTER_ADDR" not in os.environ:   # a plain `python bench.py --gpus 1 --force-dist`: rendezvous with ourselves
            import socket
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                port = sk.getsockname()[1]
            os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(args.master_port or port), "RANK": "0",
                               "WORLD_SIZE": "1", "LOCAL_RANK": "0"})
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(args.backend)

    lib = pkg.load_library()
    one_layer = args.config == 4
    half = args.config == 4
    T, H = args.tokens, args.hidden

    # ---- the batch, generated identically on every rank; this rank's shard goes to HBM ----
    if args.scaling == "strong":
        B_total = args.graphs
        if B_total < world:
            raise SystemExit("cannot shard %d graphs over %d GPUs" % (B_total, world))
        adj_all = synth.dependency_batch(B_total, T, args.degree, seed=synth.SEED)
        parts = shard.partition_graphs(adj_all.reshape(B_total, -1).sum(1, dtype=np.int64), world)
        lo, hi = parts[rank]
        counts = [h - l for l, h in parts]
        seed_x = synth.SEED
    else:
        B_total = args.graphs * world
        adj_all = synth.dependency_batch(args.graphs, T, args.degree, seed=synth.SEED + rank)
        lo, hi = 0, args.graphs
        counts = [args.graphs] * world
        seed_x = synth.SEED + rank
    B = hi - lo
    adj_np = adj_all[lo:hi]
    rowptr, colidx, _ = synth.csr_from_dense_host(adj_np)
    nnz = int(rowptr[-1])
    csr = pkg.BatchedCSR.from_arrays(rowptr, colidx, B, T, dev)
    gen = torch.Generator().manual_seed(seed_x)
    nb = adj_all.shape[0]
    x_all = torch.randn(nb, T, H, generator=gen)
    g1_all = torch.sigmoid(torch.randn(nb, H, generator=gen))
    g2_all = torch.sigmoid(torch.randn(nb, H, generator=gen))
    x_cpu, g1_cpu, g2_cpu = x_all[lo:hi], g1_all[lo:hi], g2_all[lo:hi]
    if half:
        x_cpu = x_cpu.half()
    w1, b1 = synth.layer_params(H, H, seed=1)
    w2, b2 = synth.layer_params(H, H, seed=2)
    x, g1, g2 = x_cpu.to(dev), g1_cpu.to(dev), g2_cpu.to(dev)
    layers = []
    for w, b in ((w1, b1), (w2, b2)):
        m = pkg.GraphConvolution(H, H, opt=None).to(dev)
        with torch.no_grad():
            m.weight.copy_(torch.from_numpy(w))
            m.bias.copy_(torch.from_numpy(b))
        layers.append(m.eval())
    gc1, gc2 = layers

    def set_mode(precision, path):
        for m in layers:
            m.precision = precision
            m.fused = path != "unfused"

    # N > 1: the payload of the path's only collective.  "logits": this rank's [B_r, 34] = out . Wd, the share of the
    # classifier's dense layer that depends on the block's output (bert_amir5.py:643; 34 = ACE's classes, constant.py:266);
    # a replicated synthetic Wd, one small GEMM per step inside the timed region.  "pooled": out [B_r, H] itself.
    N_CLASS = 34
    head = None
    if dist_on and args.gather == "logits":
        head = (torch.randn(H, N_CLASS, generator=torch.Generator().manual_seed(7)) / H ** 0.5).to(dev)

    # --gather-mode flag: the head launch counts itself done in these two words (ggcn_dense_head_signal); the collective's side
    # stream is gated on the count instead of on an event of the replay stream
    flag_mode = (dist_on and args.gather_mode == "flag" and head is not None and not one_layer and args.backend == "nccl")
    signal = torch.zeros(2, dtype=torch.int32, device=dev) if flag_mode else None
    launched = [0]   # flag hand-off: head launches counted on the host (= the value signal[1] reaches with the newest one)

    def forward(xx=None, cc=None, a1=None, a2=None, path=None):
        """One pass of the hot path; returns the dict of outputs (config 4: one gated layer)."""
        xx, cc = (x if xx is None else xx), (csr if cc is None else cc)
        a1, a2 = (g1 if a1 is None else a1), (g2 if a2 is None else a2)
        if one_layer:
            _, pa, pb = gc1.forward_gated(xx, cc, pool_gate_a=a1, pool_gate_b=a2, want_out=True,
                                          want_pool_a=True, want_pool_b=True)
            r = {"x1": pa, "y1": pb, "out": pa}
            if head is not None:
                r["payload"] = pkg.dense_head(r["out"], head)
        else:
            # N > 1: the logits head rides in the launch that finishes xy (ggcn_dense_head): block + head = two launches per step
            r = pkg.gated_gcn_block(xx, cc, a1, a2, gc1, gc2, one_launch=((path or args.path) == "block"),
                                    dense_head=None if head is None else ((head, None, signal) if flag_mode else (head, None)))
            if head is not None:
                r["payload"] = r["logits"]
            if flag_mode and not torch.cuda.is_current_stream_capturing():
                launched[0] += 1   # a head launch that counts itself in signal[1] (a capture launches nothing; a replay counts in step())
        return r

    # the path's only collective: all-gather of the per-shard logits [B_r, 34] (or pooled outputs [B_r, H]), launched
    # asynchronously so step i's gather (RCCL's stream, xGMI) overlaps step i+1's kernels
    gather = shard.PooledGather(counts, N_CLASS if head is not None else H, dev) if dist_on else None
    in_graph = dist_on and args.gather_mode == "graph"
    if in_graph and len(set(counts)) != 1:
        raise SystemExit("--gather-mode graph needs equal shards (%s); use the default async mode" % counts)
    gbufs = [torch.empty(world * B, N_CLASS if head is not None else H, device=dev) for _ in range(2)] if in_graph else None
    pending = []
    capture = args.capture == "on" or (args.capture == "auto" and dist_on)
    set_mode(args.precision, args.path)
    graphs = None
    capture_note = None
    if capture:
        try:
            if in_graph:   # RCCL's communicator must exist before a capture may contain a collective: one eager all-gather first
                with torch.no_grad():
                    r0 = forward()
                    dist.all_gather_into_tensor(gbufs[0], (r0["payload"] if head is not None else r0["out"]).contiguous())
                torch.cuda.synchronize(dev)
            graphs = capture_steps(torch, dev, forward, (lambda r, k: dist.all_gather_into_tensor(
                gbufs[k], (r["payload"] if head is not None else r["out"]).contiguous())) if in_graph else None)
        except Exception as e:   # noqa: BLE001 -- a refused capture must not cost the run: eager launches instead
            graphs, capture_note = None, "hipGraph capture refused (%s: %s); eager launches" % (type(e).__name__, str(e)[:200])
            torch.cuda.synchronize(dev)
    counter = [0]
    last_gathered = [None]   # what the most recently finished all-gather delivered (--check-gather)

    def step():
        with torch.no_grad():
            # step i-2's gather read the output buffer this step's replay is about to overwrite (graph copy i % 2) and
            # holds the gather slot this step will reuse: finish it FIRST (it was launched two steps ago)
            while len(pending) > 1:
                last_gathered[0] = gather.finish(pending.pop(0))
            if graphs is None:
                r = forward()
            else:
                g, r = graphs[counter[0] & 1]
                g.replay()
            counter[0] += 1
            if in_graph and graphs is not None:
                last_gathered[0] = gbufs[(counter[0] - 1) & 1]   # (filled by the replay; read after a synchronisation only)
            elif dist_on:
                if graphs is not None:
                    launched[0] += 1   # (the replay's head launch)
                pending.append(gather.start(r["payload"] if head is not None else r["out"],
                                            gate=(signal, launched[0]) if flag_mode else None))
        return r

    def sync_all():
        while pending:
            last_gathered[0] = gather.finish(pending.pop(0))
        torch.cuda.synchronize(dev)
        if flag_mode:   # (everything has finished: the host's count is re-read from the device, whoever launched heads meanwhile)
            launched[0] = int(signal[1].item())
        if dist_on:
            dist.barrier()
            torch.cuda.synchronize(dev)

    # ---- events and hooks of the timed region, made BEFORE any step runs (round 5): creating and pre-recording them idles the
    # GPU for milliseconds, and the chip needs tens of steps to ramp back (the driver's `--warmup 5` used to put that ramp inside
    # the timed region: 950, 839, 792 ... 679 us per step, profiles/r05_driver_cmd_before.txt).  From here on preconditioning,
    # the W warm-up steps and the K timed steps follow each other with nothing but the contract's barrier + synchronize between.
    # ---- timed region: EXACTLY K steps, barrier + synchronize on both sides.  HIP events on the launch stream
    # (torch's current stream IS the stream every ggcn_* call is enqueued on) bracket every step and, in eager
    # mode, the launches of the dominant kernel (ggcn_block_fused / ggcn_layer_fused* / ggcn_linear*) on every 4th step.
    # The event objects are created AND recorded once before the timed region: the first record of an event
    # creates the underlying hipEvent, which costs the host tens of microseconds -- enough to leave the GPU idle
    # between the short steps of a small shard.
    def make_events(n):
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(n)]
        for e in evs:
            e.record()
        return evs
    # An event record is a barrier packet on the stream (~2-3 us of GPU time each): with a short step (a small
    # shard) only every 4th step carries the per-launch events and the step events bracket 4 steps at a time.
    k_stride = 4          # the per-launch events of the dominant kernel ride on every 4th step (two barrier packets each)
    kernel_events = {}
    kernel_pool = make_events(8 * (args.steps // k_stride + 1)) if graphs is None else []
    sampling = [False]

    def with_events(name):
        fn = getattr(lib, name)

        def wrapped(*a):
            if not sampling[0]:
                return fn(*a)
            e0, e1 = kernel_pool.pop(), kernel_pool.pop()
            e0.record()
            rc = fn(*a)
            e1.record()
            kernel_events.setdefault(name, []).append((e0, e1))
            return rc
        return fn, wrapped
    hooked = {}
    step_pool = make_events(args.steps + 1)
    torch.cuda.synchronize(dev)
    if graphs is None:
        for name in ("ggcn_block_fused", "ggcn_layer_fused", "ggcn_layer_fused_h", "ggcn_linear", "ggcn_linear_h",
                     "ggcn_aggregate", "ggcn_aggregate_h"):
            hooked[name], w = with_events(name)
            setattr(lib, name, w)
    last = None
    n_pre = args.precondition
    if n_pre < 0:   # adaptive: run until the step time has settled (same count on every rank: rank 0 decides)
        n_pre, last = 0, None
        while n_pre < 2000:
            sync_all()
            t0 = time.perf_counter()
            for _ in range(50):
                step()
            sync_all()
            dt = time.perf_counter() - t0
            n_pre += 50
            settled = last is not None and abs(dt - last) <= 0.01 * dt and n_pre >= 150
            if dist_on:
                flag = torch.tensor([1 if settled else 0], device=dev)
                dist.broadcast(flag, src=0)
                settled = bool(flag.item())
            last = dt
            if settled:
                break
    else:
        for _ in range(n_pre):
            step()
    sparse = last is not None and (last / 50) < 300e-6 if args.precondition < 0 else dist_on
    ev_stride = 4 if sparse else 1
    # The W warm-up steps of the contract: they end in the state the timed region starts from.  Between them and t0 there is
    # only the barrier + synchronize the contract asks for (GGCN_BENCH_SERIES=1 prints the per-step series).
    for _ in range(args.warmup):
        step()
    sync_all()
    t0 = time.perf_counter()
    step_pool[0].record()
    marks = [0]
    for i in range(args.steps):
        sampling[0] = (i % k_stride) == 0
        r_last = step()
        if (i + 1) % ev_stride == 0 or i + 1 == args.steps:
            step_pool[i + 1].record()
            marks.append(i + 1)
    sampling[0] = False
    sync_all()
    elapsed = time.perf_counter() - t0
    for name, fn in hooked.items():
        setattr(lib, name, fn)
    # per-step time of every bracketed group of steps (1 step, or ev_stride steps averaged)
    step_events = [(step_pool[a], step_pool[b], b - a) for a, b in zip(marks[:-1], marks[1:])]
    step_us = [a.elapsed_time(b) * 1e3 / n for a, b, n in step_events]
    if os.environ.get("GGCN_BENCH_SERIES") and rank == 0:   # development aid: where the slow steps sit
        print("step_us series:", " ".join("%.0f" % v for v in step_us), file=sys.stderr)
    kern_us = {k: [a.elapsed_time(b) * 1e3 for a, b in v] for k, v in kernel_events.items()}
    if dist_on:
        tt = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
        nn = torch.tensor([nnz], device=dev, dtype=torch.int64)
        dist.all_reduce(nn)
        nnz_total = int(nn.item())
    else:
        nnz_total = nnz
    ms_per_step = elapsed / args.steps * 1e3
    # ---- what the last timed step computed, before anything else runs a step (graph replay reuses its output buffers) ----
    dumped = None
    if args.dump_outputs and rank == 0:
        outs = {k: v for k, v in r_last.items() if not k.startswith("_") and not (k == "payload" and "logits" in r_last)}
        if dist_on and last_gathered[0] is not None:
            outs["gathered"] = last_gathered[0]
        dumped = {"dir": args.dump_outputs, "outputs": dump_outputs(args.dump_outputs, outs),
                  "note": "the last timed step's outputs (rank 0); an output over its share of %d MiB holds the rows a fixed seed "
                          "picks" % (DUMP_BUDGET_BYTES >> 20)}

    # ---- N > 1: what the collective moved, and (on request) the gathered payload against the unsharded batch ----
    rccl = gather_check = None
    if dist_on:
        width = N_CLASS if head is not None else H
        rccl = {"backend": dist.get_backend(), "world_size_seen": dist.get_world_size(),
                "gather_bytes_per_rank": int(max(counts)) * width * 4,
                "gather_bytes_total_per_step": int(max(counts)) * width * 4 * world,
                "payload": "logits [B_r,%d]" % N_CLASS if head is not None else "pooled out [B_r,%d]" % H,
                "collective": ("all_gather_into_tensor captured inside the step's hipGraph, one per step" if in_graph and graphs is not None else
                               "all_gather_into_tensor, eager, one per step, issued from a side stream held by hipStreamWaitValue32 until the "
                               "step's head launch has counted itself done (ggcn_dense_head_signal): no event on the replay stream" if flag_mode else
                               "all_gather_into_tensor, async, one per step; shards padded to the largest B_r"),
                "gather_mode": "graph" if in_graph and graphs is not None else "flag" if flag_mode else "async"}
        if args.check_gather and args.scaling == "strong":
            got = last_gathered[0]
            if rank == 0:   # the whole batch on rank 0's GPU, one shard-sized GEMM per rank (same kernels as the ranks ran)
                rp_a, ci_a, _ = synth.csr_from_dense_host(adj_all)
                csr_a = pkg.BatchedCSR.from_arrays(rp_a, ci_a, B_total, T, dev)
                with torch.no_grad():
                    full = pkg.gated_gcn_block(x_all.to(dev), csr_a, g1_all.to(dev), g2_all.to(dev), gc1, gc2,
                                               one_launch=(args.path == "block"))["out"]
                    want = torch.cat([pkg.dense_head(full[l:h], head) if head is not None else full[l:h] for l, h in parts], 0)
                diff = float((got.float() - want).abs().max()) if got is not None else float("nan")
                gather_check = {"bitwise_equal": bool(got is not None and torch.equal(got, want)), "max_abs_diff": diff,
                                "rows": int(want.shape[0]),
                                "against": "the unsharded %d-graph batch through the same path on rank 0's GPU" % B_total}

    # ---- roofline of the dominant kernel (this rank's shard) ----
    N = B * T
    s_el = 2 if half else 4
    layer_bytes = synth.algorithmic_bytes_per_layer(B, T, H, nnz, n_gates=1, s=s_el)   # SURVEY 8d formula
    n_layers = 1 if one_layer else 2
    fwd_bytes = n_layers * layer_bytes
    lin_flops = 2.0 * N * H * H                       # algorithmic flops of gcn.py:34 per layer
    agg_flops = 2.0 * nnz * H                         # gcn.py:41 on the non-zeros
    lin_peak = MFMA_F32_PEAK_TF if args.precision == "fp32" else MFMA_BF16_PEAK_TF
    tpath = os.path.join(ROOT, "profiles", "traffic.json")   # PMC-measured HBM bytes per launch, recorded separately
    measured = json.load(open(tpath)) if os.path.exists(tpath) else {}
    traffic_note = ("traffic = HBM bytes per launch (FETCH_SIZE x2 + WRITE_SIZE, rocprofv3 --pmc, separate passes) "
                    "recorded in profiles/traffic.json for this kernel and workload; a constant of that profile run, "
                    "not re-measured by this run")
    kernels = {}
    for k, v in kern_us.items():
        kernels[k] = dict(percentiles(v), unit="us", launches_timed=len(v),
                          launches_per_step=len(v) / len(range(0, args.steps, k_stride)))
    if not kern_us:       # hipGraph replay: the per-launch events cannot be recorded; time the kernels once, eagerly
        pass

    def mfma_line(kernel, key, t_us, flops, nbytes, launches_note):
        tf = flops / (t_us * 1e-6) / 1e12
        return {"kernel": kernel, "bound": "mfma", "achieved": tf, "peak": lin_peak, "unit": "TFLOP/s",
                "frac": tf / lin_peak, "traffic": measured.get(key), "avg_launch_us": t_us,
                "algorithmic_flops_per_launch": flops, "algorithmic_bytes_per_launch": nbytes,
                "hbm_GBps": nbytes / (t_us * 1e-6) / 1e9, "hbm_frac": nbytes / (t_us * 1e-6) / 1e9 / HBM_PEAK_GBS,
                "note": launches_note + "; achieved = algorithmic flops / launch; " + ISSUE_NOTE[args.precision]
                        + "; " + traffic_note}

    roofline = None
    if "ggcn_block_fused" in kern_us:
        t = statistics.mean(kern_us["ggcn_block_fused"])
        # (ggcn_block_fused runs batches of >= 2048 graphs on the eight-wavefront workgroup that stages a row block's X planes once
        # for a W1 and a W12 column slice -- fused_block8.hip; GGCN_BLOCK_FORM=4 keeps the four-wavefront kernel)
        form8 = args.precision == "f16mx8" and lib.ggcn_block_fused_form(B, T, H, H) == 8
        roofline = mfma_line("block_fused8_kernel (both layers of the block in one launch; eight wavefronts share a row block's X planes)" if form8 else
                             "layer_fused_kernel (block form: both layers of the block in one launch)",
                             ("block_fused8_kernel:" if form8 else "block_fused_kernel:") + args.precision, t, 2 * (lin_flops + agg_flops), fwd_bytes,
                             "one launch per step = 2 layers: 2 x (2*N*K*F + 2*nnz*F) flops, 2 x SURVEY 8(d) bytes")
        # what THIS kernel has to move: X in, x out, three pools, two gates, the graphs' operand blocks and the two packed
        # weight images -- SURVEY 8(d)'s figure still holds gcn1's write + read (2 x N*H*4), which the folded block never makes
        own = N * H * 4 * 2 + 5 * B * H * 4 + B * 2176 + 2 * (H // 32) * (H // 32) * 3328
        roofline["kernel_bytes_per_launch"] = own
        if roofline.get("traffic"):
            roofline["traffic_over_kernel_bytes"] = roofline["traffic"] / own
        roofline["note"] += ("; compare `traffic` with kernel_bytes_per_launch (X + x + pools + gates + operand blocks + W: what "
                             "the one-launch block must move), not with algorithmic_bytes_per_launch: the excess is X read "
                             + ("by three column slices through a 4 MiB L2 that also holds both weight images" if form8 else
                                "by both XCD groups and by three column tiles each through 4 MiB L2s"))
    elif "ggcn_layer_fused_h" in kern_us:
        t = statistics.mean(kern_us["ggcn_layer_fused_h"])
        roofline = mfma_line("layer_fused_long_kernel (fp16 linear + LDS neighbour sums, one launch per layer)",
                             "layer_fused_long_kernel:" + args.precision, t, lin_flops + agg_flops, layer_bytes,
                             "one launch per layer")
    elif "ggcn_layer_fused" in kern_us:
        t = statistics.mean(kern_us["ggcn_layer_fused"])
        roofline = mfma_line("layer_fused_kernel", "layer_fused_kernel:" + args.precision, t, lin_flops + agg_flops,
                             layer_bytes, "one launch per layer")
    else:
        lin_key = "ggcn_linear_h" if "ggcn_linear_h" in kern_us else "ggcn_linear"
        agg_key = "ggcn_aggregate_h" if "ggcn_aggregate_h" in kern_us else "ggcn_aggregate"
        if lin_key in kern_us and agg_key in kern_us:
            t_lin, t_agg = statistics.mean(kern_us[lin_key]), statistics.mean(kern_us[agg_key])
            if t_lin >= t_agg:
                roofline = mfma_line("linear_fp32_kernel" if args.precision == "fp32" else
                                     "linear_f16_kernel" if args.precision == "f16" else
                                     "linear_split_kernel (%s)" % args.precision,
                                     "linear_split_kernel:" + args.precision, t_lin, lin_flops,
                                     2 * s_el * N * H + 4 * H * H, "the dense linear of one layer")
            else:
                agg_bytes = layer_bytes - 4 * H * H
                gbs = agg_bytes / (t_agg * 1e-6) / 1e9
                roofline = {"kernel": "aggregate_rows", "bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS,
                            "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS, "traffic": measured.get("aggregate_rows"),
                            "avg_launch_us": t_agg, "algorithmic_bytes_per_launch": agg_bytes, "note": traffic_note}
    if roofline is None:   # captured replay: whole-step figure from the per-step events
        t = statistics.mean(step_us)
        roofline = mfma_line("hipGraph replay of the step (%s path)" % args.path, "none", t,
                             n_layers * (lin_flops + agg_flops), fwd_bytes,
                             "per-launch events are not available under graph replay: whole step of this rank's shard")

    # ---- the state of this box, probed right after the timed region (N = 1; diagnostics, see box_block) ----
    box = None
    if world == 1 and not dist_on and not args.no_box:
        box = box_block(pkg, torch, dev, lib, step, sync_all, ms_per_step,
                        block_args_ok=(args.config == 2 and args.path == "block" and args.precision == "f16mx8" and graphs is None
                                       and T == 32 and B % 4 == 0 and H % 32 == 0))

    # ---- other precisions on the same inputs + accuracy of each against float64 (rank 0's shard) ----
    alt = None
    if not args.no_alt:
        alt = {}
        ns = min(64, B) if not one_layer else min(4, B)
        sub_adj = torch.from_numpy(adj_np[:ns])
        rp_s, ci_s, _ = synth.csr_from_dense_host(adj_np[:ns])
        csr_s = pkg.BatchedCSR.from_arrays(rp_s, ci_s, ns, T, dev)
        t_ = torch.from_numpy
        ref64 = block_float64(x_cpu[:ns].float(), sub_adj, g1_cpu[:ns], g2_cpu[:ns], t_(w1), t_(b1), t_(w2), t_(b2),
                              one_layer)
        xs, g1s, g2s = x[:ns].contiguous(), g1[:ns].contiguous(), g2[:ns].contiguous()
        precs = ["f16", "f16mx8", "bf16x3"] if half else (["f16mx8"] + (["f16mx6"] if _capi.has_f16mx6() else []) + ["bf16x3", "fp32"])
        for prec in precs:
            set_mode(prec, args.path)
            with torch.no_grad():
                rs = forward(xs, csr_s, g1s, g2s)
                err = max(float((rs[k].double().cpu() - ref64[k]).abs().max()) for k in ref64)
                n_alt = 10 if prec == "fp32" else 30
                for _ in range(20 if prec == "fp32" else 80):   # the chip has just idled through the float64 yardstick: ~50 ms of load settle it
                    forward()
                torch.cuda.synchronize(dev)
                ev = []
                for _ in range(n_alt):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    forward()
                    e1.record()
                    ev.append((e0, e1))
                torch.cuda.synchronize(dev)
            ms = statistics.median(a.elapsed_time(b) for a, b in ev)
            alt[prec] = {"ms_per_step": ms, "edges_per_sec": nnz / (ms * 1e-3), "max_abs_err_vs_float64": err,
                         "steps": n_alt, "timed": "median of per-step HIP events, eager, this rank's shard"}
        set_mode(args.precision, args.path)

    result = None
    if rank == 0:
        value = nnz_total * args.steps / elapsed
        per_step = percentiles(step_us)
        workload = ("BASELINE.json configs[1]%s: %d graphs x %d tokens, avg degree %g (nnz %d incl. self loops), "
                    "hidden %d, 2 gated-GCN layers, fp32 in/out" % (" sharded = configs[2]" if world > 1 and
                    args.scaling == "strong" else "", B_total, T, args.degree, nnz_total, H)) if not one_layer else \
                   ("BASELINE.json configs[3]: %d graphs x %d tokens, avg degree %g (nnz %d incl. self loops), hidden %d, "
                    "fp16 features (fp32 accumulate), 1 gated-GCN layer with both gates and pools" %
                    (B_total, T, args.degree, nnz_total, H))
        path_note = {"block": "one launch for the block (ggcn_block_fused) + a 1-workgroup reduce for xy",
                     "layers": "one launch per layer (ggcn_layer_fused)",
                     "unfused": "linear + aggregate (2 launches per layer)"}[args.path]
        if one_layer:
            path_note = ("one launch per layer (ggcn_layer_fused_h: fp16 linear + neighbour sums out of an LDS tile)"
                         if "ggcn_layer_fused_h" in kern_us else "linear + aggregate (2 launches per layer)")
        elif not (gc1.fused and args.precision != "fp32" and csr.rowmask is not None):
            path_note = "linear + aggregate (2 launches per layer)"
        total_fwd_bytes = (2 * SURVEY_8D_BYTES_PER_LAYER if (args.config == 2 and B_total == 4096 and T == 32 and H == 768
                                                              and nnz_total == 524288) else
                           n_layers * synth.algorithmic_bytes_per_layer(B_total, T, H, nnz_total, n_gates=1, s=s_el))
        result = {
            "metric": "gated_gcn_forward_edges_per_sec", "value": value, "unit": "edges/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step,
            "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
            "dtype": DTYPE_NOTE[args.precision] if not half else
                     "f16 features, " + DTYPE_NOTE[args.precision].split("(")[-1].rstrip(")"),
            "data": "synthetic",
            "config": {"workload": workload, "graphs_total": B_total, "graphs_per_gpu": counts,
                       "precision": args.precision, "path": path_note, "hipgraph_replay": bool(graphs), "capture_note": capture_note,
                       "precondition_steps": n_pre,
                       "collective": ("none" if world == 1 else
                                      "all_gather(logits[B_r,%d] = out[B_r,H] . Wd) per step, async (RCCL)" % N_CLASS if head is not None
                                      else "all_gather(out[B_r,H]) per step, async (RCCL)")},
            "step_us": dict(per_step, events_every_n_steps=ev_stride,
                            note="HIP events on the launch stream of rank 0 bracketing every step (or every 4 steps, "
                                 "averaged, when a step is short); median, p10, p90 over the K timed steps; "
                                 "ms_per_step is wall time / K, max over ranks"),
            "edge_layers_per_sec": n_layers * value,
            "forward_algorithmic_bytes": total_fwd_bytes,
            "forward_hbm_GBps": total_fwd_bytes / (elapsed / args.steps) / 1e9,
            "forward_hbm_frac": total_fwd_bytes / (elapsed / args.steps) / 1e9 / (HBM_PEAK_GBS * world),
            "roofline": roofline,
            "kernels": kernels,
        }
        if dumped is not None:
            result["dump"] = dumped
        if box is not None:
            result["box"] = box
        if rccl is not None:
            result["rccl"] = rccl
        if gather_check is not None:
            result["gather_check"] = gather_check
        if alt is not None:
            result["alt_precisions"] = alt
            if not one_layer:   # what a drop-in user gets without opting in: the module's default arithmetic
                dflt = pkg.GraphConvolution(8, 8, opt=None).precision
                result["product_default"] = dict(alt.get(dflt, {}), precision=dflt,
                                                 forward_hbm_frac=(total_fwd_bytes / (alt[dflt]["ms_per_step"] * 1e-3) / 1e9 / HBM_PEAK_GBS
                                                                   if dflt in alt else None),
                                                 headline_precision_is_opt_in=(args.precision != dflt),
                                                 note="GraphConvolution's default arithmetic is %s: inside the 1e-4 gate for |x| <= 448 and hidden "
                                                      "values < 65504, both watched by a sticky device flag in the kernels and reported "
                                                      "lazily (range_guard: overflow / accuracy window / hidden bound); bf16x3 keeps "
                                                      "the whole fp32 exponent range (opt.ggcn_precision / GGCN_PRECISION / "
                                                      "module.precision); this run's headline precision: %s" % (dflt, args.precision))
            result["max_abs_err"] = {"precision": args.precision, "value": alt[args.precision]["max_abs_err_vs_float64"],
                                     "against": "float64 evaluation of the reference formulas on the first %d graphs of the "
                                                "timed inputs (x1, y1, x, out); parity gate %s" %
                                                ((min(64, B), "1e-4 (fp32, north_star)") if not one_layer else
                                                 (min(4, B), "2e-3 (fp16 features, SURVEY 8d)"))}
        if not args.no_cpu_baseline and world == 1:   # rank 0 at N=1 only: other ranks would idle at the barrier
            t_ = torch.from_numpy
            result["cpu_baseline"] = cpu_baseline(x_cpu, t_(adj_np), g1_cpu, g2_cpu, t_(w1), t_(b1), t_(w2), t_(b2),
                                                  args.cpu_graphs, one_layer)
            result["gpu_over_cpu"] = value / result["cpu_baseline"]["value"]
        if world == 1 and args.config == 2 and not args.no_config4:
            if args.path == "block" and not one_layer:
                result["eval_logits_only"] = eval_block(pkg, torch, dev, x, csr, g1, g2, gc1, gc2)
            result["ace_cased"] = ace_block(pkg, synth, torch, dev, args.precision if args.precision in ("bf16x3", "f16mx8") else "f16mx8")
            result["config4"] = config4_block()
            result["scaling_ceiling"] = shard512_block(ms_per_step)
        print(json.dumps(result), flush=True)
    if dist_on:
        dist.barrier()
        dist.destroy_process_group()
    return result


if __name__ == "__main__":
    main()
