#!/usr/bin/env python3
"""FusedAdam.step() against torch.optim.Adam(fused=True).step() on the parameter sets of tacos.yml, charadessta.yml and activitynet_t256
with random gradients, in one process: after a warm-up of both, alternating blocks of the two, every call between two HIP events; the
whole measurement twice.  The clipped variant puts ``max_norm=1.0`` on our side and a preceding ``clip_grad_norm_`` on torch's.
    python tools/optimizer_bench.py [--calls 200] [--warmup 20] [--block 20] [--workloads tacos,charadessta,activitynet_t256]
Prints one JSON line per (run, workload, variant): the median and the 10-90 % spread of each side in microseconds, tensors and
elements, the bytes one update streams per element (28: p, m, v read and written, g read; + 4 for the norm's pass over g) and our
launches per step.  For the kernels' own times run it under the profiler with few calls:
    rocprofv3 --kernel-trace --stats -d out -- python tools/optimizer_bench.py --calls 20 --warmup 2"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(v):
    q = statistics.quantiles(v, n=10)
    return {"median": round(statistics.median(v), 2), "p10": round(q[0], 2), "p90": round(q[-1], 2), "spread": round(q[-1] - q[0], 2)}


def measure(fns, calls, warmup, block):
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    pairs, done = [], 0
    while done < calls:
        n = min(block, calls - done)
        for name, fn in fns.items():
            for _ in range(n):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                pairs.append((name, e0, e1))
        done += n
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for name, e0, e1 in pairs:
        us[name].append(e0.elapsed_time(e1) * 1e3)
    return {k: summary(v) for k, v in us.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="tacos,charadessta,activitynet_t256")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--block", type=int, default=20)
    ap.add_argument("--runs", type=int, default=2)
    args = ap.parse_args()
    import bench
    import models
    A = models.vml_amd
    dev = torch.device("cuda:0")
    A._lib.load_torch()
    for run in range(args.runs):
        for wl in args.workloads.split(","):
            T, L, C, D, dl, layers, Din, Nq, Hh, _ = bench.WORKLOADS[wl]
            torch.manual_seed(43)
            shapes = [tuple(p.shape) for p in models.SMIN(T, L, C, D, dl, layers, Din, Nq, Hh).parameters()]
            for variant, max_norm in (("plain", None), ("clipped", 1.0)):
                g = torch.Generator().manual_seed(7)
                mk = lambda: [torch.nn.Parameter(torch.randn(s, generator=g).to(dev)) for s in shapes]
                p_o, p_t = mk(), mk()
                grads = [torch.randn(s, generator=g).to(dev) * 1e-2 for s in shapes]
                for ps in (p_o, p_t):
                    for p, gr in zip(ps, grads):
                        p.grad = gr.clone()
                ours = A.FusedAdam(p_o, lr=1e-3, max_norm=max_norm)
                theirs = torch.optim.Adam(p_t, lr=1e-3, fused=True)

                def torch_step():
                    if max_norm is not None:
                        torch.nn.utils.clip_grad_norm_(p_t, max_norm)
                    theirs.step()

                res = measure({"fused_adam": ours.step, "torch_fused": torch_step}, args.calls, args.warmup, args.block)
                numel = sum(p.numel() for p in p_o)
                print(json.dumps({"run": run, "workload": wl, "variant": variant, "tensors": len(shapes), "numel": numel, "us": res,
                                  "torch_minus_ours_us": round(res["torch_fused"]["median"] - res["fused_adam"]["median"], 2),
                                  "bytes_per_element": 28 if max_norm is None else 32, "our_launches": 2 if max_norm is None else 4,
                                  "our_GBps": round(numel * (28 if max_norm is None else 32) / res["fused_adam"]["median"] * 1e-3, 1)}), flush=True)


if __name__ == "__main__":
    main()
