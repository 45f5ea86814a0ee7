#!/usr/bin/env python3
"""SMIN.score against the forward under no_grad at the bench workload (activitynet_t256: B 64, T 256, L 64, Nq 20, 3 layers), in one
process: after a warm-up of both, alternating blocks of ``model(...)`` under no_grad and ``model.score(...)``, every call between two
HIP events.
    python tools/score_bench.py [--calls 200] [--warmup 10] [--block 20] [--workload activitynet_t256]
Prints one JSON line: the median and the 10-90 % spread of each in milliseconds, their difference, the peak of allocated memory over
one call of each, and the largest difference of the scores.  For the tail kernel's own time run it under the profiler with few calls:
    rocprofv3 --kernel-trace --stats -d out -- python tools/score_bench.py --calls 20 --warmup 2"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="activitynet_t256")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--block", type=int, default=20)
    args = ap.parse_args()
    import bench
    import models
    dev = torch.device("cuda:0")
    models.vml_amd._lib.load()
    T, L, C, D, dl, layers, Din, Nq, Hh, B = bench.WORKLOADS[args.workload]
    torch.manual_seed(43)
    model = models.SMIN(T, L, C, D, dl, layers, Din, Nq, Hh, dev).to(dev)
    b = bench.make_batch(B, T, L, Nq, Din, seed=1000, device=dev)
    inputs = [b[k] for k in ("video_features", "video_mask", "query_features", "query_mask", "length_mask", "moment_mask")]
    assert model._plan(inputs[0], inputs[2]) == "node"

    def forward():
        with torch.no_grad():
            return model(*inputs)

    fns = {"forward": forward, "score": lambda: model.score(*inputs)}
    for _ in range(args.warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    pairs = []
    done = 0
    while done < args.calls:
        n = min(args.block, args.calls - done)
        for name, fn in fns.items():
            for _ in range(n):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                pairs.append((name, e0, e1))
        done += n
    torch.cuda.synchronize()
    for name, e0, e1 in pairs:
        ms[name].append(e0.elapsed_time(e1))

    def summary(v):
        q = statistics.quantiles(v, n=10)
        return {"median": round(statistics.median(v), 4), "p10": round(q[0], 4), "p90": round(q[-1], 4), "spread": round(q[-1] - q[0], 4)}

    peaks = {}
    for name, fn in fns.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        out = fn()
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated(dev)
        del out
    f, s = fns["forward"](), fns["score"]()
    diff = [float((x - y).abs().max()) for x, y in zip(f, s)]
    res = {k: summary(v) for k, v in ms.items()}
    N = int(b["moment_mask"].sum())
    print(json.dumps({"workload": args.workload, "calls": args.calls, "cells": N, "ms": res,
                      "forward_minus_score_ms": round(res["forward"]["median"] - res["score"]["median"], 4),
                      "larger_spread_ms": max(res["forward"]["spread"], res["score"]["spread"]),
                      "peak_allocated_MB": {k: round(v / 2 ** 20, 1) for k, v in peaks.items()},
                      "tail_bytes_per_call": N * (dl + 3 * D) * 4, "max_abs_diff_pm_ps_pe_pa": diff, "gemm_mode": models.vml_amd.get_gemm_mode()}))


if __name__ == "__main__":
    main()
