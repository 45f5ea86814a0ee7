#!/usr/bin/env python3
"""Times Soft-NMS moment retrieval (csrc/soft_nms.hip) on the device, run by hand:
  (a) top:   top_moments(nms="linear") and top_moments(nms="gaussian", sigma=0.5) against two baselines on the same inputs:
             hard top_moments (greedy NMS at the same threshold) and top_moments_soft_torch on the device (torch ops driven by a
             Python loop that reads the host at every pick), at (B, L, k) = (64, 64, 5), (64, 64, 64), (16, 512, 5), (16, 512, 25).
             L = 64 is the one-launch path (cur in LDS), L = 512 the banded one (k + 1 launches).
  (b) merge: merge_window_moments(nms="linear") against hard merge_window_moments at (pairs, windows, k_window, k) = (128, 57, 5, 5).
    python tools/soft_nms_bench.py [--calls 50] [--warmup 5] [--block 10] [--torch-calls 3] [--runs 2] [--groups top64,top512,merge]
Every row group runs in a process of its own (a fresh child per group and run, one at a time).  Inside it: a warm-up of all device
sides, then alternating blocks; every timed call lies between two HIP events on the stream (host issue time is inside them: the banded
path is k + 1 launches, and that is part of its cost).  The torch side is timed apart, --torch-calls calls after one warm-up.  Before
timing, the linear lists are compared with the restatement bit for bit.  Prints one JSON line per shape and run: the median and the
10-90 % spread of each side in microseconds."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GROUPS = {"top64": [(64, 64, 5), (64, 64, 64)], "top512": [(16, 512, 5), (16, 512, 25)], "merge": [(128, 57, 5, 5)]}
THR, SIGMA = 0.5, 0.5


def summary(v):
    if len(v) < 2:
        return {"median": round(v[0], 2), "calls": len(v)}
    q = statistics.quantiles(v, n=10)
    return {"median": round(statistics.median(v), 2), "p10": round(q[0], 2), "p90": round(q[-1], 2), "spread": round(q[-1] - q[0], 2),
            "calls": len(v)}


def timed_blocks(sides, calls, warmup, block):
    """{side: [microseconds per call]}: a warm-up of every side, then alternating blocks, each call between two HIP events"""
    for _ in range(warmup):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    timed, done = [], 0
    while done < calls:
        n = min(block, calls - done)
        for side, fn in sides.items():
            for _ in range(n):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                timed.append((side, a, b))
        done += n
    torch.cuda.synchronize()
    us = {s: [] for s in sides}
    for side, a, b in timed:
        us[side].append(a.elapsed_time(b) * 1e3)
    return us


def same(a, b, keys):
    return all(torch.equal(a[key].cpu().contiguous().view(torch.uint8), b[key].cpu().contiguous().view(torch.uint8)) for key in keys)


def bench_top(A, args, dev, shapes):
    for B, L, k in shapes:
        g = torch.Generator().manual_seed(L + k)
        mm = torch.triu(torch.ones(L, L, dtype=torch.bool)).expand(B, L, L).contiguous()
        pm, ps, pe, mm = (x.to(dev) for x in (torch.rand(B, L, L, generator=g), torch.rand(B, L, generator=g), torch.rand(B, L, generator=g), mm))
        linear = lambda: A.top_moments(pm, ps, pe, mm, k=k, nms_thresh=THR, nms="linear")
        restated = lambda: A.top_moments_soft_torch(pm, ps, pe, mm, k=k, nms_thresh=THR, nms="linear")
        assert same(linear(), restated(), ("idx", "score", "raw_score", "count")), "top_moments(nms='linear') and its restatement disagree"
        sides = {"hard": lambda: A.top_moments(pm, ps, pe, mm, k=k, nms_thresh=THR), "linear": linear,
                 "gaussian": lambda: A.top_moments(pm, ps, pe, mm, k=k, nms="gaussian", sigma=SIGMA)}
        us = timed_blocks(sides, args.calls, args.warmup, args.block)
        us.update(timed_blocks({"soft_torch_on_device": restated}, args.torch_calls, 1, args.torch_calls))
        row = dict(figure="top_moments", B=B, L=L, k=k, nms_thresh=THR, sigma=SIGMA, unit="us", **{s: summary(v) for s, v in us.items()})
        row["linear_over_hard"] = round(row["linear"]["median"] / row["hard"]["median"], 2)
        row["torch_over_linear"] = round(row["soft_torch_on_device"]["median"] / row["linear"]["median"], 1)
        print(json.dumps(row), flush=True)


def bench_merge(A, args, dev, shapes):
    for pairs, windows, kw, k in shapes:
        T, L, G = 128, 64, pairs * windows
        g = torch.Generator().manual_seed(windows)
        i = torch.randint(0, L, (G, kw), generator=g)
        j = torch.minimum(i + torch.randint(0, L // 4, (G, kw), generator=g), torch.tensor(L - 1))
        cand = [torch.stack([i, j], -1), torch.rand(G, kw, generator=g), torch.full((G,), kw, dtype=torch.int32),
                (torch.arange(G) % windows) * (T // 2), torch.full((G,), T, dtype=torch.int32), torch.arange(pairs + 1) * windows]
        cand = [x.to(dev) for x in cand]
        linear = lambda: A.merge_window_moments(*cand, T, L, k=k, nms_thresh=THR, nms="linear")
        want = A.merge_window_moments_torch(*[x.cpu() for x in cand], T, L, k=k, nms_thresh=THR, nms="linear")
        got = {key: v.cpu() for key, v in linear().items()}
        assert same(got, want, ("span", "score", "raw_score", "window", "cell", "count")), "the soft merge and its restatement disagree"
        sides = {"hard": lambda: A.merge_window_moments(*cand, T, L, k=k, nms_thresh=THR), "linear": linear,
                 "gaussian": lambda: A.merge_window_moments(*cand, T, L, k=k, nms="gaussian", sigma=SIGMA)}
        us = timed_blocks(sides, args.calls, args.warmup, args.block)
        row = dict(figure="merge_window_moments", pairs=pairs, windows=windows, k_window=kw, k=k, nms_thresh=THR, sigma=SIGMA, unit="us",
                   **{s: summary(v) for s, v in us.items()})
        row["linear_over_hard"] = round(row["linear"]["median"] / row["hard"]["median"], 2)
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--torch-calls", type=int, default=3)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--groups", default="top64,top512,merge")
    ap.add_argument("--limit", type=int, default=240, help="seconds a row group's process may take")
    ap.add_argument("--group", default=None, help="(internal) measure this row group in this process")
    args = ap.parse_args()
    if args.group is None:                                       # the parent never opens the device: one fresh child per group and run
        for run in range(args.runs):
            for name in args.groups.split(","):
                cmd = [sys.executable, os.path.abspath(__file__), "--group", name, "--calls", str(args.calls), "--warmup", str(args.warmup),
                       "--block", str(args.block), "--torch-calls", str(args.torch_calls)]
                res = subprocess.run(cmd, timeout=args.limit)
                if res.returncode != 0:
                    sys.exit(f"soft_nms_bench: row group {name} ended with status {res.returncode}; nothing more is started")
        return
    import models
    assert torch.cuda.is_available(), "soft_nms_bench measures on a HIP device"
    dev = torch.device("cuda:0")
    (bench_merge if args.group == "merge" else bench_top)(models.vml_amd, args, dev, GROUPS[args.group])


if __name__ == "__main__":
    main()
