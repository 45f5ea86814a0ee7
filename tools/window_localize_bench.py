#!/usr/bin/env python3
"""Throughput of SMIN.localize_windows at the ActivityNet shape (T = 256, L = 64, D = 512, dl = 128, 3 layers):
one 2-hour video of 7 200 feature rows, 16 queries on it, default window (T rows) and stride (T / 2) -- 56 windows per query.
Prints one JSON line: windows per second of the whole call (planning, resampling, masks, forward, per-window top-k, merge) and
the merge kernel's own time (HIP events around repeated launches on the final candidate buffers).

    python tools/window_localize_bench.py [--rows 7200] [--queries 16] [--max-batch 64] [--reps 5] [--forward-only-scoring]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=7200)
    ap.add_argument("--queries", type=int, default=16)
    ap.add_argument("--max-batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--forward-only-scoring", action="store_true", help="SMIN.forward_only_scoring: the windows are scored by SMIN.score")
    a = ap.parse_args()
    import models
    api = models.vml_amd
    T, L, C, D, dl, layers, Din, Nq, Hh = 256, 64, 4, 512, 128, 3, 500, 20, 256
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = models.SMIN(T, L, C, D, dl, layers, Din, Nq, Hh, dev).to(dev).eval()
    m.forward_only_scoring = a.forward_only_scoring
    raw = torch.randn(a.rows, Din, device=dev)
    qf = torch.randn(a.queries, Nq, 300, device=dev)
    qm = torch.ones(a.queries, Nq, dtype=torch.uint8, device=dev)
    vi = [0] * a.queries
    run = lambda: m.localize_windows(raw, [a.rows], qf, qm, video_index=vi, k=a.k, max_batch=a.max_batch)
    r = run()                                                          # warm-up: allocator, lazily built tables
    torch.cuda.synchronize()
    windows = int(r["n_windows"].sum())
    times = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        r = run()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    best = min(times)

    # the merge alone, on the candidates of the last call's windows (per-window top-k of the same run)
    starts, lens, vptr = api.window_plan([a.rows], T, T // 2)
    G = windows
    kw = a.k
    g = torch.Generator().manual_seed(1)
    idx_i = torch.randint(0, L, (G, kw), generator=g)
    idx = torch.stack([idx_i, torch.clamp(idx_i + torch.randint(0, 16, (G, kw), generator=g), max=L - 1)], -1).to(dev)
    score = torch.rand(G, kw, generator=g).to(dev)
    count = torch.full((G,), kw, dtype=torch.int32, device=dev)
    st = starts.repeat(a.queries).to(dev)
    ln = lens.repeat(a.queries).to(dev)
    per = int(vptr[1])
    pp = (torch.arange(a.queries + 1) * per).to(dev)
    for _ in range(3):
        api.merge_window_moments(idx, score, count, st, ln, pp, T, L, k=a.k, nms_thresh=0.5)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    nrep = 200
    e0.record()
    for _ in range(nrep):
        api.merge_window_moments(idx, score, count, st, ln, pp, T, L, k=a.k, nms_thresh=0.5)
    e1.record()
    torch.cuda.synchronize()
    merge_us = e0.elapsed_time(e1) / nrep * 1e3
    print(json.dumps({"tool": "window_localize_bench", "shape": dict(T=T, L=L, D=D, dl=dl, layers=layers, Din=Din, Nq=Nq),
                      "forward_only_scoring": a.forward_only_scoring, "rows": a.rows, "queries": a.queries, "windows": windows, "max_batch": a.max_batch, "k": a.k,
                      "call_s_best": round(best, 4), "call_s_all": [round(x, 4) for x in times],
                      "windows_per_s": round(windows / best, 1), "merge_us_per_call": round(merge_us, 2),
                      "merge_candidates": G * kw, "layout_status": int(api._lib.load_torch().layout_status(dev)[0])}))


if __name__ == "__main__":
    main()
