#!/usr/bin/env python3
"""What the per-group host read of a long-video evaluation loop costs: training.test_model_windows against the
same loop with the metric computed on the host, in one process, on the same groups and model.

    python tools/window_eval_bench.py [--rows 7200] [--queries 16] [--groups 4] [--blocks 10] [--forward-only-scoring]

Shape of INTEGRATION.md 3f (ActivityNet, T = 256, L = 64): every group is one video of ``--rows`` feature rows with ``--queries``
queries on it, default window (T rows) and stride (T / 2) -- 896 windows per group at the defaults.  Loops over ``--groups`` groups:
  A  ``test_model_windows`` with an EpochMeter: ``update_spans`` per group, one ``result()`` per block;
  B  the loop a caller has to write without it: ``localize_windows``, then ``span`` and ``count`` copied to the host per group
     (``.cpu()``) and R@n, IoU=m / mIoU formed there in numpy fp32.
After one warm-up pass of both loops, blocks alternate A, B, A, B ...; a host clock is taken around each block, which ends in a
device synchronise.  Reported: the median over the blocks of the time per group and its 10-90 % spread, in milliseconds.  One JSON
line, then a table.  Profiler off (run the tool under ``rocprofv3 --kernel-trace --stats`` for the kernels' own times)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_LIST, M_LIST = (1, 5), (0.1, 0.3, 0.5, 0.7)


def summary(ms):
    q = statistics.quantiles(ms, n=10)
    return {"median": round(statistics.median(ms), 4), "p10": round(q[0], 4), "p90": round(q[-1], 4), "spread": round(q[-1] - q[0], 4)}


def host_metric(span, count, gt, acc):
    """R@n, IoU=m hits and the top-1 IoU sum of one group on the host (numpy fp32, vectorised), added to acc."""
    st, en = span[..., 0], span[..., 1]
    gs, ge = gt[:, 0:1], gt[:, 1:2]
    with np.errstate(invalid="ignore", divide="ignore"):
        inter = np.fmax(np.fmin(en, ge) - np.fmax(st, gs), np.float32(0))
        uni = np.fmax(en, ge) - np.fmin(st, gs)
        iou = np.where(uni > 0, inter / uni, np.float32(0))
    valid = np.arange(span.shape[1])[None, :] < count[:, None]
    iou = np.where(valid, iou, np.float32(0))
    acc[0] += span.shape[0]
    acc[3] += iou[:, 0].astype(np.float64).sum()
    for a, n in enumerate(N_LIST):
        for c, m in enumerate(M_LIST):
            acc[4 + a * len(M_LIST) + c] += ((iou[:, :n] > np.float32(m)) & valid[:, :n]).any(axis=1).sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=7200)
    ap.add_argument("--queries", type=int, default=16)
    ap.add_argument("--groups", type=int, default=4, help="groups per timed block")
    ap.add_argument("--blocks", type=int, default=10, help="timed blocks per loop")
    ap.add_argument("--max-batch", type=int, default=64)
    ap.add_argument("--forward-only-scoring", action="store_true")
    a = ap.parse_args()
    if torch.cuda.device_count() < 1:
        print("window_eval_bench: no HIP device found", file=sys.stderr)
        return 1
    import models
    api = models.vml_amd
    T, L, C, D, dl, layers, Din, Nq, Hh = 256, 64, 4, 512, 128, 3, 500, 20, 256
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = models.SMIN(T, L, C, D, dl, layers, Din, Nq, Hh, dev).to(dev).eval()
    model.forward_only_scoring = a.forward_only_scoring
    rng = np.random.default_rng(1)
    groups = []
    for _ in range(a.groups):
        ts = rng.uniform(0.0, 0.9, a.queries) * a.rows
        groups.append(dict(raw=torch.randn(a.rows, Din, device=dev), lengths=np.array([a.rows]), query_features=torch.randn(a.queries, Nq, 300, device=dev),
                           query_mask=torch.ones(a.queries, Nq, dtype=torch.uint8, device=dev), video_index=np.zeros(a.queries, np.int64),
                           times=np.stack([ts, ts + rng.uniform(4.0, 120.0, a.queries)], 1), duration=np.full(a.queries, float(a.rows))))
    meter = api.EpochMeter(n=N_LIST, m=M_LIST, device=dev)

    def loop_a(gs):
        meter.reset()
        return api.test_model_windows(model, gs, meter, max_batch=a.max_batch)

    def loop_b(gs):
        acc = np.zeros(4 + len(N_LIST) * len(M_LIST), np.float64)
        for g in gs:
            out = model.localize_windows(g["raw"], g["lengths"], g["query_features"], g["query_mask"], video_index=g["video_index"],
                                         max_batch=a.max_batch)
            gt = (g["times"] / g["duration"][:, None] * g["lengths"][g["video_index"]].astype(np.float64)[:, None]).astype(np.float32)
            host_metric(out["span"].cpu().numpy(), out["count"].cpu().numpy(), gt, acc)
        r = {f"R@{n}, IoU={m}": acc[4 + i * len(M_LIST) + c] / acc[0] for i, n in enumerate(N_LIST) for c, m in enumerate(M_LIST)}
        r.update(mIoU=acc[3] / acc[0], num_samples=int(acc[0]))
        return {k: (v if isinstance(v, int) else float(v)) for k, v in r.items()}

    ra, rb = loop_a(groups), loop_b(groups)                                    # warm-up, and the two loops agree
    torch.cuda.synchronize()
    agree = bool(all(ra[k] == rb[k] for k in rb if k != "mIoU") and abs(ra["mIoU"] - rb["mIoU"]) <= 1e-12)
    ms = {"A": [], "B": []}
    for _ in range(a.blocks):
        for name, fn in (("A", loop_a), ("B", loop_b)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(groups)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / len(groups))
    sa, sb = summary(ms["A"]), summary(ms["B"])
    windows = int(api.window_plan([a.rows], T, T // 2)[2][-1]) * a.queries
    print(json.dumps({"rows": a.rows, "queries": a.queries, "windows_per_group": windows, "groups": a.groups, "blocks": a.blocks,
                      "forward_only_scoring": a.forward_only_scoring, "gemm_mode": api.get_gemm_mode(), "loops_agree": agree,
                      "A_ms_per_group": sa, "B_ms_per_group": sb, "B_minus_A_ms": round(sb["median"] - sa["median"], 4)}), flush=True)
    print("| loop | ms per group (10-90 % spread) |")
    print("|---|---|")
    print(f"| A: test_model_windows, one read per block | {sa['median']:.3f} ({sa['spread']:.3f}) |")
    print(f"| B: metric on the host, reads per group | {sb['median']:.3f} ({sb['spread']:.3f}) |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
