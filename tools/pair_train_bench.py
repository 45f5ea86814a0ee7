#!/usr/bin/env python3
"""A training step over (video, query) pairs that share their videos and queries, in one process:
  (a) pairs:    SMIN.forward_pairs (each video and each query encoded once, smin_pair_assemble / smin_pair_assemble_bwd between the
                encoders and the layers), loss_fn over training.pair_targets, backward;
  (b) expanded: the same pairs with every pair's video and query features expanded to a row of its own (index_select, inside the
                timed call: a new batch needs it every step) and handed to SMIN.forward, the same loss, backward -- the only route
                before forward_pairs.
Both sides know their valid-cell count (no host read in a step) and leave the gradients in .grad; no optimizer step.
Shapes: tacos.yml and activitynet.yml; layouts "8x8" (8 videos x 8 queries, all 64 pairs) and "16x4" (16 queries, each against its own
video and three others of 16: 64 pairs).  After a warm-up of both, alternating blocks of the two; every timed call lies between two HIP
events (host issue time is inside them).
    python tools/pair_train_bench.py [--calls 100] [--warmup 5] [--block 10] [--runs 2] [--shapes tacos_yml,anet_yml] [--layouts 8x8,16x4]
Prints one JSON line per shape, layout and run: the median and the 10-90 % spread of each side in microseconds, each side's
torch.cuda.max_memory_allocated over one step (bytes above what was allocated before the step), and the time of
smin_pair_assemble_bwd alone at that shape (C ABI, random operands) beside the bytes it moves, counted from its loops."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {   # T, L, C, D, dl, layers, Din, Nq, H  (BASELINE.json configs)
    "tacos_yml": (128, 32, 4, 512, 128, 3, 4096, 14, 256),
    "anet_yml": (128, 64, 4, 512, 128, 3, 500, 20, 256),
}


def layout(name):
    """V, Q, video_index, query_index, gt_video"""
    if name == "8x8":
        return 8, 8, np.tile(np.arange(8), 8), np.repeat(np.arange(8), 8), np.arange(8)
    if name == "16x4":
        qi = np.repeat(np.arange(16), 4)
        return 16, 16, (qi + np.tile(np.arange(4), 16)) % 16, qi, np.arange(16)
    raise ValueError(f"unknown layout {name!r}")


def summary(v):
    q = statistics.quantiles(v, n=10)
    return {"median": round(statistics.median(v), 2), "p10": round(q[0], 2), "p90": round(q[-1], 2), "spread": round(q[-1] - q[0], 2)}


def kernel_alone(A, dev, P, V, Q, T, Nq, D, vi, qi, calls):
    """microseconds of smin_pair_assemble_bwd (both launches) and the bytes its loops move"""
    L_ = A._lib
    lib = L_.load()
    plan = A.PairPlan(vi, qi, V, Q, dev)
    df, dfw, dfs = torch.randn(P, T, D, device=dev), torch.randn(P, Nq, D, device=dev), torch.randn(P, D, device=dev)
    fv, fsb = torch.randn(V, T, D, device=dev), torch.randn(Q, D, device=dev)
    outs = [torch.empty(V, T, D, device=dev), torch.empty(Q, Nq, D, device=dev), torch.empty(Q, D, device=dev)]
    nbytes = lib.smin_pair_assemble_bwd_workspace_bytes(P, T, D)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    args = [L_.ptr(x) for x in (df, dfw, dfs, fv, fsb, plan.video_index, plan.query_index, plan.v_ptr, plan.v_pairs, plan.q_ptr, plan.q_pairs)]

    def call():
        L_.check(lib.smin_pair_assemble_bwd(L_.stream(), *args, P, V, Q, T, Nq, D, *[L_.ptr(o) for o in outs], L_.ptr(ws), nbytes), "smin_pair_assemble_bwd")

    for _ in range(5):
        call()
    ev = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        ev.append((a, b))
    torch.cuda.synchronize()
    TC = (T + 3) // 4
    counted = {"df_read": 4 * P * T * D, "fv_read": 4 * V * T * D, "dfv_write": 4 * V * T * D, "partials_write_and_read": 2 * 4 * P * TC * D,
               "fs_bank_gathers": 4 * P * TC * D, "dfw_read": 4 * P * Nq * D, "dfw_bank_write": 4 * Q * Nq * D, "dfs_read": 4 * P * D, "dfs_bank_write": 4 * Q * D}
    us = summary([a.elapsed_time(b) * 1e3 for a, b in ev])
    total = sum(counted.values())
    return {"us": us, "counted_bytes": counted, "counted_total": total, "GB_per_s_at_median": round(total / us["median"] / 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--shapes", default="tacos_yml,anet_yml")
    ap.add_argument("--layouts", default="8x8,16x4")
    args = ap.parse_args()
    import models
    from oracle import smin_oracle as O
    from tests import helpers as H
    A = models.vml_amd
    assert torch.cuda.is_available(), "pair_train_bench needs a HIP device"
    dev = torch.device("cuda:0")
    A._lib.load_torch()
    for name in args.shapes.split(","):
        T, L, C, D, dl, layers, Din, Nq, Hh = shape = SHAPES[name]
        m = models.SMIN(*shape, dev)
        m.load_state_dict(O.formula_state_dict(H.smin_shapes(*shape), gain=1.3))
        m = m.to(dev).train()
        for lay in args.layouts.split(","):
            V, Q, vi, qi, gt = layout(lay)
            P = vi.shape[0]
            vb = {k: v.to(dev) for k, v in O.synthetic_batch(V, T, L, Nq, Din, seed=1, with_labels=False).items()}
            qb = {k: v.to(dev) for k, v in O.synthetic_batch(Q, T, L, Nq, Din, seed=2).items()}
            vid = {k: vb[k] for k in ("video_features", "video_mask", "length_mask", "moment_mask")}
            inputs = [vid["video_features"], vid["video_mask"], qb["query_features"], qb["query_mask"], vid["length_mask"], vid["moment_mask"]]
            cells = vid["moment_mask"].reshape(V, -1).sum(1).tolist()
            known = int(sum(cells[v] for v in vi))
            vi_d, qi_d = torch.from_numpy(vi).to(dev), torch.from_numpy(qi).to(dev)

            def loss_of(out, t):
                return A.loss_fn(out[0], t["ym"], t["sm"], t["moment_mask"], out[1], t["ys"], t["ss"], out[2], t["ye"], t["se"], out[3], t["ya"], t["length_mask"])

            def side_a():
                for p in m.parameters():
                    p.grad = None
                plan = A.PairPlan(vi, qi, V, Q, dev, gt_video=gt)
                out = m.forward_pairs(*inputs, None, None, cell_counts=cells, plan=plan)
                loss_of(out, A.pair_targets(vid, qb, None, None, None, plan=plan)).backward()

            def side_b():
                for p in m.parameters():
                    p.grad = None
                t = A.pair_targets(vid, qb, vi, qi, gt)
                m.known_cell_count = known
                out = m(inputs[0].index_select(0, vi_d), inputs[1].index_select(0, vi_d), inputs[2].index_select(0, qi_d), inputs[3].index_select(0, qi_d),
                        t["length_mask"], t["moment_mask"])
                m.known_cell_count = None
                loss_of(out, t).backward()

            sides = {"pairs": side_a, "expanded": side_b}
            for _ in range(args.warmup):
                for fn in sides.values():
                    fn()
            torch.cuda.synchronize()
            peak = {}
            for side, fn in sides.items():
                for p in m.parameters():
                    p.grad = None
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats(dev)
                base = torch.cuda.memory_allocated(dev)
                fn()
                torch.cuda.synchronize()
                peak[side] = torch.cuda.max_memory_allocated(dev) - base
            alone = kernel_alone(A, dev, P, V, Q, T, Nq, D, vi, qi, args.calls)
            for run in range(args.runs):
                timed, done = [], 0
                while done < args.calls:
                    n = min(args.block, args.calls - done)
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
                res = {s: summary(v) for s, v in us.items()}
                print(json.dumps({"shape": name, "layout": lay, "run": run, "V": V, "Q": Q, "pairs": P, "gemm_mode": A.get_gemm_mode(), "calls": args.calls, "us": res,
                                  "expanded_over_pairs": round(res["expanded"]["median"] / res["pairs"]["median"], 3), "peak_step_bytes": peak,
                                  "smin_pair_assemble_bwd": alone}), flush=True)
            del vb, qb, vid, inputs
            torch.cuda.empty_cache()
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
