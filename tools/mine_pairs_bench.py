#!/usr/bin/env python3
"""Hard-negative mining on the device, in one process:
  (a) the pair plan alone, from a (Q, V) score matrix and gt_video on the device:
        kernel: smin_mine_pairs through the C ABI (four launches);
        torch:  the equivalent torch route, which reads nothing back either -- the query's own video masked out, topk, then the
                groupings by scatter_add (bincount's stand-in without its host read) / cumsum / a stable argsort;
      shapes (Q, V, N): (16, 16, 3) and (1024, 1024, 7);
  (b) a whole training step without the optimizer at V = Q = 16 full-length videos, tacos.yml and activitynet.yml:
        mined:     encode_videos / encode_queries, SMIN.mine_pairs at N = 3 (256 pairs scored), forward_pairs over the plan (64 pairs
                   trained), loss_fn over pair_targets, backward -- training.train_epoch_mined's step;
        all_pairs: forward_pairs over all 256 pairs, the same loss, backward: the only way to show the model every negative without
                   mining;
        random64:  forward_pairs over a fixed list of 64 pairs (each query's own video and three drawn once): the floor, a step that
                   chooses nothing.
      All three know their valid-cell count (no host read in a step) and leave the gradients in .grad.
After a warm-up of every side, alternating blocks of the sides; every timed call lies between two HIP events (host issue time is
inside them).
    python tools/mine_pairs_bench.py [--calls 100] [--warmup 5] [--block 10] [--runs 2] [--shapes tacos_yml,anet_yml] [--skip-steps]
Prints one JSON line per part, shape and run: the median and the 10-90 % spread of each side in microseconds and, for (b), each
side's torch.cuda.max_memory_allocated over one step (bytes above what was allocated before the step)."""
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
PLAN_SHAPES = [(16, 16, 3), (1024, 1024, 7)]


def summary(v):
    q = statistics.quantiles(v, n=10)
    return {"median": round(statistics.median(v), 2), "p10": round(q[0], 2), "p90": round(q[-1], 2), "spread": round(q[-1] - q[0], 2)}


def alternate(sides, calls, block, warmup):
    """{side: summary of microseconds} over alternating blocks of the sides"""
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
    return {s: summary(v) for s, v in us.items()}


def plan_sides(A, dev, Q, V, N, skip=0):
    L_ = A._lib
    lib = L_.load()
    g = torch.Generator().manual_seed(Q + V)
    score = torch.randn(Q, V, generator=g).to(dev)
    gt = torch.randint(0, V, (Q,), generator=g)
    gt_d, gt_col = gt.to(torch.int32).to(dev), gt.to(dev).reshape(Q, 1)
    P = Q * (1 + N)
    outs = [torch.empty(n, dtype=torch.int32, device=dev) for n in (P, P, V + 1, P, Q + 1, P)]
    nbytes = lib.smin_mine_pairs_ws_bytes(Q, V, N)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    zero, ones = torch.zeros(1, dtype=torch.int64, device=dev), torch.ones(P, dtype=torch.int64, device=dev)

    def kernel():
        L_.check(lib.smin_mine_pairs(L_.stream(), L_.ptr(score), L_.ptr(gt_d), Q, V, N, skip, *[L_.ptr(o) for o in outs], L_.ptr(ws), nbytes), "smin_mine_pairs")
        return outs

    def torch_route():
        masked = score.scatter(1, gt_col, float("-inf"))
        neg = masked.topk(skip + N, dim=1).indices[:, skip:]
        vi = torch.cat([gt_col, neg], dim=1).reshape(-1)
        qi = torch.arange(Q, device=dev).repeat_interleave(1 + N)
        counts = torch.zeros(V, dtype=torch.int64, device=dev).scatter_add_(0, vi, ones)
        v_ptr = torch.cat([zero, counts.cumsum(0)])
        v_pairs = torch.sort(vi, stable=True).indices
        return [x.to(torch.int32) for x in (vi, qi, v_ptr, v_pairs, torch.arange(Q + 1, device=dev) * (1 + N), torch.arange(P, device=dev))]

    return {"kernel": kernel, "torch": torch_route}


def check_plan(sides):
    """the two routes agree wherever the scores have no ties (random normal scores: none), before anything is timed"""
    a, b = sides["kernel"](), sides["torch"]()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y), "the kernel and the torch route disagree"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--shapes", default="tacos_yml,anet_yml")
    ap.add_argument("--skip-steps", action="store_true", help="part (a) only")
    args = ap.parse_args()
    import models
    from oracle import smin_oracle as O
    from tests import helpers as H
    A = models.vml_amd
    assert torch.cuda.is_available(), "mine_pairs_bench needs a HIP device"
    dev = torch.device("cuda:0")
    A._lib.load_torch()
    for Q, V, N in PLAN_SHAPES:
        sides = plan_sides(A, dev, Q, V, N)
        check_plan(sides)
        for run in range(args.runs):
            res = alternate(sides, args.calls, args.block, args.warmup)
            print(json.dumps({"part": "plan", "Q": Q, "V": V, "N": N, "run": run, "calls": args.calls, "us": res,
                              "torch_over_kernel": round(res["torch"]["median"] / res["kernel"]["median"], 3)}), flush=True)
    if args.skip_steps:
        return
    V = Q = 16
    N = 3
    for name in args.shapes.split(","):
        T, L, C, D, dl, layers, Din, Nq, Hh = shape = SHAPES[name]
        m = models.SMIN(*shape, dev)
        m.load_state_dict(O.formula_state_dict(H.smin_shapes(*shape), gain=1.3))
        m = m.to(dev).train()
        vb = {k: v.to(dev) for k, v in O.synthetic_batch(V, T, L, Nq, Din, seed=1, with_labels=False, full_length=True).items()}
        qb = {k: v.to(dev) for k, v in O.synthetic_batch(Q, T, L, Nq, Din, seed=2, full_length=True).items()}
        vid = {k: vb[k] for k in ("video_features", "video_mask", "length_mask", "moment_mask")}
        inputs = [vid["video_features"], vid["video_mask"], qb["query_features"], qb["query_mask"], vid["length_mask"], vid["moment_mask"]]
        cells = vid["moment_mask"].reshape(V, -1).sum(1).tolist()
        assert len(set(cells)) == 1
        gt = np.arange(Q)
        rng = np.random.RandomState(7)
        qi_all, vi_all = np.repeat(np.arange(Q), V), np.tile(np.arange(V), Q)
        qi_64 = np.repeat(np.arange(Q), 1 + N)
        vi_64 = np.concatenate([[q] + list(rng.choice([v for v in range(V) if v != q], N, replace=False)) for q in range(Q)])

        def loss_of(out, t):
            return A.loss_fn(out[0], t["ym"], t["sm"], t["moment_mask"], out[1], t["ys"], t["ss"], out[2], t["ye"], t["se"], out[3], t["ya"], t["length_mask"])

        def step(plan):
            out = m.forward_pairs(*inputs, None, None, cell_counts=cells, plan=plan)
            loss_of(out, A.pair_targets(vid, qb, None, None, None, plan=plan)).backward()

        def clear():
            for p in m.parameters():
                p.grad = None

        def mined():
            clear()
            with torch.no_grad():
                videos = m.encode_videos(*[vid[k] for k in ("video_features", "video_mask", "length_mask", "moment_mask")], cell_counts=cells)
                queries = m.encode_queries(qb["query_features"], qb["query_mask"])
                plan = m.mine_pairs(videos, queries, gt, N)
            step(plan)

        def listed(vi, qi):
            def fn():
                clear()
                step(A.PairPlan(vi, qi, V, Q, dev, gt_video=gt))
            return fn

        sides = {"mined": mined, "all_pairs": listed(vi_all, qi_all), "random64": listed(vi_64, qi_64)}
        for fn in sides.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        peak = {}
        for side, fn in sides.items():
            clear()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            fn()
            torch.cuda.synchronize()
            peak[side] = torch.cuda.max_memory_allocated(dev) - base
        for run in range(args.runs):
            res = alternate(sides, args.calls, args.block, args.warmup)
            print(json.dumps({"part": "step", "shape": name, "run": run, "V": V, "Q": Q, "N": N, "gemm_mode": A.get_gemm_mode(), "calls": args.calls, "us": res,
                              "all_pairs_over_mined": round(res["all_pairs"]["median"] / res["mined"]["median"], 3),
                              "mined_over_random64": round(res["mined"]["median"] / res["random64"]["median"], 3), "peak_step_bytes": peak}), flush=True)
        del m, vb, qb, vid, inputs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
