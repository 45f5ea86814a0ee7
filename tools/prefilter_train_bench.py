#!/usr/bin/env python3
"""What training the first-stage video score costs, in one process:
  (a) term:  forward + backward of training.prefilter_rank_loss (the modules' encoders, smin_prefilter_scores with maps,
             smin_pair_rank_fwd / _bwd, smin_prefilter_maps_bwd, the encoders' backward) against the same term through
             prefilter_scores_torch and autograd on the device -- the only route before smin_prefilter_maps_bwd: the same encoders, the
             same all-pairs plan and the same pair_rank_loss, the maps and their backward as torch ops -- at (Q, V) = (16, 16) and
             (64, 64);
  (b) step:  a mined step (3p's shape: V = Q = 16, three negatives per query, equal cell counts) with prefilter_weight = 0.5 against the
             same step without the term (the parent's step), forward + backward, no optimizer.
Shapes: tacos.yml and activitynet.yml (BASELINE.json configs).  After a warm-up of all sides, alternating blocks; every timed call lies
between two HIP events (host issue time is inside them).
    python tools/prefilter_train_bench.py [--calls 100] [--warmup 5] [--block 10] [--runs 2] [--shapes tacos_yml,anet_yml] [--skip-step]
Prints one JSON line per part, shape, size and run: the median and the 10-90 % spread of each side in microseconds."""
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
TERM_SIZES = [(16, 16), (64, 64)]
TAU = GAMMA = 0.1


def summary(v):
    q = statistics.quantiles(v, n=10)
    return {"median": round(statistics.median(v), 2), "p10": round(q[0], 2), "p90": round(q[-1], 2), "spread": round(q[-1] - q[0], 2)}


def timed_blocks(sides, calls, warmup, block):
    """{side: summary of microseconds per call}: a warm-up of every side, then alternating blocks, each call between two HIP events"""
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


def build(models, A, shape, V, Q, dev):
    from oracle import smin_oracle as O
    from tests import helpers as H
    T, L, C, D, dl, layers, Din, Nq, Hh = shape
    m = models.SMIN(*shape, dev)
    m.load_state_dict(O.formula_state_dict(H.smin_shapes(*shape), gain=1.3))
    m = m.to(dev).train()
    vb = {k: v.to(dev) for k, v in O.synthetic_batch(V, T, L, Nq, Din, seed=1, with_labels=False, full_length=True).items()}
    qb = {k: v.to(dev) for k, v in O.synthetic_batch(Q, T, L, Nq, Din, seed=2, full_length=True).items()}
    g = {k: vb[k] for k in ("video_features", "video_mask", "length_mask", "moment_mask")}
    g.update(qb)
    g["gt_video"] = np.arange(Q) % V
    g["cell_counts"] = g["moment_mask"].reshape(V, -1).sum(1).tolist()
    assert len(set(g["cell_counts"])) == 1
    return m, g


def clear(m):
    for p in m.parameters():
        p.grad = None


def bench_term(A, models, args, dev):
    for name in args.shapes.split(","):
        shape = SHAPES[name]
        T, L, C, D = shape[:4]
        for Q, V in TERM_SIZES:
            m, g = build(models, A, shape, V, Q, dev)
            plan = A.training.all_pairs_plan(V, Q, g["gt_video"], dev)
            mm_pairs = g["moment_mask"].index_select(0, plan.video_index)
            heads = (m.localization.conv_layer_pm, m.localization.conv_layer_ps, m.localization.conv_layer_pe)

            def kernels():
                clear(m)
                loss = A.prefilter_rank_loss(m, g, TAU, GAMMA)
                loss.backward()
                return loss

            def torch_route():
                clear(m)
                fv = m.backbone.videoencoder(g["video_features"], g["video_mask"].reshape(V, -1, 1))
                fs, _ = m.backbone.queryencoder(g["query_features"], g["query_mask"])
                w, b = torch.stack([h.weight.reshape(D) for h in heads]), torch.cat([h.bias.reshape(1) for h in heads])
                out = A.prefilter_scores_torch(fv, fs, w, b, g["length_mask"], g["moment_mask"], T, L, C, TAU, maps=True)
                loss = A.pair_rank_loss(out[3].reshape(Q * V, L, L), out[4].reshape(Q * V, L), out[5].reshape(Q * V, L), mm_pairs, plan, TAU, GAMMA)
                loss.backward()
                return loss

            lk = kernels().item()
            gk = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
            lt = torch_route().item()
            diff = max(((gk[k] - p.grad).abs().max() / gk[k].abs().max().clamp_min(1e-30)).item() for k, p in m.named_parameters() if p.grad is not None)
            for run in range(args.runs):
                res = timed_blocks({"kernels": kernels, "torch_route": torch_route}, args.calls, args.warmup, args.block)
                print(json.dumps({"bench": "term", "shape": name, "run": run, "Q": Q, "V": V, "gemm_mode": A.get_gemm_mode(), "calls": args.calls,
                                  "loss": [lk, lt], "grad_max_rel_diff": diff, "us": res,
                                  "kernels_over_torch": round(res["kernels"]["median"] / res["torch_route"]["median"], 4)}), flush=True)
            del m, g
            torch.cuda.empty_cache()


def bench_step(A, models, args, dev):
    V = Q = 16
    N = 3
    for name in args.shapes.split(","):
        m, g = build(models, A, SHAPES[name], V, Q, dev)
        inputs = [g[k] for k in A.training.MODEL_INPUTS]

        def step(weight):
            def fn():
                clear(m)
                with torch.no_grad():
                    videos = m.encode_videos(g["video_features"], g["video_mask"], g["length_mask"], g["moment_mask"], cell_counts=g["cell_counts"])
                    queries = m.encode_queries(g["query_features"], g["query_mask"])
                    plan = m.mine_pairs(videos, queries, g["gt_video"], N)
                out = m.forward_pairs(*inputs, None, None, cell_counts=g["cell_counts"], plan=plan)
                t = A.pair_targets(g, g, None, None, None, plan=plan)
                loss = A.loss_fn(out[0], t["ym"], t["sm"], t["moment_mask"], out[1], t["ys"], t["ss"], out[2], t["ye"], t["se"], out[3], t["ya"],
                                 t["length_mask"])
                if weight != 0.0:
                    loss = loss + weight * A.prefilter_rank_loss(m, g, TAU, GAMMA)
                loss.backward()
            return fn

        sides = {"parent_step": step(0.0), "with_prefilter_term": step(0.5)}
        for run in range(args.runs):
            res = timed_blocks(sides, args.calls, args.warmup, args.block)
            print(json.dumps({"bench": "step", "shape": name, "run": run, "Q": Q, "V": V, "N": N, "gemm_mode": A.get_gemm_mode(), "calls": args.calls,
                              "us": res, "added_us": round(res["with_prefilter_term"]["median"] - res["parent_step"]["median"], 2),
                              "with_over_parent": round(res["with_prefilter_term"]["median"] / res["parent_step"]["median"], 4)}), flush=True)
        del m, g
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--shapes", default="tacos_yml,anet_yml")
    ap.add_argument("--skip-step", action="store_true", help="part (a) only")
    args = ap.parse_args()
    import models
    A = models.vml_amd
    assert torch.cuda.is_available(), "prefilter_train_bench needs a HIP device"
    dev = torch.device("cuda:0")
    A._lib.load_torch()
    bench_term(A, models, args, dev)
    if not args.skip_step:
        bench_step(A, models, args, dev)


if __name__ == "__main__":
    main()
