#!/usr/bin/env python3
"""What the first-stage pruning of corpus search costs and saves, in one process:
  (a) first stage: moments.prefilter_scores + rank_videos + prefilter_select (smin_prefilter_scores, smin_video_rank,
               smin_prefilter_select) on random banks at (Q, V) = (16, 32) and (1024, 1024), against the same stage as torch ops on the
               device: prefilter_scores_torch over chunks of queries (its (Q, V, L, L) maps do not fit at 2^20 pairs), a stable argsort
               of the (Q, V) scores and prefilter_select_torch;
  (b) search:  SMIN.search of Q = 16 queries over V = 32 videos with prefilter=8 against the same call without it (every pair through
               the full model: the only route before the option), with each side's peak device memory.
Shapes: tacos.yml and activitynet.yml (BASELINE.json configs), chunks of 64 pairs, forward_only_scoring (3m's shape).
After a warm-up of all sides, alternating blocks; every timed call lies between two HIP events (host issue time is inside them).
    python tools/prefilter_bench.py [--calls 100] [--big-calls 10] [--warmup 10] [--block 10] [--runs 2] [--shapes tacos_yml,anet_yml]
                                    [--skip-search] [--skip-big] [--skip-first-stage] [--full-length]
Prints one JSON line per shape, size and run: the median and the 10-90 % spread of each side in microseconds."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {   # T, L, C, D, dl, layers, Din, Nq, H  (BASELINE.json configs)
    "tacos_yml": (128, 32, 4, 512, 128, 3, 4096, 14, 256),
    "anet_yml": (128, 64, 4, 512, 128, 3, 500, 20, 256),
}
TAU, KEEP = 0.1, 8


def summary(v):
    q = statistics.quantiles(v, n=10)
    return {"median": round(statistics.median(v), 2), "p10": round(q[0], 2), "p90": round(q[-1], 2), "spread": round(q[-1] - q[0], 2)}


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


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def bench_first_stage(A, args, dev):
    g = torch.Generator().manual_seed(11)
    sizes = [(16, 32, args.calls, args.warmup)] + ([] if args.skip_big else [(1024, 1024, args.big_calls, 2)])
    for name in args.shapes.split(","):
        T, L, C, D = SHAPES[name][:4]
        for Q, V, calls, warmup in sizes:
            fv, fs = torch.randn(V, T, D, generator=g).to(dev), torch.randn(Q, D, generator=g).to(dev)
            w, b = (torch.randn(3, D, generator=g) / D ** 0.5).to(dev), (torch.randn(3, generator=g) / 2).to(dev)
            lm = torch.ones(V, L, dtype=torch.bool, device=dev)
            mm = torch.triu(torch.ones(L, L, dtype=torch.bool, device=dev)).expand(V, L, L).contiguous()
            video = torch.arange(V, dtype=torch.int32, device=dev).repeat(Q)
            ptr = torch.arange(Q + 1, dtype=torch.int32, device=dev) * V
            qchunk = max(1, min(Q, (64 << 20) // (V * L * L)))                       # the restatement's maps: 256 MB of fp32 per chunk

            def kernels():
                score, _, cells = A.prefilter_scores(fv, fs, w, b, lm, mm, T, L, C, TAU)
                vr = A.rank_videos(score.reshape(-1), cells.reshape(-1), video, ptr, n=1)
                return score, A.prefilter_select(vr["pair_rank"].reshape(Q, V), KEEP)

            def torch_ops():
                score = torch.cat([A.prefilter_scores_torch(fv, fs[q0:q0 + qchunk], w, b, lm, mm, T, L, C, TAU)[0] for q0 in range(0, Q, qchunk)])
                order = torch.argsort(score, dim=1, descending=True, stable=True)
                rank = torch.empty_like(order)
                rank.scatter_(1, order, torch.arange(V, device=dev).expand_as(order))
                return score, A.prefilter_select_torch(rank, KEEP)

            ks, (kv, _) = kernels()
            ts, (tv, _) = torch_ops()
            err = (ks - ts).abs().max().item()
            agree = (kv.long() == tv.long()).all(dim=1).float().mean().item()        # (ties and roundings may order two videos differently)
            for run in range(args.runs):
                us = timed_blocks({"kernels": kernels, "torch_ops": torch_ops}, calls, warmup, min(args.block, calls))
                res = {s: summary(v) for s, v in us.items()}
                print(json.dumps({"bench": "first_stage", "shape": name, "run": run, "Q": Q, "V": V, "keep": KEEP, "gemm_mode": A.get_gemm_mode(),
                                  "calls": calls, "torch_query_chunk": qchunk, "score_max_abs_diff": err, "lists_equal_share": round(agree, 4),
                                  "us": res, "kernels_over_torch": round(res["kernels"]["median"] / res["torch_ops"]["median"], 4)}), flush=True)
            del fv, fs, mm
            torch.cuda.empty_cache()


def bench_search(A, models, args, dev):
    from oracle import smin_oracle as O
    from tests import helpers as H
    Q, V, mb, k = args.Q, args.V, args.max_batch, args.k
    for name in args.shapes.split(","):
        T, L, C, D, dl, layers, Din, Nq, Hh = shape = SHAPES[name]
        m = models.SMIN(*shape, dev)
        m.load_state_dict(O.formula_state_dict(H.smin_shapes(*shape), gain=1.3))
        m = m.to(dev).eval()
        m.forward_only_scoring = True
        vb_ = {k_: v.to(dev) for k_, v in O.synthetic_batch(V, T, L, Nq, Din, seed=1, with_labels=False, full_length=args.full_length).items()}
        qb_ = {k_: v.to(dev) for k_, v in O.synthetic_batch(Q, T, L, Nq, Din, seed=2, with_labels=False).items()}
        banks = (m.encode_videos(*[vb_[key] for key in ("video_features", "video_mask", "length_mask", "moment_mask")]),
                 m.encode_queries(qb_["query_features"], qb_["query_mask"]))
        sides = {"full": lambda: m.search(*banks, k=k, max_batch=mb),
                 "prefilter": lambda: m.search(*banks, k=k, max_batch=mb, prefilter=KEEP, tau=TAU),
                 "first_stage_only": lambda: m.prefilter_videos(*banks, KEEP, tau=TAU)}
        full, cut = sides["full"](), sides["prefilter"]()
        top1 = (full["video"][:, 0] == cut["video"][:, 0]).float().mean().item()     # (synthetic inputs, formula weights: no recall claim)
        mem = {s: peak_mb(fn) for s, fn in sides.items()}
        for run in range(args.runs):
            us = timed_blocks(sides, args.calls, args.warmup, args.block)
            res = {s: summary(v) for s, v in us.items()}
            print(json.dumps({"bench": "search", "shape": name, "run": run, "Q": Q, "V": V, "keep": KEEP, "max_batch": mb, "k": k,
                              "equal_cell_counts": len(set(banks[0].cell_counts)) == 1, "gemm_mode": A.get_gemm_mode(), "calls": args.calls,
                              "us": res, "peak_mb": mem, "same_top1_video_share": round(top1, 4),
                              "prefilter_over_full": round(res["prefilter"]["median"] / res["full"]["median"], 4)}), flush=True)
        del m, banks, vb_, qb_
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Q", type=int, default=16)
    ap.add_argument("--V", type=int, default=32)
    ap.add_argument("--max-batch", type=int, default=64)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--big-calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--shapes", default="tacos_yml,anet_yml")
    ap.add_argument("--skip-search", action="store_true")
    ap.add_argument("--skip-big", action="store_true")
    ap.add_argument("--skip-first-stage", action="store_true")
    ap.add_argument("--full-length", action="store_true", help="videos of equal length: equal cell_counts, so the pruned search reads nothing back")
    args = ap.parse_args()
    import models
    A = models.vml_amd
    assert torch.cuda.is_available(), "prefilter_bench needs a HIP device"
    dev = torch.device("cuda:0")
    A._lib.load_torch()
    if not args.skip_first_stage:
        bench_first_stage(A, args, dev)
    if not args.skip_search:
        bench_search(A, models, args, dev)


if __name__ == "__main__":
    main()
