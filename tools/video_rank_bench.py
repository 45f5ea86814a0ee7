#!/usr/bin/env python3
"""What the video-level score costs in corpus search, and the new kernels alone, in one process:
  (a) search:  SMIN.search over prebuilt banks, plain (the code of before the options: the baseline) against
               search(video_weight=7.5, max_videos=8) -- one pair_pool per chunk, smin_video_rank, smin_moment_reweight on top -- and
               against the plain search followed by the same pooling, ranking and weighting as torch ops on the device: the real
               pairs' maps, kept from one scoring pass outside the timed region, pooled chunk by chunk with pair_pool_torch (search
               does not hand its maps out, so a caller would pay a second scoring pass for them, which this side is not charged),
               a dense stable argsort, and the weights gathered onto the ranked list;
  (b) kernels: smin_pair_pool, smin_group_pool, smin_video_rank and smin_moment_reweight alone at (Q, V) = (16, 32) and (1024, 1024)
               against torch ops on the device: the ``*_torch`` restatements where they are device code (pair_pool_torch,
               reweight_moments_torch) and, where the restatement is a host loop (rank_videos_torch, group_pool_torch), the dense torch
               form a user would write: a stable argsort of the (Q, V) score matrix, the inverse permutation, exp; segment sums by
               index_add_.  pair_pool is measured at min(Q * V, 16384) maps of L = 32 (the maps of 2^20 pairs do not fit a chunk loop).
Shapes of (a): tacos.yml and activitynet.yml, Q = 16 queries, V = 32 videos, chunks of 64 pairs, forward_only_scoring (3m's shape).
After a warm-up of all sides, alternating blocks; every timed call lies between two HIP events (host issue time is inside them).
    python tools/video_rank_bench.py [--calls 100] [--warmup 10] [--block 10] [--runs 2] [--shapes tacos_yml,anet_yml] [--skip-search]
Prints one JSON line per shape and run, and one per kernel shape: the median and the 10-90 % spread of each side in microseconds."""
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
ALPHA, TAU = 7.5, 0.1


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


def dense_rank_torch(score, alpha):
    """rank and weight of a dense (Q, V) score matrix as torch ops on the device: ties -> lower video (a stable sort)"""
    order = torch.argsort(score, dim=1, descending=True, stable=True)
    rank = torch.empty_like(order)
    rank.scatter_(1, order, torch.arange(score.shape[1], device=score.device).expand_as(order))
    return rank, torch.exp(alpha * (score - score.max(dim=1, keepdim=True).values)), order


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
        vb_ = {k_: v.to(dev) for k_, v in O.synthetic_batch(V, T, L, Nq, Din, seed=1, with_labels=False).items()}
        qb_ = {k_: v.to(dev) for k_, v in O.synthetic_batch(Q, T, L, Nq, Din, seed=2, with_labels=False).items()}
        banks = (m.encode_videos(*[vb_[key] for key in ("video_features", "video_mask", "length_mask", "moment_mask")]),
                 m.encode_queries(qb_["query_features"], qb_["query_mask"]))
        qi, vi = np.repeat(np.arange(Q), V), np.tile(np.arange(V), Q)
        reps = -(-Q * V // mb)
        maps = []                                                                    # every chunk's maps, for the torch side's pooling
        for c0 in range(0, Q * V, mb):
            pm, ps, pe, _ = m.score_pairs(*banks, vi[c0:c0 + mb], qi[c0:c0 + mb])
            maps.append((pm, ps, pe, banks[0].moment_mask.index_select(0, torch.from_numpy(vi[c0:c0 + mb]).to(dev))))
        vid_of = torch.from_numpy(vi).to(dev)

        def plain():
            return m.search(*banks, k=k, max_batch=mb)

        def weighted():
            return m.search(*banks, k=k, max_batch=mb, video_weight=ALPHA, max_videos=8, tau=TAU)

        def torch_route():
            r = m.search(*banks, k=k, max_batch=mb)
            s = torch.cat([A.pair_pool_torch(*x, TAU)[0] for x in maps]).reshape(Q, V)
            rank, weight, _ = dense_rank_torch(s, ALPHA)
            w = weight.reshape(-1)[(torch.arange(Q, device=dev).unsqueeze(1) * V + r["video"].clamp_min(0)).reshape(-1)].reshape(Q, k)
            return r["score"] * w, rank, vid_of

        sides = {"plain": plain, "weighted": weighted, "plain_plus_torch": torch_route}
        for run in range(args.runs):
            us = timed_blocks(sides, args.calls, args.warmup, args.block)
            res = {s: summary(v) for s, v in us.items()}
            print(json.dumps({"bench": "search", "shape": name, "run": run, "Q": Q, "V": V, "max_batch": mb, "chunks": reps, "k": k,
                              "gemm_mode": A.get_gemm_mode(), "calls": args.calls, "us": res,
                              "added_us": round(res["weighted"]["median"] - res["plain"]["median"], 2),
                              "added_us_torch": round(res["plain_plus_torch"]["median"] - res["plain"]["median"], 2),
                              "weighted_over_plain": round(res["weighted"]["median"] / res["plain"]["median"], 4)}), flush=True)
        del m, banks, vb_, qb_, maps
        torch.cuda.empty_cache()


def bench_kernels(A, args, dev):
    g = torch.Generator().manual_seed(5)
    for Q, V in ((16, 32), (1024, 1024)):
        P, k, L = Q * V, 5, 32
        score = torch.rand(Q, V, generator=g).to(dev)
        flat, cells = score.reshape(-1).contiguous(), torch.full((P,), 7.0, device=dev)
        video = torch.arange(V, dtype=torch.int32).repeat(Q).to(dev)
        ptr = (torch.arange(Q + 1, dtype=torch.int32) * V).to(dev)
        lists, count = torch.rand(P, k, generator=g).to(dev), torch.full((P,), k, dtype=torch.int32, device=dev)
        vr = A.rank_videos(flat, cells, video, ptr, n=5, alpha=ALPHA)
        want_rank, want_weight, _ = dense_rank_torch(score, ALPHA)
        assert torch.equal(vr["pair_rank"].reshape(Q, V).long(), want_rank)          # (distinct scores: the two sides rank alike)
        Pm = min(P, 16384)
        pm, ps, pe = torch.rand(Pm, L, L, generator=g).to(dev), torch.rand(Pm, L, generator=g).to(dev), torch.rand(Pm, L, generator=g).to(dev)
        mm = torch.triu(torch.ones(L, L, dtype=torch.bool)).expand(Pm, L, L).contiguous().to(dev)
        _, pool, pcells = A.pair_pool(pm, ps, pe, mm, TAU)
        W, G2 = Pm, Pm // 4                                                          # groups of four windows
        gp = (torch.arange(G2 + 1, dtype=torch.int32) * 4).to(dev)
        group_of = torch.arange(W, device=dev) // 4

        def group_torch():
            big = torch.full((G2,), float("-inf"), device=dev).scatter_reduce_(0, group_of, pool[:, 0], "amax")
            s = torch.zeros(G2, device=dev).index_add_(0, group_of, pool[:, 1] * torch.exp((pool[:, 0] - big[group_of]) / TAU))
            n = torch.zeros(G2, device=dev).index_add_(0, group_of, pcells)
            return big + TAU * torch.log(s / n)

        sides = {
            "pair_pool": lambda: A.pair_pool(pm, ps, pe, mm, TAU), "pair_pool_torch": lambda: A.pair_pool_torch(pm, ps, pe, mm, TAU),
            "group_pool": lambda: A.group_pool(pool, pcells, gp, TAU), "group_pool_torch_dense": group_torch,
            "video_rank": lambda: A.rank_videos(flat, cells, video, ptr, n=5, alpha=ALPHA), "video_rank_torch_dense": lambda: dense_rank_torch(score, ALPHA),
            "moment_reweight": lambda: A.reweight_moments(lists, count, vr["pair_rank"], vr["weight"], 8),
            "moment_reweight_torch": lambda: A.reweight_moments_torch(lists, count, vr["pair_rank"], vr["weight"], 8),
        }
        us = timed_blocks(sides, args.calls, args.warmup, args.block)
        print(json.dumps({"bench": "kernels", "Q": Q, "V": V, "pairs": P, "k": k, "pool_maps": Pm, "L": L, "calls": args.calls,
                          "us": {s: summary(v) for s, v in us.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Q", type=int, default=16)
    ap.add_argument("--V", type=int, default=32)
    ap.add_argument("--max-batch", type=int, default=64)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--shapes", default="tacos_yml,anet_yml")
    ap.add_argument("--skip-search", action="store_true")
    args = ap.parse_args()
    import models
    A = models.vml_amd
    assert torch.cuda.is_available(), "video_rank_bench needs a HIP device"
    dev = torch.device("cuda:0")
    A._lib.load_torch()
    bench_kernels(A, args, dev)
    if not args.skip_search:
        bench_search(A, models, args, dev)


if __name__ == "__main__":
    main()
