#!/usr/bin/env python3
"""Times the weighted merge of sharded search results on the device, run by hand:
  (a) merge:  S = 2 and S = 16 carry lists of 64 span entries (counts in 32 .. 64, 64 videos a list) at Q = 1024 queries, K = 64:
        merge_search_windows_weighted         the whole call: the cat of the pooled matrices, smin_video_rank over the S * 64 videos,
                                              one smin_span_search_merge_weighted;
        merge_kernel                          that one launch alone, the video tables given;
        cat+torch+corpus_span_topk            the only device route there was before, the video tables given as well: the lists
                                              concatenated into one-slot groups, the weights gathered and the cut applied by torch ops,
                                              smin_corpus_span_topk at k_video = 1;
        merge_search_windows                  the plain merge of the same lists: what the counting costs over the binary search.
      The first three give the same list, bit for bit, which is checked before any timing.
  (b) search: one weighted sharded search at 3m's shape -- 16 queries x 32 videos in 4 shards of 8, tacos.yml, chunks of 64 pairs,
      forward_only_scoring -- by training.search_shards_weighted against the one-bank search(video_weight=7.5, max_videos=8): time per
      call and the peak of torch's allocator over the call.
    python tools/weighted_merge_bench.py [--calls 20] [--warmup 3] [--runs 2] [--limit 300] [--skip-search]
span_merge_bench's method: every figure is the median of --calls timed calls after --warmup, each call between two device
synchronisations on the host clock (host issue time is inside), with the 10 % and 90 % quantiles; each figure runs under a time limit
of its own: SIGALRM, left at its default action, ends the process --limit seconds after the figure began.  The whole set is measured
--runs times.  Prints one JSON line per figure, microseconds."""
import argparse
import json
import os
import signal
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KEYS = ("video", "span", "score", "window", "cell", "count")
TACOS = (128, 32, 4, 512, 128, 3, 4096, 14, 256)        # T, L, C, D, dl, layers, Din, Nq, H  (BASELINE.json configs)
ALPHA, TAU = 7.5, 0.1


def carry_lists(S, Q, ks, videos, seed, dev):
    """S carry lists in search_windows' order under their own (shard) weights: raw scores descending per query, ties improbable"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(S):
        raw = torch.rand(Q, ks, generator=g).sort(dim=1, descending=True).values
        r = {"video": torch.randint(0, videos, (Q, ks), generator=g, dtype=torch.int64), "span": torch.rand(Q, ks, 2, generator=g) * 100,
             "score": raw, "raw": raw, "window": torch.randint(0, 9, (Q, ks), generator=g, dtype=torch.int64),
             "cell": torch.randint(0, 64, (Q, ks, 2), generator=g, dtype=torch.int64),
             "count": torch.randint(ks // 2, ks + 1, (Q,), generator=g, dtype=torch.int32),
             "pair_score": torch.rand(Q, videos, generator=g), "pair_cells": torch.full((Q, videos), 7.0)}
        out.append({key: v.to(dev) for key, v in r.items()})
    return out


def cat_torch_topk(A, lists, offsets, K, rank, weight, cut):
    """every candidate a group of one slot, query-major: value and cut by torch ops, then corpus_span_topk"""
    Q, ks = lists[0]["raw"].shape
    S, dev = len(lists), rank.device
    cat = lambda key, *tail: torch.cat([r[key] for r in lists], dim=1).reshape(-1, 1, *tail)
    g = torch.cat([r["video"] + off for r, off in zip(lists, offsets)], dim=1)                  # (Q, S * ks)
    slot = torch.arange(ks, device=dev).unsqueeze(0)
    listed = torch.cat([slot < r["count"].unsqueeze(1) for r in lists], dim=1)
    vr = torch.gather(rank, 1, g)
    keep = listed & (vr >= 0) & (vr < cut)
    value = torch.cat([r["raw"] for r in lists], dim=1) * torch.gather(weight, 1, g)
    ptr = torch.arange(Q + 1, device=dev, dtype=torch.int32) * (S * ks)
    return A.corpus_span_topk(cat("span", 2), value.reshape(-1, 1), cat("window"), cat("cell", 2), keep.reshape(-1).to(torch.int32),
                              g.reshape(-1).to(torch.int32), ptr, k=K)


def timed(name, fn, calls, warmup, limit, **extra):
    signal.alarm(limit)                                         # the figure's own time limit: the default action ends the process
    for _ in range(warmup):
        fn()
    us = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) * 1e6)
    signal.alarm(0)
    q = statistics.quantiles(us, n=10)
    line = dict(figure=name, median_us=round(statistics.median(us), 1), p10_us=round(q[0], 1), p90_us=round(q[-1], 1), calls=calls, **extra)
    print(json.dumps(line), flush=True)
    return line


def same(a, b, keys=KEYS):
    return all(torch.equal(a[key].cpu().contiguous().view(torch.uint8), b[key].cpu().contiguous().view(torch.uint8)) for key in keys)


def bench_merge(A, args, dev):
    M = A.moments
    Q, k, videos, cut = args.Q, args.k, 64, 48
    for run in range(args.runs):
        for S in (2, 16):
            lists = carry_lists(S, Q, k, videos, seed=S, dev=dev)
            offsets = [videos * s for s in range(S)]
            V = videos * S
            kw = dict(k=k, video_weight=ALPHA, max_videos=cut, n_videos=5)
            got = A.merge_search_windows_weighted(lists, offsets, **kw)
            vr = A.rank_videos(got["pair_score"].reshape(-1), got["pair_cells"].reshape(-1), torch.arange(V, dtype=torch.int32, device=dev).repeat(Q),
                               torch.arange(Q + 1, dtype=torch.int32, device=dev) * V, n=5, alpha=ALPHA)
            rank, weight = vr["pair_rank"].reshape(Q, V), vr["weight"].reshape(Q, V)
            kernel = lambda: M._merge_weighted("bench", lists, offsets, Q, k, M._WEIGHTED_SPAN_FIELDS, rank, weight, V, cut)
            rank64 = rank.to(torch.int64)
            assert same(got, kernel(), KEYS + ("raw",)), "the whole call and the launch alone disagree"
            assert same(got, cat_torch_topk(A, lists, offsets, k, rank64, weight, cut)), "the weighted merge and cat + torch + corpus_span_topk disagree"
            shape = dict(run=run, S=S, Q=Q, k_list=k, K=k, V=V, max_videos=cut)
            timed("merge_search_windows_weighted", lambda: A.merge_search_windows_weighted(lists, offsets, **kw), args.calls, args.warmup, args.limit, **shape)
            timed("merge_kernel", kernel, args.calls, args.warmup, args.limit, **shape)
            timed("cat+torch+corpus_span_topk", lambda: cat_torch_topk(A, lists, offsets, k, rank64, weight, cut), args.calls, args.warmup, args.limit, **shape)
            timed("merge_search_windows", lambda: A.merge_search_windows(lists, offsets, k=k), args.calls, args.warmup, args.limit, **shape)


def bench_search(A, models, args, dev):
    from oracle import smin_oracle as O
    from tests import helpers as H
    Q, V, shards, mb, k, kv = 16, 32, 4, 64, 5, 5
    T, L, C, D, dl, layers, Din, Nq, Hh = TACOS
    m = models.SMIN(*TACOS, dev)
    m.load_state_dict(O.formula_state_dict(H.smin_shapes(*TACOS), gain=1.3))
    m = m.to(dev).eval()
    m.forward_only_scoring = True
    keys = ("video_features", "video_mask", "length_mask", "moment_mask")
    vb_ = {k_: v.to(dev) for k_, v in O.synthetic_batch(V, T, L, Nq, Din, seed=1, with_labels=False).items()}
    qb_ = {k_: v.to(dev) for k_, v in O.synthetic_batch(Q, T, L, Nq, Din, seed=2, with_labels=False).items()}
    queries = m.encode_queries(qb_["query_features"], qb_["query_mask"])
    whole = m.encode_videos(*[vb_[key] for key in keys])
    per = V // shards
    parts = [dict({key: vb_[key][s * per:(s + 1) * per] for key in keys}, duration=np.ones(per), cell_counts=whole.cell_counts[s * per:(s + 1) * per])
             for s in range(shards)]
    kw = dict(k=k, k_video=kv, max_batch=mb, video_weight=ALPHA, max_videos=8, tau=TAU)

    def one_bank():                                              # encodes too: the sharded route cannot keep its banks
        bank = m.encode_videos(*[vb_[key] for key in keys], cell_counts=whole.cell_counts)
        return m.search(bank, queries, **kw)

    def sharded():
        return A.search_shards_weighted(m, parts, queries, **kw)[0]

    a, b = one_bank(), sharded()
    diff = (a["score"] - b["score"]).abs().max().item()
    print(json.dumps({"bench": "search", "check": "sharded against one bank", "max_score_difference": diff,
                      "same_videos": bool(torch.equal(a["video"], b["video"]))}), flush=True)
    for run in range(args.runs):
        for name, fn in (("search one bank", one_bank), ("search_shards_weighted", sharded)):
            fn()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            fn()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated(dev) - base
            timed(name, fn, args.calls, args.warmup, args.limit, run=run, shape="tacos_yml", Q=Q, V=V, shards=shards if fn is sharded else 1,
                  max_batch=mb, k=k, k_video=kv, carry_slots=A.moments.carry_slots(k, kv, 8), peak_bytes_over_call=int(peak))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Q", type=int, default=1024)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--skip-search", action="store_true")
    args = ap.parse_args()
    if args.calls < 20:
        ap.error("a figure is the median of at least 20 timed calls")
    import models
    A = models.vml_amd
    assert torch.cuda.is_available(), "weighted_merge_bench measures on a HIP device"
    dev = torch.device("cuda:0")
    A._lib.load_torch()
    bench_merge(A, args, dev)
    if not args.skip_search:
        bench_search(A, models, args, dev)


if __name__ == "__main__":
    main()
