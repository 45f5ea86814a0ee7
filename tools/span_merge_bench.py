#!/usr/bin/env python3
"""Times the merge of span-valued search results across shards on the device, run by hand:
  merge_search_windows of S = 2 and S = 16 ranked span lists of 64 entries (counts in 32 .. 64) at Q = 1024 queries, K = 64, against
    (b) cat + corpus_span_topk: the only device route there was before -- the lists concatenated into one-slot groups (torch.cat, the
        global video ids and the counts as per-group flags formed by torch ops) and smin_corpus_span_topk at k_video = 1;
    (c) host: the lists copied to the host and merged by a Python loop (merge_search_windows_torch on .cpu() lists);
  and, beside it, merge_search on cell lists of the same shape: the K-round loop against the one-pass rank.
    python tools/span_merge_bench.py [--calls 20] [--warmup 3] [--runs 2] [--limit 300]
bench_corpus_eval's method: every figure is the median of --calls timed calls after --warmup, each call between two device
synchronisations on the host clock (host issue time is inside), with the 10 % and 90 % quantiles; each figure runs under a time limit
of its own: SIGALRM, left at its default action, ends the process --limit seconds after the figure began.  The three sides are compared
once per S and must give the same list, bit for bit.  The whole set is measured --runs times.  Prints one JSON line per figure,
microseconds."""
import argparse
import json
import os
import signal
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KEYS = ("video", "span", "score", "window", "cell", "count")


def ranked_lists(S, Q, ks, videos, seed, dev):
    """S span lists ordered as search_windows orders them (scores descending per query, ties improbable) and the cell lists of the same
    scores, videos and counts: videos of the shard, counts in [ks/2, ks]"""
    g = torch.Generator().manual_seed(seed)
    spans, cells = [], []
    for _ in range(S):
        score = torch.rand(Q, ks, generator=g).sort(dim=1, descending=True).values
        video = torch.randint(0, videos, (Q, ks), generator=g, dtype=torch.int64)
        count = torch.randint(ks // 2, ks + 1, (Q,), generator=g, dtype=torch.int32)
        cell = torch.randint(0, 64, (Q, ks, 2), generator=g, dtype=torch.int64)
        r = {"video": video, "span": torch.rand(Q, ks, 2, generator=g) * 100, "score": score, "window": torch.randint(0, 9, (Q, ks), generator=g, dtype=torch.int64),
             "cell": cell, "count": count}
        spans.append({key: v.to(dev) for key, v in r.items()})
        cells.append({"video": spans[-1]["video"], "idx": spans[-1]["cell"], "score": spans[-1]["score"], "count": spans[-1]["count"]})
    return spans, cells


def cat_span_topk(A, lists, offsets, K):
    """(b): every candidate a group of one slot, query-major, through corpus_span_topk"""
    Q, ks = lists[0]["score"].shape
    S = len(lists)
    cat = lambda key, *tail: torch.cat([r[key] for r in lists], dim=1).reshape(-1, 1, *tail)
    video = torch.cat([r["video"] + off for r, off in zip(lists, offsets)], dim=1).reshape(-1).to(torch.int32)
    slot = torch.arange(ks, device=video.device).unsqueeze(0)
    count = torch.cat([slot < r["count"].unsqueeze(1) for r in lists], dim=1).reshape(-1).to(torch.int32)
    ptr = torch.arange(Q + 1, device=video.device, dtype=torch.int32) * (S * ks)
    return A.corpus_span_topk(cat("span", 2), cat("score"), cat("window"), cat("cell", 2), count, video, ptr, k=K)


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


def same(a, b):
    return all(torch.equal(a[key].cpu().contiguous().view(torch.uint8), b[key].cpu().contiguous().view(torch.uint8)) for key in KEYS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Q", type=int, default=1024)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--limit", type=int, default=300)
    args = ap.parse_args()
    if args.calls < 20:
        ap.error("a figure is the median of at least 20 timed calls")
    import models
    A = models.vml_amd
    assert torch.cuda.is_available(), "span_merge_bench measures on a HIP device"
    dev = torch.device("cuda:0")
    Q, k = args.Q, args.k
    for run in range(args.runs):
        for S in (2, 16):
            lists, cells = ranked_lists(S, Q, k, 1000, seed=S, dev=dev)
            offsets = [1000 * s for s in range(S)]
            host = lambda: A.merge_search_windows_torch([{key: v.cpu() for key, v in r.items()} for r in lists], offsets, k=k)
            got = A.merge_search_windows(lists, offsets, k=k)
            assert same(got, cat_span_topk(A, lists, offsets, k)), "merge_search_windows and cat + corpus_span_topk disagree"
            assert same(got, host()), "merge_search_windows and the host loop disagree"
            shape = dict(run=run, S=S, Q=Q, k_list=k, K=k)
            timed("merge_search_windows", lambda: A.merge_search_windows(lists, offsets, k=k), args.calls, args.warmup, args.limit, **shape)
            timed("cat+corpus_span_topk", lambda: cat_span_topk(A, lists, offsets, k), args.calls, args.warmup, args.limit, **shape)
            timed("merge_search (cell lists)", lambda: A.merge_search(cells, offsets, k=k), args.calls, args.warmup, args.limit, **shape)
            timed("host loop", host, args.calls, args.warmup, args.limit, **shape)


if __name__ == "__main__":
    main()
