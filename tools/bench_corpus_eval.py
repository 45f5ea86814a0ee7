#!/usr/bin/env python3
"""Times the evaluation side of corpus search on the device, run by hand:
  merge_search of S = 2 and S = 16 ranked lists of 64 entries at Q = 1024 queries, K = 64, against
    (a) cat + corpus_topk: the route it replaces with code that was there before -- the lists concatenated into one-entry pairs
        (torch.cat, the global video ids and the counts as per-pair flags formed by torch ops) and smin_corpus_topk at k_video = 1;
    (b) host: the lists copied to the host and merged by a Python loop (merge_search_torch on .cpu() lists);
  CorpusMeter.update at Q = 1024, k = 64 against CorpusMeterTorch on the device (torch ops, one host read per update).
    python tools/bench_corpus_eval.py [--calls 20] [--warmup 3] [--limit 300]
Every figure is the median of --calls timed calls after --warmup, each call between two device synchronisations on the host clock
(host issue time is inside).  Each figure runs under a time limit of its own: SIGALRM, left at its default action, ends the process
--limit seconds after the figure began.  merge_search and (a) are compared once per S and must give the same list.
Prints one JSON line per figure, microseconds."""
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
KEYS = ("video", "idx", "score", "count")


def ranked_lists(S, Q, ks, videos, seed, dev):
    """S lists ordered as search orders them: scores descending per query (ties improbable), videos of the shard, counts in [ks/2, ks]"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(S):
        score = torch.rand(Q, ks, generator=g).sort(dim=1, descending=True).values
        r = {"video": torch.randint(0, videos, (Q, ks), generator=g, dtype=torch.int64), "idx": torch.randint(0, 64, (Q, ks, 2), generator=g, dtype=torch.int64),
             "score": score, "count": torch.randint(ks // 2, ks + 1, (Q,), generator=g, dtype=torch.int32)}
        out.append({key: v.to(dev) for key, v in r.items()})
    return out


def cat_topk(A, lists, offsets, K):
    """(a): every candidate a pair of one entry, query-major, through corpus_topk"""
    Q, ks = lists[0]["score"].shape
    S = len(lists)
    score = torch.cat([r["score"] for r in lists], dim=1).reshape(-1, 1)
    idx = torch.cat([r["idx"] for r in lists], dim=1).reshape(-1, 1, 2)
    video = torch.cat([r["video"] + off for r, off in zip(lists, offsets)], dim=1).reshape(-1).to(torch.int32)
    slot = torch.arange(ks, device=score.device).unsqueeze(0)
    count = torch.cat([slot < r["count"].unsqueeze(1) for r in lists], dim=1).reshape(-1).to(torch.int32)
    ptr = torch.arange(Q + 1, device=score.device, dtype=torch.int32) * (S * ks)
    return A.corpus_topk(score, idx, count, video, ptr, k=K)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Q", type=int, default=1024)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300)
    args = ap.parse_args()
    if args.calls < 20:
        ap.error("a figure is the median of at least 20 timed calls")
    import models
    A = models.vml_amd
    assert torch.cuda.is_available(), "bench_corpus_eval measures on a HIP device"
    dev = torch.device("cuda:0")
    Q, k = args.Q, args.k
    for S in (2, 16):
        lists = ranked_lists(S, Q, k, 1000, seed=S, dev=dev)
        offsets = [1000 * s for s in range(S)]
        got, want = A.merge_search(lists, offsets, k=k), cat_topk(A, lists, offsets, k)
        assert all(torch.equal(got[key], want[key]) for key in KEYS), "merge_search and cat + corpus_topk disagree"
        shape = dict(S=S, Q=Q, k_list=k, K=k)
        timed("merge_search", lambda: A.merge_search(lists, offsets, k=k), args.calls, args.warmup, args.limit, **shape)
        timed("cat+corpus_topk", lambda: cat_topk(A, lists, offsets, k), args.calls, args.warmup, args.limit, **shape)
        timed("host loop", lambda: A.merge_search_torch([{key: v.cpu() for key, v in r.items()} for r in lists], offsets, k=k), args.calls, 1,
              args.limit, **shape)
    g = torch.Generator().manual_seed(5)
    result = ranked_lists(1, Q, k, 50, seed=9, dev=dev)[0]
    st = torch.rand(Q, k, generator=g) * 100
    result["times"] = torch.stack([st, st + torch.rand(Q, k, generator=g) * 30 + 1], dim=2).to(dev)
    gt_video = torch.randint(0, 50, (Q,), generator=g, dtype=torch.int64).to(dev)
    gs = torch.rand(Q, generator=g) * 100
    gt = torch.stack([gs, gs + torch.rand(Q, generator=g) * 30 + 1], dim=1).to(dev)
    a, b = A.CorpusMeter(device=dev), A.CorpusMeterTorch(device=dev)
    a.update(result, gt_video, gt)
    b.update(result, gt_video, gt)
    assert torch.equal(a.state, b.state), "CorpusMeter and CorpusMeterTorch disagree"
    timed("CorpusMeter.update", lambda: a.update(result, gt_video, gt), args.calls, args.warmup, args.limit, Q=Q, k=k)
    timed("CorpusMeterTorch.update", lambda: b.update(result, gt_video, gt), args.calls, args.warmup, args.limit, Q=Q, k=k)


if __name__ == "__main__":
    main()
