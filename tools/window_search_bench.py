#!/usr/bin/env python3
"""Q queries against a corpus of V long videos, from a window bank against the loop a caller had before it, in one process
(INTEGRATION.md 3r):
  (a) banks: SMIN.search_windows over a prebuilt WindowBank and QueryBank (score_pairs per chunk from the banks, top_moments, one
             smin_merge_window_moments over the (query, video) groups, one smin_corpus_span_topk); building the two banks is timed on
             its own, once per run;
  (b) loop:  SMIN.localize_windows called once over all Q * V (query, video) pairs (video_index repeated: every pair samples, projects
             and encodes its windows and its query again), then a torch.topk over each query's V * k merged moments on the device --
             the only route before the banks.  The queries' rows are expanded to one per pair outside the timed region.
Shapes: tacos.yml and activitynet.yml, Q = 16 queries, V = 8 videos of about 7 windows each at the default window (T rows) and stride
(T / 2), k = 5, chunks of 64, forward_only_scoring on both sides.  After a warm-up of both, alternating blocks of the two; every timed
call lies between two HIP events (host issue time is inside them).  Then the ranking kernel alone -- 50 launches of
smin_corpus_span_topk back to back between two events, divided by 50 -- against moments.corpus_span_topk_torch on the device, at
(Q, groups per query, k_video, K) = (16, 8, 5, 5) and (1024, 64, 5, 25).
    python tools/window_search_bench.py [--calls 100] [--warmup 5] [--block 10] [--runs 2] [--shapes tacos_yml,anet_yml] [--no-kernel]
Prints one JSON line per shape and run -- the median and the 10-90 % spread of each side in microseconds, the time to build the banks,
each side's peak device memory over one call (and over the build) in bytes above what was allocated before it -- and one per kernel
shape and run.

With ``--prefilter M[,M...]`` the sides are instead: "banks", the search over all pairs as above; "pruned_M",
search_windows(prefilter=M) (``--trim``: trim=True) for each M; "first_stage", prefilter_videos alone over the Q x windows pairs; and
"expand", smin_window_expand's three launches alone (50 calls back to back between two events, divided by 50) at the largest M's
shape.  ``--corpus unequal`` replaces the corpus by 8 videos of 1, 2, 3, 5, 8, 13, 25 and 57 windows; the line then carries each M's
``cap`` and ``total``.  The loop side (b) and the ranking kernel are not run in this mode."""
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
CORPORA = {  # a video's rows in units of T, at window T and stride T / 2
    "equal": (4.0, 3.9, 4.15, 3.75, 4.0, 4.4, 3.5, 4.0),                 # 7 or 8 windows each
    "unequal": (1.0, 1.5, 2.0, 3.0, 4.5, 7.0, 13.0, 29.0),               # 1, 2, 3, 5, 8, 13, 25 and 57 windows
}


def summary(v):
    q = statistics.quantiles(v, n=10)
    return {"median": round(statistics.median(v), 2), "p10": round(q[0], 2), "p90": round(q[-1], 2), "spread": round(q[-1] - q[0], 2)}


def alternate(sides, calls, block):
    """{side: [microseconds per call]}: blocks of ``block`` calls of each side in turn, every call between two HIP events"""
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


def peak_bytes(fn):
    """peak device memory of one call of fn above what was allocated before it"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def span_lists(Q, per_query, kv, dev, seed):
    """merge_window_moments-shaped lists of Q * per_query groups with random scores and counts"""
    g = torch.Generator().manual_seed(seed)
    G2 = Q * per_query
    span = torch.rand(G2, kv, 2, generator=g) * 1000
    score = torch.rand(G2, kv, generator=g)
    window = torch.randint(0, 8, (G2, kv), generator=g, dtype=torch.int64)
    cell = torch.randint(0, 64, (G2, kv, 2), generator=g, dtype=torch.int64)
    count = torch.randint(0, kv + 1, (G2,), generator=g, dtype=torch.int32)
    video = (torch.arange(G2) % per_query).to(torch.int32)
    ptr = (torch.arange(Q + 1) * per_query).to(torch.int32)
    return [t.to(dev) for t in (span, score, window, cell, count, video, ptr)]


def pruned_mode(args, A, m, banks, side_a, prefilters, name, n_windows):
    """--prefilter: the search over all pairs against search_windows(prefilter=M), the first stage alone and the expand launches alone"""
    wb, qb = banks
    Q, V, mb, k, REP = len(qb), wb.n_videos, args.max_batch, args.k, 50
    sides, plan = {"banks": side_a}, {}
    for M in prefilters:
        sides[f"pruned_{M}"] = lambda M=M: m.search_windows(wb, qb, k=k, max_batch=mb, prefilter=M, trim=args.trim)
        r = sides[f"pruned_{M}"]()
        plan[str(M)] = {"cap": A.survivor_window_capacity(wb.video_ptr, min(M, V), Q), "total": int(r["window_pairs"])}
    M = max(prefilters)
    sides["first_stage"] = lambda: m.prefilter_videos(wb, qb, M)
    sel = m.prefilter_videos(wb, qb, M)["video"].to(torch.int32)
    cap = plan[str(M)]["cap"]
    want = A.expand_survivor_windows_torch(sel, wb.video_ptr_d, len(wb), cap)
    got = A.expand_survivor_windows(sel, wb.video_ptr_d, len(wb), cap)
    assert all(torch.equal(g, w) for g, w in zip(got, want)), "the kernel and its restatement disagree"

    def expand():                                                                          # REP calls back to back: the queue hides the host
        for _ in range(REP):
            A.expand_survivor_windows(sel, wb.video_ptr_d, len(wb), cap)

    for _ in range(args.warmup):
        for fn in sides.values():
            fn()
        expand()
    torch.cuda.synchronize()
    for run in range(args.runs):
        us = alternate(sides, args.calls, args.block)
        us["expand"] = [v / REP for v in alternate({"expand": expand}, max(args.calls // 5, 10), args.block)["expand"]]
        res = {s: summary(v) for s, v in us.items()}
        print(json.dumps({"shape": name, "run": run, "corpus": args.corpus, "Q": Q, "V": V, "windows": n_windows, "query_window_pairs": Q * n_windows,
                          "windows_per_video": (wb.video_ptr[1:] - wb.video_ptr[:-1]).tolist(), "max_batch": mb, "k": k, "trim": args.trim,
                          "gemm_mode": A.get_gemm_mode(), "calls": args.calls, "plan": plan, "us": res,
                          "pruned_over_banks": {str(M): round(res[f"pruned_{M}"]["median"] / res["banks"]["median"], 3) for M in prefilters}}),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Q", type=int, default=16)
    ap.add_argument("--max-batch", type=int, default=64)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--shapes", default="tacos_yml,anet_yml")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--prefilter", default="", help="M[,M...]: time search_windows(prefilter=M) against the search over all pairs")
    ap.add_argument("--trim", action="store_true", help="with --prefilter: trim=True (one host read per call)")
    ap.add_argument("--corpus", choices=sorted(CORPORA), default="equal")
    args = ap.parse_args()
    prefilters = [int(x) for x in args.prefilter.split(",") if x]
    ROWS = CORPORA[args.corpus]
    import models
    from oracle import smin_oracle as O
    from tests import helpers as H
    A = models.vml_amd
    assert torch.cuda.is_available(), "window_search_bench needs a HIP device"
    dev = torch.device("cuda:0")
    A._lib.load_torch()
    Q, mb, k, V = args.Q, args.max_batch, args.k, len(ROWS)
    for name in [s for s in args.shapes.split(",") if s]:
        T, L, C, D, dl, layers, Din, Nq, Hh = shape = SHAPES[name]
        m = models.SMIN(*shape, dev)
        m.load_state_dict(O.formula_state_dict(H.smin_shapes(*shape), gain=1.3))
        m = m.to(dev).eval()
        m.forward_only_scoring = True
        lengths = [int(r * T) for r in ROWS]
        g = torch.Generator().manual_seed(1)
        raw = torch.randn(sum(lengths), Din, generator=g).to(dev)
        qb_ = O.synthetic_batch(Q, T, L, Nq, Din, seed=2, with_labels=False)
        qf, qm = qb_["query_features"].to(dev), qb_["query_mask"].to(dev)
        vi = np.tile(np.arange(V), Q)
        qrows = torch.from_numpy(np.repeat(np.arange(Q), V)).to(dev)
        qf_pairs, qm_pairs = qf.index_select(0, qrows), qm.index_select(0, qrows)          # (b)'s queries, one row per pair
        video_of = torch.from_numpy(vi).to(dev).reshape(Q, V, 1).expand(Q, V, k).reshape(Q, V * k)
        n_windows = int(A.window_plan(lengths, T, T // 2)[2][-1])

        def build():
            return m.encode_windows(raw, lengths, max_batch=mb), m.encode_queries(qf, qm)

        banks = build()

        def side_a():
            return m.search_windows(*banks, k=k, max_batch=mb)

        def side_b():
            r = m.localize_windows(raw, lengths, qf_pairs, qm_pairs, video_index=vi, k=k, max_batch=mb)
            listed = torch.arange(k, device=dev).unsqueeze(0) < r["count"].to(torch.int64).unsqueeze(1)
            score = torch.where(listed, r["score"], torch.full_like(r["score"], float("-inf"))).reshape(Q, V * k)
            top = torch.topk(score, k, dim=1)
            span = r["span"].reshape(Q, V * k, 2).gather(1, top.indices.unsqueeze(-1).expand(Q, k, 2))
            return video_of.gather(1, top.indices), span, top.values

        if prefilters:
            pruned_mode(args, A, m, banks, side_a, prefilters, name, n_windows)
            del m, banks, raw, qf, qm, qf_pairs, qm_pairs
            torch.cuda.empty_cache()
            continue
        sides = {"banks": side_a, "loop": side_b}
        for _ in range(args.warmup):
            for fn in sides.values():
                fn()
        torch.cuda.synchronize()
        a, b = side_a(), side_b()
        agree = float((a["score"] - b[2]).abs().max())                                     # the two sides rank the same moments (up to rounding)
        peaks = {"build_banks": peak_bytes(build), "banks": peak_bytes(side_a), "loop": peak_bytes(side_b)}
        held = {"raw": 4 * raw.numel(), "window_bank_fv": 4 * banks[0].fv.numel(), "sampled_windows_not_kept": 4 * n_windows * T * Din}
        for run in range(args.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            build()
            e1.record()
            us = alternate(sides, args.calls, args.block)
            res = {s: summary(v) for s, v in us.items()}
            print(json.dumps({"shape": name, "run": run, "Q": Q, "V": V, "windows": n_windows, "query_window_pairs": Q * n_windows, "max_batch": mb, "k": k,
                              "gemm_mode": A.get_gemm_mode(), "calls": args.calls, "us": res, "build_banks_us": round(e0.elapsed_time(e1) * 1e3, 2),
                              "loop_over_banks": round(res["loop"]["median"] / res["banks"]["median"], 3), "peak_bytes": peaks, "held_bytes": held,
                              "max_score_difference": agree}), flush=True)
        del m, banks, raw, qf, qm, qf_pairs, qm_pairs, a, b
        torch.cuda.empty_cache()
    if args.no_kernel or prefilters:
        return
    L_, REP = A._lib, 50
    for Qk, per_query, kv, K, torch_calls in ((16, 8, 5, 5, 20), (1024, 64, 5, 25, 3)):
        lists = span_lists(Qk, per_query, kv, dev, seed=7)
        got, want = A.corpus_span_topk(*lists, k=K), A.corpus_span_topk_torch(*lists, k=K)
        assert all(torch.equal(got[key].view(torch.uint8), want[key].view(torch.uint8)) for key in got), "the kernel and its restatement disagree"
        outs = [torch.empty_like(got[key]) for key in ("video", "span", "score", "window", "cell", "count")]
        ptrs = [L_.ptr(t) for t in lists] + [Qk, kv, K] + [L_.ptr(t) for t in outs]

        def launches():                                                                    # REP launches back to back: the queue hides the host
            for _ in range(REP):
                L_.call("smin_corpus_span_topk", L_.stream(), *ptrs)

        for _ in range(args.warmup):
            launches()
        for run in range(args.runs):
            us = alternate({"kernel": launches}, max(args.calls // 2, 10), args.block)
            us["kernel"] = [v / REP for v in us["kernel"]]
            us.update(alternate({"torch": lambda: A.corpus_span_topk_torch(*lists, k=K)}, torch_calls, torch_calls))
            res = {s: summary(v) for s, v in us.items()}
            print(json.dumps({"kernel": "smin_corpus_span_topk", "run": run, "Q": Qk, "groups_per_query": per_query, "k_video": kv, "K": K,
                              "launches_per_sample": REP, "us": res, "torch_over_kernel": round(res["torch"]["median"] / res["kernel"]["median"], 1)}), flush=True)

if __name__ == "__main__":
    main()
