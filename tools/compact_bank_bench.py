#!/usr/bin/env python3
"""Compact video banks against the fp32 bank, in one process, for storage = fp32 / bf16 / int8:
  (a) per model shape (tacos.yml, activitynet.yml; Q = 16 queries, V = 32 videos, chunks of 64 pairs, forward_only_scoring):
      the bank's bytes, SMIN.encode_videos(storage=...) and, alone, VideoBank.compact(storage); SMIN.search and SMIN.search(prefilter=8)
      over the bank, with the peak device memory of one call of each; and how far the code moves the results on these synthetic
      inputs -- max |delta| of score_pairs' four tensors against the fp32 bank, and the share of each query's top-k (video, start, end)
      that the fp32 search lists as well (mean and minimum over the queries).  No real data is read: this is no accuracy figure.
  (b) the first stage alone at (Q, V) = (16, 4096) and (1024, 1024), T = 128, L = 32, D = 512, random banks: moments.prefilter_scores on
      the fp32 bank, on the codes (the loader decodes inside the contraction) and as bank_decode followed by prefilter_scores on
      the decoded bank (what a caller without the fused loader would do).
After a warm-up of every side, alternating blocks of the sides; every timed call lies between two HIP events (host issue time is
inside them).
    python tools/compact_bank_bench.py [--calls 60] [--warmup 5] [--block 10] [--stage-calls 20] [--shapes tacos_yml,anet_yml] [--skip-stage]
Prints one JSON line per shape and one per first-stage size: medians and 10-90 % spreads in microseconds, bytes, drifts."""
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
STORAGES = ("fp32", "bf16", "int8")
STAGE_SIZES = ((16, 4096), (1024, 1024))


def summary(v):
    q = statistics.quantiles(v, n=10)
    return {"median": round(statistics.median(v), 2), "p10": round(q[0], 2), "p90": round(q[-1], 2), "spread": round(q[-1] - q[0], 2)}


def timed_blocks(sides, calls, warmup, block):
    """{side: summary of microseconds per call}: a warm-up of every side, then alternating blocks, each call between two events"""
    for _ in range(warmup):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    stamps, done = [], 0
    while done < calls:
        n = min(block, calls - done)
        for side, fn in sides.items():
            for _ in range(n):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                stamps.append((side, a, b))
        done += n
    torch.cuda.synchronize()
    us = {s: [] for s in sides}
    for side, a, b in stamps:
        us[side].append(a.elapsed_time(b) * 1e3)
    return {s: summary(v) for s, v in us.items()}


def peak_bytes(fn):
    """the peak of torch's allocator over one call, above what was allocated before it"""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def topk_overlap(got, want):
    """per query, the share of got's listed (video, start, end) entries that want lists too: (mean, min) over the queries"""
    shares = []
    for q in range(got["video"].shape[0]):
        key = lambda r, n: {(int(r["video"][q, i]), int(r["idx"][q, i, 0]), int(r["idx"][q, i, 1])) for i in range(n)}
        a, b = key(got, int(got["count"][q])), key(want, int(want["count"][q]))
        shares.append(len(a & b) / max(len(a), 1))
    return round(sum(shares) / len(shares), 4), round(min(shares), 4)


def model_shape(A, name, args, dev):
    import models
    from oracle import smin_oracle as O
    from tests import helpers as H
    import numpy as np
    T, L, C, D, dl, layers, Din, Nq, Hh = shape = SHAPES[name]
    Q, V, mb, k = args.Q, args.V, args.max_batch, args.k
    m = models.SMIN(*shape, dev)
    m.load_state_dict(O.formula_state_dict(H.smin_shapes(*shape), gain=1.3))
    m = m.to(dev).eval()
    m.forward_only_scoring = True
    vb_ = {k_: v.to(dev) for k_, v in O.synthetic_batch(V, T, L, Nq, Din, seed=1, with_labels=False).items()}
    qb_ = {k_: v.to(dev) for k_, v in O.synthetic_batch(Q, T, L, Nq, Din, seed=2, with_labels=False).items()}
    vid = [vb_[key] for key in ("video_features", "video_mask", "length_mask", "moment_mask")]
    qb = m.encode_queries(qb_["query_features"], qb_["query_mask"])
    counts = vb_["moment_mask"].reshape(V, -1).sum(1).tolist()
    banks = {s: m.encode_videos(*vid, cell_counts=counts, storage=s) for s in STORAGES}
    out = {"shape": name, "Q": Q, "V": V, "max_batch": mb, "k": k, "gemm_mode": A.get_gemm_mode(), "calls": args.calls,
           "bank_bytes": {s: b.nbytes for s, b in banks.items()}}
    out["encode_videos_us"] = timed_blocks({s: (lambda s=s: m.encode_videos(*vid, cell_counts=counts, storage=s)) for s in STORAGES},
                                           args.calls, args.warmup, args.block)
    out["compact_us"] = timed_blocks({s: (lambda s=s: banks["fp32"].compact(s)) for s in STORAGES[1:]}, args.calls, args.warmup, args.block)
    out["search_us"] = timed_blocks({s: (lambda s=s: m.search(banks[s], qb, k=k, max_batch=mb)) for s in STORAGES}, args.calls, args.warmup, args.block)
    out["search_prefilter8_us"] = timed_blocks({s: (lambda s=s: m.search(banks[s], qb, k=k, max_batch=mb, prefilter=8)) for s in STORAGES},
                                               args.calls, args.warmup, args.block)
    out["search_peak_bytes"] = {s: peak_bytes(lambda s=s: m.search(banks[s], qb, k=k, max_batch=mb)) for s in STORAGES}
    out["search_prefilter8_peak_bytes"] = {s: peak_bytes(lambda s=s: m.search(banks[s], qb, k=k, max_batch=mb, prefilter=8)) for s in STORAGES}
    # drift on these synthetic inputs, against the fp32 bank
    qi, vi = np.repeat(np.arange(Q), V), np.tile(np.arange(V), Q)
    scores = {s: [torch.cat([t.double() for t in parts]) for parts in
                  zip(*[m.score_pairs(banks[s], qb, vi[c:c + mb], qi[c:c + mb]) for c in range(0, Q * V, mb)])] for s in STORAGES}
    lists = {s: {key: v.cpu() for key, v in m.search(banks[s], qb, k=k, max_batch=mb).items()} for s in STORAGES}
    pruned = {s: {key: v.cpu() for key, v in m.search(banks[s], qb, k=k, max_batch=mb, prefilter=8).items()} for s in STORAGES}
    out["drift"] = {}
    for s in STORAGES[1:]:
        d = {key: float((a - b).abs().max()) for key, a, b in zip(("pm", "ps", "pe", "pa"), scores[s], scores["fp32"])}
        d["topk_overlap_mean_min"] = topk_overlap(lists[s], lists["fp32"])
        d["topk_overlap_prefilter8_mean_min"] = topk_overlap(pruned[s], pruned["fp32"])
        d["prefilter8_same_videos"] = round(float((pruned[s]["prefilter_video"] == pruned["fp32"]["prefilter_video"]).all(dim=1).float().mean()), 4)
        out["drift"][s] = d
    print(json.dumps(out), flush=True)


def first_stage(A, Q, V, args, dev):
    T, L, C, D = 128, 32, 4, 512
    g = torch.Generator().manual_seed(Q + V)
    fv = torch.randn(V, T, D, generator=g).to(dev)
    fs = torch.randn(Q, D, generator=g).to(dev)
    w, b = (torch.randn(3, D, generator=g) / D ** 0.5).to(dev), (torch.randn(3, generator=g) / 2).to(dev)
    lm = torch.ones(V, L, dtype=torch.bool, device=dev)
    mm = torch.triu(torch.ones(L, L, dtype=torch.bool, device=dev)).unsqueeze(0).expand(V, L, L).contiguous()
    run = lambda bank, scale=None: A.prefilter_scores(bank, fs, w, b, lm, mm, T, L, C, 0.1, fv_scale=scale)
    codes = {s: A.bank_encode(fv, s) for s in STORAGES[1:]}
    sides = {"fp32": lambda: run(fv)}
    for s, (c, sc) in codes.items():
        sides[s + "_fused"] = lambda c=c, sc=sc: run(c, sc)
        sides[s + "_decode_then_fp32"] = lambda c=c, sc=sc: run(A.bank_decode(c, sc))
    res = timed_blocks(sides, args.stage_calls, args.warmup, max(1, min(args.block, args.stage_calls)))
    same = {s: all(torch.equal(x, y) for x, y in zip(run(c, sc), run(A.bank_decode(c, sc)))) for s, (c, sc) in codes.items()}
    drift = {s: float((run(c, sc)[0] - run(fv)[0]).abs().max()) for s, (c, sc) in codes.items()}
    print(json.dumps({"first_stage": {"Q": Q, "V": V, "T": T, "L": L, "D": D}, "gemm_mode": A.get_gemm_mode(), "calls": args.stage_calls,
                      "bank_bytes": {"fp32": fv.numel() * 4, **{s: c.numel() * c.element_size() + (0 if sc is None else sc.numel() * 4) for s, (c, sc) in codes.items()}},
                      "us": res, "fused_equals_decoded_bits": same, "score_max_abs_delta_vs_fp32": drift}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Q", type=int, default=16)
    ap.add_argument("--V", type=int, default=32)
    ap.add_argument("--max-batch", type=int, default=64)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--stage-calls", type=int, default=20)
    ap.add_argument("--shapes", default="tacos_yml,anet_yml")
    ap.add_argument("--skip-stage", action="store_true")
    args = ap.parse_args()
    import models
    A = models.vml_amd
    assert torch.cuda.is_available(), "compact_bank_bench needs a HIP device"
    dev = torch.device("cuda:0")
    A._lib.load_torch()
    with torch.no_grad():
        for name in [n for n in args.shapes.split(",") if n]:
            model_shape(A, name, args, dev)
            torch.cuda.empty_cache()
        if not args.skip_stage:
            for Q, V in STAGE_SIZES:
                first_stage(A, Q, V, args, dev)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
