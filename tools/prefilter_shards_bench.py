#!/usr/bin/env python3
"""What the corpus-wide first-stage cut over shards costs and saves, in one process:
  (a) search:  Q = 16 queries over V = 32 videos that come in 4 shards, prefilter=8:
               `shards_prefiltered`  training.search_shards_prefiltered -- per shard encode_videos + fold_survivors, then one
                                     search_survivors (the full model on Q * 8 pairs);
               `shards_unpruned`     training.search_shards over the same shards, every pair through the full model: the only route
                                     for a sharded corpus before;
               `one_bank_prefilter`  encode_videos of all 32 videos + search(prefilter=8): the route of 3v where the corpus fits in
                                     one bank (`one_bank_search_only`: the same without the encoding, as 3v's table times it);
               with each side's peak of torch's allocator over the call;
  (b) launches: moments.prefilter_fold and moments.survivors_admit alone on random scores and banks at (Q, Vs, M) = (16, 32, 8) and
               (1024, 1024, 100), next to prefilter_scores on the same shard.  The fold starts from the state one earlier shard of Vs
               videos leaves (`fold`, `admit`: the steady state, about half the slots change hands on random scores) and from the
               empty state (`fold_first`, `admit_first`: every slot is filled).
Shapes: tacos.yml and activitynet.yml (BASELINE.json configs), chunks of 64 pairs, forward_only_scoring (3m's and 3v's shape).
After a warm-up of all sides, alternating blocks; every timed call lies between two HIP events (host issue time is inside them).
    python tools/prefilter_shards_bench.py [--calls 100] [--big-calls 10] [--warmup 10] [--block 10] [--runs 2] [--shapes tacos_yml,anet_yml]
                                           [--skip-search] [--skip-big] [--skip-launches] [--full-length]
Prints one JSON line per shape, size and run: the median and the 10-90 % spread of each side in microseconds."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.prefilter_bench import SHAPES, TAU, KEEP, peak_mb, summary, timed_blocks  # noqa: E402

VIDEO_KEYS = ("video_features", "video_mask", "length_mask", "moment_mask")


def bench_search(A, models, args, dev):
    from oracle import smin_oracle as O
    from tests import helpers as H
    Q, V, mb, k, S = args.Q, args.V, args.max_batch, args.k, args.shards
    edges = [V * s // S for s in range(S + 1)]
    for name in args.shapes.split(","):
        T, L, C, D, dl, layers, Din, Nq, Hh = shape = SHAPES[name]
        m = models.SMIN(*shape, dev)
        m.load_state_dict(O.formula_state_dict(H.smin_shapes(*shape), gain=1.3))
        m = m.to(dev).eval()
        m.forward_only_scoring = True
        vb_ = {k_: v.to(dev) for k_, v in O.synthetic_batch(V, T, L, Nq, Din, seed=1, with_labels=False, full_length=args.full_length).items()}
        qb_ = {k_: v.to(dev) for k_, v in O.synthetic_batch(Q, T, L, Nq, Din, seed=2, with_labels=False).items()}
        whole = [vb_[key] for key in VIDEO_KEYS]
        vb, qb = m.encode_videos(*whole), m.encode_queries(qb_["query_features"], qb_["query_mask"])
        counts = vb.cell_counts
        shards = [dict({key: vb_[key][a:b] for key in VIDEO_KEYS}, duration=np.ones(b - a), cell_counts=counts[a:b]) for a, b in zip(edges[:-1], edges[1:])]
        sides = {"shards_prefiltered": lambda: A.search_shards_prefiltered(m, shards, qb, prefilter=KEEP, k=k, k_video=k, max_batch=mb, tau=TAU)[0],
                 "shards_unpruned": lambda: A.training.search_shards(m, shards, qb, k=k, k_video=k, max_batch=mb)[0],
                 "one_bank_prefilter": lambda: m.search(m.encode_videos(*whole, cell_counts=counts), qb, k=k, max_batch=mb, prefilter=KEEP, tau=TAU),
                 "one_bank_search_only": lambda: m.search(vb, qb, k=k, max_batch=mb, prefilter=KEEP, tau=TAU)}
        got, want, full = sides["shards_prefiltered"](), sides["one_bank_search_only"](), sides["shards_unpruned"]()
        same = all(torch.equal(got[key].view(torch.uint8), want[key].view(torch.uint8)) for key in ("video", "idx", "score", "count", "prefilter_video", "prefilter_score"))
        top1 = (full["video"][:, 0] == got["video"][:, 0]).float().mean().item()     # (synthetic inputs, formula weights: no recall claim)
        mem = {s: peak_mb(fn) for s, fn in sides.items()}
        for run in range(args.runs):
            us = timed_blocks(sides, args.calls, args.warmup, args.block)
            res = {s: summary(v) for s, v in us.items()}
            print(json.dumps({"bench": "search", "shape": name, "run": run, "Q": Q, "V": V, "shards": S, "keep": KEEP, "max_batch": mb, "k": k,
                              "equal_cell_counts": len(set(counts)) == 1, "gemm_mode": A.get_gemm_mode(), "calls": args.calls, "us": res,
                              "peak_mb": mem, "bits_equal_one_bank": same, "same_top1_video_share": round(top1, 4),
                              "prefiltered_over_unpruned": round(res["shards_prefiltered"]["median"] / res["shards_unpruned"]["median"], 4),
                              "prefiltered_over_one_bank": round(res["shards_prefiltered"]["median"] / res["one_bank_prefilter"]["median"], 4)}), flush=True)
        del m, vb, qb, vb_, qb_, shards, whole
        torch.cuda.empty_cache()


def bench_launches(A, args, dev):
    g = torch.Generator().manual_seed(13)
    sizes = [(16, 32, KEEP, args.calls, args.warmup)] + ([] if args.skip_big else [(1024, 1024, 100, args.big_calls, 2)])
    for name in args.shapes.split(","):
        T, L, C, D = SHAPES[name][:4]
        for Q, Vs, M, calls, warmup in sizes:
            fv, fs = torch.randn(Vs, T, D, generator=g).to(dev), torch.randn(Q, D, generator=g).to(dev)
            w, b = (torch.randn(3, D, generator=g) / D ** 0.5).to(dev), (torch.randn(3, generator=g) / 2).to(dev)
            lm = torch.ones(Vs, L, dtype=torch.bool, device=dev)
            mm = torch.triu(torch.ones(L, L, dtype=torch.bool, device=dev)).expand(Vs, L, L).contiguous()
            vm = torch.ones(Vs, T, 1, dtype=torch.uint8, device=dev)
            shard = (fv, vm, lm, mm)
            out = tuple(torch.empty((Q * M,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev) for t in shard)
            score, _, cells = A.prefilter_scores(fv, fs, w, b, lm, mm, T, L, C, TAU)
            earlier = torch.randn(Q, Vs, generator=g).to(dev) * score.std() + score.mean()       # an earlier shard's scores, alike
            empty = (torch.zeros(Q, M, device=dev), torch.zeros(Q, M, device=dev), torch.full((Q, M), -1, dtype=torch.int32, device=dev))
            primed = tuple(t.clone() for t in empty)
            A.prefilter_fold(*primed, earlier, cells, 0)
            state = tuple(t.clone() for t in empty)
            n_old = min(M, Vs)
            cp_first, cp = A.prefilter_fold(*[t.clone() for t in empty], score, cells, 0), A.prefilter_fold(*[t.clone() for t in primed], score, cells, Vs)
            changed = (cp >= 0).float().mean().item()

            def fold(start, seen):                                                   # (the state is restored by three small device copies, timed too)
                for dst, src in zip(state, start):
                    dst.copy_(src)
                return A.prefilter_fold(*state, score, cells, seen)

            sides = {"prefilter_scores": lambda: A.prefilter_scores(fv, fs, w, b, lm, mm, T, L, C, TAU),
                     "fold": lambda: fold(primed, Vs), "fold_first": lambda: fold(empty, 0),
                     "state_restore_only": lambda: [dst.copy_(src) for dst, src in zip(state, primed)],
                     "admit": lambda: A.survivors_admit(cp, shard, out), "admit_first": lambda: A.survivors_admit(cp_first, shard, out)}
            for run in range(args.runs):
                us = timed_blocks(sides, calls, warmup, min(args.block, calls))
                res = {s: summary(v) for s, v in us.items()}
                print(json.dumps({"bench": "launches", "shape": name, "run": run, "Q": Q, "Vs": Vs, "M": M, "n_old": n_old, "calls": calls,
                                  "slots_changed_share": round(changed, 4), "survivor_rows_mb": round(sum(t.numel() * t.element_size() for t in out) / 2 ** 20, 1),
                                  "gemm_mode": A.get_gemm_mode(), "us": res}), flush=True)
            del fv, mm, out, shard
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Q", type=int, default=16)
    ap.add_argument("--V", type=int, default=32)
    ap.add_argument("--shards", type=int, default=4)
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
    ap.add_argument("--skip-launches", action="store_true")
    ap.add_argument("--full-length", action="store_true", help="videos of equal length: equal cell_counts, so the pruned routes read nothing back")
    args = ap.parse_args()
    import models
    A = models.vml_amd
    assert torch.cuda.is_available(), "prefilter_shards_bench needs a HIP device"
    dev = torch.device("cuda:0")
    A._lib.load_torch()
    if not args.skip_launches:
        bench_launches(A, args, dev)
    if not args.skip_search:
        bench_search(A, models, args, dev)


if __name__ == "__main__":
    main()
