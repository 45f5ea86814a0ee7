#!/usr/bin/env python3
"""Q queries against V videos, from banks against expanded pairs, in one process:
  (a) banks:    SMIN.search over prebuilt banks (score_pairs per chunk, top_moments, one smin_corpus_topk); building the two banks is
                timed on its own, once per run;
  (b) expanded: the same pairs in the same chunks, each chunk's video and query features expanded to one row per pair and handed to
                SMIN.localize -- what a caller had before the banks (no merge across videos exists on that side, so (b) does less).
Shapes: tacos.yml and activitynet.yml, Q = 16 queries, V = 32 videos, chunks of 64 pairs, forward_only_scoring on both sides.  After a
warm-up of both, alternating blocks of the two; every timed call lies between two HIP events (host issue time is inside them).
    python tools/corpus_search_bench.py [--calls 200] [--warmup 10] [--block 20] [--runs 2] [--shapes tacos_yml,anet_yml] [--launches]
Prints one JSON line per shape and run: the median and the 10-90 % spread of each side in microseconds, the bytes of video features each
side needs on the device, and with --launches the kernels per chunk of each side as torch.profiler counts them (one extra call each)."""
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


def summary(v):
    q = statistics.quantiles(v, n=10)
    return {"median": round(statistics.median(v), 2), "p10": round(q[0], 2), "p90": round(q[-1], 2), "spread": round(q[-1] - q[0], 2)}


def kernels_of(fn):
    """device kernels of one call of fn, as torch.profiler lists them"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Q", type=int, default=16)
    ap.add_argument("--V", type=int, default=32)
    ap.add_argument("--max-batch", type=int, default=64)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--block", type=int, default=20)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--shapes", default="tacos_yml,anet_yml")
    ap.add_argument("--launches", action="store_true")
    args = ap.parse_args()
    import models
    from oracle import smin_oracle as O
    from tests import helpers as H
    A = models.vml_amd
    assert torch.cuda.is_available(), "corpus_search_bench needs a HIP device"
    dev = torch.device("cuda:0")
    A._lib.load_torch()
    Q, V, mb, k = args.Q, args.V, args.max_batch, args.k
    for name in args.shapes.split(","):
        T, L, C, D, dl, layers, Din, Nq, Hh = shape = SHAPES[name]
        m = models.SMIN(*shape, dev)
        m.load_state_dict(O.formula_state_dict(H.smin_shapes(*shape), gain=1.3))
        m = m.to(dev).eval()
        m.forward_only_scoring = True
        vb_ = {k_: v.to(dev) for k_, v in O.synthetic_batch(V, T, L, Nq, Din, seed=1, with_labels=False).items()}
        qb_ = {k_: v.to(dev) for k_, v in O.synthetic_batch(Q, T, L, Nq, Din, seed=2, with_labels=False).items()}
        vid = [vb_[key] for key in ("video_features", "video_mask", "length_mask", "moment_mask")]
        qry = [qb_["query_features"], qb_["query_mask"]]
        qi, vi = np.repeat(np.arange(Q), V), np.tile(np.arange(V), Q)
        P = qi.shape[0]
        chunks = [(torch.from_numpy(vi[c0:c0 + mb]).to(dev), torch.from_numpy(qi[c0:c0 + mb]).to(dev)) for c0 in range(0, P, mb)]
        cells = [int(vb_["moment_mask"][v_].sum()) for v_ in range(V)]
        known = [int(sum(cells[v_] for v_ in vi[c0:c0 + mb])) for c0 in range(0, P, mb)]

        def build():
            return m.encode_videos(*vid), m.encode_queries(*qry)

        banks = build()

        def side_a():
            return m.search(*banks, k=k, max_batch=mb)

        def side_b():
            out = []
            for (v_d, q_d), n in zip(chunks, known):
                m.known_cell_count = n                                           # as search: no chunk reads its cell count back
                out.append(m.localize(vid[0].index_select(0, v_d), vid[1].index_select(0, v_d), qry[0].index_select(0, q_d), qry[1].index_select(0, q_d),
                                      vid[2].index_select(0, v_d), vid[3].index_select(0, v_d), k=k))
            m.known_cell_count = None
            return out

        sides = {"banks": side_a, "expanded": side_b}
        for _ in range(args.warmup):
            for fn in sides.values():
                fn()
        torch.cuda.synchronize()
        # video features on the device: (a) the raw features while the bank is built, then f_v (V, T, D) for good and a chunk's f;
        # (b) the raw features for good and a chunk's expanded copy (and that chunk's f_v and f inside the scorer)
        pc = min(mb, P)
        feat = {"banks": {"build_raw": 4 * V * T * Din, "bank_fv": 4 * V * T * D, "per_chunk": 4 * pc * T * D},
                "expanded": {"raw": 4 * V * T * Din, "per_chunk": 4 * pc * T * Din + 2 * 4 * pc * T * D}}
        for run in range(args.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            build()
            e1.record()
            timed, done = [], 0
            while done < args.calls:
                n = min(args.block, args.calls - done)
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
            res = {s: summary(v) for s, v in us.items()}
            print(json.dumps({"shape": name, "run": run, "Q": Q, "V": V, "pairs": P, "max_batch": mb, "chunks": len(chunks), "k": k, "gemm_mode": A.get_gemm_mode(),
                              "calls": args.calls, "us": res, "build_banks_us": round(e0.elapsed_time(e1) * 1e3, 2),
                              "expanded_over_banks": round(res["expanded"]["median"] / res["banks"]["median"], 3),
                              "video_feature_bytes": feat}), flush=True)
        if args.launches:
            print(json.dumps({"shape": name, "kernels_per_chunk": {s: round(kernels_of(fn) / len(chunks), 1) for s, fn in sides.items()},
                              "chunks": len(chunks)}), flush=True)
        del m, banks, vid, qry, vb_, qb_
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
