#!/usr/bin/env python3
"""Fine-tuning step of a GloVe-sized word table, dense against row-sparse, in one process:
  (a) dense:  embed_tokens(differentiable=True) backward -- a zero-filled (V, E) gradient -- plus FusedAdam([table]).step();
  (b) rows:   embed_tokens(differentiable=True, sparse_grad=True) backward -- the batch's distinct rows -- plus RowSparseAdam.step().
Shape: V = 400002, E = 300, B = 64, Nq = 20, ids drawn uniformly.  After a warm-up of both, alternating blocks of the two; every timed
region (backward + step; the forward lookup that builds the graph runs before the first event) lies between two HIP events.
    python tools/row_adam_bench.py [--calls 200] [--warmup 20] [--block 20] [--runs 2]
Prints one JSON line per run: the median and the 10-90 % spread of each side in microseconds, the bytes each side has to move as
counted from the shapes, and each side's peak of torch.cuda.max_memory_allocated above the level before its tensors were made
(table + two moments on both sides; (a) adds the dense gradient)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(v):
    q = statistics.quantiles(v, n=10)
    return {"median": round(statistics.median(v), 2), "p10": round(q[0], 2), "p90": round(q[-1], 2), "spread": round(q[-1] - q[0], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--V", type=int, default=400002)
    ap.add_argument("--E", type=int, default=300)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--Nq", type=int, default=20)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--block", type=int, default=20)
    ap.add_argument("--runs", type=int, default=2)
    args = ap.parse_args()
    if args.calls < 100:
        ap.error("--calls must be at least 100")
    import models
    A = models.vml_amd
    assert torch.cuda.is_available(), "row_adam_bench needs a HIP device"
    dev = torch.device("cuda:0")
    A._lib.load_torch()
    V, E, B, Nq = args.V, args.E, args.B, args.Nq
    g = torch.Generator().manual_seed(7)
    tok = torch.randint(0, V, (B, Nq), generator=g).to(dev)
    dqf = (torch.randn(B, Nq, E, generator=g) * 1e-2).to(dev)
    distinct = int(torch.unique(tok).numel())

    def side(sparse):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        table = torch.randn(V, E, device=dev).requires_grad_(True)
        opt = A.RowSparseAdam(table, lr=1e-3) if sparse else A.FusedAdam([table], lr=1e-3)

        def prepare():
            opt.zero_grad(set_to_none=True)
            return A.embed_tokens(tok, table, differentiable=True, sparse_grad=sparse)[0]

        def timed(qf):
            qf.backward(dqf)
            opt.step()

        for _ in range(args.warmup):
            timed(prepare())
        torch.cuda.synchronize()
        return prepare, timed, torch.cuda.max_memory_allocated() - base

    sides, peak = {}, {}
    for name, sparse in (("dense", False), ("rows", True)):
        *sides[name], peak[name] = side(sparse)
    table_bytes = 4 * V * E
    # dense: the gradient's zero fill, then p, g, m, v read and p, m, v written over the table; rows: the batch's gradient rows read and
    # the distinct rows written, then the same seven passes over the distinct rows only
    moved = {"dense": table_bytes * (1 + 7), "rows": 4 * E * (B * Nq + distinct) + 4 * E * distinct * 7}
    for run in range(args.runs):
        pairs, done = [], 0
        while done < args.calls:
            n = min(args.block, args.calls - done)
            for name, (prepare, timed) in sides.items():
                for _ in range(n):
                    qf = prepare()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    timed(qf)
                    e1.record()
                    pairs.append((name, e0, e1))
            done += n
        torch.cuda.synchronize()
        us = {k: [] for k in sides}
        for name, e0, e1 in pairs:
            us[name].append(e0.elapsed_time(e1) * 1e3)
        res = {k: summary(v) for k, v in us.items()}
        print(json.dumps({"run": run, "V": V, "E": E, "B": B, "Nq": Nq, "distinct_ids": distinct, "calls": args.calls, "us": res,
                          "dense_over_rows": round(res["dense"]["median"] / res["rows"]["median"], 1),
                          "bytes_moved": moved, "dense_GBps": round(moved["dense"] / res["dense"]["median"] * 1e-3, 1),
                          "peak_bytes_allocated": peak}), flush=True)


if __name__ == "__main__":
    main()
