#!/usr/bin/env python3
"""Step of a GloVe-sized word table from the gradients of R data-parallel ranks, in one process on one GPU: the R
gradients are stand-ins for gathered ones -- the gather itself is not part of either side.
  (a) rows:   merge_row_grads(R row gradients, scale=1/R as a device value made once) plus RowSparseAdam.step();
  (b) dense:  R dense (V, E) gradients summed ((g0 + g1) + ..., R - 1 passes of three table-sized streams, as a reduction over ranks
              has to touch every row) plus FusedAdam([table]).step().
Shape: V = 400002, E = 300, n = 1280 slots a rank, R in {2, 8}, ids drawn uniformly.  After a warm-up of both, alternating blocks of the
two; every timed region lies between two HIP events.
    python tools/row_merge_bench.py [--R 2 8] [--calls 200] [--warmup 20] [--block 20] [--runs 2]
Prints one JSON line per R and run: the median and the 10-90 % spread of each side in microseconds, the slots listed and the size of the
union, and the bytes each side has to move as counted from the shapes."""
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
    ap.add_argument("--R", type=int, nargs="+", default=[2, 8])
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--block", type=int, default=20)
    ap.add_argument("--runs", type=int, default=2)
    args = ap.parse_args()
    if args.calls < 100:
        ap.error("--calls must be at least 100")
    import models
    A = models.vml_amd
    assert torch.cuda.is_available(), "row_merge_bench needs a HIP device"
    dev = torch.device("cuda:0")
    A._lib.load_torch()
    V, E, B, Nq = args.V, args.E, args.B, args.Nq
    table_bytes = 4 * V * E
    for R in args.R:
        g = torch.Generator().manual_seed(7 + R)
        lists, dense = [], []
        for _ in range(R):                                               # one backward per stand-in rank, on tables of their own
            tok = torch.randint(0, V, (B, Nq), generator=g).to(dev)
            dqf = (torch.randn(B, Nq, E, generator=g) * 1e-2).to(dev)
            t = torch.zeros(V, E, device=dev).requires_grad_(True)
            A.embed_tokens(tok, t, differentiable=True, sparse_grad=True)[0].backward(dqf)
            lists.append(t.row_grad)
            dense.append(t.row_grad.to_dense())
            del t
        listed = sum(int(rg.count.item()) for rg in lists)
        union = int(A.merge_row_grads(lists).count.item())

        ta = torch.randn(V, E, device=dev).requires_grad_(True)
        oa = A.RowSparseAdam(ta, lr=1e-3)
        tb = torch.randn(V, E, device=dev).requires_grad_(True)
        ob = A.FusedAdam([tb], lr=1e-3)

        inv = torch.full((1,), 1.0 / R, dtype=torch.float64, device=dev)

        def rows_side():
            ta.row_grad = A.merge_row_grads(lists, scale=inv)
            oa.step()

        def dense_side():
            acc = dense[0] + dense[1] if R > 1 else dense[0]
            for d in dense[2:]:
                acc = acc + d
            tb.grad = acc
            ob.step()

        sides = {"rows": rows_side, "dense": dense_side}
        for fn in sides.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        # rows: the listed rows read and the union's rows written by the merge, then seven passes over the union's rows;
        # dense: R - 1 additions of two table-sized operands into a third, then p, g, m, v read and p, m, v written over the table
        moved = {"rows": 4 * E * (listed + union) + 4 * E * union * 7, "dense": table_bytes * (3 * max(R - 1, 0) + 7)}
        for run in range(args.runs):
            pairs, done = [], 0
            while done < args.calls:
                k = min(args.block, args.calls - done)
                for name, fn in sides.items():
                    for _ in range(k):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        fn()
                        e1.record()
                        pairs.append((name, e0, e1))
                done += k
            torch.cuda.synchronize()
            us = {k: [] for k in sides}
            for name, e0, e1 in pairs:
                us[name].append(e0.elapsed_time(e1) * 1e3)
            res = {k: summary(v) for k, v in us.items()}
            print(json.dumps({"R": R, "run": run, "V": V, "E": E, "slots_per_list": B * Nq, "listed": listed, "union": union,
                              "calls": args.calls, "us": res, "dense_over_rows": round(res["dense"]["median"] / res["rows"]["median"], 1),
                              "bytes_moved": moved}), flush=True)
        del ta, tb, oa, ob, lists, dense
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
