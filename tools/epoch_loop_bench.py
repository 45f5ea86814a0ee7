#!/usr/bin/env python3
"""What the host reads of a reference-style epoch cost: the loop as it ran before the epoch meter against training.train_epoch /
eval_epoch, in one process, on the same fed batches and twin models.

    python tools/epoch_loop_bench.py [--workloads tacos,charadessta,activitynet_t256] [--batches 8] [--block 16] [--blocks 12]

Per workload (shapes of bench.WORKLOADS / BASELINE.md): ``--batches`` synthetic ragged host batches go through BatchFeeder once and
stay on the device (with their cell counts), so both loops consume identical tensors and no H2D copy is inside the timing.  Loops:
  A  the reference's loop (main.py:135-191) as it runs without the meter: no count handed to the forward (the forward reads it back),
     ``loss.item()`` and ``compute_ious`` on every batch;
  B  ``train_epoch`` / ``eval_epoch`` with an EpochMeter: the batch's host-computed count, one ``result()`` per block.
After one warm-up pass of both loops over every batch (every shape), blocks of ``--block`` steps alternate A, B, A, B ...; a host
clock is taken around each block, which ends in a device synchronise.  Reported: the median over the blocks of the time per step
and its 10-90 % spread, in milliseconds, for train and eval.  One JSON line per workload, then a table.  Profiler off."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_batches(B, T, Nq, Din, count, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(count):
        dur = torch.rand(B, generator=g) * 100 + 5
        ts = torch.rand(B, generator=g) * dur * 0.5
        te = ts + 1.0 + torch.rand(B, generator=g) * (dur - ts - 1.0).clamp(min=0)
        nf = torch.randint(max(T // 2, 1), T + 1, (B,), generator=g)
        nf[0] = T
        vf = torch.randn(B, T, Din, generator=g)
        vf[torch.arange(T).unsqueeze(0) >= nf.unsqueeze(1)] = 0
        out.append(dict(video_features=vf, query_features=torch.randn(B, Nq, 300, generator=g), nfeats=nf,
                        qlen=torch.randint(2, Nq + 1, (B,), generator=g), times=torch.stack([ts, te], 1), duration=dur))
    return out


def summary(per_step_ms):
    q = statistics.quantiles(per_step_ms, n=10)
    return {"median": round(statistics.median(per_step_ms), 4), "p10": round(q[0], 4), "p90": round(q[-1], 4), "spread": round(q[-1] - q[0], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="tacos,charadessta,activitynet_t256")
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--block", type=int, default=16, help="steps per timed block")
    ap.add_argument("--blocks", type=int, default=12, help="timed blocks per loop")
    args = ap.parse_args()
    if torch.cuda.device_count() < 1:
        print("epoch_loop_bench: no HIP device found", file=sys.stderr)
        return 1
    import bench
    import models
    V = models.vml_amd
    from vml_amd.training import MODEL_INPUTS
    dev = torch.device("cuda:0")
    V._lib.load()
    rows = []
    for w in args.workloads.split(","):
        T, L, C, D, dl, layers, Din, Nq, Hh, B = bench.WORKLOADS[w]
        fed = []
        for f in V.BatchFeeder(T, L, Nq, dev).feed(host_batches(B, T, Nq, Din, args.batches, seed=77)):
            c = V.FedBatch((k, v.clone()) for k, v in f.items())
            c.cell_count = f.cell_count
            fed.append(c)
        plain = [dict(f) for f in fed]                                          # loop A sees no count
        torch.manual_seed(43)
        ma = models.SMIN(T, L, C, D, dl, layers, Din, Nq, Hh, dev).to(dev)
        mb = models.SMIN(T, L, C, D, dl, layers, Din, Nq, Hh, dev).to(dev)
        mb.load_state_dict(ma.state_dict())
        oa, ob = (torch.optim.Adam(m.parameters(), lr=5e-4, fused=True) for m in (ma, mb))
        meter = V.EpochMeter(device=dev)

        def loss_of(out, b):
            pm, ps, pe, pa = out
            return V.loss_fn(pm, b["ym"], b["sm"], b["moment_mask"], ps, b["ys"], b["ss"], pe, b["ye"], b["se"], pa, b["ya"], b["length_mask"])

        def train_a(bs):
            ma.train()
            total, metrics, num = 0.0, {}, 0
            for b in bs:
                n = b["video_features"].shape[0]
                oa.zero_grad()
                out = ma(*[b[k] for k in MODEL_INPUTS])
                loss = loss_of(out, b)
                total += loss.item() * n
                iou = V.compute_ious(out[0], out[1], out[2], b["moment_mask"], b["sm"])
                metrics = {k: metrics.get(k, 0.0) + v for k, v in iou.items()}
                loss.backward()
                oa.step()
                num += n
            return total / num, {k: v / num for k, v in metrics.items()}

        def eval_a(bs):
            ma.eval()
            total, metrics, num = 0.0, {}, 0
            with torch.no_grad():
                for b in bs:
                    n = b["video_features"].shape[0]
                    out = ma(*[b[k] for k in MODEL_INPUTS])
                    total += loss_of(out, b).item() * n
                    iou = V.compute_ious(out[0], out[1], out[2], b["moment_mask"], b["sm"])
                    metrics = {k: metrics.get(k, 0.0) + v for k, v in iou.items()}
                    num += n
            return total / num, {k: v / num for k, v in metrics.items()}

        def train_b(bs):
            meter.reset()
            return V.train_epoch(mb, ob, bs, meter)

        def eval_b(bs):
            meter.reset()
            return V.eval_epoch(mb, bs, meter)

        res = {"workload": w, "B": B, "T": T, "L": L, "batches": args.batches, "block": args.block, "blocks": args.blocks,
               "cells": [f.cell_count for f in fed], "gemm_mode": V.get_gemm_mode()}
        for phase, fa, fb in (("train", train_a, train_b), ("eval", eval_a, eval_b)):
            fa(plain), fb(fed)                                                  # warm-up: every shape through both loops
            torch.cuda.synchronize()
            ms = {"A": [], "B": []}
            for blk in range(args.blocks):
                idx = [(blk * args.block + s) % len(fed) for s in range(args.block)]
                for name, fn, src in (("A", fa, plain), ("B", fb, fed)):
                    bs = [src[i] for i in idx]
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn(bs)
                    torch.cuda.synchronize()
                    ms[name].append((time.perf_counter() - t0) * 1e3 / args.block)
            a, b_ = summary(ms["A"]), summary(ms["B"])
            res[phase] = {"A_ms_per_step": a, "B_ms_per_step": b_, "A_minus_B_ms": round(a["median"] - b_["median"], 4)}
            rows.append((w, phase, a, b_))
        print(json.dumps(res), flush=True)
        del ma, mb, oa, ob, fed, plain
        torch.cuda.empty_cache()
    print("| workload | loop | A: per-batch reads, ms/step (10-90 % spread) | B: epoch meter, ms/step (10-90 % spread) | A - B |")
    print("|---|---|---|---|---|")
    for w, phase, a, b_ in rows:
        print(f"| {w} | {phase} | {a['median']:.3f} ({a['spread']:.3f}) | {b_['median']:.3f} ({b_['spread']:.3f}) | {a['median'] - b_['median']:+.3f} |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
