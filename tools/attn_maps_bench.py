#!/usr/bin/env python3
"""Cost of SMIN.keep_attention at the bench workload (activitynet_t256: B 64, T 256, L 64, Nq 20, 3 layers): the train step
(zero_grad + forward + loss + backward + Adam) and the forward alone under no_grad, with the maps off and on, in interleaved
rounds after a warm-up of both.
    python tools/attn_maps_bench.py [--rounds 6] [--steps 5] [--warmup 3] [--workload activitynet_t256]
Prints one JSON line: milliseconds per step / forward for off and on (median over rounds) and the on - off difference."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="activitynet_t256")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import bench
    import models
    from vml_amd import loss_fn
    dev = torch.device("cuda:0")
    models.vml_amd._lib.load()
    T, L, C, D, dl, layers, Din, Nq, Hh, B = bench.WORKLOADS[args.workload]
    torch.manual_seed(43)
    model = models.SMIN(T, L, C, D, dl, layers, Din, Nq, Hh, dev).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=5e-4, fused=True)
    b = bench.make_batch(B, T, L, Nq, Din, seed=1000, device=dev)
    inputs = [b[k] for k in ("video_features", "video_mask", "query_features", "query_mask", "length_mask", "moment_mask")]

    def train_step():
        opt.zero_grad(set_to_none=True)
        pm, ps, pe, pa = model(*inputs)
        loss = loss_fn(pm, b["ym"], b["sm"], b["moment_mask"], ps, b["ys"], b["ss"], pe, b["ye"], b["se"], pa, b["ya"], b["length_mask"])
        loss.backward()
        opt.step()

    def forward():
        with torch.no_grad():
            model(*inputs)

    def timed(fn, keep):
        model.keep_attention = keep
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    for keep in (False, True):
        model.keep_attention = keep
        for _ in range(args.warmup):
            train_step()
            forward()
    res = {k: [] for k in ("step_off", "step_on", "fwd_off", "fwd_on")}
    for r in range(args.rounds):                                  # interleaved, the order alternating per round
        order = (False, True) if r % 2 == 0 else (True, False)
        for keep in order:
            res["step_on" if keep else "step_off"].append(timed(train_step, keep))
        for keep in order:
            res["fwd_on" if keep else "fwd_off"].append(timed(forward, keep))
    med = {k: statistics.median(v) for k, v in res.items()}
    maps_mb = layers * (B * L * L * C * Nq + B * L * Nq) * 4 / 1e6
    print(json.dumps({"workload": args.workload, "ms": {k: round(v, 3) for k, v in med.items()},
                      "all": {k: [round(x, 3) for x in v] for k, v in res.items()},
                      "step_on_minus_off_pct": round(100 * (med["step_on"] / med["step_off"] - 1), 3),
                      "fwd_on_minus_off_pct": round(100 * (med["fwd_on"] / med["fwd_off"] - 1), 3),
                      "maps_MB_per_forward": round(maps_mb, 1)}))


if __name__ == "__main__":
    main()
