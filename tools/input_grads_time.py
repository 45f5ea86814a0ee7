#!/usr/bin/env python3
"""What SMIN.input_grads adds to a train step: forward and backward time of the one-node step with the inputs' gradients formed
(input_grads = True, video_features / query_features requiring grad) against the same step without them, alternated step by step.

    python tools/input_grads_time.py [--workload activitynet_t256] [--steps 30] [--warmup 5] [--out result.json]

Times are device events around the forward and around backward() on the current stream (the one-node backward joins its other
streams there before it returns); the medians of the alternated steps are printed as one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {   # T, L, C, D, dl, layers, Din, Nq, H, B
    "activitynet_t256": (256, 64, 4, 512, 128, 3, 500, 20, 256, 64),
    "tacos_d500": (128, 32, 4, 512, 128, 3, 500, 14, 256, 64),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="activitynet_t256", choices=sorted(WORKLOADS))
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import models
    from oracle import smin_oracle as O
    from tests import helpers as H
    from vml_amd import loss_fn
    assert torch.cuda.is_available(), "input_grads_time.py measures on a HIP device"
    T, L, C, D, dl, layers, Din, Nq, Hh, B = WORKLOADS[args.workload]
    dev = torch.device("cuda:0")
    sd = O.formula_state_dict(H.smin_shapes(T, L, C, D, dl, layers, Din, Nq, Hh), gain=1.2)
    m = models.SMIN(T, L, C, D, dl, layers, Din, Nq, Hh, dev)
    m.load_state_dict(sd)
    m = m.to(dev)
    b = {k: v.to(dev) for k, v in O.synthetic_batch(B, T, L, Nq, Din, seed=1).items()}
    times = {False: ([], []), True: ([], [])}

    def step(on):
        m.input_grads = on
        inp = [x.clone() for x in H.model_inputs(b)]
        if on:
            inp[0].requires_grad_(True)
            inp[2].requires_grad_(True)
        m.zero_grad(set_to_none=True)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        out = m(*inp)
        loss = loss_fn(out[0], b["ym"], b["sm"], b["moment_mask"], out[1], b["ys"], b["ss"], out[2], b["ye"], b["se"], out[3], b["ya"],
                       b["length_mask"])
        e[1].record()
        loss.backward()
        e[2].record()
        torch.cuda.synchronize()
        if on:
            assert inp[0].grad is not None and inp[2].grad is not None
        return e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])

    for i in range(args.warmup + args.steps):
        for on in ((False, True) if i % 2 == 0 else (True, False)):
            f, bw = step(on)
            if i >= args.warmup:
                times[on][0].append(f)
                times[on][1].append(bw)
    err = models.vml_amd._lib.load().smin_lstm_cluster_error()
    med = {on: (statistics.median(times[on][0]), statistics.median(times[on][1])) for on in times}
    spread = {on: (min(times[on][1]), max(times[on][1])) for on in times}
    res = dict(workload=args.workload, B=B, steps=args.steps, fwd_ms_off=round(med[False][0], 4), bwd_ms_off=round(med[False][1], 4),
               fwd_ms_on=round(med[True][0], 4), bwd_ms_on=round(med[True][1], 4), bwd_added_ms=round(med[True][1] - med[False][1], 4),
               bwd_range_off=[round(x, 4) for x in spread[False]], bwd_range_on=[round(x, 4) for x in spread[True]], cluster_error=err)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
